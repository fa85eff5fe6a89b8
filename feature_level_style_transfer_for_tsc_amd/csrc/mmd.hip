// Transfer monitor (gfx950): the multi-kernel maximum mean discrepancy between feature sets, on the device and under graph replay —
// the number behind the t-SNE dumps of the reference's joint epoch (train_and_test.py:564-621, :792-797).  monitor.py holds the
// definition (mmd2_reference, fp64); three launches compute it:
//
//   fst_mmd_centre   c[k] = mean over the rows of ONE set of column k.  A workgroup owns 64 columns; its four waves sum a quarter
//                    of the rows each, in row order, and wave 0 adds the four partial sums as (0 + 1) + (2 + 3): deterministic.
//   fst_mmd_gram     G = Zc·Zcᵀ (fp32, [R][R], R <= 1024) of the pooled rows Z = [X_0; X_1; ...] of up to four row sets that
//                    need not be adjacent in memory, Zc = Z − c subtracted in fp32 while a row is staged, before the bf16 split.
//                    Split-bf16 products on gemm.hip's tile (GemmBf3 of gemm_bf3.h: staging, fragment reads, the three MFMAs):
//                    a 256-thread workgroup owns one 128 × 128 tile of the UPPER triangle of tiles and one slab of K; a diagonal
//                    tile stages its rows once.  A stage is 32 columns; columns past D enter as zeros and are never read.  Slab z
//                    covers columns [z·8192, (z+1)·8192): the boundaries depend on D alone, so the bits of G_ij depend on rows i
//                    and j and on nothing else — not on the other sets of the launch, nor on where the rows sit in the pool.  The
//                    row of the pool with the smaller index is always the A operand (lo·hi + hi·lo + hi·hi is not symmetric in
//                    its operands).  A second kernel adds the slabs in slab order (gemm.hip's four chains) and writes G_ij and
//                    G_ji from the same sum: G is exactly symmetric.  No atomics, no zero fill: same inputs, same bits.
//   fst_mmd_fold     per pair (a, b) of sets one workgroup of 1024 threads, all in fp64 from the fp32 Gram: d²_ij = G_ii + G_jj −
//                    2 G_ij clamped at 0 (a NaN stays a NaN), the mean-distance bandwidth (or a positive device word in its place),
//                    the Gaussian bank and the unbiased estimator; five outputs per pair, added into running sums under a device
//                    word.  Thread t takes the elements t, t + 1024, ... of the pair's own N × N index space (i < j), and the
//                    threads' sums meet in a fixed tree: the result depends on the pair's rows only.
#include <math.h>

#include "gemm_bf3.h"

#define MMD_MAX_SETS FST_MMD_MAX_SETS
#define MMD_MAX_ROWS FST_MMD_MAX_ROWS
#define MMD_MAX_PAIRS FST_MMD_MAX_PAIRS
#define MMD_MAX_KERNELS FST_MMD_MAX_KERNELS
#define MMD_BT 128                  // tile edge
#define MMD_BK 32                   // columns per stage
#define MMD_SLAB_K 8192             // columns per slab
#define MMD_TILE (MMD_BT * MMD_BT)
#define MMD_FOLD_T 1024

struct MmdSets {
  const float* x[MMD_MAX_SETS];
  long long ld[MMD_MAX_SETS];
  int first[MMD_MAX_SETS + 1];      // first[s]: the pool row of set s's row 0; first[n]: R
  int n;
};

struct MmdGramParams {
  MmdSets sets;
  const float* centre;              // [D] or null
  float* slab;                      // [splits][tiles][128][128]
  float* G;                         // [R][R]
  int R, D, splits, tiles, row_blocks, vec;
};

// tile t of the upper triangle, row by row: (0,0) (0,1) ... (0,nb-1) (1,1) ...
__device__ __forceinline__ void mmd_tile_of(int t, int nb, int& ti, int& tj) {
  ti = 0;
  while (t >= nb - ti) { t -= nb - ti; ++ti; }
  tj = ti + t;
}

// pool row r: where it starts in memory (null past the last row)
__device__ __forceinline__ const float* mmd_row(const MmdSets& s, int r) {
  if (r >= s.first[s.n]) return nullptr;
  const float* p = s.x[0];
  long long ld = s.ld[0];
  int f = 0;
#pragma unroll
  for (int q = 1; q < MMD_MAX_SETS; ++q)
    if (q < s.n && r >= s.first[q]) { p = s.x[q]; ld = s.ld[q]; f = s.first[q]; }
  return p + (long long)(r - f) * ld;
}

// columns kk .. kk + 3 of four rows (GemmBf3's [rows][K] thread map), minus the centre; a column at or past k_end and a row past
// the pool are zeros and are not read
__device__ __forceinline__ void mmd_fetch(float (&v)[MMD_BT / 8], const float* const (&row)[MMD_BT / 32], const float* centre, int vec,
                                          int kk, int k_end) {
  float c[4] = {0.f, 0.f, 0.f, 0.f};
  if (centre) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (kk + e < k_end) c[e] = centre[kk + e];
  }
#pragma unroll
  for (int j = 0; j < MMD_BT / 32; ++j) {
    const float* q = row[j];
    float w[4] = {0.f, 0.f, 0.f, 0.f};
    if (q) {
      if (vec && kk + 4 <= k_end) {
        const float4 u = *reinterpret_cast<const float4*>(q + kk);
        w[0] = u.x - c[0]; w[1] = u.y - c[1]; w[2] = u.z - c[2]; w[3] = u.w - c[3];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (kk + e < k_end) w[e] = q[kk + e] - c[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * j + e] = w[e];
  }
}

__global__ __launch_bounds__(256, 2) void mmd_gram_kernel(MmdGramParams p) {
  __shared__ __attribute__((aligned(16))) char lds[2 * GemmBf3::IMAGES * MMD_BT * GemmBf3::PITCH];
  constexpr int PITCH = GemmBf3::PITCH;
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1;
  int ti, tj;
  mmd_tile_of(blockIdx.x, p.row_blocks, ti, tj);
  const bool diag = ti == tj;
  char* const a_img = lds;
  char* const b_img = diag ? lds : lds + GemmBf3::IMAGES * MMD_BT * PITCH;
  const int k_begin = blockIdx.y * MMD_SLAB_K;
  const int k_end = min(p.D, k_begin + MMD_SLAB_K);
  const int n_st = (k_end - k_begin + MMD_BK - 1) / MMD_BK;

  const float* ra[MMD_BT / 32];
  const float* rb[MMD_BT / 32];
#pragma unroll
  for (int j = 0; j < MMD_BT / 32; ++j) {
    ra[j] = mmd_row(p.sets, ti * MMD_BT + (tid >> 3) + 32 * j);
    rb[j] = mmd_row(p.sets, tj * MMD_BT + (tid >> 3) + 32 * j);
  }
  const int kt = 4 * (tid & 7);

  f32x16 acc[2][2];
  zero_acc(acc);
  float va[MMD_BT / 8], vb[MMD_BT / 8];
  mmd_fetch(va, ra, p.centre, p.vec, k_begin + kt, k_end);
  if (!diag) mmd_fetch(vb, rb, p.centre, p.vec, k_begin + kt, k_end);
  const int a_off = (wm * 64 + l31) * PITCH + GemmBf3::HALF * half;
  const int b_off = (wn * 64 + l31) * PITCH + GemmBf3::HALF * half;
  for (int s = 0; s < n_st; ++s) {
    __syncthreads();                                       // every wave is past its fragment reads of the previous stage
    GemmBf3::stage<MMD_BT>(va, a_img, 0, tid);
    if (!diag) GemmBf3::stage<MMD_BT>(vb, b_img, 0, tid);
    __syncthreads();
    if (s + 1 < n_st) {                                    // the next stage's rows travel under this stage's MFMAs
      const int kk = k_begin + (s + 1) * MMD_BK + kt;
      mmd_fetch(va, ra, p.centre, p.vec, kk, k_end);
      if (!diag) mmd_fetch(vb, rb, p.centre, p.vec, kk, k_end);
    }
    GemmBf3::multiply<2, 2>(acc, a_img + a_off, b_img + b_off);
  }

  // accumulator layout: lane = column n, register r = row (r&3) + 8(r>>2) + 4·half.  The whole tile goes to its slab, rows and
  // columns past the pool included (zeros): the workspace holds whole tiles
  float* const out = p.slab + ((long long)blockIdx.y * p.tiles + blockIdx.x) * MMD_TILE;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = wn * 64 + 32 * j + l31;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int mr = wm * 64 + 32 * i + 4 * half;
#pragma unroll
      for (int r = 0; r < 16; ++r) out[(mr + (r & 3) + 8 * (r >> 2)) * MMD_BT + n] = acc[i][j][r];
    }
  }
}

// G_ij = G_ji = Σ_z slab[z][tile][i][j] for i <= j: slab z joins chain z mod 4 in ascending z (a tail of fewer than four joins
// chain 0), then (s0 + s1) + (s2 + s3) — gemm_reduce_kernel's order
__global__ __launch_bounds__(256) void mmd_gram_reduce_kernel(MmdGramParams p) {
  int ti, tj;
  mmd_tile_of(blockIdx.y, p.row_blocks, ti, tj);
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int m = e / MMD_BT, n = e % MMD_BT;
  const int gi = ti * MMD_BT + m, gj = tj * MMD_BT + n;
  if (gi >= p.R || gj >= p.R || gi > gj) return;
  const long long st = (long long)p.tiles * MMD_TILE;
  const float* q = p.slab + (long long)blockIdx.y * MMD_TILE + e;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int z = 0;
  for (; z + 4 <= p.splits; z += 4) {
    s0 += q[z * st]; s1 += q[(z + 1) * st]; s2 += q[(z + 2) * st]; s3 += q[(z + 3) * st];
  }
  for (; z < p.splits; ++z) s0 += q[z * st];
  const float v = (s0 + s1) + (s2 + s3);
  p.G[(long long)gi * p.R + gj] = v;
  if (gi != gj) p.G[(long long)gj * p.R + gi] = v;
}

static int mmd_row_blocks(int R) { return (R + MMD_BT - 1) / MMD_BT; }
static int mmd_tiles(int R) { const int nb = mmd_row_blocks(R); return nb * (nb + 1) / 2; }

extern "C" int fst_mmd_gram_splits(int R, int D) {
  if (R < 1 || R > MMD_MAX_ROWS || D < 1 || D > (1 << 28)) return -1;
  return (int)(((long long)D + MMD_SLAB_K - 1) / MMD_SLAB_K);
}

extern "C" int64_t fst_mmd_gram_workspace_floats(int R, int D) {
  const int splits = fst_mmd_gram_splits(R, D);
  return splits < 0 ? -1 : (int64_t)splits * mmd_tiles(R) * MMD_TILE;
}

// sets (host arrays of n_sets entries) -> MmdSets; the checks every entry point of the file shares
static int mmd_bind_sets(const char* who, MmdSets& s, const int32_t* rows_host, int n_sets) {
  FST_REQUIRE(rows_host && n_sets >= 1 && n_sets <= MMD_MAX_SETS, "%s: %d sets (1..%d)", who, n_sets, MMD_MAX_SETS);
  long long R = 0;
  for (int i = 0; i < n_sets; ++i) {
    FST_REQUIRE(rows_host[i] >= 1 && rows_host[i] <= MMD_MAX_ROWS, "%s: set %d has %d rows (1..%d)", who, i, rows_host[i], MMD_MAX_ROWS);
    s.first[i] = (int)R;
    R += rows_host[i];
  }
  FST_REQUIRE(R <= MMD_MAX_ROWS, "%s: %lld rows in all (at most %d)", who, R, MMD_MAX_ROWS);
  for (int i = n_sets; i <= MMD_MAX_SETS; ++i) s.first[i] = (int)R;
  s.n = n_sets;
  return 0;
}

static bool mmd_disjoint(const void* p, uint64_t p_bytes, const void* q, uint64_t q_bytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a + p_bytes <= b || b + q_bytes <= a;
}

extern "C" int fst_mmd_gram(const float* const* x_host, const int32_t* rows_host, const int64_t* ld_host, int n_sets, int D,
                            const float* centre, float* G, float* workspace, int64_t workspace_floats, void* stream) {
  MmdGramParams p = {};
  if (mmd_bind_sets("fst_mmd_gram", p.sets, rows_host, n_sets)) return -1;
  FST_REQUIRE(x_host && ld_host && G && workspace, "fst_mmd_gram: null pointer");
  FST_REQUIRE(D >= 1 && D <= (1 << 28), "fst_mmd_gram: D = %d (1..2^28)", D);
  const int R = p.sets.first[n_sets];
  const int64_t need = fst_mmd_gram_workspace_floats(R, D);
  FST_REQUIRE(workspace_floats >= need, "fst_mmd_gram: workspace of %lld floats is too small (fst_mmd_gram_workspace_floats(%d, %d) = %lld)",
              (long long)workspace_floats, R, D, (long long)need);
  FST_REQUIRE(fst_aligned16(G) && fst_aligned16(workspace) && ((uintptr_t)centre & 3) == 0,
              "fst_mmd_gram: G and the workspace must be 16-byte aligned, the centre 4-byte");
  const uint64_t g_bytes = (uint64_t)R * R * 4, ws_bytes = (uint64_t)need * 4;
  FST_REQUIRE(mmd_disjoint(G, g_bytes, workspace, ws_bytes), "fst_mmd_gram: G overlaps the workspace");
  FST_REQUIRE(!centre || (mmd_disjoint(G, g_bytes, centre, (uint64_t)D * 4) && mmd_disjoint(workspace, ws_bytes, centre, (uint64_t)D * 4)),
              "fst_mmd_gram: the centre overlaps an output");
  int vec = 1;
  for (int i = 0; i < n_sets; ++i) {
    FST_REQUIRE(x_host[i] && fst_aligned16(x_host[i]), "fst_mmd_gram: set %d: null pointer, or one off a 16-byte boundary", i);
    FST_REQUIRE(ld_host[i] >= D && ld_host[i] < (1LL << 40), "fst_mmd_gram: set %d: row stride %lld is smaller than D = %d", i,
                (long long)ld_host[i], D);
    const uint64_t bytes = ((uint64_t)(rows_host[i] - 1) * ld_host[i] + D) * 4;
    FST_REQUIRE(mmd_disjoint(G, g_bytes, x_host[i], bytes) && mmd_disjoint(workspace, ws_bytes, x_host[i], bytes),
                "fst_mmd_gram: set %d overlaps an output", i);
    p.sets.x[i] = x_host[i];
    p.sets.ld[i] = ld_host[i];
    vec &= ld_host[i] % 4 == 0;
  }
  p.centre = centre; p.slab = workspace; p.G = G; p.R = R; p.D = D; p.vec = vec;
  p.splits = fst_mmd_gram_splits(R, D);
  p.tiles = mmd_tiles(R);
  p.row_blocks = mmd_row_blocks(R);
  hipLaunchKernelGGL(mmd_gram_kernel, dim3((unsigned)p.tiles, (unsigned)p.splits), dim3(256), 0, (hipStream_t)stream, p);
  FST_LAUNCH_CHECK();
  hipLaunchKernelGGL(mmd_gram_reduce_kernel, dim3(MMD_TILE / 256, (unsigned)p.tiles), dim3(256), 0, (hipStream_t)stream, p);
  FST_LAUNCH_CHECK();
  return 0;
}

// ---- the column mean of one set
__global__ __launch_bounds__(256) void mmd_centre_kernel(const float* __restrict__ x, long long ld, int n, int D, float* __restrict__ c) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + lane;
  const int r0 = (int)((long long)w * n / 4), r1 = (int)((long long)(w + 1) * n / 4);
  float s = 0.f;
  if (k < D) {
    const float* q = x + (long long)r0 * ld + k;
    for (int r = r0; r < r1; ++r, q += ld) s += *q;
  }
  part[w][lane] = s;
  __syncthreads();
  if (w == 0 && k < D) c[k] = ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) / (float)n;
}

extern "C" int fst_mmd_centre(const float* x, int64_t ld, int n, int D, float* centre, void* stream) {
  FST_REQUIRE(x && centre && n >= 1 && n <= MMD_MAX_ROWS && D >= 1 && D <= (1 << 28) && ld >= D && ld < (1LL << 40),
              "fst_mmd_centre: bad arguments (n=%d (1..%d), D=%d, ld=%lld >= D)", n, MMD_MAX_ROWS, D, (long long)ld);
  FST_REQUIRE((((uintptr_t)x | (uintptr_t)centre) & 3) == 0, "fst_mmd_centre: pointers must be 4-byte aligned");
  FST_REQUIRE(mmd_disjoint(centre, (uint64_t)D * 4, x, ((uint64_t)(n - 1) * ld + D) * 4), "fst_mmd_centre: the centre overlaps the set");
  hipLaunchKernelGGL(mmd_centre_kernel, dim3((unsigned)((D + 63) / 64)), dim3(256), 0, (hipStream_t)stream, x, (long long)ld, n, D, centre);
  FST_LAUNCH_CHECK();
  return 0;
}

// ---- the fold: Gram -> distances -> bandwidth -> kernel bank -> estimator, per pair of sets
struct MmdFoldParams {
  const float* G;
  int R;
  int first[MMD_MAX_SETS + 1];
  int pair[MMD_MAX_PAIRS][2];
  int kernels;
  double scale[MMD_MAX_KERNELS];    // mul^(q − kernels/2)
  const double* bandwidth_override; // one word or null: a positive value replaces the mean-distance bandwidth
  const int* live;                  // one word or null: 0 = report only, the running sums stay as they are
  double* out;                      // [pairs][5]  mmd2, bw, mean d² within a, within b, between
  double* sum;                      // [pairs][5]
  int* count;                       // [pairs]
  int* nonfinite;                   // one word: folds whose mmd2 was not finite (they are left out of the sums)
};

// the 1024 threads' triples, added in a fixed tree; every thread returns with the totals
__device__ __forceinline__ void mmd_block_sum3(double (&v)[3], double (*red)[MMD_FOLD_T]) {
  const int t = threadIdx.x;
  __syncthreads();                                         // the previous use of red is over
#pragma unroll
  for (int c = 0; c < 3; ++c) red[c][t] = v[c];
  __syncthreads();
  for (int s = MMD_FOLD_T / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int c = 0; c < 3; ++c) red[c][t] += red[c][t + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = red[c][0];
}

__global__ __launch_bounds__(MMD_FOLD_T) void mmd_fold_kernel(MmdFoldParams p) {
  __shared__ double diag[MMD_MAX_ROWS];
  __shared__ double red[3][MMD_FOLD_T];
  __shared__ double ninv[MMD_MAX_KERNELS];
  const int t = threadIdx.x, pi = blockIdx.x;
  int fa = 0, fb = 0, la = 0, lb = 0;                     // first pool row and one past the last, of both sets
#pragma unroll
  for (int s = 0; s < MMD_MAX_SETS; ++s) {
    if (s == p.pair[pi][0]) { fa = p.first[s]; la = p.first[s + 1]; }
    if (s == p.pair[pi][1]) { fb = p.first[s]; lb = p.first[s + 1]; }
  }
  const int n = la - fa, m = lb - fb, N = n + m;
  const float* __restrict__ G = p.G;
  const long long R = p.R;
  for (int i = t; i < N; i += MMD_FOLD_T) {
    const long long r = i < n ? fa + i : fb + (i - n);
    diag[i] = (double)G[r * R + r];
  }
  __syncthreads();

  // pass 1: Σ d² over i < j, by region: [0] inside a, [1] inside b, [2] between
  const int total = N * N;
  double s3[3] = {0.0, 0.0, 0.0};
  for (int e = t; e < total; e += MMD_FOLD_T) {
    const int i = e / N, j = e - i * N;
    if (j <= i) continue;
    const long long ri = i < n ? fa + i : fb + (i - n), rj = j < n ? fa + j : fb + (j - n);
    const double v = diag[i] + diag[j] - 2.0 * (double)G[ri * R + rj];
    const double d2 = v < 0.0 ? 0.0 : v;                   // (a NaN stays a NaN)
    s3[j < n ? 0 : (i >= n ? 1 : 2)] += d2;
  }
  mmd_block_sum3(s3, red);
  const double pairs_all = 0.5 * ((double)N * N - N);
  double bw = (s3[0] + s3[1] + s3[2]) / pairs_all;
  const double mean_a = s3[0] / (0.5 * ((double)n * n - n)), mean_b = s3[1] / (0.5 * ((double)m * m - m));
  const double mean_ab = s3[2] / ((double)n * m);
  if (p.bandwidth_override) {
    const double o = p.bandwidth_override[0];
    if (o > 0.0) bw = o;
  }
  double mmd2 = 0.0;
  if (bw != 0.0) {                                         // (bw == 0: every row equals every other; a NaN bandwidth goes on and is counted)
    if (t < p.kernels) ninv[t] = -1.0 / (bw * p.scale[t]);
    __syncthreads();
    double k3[3] = {0.0, 0.0, 0.0};
    for (int e = t; e < total; e += MMD_FOLD_T) {
      const int i = e / N, j = e - i * N;
      if (j <= i) continue;
      const long long ri = i < n ? fa + i : fb + (i - n), rj = j < n ? fa + j : fb + (j - n);
      const double v = diag[i] + diag[j] - 2.0 * (double)G[ri * R + rj];
      const double d2 = v < 0.0 ? 0.0 : v;
      double k = 0.0;
      for (int q = 0; q < p.kernels; ++q) k += exp(d2 * ninv[q]);
      k3[j < n ? 0 : (i >= n ? 1 : 2)] += k;
    }
    mmd_block_sum3(k3, red);
    mmd2 = k3[0] / (0.5 * ((double)n * n - n)) + k3[1] / (0.5 * ((double)m * m - m)) - 2.0 * k3[2] / ((double)n * m);
  }
  if (t != 0) return;
  const double five[5] = {mmd2, bw, mean_a, mean_b, mean_ab};
  for (int c = 0; c < 5; ++c) p.out[pi * 5 + c] = five[c];
  if (p.live && p.live[0] == 0) return;
  if (!isfinite(mmd2)) {
    atomicAdd(p.nonfinite, 1);                             // integer: the word is the same in any order of the pairs
    return;
  }
  for (int c = 0; c < 5; ++c) p.sum[pi * 5 + c] += five[c];
  p.count[pi] += 1;
}

extern "C" int fst_mmd_fold(const float* G, const int32_t* rows_host, int n_sets, const int32_t* pairs_host, int n_pairs, int kernels,
                            float mul_f32, const double* bandwidth_override_dev, const int32_t* live_dev, double* out, double* sum,
                            int32_t* count, int32_t* nonfinite, void* stream) {
  const double mul = (double)mul_f32;
  MmdSets s = {};
  if (mmd_bind_sets("fst_mmd_fold", s, rows_host, n_sets)) return -1;
  FST_REQUIRE(G && out && sum && count && nonfinite && pairs_host, "fst_mmd_fold: null pointer");
  FST_REQUIRE(n_pairs >= 1 && n_pairs <= MMD_MAX_PAIRS, "fst_mmd_fold: %d pairs (1..%d)", n_pairs, MMD_MAX_PAIRS);
  FST_REQUIRE(kernels >= 1 && kernels <= MMD_MAX_KERNELS && mul > 0.0 && mul <= 1e30, "fst_mmd_fold: kernels = %d (1..%d), mul = %g (0 < mul <= 1e30)",
              kernels, MMD_MAX_KERNELS, mul);
  FST_REQUIRE((((uintptr_t)G | (uintptr_t)count | (uintptr_t)nonfinite | (uintptr_t)live_dev) & 3) == 0 &&
              (((uintptr_t)out | (uintptr_t)sum | (uintptr_t)bandwidth_override_dev) & 7) == 0,
              "fst_mmd_fold: G, count, nonfinite and live must be 4-byte aligned, out, sum and the bandwidth word 8-byte");
  MmdFoldParams p = {};
  for (int i = 0; i < n_pairs; ++i) {
    const int a = pairs_host[2 * i], b = pairs_host[2 * i + 1];
    FST_REQUIRE(a >= 0 && b >= 0 && a < n_sets && b < n_sets && a != b, "fst_mmd_fold: pair %d = (%d, %d) of %d sets", i, a, b, n_sets);
    FST_REQUIRE(rows_host[a] >= 2 && rows_host[b] >= 2, "fst_mmd_fold: pair %d: a set of fewer than 2 rows", i);
    p.pair[i][0] = a; p.pair[i][1] = b;
  }
  const int R = s.first[n_sets];
  const uint64_t g_bytes = (uint64_t)R * R * 4;
  FST_REQUIRE(mmd_disjoint(G, g_bytes, out, (uint64_t)n_pairs * 40) && mmd_disjoint(G, g_bytes, sum, (uint64_t)n_pairs * 40) &&
              mmd_disjoint(out, (uint64_t)n_pairs * 40, sum, (uint64_t)n_pairs * 40), "fst_mmd_fold: G, out and sum overlap");
  p.G = G; p.R = R; p.kernels = kernels;
  for (int i = 0; i <= MMD_MAX_SETS; ++i) p.first[i] = s.first[i];
  for (int q = 0; q < kernels; ++q) p.scale[q] = pow(mul, (double)(q - kernels / 2));
  p.bandwidth_override = bandwidth_override_dev; p.live = live_dev; p.out = out; p.sum = sum; p.count = count; p.nonfinite = nonfinite;
  hipLaunchKernelGGL(mmd_fold_kernel, dim3((unsigned)n_pairs), dim3(MMD_FOLD_T), 0, (hipStream_t)stream, p);
  FST_LAUNCH_CHECK();
  return 0;
}
