// Fused WaveGlow WN layer for gfx950 (Simplified_NF_WaveGlow.py:101-123, gate :44-54).
//
// One launch per layer and direction instead of three:
//
//   forward   g = W_in (*) a  (3 dilated taps, n channels each) + W_cond · u0 + (b_in + b_cond)        GEMM 1
//             t = tanh(g[:n]),  s = sigmoid(g[n:]),  acts = t·s                       in registers
//             r = W_rs · acts + b_rs;   a_next = a + r[:n];   out (+)= r[n:]                          GEMM 2
//             (last layer: W_rs has n rows, all of them skip rows: out += r)
//   backward  dacts = W_rsᵀ · [d_a_next ; d_out]                                                     GEMM 3
//             dg[:n] = dacts·s·(1−t²),  dg[n:] = dacts·t·s·(1−s)                      in registers
//
// so the [B, 2n, L] pre-activation never reaches HBM and acts is (optionally) never written: per layer forward the
// traffic is  a + u0 + out (read)  and  a_next + out + t,s (written) — 391 MB at B=256, L=512, n=120 against 880 MB for the
// three-launch form.
//
// Structure (shared with conv_gemm_bf3_kernel): split-bf16 products — hi·hi + hi·lo + lo·hi on
// the 32x32x16 bf16 MFMA, fp32 accumulation — operands through a 3-slot LDS ring filled by LDS-DMA, one raw
// s_barrier per 16-deep stage behind a counted vmcnt.  A workgroup = 4 waves = one batch element × 128 time samples;
// every wave owns ALL 256 (padded) output rows of its 32 samples, so that
//   * row m (tanh half) and row m+128 (sigmoid half) of GEMM 1 sit in the same lane and register index (blocks b and b+4):
//     the gate is pure per-lane VALU work on the accumulators;
//   * the 32×32 accumulator tiles of acts are, register for register, the B operand of GEMM 2 (a following MFMA that
//     sums over the accumulator's ROW index takes it with no lane movement: cdna_hip_programming.md §3) — the weights
//     of GEMM 2 are packed in the k-order that layout implies (wn_pack_kernel).
// Biases ride in the GEMMs: GEMM 1 has a constant-one input row (the first padding channel of the conditioning
// chunk, fed from a 16-byte block of ones), GEMM 2 sees acts[n] = 1 — so n < 128 is required (one spare K row).
// Two workgroups share a CU (79 KB of LDS, ≤ 256 registers): one's t,s store burst is the other's MFMA time.
#include "fst_device.h"
#include <type_traits>

#define WS_MAXL 10                                  // layers of a WN stack the one-launch kernels take (tables in the kernel arguments)
#define WN_TN 128                                  // time samples per workgroup
// forward kernel, per NW waves: WN_NBLK = NW + 1 32-sample column blocks per 8-channel row group (+1: sub-shift spill), WN_GS =
// WN_NBLK·1024 + 128 bytes per row group (+128: the lane halves hit different banks), ring slot = WN_A_BYTES + 2·WN_GS
#define WN_A_BYTES (8 * 2048)                      // 8 row blocks × (1 KiB hi + 1 KiB lo fragments)
#define WN_TILE_BYTES (32 * 36 * 4)                // one wave's [32][36] fp32 transpose tile
#define WN_FWD_LDS(NW) (3 * (WN_A_BYTES + 2 * (((NW) + 1) * 1024 + 128)))

// sigmoid and tanh from v_exp_f32 / v_rcp_f32 (≈1 ulp each): absolute error ≈ 2e-7, saturating correctly at ±inf
__device__ __forceinline__ float wn_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504f * x));
}
__device__ __forceinline__ float wn_tanh(float x) {
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.88539008f * x));
}

// GEMM-1 stage k < 3·CH → (chunk, tap): chunks in groups of WN_GRP, tap-major inside a group — the three windows of a chunk
// (the same lines but for 2·dil samples) are fetched WN_GRP stages apart: late enough for the first to have landed (adjacent
// stages pulling the same lines while in flight measured 35 % slower), early enough to still be in L2.
constexpr int WN_GRP = 2;
__host__ __device__ __forceinline__ void wn_stage_chunk_tap(int k, int CH, int& c, int& tap) {
  const int g = k / (3 * WN_GRP), rem = k - g * 3 * WN_GRP;
  const int gs = CH - g * WN_GRP < WN_GRP ? CH - g * WN_GRP : WN_GRP;
  tap = rem / gs;
  c = g * WN_GRP + rem - gs * tap;
}

// ------------------------------------------------------------------------------------------------
// weight images: four formats (forward here; backward, projected backward and data gradient beside their kernels), each a run of
// 2 KiB blocks = 64 lanes × 8 bf16 hi then 64 lanes × 8 bf16 lo, the A fragments of the 32x32x16 bf16 MFMA (lane l: row l&31 of
// the block, k = 8·(l>>5) + j), then 16 B of zeros (forward: and 16 B of ones) that the consumers' LDS-DMA reads for whatever lies
// outside a tensor.  Where an image ends — its size, its pack grid, its tail and every consumer's zero16 — is one function per format:
// ------------------------------------------------------------------------------------------------
__host__ __device__ static inline int wn_ch(int n) { return (n + 15) / 16; }
__host__ __device__ static inline int wn_ch2(int h) { return (h + 1 + 15) / 16; }
__host__ __device__ static inline int wn_fwd_stages(int CH, int CH2) { return 3 * CH + CH2 + 8; }                         // of 8 blocks
__host__ __device__ static inline int wn_bwd_stages(int CH, int last) { return (last ? 1 : 2) * CH; }                     // of 4 blocks
__host__ __device__ static inline int wn_bwd_proj_stages(int CH, int CHO, int last) { return (last ? 0 : CH) + CHO; }     // of 4 blocks
__host__ __device__ static inline int wn_dgrad_chunks(int n) { return (2 * n + 15) / 16; }                                // of 13 blocks

// one block of an image: lane `lane`'s eight values as four hi and four lo bf16 pairs
__device__ __forceinline__ void wn_store_frag(uint4* img, long long block, int lane, const float (&v)[8]) {
  unsigned hi[4], lo[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) split_bf16_pair(v[2 * j], v[2 * j + 1], hi[j], lo[j]);
  uint4* dst = img + block * 128 + lane;
  dst[0] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
  dst[64] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}
// the constants behind an image's n_blocks blocks, written by workgroup 0 of its pack
template <bool ONES>
__device__ __forceinline__ void wn_store_tail(uint4* img, long long n_blocks, int bx, int lane) {
  if (bx == 0 && lane < (ONES ? 2 : 1)) {
    const unsigned w = lane ? 0x3f800000u : 0u;
    img[n_blocks * 128 + lane] = make_uint4(w, w, w, w);
  }
}

// The arguments of a pack kernel: layer blockIdx.y of up to WS_MAXL layers, NSRC source tensors each; a format's scalars ride beside
// the table.  ML = the table's capacity: WS_MAXL for a stack entry point, 1 for a per-layer one (the same kernel, instantiated for a
// table of one: a per-layer call measured 0.2-0.4 us dearer with 568 bytes of arguments than with 64).
template <int NSRC, int ML = WS_MAXL>
struct WnPackTable {
  const float* src[NSRC][ML];
  uint4* img[ML];
  int nl, last_layer;   // the layer packed as `last` (a stack's top layer: nl - 1), or -1 for none
};
static_assert(sizeof(WnPackTable<6>) + 64 <= 4096, "kernel arguments: the largest pack table and its scalars");

// who; kernel; src[j][i] = source j of layer i; image_bytes against `expected`; blocks[l]: workgroups of a layer packed with
// last = l.  The grid is (the most blocks of any layer, nl): a kernel leaves early in a layer with fewer.  mid(): the entry point's
// own tests that sit between the layer count and the image size.
template <int NSRC, int ML, class Mid, class... S>
static int wn_pack_launch(const char* who, void (*kernel)(WnPackTable<NSRC, ML>, S...), const float* const* const (&src)[NSRC],
                          int nl, int last_layer, void* const* images, int64_t image_bytes, int64_t expected, const int (&blocks)[2],
                          Mid mid, void* stream, S... scalars) {
  constexpr bool stack = ML > 1;                     // the entry point takes tables, and its messages say so
  bool tables = images != nullptr;
  for (int j = 0; j < NSRC; ++j) tables = tables && src[j];
  FST_REQUIRE(tables, "%s: null table", who);
  FST_REQUIRE(nl >= 1 && nl <= ML, "%s: %d layers (1..%d)", who, nl, ML);
  if (int rc = mid()) return rc;
  FST_REQUIRE(image_bytes == expected, "%s: %s %lld bytes, expected %lld", who, stack ? "images are" : "image is",
              (long long)image_bytes, (long long)expected);
  WnPackTable<NSRC, ML> t = {};
  int grid_x = 0;
  for (int i = 0; i < nl; ++i) {
    bool operands = images[i] != nullptr;
    for (int j = 0; j < NSRC; ++j) operands = operands && src[j][i];
    FST_REQUIRE(operands, "%s: null operand in layer %d", who, i);
    FST_REQUIRE(fst_aligned16(images[i]), "%s: %s must be 16-byte aligned", who, stack ? "images" : "image");
    for (int j = 0; j < NSRC; ++j) t.src[j][i] = src[j][i];
    t.img[i] = static_cast<uint4*>(images[i]);
    grid_x = blocks[i == last_layer] > grid_x ? blocks[i == last_layer] : grid_x;
  }
  t.nl = nl; t.last_layer = last_layer;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid_x, (unsigned)nl), dim3(64), 0, (hipStream_t)stream, t, scalars...);
  FST_LAUNCH_CHECK();
  return 0;
}
static inline int wn_no_tests() { return 0; }

// ------------------------------------------------------------------------------------------------
// forward weight image
//   [S1 stages of GEMM 1][8 k-steps of GEMM 2][16 B of zeros][16 B of ones]
// one stage / k-step = 8 row blocks = 16 KiB.
//   GEMM 1  stage k < 3·CH = (chunk c < CH = ⌈n/16⌉, tap) in wn_stage_chunk_tap order: channels 16c.. of `a` at tap `tap`;
//           then CH2 = ⌈(h+1)/16⌉ stages
//           of the conditioning input (zero shift) whose channel h is the constant-one row carrying b_in + b_cond.
//           rows: blocks 0-3 = tanh rows 0..n-1, blocks 4-7 = sigmoid rows n..2n-1.
//   GEMM 2  k-step ks = (blk, s): element j of lane half hh multiplies acts row blk·32 + 16s + 8(j>>2) + 4hh + (j&3)
//           (the order in which an accumulator tile delivers its rows as a B operand); k = n carries b_rs.
//           rows: blocks 0-3 = residual rows (→ a_next), blocks 4-7 = skip rows (→ out); last layer: only skip rows.
// ------------------------------------------------------------------------------------------------
// sources: in_w [2n][n][3], cond_w [2n][h], in_b [2n], cond_b [2n], rs_w [2n][n] (last: [n][n]), rs_b [2n] (last: [n]).
// Workgroup blockIdx.x of layer blockIdx.y (64 lanes): row block bx & 7 of stage bx >> 3.
template <int ML>
__global__ __launch_bounds__(64) void wn_pack_kernel(WnPackTable<6, ML> t, int n, int h) {
  const int i = blockIdx.y, bx = blockIdx.x, last = i == t.last_layer;
  const float *in_w = t.src[0][i], *cond_w = t.src[1][i], *in_b = t.src[2][i], *cond_b = t.src[3][i], *rs_w = t.src[4][i], *rs_b = t.src[5][i];
  const int lane = threadIdx.x, blk = bx & 7, st = bx >> 3;
  const int CH = wn_ch(n), CH2 = wn_ch2(h), S1 = 3 * CH + CH2;
  const int hh = lane >> 5, rowb = (blk & 3) * 32 + (lane & 31);
  const bool row_ok = rowb < n;
  float v[8];
  if (st < S1) {
    const int row = (blk < 4 ? 0 : n) + rowb;                       // tanh | sigmoid half of the in_layer / cond_layer
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float w = 0.f;
      if (row_ok) {
        if (st < 3 * CH) {
          int cc, tap;
          wn_stage_chunk_tap(st, CH, cc, tap);
          const int c = cc * 16 + 8 * hh + j;
          if (c < n) w = in_w[((long long)row * n + c) * 3 + tap];
        } else {
          const int c = (st - 3 * CH) * 16 + 8 * hh + j;
          if (c < h) w = cond_w[(long long)row * h + c];
          else if (c == h) w = in_b[row] + cond_b[row];
        }
      }
      v[j] = w;
    }
  } else {
    const int ks = st - S1, kb = ks >> 1, s = ks & 1;
    const bool skip = blk >= 4;
    const bool live = row_ok && (!last || skip);
    const int row = (skip && !last ? n : 0) + rowb;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = kb * 32 + 16 * s + 8 * (j >> 2) + 4 * hh + (j & 3);
      float w = 0.f;
      if (live) {
        if (k < n) w = rs_w[(long long)row * n + k];
        else if (k == n) w = rs_b[row];
      }
      v[j] = w;
    }
  }
  wn_store_frag(t.img[i], bx, lane, v);
  wn_store_tail<true>(t.img[i], wn_fwd_stages(CH, CH2) * 8, bx, lane);
}

extern "C" int64_t fst_wn_image_bytes(int n, int h) {
  if (n <= 0 || h <= 0) return -1;
  return (int64_t)wn_fwd_stages(wn_ch(n), wn_ch2(h)) * WN_A_BYTES + 32;
}

extern "C" int fst_wn_pack(const float* in_w, const float* cond_w, const float* in_b, const float* cond_b,
                           const float* rs_w, const float* rs_b, int n, int h, int ntaps, int last, void* image,
                           int64_t image_bytes, void* stream) {
  FST_REQUIRE(in_w && cond_w && in_b && cond_b && rs_w && rs_b && image, "fst_wn_pack: null operand");
  FST_REQUIRE(ntaps == 3, "fst_wn_pack: the fused WN kernels are 3-tap (in_w [2n][n][3]); got %d taps", ntaps);
  FST_REQUIRE(n > 0 && n < 128 && h > 0, "fst_wn_pack: needs 0 < n < 128 (one spare K row carries the bias), h > 0; n=%d h=%d", n, h);
  const int blocks = wn_fwd_stages(wn_ch(n), wn_ch2(h)) * 8;
  return wn_pack_launch("fst_wn_pack", wn_pack_kernel<1>, {&in_w, &cond_w, &in_b, &cond_b, &rs_w, &rs_b}, 1, last ? 0 : -1, &image,
                        image_bytes, fst_wn_image_bytes(n, h), {blocks, blocks}, wn_no_tests, stream, n, h);
}

extern "C" int fst_wn_pack_stack(const float* const* in_w, const float* const* cond_w, const float* const* in_b,
                                 const float* const* cond_b, const float* const* rs_w, const float* const* rs_b, int nl, int n, int h,
                                 int ntaps, void* const* images, int64_t image_bytes, void* stream) {
  const int blocks = wn_fwd_stages(wn_ch(n), wn_ch2(h)) * 8;
  const auto mid = [&]() -> int {
    FST_REQUIRE(ntaps == 3, "fst_wn_pack_stack: the fused WN kernels are 3-tap (in_w [2n][n][3]); got %d taps", ntaps);
    FST_REQUIRE(n > 0 && n < 128 && h > 0, "fst_wn_pack_stack: needs 0 < n < 128 (one spare K row carries the bias), h > 0; n=%d h=%d", n, h);
    return 0;
  };
  return wn_pack_launch("fst_wn_pack_stack", wn_pack_kernel<WS_MAXL>, {in_w, cond_w, in_b, cond_b, rs_w, rs_b}, nl, nl - 1, images,
                        image_bytes, fst_wn_image_bytes(n, h), {blocks, blocks}, mid, stream, n, h);
}

#ifdef FST_STAMPS
// per-phase cycle sums of the fused forward kernel and the stack backward, lane 0 of every wave (fst_device.h)
__device__ unsigned long long wn_stamps[12];
extern "C" int fst_debug_wn_stamps(unsigned long long* out_host, int reset) { return fst_read_stamps(wn_stamps, out_host, reset); }
#endif

// ------------------------------------------------------------------------------------------------
// forward layer
// ------------------------------------------------------------------------------------------------
struct WnFwdParams {
  const float* a;
  long long a_bs;
  const float* u0;
  long long u0_bs;
  const char* img;
  float* ts;       // [B][2n][L]
  float* acts;     // [B][n][L] or null
  float* a_next;   // [B][n][L] (null on the last layer)
  float* out;      // [B][n][L]
  int B, L, n, h, dil, first, last;
  int CH, CH2, tiles_per_seq, n_wg;
};

// One accumulator tile (lane = time sample, registers = rows) → wave-private LDS tile [32][36] → each lane owns 4
// consecutive samples of rows rrow + 8j: four 16-byte global accesses per 32×32 tile, 8 rows × 128 contiguous bytes
// per wave-instruction.  MODE 0: store; 1: dst = v + res; 2: dst += v.
template <int MODE>
__device__ __forceinline__ void wn_store_tile(const float (&v)[16], float* tile, float* dst_rows, const float* res_rows,
                                              int rows_valid, int L, int t, int lane) {
  const int half = lane >> 5, l31 = lane & 31;
#pragma unroll
  for (int r = 0; r < 16; ++r) tile[((r & 3) + 8 * (r >> 2) + 4 * half) * 36 + l31] = v[r];
  const int rrow = lane >> 3, c4 = (lane & 7) * 4;
  const bool t_ok = t + c4 < L;
  float4 o[4], e[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = rrow + 8 * j;
    o[j] = *reinterpret_cast<const float4*>(tile + row * 36 + c4);
    e[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MODE != 0 && t_ok && row < rows_valid) {
      const float* src = (MODE == 1 ? res_rows : dst_rows) + (long long)row * L + t + c4;
      e[j] = *reinterpret_cast<const float4*>(src);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = rrow + 8 * j;
    if (t_ok && row < rows_valid) {
      float4 w = o[j];
      w.x += e[j].x; w.y += e[j].y; w.z += e[j].z; w.w += e[j].w;
      *reinterpret_cast<float4*>(dst_rows + (long long)row * L + t + c4) = w;
    }
  }
}

// the four 16-byte pieces (rows rrow + 8j, samples c4..c4+3) a lane contributes to a 32×32 tile
__device__ __forceinline__ void wn_fetch_tile(float4 (&q)[4], const float* src_rows, int rows_valid, int L, int t, int lane) {
  const int rrow = lane >> 3, c4 = (lane & 7) * 4;
  const bool t_ok = t + c4 < L;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = rrow + 8 * j;
    q[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t_ok && row < rows_valid) q[j] = *reinterpret_cast<const float4*>(src_rows + (long long)row * L + t + c4);
  }
}
// Accumulator layout ↔ global memory directly (lane = time sample, register r = row (r&3) + 8(r>>2) + 4·half): one
// wave-instruction moves two rows × 32 consecutive samples (two full 128-byte segments).  Sixteen dword accesses per tile
// instead of four 16-byte ones, but no LDS transpose and — for the loads — no wait inside an epilogue: operand tiles are
// read INTO the accumulators before the GEMM that adds to them (out = operand + A·B), so their latency hides under the
// ring's first stages, and being older than every LDS-DMA piece they are covered by the counted waits as they stand.
__device__ __forceinline__ void wn_acc_load(f32x16& v, const float* src_rows, int rows_valid, int L, int t, int lane) {
  const int half = lane >> 5, l31 = lane & 31;
  const bool t_ok = t + l31 < L && src_rows != nullptr;
  // one per-lane address; the row term of every access is wave-uniform (scalar offset)
  const float* lp = src_rows + ((long long)(4 * half) * L + t + l31);
  const int rv = rows_valid - 4 * half;                  // rows this lane half may touch: (r&3) + 8(r>>2) < rv
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2);
    v[r] = (t_ok && row < rv) ? lp[(long long)row * L] : 0.f;
  }
}
__device__ __forceinline__ void wn_acc_store(const f32x16& v, float* dst_rows, int rows_valid, int L, int t, int lane) {
  const int half = lane >> 5, l31 = lane & 31;
  const bool t_ok = t + l31 < L;
  float* lp = dst_rows + ((long long)(4 * half) * L + t + l31);
  const int rv = rows_valid - 4 * half;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2);
    if (t_ok && row < rv) lp[(long long)row * L] = v[r];
  }
}
__device__ __forceinline__ void wn_acc_store(const float (&v)[16], float* dst_rows, int rows_valid, int L, int t, int lane) {
  const int half = lane >> 5, l31 = lane & 31;
  const bool t_ok = t + l31 < L;
  float* lp = dst_rows + ((long long)(4 * half) * L + t + l31);
  const int rv = rows_valid - 4 * half;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2);
    if (t_ok && row < rv) lp[(long long)row * L] = v[r];
  }
}
// ... through the wave-private tile into the accumulator layout (lane = sample, registers = rows)
__device__ __forceinline__ void wn_tile_to_acc(float (&v)[16], const float4 (&q)[4], float* tile, int lane) {
  const int rrow = lane >> 3, c4 = (lane & 7) * 4, half = lane >> 5, l31 = lane & 31;
#pragma unroll
  for (int j = 0; j < 4; ++j) *reinterpret_cast<float4*>(tile + (rrow + 8 * j) * 36 + c4) = q[j];
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = tile[((r & 3) + 8 * (r >> 2) + 4 * half) * 36 + l31];
}

// Accumulator layout <-> global memory through raw buffer instructions: one descriptor per [rows][L] matrix of a batch element,
// ONE per-lane byte offset for the whole kernel (vlane = (4·half·L + l31)·4) and the row / column term of every access in the
// instruction's scalar offset — an access is one buffer_load/store_dword with no VALU work, no 64-bit address and no exec mask
// (wn_acc_load / _store form sixteen per-lane addresses per tile; the persistent kernel below has no registers for that).
// Columns beyond the sequence: the lane's offset is pushed out of the descriptor's range (loads return 0, stores are dropped by
// the hardware's range check).  Rows beyond the matrix: wave-uniform tests per register (the two lane halves of a register
// are 4 rows apart: a register whose upper half only is out of range goes through the half-masked offset).
#define WS_OOB 0x80000000u
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ws_rsrc(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x40000000, 0x00020000);
}
struct WsLane { unsigned vo, vo_lo; };     // offsets of a lane whose column exists: both halves / lower half only
__device__ __forceinline__ WsLane ws_lane(unsigned vlane, int tcol, int L, int lane) {
  WsLane w;
  w.vo = tcol + (lane & 31) < L ? vlane : WS_OOB;
  w.vo_lo = lane < 32 ? w.vo : WS_OOB;
  return w;
}
// tile = rows row0 .. row0+31 (rv of them exist, rv may be <= 0 or >= 32), columns tcol .. tcol+31 of the matrix behind `rs`
// (The scalar offsets are formed from an opaque copy of L: loop-invariant otherwise, the compiler computes those of every tile of
// the kernel ahead of the layer loop and keeps — i.e. spills — hundreds of them.)
__device__ __forceinline__ int ws_opaque(int x) {
  asm volatile("" : "+s"(x));
  return x;
}
__device__ __forceinline__ void ws_acc_load(f32x16& v, __amdgpu_buffer_rsrc_t rs, const WsLane w, int row0, int tcol, int rv, int L) {
  L = ws_opaque(L);
  rv = ws_opaque(rv);
  const int sbase = (row0 * L + tcol) * 4;
  if (rv >= 32) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      v[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, w.vo, sbase + ((r & 3) + 8 * (r >> 2)) * L * 4, 0));
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2);
      float x = 0.f;
      if (row < rv) x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, row + 4 < rv ? w.vo : w.vo_lo, sbase + row * L * 4, 0));
      v[r] = x;
    }
  }
}
template <class V>
__device__ __forceinline__ void ws_acc_store(const V& v, __amdgpu_buffer_rsrc_t rs, const WsLane w, int row0, int tcol, int rv, int L) {
  L = ws_opaque(L);
  rv = ws_opaque(rv);
  const int sbase = (row0 * L + tcol) * 4;
  if (rv >= 32) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)v[r]), rs, w.vo, sbase + ((r & 3) + 8 * (r >> 2)) * L * 4, 0);
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2);
      if (row < rv)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)v[r]), rs, row + 4 < rv ? w.vo : w.vo_lo, sbase + row * L * 4, 0);
    }
  }
}

// Row sums of an accumulator tile on its way out (bias gradients: Σ_{b,t} of every row): after the transpose each lane
// holds four consecutive samples of rows rrow + 8j, so a row's 32 samples are 8 lanes × float4 — three butterfly steps,
// then one LDS float add per row and wave.  `rows` = this WAVE's LDS array indexed by the tile's absolute row: one lane owns
// an entry, so the add is a plain read-modify-write in program order and the workgroup's sum over its waves (taken by the
// caller in wave order) is the same in every run — LDS float atomics from several waves were not.
__device__ __forceinline__ void wn_tile_row_sums(const float* tile, float* rows, int row0, int rows_valid, int L, int t, int lane) {
  const int rrow = lane >> 3, c4 = (lane & 7) * 4;
  const bool t_ok = t + c4 < L;                          // samples beyond the sequence are not part of the sum (L % 4 == 0)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 o = *reinterpret_cast<const float4*>(tile + (rrow + 8 * j) * 36 + c4);
    float s4 = t_ok ? (o.x + o.y) + (o.z + o.w) : 0.f;
    s4 += __shfl_xor(s4, 1, 64);
    s4 += __shfl_xor(s4, 2, 64);
    s4 += __shfl_xor(s4, 4, 64);
    if ((lane & 7) == 0 && rrow + 8 * j < rows_valid) rows[row0 + rrow + 8 * j] += s4;
  }
}

// NW waves per workgroup = 32·NW time samples: every wave streams the whole weight image through LDS whatever the tile width, so
// the L2→LDS fill per sample — the limiter of the 4-wave form (830 MB of pieces per launch) — halves at NW = 8
// (one workgroup of 8 waves per CU instead of two of 4: the same 2 waves per SIMD).
// one tile (32·NW samples from t0 of batch element b) of one layer: the whole body of the forward kernel
// (the arguments stay in the kernel-argument segment — constant address space: scalar loads at the point of use, rematerialised
// rather than kept in registers — for the per-layer kernel and for the persistent one alike)
typedef const __attribute__((address_space(4))) WnFwdParams WnFwdArgs;
// SAVE = false: the tile of a pass that no backward follows (wn_layer_infer_kernel / wn_stack_infer_kernel) — the gate block stores
// neither t,s nor acts (p.ts / p.acts are null and never touched); every other instruction is the saving tile's, in the same order
template <int NW, bool SAVE = true>
__device__ __forceinline__ void wn_fwd_tile(WnFwdArgs& p, const int b, const int t0, char* const ldsb) {
  constexpr int F_TN = 32 * NW, F_NBLK = F_TN / 32 + 1, F_GS = F_NBLK * 1024 + 128, F_SLOT = WN_A_BYTES + 2 * F_GS;
  constexpr int NA = WN_A_BYTES / 1024;              // 16 one-KiB pieces of A per stage
  constexpr int NI1 = NA + 2 * F_NBLK;              // 26 (NW = 4) / 34 (NW = 8) LDS-DMA wave-instructions per GEMM-1 stage
  int tid_o = threadIdx.x;
  asm volatile("" : "+v"(tid_o));                    // opaque per call: in the persistent kernel nothing derived from the lane id is
  const int tid = tid_o, lane = tid & 63;            //   hoisted out of the tile loops and kept alive across the whole body
  const int half = lane >> 5, l31 = lane & 31;
  const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_n0 = wave_s * 32;
  const int L = p.L, n = p.n, h = p.h, CH = p.CH;
  const int S1 = 3 * CH + p.CH2;
  const char* const zero16 = p.img + (long long)(S1 + 8) * WN_A_BYTES;     // S1 + 8 = wn_fwd_stages(CH, CH2), spelt out: the
                                                                          // call reorders this kernel's scalar code (ten to eighty instructions)
  const char* const ones16 = zero16 + 16;
  const float* const ab = p.a + (long long)b * p.a_bs;
  const float* const ub = p.u0 + (long long)b * p.u0_bs;

  // LDS-DMA of stage k into ring slot `slot`.  GEMM-1 stages: pieces [0, NA) are A, the rest the B sub-tiles
  // (8 channels × 32 samples of the 16-byte aligned, tap-shifted window); GEMM-2 k-steps: A only.
  // One stage's LDS-DMA, described by wave-uniform scalars (stage_src) and issued piece by piece (issue_piece: piece i of
  // this wave is ring piece wave + 4i).  GEMM-1 stages: pieces [0, NA) are A, the rest the B sub-tiles (8 channels × 32
  // samples of the 16-byte aligned, tap-shifted window); GEMM-2 k-steps: A only.
  struct StageSrc {
    char* sl;
    const char* asrc;
    const float* xb;
    int c_count, ones_row, t4, a0;
    bool spill, gemm2;
  };
  auto stage_src = [&](int k, int slot) {
    StageSrc ss;
    ss.sl = ldsb + slot * F_SLOT;
    ss.asrc = p.img + (long long)k * WN_A_BYTES;
    ss.gemm2 = k >= S1;
    ss.a0 = p.last ? 8 : 0;                            // last layer: only the skip-row blocks of GEMM 2 exist
    int shift = 0;
    if (k < 3 * CH) {
      int c, tap;
      wn_stage_chunk_tap(k, CH, c, tap);
      ss.xb = ab + (long long)(16 * c) * L;
      ss.c_count = min(16, n - 16 * c);
      ss.ones_row = -1;
      shift = (tap - 1) * p.dil;
    } else {
      const int c = k - 3 * CH;
      ss.xb = ub + (long long)(16 * c) * L;
      ss.c_count = min(16, h - 16 * c);
      ss.ones_row = h - 16 * c;                        // in [0, 16) on exactly one conditioning stage
    }
    const int tbase = t0 + shift;
    ss.t4 = tbase & ~3;
    ss.spill = (tbase & 3) != 0;
    return ss;
  };
  auto issue_piece = [&](const StageSrc& ss, int i) {
    if (ss.gemm2) {
      const int idx = ss.a0 + wave_s + NW * i;
      if (i < 16 / NW && idx < NA)
        lds_dma16(ss.asrc + idx * 1024 + lane * 16, ss.sl + idx * 1024);
      return;
    }
    const int idx = wave_s + NW * i;
    if (idx >= NI1) return;                            // wave-uniform
    if (idx < NA) {
      lds_dma16(ss.asrc + idx * 1024 + lane * 16, ss.sl + idx * 1024);
    } else {
      const int bi = idx - NA;
      const int gq = bi >= F_NBLK ? 1 : 0, m = bi - gq * F_NBLK;
      const int row = 8 * gq + (lane >> 3);
      const int t = ss.t4 + 32 * m + 4 * (lane & 7);
      bool ok = row < ss.c_count && t >= 0 && t < L;
      if (m == F_NBLK - 1) ok = ok && ss.spill && (lane & 7) == 0;
      const char* src = ok ? reinterpret_cast<const char*>(ss.xb + ((long long)row * L + t)) : (row == ss.ones_row ? ones16 : zero16);
      lds_dma16(src, ss.sl + WN_A_BYTES + gq * F_GS + m * 1024);
    }
  };
  constexpr int NPW1 = (NI1 + NW - 1) / NW;            // pieces per wave per GEMM-1 stage (waves >= NI1 % NW issue one fewer)
  static_assert(NPW1 <= 8, "the pieces of a stage are issued between the eight MFMA triples");
  auto issue = [&](int k, int slot) {
    const StageSrc ss = stage_src(k, slot);
#pragma unroll
    for (int i = 0; i < NPW1; ++i) issue_piece(ss, i);
  };
  // wait until this wave's pieces of the stage about to be read have landed; `next` = the one stage issued after it
  auto wait_for = [&](int next, int S) {
    if (next >= S) wait_vmcnt<0>();
    else if (next < S1) { if (wave_s < (NI1 % NW)) wait_vmcnt<(NI1 + NW - 1) / NW>(); else wait_vmcnt<NI1 / NW>(); }
    else if (p.last) wait_vmcnt<8 / NW>();
    else wait_vmcnt<16 / NW>();
  };

  f32x16 acc[8];
#pragma unroll
  for (int mb = 0; mb < 8; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mb][r] = 0.f;

  const int S = S1 + 8;
  FST_SUMS(12);
  FST_T(ts0);
  issue(0, 0);
  issue(1, 1);
  int slot = 0;
  FST_T(ts1);
  FST_ACC(0, ts0, ts1);                                // prologue
  // ---------------------------------------------------------------- GEMM 1: g = [W_in | W_cond | b] · [a taps ; u0 ; 1]
  for (int k = 0; k < S1; ++k) {
    FST_T(ta);
    wait_for(k + 1, S);
    FST_T(tb);
    FST_ACC(1, ta, tb);                                // vmcnt wait
    __builtin_amdgcn_s_barrier();                      // stage k is in LDS for everyone; the slot refilled next is drained
    FST_T(tc);
    FST_ACC(2, tb, tc);                                // barrier
    // stage k+2 goes into the slot every wave has just finished reading (k + 2 < S always holds here: 8 k-steps of
    // GEMM 2 follow).  Its pieces are issued one by one BETWEEN the MFMA triples below: an LDS-DMA issue costs the wave
    // 60-180 cycles, an MFMA holds the issue port for 8 of its 32 — interleaved, the address arithmetic and the issue
    // ride in the matrix pipe's shadow instead of in front of it.
    const StageSrc nxt = stage_src(k + 2, slot >= 1 ? slot - 1 : 2);
    FST_T(td);
    FST_ACC(3, tc, td);                                // LDS-DMA issue
    int shift = 0;
    if (k < 3 * CH) {
      int c_, tap_;
      wn_stage_chunk_tap(k, CH, c_, tap_);
      shift = (tap_ - 1) * p.dil;
    }
    const int sub = (t0 + shift) & 3;
    const char* base = ldsb + slot * F_SLOT;
    const int colx = wave_n0 + l31 + sub;
    const char* bp = base + WN_A_BYTES + half * F_GS + (colx >> 5) * 1024 + (colx & 31) * 4;
    // A fragments run ONE row block ahead of the MFMAs that consume them (two register pairs in rotation): read right in front
    // of their MFMAs — as the first form of this loop did, one `ds_read_b128; s_waitcnt lgkmcnt(0)` per fragment — every one of the
    // 16 reads of a stage exposed the LDS latency to a wave with nothing else to issue (115 such waits in the kernel's code)
    bf16x8 fah[2], fal[2];
    auto a_frag = [&](int mb) { lds_read_a_frag(base, mb, lane, fah[mb % 2], fal[mb % 2]); };
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const float*>(bp + j * 128);
    a_frag(0);                                             // lands under the split of the B fragment below
    bf16x8 bh, bl;
    split_bf16x8(v, bh, bl);
#ifdef FST_STAMPS
    asm volatile("" ::"v"(bh), "v"(bl));
#endif
    FST_T(te);
    FST_ACC(4, td, te);                                // B fragment: LDS reads + split
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) {
      if (mb + 1 < 8) a_frag(mb + 1);
      mfma_bf3(acc[mb], fah[mb % 2], fal[mb % 2], bh, bl);
      if (mb < NPW1) {
        __builtin_amdgcn_sched_barrier(0);
        issue_piece(nxt, mb);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    FST_T(tf);
    FST_ACC(5, te, tf);                                // A fragments + MFMA issue
    slot = slot == 2 ? 0 : slot + 1;
  }
  FST_T(tg0);

  // ---------------------------------------------------------------- gate (between stage S1-1 and the first k-step of GEMM 2)
  // Drain: the two k-steps in flight (S1, S1+1: A only, L2 hits issued one and two stages ago) land, so from here on
  // the t,s stores below are OLDER than every LDS-DMA a counted vmcnt will wait for — a counted wait retires
  // everything older than what it waits for, i.e. the stores get two k-steps of MFMA time to complete before the wait
  // in front of k-step S1+2 can see them.
  // (SAVE = false: there are no such stores.  The counts of wait_for stand — a counted wait names how many of the NEWEST operations,
  // the LDS-DMA pieces of the k-step issued last, may still fly; the t,s stores were older than every piece a counted wait is placed
  // behind, as the a / out operand loads of the gate still are, so they never entered a count.)
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();                        // every wave is past its last B read: the B areas are free
  const int tcol = t0 + wave_n0;
  // accumulator-layout global accesses as raw buffer instructions: one descriptor per matrix of this batch element, ONE per-lane
  // offset, row / column terms in the scalar offset (no 64-bit per-lane addresses, no exec masks: see ws_acc_load)
  const WsLane wl = ws_lane((unsigned)(4 * half * L + l31) * 4u, tcol, L, lane);
  const __amdgpu_buffer_rsrc_t ts_rs = ws_rsrc(SAVE ? p.ts + (long long)b * (2 * n) * L : nullptr);
  const __amdgpu_buffer_rsrc_t a_rs = ws_rsrc(ab), out_rs = ws_rsrc(p.out + (long long)b * n * L);
  const __amdgpu_buffer_rsrc_t an_rs = ws_rsrc(p.a_next ? p.a_next + (long long)b * n * L : p.out);
  bf16x8 bh2[8], bl2[8];
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) {
    float tv[16], sv[16], av[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float gt = acc[blk][r], gs = acc[blk + 4][r];
      tv[r] = wn_tanh(gt);
      sv[r] = wn_sigmoid(gs);
      const int row = blk * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      av[r] = row == n ? 1.0f : tv[r] * sv[r];         // acts[n] = 1 carries b_rs through GEMM 2 (rows > n: tanh(0)·σ(0) = 0)
    }
    const int rows_valid = n - blk * 32;               // may be <= 0: nothing stored
    if constexpr (SAVE) {
      ws_acc_store(tv, ts_rs, wl, blk * 32, tcol, rows_valid, L);
      ws_acc_store(sv, ts_rs, wl, n + blk * 32, tcol, rows_valid, L);
      if (p.acts) {
        float aw[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) aw[r] = tv[r] * sv[r];
        wn_acc_store(aw, p.acts + ((long long)b * n + blk * 32) * L, rows_valid, L, tcol, lane);
      }
    } else {
      // The stores also pinned this block's gate in front of the operand loads below: they consume tv / sv here.  Without them
      // nothing uses the gate's result before GEMM 2, the compiler sinks the tanh / sigmoid chains of all four blocks behind the
      // loads, and the loads land in fresh registers beside accumulators that still hold the gate's input: 300-430 spilled
      // VGPRs and 204 bytes of scratch in the first build.  An empty volatile statement per value keeps the order (volatile
      // statements are not reordered among themselves, and ws_acc_load starts with one); it emits no instruction.
#pragma unroll
      for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(av[r]));
    }
    // GEMM 2 accumulates onto what its rows are added to — the layer input for the residual rows (a_next = a + r), the
    // running skip sum for the skip rows (out += r) — read here, in accumulator layout, into the two accumulators the
    // gate has just consumed: the round trip hides under the remaining gate blocks and the first k-steps
    {
      const int rows_e = n - blk * 32;
      ws_acc_load(acc[blk], a_rs, wl, blk * 32, tcol, p.last ? 0 : rows_e, L);
      ws_acc_load(acc[blk + 4], out_rs, wl, blk * 32, tcol, p.first ? 0 : rows_e, L);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = av[8 * s + j];
      split_bf16x8(v, bh2[2 * blk + s], bl2[2 * blk + s]);
    }
  }
  asm volatile("" ::: "memory");                       // the stores stay in front of the LDS-DMA issued below
  FST_T(tg1);
  FST_ACC(6, tg0, tg1);                                // drain + gate + t,s stores (issue)

  // ---------------------------------------------------------------- GEMM 2: [a ; out] += [W_rs | b] · [acts ; 1]
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    const int k = S1 + ks;
    if (ks >= 2) wait_for(k + 1, S);                   // k-steps S1 and S1+1 landed at the drain above
    if (ks >= 1) __builtin_amdgcn_s_barrier();
    const bool more = k + 2 < S;
    const StageSrc nxt = stage_src(more ? k + 2 : k, slot >= 1 ? slot - 1 : 2);
    const char* base = ldsb + slot * F_SLOT;
    // (fragments one row block ahead, as in GEMM 1; on the last layer the residual-row blocks 0-3 are neither read nor multiplied)
    bf16x8 fah[2], fal[2];
    auto a_frag = [&](int mb) { lds_read_a_frag(base, mb, lane, fah[mb % 2], fal[mb % 2]); };
    if (!p.last) a_frag(0);
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) {
      if (mb + 1 < 8 && !(p.last && mb + 1 < 4)) a_frag(mb + 1);
      if (!(p.last && mb < 4)) mfma_bf3(acc[mb], fah[mb % 2], fal[mb % 2], bh2[ks], bl2[ks]);   // wave-uniform
      if (more && mb >= 4) {                           // four pieces per wave, behind the skip-row blocks (live on every layer)
        __builtin_amdgcn_sched_barrier(0);
        issue_piece(nxt, mb - 4);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    slot = slot == 2 ? 0 : slot + 1;
  }

  FST_T(tg2);
  FST_ACC(7, tg1, tg2);                                // GEMM 2
  // ---------------------------------------------------------------- a_next = a + r[:n];  out (+)= r[n:]
  // straight from the accumulators (the operands were read into them before GEMM 2): stores only, nothing to wait for
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) {
    const int rows_e = n - blk * 32;
    if (!p.last) ws_acc_store(acc[blk], an_rs, wl, blk * 32, tcol, rows_e, L);
    ws_acc_store(acc[blk + 4], out_rs, wl, blk * 32, tcol, rows_e, L);
  }
  FST_T(tg3);
  FST_ACC(8, tg2, tg3);                                // final epilogue (issue; includes waiting for the operand loads)
  FST_ACC(9, ts0, tg3);                                // whole wave
  FST_FLUSH(wn_stamps);
}

template <int NW>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void wn_layer_fwd_kernel(WnFwdParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // Workgroup → tile: ids that differ by a multiple of 8 share an XCD (round-robin dispatch), so give each XCD a
  // contiguous run of tiles: the tiles of one sequence, which re-read each other's halo for the dilated taps, then
  // meet in one L2.  Speed only.
  int wg = blockIdx.x;
  if ((p.n_wg & 7) == 0) wg = (wg & 7) * (p.n_wg >> 3) + (wg >> 3);
  const int b = wg / p.tiles_per_seq;
  const int t0 = (wg - b * p.tiles_per_seq) * (32 * NW);
  wn_fwd_tile<NW>(*(WnFwdArgs*)__builtin_amdgcn_kernarg_segment_ptr(), b, t0, reinterpret_cast<char*>(lds));
}

// ------------------------------------------------------------------------------------------------
// The forward of a whole WN stack in ONE persistent launch
//
// Launched layer by layer, every workgroup of the forward kernel walks the same phases at the same time — operand fetch, GEMM 1,
// the gate with its t,s stores, GEMM 2, the a_next / out stores — and the memory system alternates between idle (the GEMMs) and
// saturated (245 MB of stores + 195 MB of loads per layer in two bursts per tile round: the epilogue alone is 126 MB that no
// CU can multiply under; stamps: a third of a wave's life, profiles/r03_wn_fwd_stamps.txt).  Here ONE workgroup walks all tiles
// of its batch elements through all layers (the same tile body, the layer's arguments from tables in the kernel-argument
// segment; a_next / out of one layer are read by the next through the SAME CU: s_waitcnt vmcnt(0) + barrier between tiles, as in
// wn_stack_bwd_kernel), and nothing synchronises the workgroups with each other.  (Starting every other workgroup late, so that one
// half of the chip stores while the other multiplies, measured no gain at any delay: profiles/r04_wn_fwd_stack_timing.txt.)
// ------------------------------------------------------------------------------------------------
struct WnFwdStackParams {
  WnFwdParams layer[WS_MAXL];      // every layer's arguments as the per-layer launch would get them (a = the previous layer's a_next)
  int nl;
};

__global__ __launch_bounds__(512, 1) void wn_stack_fwd_kernel(WnFwdStackParams ps_by_value) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // a layer's arguments are read where they are used, with scalar loads from the kernel-argument segment at a run-time offset
  // (invariant memory: nothing has to stay in registers across the tile body)
  typedef const __attribute__((address_space(4))) WnFwdStackParams StackArgs;
  StackArgs& ps = *(StackArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  (void)ps_by_value;
  char* const ldsb = reinterpret_cast<char*>(lds);
  const int B = ps.layer[0].B, passes = ps.layer[0].tiles_per_seq;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    for (int layer = 0; layer < ps.nl; ++layer) {
      for (int pass = 0; pass < passes; ++pass) {
        WnFwdArgs* qp = &ps.layer[layer];
        asm volatile("" : "+s"(qp));                       // (opaque: the layer's arguments are loaded inside the tile body, not hoisted out of the loops)
        wn_fwd_tile<8>(*qp, b, pass * 256, ldsb);
        // this tile's stores (a_next, out, t,s) are complete and every wave is past its LDS reads before the next tile's
        // LDS-DMA refills the ring and reads what was stored
        wait_vmcnt<0>();
        __syncthreads();
      }
    }
  }
}

// The same two kernels for a pass that no backward follows: wn_fwd_tile<NW, false> — no t,s / acts stores, a_next and out bit for bit
// the saving kernels'.  Same workgroup → tile map, same persistent loop (a_next of layer i may be the buffer layer i − 1 read: every
// tile of a layer is stored and waited for — vmcnt(0) + barrier — before this workgroup starts the next layer, and no other
// workgroup touches this batch element).
template <int NW>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void wn_layer_infer_kernel(WnFwdParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int wg = blockIdx.x;
  if ((p.n_wg & 7) == 0) wg = (wg & 7) * (p.n_wg >> 3) + (wg >> 3);
  const int b = wg / p.tiles_per_seq;
  const int t0 = (wg - b * p.tiles_per_seq) * (32 * NW);
  wn_fwd_tile<NW, false>(*(WnFwdArgs*)__builtin_amdgcn_kernarg_segment_ptr(), b, t0, reinterpret_cast<char*>(lds));
}

__global__ __launch_bounds__(512, 1) void wn_stack_infer_kernel(WnFwdStackParams ps_by_value) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  typedef const __attribute__((address_space(4))) WnFwdStackParams StackArgs;
  StackArgs& ps = *(StackArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  (void)ps_by_value;
  char* const ldsb = reinterpret_cast<char*>(lds);
  const int B = ps.layer[0].B, passes = ps.layer[0].tiles_per_seq;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    for (int layer = 0; layer < ps.nl; ++layer) {
      for (int pass = 0; pass < passes; ++pass) {
        WnFwdArgs* qp = &ps.layer[layer];
        asm volatile("" : "+s"(qp));                       // (opaque, as in wn_stack_fwd_kernel)
        wn_fwd_tile<8, false>(*qp, b, pass * 256, ldsb);
        // this tile's stores (a_next, out) are complete and every wave is past its LDS reads before the next tile's LDS-DMA
        // refills the ring and reads what was stored
        wait_vmcnt<0>();
        __syncthreads();
      }
    }
  }
}

extern "C" int fst_wn_stack_fwd_ok(int n, int h, int L, int nl) {
  return n > 0 && n < 128 && h > 0 && L > 0 && L % 256 == 0 && nl >= 1 && nl <= WS_MAXL;
}

// The launch behind fst_wn_stack_fwd (save: ts[i] receives layer i's gate halves) and fst_wn_stack_infer (no ts table: nothing but
// a_next and out is stored, so a_next[i] may be the buffer layer i − 1 read, but not layer i's own input).
static int wn_stack_fwd_launch(const char* who, bool save, const float* const* a_in, const int64_t* a_bs, const void* const* images,
                               int64_t image_bytes, float* const* ts, float* const* a_next, const float* u0, int64_t u0_bs,
                               float* out, int nl, int B, int L, int n, int h, int64_t numel_a, void* stream) {
  FST_REQUIRE(a_in && a_bs && images && (ts || !save) && a_next && u0 && out, "%s: null operand", who);
  FST_REQUIRE(fst_wn_stack_fwd_ok(n, h, L, nl) && B > 0, "%s: B=%d L=%d n=%d h=%d nl=%d (needs n < 128, L %% 256 == 0, "
              "1 <= nl <= %d)", who, B, L, n, h, nl, WS_MAXL);
  FST_REQUIRE((long long)B * n * L == (long long)numel_a, "%s: B*n*L = %d*%d*%d does not match the element count %lld "
              "of the [B, n, L] tensors", who, B, n, L, (long long)numel_a);
  FST_REQUIRE(image_bytes == fst_wn_image_bytes(n, h), "%s: images are %lld bytes, expected %lld", who,
              (long long)image_bytes, (long long)fst_wn_image_bytes(n, h));
  FST_REQUIRE(B == 1 || u0_bs >= (int64_t)h * L, "%s: batch stride of u0 smaller than a sample", who);
  FST_REQUIRE(u0_bs % 4 == 0 && fst_aligned16(u0) && fst_aligned16(out), "%s: needs 16-byte aligned tensors", who);
  WnFwdStackParams p = {};
  for (int i = 0; i < nl; ++i) {
    const bool last = i == nl - 1;
    float* const ts_i = save ? ts[i] : nullptr;
    FST_REQUIRE(a_in[i] && images[i] && (ts_i || !save) && (a_next[i] || last), "%s: null operand of layer %d", who, i);
    FST_REQUIRE(a_bs[i] >= (int64_t)n * L && a_bs[i] % 4 == 0 && fst_aligned16(a_in[i]) && fst_aligned16(images[i]) && fst_aligned16(ts_i) && fst_aligned16(a_next[i]),
                "%s: layer %d: batch stride %lld smaller than a sample, or an operand that is not 16-byte aligned", who, i,
                (long long)a_bs[i]);
    FST_REQUIRE(last || a_in[i + 1] == a_next[i], "%s: the input of layer %d is not the a_next of layer %d", who, i + 1, i);
    FST_REQUIRE(save || last || a_next[i] != a_in[i], "%s: layer %d would store a_next over the input its neighbouring "
                "tiles still read", who, i);
    WnFwdParams& q = p.layer[i];
    q.a = a_in[i]; q.a_bs = a_bs[i]; q.u0 = u0; q.u0_bs = u0_bs; q.img = static_cast<const char*>(images[i]);
    q.ts = ts_i; q.acts = nullptr; q.a_next = last ? nullptr : a_next[i]; q.out = out;
    q.B = B; q.L = L; q.n = n; q.h = h; q.dil = 1 << i; q.first = i == 0; q.last = last;
    q.CH = wn_ch(n); q.CH2 = wn_ch2(h); q.tiles_per_seq = L / 256; q.n_wg = 0;
  }
  p.nl = nl;
  const int cus = fst_cu_count_or(256);
  const dim3 grid((unsigned)(B < cus ? B : cus));        // one resident workgroup per CU walks its batch elements
  if (int rc = fst_allow_full_lds(save ? (const void*)wn_stack_fwd_kernel : (const void*)wn_stack_infer_kernel, who)) return rc;
  fst_wn_set_route(save ? FST_WN_ROUTE_STACK_FWD : FST_WN_ROUTE_STACK_INFER, 8, 0, 0, 0, (int)grid.x, 1, 1, L / 256, 3, nl, WN_FWD_LDS(8));
  if (save) {
    hipLaunchKernelGGL(wn_stack_fwd_kernel, grid, dim3(512), WN_FWD_LDS(8), (hipStream_t)stream, p);
  } else {
    hipLaunchKernelGGL(wn_stack_infer_kernel, grid, dim3(512), WN_FWD_LDS(8), (hipStream_t)stream, p);
  }
  FST_LAUNCH_CHECK();
  return 0;
}

extern "C" int fst_wn_stack_fwd(const float* const* a_in, const int64_t* a_bs, const void* const* images, int64_t image_bytes,
                                float* const* ts, float* const* a_next, const float* u0, int64_t u0_bs, float* out, int nl, int B,
                                int L, int n, int h, int64_t numel_a, void* stream) {
  fst_wn_clear_route();
  return wn_stack_fwd_launch("fst_wn_stack_fwd", true, a_in, a_bs, images, image_bytes, ts, a_next, u0, u0_bs, out, nl, B, L, n, h,
                             numel_a, stream);
}

extern "C" int fst_wn_stack_infer(const float* const* a_in, const int64_t* a_bs, const void* const* images, int64_t image_bytes,
                                  float* const* a_next, const float* u0, int64_t u0_bs, float* out, int nl, int B, int L, int n, int h,
                                  int64_t numel_a, void* stream) {
  fst_wn_clear_route();
  return wn_stack_fwd_launch("fst_wn_stack_infer", false, a_in, a_bs, images, image_bytes, nullptr, a_next, u0, u0_bs, out, nl, B, L,
                             n, h, numel_a, stream);
}

// The launch behind fst_wn_layer_fwd (save: ts, and acts where given, are written) and fst_wn_layer_infer (neither exists; a_next
// must then not be a: a tile's neighbours read a's halo while the tile stores a_next).
static int wn_layer_fwd_launch(const char* who, bool save, const float* a, int64_t a_bs, const float* u0, int64_t u0_bs,
                               const void* image, int64_t image_bytes, float* ts, float* acts, float* a_next, float* out, int first,
                               int last, int B, int L, int n, int h, int dil, int64_t numel_a, void* stream) {
  FST_REQUIRE(a && u0 && image && (ts || !save) && out && (last || a_next), "%s: null operand", who);
  FST_REQUIRE(B > 0 && L > 0 && n > 0 && n < 128 && h > 0 && dil > 0, "%s: B=%d L=%d n=%d h=%d dil=%d (needs n < 128)", who,
              B, L, n, h, dil);
  FST_REQUIRE((long long)B * n * L == (long long)numel_a, "%s: B*n*L = %d*%d*%d does not match the element count %lld "
              "of the [B, n, L] tensors", who, B, n, L, (long long)numel_a);
  FST_REQUIRE(image_bytes == fst_wn_image_bytes(n, h), "%s: image is %lld bytes, expected %lld", who,
              (long long)image_bytes, (long long)fst_wn_image_bytes(n, h));
  FST_REQUIRE(B == 1 || (a_bs >= (int64_t)n * L && u0_bs >= (int64_t)h * L), "%s: batch stride smaller than a sample", who);
  FST_REQUIRE(L % 4 == 0 && a_bs % 4 == 0 && u0_bs % 4 == 0 && fst_aligned16(a) && fst_aligned16(u0) && fst_aligned16(image) && fst_aligned16(ts) && fst_aligned16(acts) &&
              fst_aligned16(a_next) && fst_aligned16(out), "%s: needs L %% 4 == 0 and 16-byte aligned tensors (L=%d)", who, L);
  FST_REQUIRE(save || last || a_next != a, "%s: a_next is a — a tile's neighbours read a's halo while the tile stores a_next", who);
  WnFwdParams p;
  p.a = a; p.a_bs = a_bs; p.u0 = u0; p.u0_bs = u0_bs; p.img = static_cast<const char*>(image);
  p.ts = ts; p.acts = acts; p.a_next = last ? nullptr : a_next; p.out = out;
  p.B = B; p.L = L; p.n = n; p.h = h; p.dil = dil; p.first = first ? 1 : 0; p.last = last ? 1 : 0;
  p.CH = wn_ch(n); p.CH2 = wn_ch2(h);
  // 256-sample tiles (8 waves) when they divide the sequence and still fill the chip, else 128-sample tiles (4 waves, two per CU)
  const int cus = fst_cu_count_or(256);
  const int nw = (L % 256 == 0 && (long long)B * (L / 256) >= cus) ? 8 : 4;
  const int tn = 32 * nw;
  p.tiles_per_seq = (L + tn - 1) / tn;
  p.n_wg = B * p.tiles_per_seq;
  const dim3 grid((unsigned)p.n_wg), block(64 * nw);
  const int lds = nw == 8 ? WN_FWD_LDS(8) : WN_FWD_LDS(4);
  const void* const kernel = save ? (nw == 8 ? (const void*)wn_layer_fwd_kernel<8> : (const void*)wn_layer_fwd_kernel<4>)
                                  : (nw == 8 ? (const void*)wn_layer_infer_kernel<8> : (const void*)wn_layer_infer_kernel<4>);
  if (int rc = fst_allow_full_lds(kernel, who)) return rc;
  fst_wn_set_route(save ? FST_WN_ROUTE_LAYER_FWD : FST_WN_ROUTE_LAYER_INFER, nw, 0, 0, 0, p.n_wg, 1, 1, p.tiles_per_seq, 3, 1, lds);
  if (save) {
    if (nw == 8) hipLaunchKernelGGL(wn_layer_fwd_kernel<8>, grid, block, lds, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(wn_layer_fwd_kernel<4>, grid, block, lds, (hipStream_t)stream, p);
  } else {
    if (nw == 8) hipLaunchKernelGGL(wn_layer_infer_kernel<8>, grid, block, lds, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(wn_layer_infer_kernel<4>, grid, block, lds, (hipStream_t)stream, p);
  }
  FST_LAUNCH_CHECK();
  return 0;
}

extern "C" int fst_wn_layer_fwd(const float* a, int64_t a_bs, const float* u0, int64_t u0_bs, const void* image,
                                int64_t image_bytes, float* ts, float* acts, float* a_next, float* out, int first, int last,
                                int B, int L, int n, int h, int dil, int64_t numel_a, void* stream) {
  fst_wn_clear_route();
  return wn_layer_fwd_launch("fst_wn_layer_fwd", true, a, a_bs, u0, u0_bs, image, image_bytes, ts, acts, a_next, out, first, last, B, L,
                             n, h, dil, numel_a, stream);
}

extern "C" int fst_wn_layer_infer(const float* a, int64_t a_bs, const float* u0, int64_t u0_bs, const void* image,
                                  int64_t image_bytes, float* a_next, float* out, int first, int last, int B, int L, int n, int h,
                                  int dil, int64_t numel_a, void* stream) {
  fst_wn_clear_route();
  return wn_layer_fwd_launch("fst_wn_layer_infer", false, a, a_bs, u0, u0_bs, image, image_bytes, nullptr, nullptr, a_next, out, first,
                             last, B, L, n, h, dil, numel_a, stream);
}

// ------------------------------------------------------------------------------------------------
// backward through res_skip and the gate:  dacts = W_rsᵀ·[d_a_next ; d_out],  dg = gate'(t, s)·dacts
//
// GEMM 3 has M = n (4 row blocks), K = 2n (n on the last layer): 12 MFMAs per 16-deep stage against 16 KiB of operand
// fill, and its inputs and outputs (d_a_next, d_out, t, s read once; dg written once) are 378 MB per layer — HBM-bound by a
// factor seven, so the kernel is shaped for streaming: small workgroups (one batch element × 128 samples, 50 KB of LDS,
// two per CU — WN_BWD_OCC), the t,s tiles of the first row block prefetched before the GEMM, the next block's while one is gated.
// Image: S3 = 2·CH (CH on the last layer) stages × 4 row blocks × (1 KiB hi + 1 KiB lo), then 16 B of zeros; stage (src, c):
// lane l holds W_rs[src·n + 16c + 8(l>>5) + j][blk·32 + (l&31)] — W_rs transposed, rows = acts channels.
// ------------------------------------------------------------------------------------------------
constexpr int WN_BWD_OCC = 2;                        // workgroups per CU the register budget is set for: 1024 tiles of the metric shape = two full
                                                     // rounds of 512 slots (three per CU: 1.33 rounds, 77 -> 70 us; and no scratch)
#define WN_BW_NB 4                                   // column blocks of a B row group (no tap shift: no spill block)
#define WN_BW_GS (WN_BW_NB * 1024 + 128)
#define WN_BW_A (4 * 2048)
#define WN_BW_SLOT (WN_BW_A + 2 * WN_BW_GS)
#define WN_BW_LDS (3 * WN_BW_SLOT)

// Workgroup bx of a layer's d_a / d_out stages: row block bx & 3 of stage bx >> 2, from rs_w [2n][n] (last: [n][n]).  acc_order:
// the d_a stages in the k-order in which a 32x32 accumulator tile delivers its rows as a B operand.
__device__ __forceinline__ void wn_pack_bwd_body(uint4* img, const float* rs_w, int n, int last, int acc_order, int bx) {
  const int lane = threadIdx.x, blk = bx & 3, st = bx >> 2;
  const int CH = wn_ch(n), hh = lane >> 5, m = blk * 32 + (lane & 31);
  const int src = last ? 0 : st / CH, c = st - src * CH;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    // acc_order (fst_wn_stack_bwd keeps d_a in its accumulators and multiplies straight out of them): element j of lane half
    // hh multiplies row 16c + 8(j>>2) + 4hh + (j&3) — registers 8s..8s+7 of the tile of row block c>>1, s = c&1
    const bool perm = acc_order && !last && src == 0;
    const int ch = 16 * c + (perm ? 8 * (j >> 2) + 4 * hh + (j & 3) : 8 * hh + j);
    v[j] = (m < n && ch < n) ? rs_w[(long long)(src * n + ch) * n + m] : 0.f;
  }
  wn_store_frag(img, bx, lane, v);
}

// source: rs_w.  Layer blockIdx.y; the `last` layer has half the stages, its other workgroups leave.
template <int ML>
__global__ __launch_bounds__(64) void wn_pack_bwd_kernel(WnPackTable<1, ML> t, int n, int acc_order) {
  const int i = blockIdx.y, bx = blockIdx.x, last = i == t.last_layer, n_blocks = wn_bwd_stages(wn_ch(n), last) * 4;
  if (bx >= n_blocks) return;
  wn_pack_bwd_body(t.img[i], t.src[0][i], n, last, acc_order, bx);
  wn_store_tail<false>(t.img[i], n_blocks, bx, threadIdx.x);
}

extern "C" int64_t fst_wn_bwd_image_bytes(int n, int last) {
  if (n <= 0) return -1;
  return (int64_t)wn_bwd_stages(wn_ch(n), last) * WN_BW_A + 16;
}

extern "C" int fst_wn_pack_bwd(const float* rs_w, int n, int last, int acc_order, void* image, int64_t image_bytes, void* stream) {
  FST_REQUIRE(rs_w && image && n > 0 && n <= 128, "fst_wn_pack_bwd: bad arguments (n=%d, needs n <= 128)", n);
  return wn_pack_launch("fst_wn_pack_bwd", wn_pack_bwd_kernel<1>, {&rs_w}, 1, last ? 0 : -1, &image, image_bytes,
                        fst_wn_bwd_image_bytes(n, last), {wn_bwd_stages(wn_ch(n), 0) * 4, wn_bwd_stages(wn_ch(n), 1) * 4}, wn_no_tests,
                        stream, n, acc_order ? 1 : 0);
}

// images[i] of fst_wn_bwd_image_bytes(n, i == nl - 1) bytes: image_bytes is that of the layers below the top one
extern "C" int fst_wn_pack_bwd_stack(const float* const* rs_w, int nl, int n, int acc_order, void* const* images, int64_t image_bytes,
                                     void* stream) {
  FST_REQUIRE(rs_w && images && n > 0 && n <= 128, "fst_wn_pack_bwd_stack: bad arguments (n=%d, needs n <= 128)", n);
  return wn_pack_launch("fst_wn_pack_bwd_stack", wn_pack_bwd_kernel<WS_MAXL>, {rs_w}, nl, nl - 1, images, image_bytes,
                        fst_wn_bwd_image_bytes(n, 0), {wn_bwd_stages(wn_ch(n), 0) * 4, wn_bwd_stages(wn_ch(n), 1) * 4}, wn_no_tests,
                        stream, n, acc_order ? 1 : 0);
}

// ------------------------------------------------------------------------------------------------
// The projected image of fst_wn_stack_bwd_proj: d_out = W_endᵀ·do is a rank-2h image of the end conv's cotangent do [B][2h][L],
// so the skip half of GEMM 3 is  W_skip,iᵀ·d_out = (W_end·W_skip,i)ᵀ·do  and the kernel multiplies do itself: 2h operand rows
// instead of n, CHO = ceil(2h/16) stages instead of CH.  Per layer [d_a stages: CH, acc_order][skip stages: CHO] (the top layer:
// skip stages only), then 16 B of zeros.  Skip stage c: lane l holds F_i[16c + 8(l>>5) + j][blk·32 + (l&31)], F_i = W_end·W_skip,i
// ([2h][n]; rows >= 2h and columns >= n are zero) — every element one fp32 fmaf chain over k = 0..n-1, then the hi/lo split.
// ------------------------------------------------------------------------------------------------
// source: rs_w; end_w [2h][n] is the stack's
__global__ __launch_bounds__(64) void wn_pack_bwd_proj_kernel(WnPackTable<1> t, const float* end_w, int n, int h2) {
  const int i = blockIdx.y, bx = blockIdx.x, lane = threadIdx.x, last = i == t.last_layer;
  const int n_da = last ? 0 : wn_ch(n), n_blocks = wn_bwd_proj_stages(wn_ch(n), wn_ch(h2), last) * 4;
  if (bx >= n_blocks) return;
  wn_store_tail<false>(t.img[i], n_blocks, bx, lane);
  if ((bx >> 2) < n_da) {                              // a d_a stage: what fst_wn_pack_bwd (acc_order = 1) writes there
    wn_pack_bwd_body(t.img[i], t.src[0][i], n, 0, 1, bx);
    return;
  }
  const int blk = bx & 3, c = (bx >> 2) - n_da;
  const int m = blk * 32 + (lane & 31), hh = lane >> 5;
  const float* const w_skip = t.src[0][i] + (long long)(last ? 0 : n) * n;     // [n][n]: skip channel k, acts channel m
  // the stage's 16 rows of W_end, rows >= h2 as zeros: every lane then runs the same chain of independent loads
  __shared__ float e_rows[16 * 128];
  for (int x = lane; x < 16 * n; x += 64) {
    const int r = x / n, k = x - r * n;
    e_rows[r * 128 + k] = 16 * c + r < h2 ? end_w[(long long)(16 * c + r) * n + k] : 0.f;
  }
  __syncthreads();
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0.f;
  if (m < n) {
#pragma unroll 8
    for (int k = 0; k < n; ++k) {                        // one fmaf chain per element, k ascending
      const float w = w_skip[(long long)k * n + m];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = fmaf(e_rows[(8 * hh + j) * 128 + k], w, v[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (16 * c + 8 * hh + j >= h2) v[j] = 0.f;           // dead rows are zeros whatever the weights hold
  wn_store_frag(t.img[i], bx, lane, v);
}

extern "C" int64_t fst_wn_bwd_proj_image_bytes(int n, int h2, int last) {
  if (n <= 0 || h2 <= 0) return -1;
  return (int64_t)wn_bwd_proj_stages(wn_ch(n), wn_ch(h2), last) * WN_BW_A + 16;
}

// images[i] of fst_wn_bwd_proj_image_bytes(n, h2, i == nl - 1) bytes: image_bytes is that of the layers below the top one
extern "C" int fst_wn_pack_bwd_proj_stack(const float* const* rs_w, const float* end_w, int nl, int n, int h2, void* const* images,
                                          int64_t image_bytes, void* stream) {
  FST_REQUIRE(rs_w && end_w && images && n > 0 && n <= 128 && h2 > 0 && h2 <= 64,
              "fst_wn_pack_bwd_proj_stack: bad arguments (n=%d, h2=%d; needs n <= 128, h2 <= 64)", n, h2);
  const int CH = wn_ch(n), CHO = wn_ch(h2);
  return wn_pack_launch("fst_wn_pack_bwd_proj_stack", wn_pack_bwd_proj_kernel, {rs_w}, nl, nl - 1, images, image_bytes,
                        fst_wn_bwd_proj_image_bytes(n, h2, 0), {wn_bwd_proj_stages(CH, CHO, 0) * 4, wn_bwd_proj_stages(CH, CHO, 1) * 4},
                        wn_no_tests, stream, end_w, n, h2);
}

struct WnBwdParams {
  const float* d_a;    // [B][n][L], null on the last layer
  const float* d_out;  // [B][n][L]
  const float* ts;     // [B][2n][L]
  const char* img;
  float* dg;           // [B][2n][L]
  float* row_sums;     // optional [256][n_wg]: per-workgroup Σ_t dg[row] (rows [0, 2n)) — the in_layer / cond_layer bias gradient
  int B, L, n, last, CH, tiles_per_seq, n_wg;
};

// One stage of GEMM 3 for one 32-sample column block: the stage's four row blocks of W_rsᵀ (A fragments at base) times the
// B fragment (bh, bl).  The body of wn_layer_bwd_kernel's stage loop and of both operand sources of wn_stack_bwd_kernel's phase A.
__device__ __forceinline__ void wn_bwd_multiply(f32x16 (&acc)[4], const char* base, int lane, bf16x8 bh, bf16x8 bl) {
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    bf16x8 ah, al;
    lds_read_a_frag(base, mb, lane, ah, al);
    mfma_bf3(acc[mb], ah, al, bh, bl);
  }
}

// [8 waves][R] per-wave row sums in LDS -> out[R][stride] at column col, the waves added in a fixed order (after a workgroup
// barrier: every wave has added its last tile).  512 threads.
__device__ __forceinline__ void wn_reduce_row_sums(const float* rsum, int R, float* out, int stride, int col, int tid) {
  __syncthreads();
  if (tid < R) {
    float s8 = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) s8 += rsum[w * R + tid];
    out[(long long)tid * stride + col] = s8;
  }
}

__global__ __launch_bounds__(256, WN_BWD_OCC) void wn_layer_bwd_kernel(WnBwdParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  char* const ldsb = reinterpret_cast<char*>(lds);
  const int tid = threadIdx.x, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
  int wg = blockIdx.x;
  if ((p.n_wg & 7) == 0) wg = (wg & 7) * (p.n_wg >> 3) + (wg >> 3);
  const int b = wg / p.tiles_per_seq;
  const int t0 = (wg - b * p.tiles_per_seq) * WN_TN;
  const int wave_n0 = wave_s * 32;
  const int L = p.L, n = p.n, CH = p.CH;
  const int S3 = wn_bwd_stages(CH, p.last);
  const char* const zero16 = p.img + (long long)S3 * WN_BW_A;
  const float* const ts_b = p.ts + (long long)b * (2 * n) * L;
  const int tcol = t0 + wave_n0;

  // pieces per stage: 8 of A, 2 x 4 of B = 16 -> exactly four per wave
  auto issue = [&](int k, int slot) {
    char* const sl = ldsb + slot * WN_BW_SLOT;
    const char* asrc = p.img + (long long)k * WN_BW_A;
    const bool from_da = !p.last && k < CH;
    const int c = from_da ? k : k - (p.last ? 0 : CH);
    const float* xb = (from_da ? p.d_a : p.d_out) + ((long long)b * n + 16 * c) * L;
    const int c_count = min(16, n - 16 * c);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = wave_s + 4 * i;
      if (idx < 8) {
        lds_dma16(asrc + idx * 1024 + lane * 16, sl + idx * 1024);
      } else {
        const int bi = idx - 8;
        const int gq = bi >> 2, m = bi & 3;
        const int row = 8 * gq + (lane >> 3);
        const int t = t0 + 32 * m + 4 * (lane & 7);
        const bool ok = row < c_count && t < L;
        const char* src = ok ? reinterpret_cast<const char*>(xb + ((long long)row * L + t)) : zero16;
        lds_dma16(src, sl + WN_BW_A + gq * WN_BW_GS + m * 1024);
      }
    }
  };

  f32x16 acc[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mb][r] = 0.f;

  // The gate halves of the first row block, issued BEFORE any LDS-DMA: they are then the oldest vector-memory operations
  // of the wave, so every counted wait below (which retires everything older than what it leaves in flight) covers them
  // and the counts stay "pieces of the next stage".  First use is after the GEMM.
  float4 qt[4], qs[4];
  wn_fetch_tile(qt, ts_b, n, L, tcol, lane);
  wn_fetch_tile(qs, ts_b + (long long)n * L, n, L, tcol, lane);
  asm volatile("" ::: "memory");
  issue(0, 0);
  if (S3 > 1) issue(1, 1);
  int slot = 0;
  for (int k = 0; k < S3; ++k) {
    if (k + 1 < S3) wait_vmcnt<4>(); else wait_vmcnt<0>();           // stage k landed; stage k+1's 4 pieces may fly on
    __builtin_amdgcn_s_barrier();
    if (k + 2 < S3) issue(k + 2, slot >= 1 ? slot - 1 : 2);
    const char* base = ldsb + slot * WN_BW_SLOT;
    const int colx = wave_n0 + l31;
    const char* bp = base + WN_BW_A + half * WN_BW_GS + (colx >> 5) * 1024 + (colx & 31) * 4;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const float*>(bp + j * 128);
    bf16x8 bh, bl;
    split_bf16x8(v, bh, bl);
    wn_bwd_multiply(acc, base, lane, bh, bl);
    slot = slot == 2 ? 0 : slot + 1;
  }
  __syncthreads();                                     // every wave is past its last fragment read: the ring becomes tiles
  float* const tile = reinterpret_cast<float*>(ldsb + wave_s * WN_TILE_BYTES);
  float* const rsum = reinterpret_cast<float*>(ldsb + 4 * WN_TILE_BYTES);      // [4 waves][256] row sums of this workgroup's dg tile
  float* const rsum_w = rsum + wave_s * 256;
  if (p.row_sums) {
#pragma unroll
    for (int w = 0; w < 4; ++w) rsum[w * 256 + tid] = 0.f;
    __syncthreads();
  }
  float* const dg_b = p.dg + (long long)b * (2 * n) * L;
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) {
    const int rows_valid = n - blk * 32;
    float tv[16], sv[16], gt[16], gs[16];
    wn_tile_to_acc(tv, qt, tile, lane);
    wn_tile_to_acc(sv, qs, tile, lane);
    if (blk < 3) {                                     // next row block's gate halves, in flight while this one is gated
      wn_fetch_tile(qt, ts_b + (long long)((blk + 1) * 32) * L, n - (blk + 1) * 32, L, tcol, lane);
      wn_fetch_tile(qs, ts_b + (long long)(n + (blk + 1) * 32) * L, n - (blk + 1) * 32, L, tcol, lane);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float d = acc[blk][r], t = tv[r], s = sv[r];
      gt[r] = d * s * (1.f - t * t);
      gs[r] = d * t * s * (1.f - s);
    }
    wn_store_tile<0>(gt, tile, dg_b + (long long)(blk * 32) * L, nullptr, rows_valid, L, tcol, lane);
    if (p.row_sums) wn_tile_row_sums(tile, rsum_w, blk * 32, rows_valid, L, tcol, lane);
    wn_store_tile<0>(gs, tile, dg_b + (long long)(n + blk * 32) * L, nullptr, rows_valid, L, tcol, lane);
    if (p.row_sums) wn_tile_row_sums(tile, rsum_w, n + blk * 32, rows_valid, L, tcol, lane);
  }
  if (p.row_sums) {
    __syncthreads();
    // [256][n_wg]: the caller's sum runs over the contiguous axis; waves added in a fixed order
    p.row_sums[(long long)tid * p.n_wg + wg] = (rsum[tid] + rsum[256 + tid]) + (rsum[512 + tid] + rsum[768 + tid]);
  }
}

extern "C" int fst_wn_layer_bwd(const float* d_a, const float* d_out, const float* ts, const void* image, int64_t image_bytes,
                                float* dg, float* row_sums, int64_t row_sums_rows, int last, int B, int L, int n,
                                int64_t numel_a, void* stream) {
  fst_wn_clear_route();
  FST_REQUIRE(d_out && ts && image && dg && (last || d_a), "fst_wn_layer_bwd: null operand");
  FST_REQUIRE(B > 0 && L > 0 && n > 0 && n <= 128, "fst_wn_layer_bwd: B=%d L=%d n=%d (needs n <= 128)", B, L, n);
  FST_REQUIRE((long long)B * n * L == (long long)numel_a, "fst_wn_layer_bwd: B*n*L = %d*%d*%d does not match the element count %lld "
              "of the [B, n, L] tensors", B, n, L, (long long)numel_a);
  FST_REQUIRE(image_bytes == fst_wn_bwd_image_bytes(n, last), "fst_wn_layer_bwd: image is %lld bytes, expected %lld",
              (long long)image_bytes, (long long)fst_wn_bwd_image_bytes(n, last));
  FST_REQUIRE(L % 4 == 0 && fst_aligned16(d_a) && fst_aligned16(d_out) && fst_aligned16(ts) && fst_aligned16(image) && fst_aligned16(dg),
              "fst_wn_layer_bwd: needs L %% 4 == 0 and 16-byte aligned tensors (L=%d)", L);
  WnBwdParams p;
  p.d_a = last ? nullptr : d_a; p.d_out = d_out; p.ts = ts; p.img = static_cast<const char*>(image); p.dg = dg;
  p.row_sums = row_sums;
  p.B = B; p.L = L; p.n = n; p.last = last ? 1 : 0; p.CH = wn_ch(n);
  p.tiles_per_seq = (L + WN_TN - 1) / WN_TN;
  p.n_wg = B * p.tiles_per_seq;
  FST_REQUIRE(row_sums == nullptr || row_sums_rows == p.n_wg, "fst_wn_layer_bwd: row_sums has %lld rows, the launch has %d "
              "workgroups (B x ceil(L/128))", (long long)row_sums_rows, p.n_wg);
  if (int rc = fst_allow_full_lds((const void*)wn_layer_bwd_kernel, "fst_wn_layer_bwd")) return rc;
  fst_wn_set_route(FST_WN_ROUTE_LAYER_BWD, 0, 0, 0, 0, p.n_wg, 1, 1, p.tiles_per_seq, 3, 1, WN_BW_LDS);
  hipLaunchKernelGGL(wn_layer_bwd_kernel, dim3((unsigned)p.n_wg), dim3(256), WN_BW_LDS, (hipStream_t)stream, p);
  FST_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// data gradient of the in_layer + cond_layer:   d_a = d_a_next + W_inᵀ (*) dg  (3 dilated taps),   d_u0 += W_condᵀ · dg
//
// The LDS-DMA path, not the matrix pipe, bounds these GEMMs (tools/dma_ring_probe.hip: ≈34 GB/s per CU, 8.7 TB/s chip-wide,
// whatever the prefetch depth): so the kernel is shaped to move few bytes per MFMA.
//   * one stage = 16 channels of dg with ALL THREE taps: the B window [16 ch][256 + 2·dil (+3)] is fetched once and each tap
//     reads it at its own column offset (a third of the B bytes for small dilations; the per-tap form fetched three windows);
//   * the 25 conditioning rows ride along as a fifth row block of the centre tap instead of a second pass over dg;
//   * a workgroup = 8 waves = one batch element × 256 time samples (each wave 32 samples × 5 row blocks): the weight bytes
//     per output sample are half those of a 128-sample tile.
// Image: per 16-channel chunk 13 row blocks × (1 KiB hi + 1 KiB lo): [tap 0: 4 blocks of d_a rows][tap 1: 4 + the d_u0 block]
// [tap 2: 4]; tap τ multiplies dg at t + (1 − τ)·dil.  Ring of 2 slots (ns of fst_wn_last_route): with 512-sample tiles a slot is
// 61 696 bytes at dilation 1 and grows with the dilation, so three never fit 160 KiB.
// ------------------------------------------------------------------------------------------------
#define DG_NCB 2                                     // 32-sample column blocks per wave
#define DG_TN (8 * 32 * DG_NCB)                       // time samples per workgroup (8 waves)
#define DG_A_BLOCKS 13
#define DG_A_BYTES (DG_A_BLOCKS * 2048)

// sources: in_w [2n][n][3], cond_w [2n][h].  Workgroup blockIdx.x of the 13·CHK of layer blockIdx.y.
template <int ML>
__global__ __launch_bounds__(64) void wn_pack_dgrad_kernel(WnPackTable<2, ML> t, int n, int h) {
  const int i = blockIdx.y, bx = blockIdx.x;
  const float *in_w = t.src[0][i], *cond_w = t.src[1][i];
  const int lane = threadIdx.x, ab = bx % DG_A_BLOCKS, c = bx / DG_A_BLOCKS;
  const int hh = lane >> 5, l31 = lane & 31;
  // block ab of the chunk -> (tap, row block)
  int tap, blk;
  if (ab < 4) { tap = 0; blk = ab; } else if (ab < 9) { tap = 1; blk = ab - 4; } else { tap = 2; blk = ab - 9; }
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 16 * c + 8 * hh + j;                   // dg channel = output row of the forward convs
    float w = 0.f;
    if (k < 2 * n) {
      if (blk < 4) {
        const int m = blk * 32 + l31;
        if (m < n) w = in_w[((long long)k * n + m) * 3 + tap];
      } else {
        if (l31 < h) w = cond_w[(long long)k * h + l31];
      }
    }
    v[j] = w;
  }
  wn_store_frag(t.img[i], bx, lane, v);
  wn_store_tail<false>(t.img[i], wn_dgrad_chunks(n) * DG_A_BLOCKS, bx, lane);
}

extern "C" int64_t fst_wn_dgrad_image_bytes(int n) {
  if (n <= 0) return -1;
  return (int64_t)wn_dgrad_chunks(n) * DG_A_BYTES + 16;
}

extern "C" int fst_wn_pack_dgrad(const float* in_w, const float* cond_w, int n, int h, int ntaps, void* image, int64_t image_bytes,
                                 void* stream) {
  FST_REQUIRE(in_w && cond_w && image && n > 0 && n <= 128 && h > 0 && h <= 32, "fst_wn_pack_dgrad: needs n <= 128, h <= 32 (n=%d h=%d)", n, h);
  FST_REQUIRE(ntaps == 3, "fst_wn_pack_dgrad: the fused WN kernels are 3-tap (in_w [2n][n][3]); got %d taps", ntaps);
  const int blocks = wn_dgrad_chunks(n) * DG_A_BLOCKS;
  return wn_pack_launch("fst_wn_pack_dgrad", wn_pack_dgrad_kernel<1>, {&in_w, &cond_w}, 1, -1, &image, image_bytes,
                        fst_wn_dgrad_image_bytes(n), {blocks, blocks}, wn_no_tests, stream, n, h);
}

extern "C" int fst_wn_pack_dgrad_stack(const float* const* in_w, const float* const* cond_w, int nl, int n, int h, int ntaps,
                                       void* const* images, int64_t image_bytes, void* stream) {
  FST_REQUIRE(in_w && cond_w && images && n > 0 && n <= 128 && h > 0 && h <= 32, "fst_wn_pack_dgrad_stack: needs n <= 128, h <= 32 (n=%d h=%d)", n, h);
  const int blocks = wn_dgrad_chunks(n) * DG_A_BLOCKS;
  const auto mid = [&]() -> int {
    FST_REQUIRE(ntaps == 3, "fst_wn_pack_dgrad_stack: the fused WN kernels are 3-tap (in_w [2n][n][3]); got %d taps", ntaps);
    return 0;
  };
  return wn_pack_launch("fst_wn_pack_dgrad_stack", wn_pack_dgrad_kernel<WS_MAXL>, {in_w, cond_w}, nl, nl - 1, images, image_bytes,
                        fst_wn_dgrad_image_bytes(n), {blocks, blocks}, mid, stream, n, h);
}

// One data-gradient stage into the ring slot at sl, as 1-KiB LDS-DMA pieces dealt round the eight waves: the 13 weight blocks of
// chunk c of the image, then the two 8-channel row groups of the dg window [16 channels of chunk c][nblkw blocks from column
// (t0 - dil) & ~3] of one batch element (dg_b: its [2n][L] matrix); rows past 2n and columns outside [0, L) read the image's zeros.
__device__ __forceinline__ void wn_dgrad_issue(char* sl, const char* img, const float* dg_b, int c, int t0, int n, int L, int dil,
                                               int nblkw, int gsw, int wave_s, int lane) {
  const char* asrc = img + (long long)c * DG_A_BYTES;
  const char* const zero16 = img + (long long)wn_dgrad_chunks(n) * DG_A_BYTES;   // 16 bytes of zeros behind the last chunk
  const float* xb = dg_b + (long long)(16 * c) * L;
  const int c_count = min(16, 2 * n - 16 * c);
  const int w4 = (t0 - dil) & ~3;                        // 16-byte aligned start of the window (first column any tap needs)
  const int NI = DG_A_BLOCKS * 2 + 2 * nblkw;            // 1-KiB pieces per stage
  for (int idx = wave_s; idx < NI; idx += 8) {           // wave-uniform trip count
    if (idx < 2 * DG_A_BLOCKS) {
      lds_dma16(asrc + idx * 1024 + lane * 16, sl + idx * 1024);
    } else {
      const int bi = idx - 2 * DG_A_BLOCKS;
      const int gq = bi >= nblkw ? 1 : 0, m = bi - gq * nblkw;
      const int row = 8 * gq + (lane >> 3);
      const int t = w4 + 32 * m + 4 * (lane & 7);
      const bool ok = row < c_count && t >= 0 && t < L;
      const char* src = ok ? reinterpret_cast<const char*>(xb + ((long long)row * L + t)) : zero16;
      lds_dma16(src, sl + DG_A_BYTES + gq * gsw + m * 1024);
    }
  }
}

// The three taps of one landed stage (ring slot at base) into a wave's accumulators: per tap this wave's DG_NCB column blocks of
// the tap's window — the fragment of a weight block is read from LDS once and multiplied against all of them (LDS reads,
// 128 B/clk/CU, bound the one-column-block form of this loop).  sub = (t0 - dil) & 3, the window's sub-piece column offset.
__device__ __forceinline__ void wn_dgrad_stage(f32x16 (&acc)[5][DG_NCB], const char* base, int gsw, int wave_n0, int dil, int sub,
                                               int lane) {
  const int half = lane >> 5, l31 = lane & 31;
#pragma unroll
  for (int tap = 0; tap < 3; ++tap) {
    bf16x8 bh[DG_NCB], bl[DG_NCB];
#pragma unroll
    for (int cb = 0; cb < DG_NCB; ++cb) {
      const int colx = wave_n0 + 32 * cb + l31 + (2 - tap) * dil + sub;
      const char* bp = base + DG_A_BYTES + half * gsw + (colx >> 5) * 1024 + (colx & 31) * 4;
      float v8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v8[j] = *reinterpret_cast<const float*>(bp + j * 128);
      split_bf16x8(v8, bh[cb], bl[cb]);
    }
    const char* ab = base + (tap == 0 ? 0 : (tap == 1 ? 4 : 9)) * 2048;
#pragma unroll
    for (int mb = 0; mb < 5; ++mb) {
      if (mb == 4 && tap != 1) continue;               // the d_u0 block exists on the centre tap only
      bf16x8 ah, al;
      lds_read_a_frag(ab, mb, lane, ah, al);
#pragma unroll
      for (int cb = 0; cb < DG_NCB; ++cb) mfma_bf3(acc[mb][cb], ah, al, bh[cb], bl[cb]);
    }
  }
}

struct WnDgradParams {
  const float* dg;      // [B][2n][L]
  const char* img;
  const float* d_a;     // [B][n][L] residual cotangent, or null
  float* d_a_new;       // [B][n][L]
  float* d_u0;          // [B][h][L] with batch stride d_u0_bs (a channel slice of a wider tensor passes as it is), accumulated
  long long d_u0_bs;
  float* row_sums;      // optional [128][n_wg]: per-workgroup Σ_t d_a_new[row] — the res rows of the next res_skip bias gradient
  int B, L, n, h, dil, CHK, tiles_per_seq, n_wg;
  int nblkw;            // 32-sample column blocks of the window
  int gsw;              // bytes per 8-channel row group of the window
  int slot;             // bytes per ring slot
  int ns;               // ring slots (with DG_TN = 512 always 2: three never fit the LDS)
};

template <int N>
__device__ __forceinline__ void wn_wait_sw(int n) {
  // counted wait for a wave-uniform run-time count (the immediates are instantiated below)
  if (n == N) { wait_vmcnt<N>(); return; }
  if constexpr (N > 0) wn_wait_sw<N - 1>(n);
}

__global__ __launch_bounds__(512, 2) void wn_layer_dgrad_kernel(WnDgradParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  char* const ldsb = reinterpret_cast<char*>(lds);
  const int tid = threadIdx.x, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_n0 = wave_s * (32 * DG_NCB);
  const int L = p.L, n = p.n, CHK = p.CHK, dil = p.dil;
  const int NI = DG_A_BLOCKS * 2 + 2 * p.nblkw;        // 1-KiB pieces per stage
  const int my_pieces = (NI - wave_s + 7) >> 3;        // pieces idx = wave + 8 i < NI
  const int depth = p.ns - 1;                          // stages in flight

  // Workgroups are persistent: the launch has one per CU (the ring leaves room for one) and workgroup j walks the virtual
  // ids j, j + gridDim, ...  Ids that differ by a multiple of 8 share an XCD (round-robin dispatch), so each XCD gets a
  // contiguous run of tiles — the tiles of one sequence, which re-read each other's halo, meet in one L2.
  auto tile_of = [&](int v, int& b, int& t0) {
    int wg = v;
    if ((p.n_wg & 7) == 0) wg = (wg & 7) * (p.n_wg >> 3) + (wg >> 3);
    b = wg / p.tiles_per_seq;
    t0 = (wg - b * p.tiles_per_seq) * DG_TN;
    return wg;
  };
  auto issue = [&](int b, int t0, int c, int slot) {
    wn_dgrad_issue(ldsb + slot * p.slot, p.img, p.dg + (long long)b * (2 * n) * L, c, t0, n, L, dil, p.nblkw, p.gsw, wave_s, lane);
  };

  // The epilogue's transpose tiles and row-sum array live in ring slot 0; a tile whose predecessor's epilogue is still
  // running starts its ring at slot 1, so its first stages stream in underneath that epilogue.
  int first_slot = 0;
  for (int v = blockIdx.x; v < p.n_wg; v += gridDim.x) {
    int b, t0;
    const int wg = tile_of(v, b, t0);
    const int sub = (t0 - dil) & 3;
    // accumulators start as the tensors the products are added to: d_a rows of block i (if a residual cotangent comes
    // in), then the d_u0 rows (accumulated in place)
    f32x16 acc[5][DG_NCB];
#pragma unroll
    for (int mb = 0; mb < 5; ++mb)
#pragma unroll
      for (int cb = 0; cb < DG_NCB; ++cb) {
        const float* src = mb < 4 ? (p.d_a ? p.d_a + ((long long)b * n + mb * 32) * L : nullptr) : p.d_u0 + (long long)b * p.d_u0_bs;
        const int rows = mb < 4 ? (p.d_a ? n - mb * 32 : 0) : p.h;
        wn_acc_load(acc[mb][cb], src, rows, L, t0 + wave_n0 + 32 * cb, lane);
      }
    // first tile: the ring is primed AFTER the operand loads, which are then older than every LDS-DMA piece and covered by
    // the counted waits as they stand (a later tile's ring was primed under its predecessor's epilogue: its first wait
    // also waits for these loads — vmcnt retires in order — which is merely conservative)
    if (first_slot == 0)
      for (int d = 0; d < depth && d < CHK; ++d) issue(b, t0, d, d);

    int slot = first_slot;
    for (int c = 0; c < CHK; ++c) {
      // stages still allowed in flight behind stage c: those already issued, i.e. min(depth - 1, CHK - 1 - c).  (After a
      // predecessor tile the epilogue's own stores may still be in flight and count too: they are NEWER than the stage
      // waited for, so the count is merely conservative — vmcnt retires in issue order.)
      const int newer = min(depth - 1, CHK - 1 - c);
      wn_wait_sw<16>(newer * my_pieces);
      __builtin_amdgcn_s_barrier();
      if (c + depth < CHK) issue(b, t0, c + depth, (slot + depth) % p.ns);
      wn_dgrad_stage(acc, ldsb + slot * p.slot, p.gsw, wave_n0, dil, sub, lane);
      slot = slot + 1 == p.ns ? 0 : slot + 1;
    }
    __syncthreads();                                     // every wave is past its last fragment read: the ring is free
    // the next tile's first stages go into slots 1.. while this tile's epilogue works in slot 0
    if (v + (int)gridDim.x < p.n_wg) {
      int bn, tn;
      tile_of(v + gridDim.x, bn, tn);
      for (int d = 0; d < depth && d < CHK; ++d) issue(bn, tn, d, 1 + d);
      first_slot = 1;
    }
    float* const tile = reinterpret_cast<float*>(ldsb + wave_s * WN_TILE_BYTES);
    float* const rsum = reinterpret_cast<float*>(ldsb + 8 * WN_TILE_BYTES);      // [8 waves][128]
    float* const rsum_w = rsum + wave_s * 128;
    if (p.row_sums) {
      rsum[tid] = 0.f; rsum[512 + tid] = 0.f;
      __syncthreads();
    }
    // 5 × DG_NCB tiles straight from the accumulators; the bias-gradient row sums (when asked for) go through the
    // wave's transpose tile
#pragma unroll
    for (int k = 0; k < 5 * DG_NCB; ++k) {
      const int i = k / DG_NCB, cb = k % DG_NCB, tcol = t0 + wave_n0 + 32 * cb;
      float* dst = i < 4 ? p.d_a_new + ((long long)b * n + i * 32) * L : p.d_u0 + (long long)b * p.d_u0_bs;
      const int rows = i < 4 ? n - i * 32 : p.h;
      wn_acc_store(acc[i][cb], dst, rows, L, tcol, lane);
      if (p.row_sums && i < 4) {
#pragma unroll
        for (int r = 0; r < 16; ++r) tile[((r & 3) + 8 * (r >> 2) + 4 * half) * 36 + l31] = acc[i][cb][r];
        wn_tile_row_sums(tile, rsum_w, i * 32, rows, L, tcol, lane);
      }
    }
    if (p.row_sums) wn_reduce_row_sums(rsum, 128, p.row_sums, p.n_wg, wg, tid);       // [128][n_wg]
  }
}

// window geometry of one fst_wn_layer_dgrad stage at dilation dil: (32-sample blocks per window, bytes per window, bytes per ring slot)
static inline void wn_dgrad_geometry(int dil, int* nblkw, int* gsw, int* slot) {
  *nblkw = (DG_TN + 2 * dil + 3 + 31) / 32;
  *gsw = *nblkw * 1024 + 128;
  *slot = DG_A_BYTES + 2 * *gsw;
}

// 1 when fst_wn_layer_dgrad serves (n, h, dil): two ring slots fit the 160 KiB of LDS (with 512-sample tiles: up to dilation
// 128, i.e. WN stacks of up to 8 layers); the host side falls back to the generic data-gradient launch otherwise.
extern "C" int fst_wn_dgrad_fits(int n, int h, int dil) {
  if (!(n > 0 && n <= 128 && h > 0 && h <= 32 && dil > 0)) return 0;
  int nblkw, gsw, slot;
  wn_dgrad_geometry(dil, &nblkw, &gsw, &slot);
  return 2 * slot <= 160 * 1024 ? 1 : 0;
}

extern "C" int fst_wn_layer_dgrad(const float* dg, const void* image, int64_t image_bytes, const float* d_a, float* d_a_new,
                                  float* d_u0, float* row_sums, int64_t row_sums_rows, int B, int L, int n, int h, int dil,
                                  int64_t numel_a, int64_t d_u0_bs, void* stream) {
  fst_wn_clear_route();
  FST_REQUIRE(dg && image && d_a_new && d_u0, "fst_wn_layer_dgrad: null operand");
  FST_REQUIRE(B > 0 && L > 0 && n > 0 && n <= 128 && h > 0 && h <= 32 && dil > 0, "fst_wn_layer_dgrad: B=%d L=%d n=%d h=%d dil=%d", B, L,
              n, h, dil);
  FST_REQUIRE((long long)B * n * L == (long long)numel_a,
              "fst_wn_layer_dgrad: B*n*L does not match the element count %lld of the [B][n][L] tensors", (long long)numel_a);
  FST_REQUIRE(d_u0_bs >= (int64_t)h * L && d_u0_bs % 4 == 0,
              "fst_wn_layer_dgrad: d_u0 batch stride %lld (needs >= h*L = %lld and a multiple of 4)", (long long)d_u0_bs, (long long)h * L);
  FST_REQUIRE(image_bytes == fst_wn_dgrad_image_bytes(n), "fst_wn_layer_dgrad: image is %lld bytes, expected %lld",
              (long long)image_bytes, (long long)fst_wn_dgrad_image_bytes(n));
  FST_REQUIRE(L % 4 == 0 && fst_aligned16(dg) && fst_aligned16(image) && fst_aligned16(d_a) && fst_aligned16(d_a_new) && fst_aligned16(d_u0),
              "fst_wn_layer_dgrad: needs L %% 4 == 0 and 16-byte aligned tensors (L=%d)", L);
  WnDgradParams p;
  p.dg = dg; p.img = static_cast<const char*>(image); p.d_a = d_a; p.d_a_new = d_a_new; p.d_u0 = d_u0; p.d_u0_bs = d_u0_bs;
  p.row_sums = row_sums;
  p.B = B; p.L = L; p.n = n; p.h = h; p.dil = dil; p.CHK = wn_dgrad_chunks(n);
  p.tiles_per_seq = (L + DG_TN - 1) / DG_TN;
  p.n_wg = B * p.tiles_per_seq;
  FST_REQUIRE(row_sums == nullptr || row_sums_rows == p.n_wg, "fst_wn_layer_dgrad: row_sums has %lld rows, the launch has %d "
              "workgroups (B x ceil(L/512))", (long long)row_sums_rows, p.n_wg);
  wn_dgrad_geometry(dil, &p.nblkw, &p.gsw, &p.slot);
  p.ns = 2;
  FST_REQUIRE(2 * p.slot <= 160 * 1024, "fst_wn_layer_dgrad: dilation %d needs a %d-byte window slot: too large for LDS", dil, p.slot);
  size_t lds_bytes = (size_t)p.ns * p.slot;
  if (lds_bytes < 8 * WN_TILE_BYTES + 4096) lds_bytes = 8 * WN_TILE_BYTES + 4096;   // tiles + the per-wave row-sum arrays
  if (int rc = fst_allow_full_lds((const void*)wn_layer_dgrad_kernel, "fst_wn_layer_dgrad")) return rc;
  // one persistent workgroup per CU (two rings do not fit one)
  int grid = p.n_wg;
  const int cus = fst_cu_count();
  if (cus > 0 && grid > cus && (size_t)2 * lds_bytes > 160 * 1024) grid = cus;
  fst_wn_set_route(FST_WN_ROUTE_LAYER_DGRAD, 0, 0, 0, 0, grid, 1, 1, p.tiles_per_seq, p.ns, 1, (int)lds_bytes);
  hipLaunchKernelGGL(wn_layer_dgrad_kernel, dim3((unsigned)grid), dim3(512), lds_bytes, (hipStream_t)stream, p);
  FST_LAUNCH_CHECK();
  return 0;
}

// Row sums of an accumulator tile WITHOUT an LDS transpose (the persistent kernel's LDS holds a layer's weights): a lane holds
// 16 rows x 1 column; a halving butterfly over the 32 lanes of a half — at distance 16 a lane keeps registers 0-7 (bit 4 clear)
// or 8-15 and adds the partner's copy of the same registers, at distance 8 four of those eight, ... — leaves every lane with ONE
// row's total after 8 + 4 + 2 + 1 exchanges, one more at distance 1 completes it: 16 exchanges per tile instead of 80.
// Lane l31 (even) of half hh ends with row (j&3) + 8(j>>2) + 4hh, j = 8·bit4 + 4·bit3 + 2·bit2 + bit1 of l31; it adds the total
// to ITS entry of the wave's row array (plain read-modify-write in program order: the same sum in every run).
__device__ __forceinline__ void ws_row_sums(const float (&v)[16], float* rows_w, int row0, int rows_valid, bool col_ok, int lane) {
  const int l31 = lane & 31, half = lane >> 5;
  float a8[8], a4[4], a2[2];
  const bool b4 = (l31 & 16) != 0, b3 = (l31 & 8) != 0, b2 = (l31 & 4) != 0, b1 = (l31 & 2) != 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float lo = col_ok ? v[j] : 0.f, hi = col_ok ? v[8 + j] : 0.f;
    a8[j] = (b4 ? hi : lo) + __shfl_xor(b4 ? lo : hi, 16, 64);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) a4[j] = (b3 ? a8[4 + j] : a8[j]) + __shfl_xor(b3 ? a8[j] : a8[4 + j], 8, 64);
#pragma unroll
  for (int j = 0; j < 2; ++j) a2[j] = (b2 ? a4[2 + j] : a4[j]) + __shfl_xor(b2 ? a4[j] : a4[2 + j], 4, 64);
  float a1 = (b1 ? a2[1] : a2[0]) + __shfl_xor(b1 ? a2[0] : a2[1], 2, 64);
  a1 += __shfl_xor(a1, 1, 64);
  const int j = (b4 ? 8 : 0) + (b3 ? 4 : 0) + (b2 ? 2 : 0) + (b1 ? 1 : 0);
  const int row = (j & 3) + 8 * (j >> 2) + 4 * half;
  if ((l31 & 1) == 0 && row < rows_valid) rows_w[row0 + row] += a1;
}

// ------------------------------------------------------------------------------------------------
// The whole backward of a WN stack in ONE persistent launch (sequences of up to 512 samples)
//
// fst_wn_layer_bwd + fst_wn_layer_dgrad, per layer, are two launches whose every workgroup walks the same phases at the same
// time — operand loads, the GEMM, stores — and d_a / dg / d_u0 make a round trip through the memory fabric at every launch
// boundary: 660 MB per layer at B=256, L=512 (counters: profiles/r04_stack_*), which is what bounds them.  With L <= 512 a
// 512-sample tile IS a whole sequence: the dilated taps never look outside the tile, so the chain
//     dacts = W_rsᵀ·[d_a ; d_out]  →  dg = gate'(t, s)·dacts  →  d_a += W_inᵀ (*) dg,  d_u0 += W_condᵀ·dg        (layer nl−1 … 0)
// of one batch element depends on nothing another workgroup produces.  One workgroup (8 waves × 64 samples) therefore walks
// all layers of its batch element and d_a NEVER LEAVES ITS ACCUMULATORS: phase B (the data gradient) accumulates into them,
// phase A (res_skip / gate backward) multiplies straight out of them — an accumulator tile is, register for register, the B
// operand of an MFMA that sums over its rows; the weight image holds the d_a stages in that k-order (fst_wn_pack_bwd,
// acc_order) — and d_a is stored only where something outside reads it (layer 0: the start conv; every layer in the full
// pass: the res_skip weight gradients).  That takes the three d_a passes (189 of the 660 MB) off the fabric, the launch
// boundaries (2 per layer) are gone, and — nothing synchronising the workgroups with each other — the CUs drift apart, so one
// CU's load / store phases run under other CUs' GEMM phases.  In GradNorm's partial passes (no weight gradients) dg lives in a
// scratch tensor that is rewritten layer after layer.
//
// Phase A runs as TWO column passes (the wave's two 32-sample column blocks one after the other): d_a occupies 128 registers,
// so the dacts accumulators get 64 (4 row blocks × 1 column block).  Per pass: the skip stages (the operand straight from
// memory in fragment layout, the weights from the layer's resident image), then the d_a stages (the operand from the
// accumulators), then the gate on four tiles.
//
// The skip operand is d_out [B][n][L] against W_skip,iᵀ (fst_wn_stack_bwd: SR = n rows, SCH = CH stages) or — the form
// GradNorm's partial passes run — the end conv's cotangent do [B][2h][L] against (W_end·W_skip,i)ᵀ (fst_wn_stack_bwd_proj, images of
// fst_wn_pack_bwd_proj_stack: SR = 2h, SCH = ceil(2h/16)): d_out = W_endᵀ·do has rank 2h, so every wave re-reading its n-channel
// slice of it in every layer moved n/2h times the bytes the result needs (62.9 vs 26.2 MB per layer at n = 120, h = 25, B = 256,
// L = 512), and the pass took CH MFMA stages where ceil(2h/16) do.  One kernel, two row / stage counts in its arguments.  Phase B = the body of
// wn_layer_dgrad_kernel.  Global stores of one phase (dg, d_u0) are read by the next through LDS-DMA / loads of the SAME
// workgroup: s_waitcnt vmcnt(0) by every wave + a workgroup barrier orders them (one CU, one L1).
// ------------------------------------------------------------------------------------------------
#define WS_TN 512
#define WS_NB 8                                    // 32-sample column blocks of a phase-A window row group: one per wave and column pass
#define WS_GS (WS_NB * 1024 + 128)
#define WS_SLOT_A (WN_BW_A + 2 * WS_GS)
#define WS_LDS_A (16 * WN_BW_A)                     // a layer's resident W_rsᵀ image: up to 16 stages (n <= 128) of 8 KiB

struct WnStackParams {
  const float* ts[WS_MAXL];      // saved gate halves [B][2n][L] per layer
  const char* img_b[WS_MAXL];    // fst_wn_pack_bwd images (acc_order = 1)
  const char* img_d[WS_MAXL];    // fst_wn_pack_dgrad images
  float* dg[WS_MAXL];            // [B][2n][L] per layer (partial passes: one scratch tensor for all)
  float* da_out[WS_MAXL];        // cotangent of the layer's input [B][n][L]: written when not null (layer 0: always)
  float* rs_b[WS_MAXL];          // optional [256][B]: per-sequence Σ_t dg[row]
  float* rs_d[WS_MAXL];          // optional [128][B]: per-sequence Σ_t da_out[row]
  const float* d_out;            // the skip operand [B][SR][L]: d_out (SR = n), or the end conv's cotangent do (SR = 2h: the projected form)
  float* d_u0;                   // [B][h][L] with batch stride d_u0_bs, accumulated in place
  long long d_u0_bs;
  int dil[WS_MAXL], nblkw[WS_MAXL], gsw[WS_MAXL], slot_d[WS_MAXL];
  int nl, B, L, n, h, CH, CHK;
  int SR, SCH;                   // rows of the skip operand and its stages in the image: n, CH — or 2h, ceil(2h/16) (fst_wn_pack_bwd_proj_stack)
};

__global__ __launch_bounds__(512, 2) void wn_stack_bwd_kernel(WnStackParams p_by_value) {
  // The per-layer tables are indexed with a run-time layer number: read through the kernarg segment they are scalar loads at a
  // computed offset; indexing the by-value struct would make the compiler copy it to scratch (1 KiB per lane) or keep all of
  // it in SGPRs (639 spilled).
  const auto& p = *(const __attribute__((address_space(4))) WnStackParams*)__builtin_amdgcn_kernarg_segment_ptr();
  (void)p_by_value;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  char* const ldsb = reinterpret_cast<char*>(lds);
  const int tid = threadIdx.x, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_n0 = wave_s * 64;
  const int L = p.L, n = p.n, CH = p.CH, CHK = p.CHK;
  // phase A's LDS: [the layer's whole W_rsᵀ image, resident for both column passes: up to 16 x 8 KiB][the row-sum arrays] — the
  // next layer's image streams in while a phase-B epilogue is still adding row sums
  float* const rsum = reinterpret_cast<float*>(ldsb + WS_LDS_A);        // [8 waves][256]
  float* const rsum_w = rsum + wave_s * 256;
  const unsigned vlane = (unsigned)(4 * half * L + l31) * 4u;
  const WsLane wl0 = ws_lane(vlane, wave_n0, L, lane), wl1 = ws_lane(vlane, wave_n0 + 32, L, lane);

  // layer i's W_rsᵀ image ([d_a stages][skip stages]; the top layer: skip stages only): one 1-KiB piece per wave and stage
  auto issue_res = [&](int i) {
    const int S3 = wn_bwd_proj_stages(CH, p.SCH, i == p.nl - 1);
    const char* const img = p.img_b[i];
    for (int c = 0; c < S3; ++c)
      lds_dma16(img + (long long)c * WN_BW_A + wave_s * 1024 + lane * 16, ldsb + c * WN_BW_A + wave_s * 1024);
  };
  // per-lane byte offset of a B-fragment element of a [channel][time] matrix read straight from memory: lane half hh reads
  // channels 8hh + j of a 16-channel chunk at column l31 of its block
  const unsigned vfrag = (unsigned)(8 * half * L + l31) * 4u;

  FST_SUMS(12);
  FST_T(tw0);
  bool primed = false;                                     // the weight image of the layer at hand is already in flight
  for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
    // acc[0..3] = the cotangent of the residual stream (d_a), carried from layer to layer; acc[4] = the conditioning rows (d_u0)
    f32x16 acc[5][2];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mb][cb][r] = 0.f;     // the top layer has no residual output
    for (int i = p.nl - 1; i >= 0; --i) {
      const bool last = i == p.nl - 1;
      // ============================================================ phase A: dg = gate'(t, s) · W_rsᵀ·[d_a ; d_out]
      {
        // the tanh | sigmoid halves are two [n][L] matrices
        const __amdgpu_buffer_rsrc_t ts_t = ws_rsrc(p.ts[i] + (long long)b * (2 * n) * L);
        const __amdgpu_buffer_rsrc_t ts_s = ws_rsrc(p.ts[i] + ((long long)b * 2 + 1) * n * L);
        const __amdgpu_buffer_rsrc_t dg_t = ws_rsrc(p.dg[i] + (long long)b * (2 * n) * L);
        const __amdgpu_buffer_rsrc_t dg_s = ws_rsrc(p.dg[i] + ((long long)b * 2 + 1) * n * L);
        const __amdgpu_buffer_rsrc_t dout_r = ws_rsrc(p.d_out + (long long)b * p.SR * L);
        float* const rs_out = p.rs_b[i];
        FST_T(ta0);
        if (!primed) issue_res(i);
        primed = false;
        if (rs_out) {
#pragma unroll
          for (int w = 0; w < 4; ++w) rsum[w * 512 + tid] = 0.f;
        }
        wait_vmcnt<0>();                                     // this wave's pieces of the image have landed ...
        __syncthreads();                                     // ... and everyone's; the row-sum arrays are zeroed
        FST_T(ta1);
        FST_ACC(0, ta0, ta1);                            // phase A: waiting for the weight image
        const char* const w_dout = ldsb + (long long)(last ? 0 : CH) * WN_BW_A;
        auto run_pass = [&](auto pc) {
          constexpr int cb = decltype(pc)::value;
          const WsLane wl = cb ? wl1 : wl0;
          const int tcol = wave_n0 + 32 * cb;
          f32x16 da[4];                                    // dacts rows of this column block
#pragma unroll
          for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) da[mb][r] = 0.f;
          FST_T(tp0);
          // ---- the skip stages (d_out, or do against the projected image): the operand comes straight from memory in fragment
          // layout (eight dword loads per stage: lane half hh reads channels 8hh + j at its column), the next stage's in flight while one is multiplied — no ring, no barrier
          const unsigned vf = tcol + l31 < L ? vfrag : WS_OOB, vf_lo = half == 0 ? vf : WS_OOB;
          auto load_dout = [&](float (&v)[8], int c) {
            const int Lq = ws_opaque(L), nq = ws_opaque(p.SR);
            const int sbase = (16 * c * Lq + tcol) * 4;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              float x = 0.f;
              if (16 * c + j < nq)
                x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dout_r, 16 * c + 8 + j < nq ? vf : vf_lo, sbase + j * Lq * 4, 0));
              v[j] = x;
            }
          };
          float vn[8];
          load_dout(vn, 0);
          const int SCH = p.SCH;
          for (int k = 0; k < SCH; ++k) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = vn[j];
            if (k + 1 < SCH) load_dout(vn, k + 1);
            bf16x8 bh, bl;
            split_bf16x8(v, bh, bl);
            wn_bwd_multiply(da, w_dout + k * WN_BW_A, lane, bh, bl);
          }
          // ---- the d_a stages: the operand IS the accumulator tile (registers 8s..8s+7 of row block c>>1 are k-step c&1)
          if (!last) {
            auto da_stage = [&](auto cc) {
              constexpr int c = decltype(cc)::value;
              if (c < CH) {                                // wave-uniform
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = acc[c >> 1][cb][8 * (c & 1) + j];
                bf16x8 bh, bl;
                split_bf16x8(v, bh, bl);
                wn_bwd_multiply(da, ldsb + c * WN_BW_A, lane, bh, bl);
                __builtin_amdgcn_sched_barrier(0);        // stage by stage: hoisted fragment reads of later stages cost registers
              }
            };
            da_stage(std::integral_constant<int, 0>{}); da_stage(std::integral_constant<int, 1>{});
            da_stage(std::integral_constant<int, 2>{}); da_stage(std::integral_constant<int, 3>{});
            da_stage(std::integral_constant<int, 4>{}); da_stage(std::integral_constant<int, 5>{});
            da_stage(std::integral_constant<int, 6>{}); da_stage(std::integral_constant<int, 7>{});
          }
          FST_T(tp1);
          FST_ACC(1, tp0, tp1);                          // phase A: GEMM stages of a pass
          // ---- gate: four tiles (row blocks) of this column block
#pragma unroll
          for (int blk = 0; blk < 4; ++blk) {
            const int rows_valid = n - blk * 32;
            f32x16 tv, sv;
            ws_acc_load(tv, ts_t, wl, blk * 32, tcol, rows_valid, L);
            ws_acc_load(sv, ts_s, wl, blk * 32, tcol, rows_valid, L);
            float gt[16], gs[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float d = da[blk][r], t = tv[r], s2 = sv[r];
              gt[r] = d * s2 * (1.f - t * t);
              gs[r] = d * t * s2 * (1.f - s2);
            }
            ws_acc_store(gt, dg_t, wl, blk * 32, tcol, rows_valid, L);
            ws_acc_store(gs, dg_s, wl, blk * 32, tcol, rows_valid, L);
            if (rs_out) {
              ws_row_sums(gt, rsum_w, blk * 32, rows_valid, tcol + l31 < L, lane);
              ws_row_sums(gs, rsum_w, n + blk * 32, rows_valid, tcol + l31 < L, lane);
            }
            __builtin_amdgcn_sched_barrier(0);            // tile by tile (a scheduler that hoists the loads of later tiles runs out of registers)
          }
          FST_T(tp2);
          FST_ACC(2, tp1, tp2);                          // phase A: gate epilogue of a pass
        };
        run_pass(std::integral_constant<int, 0>{});
        run_pass(std::integral_constant<int, 1>{});
        if (rs_out) wn_reduce_row_sums(rsum, 256, rs_out, p.B, b, tid);       // [256][B]
        FST_T(ta3);
        wait_vmcnt<0>();                                     // this wave's dg stores have reached L2 ...
        __syncthreads();                                     // ... and so have everyone's: phase B may fetch them; the ring is free
        FST_T(ta4);
        FST_ACC(3, ta3, ta4);                            // phase A -> B: store drain + barrier
      }
      // ============================================================ phase B: d_a += W_inᵀ (*) dg,  d_u0 += W_condᵀ·dg
      {
        const int dil = p.dil[i], nblkw = p.nblkw[i], gsw = p.gsw[i], slotb = p.slot_d[i];
        const char* const img = p.img_d[i];
        const float* const dgr = p.dg[i] + (long long)b * (2 * n) * L;
        float* const da_store = p.da_out[i];
        const __amdgpu_buffer_rsrc_t dan_r = ws_rsrc(da_store ? da_store + (long long)b * n * L : nullptr);
        const __amdgpu_buffer_rsrc_t du_r = ws_rsrc(p.d_u0 + (long long)b * p.d_u0_bs);
        float* const rs_out = p.rs_d[i];
        const int sub = (0 - dil) & 3;                       // a 512-sample tile is the whole sequence: t0 = 0
        auto issue = [&](int c, int slot) { wn_dgrad_issue(ldsb + slot * slotb, img, dgr, c, 0, n, L, dil, nblkw, gsw, wave_s, lane); };
        FST_T(tb0);
        // the d_a tiles are where the previous layer left them; the conditioning rows come from memory
        ws_acc_load(acc[4][0], du_r, wl0, 0, wave_n0, p.h, L);
        ws_acc_load(acc[4][1], du_r, wl1, 0, wave_n0 + 32, p.h, L);
        asm volatile("" ::: "memory");
        issue(0, 0);                                         // two ring slots: one stage in flight while one is multiplied
        int slot = 0;
        FST_T(tb1);
        FST_ACC(4, tb0, tb1);                            // phase B: conditioning-row loads + first stage (issue)
        for (int c = 0; c < CHK; ++c) {
          wait_vmcnt<0>();
          __builtin_amdgcn_s_barrier();
          if (c + 1 < CHK) issue(c + 1, slot ^ 1);
          wn_dgrad_stage(acc, ldsb + slot * slotb, gsw, wave_n0, dil, sub, lane);
          slot ^= 1;
        }
        FST_T(tb2);
        FST_ACC(5, tb1, tb2);                            // phase B: GEMM loop
        __syncthreads();                                     // every wave is past its last fragment read: the ring is free
        // the weight image of the next phase A (the layer below, or the top layer of this workgroup's next sequence) depends on
        // nothing this phase stores: it streams into LDS now, under the stores below
        {
          const int ni = i > 0 ? i - 1 : p.nl - 1, nb = i > 0 ? b : b + (int)gridDim.x;
          if (nb < p.B) {
            issue_res(ni);
            primed = true;
          }
        }
        if (rs_out) {
          rsum[tid] = 0.f; rsum[512 + tid] = 0.f;
          __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < 5 * DG_NCB; ++k) {
          const int ib = k / DG_NCB, cb = k % DG_NCB, tcol = wave_n0 + 32 * cb;
          const int rows = ib < 4 ? n - ib * 32 : p.h;
          if (ib < 4) {
            if (da_store) ws_acc_store(acc[ib][cb], dan_r, cb ? wl1 : wl0, ib * 32, tcol, rows, L);
          } else {
            ws_acc_store(acc[ib][cb], du_r, cb ? wl1 : wl0, 0, tcol, rows, L);
          }
          if (rs_out && ib < 4) {
            float av[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) av[r] = acc[ib][cb][r];
            ws_row_sums(av, rsum + wave_s * 128, ib * 32, rows, tcol + l31 < L, lane);
          }
        }
        if (rs_out) wn_reduce_row_sums(rsum, 128, rs_out, p.B, b, tid);       // [128][B]
        FST_T(tb3);
        FST_ACC(6, tb2, tb3);                            // phase B: epilogue stores (issue)
        // d_u0 of this layer must be in L2 before the next layer's phase B reads it back (the wait also retires the primed stages)
        wait_vmcnt<0>();
        __syncthreads();
        FST_T(tb4);
        FST_ACC(7, tb3, tb4);                            // phase B -> A: store drain + barrier
      }
    }
  }
  FST_T(tw1);
  FST_ACC(9, tw0, tw1);
  FST_FLUSH(wn_stamps);
}

// 1 when fst_wn_stack_bwd serves a WN stack of nl layers on sequences of L samples (dilations 1, 2, 4, ... as the reference's WN)
extern "C" int fst_wn_stack_bwd_ok(int n, int h, int L, int nl) {
  if (!(n > 0 && n <= 128 && h > 0 && h <= 32 && L > 0 && L <= WS_TN && L % 4 == 0 && nl > 0 && nl <= WS_MAXL)) return 0;
  for (int i = 0; i < nl; ++i)
    if (i >= 20 || !fst_wn_dgrad_fits(n, h, 1 << i)) return 0;
  return 1;
}

// the launch behind fst_wn_stack_bwd (skip = d_out: rows = n) and fst_wn_stack_bwd_proj (skip = do: rows = 2h)
static int wn_stack_bwd_launch(const char* who, const float* const* ts, const void* const* img_b, const void* const* img_d,
                               float* const* dg, float* const* da_out, float* const* rs_b, float* const* rs_d, const float* skip,
                               int skip_rows, float* d_u0, int64_t d_u0_bs, int nl, int B, int L, int n, int h, int64_t numel_a,
                               void* stream) {
  FST_REQUIRE(ts && img_b && img_d && dg && da_out && skip && d_u0, "%s: null table", who);
  FST_REQUIRE(fst_wn_stack_bwd_ok(n, h, L, nl), "%s: not served: n=%d h=%d L=%d nl=%d (needs n <= 128, h <= 32, "
              "L <= 512, L %% 4 == 0, nl <= %d)", who, n, h, L, nl, WS_MAXL);
  FST_REQUIRE(B > 0 && (long long)B * n * L == (long long)numel_a,
              "%s: B*n*L does not match the element count %lld of the [B][n][L] tensors", who, (long long)numel_a);
  FST_REQUIRE(d_u0_bs >= (int64_t)h * L && d_u0_bs % 4 == 0,
              "%s: d_u0 batch stride %lld (needs >= h*L = %lld and a multiple of 4)", who, (long long)d_u0_bs, (long long)h * L);
  FST_REQUIRE((rs_b == nullptr) == (rs_d == nullptr), "%s: row sums of both kinds or of neither", who);
  WnStackParams p = {};
  size_t lds_bytes = WS_LDS_A + 8192;                                // phase A: the weight image and the row-sum arrays
  for (int i = 0; i < nl; ++i) {
    FST_REQUIRE(ts[i] && img_b[i] && img_d[i] && dg[i] && (i > 0 || da_out[i]), "%s: null operand of layer %d", who, i);
    FST_REQUIRE(fst_aligned16(ts[i]) && fst_aligned16(img_b[i]) && fst_aligned16(img_d[i]) && fst_aligned16(dg[i]) && fst_aligned16(da_out[i]),
                "%s: operands of layer %d must be 16-byte aligned", who, i);
    p.ts[i] = ts[i]; p.img_b[i] = static_cast<const char*>(img_b[i]); p.img_d[i] = static_cast<const char*>(img_d[i]);
    p.dg[i] = dg[i]; p.da_out[i] = da_out[i];
    p.rs_b[i] = rs_b ? rs_b[i] : nullptr; p.rs_d[i] = rs_d ? rs_d[i] : nullptr;
    p.dil[i] = 1 << i;
    wn_dgrad_geometry(p.dil[i], &p.nblkw[i], &p.gsw[i], &p.slot_d[i]);
    if ((size_t)2 * p.slot_d[i] > lds_bytes) lds_bytes = (size_t)2 * p.slot_d[i];
  }
  FST_REQUIRE(fst_aligned16(skip) && fst_aligned16(d_u0), "%s: %s / d_u0 must be 16-byte aligned", who, skip_rows == n ? "d_out" : "d_o");
  FST_REQUIRE(lds_bytes <= 160 * 1024, "%s: %zu bytes of LDS", who, lds_bytes);
  p.d_out = skip; p.d_u0 = d_u0; p.d_u0_bs = d_u0_bs;
  p.nl = nl; p.B = B; p.L = L; p.n = n; p.h = h; p.CH = wn_ch(n); p.CHK = wn_dgrad_chunks(n);
  p.SR = skip_rows; p.SCH = wn_ch(skip_rows);
  FST_REQUIRE((size_t)(p.CH + p.SCH) * WN_BW_A <= WS_LDS_A, "%s: a weight image of %d stages does not fit its LDS", who, p.CH + p.SCH);
  if (int rc = fst_allow_full_lds((const void*)wn_stack_bwd_kernel, who)) return rc;
  const int cus = fst_cu_count_or(256);
  const int grid = B < cus ? B : cus;                    // one resident workgroup per CU walks its batch elements
  fst_wn_set_route(FST_WN_ROUTE_STACK_BWD, 0, 0, 0, 0, grid, 1, 1, 1, 2, nl, (int)lds_bytes);
  hipLaunchKernelGGL(wn_stack_bwd_kernel, dim3((unsigned)grid), dim3(512), lds_bytes, (hipStream_t)stream, p);
  FST_LAUNCH_CHECK();
  return 0;
}

extern "C" int fst_wn_stack_bwd(const float* const* ts, const void* const* img_b, const void* const* img_d, float* const* dg,
                                float* const* da_out, float* const* rs_b, float* const* rs_d, const float* d_out, float* d_u0,
                                int64_t d_u0_bs, int nl, int B, int L, int n, int h, int64_t numel_a, void* stream) {
  fst_wn_clear_route();
  return wn_stack_bwd_launch("fst_wn_stack_bwd", ts, img_b, img_d, dg, da_out, rs_b, rs_d, d_out, n, d_u0, d_u0_bs, nl, B, L, n, h,
                             numel_a, stream);
}

// The same launch on the end conv's cotangent: d_o [B][h2][L] in place of d_out = W_endᵀ·d_o, img_b the images of
// fst_wn_pack_bwd_proj_stack (skip stages = (W_end·W_skip,i)ᵀ).  numel_o = element count of d_o as the caller holds it.
extern "C" int fst_wn_stack_bwd_proj(const float* const* ts, const void* const* img_b, const void* const* img_d, float* const* dg,
                                     float* const* da_out, float* const* rs_b, float* const* rs_d, const float* d_o, int h2,
                                     int64_t numel_o, float* d_u0, int64_t d_u0_bs, int nl, int B, int L, int n, int h,
                                     int64_t numel_a, void* stream) {
  fst_wn_clear_route();
  FST_REQUIRE(h2 > 0 && h2 <= 64, "fst_wn_stack_bwd_proj: h2=%d (needs 0 < h2 <= 64)", h2);
  FST_REQUIRE(B > 0 && L > 0 && (long long)B * h2 * L == (long long)numel_o,
              "fst_wn_stack_bwd_proj: B*h2*L does not match the element count %lld of d_o [B][h2][L]", (long long)numel_o);
  return wn_stack_bwd_launch("fst_wn_stack_bwd_proj", ts, img_b, img_d, dg, da_out, rs_b, rs_d, d_o, h2, d_u0, d_u0_bs, nl, B, L, n, h,
                             numel_a, stream);
}
