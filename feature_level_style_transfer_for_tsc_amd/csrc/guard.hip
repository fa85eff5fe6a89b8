// Anomaly guard of the train step: decide ON THE DEVICE whether a step's update would consume a NaN or an inf, and make such a
// step a no-op on the trainer's state — with no host read, so it works inside a replayed hipGraph (the reference's only
// protection is torch.autograd.set_detect_anomaly, train_and_test.py:24, which cannot run under capture).
//
//   fst_nonfinite_multi    counts the non-finite elements of many fp32 tensors per GROUP (a tensor carries a group id < 32) and
//                          writes three device words: verdict (1 if a group of the verdict mask counted anything), ok = 1 − verdict
//                          as fp32, and a cumulative counter of skipped steps.
//   fst_guard_copy_multi   a multi-tensor copy in 4-byte words that runs unconditionally (verdict == NULL: the SAVE of state that
//                          cannot be guarded at its writer) or only when (*verdict != 0) == when (the ROLL-BACK).
//   (the optimiser updates behind the verdict word are in optim.hip, beside the update bodies they share)
//   fst_sumsq_multi        the same walk over the same tensors, adding x*x instead of counting: per-group L2 norms of the gradients,
//                          and from them and a device vector of limits the factors that clip each group and then the whole.
//   fst_scale_multi        x *= coef[group] in place, the factors read from device memory when the kernel runs: a replayed
//                          hipGraph clips by what its own scan found, and a workgroup whose factor is 1.0f touches nothing.
//   fst_ema_multi          avg = fma(w[group], live − avg, avg) over pairs of tensors: an exponential moving average of the weights
//                          whose per-group weight a one-workgroup prologue derives, when it runs, from a device decay, a warm-up
//                          count, the call's mask of active groups and the guard's verdict; w == 0 touches nothing.
//   fst_swap_multi         exchanges pairs of tensors in place (the averages into the modules' storage for evaluation, and back).
//   fst_accum_multi        folds gradients into fp32 accumulators over a window of k calls whose position j is a device word:
//                          acc = g when the window opens, acc += g after, and g = acc / k in place on the call that closes it.
//
// House style of optim.hip: the pointer tuples ride BY VALUE in the kernel arguments, at most 64 per launch, so a captured launch
// carries them (the chunks of a call, the grid of a launch and the test of an entry are fst_multi.h's); no float atomics and no
// zero fill: every workgroup of a scan writes its own slot with a plain store (and plain zeros into the slots of its tensor that
// no workgroup of this launch owns), the finalising launch adds the slots.  The counts are integers, so their sum does not depend
// on the order of the additions: the finaliser's LDS integer adds give the same words on every run.  A scan only reads its inputs.
//
// Written once each: the walk over ONE tensor in 16-byte quads with its odd ends (quad_walk: the count, the sum of squares and the
// scale are its three element functors), a scan's record in the slot array (slot_record), the walk over a PAIR of tensors
// (pair_tensor: the average, the exchange and the accumulation), and the two argument structs with their checks and fills
// (GroupArgs, PairArgs).
#include "fst_multi.h"

#define NF_REC (FST_MULTI_WG + 1)   // a tensor's record in the slot array: its group id, then the words of its FST_MULTI_WG workgroups
#define GC_GROUPS 32                // groups; norms and limits carry one more word, the total

struct GroupArgs {
  float* x[FST_MULTI_T];
  int numel[FST_MULTI_T];
  int group[FST_MULTI_T];
  int n, base;                      // tensors of this launch; index of its first tensor in the call (its record in the slot array)
};
static_assert(sizeof(GroupArgs) + sizeof(void*) <= 4096, "kernel arguments: 4 KB at most");

// NaN and ±inf are the values whose exponent bits are all ones; a test on the bits cannot be folded away by fast-math rules
__device__ __forceinline__ int nonfinite_bits(uint32_t b) { return (b & 0x7f800000u) == 0x7f800000u; }

// One workgroup's share of x[0, n) on a grid of up to FST_MULTI_WG workgroups per tensor, grid-stride beyond: 16-byte accesses
// over the aligned middle of the tensor; the up to three elements in front of the first 16-byte boundary and the up to three after
// the last full quad go to workgroup 0.  A thread hands op its elements in this order: its quads in index order, each as
// .x .y .z .w, then its head element, then its tail element (a sum that op keeps depends on it).  Op::writes: op changes the
// element, which is stored back; otherwise x is only read.
template <class Op>
__device__ __forceinline__ void quad_walk(float* __restrict__ x, int n, Op& op) {
  int head = (int)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) >> 2);
  head = head < n ? head : n;
  const int nv = (n - head) >> 2;
  const int tail0 = head + 4 * nv;
  float4* __restrict__ xv = (float4*)(x + head);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nv; i += gridDim.x * 256) {
    float4 q = xv[i];
    op(q.x); op(q.y); op(q.z); op(q.w);
    if (Op::writes) xv[i] = q;
  }
  if (blockIdx.x == 0) {
    if ((int)threadIdx.x < head) {
      float e = x[threadIdx.x];
      op(e);
      if (Op::writes) x[threadIdx.x] = e;
    }
    if ((int)threadIdx.x < n - tail0) {
      float e = x[tail0 + threadIdx.x];
      op(e);
      if (Op::writes) x[tail0 + threadIdx.x] = e;
    }
  }
}

struct CountOp {
  static constexpr bool writes = false;
  int c;
  __device__ __forceinline__ void operator()(float e) { c += nonfinite_bits(__float_as_uint(e)); }
};

// thread 0 of a scan's workgroup: the tensor's group id (workgroup 0), the workgroup's own slot, and plain zeros into the slots
// that no workgroup of this launch owns
template <class W>
__device__ __forceinline__ void slot_record(W* __restrict__ rec, int group, W total) {
  if (blockIdx.x == 0) rec[0] = (W)group;
  rec[1 + blockIdx.x] = total;
  for (int s = blockIdx.x + gridDim.x; s < FST_MULTI_WG; s += gridDim.x) rec[1 + s] = (W)0;
}

__global__ __launch_bounds__(256) void nonfinite_multi_kernel(GroupArgs a, int* __restrict__ slots) {
  const int t = blockIdx.y;
  if (t >= a.n) return;
  CountOp op{0};
  quad_walk(a.x[t], a.numel[t], op);
  __shared__ int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  if (op.c) atomicAdd(&total, op.c);                                // LDS, integer
  __syncthreads();
  if (threadIdx.x == 0) slot_record(slots + (size_t)(a.base + t) * NF_REC, a.group[t], total);
}

// one workgroup: counts[32] = per-group sums of every slot, then the three words (each may be NULL: not written)
__global__ __launch_bounds__(256) void nonfinite_finalize_kernel(const int* __restrict__ slots, int n_tensors, unsigned verdict_mask,
                                                                 int* __restrict__ counts, int* __restrict__ verdict,
                                                                 float* __restrict__ ok, int* __restrict__ skipped) {
  __shared__ int cnt[32];
  if (threadIdx.x < 32) cnt[threadIdx.x] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n_tensors * FST_MULTI_WG; i += 256) {
    const int* rec = slots + (size_t)(i / FST_MULTI_WG) * NF_REC;
    const int c = rec[1 + i % FST_MULTI_WG];
    if (c) atomicAdd(&cnt[rec[0] & 31], c);                         // LDS, integer: the sum is the same in any order
  }
  __syncthreads();
  if (threadIdx.x < 32) counts[threadIdx.x] = cnt[threadIdx.x];
  if (threadIdx.x == 0) {
    int any = 0;
    for (int g = 0; g < 32; ++g) any |= ((verdict_mask >> g) & 1u) && cnt[g] > 0;
    if (verdict) verdict[0] = any;
    if (ok) ok[0] = 1.0f - (float)any;
    if (skipped) skipped[0] += any;
  }
}

// every (tensor, count, group) entry of a call before its first launch
static int check_group_tensors(const char* who, const void* const* x_host, const int64_t* numel_host, const int32_t* group_host, int n_tensors) {
  FST_REQUIRE(n_tensors >= 0 && n_tensors < (1 << 24) && (n_tensors == 0 || (x_host && numel_host && group_host)), "%s: bad arguments", who);
  for (int i = 0; i < n_tensors; ++i) {
    FST_REQUIRE(fst_multi_entry_ok({x_host[i]}, numel_host[i], 4), "%s: tensor %d: null or misaligned pointer, or bad element count", who, i);
    FST_REQUIRE(group_host[i] >= 0 && group_host[i] < GC_GROUPS, "%s: tensor %d: group %d is not in 0..31", who, i, group_host[i]);
  }
  return 0;
}

static void fill_group(GroupArgs& a, const void* const* x_host, const int64_t* numel_host, const int32_t* group_host, int base, int n) {
  a.n = n; a.base = base;
  for (int i = 0; i < n; ++i) { a.x[i] = (float*)x_host[base + i]; a.numel[i] = (int)numel_host[base + i]; a.group[i] = group_host[base + i]; }
}

extern "C" int64_t fst_nonfinite_slots(int n_tensors) { return n_tensors < 0 ? -1 : (int64_t)n_tensors * NF_REC; }

extern "C" int fst_nonfinite_multi(const float* const* x_host, const int64_t* numel_host, const int32_t* group_host, int n_tensors,
                                   int32_t verdict_mask, int32_t* slots_dev, int64_t slots_len, int32_t* counts_dev,
                                   int32_t* verdict_dev, float* ok_dev, int32_t* skipped_dev, void* stream) {
  FST_REQUIRE(n_tensors >= 0 && n_tensors < (1 << 24) && counts_dev && (n_tensors == 0 || (x_host && numel_host && group_host && slots_dev)),
              "fst_nonfinite_multi: bad arguments");
  FST_REQUIRE(slots_len >= fst_nonfinite_slots(n_tensors), "fst_nonfinite_multi: %lld slots, %lld needed", (long long)slots_len,
              (long long)fst_nonfinite_slots(n_tensors));
  if (check_group_tensors("fst_nonfinite_multi", (const void* const*)x_host, numel_host, group_host, n_tensors)) return -1;
  if (int rc = fst_multi_chunks(n_tensors, [&](int base, int n) {
        GroupArgs a;
        fill_group(a, (const void* const*)x_host, numel_host, group_host, base, n);
        hipLaunchKernelGGL(nonfinite_multi_kernel, fst_multi_grid(numel_host + base, n), dim3(256), 0, (hipStream_t)stream, a, (int*)slots_dev);
        FST_LAUNCH_CHECK();
        return 0;
      })) return rc;
  hipLaunchKernelGGL(nonfinite_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)slots_dev, n_tensors,
                     (unsigned)verdict_mask, (int*)counts_dev, (int*)verdict_dev, ok_dev, (int*)skipped_dev);
  FST_LAUNCH_CHECK();
  return 0;
}

struct GuardCopyArgs {
  uint32_t* dst[FST_MULTI_T];
  const uint32_t* src[FST_MULTI_T];
  int words[FST_MULTI_T];
  int n;
};
static_assert(sizeof(GuardCopyArgs) + sizeof(const int*) + sizeof(int) <= 4096, "kernel arguments: 4 KB at most");

// verdict is read when the kernel runs, one uniform load per workgroup; a workgroup that is not to copy returns before its first
// load.  16-byte moves where both pointers allow, 4-byte words otherwise.
__global__ __launch_bounds__(256) void guard_copy_multi_kernel(GuardCopyArgs a, const int* __restrict__ verdict, int when) {
  const int t = blockIdx.y;
  if (t >= a.n) return;
  if (verdict && (verdict[0] != 0) != (when != 0)) return;
  uint32_t* __restrict__ d = a.dst[t];
  const uint32_t* __restrict__ s = a.src[t];
  const int n = a.words[t];
  if ((((uintptr_t)d | (uintptr_t)s) & 15u) == 0) {
    const int nv = n >> 2;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nv; i += gridDim.x * 256) ((uint4*)d)[i] = ((const uint4*)s)[i];
    if (blockIdx.x == 0 && (int)threadIdx.x < n - 4 * nv) d[4 * nv + threadIdx.x] = s[4 * nv + threadIdx.x];
    return;
  }
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) d[i] = s[i];
}

extern "C" int fst_guard_copy_multi(void* const* dst_host, const void* const* src_host, const int64_t* words_host, int n_tensors,
                                    const int32_t* verdict_dev, int when, void* stream) {
  FST_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || (dst_host && src_host && words_host)) && (when == 0 || when == 1),
              "fst_guard_copy_multi: bad arguments");
  for (int i = 0; i < n_tensors; ++i) {                              // all of them before the first launch; they may overlap
    FST_REQUIRE(fst_multi_entry_ok({dst_host[i], src_host[i]}, words_host[i], 4) && dst_host[i] != src_host[i],
                "fst_guard_copy_multi: tensor %d: null, equal or misaligned pointers, or bad word count", i);
  }
  return fst_multi_chunks(n_tensors, [&](int base, int n) {
    GuardCopyArgs a;
    a.n = n;
    for (int i = 0; i < n; ++i) {
      a.dst[i] = (uint32_t*)dst_host[base + i]; a.src[i] = (const uint32_t*)src_host[base + i]; a.words[i] = (int)words_host[base + i];
    }
    hipLaunchKernelGGL(guard_copy_multi_kernel, fst_multi_grid(words_host + base, n), dim3(256), 0, (hipStream_t)stream, a,
                       (const int*)verdict_dev, when);
    FST_LAUNCH_CHECK();
    return 0;
  });
}

// ---- gradient norms and clipping: the scan's walk with x*x in place of the count, and the scale that applies what it decided.
// The slot array has the scan's layout in fp32: per tensor NF_REC words, its group id (as a float: exact below 32), then the
// partial sums of its up to FST_MULTI_WG workgroups.  No float atomics: a thread adds its elements in one fma chain in index order, a
// wave adds its lanes in a xor butterfly (commutative adds: every lane ends with the same word), lane 0 of wave 0 adds the four
// wave sums as (0 + 1) + (2 + 3); the finaliser adds in fp64 in a fixed order.  Same inputs, same words.
struct SumsqOp {
  static constexpr bool writes = false;
  float s;
  __device__ __forceinline__ void operator()(float e) { s = __builtin_fmaf(e, e, s); }
};

__global__ __launch_bounds__(256) void sumsq_multi_kernel(GroupArgs a, float* __restrict__ slots) {
  const int t = blockIdx.y;
  if (t >= a.n) return;
  SumsqOp op{0.0f};
  quad_walk(a.x[t], a.numel[t], op);
  float s = op.s;
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  __shared__ float wave_sum[4];
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    slot_record(slots + (size_t)(a.base + t) * NF_REC, a.group[t], (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]));
}

// one workgroup.  A tensor's slots are added in slot order and a group's tensors in tensor order, all in fp64 (256 tensors at a
// time: one thread per tensor, then one thread per group).  Thread 0 then does the arithmetic of optim.clip_coefficients on the
// fp32 norms it reports, in fp64, and rounds the product once.
__global__ __launch_bounds__(256) void sumsq_finalize_kernel(const float* __restrict__ slots, int n_tensors,
                                                             const float* __restrict__ limits, float* __restrict__ norms,
                                                             float* __restrict__ coef) {
  __shared__ double tsum[256];
  __shared__ int tgroup[256];
  __shared__ double gsum[GC_GROUPS];
  __shared__ double cg[GC_GROUPS];
  double acc = 0.0;                                                  // threads 0..31: the group's sum of squares
  for (int base = 0; base < n_tensors; base += 256) {
    const int i = base + (int)threadIdx.x;
    if (i < n_tensors) {
      const float* rec = slots + (size_t)i * NF_REC;
      double s = 0.0;
      for (int k = 0; k < FST_MULTI_WG; ++k) s += (double)rec[1 + k];
      tsum[threadIdx.x] = s;
      tgroup[threadIdx.x] = (int)rec[0] & (GC_GROUPS - 1);
    }
    __syncthreads();
    if (threadIdx.x < GC_GROUPS) {
      const int m = n_tensors - base < 256 ? n_tensors - base : 256;
      for (int j = 0; j < m; ++j)
        if (tgroup[j] == (int)threadIdx.x) acc += tsum[j];
    }
    __syncthreads();
  }
  if (threadIdx.x < GC_GROUPS) gsum[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double all = 0.0;
  int bad = 0;
  for (int g = 0; g < GC_GROUPS; ++g) {
    all += gsum[g];
    const float ng = (float)sqrt(gsum[g]);
    norms[g] = ng;
    bad |= nonfinite_bits(__float_as_uint(ng));
  }
  const float total = (float)sqrt(all);
  norms[GC_GROUPS] = total;
  bad |= nonfinite_bits(__float_as_uint(total));
  double rest = 0.0;                                                 // what the per-group caps leave, squared
  for (int g = 0; g < GC_GROUPS; ++g) {
    const double ng = (double)norms[g];
    cg[g] = fmin(1.0, (double)limits[g] / (ng + 1e-6));
    rest += (cg[g] * ng) * (cg[g] * ng);
  }
  const double c = fmin(1.0, (double)limits[GC_GROUPS] / (sqrt(rest) + 1e-6));
  for (int g = 0; g < GC_GROUPS; ++g) coef[g] = bad ? 1.0f : (float)(cg[g] * c);
}

extern "C" int64_t fst_sumsq_slots(int n_tensors) { return fst_nonfinite_slots(n_tensors); }

extern "C" int fst_sumsq_multi(const float* const* x_host, const int64_t* numel_host, const int32_t* group_host, int n_tensors,
                               float* slots_dev, int64_t slots_len, const float* limits_dev, float* norms_dev, float* coef_dev,
                               void* stream) {
  if (check_group_tensors("fst_sumsq_multi", (const void* const*)x_host, numel_host, group_host, n_tensors)) return -1;
  FST_REQUIRE(limits_dev && norms_dev && coef_dev && (n_tensors == 0 || slots_dev) &&
              (((uintptr_t)limits_dev | (uintptr_t)norms_dev | (uintptr_t)coef_dev | (uintptr_t)slots_dev) & 3) == 0,
              "fst_sumsq_multi: null or misaligned limits, norms, coefficients or slots");
  FST_REQUIRE(slots_len >= fst_sumsq_slots(n_tensors), "fst_sumsq_multi: %lld slots, %lld needed", (long long)slots_len,
              (long long)fst_sumsq_slots(n_tensors));
  if (int rc = fst_multi_chunks(n_tensors, [&](int base, int n) {
        GroupArgs a;
        fill_group(a, (const void* const*)x_host, numel_host, group_host, base, n);
        hipLaunchKernelGGL(sumsq_multi_kernel, fst_multi_grid(numel_host + base, n), dim3(256), 0, (hipStream_t)stream, a, slots_dev);
        FST_LAUNCH_CHECK();
        return 0;
      })) return rc;
  hipLaunchKernelGGL(sumsq_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)slots_dev, n_tensors, limits_dev,
                     norms_dev, coef_dev);
  FST_LAUNCH_CHECK();
  return 0;
}

struct ScaleOp {
  static constexpr bool writes = true;
  float c;
  __device__ __forceinline__ void operator()(float& e) const { e *= c; }
};

// the scan's geometry, writing: coef[group] is one uniform load per workgroup, and a workgroup whose factor is exactly 1.0f
// returns before its first load of x — an unclipped step keeps its gradients' bits and pays no memory pass here
__global__ __launch_bounds__(256) void scale_multi_kernel(GroupArgs a, const float* __restrict__ coef) {
  const int t = blockIdx.y;
  if (t >= a.n) return;
  ScaleOp op{coef[a.group[t]]};
  if (op.c == 1.0f) return;
  quad_walk(a.x[t], a.numel[t], op);
}

extern "C" int fst_scale_multi(float* const* x_host, const int64_t* numel_host, const int32_t* group_host, int n_tensors,
                               const float* coef_dev, void* stream) {
  if (check_group_tensors("fst_scale_multi", (const void* const*)x_host, numel_host, group_host, n_tensors)) return -1;
  FST_REQUIRE(coef_dev && ((uintptr_t)coef_dev & 3) == 0, "fst_scale_multi: null or misaligned coefficients");
  return fst_multi_chunks(n_tensors, [&](int base, int n) {
    GroupArgs a;
    fill_group(a, (const void* const*)x_host, numel_host, group_host, base, n);
    hipLaunchKernelGGL(scale_multi_kernel, fst_multi_grid(numel_host + base, n), dim3(256), 0, (hipStream_t)stream, a, coef_dev);
    FST_LAUNCH_CHECK();
    return 0;
  });
}

// ---- weight averaging (EMA) and the in-place exchange that puts the averages into the modules' own storage.  Both walk PAIRS of
// tensors, tensor t of a launch on grid row t, in the scale's geometry.  The walk is written once (pair_walk) and instantiated for
// 16-byte and for 4-byte units: a pair whose two pointers are both 16-byte aligned goes in quads and hands the up to three
// elements behind its last quad to the dword walk; any other pair (a view that starts off a boundary, or two views that start
// differently) goes in dwords altogether.  Nothing outside [a, a + numel) and [b, b + numel) is touched.
#define EMA_GROUPS GC_GROUPS
#define EMA_DECAY 0                 // the state block, in 4-byte words: decay (fp32)
#define EMA_WARMUP 1                //   warm-up flag (int32)
#define EMA_COUNT 2                 //   count[32] (int32): completed updates per group
#define EMA_W (2 + EMA_GROUPS)      //   w[32] (fp32): the weight of this step
#define EMA_WORDS (2 + 2 * EMA_GROUPS)

struct PairArgs {
  float* a[FST_MULTI_T];
  float* b[FST_MULTI_T];
  int numel[FST_MULTI_T];
  int group[FST_MULTI_T];
  int n;
};
static_assert(sizeof(PairArgs) + sizeof(const float*) <= 4096, "kernel arguments: 4 KB at most");

template <int N>
struct alignas(4 * N) Pack {
  float v[N];
};

// units [0, units) of N floats each, starting at element `first` of both tensors.  The index is unsigned: units < 2^31 and the
// stride is at most 64 * 256, so the last increment stays below 2^32 where a signed index would overflow
template <int N, class Op>
__device__ __forceinline__ void pair_walk(float* __restrict__ a, float* __restrict__ b, int first, int units, Op op) {
  Pack<N>* __restrict__ av = (Pack<N>*)(a + first);
  Pack<N>* __restrict__ bv = (Pack<N>*)(b + first);
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < (unsigned)units; i += gridDim.x * 256u) {
    Pack<N> y = bv[i];
    Pack<N> x = y;
    if (Op::reads_a) x = av[i];
#pragma unroll
    for (int k = 0; k < N; ++k) op(x.v[k], y.v[k]);
    av[i] = x;
    if (op.writes_b) bv[i] = y;
  }
}

template <class Op>
__device__ __forceinline__ void pair_tensor(float* a, float* b, int n, Op op) {
  int done = 0;
  if ((((uintptr_t)a | (uintptr_t)b) & 15u) == 0) {
    pair_walk<4>(a, b, 0, n >> 2, op);
    done = n & ~3;
  }
  pair_walk<1>(a, b, done, n - done, op);
}

// avg = fma(w, live − avg, avg): one IEEE subtraction and one fused multiply-add, never reshaped (contraction is off and the fma
// is spelled out).  w == 1 takes the live value itself: decay 0 means "the average IS the iterate", bit for bit, which
// (live − avg) + avg only is where the subtraction happens to be exact.
struct EmaOp {
  static constexpr bool reads_a = true, writes_b = false;
  float w;
  __device__ __forceinline__ void operator()(float& avg, float& live) const {
#pragma clang fp contract(off)
    const float d = live - avg;
    avg = w == 1.0f ? live : __builtin_fmaf(w, d, avg);
  }
};

struct SwapOp {
  static constexpr bool reads_a = true, writes_b = true;
  __device__ __forceinline__ void operator()(float& x, float& y) const { const float t = x; x = y; y = t; }
};

// one workgroup, threads 0..31 a group each: the weight of THIS step from words read when the kernel runs.  A group of the mask
// takes w = 1 − d_t, d_t = decay or, warming up, min(decay, (1 + count) / (10 + count)), and counts the update; a group outside
// the mask, or any group of a step the anomaly guard skips (verdict != 0), takes w = 0 and keeps its count.
__global__ __launch_bounds__(64) void ema_weights_kernel(uint32_t active_mask, float* __restrict__ state, const int* __restrict__ verdict) {
#pragma clang fp contract(off)
  const int g = threadIdx.x;
  if (g >= EMA_GROUPS) return;
  int* count = (int*)state + EMA_COUNT;
  float w = 0.0f;
  if (((active_mask >> g) & 1u) && !(verdict && verdict[0] != 0)) {
    const int c = count[g];
    float d = state[EMA_DECAY];
    if (((const int*)state)[EMA_WARMUP] != 0) d = fminf(d, (1.0f + (float)c) / (10.0f + (float)c));
    w = 1.0f - d;
    count[g] = c + 1;
  }
  state[EMA_W + g] = w;
}

// w[group] is one uniform load per workgroup; a workgroup whose weight is exactly 0 returns before its first load of either
// tensor: an inactive module and a skipped step keep their averages' bits (NaN payloads included) and pay no memory pass
__global__ __launch_bounds__(256) void ema_multi_kernel(PairArgs a, const float* __restrict__ w_words) {
  const int t = blockIdx.y;
  if (t >= a.n) return;
  const float w = w_words[a.group[t]];
  if (w == 0.0f) return;
  pair_tensor(a.a[t], a.b[t], a.numel[t], EmaOp{w});
}

__global__ __launch_bounds__(256) void swap_multi_kernel(PairArgs a) {
  const int t = blockIdx.y;
  if (t >= a.n) return;
  pair_tensor(a.a[t], a.b[t], a.numel[t], SwapOp{});
}

// every pair of a call before its first launch: the entries of check_group_tensors on both sides (group_host == NULL: no groups),
// and two ranges that do not overlap (the walk holds both pointers restrict; an average is never its own iterate)
static int check_pairs(const char* who, float* const* a_host, float* const* b_host, const int64_t* numel_host, const int32_t* group_host,
                       int n_tensors) {
  FST_REQUIRE(n_tensors >= 0 && n_tensors < (1 << 24) && (n_tensors == 0 || (a_host && b_host && numel_host)), "%s: bad arguments", who);
  for (int i = 0; i < n_tensors; ++i) {
    FST_REQUIRE(fst_multi_entry_ok({a_host[i], b_host[i]}, numel_host[i], 4), "%s: tensor %d: null or misaligned pointer, or bad element count",
                who, i);
    FST_REQUIRE(!group_host || (group_host[i] >= 0 && group_host[i] < EMA_GROUPS), "%s: tensor %d: group %d is not in 0..31", who, i,
                group_host ? group_host[i] : 0);
    const uintptr_t a = (uintptr_t)a_host[i], b = (uintptr_t)b_host[i], bytes = (uintptr_t)numel_host[i] * 4;
    FST_REQUIRE(a + bytes <= b || b + bytes <= a, "%s: tensor %d: the two tensors overlap", who, i);
  }
  return 0;
}

static void fill_pairs(PairArgs& a, float* const* a_host, float* const* b_host, const int64_t* numel_host, const int32_t* group_host,
                       int base, int n) {
  a.n = n;
  for (int i = 0; i < n; ++i) {
    a.a[i] = a_host[base + i]; a.b[i] = b_host[base + i]; a.numel[i] = (int)numel_host[base + i];
    a.group[i] = group_host ? group_host[base + i] : 0;
  }
}

extern "C" int fst_ema_multi(float* const* avg_host, const float* const* live_host, const int64_t* numel_host, const int32_t* group_host,
                             int n_tensors, int32_t active_mask, void* state_dev, const int32_t* verdict_dev, void* stream) {
  FST_REQUIRE(n_tensors == 0 || group_host, "fst_ema_multi: bad arguments");
  if (check_pairs("fst_ema_multi", avg_host, (float* const*)live_host, numel_host, group_host, n_tensors)) return -1;
  FST_REQUIRE(state_dev && (((uintptr_t)state_dev | (uintptr_t)verdict_dev) & 3) == 0, "fst_ema_multi: null or misaligned state or verdict word");
  float* state = (float*)state_dev;
  hipLaunchKernelGGL(ema_weights_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint32_t)active_mask, state, (const int*)verdict_dev);
  FST_LAUNCH_CHECK();
  return fst_multi_chunks(n_tensors, [&](int base, int n) {
    PairArgs a;
    fill_pairs(a, avg_host, (float* const*)live_host, numel_host, group_host, base, n);
    hipLaunchKernelGGL(ema_multi_kernel, fst_multi_grid(numel_host + base, n), dim3(256), 0, (hipStream_t)stream, a,
                       (const float*)(state + EMA_W));
    FST_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int fst_swap_multi(float* const* a_host, float* const* b_host, const int64_t* numel_host, int n_tensors, void* stream) {
  if (check_pairs("fst_swap_multi", a_host, b_host, numel_host, nullptr, n_tensors)) return -1;
  return fst_multi_chunks(n_tensors, [&](int base, int n) {
    PairArgs a;
    fill_pairs(a, a_host, b_host, numel_host, nullptr, base, n);
    hipLaunchKernelGGL(swap_multi_kernel, fst_multi_grid(numel_host + base, n), dim3(256), 0, (hipStream_t)stream, a);
    FST_LAUNCH_CHECK();
    return 0;
  });
}

// ---- gradient accumulation: a window of k calls folds k gradients into one mean, the position in the window a device word, so
// that ONE captured launch series serves every position.  The state block, in 4-byte words: k (int32), j (int32, folds done in
// the open window), inv_k (fp32, the host's float32(1 / k)), windows (int32, closed windows), four reserved words.
#define ACC_K 0
#define ACC_J 1
#define ACC_INV_K 2
#define ACC_WINDOWS 3

// acc = g (the window opens: acc is not read, so it never needs a zero fill) or acc + g, one IEEE addition; on the closing call
// then g = acc * inv_k, one IEEE multiplication (contraction is off: never an fma of the two).  NaN and inf go the way IEEE sends them.
template <bool READS_ACC>
struct AccumOp {
  static constexpr bool reads_a = READS_ACC;   // false on the call that opens a window
  bool writes_b;                               // the call that closes it
  float inv_k;
  __device__ __forceinline__ void operator()(float& acc, float& g) const {
#pragma clang fp contract(off)
    acc = READS_ACC ? acc + g : g;
    if (writes_b) g = acc * inv_k;
  }
};

// k and j are uniform loads per workgroup, taken when the kernel RUNS; with k == 1 (every call opens and closes a window: the mean
// of one gradient is the gradient) a workgroup returns before its first load of either tensor
__global__ __launch_bounds__(256) void accum_multi_kernel(PairArgs a, const int* __restrict__ state) {
  const int t = blockIdx.y;
  if (t >= a.n) return;
  const int k = state[ACC_K], j = state[ACC_J];
  if (k <= 1) return;
  const bool closing = j + 1 >= k;
  const float inv_k = ((const float*)state)[ACC_INV_K];
  if (j == 0) pair_tensor(a.a[t], a.b[t], a.numel[t], AccumOp<false>{closing, inv_k});
  else pair_tensor(a.a[t], a.b[t], a.numel[t], AccumOp<true>{closing, inv_k});
}

// one workgroup, stream-ordered behind the folds of a call: the window moves on, written by lane 0 with ordinary stores
__global__ __launch_bounds__(64) void accum_advance_kernel(int* __restrict__ state) {
  if (threadIdx.x != 0) return;
  const int k = state[ACC_K], j = state[ACC_J];
  const int closing = j + 1 >= k;
  state[ACC_J] = closing ? 0 : j + 1;
  state[ACC_WINDOWS] += closing;
}

extern "C" int fst_accum_multi(float* const* acc_host, float* const* g_host, const int64_t* numel_host, int n_tensors, void* state_dev,
                               int advance, void* stream) {
  if (check_pairs("fst_accum_multi", acc_host, g_host, numel_host, nullptr, n_tensors)) return -1;
  FST_REQUIRE(state_dev && ((uintptr_t)state_dev & 15) == 0, "fst_accum_multi: null state block, or one off a 16-byte boundary");
  if (int rc = fst_multi_chunks(n_tensors, [&](int base, int n) {
        PairArgs a;
        fill_pairs(a, acc_host, g_host, numel_host, nullptr, base, n);
        hipLaunchKernelGGL(accum_multi_kernel, fst_multi_grid(numel_host + base, n), dim3(256), 0, (hipStream_t)stream, a,
                           (const int*)state_dev);
        FST_LAUNCH_CHECK();
        return 0;
      })) return rc;
  if (advance) {
    hipLaunchKernelGGL(accum_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (int*)state_dev);
    FST_LAUNCH_CHECK();
  }
  return 0;
}
