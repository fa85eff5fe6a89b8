// Device primitives shared by the matrix-core kernels of libfst_hip.so (gfx950 only): the operand split every parity
// tolerance of the project rests on, the operand-staging pieces around it, accumulator zeroing, and the diagnostic cycle stamps.
#pragma once
#include "fst_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// The split-bf16 product: v = hi + lo + O(2^-18 |v|) with hi = bf16_rne(v), lo = bf16_rne(v - hi); a product is formed as
// hi·hi + hi·lo + lo·hi.  Two floats -> (hi pair, lo pair), each a dword of two round-to-nearest bf16 (first element in the low half).
__device__ __forceinline__ void split_bf16_pair(float a, float b, unsigned& hi, unsigned& lo) {
  const f32x2 v = {a, b};
  hi = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
  const f32x2 r = {a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u)};
  lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
}

// Eight floats -> one lane's hi and lo fragments of v_mfma_f32_32x32x16_bf16 (element j of the fragment = v[j]).
__device__ __forceinline__ void split_bf16x8(const float (&v)[8], bf16x8& hi, bf16x8& lo) {
  u32x4 h, l;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned hh, ll;
    split_bf16_pair(v[2 * j], v[2 * j + 1], hh, ll);
    h[j] = hh; l[j] = ll;
  }
  hi = __builtin_bit_cast(bf16x8, h);
  lo = __builtin_bit_cast(bf16x8, l);
}

// acc += a·b as lo(a)·hi(b) + hi(a)·lo(b) + hi(a)·hi(b), fp32 accumulation.  The order is part of the arithmetic: the two
// small terms (2^-9 of the product) are added first and hi·hi last, and every accumulation of the project was validated
// bit for bit in this order — reordering the three changes the rounding of each fp32 add, i.e. the results every parity
// tolerance and every recorded output were taken with.  lo·lo (2^-18) is dropped.
__device__ __forceinline__ void mfma_bf3(f32x16& acc, bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

// Clear the accumulators of one 32x32 MFMA tile, of a row of tiles, of a grid of tiles.
__device__ __forceinline__ void zero_acc(f32x16& acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
}
template <int N>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) zero_acc(acc[j]);
}
template <int M, int N>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[M][N]) {
#pragma unroll
  for (int i = 0; i < M; ++i) zero_acc(acc[i]);
}

// The (hi, lo) A fragments of row block mb of a packed weight stage at base: per block 1 KiB hi then 1 KiB lo, 16 bytes per lane.
__device__ __forceinline__ void lds_read_a_frag(const char* base, int mb, int lane, bf16x8& ah, bf16x8& al) {
  ah = *reinterpret_cast<const bf16x8*>(base + mb * 2048 + lane * 16);
  al = *reinterpret_cast<const bf16x8*>(base + mb * 2048 + 1024 + lane * 16);
}

// wait until at most N of this wave's vector-memory operations (loads, LDS-DMA pieces) are still in flight
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// One LDS-DMA piece through the builtin (global_load_lds_dwordx4): the 64 lanes' 16 bytes from gsrc land at lds_dst + 16·lane.
__device__ __forceinline__ void lds_dma16(const void* gsrc, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc, (__attribute__((address_space(3))) void*)lds_dst,
                                   16, 0, 0);
}

// Diagnostic cycle stamps (-DFST_STAMPS, tools/build_stamps.sh; never shipped): per-phase s_memtime sums of a kernel's waves.
// A kernel declares FST_SUMS(N), takes stamps with FST_T, adds phases into slots with FST_ACC and ends with FST_FLUSH(counters),
// counters being the file's __device__ array of N slots, read on the host through fst_read_stamps.  The phase sums live in
// registers and are flushed ONCE per wave, by lane 0 (per-stage atomics would serialise on a few words and sit in vmcnt, i.e.
// measure themselves).
#ifdef FST_STAMPS
__device__ __forceinline__ unsigned long long fst_now() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
template <int N>
int fst_read_stamps(unsigned long long (&counters)[N], unsigned long long* out_host, int reset) {
  if (out_host) hipMemcpyFromSymbol(out_host, HIP_SYMBOL(counters), sizeof(counters));
  if (reset) { unsigned long long z[N] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(counters), z, sizeof(z)); }
  return 0;
}
#define FST_T(var) const unsigned long long var = fst_now()
#define FST_ACC(slot, a, b) fst_sum_[slot] += (b) - (a)
#define FST_SUMS(N) unsigned long long fst_sum_[N] = {0}
#define FST_FLUSH(counters) \
  if (lane == 0) for (int i_ = 0; i_ < (int)(sizeof(fst_sum_) / sizeof(fst_sum_[0])); ++i_) atomicAdd(&counters[i_], fst_sum_[i_])
#else
#define FST_T(var)
#define FST_ACC(slot, a, b)
#define FST_SUMS(N)
#define FST_FLUSH(counters)
#endif
