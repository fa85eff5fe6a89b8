// The split-bf16 arithmetic of a 256-thread tile frame (gemm.hip's gemm_tile, mmd.hip's Gram tile): the LDS form of a fetched
// operand tile — IMAGES images of ROWS rows of 32 k at PITCH bytes, one behind the other; HALF bytes from lane half 0's fragment
// to lane half 1's — with `stage` writing a tile into it and `multiply` taking one 32-k stage out of it: a / b point at this
// lane's row of the first image of the A / B tile.  The thread map of a staged tile of ROWS rows × 32 k, ROWS/8 floats per thread:
//   [rows][K] storage: thread t holds k = 4(t&7) .. +3 of rows (t>>3) + 32j
//   [K][rows] storage: thread t holds row t % ROWS, k = KR·(t / ROWS) .. + KR − 1   (KR = ROWS/8 consecutive k)
#pragma once
#include "fst_device.h"

// split-bf16: a hi and a lo image, rows of 32 bf16; 16 ds_read_b128 per 24 MFMAs and no conversion in the multiply
struct GemmBf3 {
  static constexpr int PITCH = 80, IMAGES = 2, HALF = 16;

  template <int ROWS>
  static __device__ __forceinline__ void stage(const float (&v)[ROWS / 8], char* hi_img, int trans, int tid) {
    constexpr int KR = ROWS / 8;
    char* const lo_img = hi_img + ROWS * PITCH;
    if (!trans) {
      const int kb = 8 * (tid & 7), r0 = tid >> 3;           // byte offset of k = 4(t&7) in a row of bf16
#pragma unroll
      for (int j = 0; j < ROWS / 32; ++j) {
        unsigned h0, l0, h1, l1;
        split_bf16_pair(v[4 * j], v[4 * j + 1], h0, l0);
        split_bf16_pair(v[4 * j + 2], v[4 * j + 3], h1, l1);
        const int off = (r0 + 32 * j) * PITCH + kb;
        *reinterpret_cast<uint2*>(hi_img + off) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(lo_img + off) = make_uint2(l0, l1);
      }
    } else {
      const int off = (tid % ROWS) * PITCH + 2 * KR * (tid / ROWS);
#pragma unroll
      for (int c = 0; c < KR / 8; ++c) {
        bf16x8 h, l;
        split_bf16x8(*reinterpret_cast<const float(*)[8]>(&v[8 * c]), h, l);   // (elements 8c..8c+7 in place: a local copy changes the schedule)
        *reinterpret_cast<bf16x8*>(hi_img + off + 16 * c) = h;
        *reinterpret_cast<bf16x8*>(lo_img + off + 16 * c) = l;
      }
    }
  }

  template <int TM, int TN>
  static __device__ __forceinline__ void multiply(f32x16 (&acc)[TM][TN], const char* a_hi, const char* b_hi) {
    const char* const a_lo = a_hi + 64 * TM * PITCH;
    const char* const b_lo = b_hi + 64 * TN * PITCH;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        ah[i] = *reinterpret_cast<const bf16x8*>(a_hi + i * 32 * PITCH + 32 * ks);
        al[i] = *reinterpret_cast<const bf16x8*>(a_lo + i * 32 * PITCH + 32 * ks);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        bh[j] = *reinterpret_cast<const bf16x8*>(b_hi + j * 32 * PITCH + 32 * ks);
        bl[j] = *reinterpret_cast<const bf16x8*>(b_lo + j * 32 * PITCH + 32 * ks);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) mfma_bf3(acc[i][j], ah[i], al[i], bh[j], bl[j]);
    }
  }
};
