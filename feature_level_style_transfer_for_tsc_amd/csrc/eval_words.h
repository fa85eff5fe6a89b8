// What eval.hip and vote.hip share: the limit on classes, the state block of a folded pass, the argmax rule and the overlap test.
#pragma once
#include "fst_common.h"

#define EVAL_MAX_C 4096

// the state block, in int32 words (two more are reserved)
#define EVAL_SEEN 0                 // rows folded in this pass; where this batch's outputs go
#define EVAL_HITS 1
#define EVAL_BATCHES 2
#define EVAL_BAD_LABEL 3            // labels outside 0..C-1
#define EVAL_NONFINITE 4            // rows holding a NaN or an inf
#define EVAL_OVERFLOW 5             // calls that found seen + valid > capacity

// a row's word in the scratch: the prediction in the low bits (C <= 4096), the row's flags above it
#define EVAL_ROW_PRED_MASK 0xFFFF
#define EVAL_ROW_HIT (1 << 28)
#define EVAL_ROW_NONFINITE (1 << 29)
#define EVAL_ROW_BAD_LABEL (1 << 30)

// torch.argmax on the CPU: the first index of the maximum, a NaN beats every number and the first NaN wins, -0.0 == +0.0 is a tie
// for the lower index.  (v, i) against (w, j): does (w, j) take the place of (v, i)?
template <typename T>
__device__ __forceinline__ bool eval_beats(T v, int i, T w, int j) {
  const bool vn = v != v, wn = w != w;
  if (vn || wn) return wn && (!vn || j < i);
  return w > v || (w == v && j < i);
}

static inline bool eval_disjoint(const void* p, uint64_t p_bytes, const void* q, uint64_t q_bytes) {
  if (!p || !q) return true;
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a + p_bytes <= b || b + q_bytes <= a;
}
