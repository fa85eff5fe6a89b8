// Host scaffolding of the multi-tensor launchers (optim.hip, guard.hip).  A call of n_tensors (pointer..., count) entries goes out
// in launches of at most FST_MULTI_T entries, carried BY VALUE in the kernel arguments, on a grid (bx, n): tensor t of a launch on
// grid row t, up to FST_MULTI_WG workgroups of 256 threads each per tensor, grid-stride beyond.  Every entry of a call is checked
// before its first launch: a refused call has launched nothing, whichever index the bad entry has.
#pragma once
#include <initializer_list>

#include "fst_common.h"

#define FST_MULTI_T 64              // tensors per launch
#define FST_MULTI_WG 64             // workgroups per tensor at most

// one entry of a call: every pointer set and on an `align`-byte boundary (a power of two; 1: any), 0 < count < 2^31
static inline bool fst_multi_entry_ok(std::initializer_list<const void*> ptrs, int64_t count, uintptr_t align) {
  for (const void* p : ptrs)
    if (!p || ((uintptr_t)p & (align - 1)) != 0) return false;
  return count > 0 && count < (1LL << 31);
}

// workgroups per tensor of a launch: four elements (one 16-byte access) per thread for its largest tensor, within FST_MULTI_WG
static inline int group_launch_bx(const int64_t* numel_host, int n) {
  long long most = 0;
  for (int i = 0; i < n; ++i) most = most > numel_host[i] ? most : numel_host[i];
  const int bx = (int)((most + 1023) / 1024);
  return bx < 1 ? 1 : (bx > FST_MULTI_WG ? FST_MULTI_WG : bx);
}

// the grid of the launch that takes the n entries whose counts start at numel_host
static inline dim3 fst_multi_grid(const int64_t* numel_host, int n) { return dim3((unsigned)group_launch_bx(numel_host, n), (unsigned)n); }

// the chunks of a call: body(base, n) for base = 0, 64, ... with n = min(64, n_tensors − base) entries each.  The body fills its
// argument struct, launches, checks the launch and returns 0; its first non-zero return ends the walk and is the result.
template <class Body>
static inline int fst_multi_chunks(int n_tensors, Body body) {
  for (int base = 0; base < n_tensors; base += FST_MULTI_T) {
    const int n = n_tensors - base < FST_MULTI_T ? n_tensors - base : FST_MULTI_T;
    if (int rc = body(base, n)) return rc;
  }
  return 0;
}
