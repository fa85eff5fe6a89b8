// Evaluation on the device: a pass over a resident data set folded batch by batch into words that stay on the device -- rows
// seen, hits, the confusion matrix, the fp64 loss sum, every prediction (and logit, if wanted) -- and closed by a launch that
// decides, on the device, whether this pass is the best so far.  A replayed evaluation so needs nothing from the host but its
// launches, and model selection (optim.guard_copy under the `improved` word) no host read.
//
//   fst_eval_fold     one batch of logits and labels into the running words: a row kernel (one wave per row, four rows per
//                     workgroup) and a one-workgroup launch behind it that adds the rows' losses IN ROW ORDER and moves the words on.
//   fst_eval_finish   one workgroup: improved / best words of the pass.
//
// House style of guard.hip and feed.hip: the pointer tuple rides by value in the kernel arguments, every argument is validated on
// the host before the first launch, every word that steers a kernel (valid, seen, the counters) is read when the kernel RUNS, no
// float atomics (the confusion cells take integer atomicAdd: integer addition commutes), and the state words are written by
// plain stores from one lane.
#include "eval_words.h"            // EVAL_MAX_C, the state block, a row's word, eval_beats, eval_disjoint: shared with vote.hip

// the best block, in 4-byte words
#define EVAL_IMPROVED 0
#define EVAL_PASSES 1
#define EVAL_BEST_HITS 2
#define EVAL_BEST_PASS 3
#define EVAL_BEST_LOSS 4            // fp64: words 4 and 5
#define EVAL_INCOMPLETE 6

struct EvalArgs {
  const float* logits;
  const int64_t* labels;
  const int* valid;
  int* state;
  double* loss;
  int* confusion;
  int64_t* pred_out;
  float* logits_out;
  double* row_nll;                  // scratch: [B]
  int* row_word;                    // scratch: [B], behind row_nll
  int64_t ld;
  int B, C, capacity;
};

__device__ __forceinline__ int eval_valid(const EvalArgs& a) {
  const int v = a.valid[0];
  return v < 0 ? 0 : (v > a.B ? a.B : v);
}

// grid ceil(B / 4) x 256 threads: wave w of a workgroup takes row 4 * blockIdx.x + w, its lanes stride over the C logits.
__global__ __launch_bounds__(256) void eval_rows_kernel(EvalArgs a) {
  const int valid = eval_valid(a), seen = a.state[EVAL_SEEN];
  if ((int64_t)seen + valid > a.capacity || seen < 0) return;
  const int lane = threadIdx.x & 63;
  const int64_t row64 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row64 >= valid) return;                                               // padding rows are never read
  const int row = (int)row64;
  const float* __restrict__ x = a.logits + (size_t)row * a.ld;
  uint32_t* __restrict__ keep = a.logits_out ? (uint32_t*)a.logits_out + ((size_t)seen + row) * a.C : nullptr;
  float best = -INFINITY;
  int at = 0x7FFFFFFF;                                                      // a lane without an element: loses every comparison
  bool odd = false;
  for (int c = lane; c < a.C; c += 64) {
    const float v = x[c];
    if (keep) keep[c] = __float_as_uint(v);
    odd |= !(fabsf(v) < INFINITY);
    if (eval_beats(best, at, v, c)) { best = v; at = c; }
  }
  for (int w = 32; w > 0; w >>= 1) {
    const float v = __shfl_xor(best, w);
    const int j = __shfl_xor(at, w);
    if (eval_beats(best, at, v, j)) { best = v; at = j; }
  }
  odd = __any(odd);
  // log-softmax as F.cross_entropy evaluates it, in fp64: (x[label] - m) - log(sum exp(x - m)); a NaN or an inf propagates
  const double m = (double)best;
  double s = 0.0;
  for (int c = lane; c < a.C; c += 64) s += exp((double)x[c] - m);
  for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w);
  if (lane != 0) return;
  const int64_t label = a.labels[row];
  const bool bad = label < 0 || label >= a.C;
  int word = at | (odd ? EVAL_ROW_NONFINITE : 0);
  double nll = 0.0;
  if (bad) {
    word |= EVAL_ROW_BAD_LABEL;
  } else {
    nll = -(((double)x[label] - m) - log(s));
    atomicAdd(a.confusion + (size_t)label * a.C + at, 1);
    if (label == at) word |= EVAL_ROW_HIT;
  }
  a.row_nll[row] = nll;
  a.row_word[row] = word;
  if (a.pred_out) a.pred_out[(size_t)seen + row] = at;
}

// one workgroup, stream-ordered behind the rows of a call: the counters as fixed-order sums through LDS, the loss as ONE chain of
// fp64 additions in row order from the running word (so a pass's loss does not depend on how it was cut into batches); then lane
// 0 moves the words on with ordinary stores.
__global__ __launch_bounds__(256) void eval_advance_kernel(EvalArgs a) {
  __shared__ double nll[256];
  __shared__ int word[256];
  __shared__ int part[3][256];
  const int valid = eval_valid(a), seen = a.state[EVAL_SEEN];
  if ((int64_t)seen + valid > a.capacity || seen < 0) {
    if (threadIdx.x == 0) a.state[EVAL_OVERFLOW] += 1;
    return;
  }
  double loss = a.loss[0];
  int hits = 0, bad = 0, odd = 0;
  for (int r0 = 0; r0 < valid; r0 += 256) {
    const int r = r0 + threadIdx.x;
    const int w = r < valid ? a.row_word[r] : EVAL_ROW_BAD_LABEL;             // (a row past the end adds nothing, like a bad label)
    nll[threadIdx.x] = r < valid ? a.row_nll[r] : 0.0;
    word[threadIdx.x] = w;
    if (r < valid) {
      hits += (w & EVAL_ROW_HIT) != 0; bad += (w & EVAL_ROW_BAD_LABEL) != 0; odd += (w & EVAL_ROW_NONFINITE) != 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = valid - r0 < 256 ? valid - r0 : 256;
#pragma unroll 8
      for (int i = 0; i < n; ++i) loss = (word[i] & EVAL_ROW_BAD_LABEL) ? loss : loss + nll[i];
    }
    __syncthreads();
  }
  part[0][threadIdx.x] = hits; part[1][threadIdx.x] = bad; part[2][threadIdx.x] = odd;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int k = 0; k < 3; ++k) part[k][threadIdx.x] += part[k][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  a.loss[0] = loss;
  a.state[EVAL_HITS] += part[0][0];
  a.state[EVAL_BAD_LABEL] += part[1][0];
  a.state[EVAL_NONFINITE] += part[2][0];
  a.state[EVAL_BATCHES] += 1;
  a.state[EVAL_SEEN] = seen + valid;
}

// one workgroup, one lane: closes a pass
__global__ __launch_bounds__(64) void eval_finish_kernel(const int* __restrict__ state, const double* __restrict__ loss_dev, int expect_rows,
                                                         int* __restrict__ best, int mode) {
  if (threadIdx.x != 0) return;
  const int hits = state[EVAL_HITS];
  const double loss = loss_dev[0];
  double* best_loss = (double*)(best + EVAL_BEST_LOSS);
  const bool complete = state[EVAL_SEEN] == expect_rows && state[EVAL_OVERFLOW] == 0 && state[EVAL_BAD_LABEL] == 0;
  const bool better = mode == 0 ? hits > best[EVAL_BEST_HITS] : loss < best_loss[0];   // (a NaN loss compares false)
  const int passes = best[EVAL_PASSES] + 1;
  if (!complete) best[EVAL_INCOMPLETE] += 1;
  if (complete && better) {
    best[EVAL_BEST_HITS] = hits;
    best[EVAL_BEST_PASS] = passes;
    best_loss[0] = loss;
  }
  best[EVAL_IMPROVED] = complete && better;
  best[EVAL_PASSES] = passes;
}

extern "C" int fst_eval_fold(const float* logits, int64_t ld, const int64_t* labels, int64_t B, int C, const void* valid_dev,
                             void* state_dev, void* loss_dev, void* confusion_dev, int64_t* pred_out, float* logits_out,
                             int64_t capacity, void* scratch, void* stream) {
  FST_REQUIRE(B >= 1 && B < (1LL << 31) && C >= 1 && C <= EVAL_MAX_C && ld >= C && ld < (1LL << 31),
              "fst_eval_fold: B %lld (1..2^31 - 1), C %d (1..%d), ld %lld (C..2^31 - 1)", (long long)B, C, EVAL_MAX_C, (long long)ld);
  FST_REQUIRE(capacity >= 1 && capacity < (1LL << 31), "fst_eval_fold: capacity %lld (1..2^31 - 1)", (long long)capacity);
  FST_REQUIRE(logits && labels && valid_dev && state_dev && loss_dev && confusion_dev && scratch, "fst_eval_fold: null pointer");
  FST_REQUIRE((((uintptr_t)logits | (uintptr_t)valid_dev | (uintptr_t)confusion_dev | (uintptr_t)logits_out) & 3) == 0,
              "fst_eval_fold: logits, valid, confusion and logits_out must be 4-byte aligned");
  FST_REQUIRE((((uintptr_t)labels | (uintptr_t)loss_dev | (uintptr_t)pred_out | (uintptr_t)scratch) & 7) == 0,
              "fst_eval_fold: labels, loss, pred_out and the scratch must be 8-byte aligned");
  FST_REQUIRE(((uintptr_t)state_dev & 15) == 0, "fst_eval_fold: the state block is off a 16-byte boundary");
  const uint64_t uB = (uint64_t)B, uC = (uint64_t)C, cap = (uint64_t)capacity;
  struct Span { const void* p; uint64_t bytes; const char* name; };
  const Span in[3] = {{logits, ((uB - 1) * (uint64_t)ld + uC) * 4, "logits"}, {labels, uB * 8, "labels"}, {valid_dev, 4, "valid"}};
  const Span out[6] = {{state_dev, 32, "state"},       {loss_dev, 8, "loss"},
                       {confusion_dev, uC * uC * 4, "confusion"}, {pred_out, cap * 8, "pred_out"},
                       {logits_out, cap * uC * 4, "logits_out"},  {scratch, uB * 12, "scratch"}};
  for (int o = 0; o < 6; ++o) {
    for (int i = 0; i < 3; ++i)
      FST_REQUIRE(eval_disjoint(out[o].p, out[o].bytes, in[i].p, in[i].bytes), "fst_eval_fold: %s overlaps %s", out[o].name, in[i].name);
    for (int q = 0; q < o; ++q)
      FST_REQUIRE(eval_disjoint(out[o].p, out[o].bytes, out[q].p, out[q].bytes), "fst_eval_fold: %s overlaps %s", out[o].name, out[q].name);
  }
  EvalArgs a = {};
  a.logits = logits; a.labels = labels; a.valid = (const int*)valid_dev; a.state = (int*)state_dev; a.loss = (double*)loss_dev;
  a.confusion = (int*)confusion_dev; a.pred_out = pred_out; a.logits_out = logits_out;
  a.row_nll = (double*)scratch; a.row_word = (int*)((double*)scratch + B);
  a.ld = ld; a.B = (int)B; a.C = C; a.capacity = (int)capacity;
  hipLaunchKernelGGL(eval_rows_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  FST_LAUNCH_CHECK();
  hipLaunchKernelGGL(eval_advance_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  FST_LAUNCH_CHECK();
  return 0;
}

extern "C" int fst_eval_finish(const void* state_dev, const void* loss_dev, int64_t expect_rows, void* best_dev, int mode, void* stream) {
  FST_REQUIRE(state_dev && loss_dev && best_dev, "fst_eval_finish: null pointer");
  FST_REQUIRE((((uintptr_t)state_dev | (uintptr_t)best_dev) & 15) == 0 && ((uintptr_t)loss_dev & 7) == 0,
              "fst_eval_finish: the state and best blocks must be 16-byte aligned, the loss word 8-byte");
  FST_REQUIRE(expect_rows >= 0 && expect_rows < (1LL << 31) && (mode == 0 || mode == 1),
              "fst_eval_finish: expect_rows %lld (0..2^31 - 1), mode %d (0: accuracy, 1: loss)", (long long)expect_rows, mode);
  FST_REQUIRE(eval_disjoint(best_dev, 32, state_dev, 32) && eval_disjoint(best_dev, 32, loss_dev, 8),
              "fst_eval_finish: the best block overlaps the state or the loss");
  hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int*)state_dev, (const double*)loss_dev,
                     (int)expect_rows, (int*)best_dev, mode);
  FST_LAUNCH_CHECK();
  return 0;
}
