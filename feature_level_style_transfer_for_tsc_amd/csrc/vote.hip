// Multi-source voting on the device (multi_source_voting.py:265-429): K target-side models vote on a resident test set, batch by
// batch, into words that stay on the device, as eval.hip folds one model's pass.
//
//   fst_vote_weights  K train-set confusion matrices -> per-class precision weights w[K][C] and scale[K][C] = base^w: one launch,
//                     one thread per class, fp64.
//   fst_vote_fold     one batch of K logit blocks into the running words: a row kernel (one wave per row, four rows per workgroup)
//                     that does the whole per-row arithmetic in fp64 -- softmax, entropy, sharpening, the scaled sum over the
//                     members, the argmax -- and a one-workgroup launch behind it that adds the rows' counters in a fixed order
//                     and moves the words on.
//
// House style of eval.hip, guard.hip and feed.hip: the pointer tuples ride by value in the kernel arguments, every argument is
// validated on the host before the first launch, every word that steers a kernel (valid, seen) is read when the kernel RUNS, no
// float atomics (the confusion cells take integer atomicAdd: integer addition commutes), and the state words are written by plain
// stores from one lane.
#include "eval_words.h"

#define VOTE_MAX_K 16

struct VoteWeightArgs {
  const int* cm[VOTE_MAX_K];
  double* weights;
  double* scale;
  double base;
  int K, C;
};

// grid ceil(C / 64) x 64 threads, thread = class c: the reads of row r of a matrix coalesce across the threads.  Two loops over the
// members: the precisions (parked in weights_out, which this thread alone reads back) and their sum with k ascending, then the
// quotients.
__global__ __launch_bounds__(64) void vote_weights_kernel(VoteWeightArgs a) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= a.C) return;
  double sum = 0.0;
  for (int k = 0; k < a.K; ++k) {
    const int* __restrict__ cm = a.cm[k];
    long long predicted = 0;
    for (int r = 0; r < a.C; ++r) predicted += cm[(size_t)r * a.C + c];
    const double prec = predicted > 0 ? (double)cm[(size_t)c * a.C + c] / (double)predicted : 0.0;
    a.weights[(size_t)k * a.C + c] = prec;
    sum += prec;
  }
  const double mean = sum / (double)a.K;
  for (int k = 0; k < a.K; ++k) {
    double w = a.weights[(size_t)k * a.C + c] / mean;
    if (!(fabs(w) < INFINITY)) w = 0.0;                                       // 0 / 0 and x / 0: the class counts for nothing
    a.weights[(size_t)k * a.C + c] = w;
    a.scale[(size_t)k * a.C + c] = pow(a.base, w);
  }
}

struct VoteArgs {
  const float* logits[VOTE_MAX_K];
  const double* scale;
  const int64_t* labels;
  const int* valid;
  int* state;
  int* member_hits;
  int* confusion;
  int64_t* pred_out;
  double* scores_out;
  int* row_word;                    // scratch: [B], as eval.hip's
  int* row_members;                 // scratch: [B], behind row_word: bit k = member k's own prediction is the label
  double sharpen;
  int64_t ld;
  int B, C, K, capacity;
};

__device__ __forceinline__ int vote_valid(const VoteArgs& a) {
  const int v = a.valid[0];
  return v < 0 ? 0 : (v > a.B ? a.B : v);
}

// grid ceil(B / 4) x 256 threads: wave w of a workgroup takes row 4 * blockIdx.x + w, its lanes stride over the C classes.  The
// lane-to-class assignment and the butterflies are fixed, so a row's bits do not depend on the batch it arrives in.
__global__ __launch_bounds__(256) void vote_rows_kernel(VoteArgs a) {
  // (m, s, f) of the row's members.  After a butterfly every lane of the wave holds the same bits; each lane stores them and reads
  // back what it stored itself, so the wave needs no barrier.
  __shared__ double member[4][VOTE_MAX_K][3];
  const int valid = vote_valid(a), seen = a.state[EVAL_SEEN];
  if ((int64_t)seen + valid > a.capacity || seen < 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row64 = (int64_t)blockIdx.x * 4 + wave;
  if (row64 >= valid) return;                                               // padding rows are never read
  const int row = (int)row64;
  const int64_t label = a.labels[row];
  const bool bad = label < 0 || label >= a.C;
  int members = 0;
  bool odd = false;
  for (int k = 0; k < a.K; ++k) {
    const float* __restrict__ x = a.logits[k] + (size_t)row * a.ld;
    float best = -INFINITY;
    int at = 0x7FFFFFFF;                                                    // a lane without an element: loses every comparison
    for (int c = lane; c < a.C; c += 64) {
      const float v = x[c];
      odd |= !(fabsf(v) < INFINITY);
      if (eval_beats(best, at, v, c)) { best = v; at = c; }
    }
    for (int w = 32; w > 0; w >>= 1) {
      const float v = __shfl_xor(best, w);
      const int j = __shfl_xor(at, w);
      if (eval_beats(best, at, v, j)) { best = v; at = j; }
    }
    members |= (!bad && at == (int)label) ? 1 << k : 0;
    // the softmax around the maximum and its entropy, H = log s - T / s: two non-negative terms, no cancellation
    const double m = (double)best;                                          // (a NaN in the row is the maximum: everything below is NaN)
    double s = 0.0, t = 0.0;
    for (int c = lane; c < a.C; c += 64) {
      const double z = (double)x[c] - m, e = exp(z);
      s += e;
      t += e == 0.0 ? 0.0 : e * z;                                          // a -inf logit: probability 0, no 0 * inf
    }
    for (int w = 32; w > 0; w >>= 1) { s += __shfl_xor(s, w); t += __shfl_xor(t, w); }
    const double H = log(s) - t / s;
    member[wave][k][0] = m;
    member[wave][k][1] = s;
    member[wave][k][2] = 1.0 + a.sharpen * exp(-H);
  }
  odd = __any(odd);
  double* __restrict__ keep = a.scores_out ? a.scores_out + ((size_t)seen + row) * a.C : nullptr;
  double top = -INFINITY;
  int at = 0x7FFFFFFF;
  for (int c = lane; c < a.C; c += 64) {
    double score = 0.0;
    for (int k = 0; k < a.K; ++k) {
      const double e = exp((double)a.logits[k][(size_t)row * a.ld + c] - member[wave][k][0]);
      score += e / member[wave][k][1] * member[wave][k][2] * a.scale[(size_t)k * a.C + c];
    }
    if (keep) keep[c] = score;
    if (eval_beats(top, at, score, c)) { top = score; at = c; }
  }
  for (int w = 32; w > 0; w >>= 1) {
    const double v = __shfl_xor(top, w);
    const int j = __shfl_xor(at, w);
    if (eval_beats(top, at, v, j)) { top = v; at = j; }
  }
  if (lane != 0) return;
  int word = at | (odd ? EVAL_ROW_NONFINITE : 0);
  if (bad) {
    word |= EVAL_ROW_BAD_LABEL;
  } else {
    atomicAdd(a.confusion + (size_t)label * a.C + at, 1);
    if (label == at) word |= EVAL_ROW_HIT;
  }
  a.row_word[row] = word;
  a.row_members[row] = members;
  a.pred_out[(size_t)seen + row] = at;
}

#define VOTE_COUNTERS (3 + VOTE_MAX_K)

// one workgroup, stream-ordered behind the rows of a call: the counters as fixed-order sums through LDS; then lane 0 moves the words
// on with ordinary stores.
__global__ __launch_bounds__(256) void vote_advance_kernel(VoteArgs a) {
  __shared__ int part[VOTE_COUNTERS][256];
  const int valid = vote_valid(a), seen = a.state[EVAL_SEEN];
  if ((int64_t)seen + valid > a.capacity || seen < 0) {
    if (threadIdx.x == 0) a.state[EVAL_OVERFLOW] += 1;
    return;
  }
  int count[VOTE_COUNTERS];
#pragma unroll
  for (int i = 0; i < VOTE_COUNTERS; ++i) count[i] = 0;
  for (int r = threadIdx.x; r < valid; r += 256) {
    const int w = a.row_word[r], members = a.row_members[r];
    count[0] += (w & EVAL_ROW_HIT) != 0; count[1] += (w & EVAL_ROW_BAD_LABEL) != 0; count[2] += (w & EVAL_ROW_NONFINITE) != 0;
#pragma unroll
    for (int k = 0; k < VOTE_MAX_K; ++k) count[3 + k] += (members >> k) & 1;
  }
#pragma unroll
  for (int i = 0; i < VOTE_COUNTERS; ++i) part[i][threadIdx.x] = count[i];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int i = 0; i < VOTE_COUNTERS; ++i) part[i][threadIdx.x] += part[i][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  a.state[EVAL_HITS] += part[0][0];
  a.state[EVAL_BAD_LABEL] += part[1][0];
  a.state[EVAL_NONFINITE] += part[2][0];
  for (int k = 0; k < a.K; ++k) a.member_hits[k] += part[3 + k][0];
  a.state[EVAL_BATCHES] += 1;
  a.state[EVAL_SEEN] = seen + valid;
}

struct VoteSpan { const void* p; uint64_t bytes; const char* name; };

// no output overlaps an input or an earlier output (inputs may share storage among themselves)
static int vote_check_spans(const char* who, const VoteSpan* in, int n_in, const VoteSpan* out, int n_out) {
  for (int o = 0; o < n_out; ++o) {
    for (int i = 0; i < n_in; ++i)
      FST_REQUIRE(eval_disjoint(out[o].p, out[o].bytes, in[i].p, in[i].bytes), "%s: %s overlaps %s", who, out[o].name, in[i].name);
    for (int q = 0; q < o; ++q)
      FST_REQUIRE(eval_disjoint(out[o].p, out[o].bytes, out[q].p, out[q].bytes), "%s: %s overlaps %s", who, out[o].name, out[q].name);
  }
  return 0;
}

static const char* const vote_member_name[VOTE_MAX_K] = {"member 0",  "member 1",  "member 2",  "member 3", "member 4",  "member 5",
                                                         "member 6",  "member 7",  "member 8",  "member 9", "member 10", "member 11",
                                                         "member 12", "member 13", "member 14", "member 15"};

extern "C" int fst_vote_weights(const void* const* confusion_host, int K, int C, float base, double* weights_out, double* scale_out,
                                void* stream) {
  FST_REQUIRE(K >= 1 && K <= VOTE_MAX_K && C >= 1 && C <= EVAL_MAX_C, "fst_vote_weights: K %d (1..%d), C %d (1..%d)", K, VOTE_MAX_K, C,
              EVAL_MAX_C);
  FST_REQUIRE(base > 0.0f && base < INFINITY, "fst_vote_weights: base %g must be positive and finite", (double)base);
  FST_REQUIRE(confusion_host && weights_out && scale_out, "fst_vote_weights: null pointer");
  FST_REQUIRE((((uintptr_t)weights_out | (uintptr_t)scale_out) & 7) == 0, "fst_vote_weights: weights_out and scale_out must be 8-byte aligned");
  const uint64_t uK = (uint64_t)K, uC = (uint64_t)C;
  VoteSpan in[VOTE_MAX_K];
  for (int k = 0; k < K; ++k) {
    FST_REQUIRE(confusion_host[k], "fst_vote_weights: null confusion matrix of member %d", k);
    FST_REQUIRE(((uintptr_t)confusion_host[k] & 3) == 0, "fst_vote_weights: the confusion matrix of member %d must be 4-byte aligned", k);
    in[k] = {confusion_host[k], uC * uC * 4, vote_member_name[k]};
  }
  const VoteSpan out[2] = {{weights_out, uK * uC * 8, "weights_out"}, {scale_out, uK * uC * 8, "scale_out"}};
  if (vote_check_spans("fst_vote_weights", in, K, out, 2)) return -1;
  VoteWeightArgs a = {};
  for (int k = 0; k < K; ++k) a.cm[k] = (const int*)confusion_host[k];
  a.weights = weights_out; a.scale = scale_out; a.base = (double)base; a.K = K; a.C = C;
  hipLaunchKernelGGL(vote_weights_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  FST_LAUNCH_CHECK();
  return 0;
}

extern "C" int fst_vote_fold(const float* const* logits_host, int K, int64_t ld, const int64_t* labels, int64_t B, int C,
                             const double* scale, const void* valid_dev, void* state_dev, void* member_hits_dev, void* confusion_dev,
                             int64_t* pred_out, double* scores_out, float sharpen, int64_t capacity, void* scratch, void* stream) {
  FST_REQUIRE(K >= 1 && K <= VOTE_MAX_K, "fst_vote_fold: K %d (1..%d)", K, VOTE_MAX_K);
  FST_REQUIRE(B >= 1 && B < (1LL << 31) && C >= 1 && C <= EVAL_MAX_C && ld >= C && ld < (1LL << 31),
              "fst_vote_fold: B %lld (1..2^31 - 1), C %d (1..%d), ld %lld (C..2^31 - 1)", (long long)B, C, EVAL_MAX_C, (long long)ld);
  FST_REQUIRE(capacity >= 1 && capacity < (1LL << 31), "fst_vote_fold: capacity %lld (1..2^31 - 1)", (long long)capacity);
  FST_REQUIRE(sharpen >= 0.0f && sharpen < INFINITY, "fst_vote_fold: sharpen %g must be finite and not negative", (double)sharpen);
  FST_REQUIRE(logits_host && labels && scale && valid_dev && state_dev && member_hits_dev && confusion_dev && pred_out && scratch,
              "fst_vote_fold: null pointer");
  FST_REQUIRE((((uintptr_t)valid_dev | (uintptr_t)member_hits_dev | (uintptr_t)confusion_dev | (uintptr_t)scratch) & 3) == 0,
              "fst_vote_fold: valid, member_hits, confusion and the scratch must be 4-byte aligned");
  FST_REQUIRE((((uintptr_t)labels | (uintptr_t)scale | (uintptr_t)pred_out | (uintptr_t)scores_out) & 7) == 0,
              "fst_vote_fold: labels, scale, pred_out and scores_out must be 8-byte aligned");
  FST_REQUIRE(((uintptr_t)state_dev & 15) == 0, "fst_vote_fold: the state block is off a 16-byte boundary");
  const uint64_t uB = (uint64_t)B, uC = (uint64_t)C, uK = (uint64_t)K, cap = (uint64_t)capacity;
  VoteSpan in[VOTE_MAX_K + 3];
  for (int k = 0; k < K; ++k) {
    FST_REQUIRE(logits_host[k], "fst_vote_fold: null logits of member %d", k);
    FST_REQUIRE(((uintptr_t)logits_host[k] & 3) == 0, "fst_vote_fold: the logits of member %d must be 4-byte aligned", k);
    in[k] = {logits_host[k], ((uB - 1) * (uint64_t)ld + uC) * 4, vote_member_name[k]};
  }
  in[K] = {labels, uB * 8, "labels"};
  in[K + 1] = {scale, uK * uC * 8, "scale"};
  in[K + 2] = {valid_dev, 4, "valid"};
  const VoteSpan out[6] = {{state_dev, 32, "state"},           {member_hits_dev, uK * 4, "member_hits"},
                           {confusion_dev, uC * uC * 4, "confusion"}, {pred_out, cap * 8, "pred_out"},
                           {scores_out, cap * uC * 8, "scores_out"},  {scratch, uB * 8, "scratch"}};
  if (vote_check_spans("fst_vote_fold", in, K + 3, out, 6)) return -1;
  VoteArgs a = {};
  for (int k = 0; k < K; ++k) a.logits[k] = logits_host[k];
  a.scale = scale; a.labels = labels; a.valid = (const int*)valid_dev; a.state = (int*)state_dev; a.member_hits = (int*)member_hits_dev;
  a.confusion = (int*)confusion_dev; a.pred_out = pred_out; a.scores_out = scores_out;
  a.row_word = (int*)scratch; a.row_members = (int*)scratch + B;
  a.sharpen = (double)sharpen; a.ld = ld; a.B = (int)B; a.C = C; a.K = K; a.capacity = (int)capacity;
  hipLaunchKernelGGL(vote_rows_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  FST_LAUNCH_CHECK();
  hipLaunchKernelGGL(vote_advance_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  FST_LAUNCH_CHECK();
  return 0;
}
