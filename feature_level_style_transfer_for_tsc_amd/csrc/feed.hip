// Device-resident datasets: the batch of a train step gathered ON THE DEVICE from a data set that was uploaded once, by an epoch
// plan that was uploaded once, so that a replayed hipGraph needs nothing from the host but its launch -- not even its batch.
//
//   fst_feed_batch   copies, for every stream (x_t, y_t, x_s, y_s, ...), the rows that the current plan row names from the
//                    resident source into the caller's destination (a capture's static input), writes the row's scalars (the CPC
//                    start indices, NoiseTransfer's ratios) into theirs, and moves the plan's cursor on.
//
// The cursor is a device word read when the kernels RUN (the window position of the gradient accumulation, guard.hip, works the
// same way): the launch pair is identical for every row of every epoch.  Rows move as 32-bit integers, so every bit pattern
// survives.  House style of guard.hip: the pointer tuples ride by value in the kernel arguments, every argument is validated on the
// host before the first launch, no atomics, and the one-workgroup advance kernel writes the state words from one lane.
#include "fst_common.h"

#define FEED_MAX_STREAMS 8
#define FEED_MAX_SCALARS 8
#define FEED_BX_MAX 2048            // workgroups of a launch at most (256 CUs x 8), spread over the streams; grid-stride beyond

// the state block, in 4-byte int32 words (three more are reserved)
#define FEED_CURSOR 0               // current plan row
#define FEED_STEPS 1                // rows in the plan
#define FEED_FED 2                  // rows served since the block was created
#define FEED_OVERRUN 3              // calls that found cursor >= steps
#define FEED_BAD_INDEX 4            // rows whose index fell outside 0..n_rows-1

struct FeedArgs {
  const uint32_t* src[FEED_MAX_STREAMS];
  uint32_t* dst[FEED_MAX_STREAMS];
  const int32_t* index[FEED_MAX_STREAMS];
  int row_words[FEED_MAX_STREAMS], n_rows[FEED_MAX_STREAMS], batch[FEED_MAX_STREAMS];
  const uint32_t* table[FEED_MAX_SCALARS];
  uint32_t* scalar_dst[FEED_MAX_SCALARS];
  int n_streams, n_scalars;
};
static_assert(sizeof(FeedArgs) + sizeof(int*) <= 4096, "kernel arguments: 4 KB at most");

template <int N>
struct alignas(4 * N) FeedWords {
  uint32_t v[N];
};

__device__ __forceinline__ bool feed_over(int cursor, int steps) { return cursor < 0 || cursor >= steps; }

// The batch of one stream as ONE flat range of units of N words, `upr` of them per row: unit u is piece u % upr of destination row
// u / upr.  A long row so spreads over as many workgroups as it has 256-unit pieces, and short rows pack several to a workgroup.
// The index is unsigned: units < 2^31 and the stride is at most FEED_BX_MAX * 256, so the last increment stays below 2^32.
// An index outside 0..n_rows-1 is compared, never used: its row is left unwritten.
template <int N>
__device__ __forceinline__ void feed_walk(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const int32_t* __restrict__ idx,
                                          int row_words, int n_rows, int batch) {
  const unsigned upr = (unsigned)row_words / N;
  const unsigned units = upr * (unsigned)batch;
  for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
    const unsigned b = u / upr, piece = u - b * upr;
    const int i = idx[b];
    if ((unsigned)i >= (unsigned)n_rows) continue;
    const FeedWords<N>* __restrict__ s = (const FeedWords<N>*)(src + (size_t)i * row_words);
    FeedWords<N>* __restrict__ d = (FeedWords<N>*)(dst + (size_t)b * row_words);
    d[piece] = s[piece];
  }
}

// grid (bx, max(n_streams, 1)).  16-byte units where every row of both sides starts on a 16-byte boundary, dword units otherwise.
__global__ __launch_bounds__(256) void feed_copy_kernel(FeedArgs a, const int* __restrict__ state) {
  const int cursor = state[FEED_CURSOR], steps = state[FEED_STEPS];
  if (feed_over(cursor, steps)) return;
  const int s = blockIdx.y;
  if (s == 0 && blockIdx.x == 0 && (int)threadIdx.x < a.n_scalars)
    a.scalar_dst[threadIdx.x][0] = a.table[threadIdx.x][(size_t)cursor * a.n_scalars + threadIdx.x];
  if (s >= a.n_streams) return;
  const int32_t* idx = a.index[s] + (size_t)cursor * a.batch[s];
  if (a.row_words[s] % 4 == 0 && (((uintptr_t)a.src[s] | (uintptr_t)a.dst[s]) & 15u) == 0)
    feed_walk<4>(a.src[s], a.dst[s], idx, a.row_words[s], a.n_rows[s], a.batch[s]);
  else
    feed_walk<1>(a.src[s], a.dst[s], idx, a.row_words[s], a.n_rows[s], a.batch[s]);
}

// one workgroup, stream-ordered behind the copies of a call: counts the row's bad indices (a fixed-order sum through LDS), then
// lane 0 moves the state on with ordinary stores.  Every lane has read the cursor before the barrier in front of those stores.
__global__ __launch_bounds__(256) void feed_advance_kernel(FeedArgs a, int* __restrict__ state) {
  __shared__ int part[256];
  const int cursor = state[FEED_CURSOR], steps = state[FEED_STEPS];
  const bool over = feed_over(cursor, steps);
  int c = 0;
  if (!over) {
    for (int s = 0; s < a.n_streams; ++s) {
      const int32_t* idx = a.index[s] + (size_t)cursor * a.batch[s];
      for (int b = threadIdx.x; b < a.batch[s]; b += 256) c += (unsigned)idx[b] >= (unsigned)a.n_rows[s];
    }
  }
  part[threadIdx.x] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (over) {
    state[FEED_OVERRUN] += 1;
  } else {
    state[FEED_BAD_INDEX] += part[0];
    state[FEED_FED] += 1;
    state[FEED_CURSOR] = cursor + 1;
  }
}

static bool feed_disjoint(const void* p, uint64_t p_bytes, const void* q, uint64_t q_bytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a + p_bytes <= b || b + q_bytes <= a;
}

extern "C" int fst_feed_batch(const void* const* src_host, void* const* dst_host, const int32_t* const* index_host,
                              const int64_t* row_words_host, const int64_t* n_rows_host, const int64_t* batch_host, int n_streams,
                              const void* const* table_host, void* const* scalar_dst_host, int n_scalars, void* state_dev, void* stream) {
  FST_REQUIRE(n_streams >= 0 && n_streams <= FEED_MAX_STREAMS && n_scalars >= 0 && n_scalars <= FEED_MAX_SCALARS,
              "fst_feed_batch: %d streams and %d scalars; at most %d and %d", n_streams, n_scalars, FEED_MAX_STREAMS, FEED_MAX_SCALARS);
  FST_REQUIRE(n_streams == 0 || (src_host && dst_host && index_host && row_words_host && n_rows_host && batch_host),
              "fst_feed_batch: bad arguments");
  FST_REQUIRE(n_scalars == 0 || (table_host && scalar_dst_host), "fst_feed_batch: bad arguments");
  FST_REQUIRE(state_dev && ((uintptr_t)state_dev & 15) == 0, "fst_feed_batch: null state block, or one off a 16-byte boundary");
  FeedArgs a = {};
  a.n_streams = n_streams; a.n_scalars = n_scalars;
  int64_t units_max = 1;
  for (int s = 0; s < n_streams; ++s) {
    const int64_t rw = row_words_host[s], nr = n_rows_host[s], b = batch_host[s];
    FST_REQUIRE(src_host[s] && dst_host[s] && index_host[s] &&
                (((uintptr_t)src_host[s] | (uintptr_t)dst_host[s] | (uintptr_t)index_host[s]) & 3) == 0,
                "fst_feed_batch: stream %d: null or misaligned pointer", s);
    FST_REQUIRE(rw > 0 && rw < (1LL << 31) && nr > 0 && nr < (1LL << 31) && b > 0 && b < (1LL << 31) && rw * b < (1LL << 31),
                "fst_feed_batch: stream %d: row_words %lld, n_rows %lld, batch %lld (each, and row_words * batch, in 1..2^31 - 1)", s,
                (long long)rw, (long long)nr, (long long)b);
    FST_REQUIRE(feed_disjoint(dst_host[s], (uint64_t)b * rw * 4, src_host[s], (uint64_t)nr * rw * 4),
                "fst_feed_batch: stream %d: the destination overlaps its source", s);
    FST_REQUIRE(feed_disjoint(dst_host[s], (uint64_t)b * rw * 4, state_dev, 32),
                "fst_feed_batch: stream %d: the destination overlaps the state block", s);
    a.src[s] = (const uint32_t*)src_host[s]; a.dst[s] = (uint32_t*)dst_host[s]; a.index[s] = index_host[s];
    a.row_words[s] = (int)rw; a.n_rows[s] = (int)nr; a.batch[s] = (int)b;
    const int64_t units = (rw % 4 == 0 ? rw / 4 : rw) * b;
    units_max = units > units_max ? units : units_max;
  }
  for (int k = 0; k < n_scalars; ++k) {
    FST_REQUIRE(table_host[k] && scalar_dst_host[k] && (((uintptr_t)table_host[k] | (uintptr_t)scalar_dst_host[k]) & 3) == 0,
                "fst_feed_batch: scalar %d: null or misaligned pointer", k);
    FST_REQUIRE(feed_disjoint(scalar_dst_host[k], 4, (const char*)table_host[k] + 4 * k, 4) && feed_disjoint(scalar_dst_host[k], 4, state_dev, 32),
                "fst_feed_batch: scalar %d: the destination overlaps its table or the state block", k);
    a.table[k] = (const uint32_t*)table_host[k]; a.scalar_dst[k] = (uint32_t*)scalar_dst_host[k];
  }
  const int ny = n_streams > 0 ? n_streams : 1;
  int64_t bx = (units_max + 255) / 256;
  const int64_t cap = FEED_BX_MAX / ny;
  bx = bx > cap ? cap : bx;
  hipLaunchKernelGGL(feed_copy_kernel, dim3((unsigned)bx, (unsigned)ny), dim3(256), 0, (hipStream_t)stream, a, (const int*)state_dev);
  FST_LAUNCH_CHECK();
  hipLaunchKernelGGL(feed_advance_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a, (int*)state_dev);
  FST_LAUNCH_CHECK();
  return 0;
}
