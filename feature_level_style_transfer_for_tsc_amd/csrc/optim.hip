// Optimiser updates of the train step as single-pass multi-tensor kernels (train_and_test.py:97-106, 742-754: ten
// torch.optim.RMSprop and one Adam over 770 small tensors).  torch's foreach implementation makes five (RMSprop) to eleven
// (Adam) passes over every tensor, each a separate multi_tensor_apply launch of at most 36-110 tensors: 150 launches and 2 ms
// per step for 36 MB of parameters.  Here a launch takes up to 64 (parameter, gradient, state...) pointer tuples BY VALUE in its
// kernel arguments (no device-side table to build or keep valid under hipGraph replay: the captured launch carries them) and
// makes ONE pass: read p, g and the moments, write p and the moments.  The chunks of a call, the grid of a launch and the test of
// an entry are fst_multi.h's.
//
// Learning rates come in two ways.  fst_rmsprop_multi / fst_adam_multi take them BY VALUE: a captured launch keeps the rate of
// capture day.  fst_rmsprop_multi_dev / fst_adam_multi_dev take DEVICE ADDRESSES of fp32 scalars (one per tensor for RMSprop, one
// per call for Adam, beside its step counter) that the kernel reads when it RUNS: a replayed graph follows whatever a scheduler
// has written there since.  The addresses ride in the kernel arguments like the other pointers (RmspropArgs<const float*>:
// 2 316 B of the 4 KB limit), the load is one uniform 4-byte read per workgroup.
//
// The anomaly guard (csrc/guard.hip writes its VERDICT word, fst_nonfinite_multi) puts the same updates behind that word:
// fst_rmsprop_multi_guard / fst_adam_multi_guard, either rate form.  Each workgroup reads verdict[0] once, a uniform 4-byte load
// when the kernel RUNS, and returns before its first store when the word is non-zero: a step whose gradients hold a NaN or inf
// leaves parameters and moments as they were, under graph replay too.
//
// There is ONE kernel per optimiser, around one update body (rmsprop_update, adam_update): the rate by value or behind an address,
// the verdict pointer null (unguarded) or not.  So equal fp32 rates give bit-identical parameters and moments in either rate form,
// and a clean guarded step gives the bits of the unguarded one.  The six entry points check their own arguments and call the
// optimiser's one host body.
#include "fst_multi.h"

// torch.optim.RMSprop (centered = False, momentum = 0, weight_decay = 0), in torch's operation order:
//   v ← v·α;  v ← v + (1−α)·g·g;  avg = √v + ε;  p ← p + (−lr)·(g / avg)
__device__ __forceinline__ void rmsprop_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ v, int n,
                                               float lr, float alpha, float eps) {
  const float oma = 1.0f - alpha;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float gi = g[i];
    float vi = v[i] * alpha;
    vi = vi + oma * gi * gi;
    v[i] = vi;
    p[i] = p[i] + (-lr) * (gi / (sqrtf(vi) + eps));
  }
}

// torch.optim.Adam (capturable branch, amsgrad = False, weight_decay = 0):
//   m ← β₁m + (1−β₁)g;  v ← β₂v + (1−β₂)g²;  p ← p − (lr / (1−β₁ᵗ)) · m / (√v / √(1−β₂ᵗ) + ε)
__device__ __forceinline__ void adam_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, int n, float step, float lr, float beta1, float beta2, float eps) {
  const float bc1 = 1.0f - powf(beta1, step), bc2s = sqrtf(1.0f - powf(beta2, step));
  const float step_size = lr / bc1;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float gi = g[i];
    const float mi = m[i] * beta1 + (1.0f - beta1) * gi;
    const float vi = v[i] * beta2 + (1.0f - beta2) * gi * gi;
    m[i] = mi; v[i] = vi;
    p[i] = p[i] - step_size * (mi / (sqrtf(vi) / bc2s + eps));
  }
}

// Every (parameter, gradient, state...) tuple of a call, checked before the first chunk is launched.  m_host is NULL for RMSprop,
// lr_dev_host is NULL unless the rates are per-tensor device addresses.
static int optim_validate(const char* who, float* const* p_host, const float* const* g_host, float* const* m_host, float* const* v_host,
                          const int64_t* numel_host, const float* const* lr_dev_host, int n_tensors) {
  for (int i = 0; i < n_tensors; ++i) {
    FST_REQUIRE(fst_multi_entry_ok({p_host[i], g_host[i], m_host ? m_host[i] : p_host[i], v_host[i]}, numel_host[i], 1),
                "%s: tensor %d: null pointer or bad element count", who, i);
    FST_REQUIRE(!lr_dev_host || lr_dev_host[i], "%s: tensor %d: null learning-rate address", who, i);
  }
  return 0;
}

// ---- RMSprop.  LR is the rate carrier: float (by value) or const float* (a DEVICE scalar, read when the kernel runs; several
// tensors may share one)
template <class LR>
struct RmspropArgs {
  float* p[FST_MULTI_T];
  const float* g[FST_MULTI_T];
  float* v[FST_MULTI_T];
  LR lr[FST_MULTI_T];
  int numel[FST_MULTI_T];
  int n;
  float alpha, eps;
};
static_assert(sizeof(RmspropArgs<float>) + sizeof(const int*) <= 4096 && sizeof(RmspropArgs<const float*>) + sizeof(const int*) <= 4096,
              "kernel arguments: 4 KB at most");

__device__ __forceinline__ float rate_of(float lr) { return lr; }
__device__ __forceinline__ float rate_of(const float* lr) { return lr[0]; }
static inline const float* const* rate_addresses(const float*) { return nullptr; }          // by value: nothing to check per tensor
static inline const float* const* rate_addresses(const float* const* lr_dev_host) { return lr_dev_host; }

// verdict == NULL: unguarded
template <class LR>
__global__ __launch_bounds__(256) void rmsprop_multi_kernel(RmspropArgs<LR> a, const int* __restrict__ verdict) {
  const int t = blockIdx.y;
  if (t >= a.n || (verdict && verdict[0] != 0)) return;
  rmsprop_update(a.p[t], a.g[t], a.v[t], a.numel[t], rate_of(a.lr[t]), a.alpha, a.eps);
}

template <class LR>
static int rmsprop_multi(const char* who, float* const* p_host, const float* const* g_host, float* const* v_host,
                         const int64_t* numel_host, const LR* lr_host, int n_tensors, float alpha, float eps, const int32_t* verdict_dev,
                         void* stream) {
  if (int rc = optim_validate(who, p_host, g_host, nullptr, v_host, numel_host, rate_addresses(lr_host), n_tensors)) return rc;
  return fst_multi_chunks(n_tensors, [&](int base, int n) {
    RmspropArgs<LR> a;
    a.n = n; a.alpha = alpha; a.eps = eps;
    for (int i = 0; i < n; ++i) {
      a.p[i] = p_host[base + i]; a.g[i] = g_host[base + i]; a.v[i] = v_host[base + i];
      a.numel[i] = (int)numel_host[base + i]; a.lr[i] = lr_host[base + i];
    }
    hipLaunchKernelGGL(rmsprop_multi_kernel<LR>, fst_multi_grid(numel_host + base, n), dim3(256), 0, (hipStream_t)stream, a,
                       (const int*)verdict_dev);
    FST_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int fst_rmsprop_multi(float* const* p_host, const float* const* g_host, float* const* v_host, const int64_t* numel_host,
                                 const float* lr_host, int n_tensors, float alpha, float eps, void* stream) {
  FST_REQUIRE(p_host && g_host && v_host && numel_host && lr_host && n_tensors >= 0, "fst_rmsprop_multi: bad arguments");
  return rmsprop_multi("fst_rmsprop_multi", p_host, g_host, v_host, numel_host, lr_host, n_tensors, alpha, eps, nullptr, stream);
}

extern "C" int fst_rmsprop_multi_dev(float* const* p_host, const float* const* g_host, float* const* v_host, const int64_t* numel_host,
                                     const float* const* lr_dev_host, int n_tensors, float alpha, float eps, void* stream) {
  FST_REQUIRE(p_host && g_host && v_host && numel_host && lr_dev_host && n_tensors >= 0, "fst_rmsprop_multi_dev: bad arguments");
  return rmsprop_multi("fst_rmsprop_multi_dev", p_host, g_host, v_host, numel_host, lr_dev_host, n_tensors, alpha, eps, nullptr, stream);
}

// the learning rates by value (lr_host) or by device address (lr_dev_host), one of the two
extern "C" int fst_rmsprop_multi_guard(float* const* p_host, const float* const* g_host, float* const* v_host,
                                       const int64_t* numel_host, const float* lr_host, const float* const* lr_dev_host, int n_tensors,
                                       float alpha, float eps, const int32_t* verdict_dev, void* stream) {
  FST_REQUIRE(p_host && g_host && v_host && numel_host && n_tensors >= 0 && verdict_dev, "fst_rmsprop_multi_guard: bad arguments");
  FST_REQUIRE((lr_host != nullptr) != (lr_dev_host != nullptr),
              "fst_rmsprop_multi_guard: the learning rates by value or by device address, one of the two");
  const char* who = "fst_rmsprop_multi_guard";
  return lr_host ? rmsprop_multi(who, p_host, g_host, v_host, numel_host, lr_host, n_tensors, alpha, eps, verdict_dev, stream)
                 : rmsprop_multi(who, p_host, g_host, v_host, numel_host, lr_dev_host, n_tensors, alpha, eps, verdict_dev, stream);
}

// ---- Adam
struct AdamArgs {
  float* p[FST_MULTI_T];
  const float* g[FST_MULTI_T];
  float* m[FST_MULTI_T];
  float* v[FST_MULTI_T];
  int numel[FST_MULTI_T];
  int n;
  const float* step;    // DEVICE scalar: the step count t (already incremented), shared by every tensor
  float lr, beta1, beta2, eps;
};
static_assert(sizeof(AdamArgs) + 2 * sizeof(const void*) <= 4096, "kernel arguments: 4 KB at most");

// lr_dev == NULL: the rate is a.lr; otherwise lr_dev[0], read when the kernel runs.  verdict == NULL: unguarded
__global__ __launch_bounds__(256) void adam_multi_kernel(AdamArgs a, const float* __restrict__ lr_dev, const int* __restrict__ verdict) {
  const int t = blockIdx.y;
  if (t >= a.n || (verdict && verdict[0] != 0)) return;
  adam_update(a.p[t], a.g[t], a.m[t], a.v[t], a.numel[t], a.step[0], lr_dev ? lr_dev[0] : a.lr, a.beta1, a.beta2, a.eps);
}

static int adam_multi(const char* who, float* const* p_host, const float* const* g_host, float* const* m_host, float* const* v_host,
                      const int64_t* numel_host, int n_tensors, const float* step_dev, float lr, const float* lr_dev, float beta1,
                      float beta2, float eps, const int32_t* verdict_dev, void* stream) {
  if (int rc = optim_validate(who, p_host, g_host, m_host, v_host, numel_host, nullptr, n_tensors)) return rc;
  return fst_multi_chunks(n_tensors, [&](int base, int n) {
    AdamArgs a;
    a.n = n; a.step = step_dev; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
    for (int i = 0; i < n; ++i) {
      a.p[i] = p_host[base + i]; a.g[i] = g_host[base + i]; a.m[i] = m_host[base + i]; a.v[i] = v_host[base + i];
      a.numel[i] = (int)numel_host[base + i];
    }
    hipLaunchKernelGGL(adam_multi_kernel, fst_multi_grid(numel_host + base, n), dim3(256), 0, (hipStream_t)stream, a, lr_dev,
                       (const int*)verdict_dev);
    FST_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int fst_adam_multi(float* const* p_host, const float* const* g_host, float* const* m_host, float* const* v_host,
                              const int64_t* numel_host, int n_tensors, const float* step_dev, float lr, float beta1, float beta2,
                              float eps, void* stream) {
  FST_REQUIRE(p_host && g_host && m_host && v_host && numel_host && step_dev && n_tensors >= 0, "fst_adam_multi: bad arguments");
  return adam_multi("fst_adam_multi", p_host, g_host, m_host, v_host, numel_host, n_tensors, step_dev, lr, nullptr, beta1, beta2, eps,
                    nullptr, stream);
}

extern "C" int fst_adam_multi_dev(float* const* p_host, const float* const* g_host, float* const* m_host, float* const* v_host,
                                  const int64_t* numel_host, int n_tensors, const float* step_dev, const float* lr_dev, float beta1,
                                  float beta2, float eps, void* stream) {
  FST_REQUIRE(p_host && g_host && m_host && v_host && numel_host && step_dev && n_tensors >= 0, "fst_adam_multi_dev: bad arguments");
  FST_REQUIRE(lr_dev, "fst_adam_multi_dev: null learning-rate address");
  return adam_multi("fst_adam_multi_dev", p_host, g_host, m_host, v_host, numel_host, n_tensors, step_dev, 0.0f, lr_dev, beta1, beta2,
                    eps, nullptr, stream);
}

// lr_dev == NULL: the rate is lr
extern "C" int fst_adam_multi_guard(float* const* p_host, const float* const* g_host, float* const* m_host, float* const* v_host,
                                    const int64_t* numel_host, int n_tensors, const float* step_dev, float lr, const float* lr_dev,
                                    float beta1, float beta2, float eps, const int32_t* verdict_dev, void* stream) {
  FST_REQUIRE(p_host && g_host && m_host && v_host && numel_host && step_dev && n_tensors >= 0 && verdict_dev,
              "fst_adam_multi_guard: bad arguments");
  return adam_multi("fst_adam_multi_guard", p_host, g_host, m_host, v_host, numel_host, n_tensors, step_dev, lr, lr_dev, beta1, beta2,
                    eps, verdict_dev, stream);
}
