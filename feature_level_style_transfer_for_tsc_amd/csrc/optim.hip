// Optimiser updates of the train step as single-pass multi-tensor kernels (train_and_test.py:97-106, 742-754: ten
// torch.optim.RMSprop and one Adam over 770 small tensors).  torch's foreach implementation makes five (RMSprop) to eleven
// (Adam) passes over every tensor, each a separate multi_tensor_apply launch of at most 36-110 tensors: 150 launches and 2 ms
// per step for 36 MB of parameters.  Here a launch takes up to 64 (parameter, gradient, state...) pointer tuples BY VALUE in its
// kernel arguments (no device-side table to build or keep valid under hipGraph replay: the captured launch carries them) and
// makes ONE pass: read p, g and the moments, write p and the moments.
//
// Learning rates come in two ways.  fst_rmsprop_multi / fst_adam_multi take them BY VALUE: a captured launch keeps the rate of
// capture day.  fst_rmsprop_multi_dev / fst_adam_multi_dev take DEVICE ADDRESSES of fp32 scalars (one per tensor for RMSprop, one
// per call for Adam, beside its step counter) that the kernel reads when it RUNS: a replayed graph follows whatever a scheduler
// has written there since.  The addresses ride in the kernel arguments like the other pointers (RmspropDevArgs: 2 316 B of the
// 4 KB limit), the load is one uniform 4-byte read per workgroup.  Each update body is written once (rmsprop_update,
// adam_update) and called by both kernels, so equal fp32 rates give bit-identical parameters and moments on either path.
#include "fst_common.h"

#define OPT_MAX_T 64

struct RmspropArgs {
  float* p[OPT_MAX_T];
  const float* g[OPT_MAX_T];
  float* v[OPT_MAX_T];
  int numel[OPT_MAX_T];
  float lr[OPT_MAX_T];
  int n;
  float alpha, eps;
};

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

__global__ __launch_bounds__(256) void rmsprop_multi_kernel(RmspropArgs a) {
  const int t = blockIdx.y;
  if (t >= a.n) return;
  rmsprop_update(a.p[t], a.g[t], a.v[t], a.numel[t], a.lr[t], a.alpha, a.eps);
}

struct RmspropDevArgs {
  float* p[OPT_MAX_T];
  const float* g[OPT_MAX_T];
  float* v[OPT_MAX_T];
  const float* lr[OPT_MAX_T];   // DEVICE scalars, read when the kernel runs (several tensors may share one)
  int numel[OPT_MAX_T];
  int n;
  float alpha, eps;
};
static_assert(sizeof(RmspropDevArgs) <= 4096, "kernel arguments: 4 KB at most");

__global__ __launch_bounds__(256) void rmsprop_multi_dev_kernel(RmspropDevArgs a) {
  const int t = blockIdx.y;
  if (t >= a.n) return;
  rmsprop_update(a.p[t], a.g[t], a.v[t], a.numel[t], a.lr[t][0], a.alpha, a.eps);
}

// Every (parameter, gradient, state...) tuple of a call is checked here BEFORE the first chunk is launched: a refused call has
// updated nothing, whichever index the bad entry has.  m_host is NULL for RMSprop, lr_dev_host is NULL unless the rates are
// per-tensor device addresses.
static int optim_validate(const char* who, float* const* p_host, const float* const* g_host, float* const* m_host, float* const* v_host,
                          const int64_t* numel_host, const float* const* lr_dev_host, int n_tensors) {
  for (int i = 0; i < n_tensors; ++i) {
    FST_REQUIRE(p_host[i] && g_host[i] && (!m_host || m_host[i]) && v_host[i] && numel_host[i] > 0 && numel_host[i] < (1LL << 31),
                "%s: tensor %d: null pointer or bad element count", who, i);
    FST_REQUIRE(!lr_dev_host || lr_dev_host[i], "%s: tensor %d: null learning-rate address", who, i);
  }
  return 0;
}

extern "C" int fst_rmsprop_multi(float* const* p_host, const float* const* g_host, float* const* v_host, const int64_t* numel_host,
                                 const float* lr_host, int n_tensors, float alpha, float eps, void* stream) {
  FST_REQUIRE(p_host && g_host && v_host && numel_host && lr_host && n_tensors >= 0, "fst_rmsprop_multi: bad arguments");
  if (int rc = optim_validate("fst_rmsprop_multi", p_host, g_host, nullptr, v_host, numel_host, nullptr, n_tensors)) return rc;
  for (int base = 0; base < n_tensors; base += OPT_MAX_T) {
    RmspropArgs a;
    a.n = n_tensors - base < OPT_MAX_T ? n_tensors - base : OPT_MAX_T;
    a.alpha = alpha; a.eps = eps;
    long long most = 0;
    for (int i = 0; i < a.n; ++i) {
      a.p[i] = p_host[base + i]; a.g[i] = g_host[base + i]; a.v[i] = v_host[base + i];
      a.numel[i] = (int)numel_host[base + i]; a.lr[i] = lr_host[base + i];
      most = most > numel_host[base + i] ? most : numel_host[base + i];
    }
    int bx = (int)((most + 1023) / 1024);                  // four elements per thread for the largest tensor ...
    bx = bx < 1 ? 1 : (bx > 64 ? 64 : bx);                 // ... within 64 workgroups per tensor (grid-stride beyond)
    hipLaunchKernelGGL(rmsprop_multi_kernel, dim3((unsigned)bx, (unsigned)a.n), dim3(256), 0, (hipStream_t)stream, a);
    FST_LAUNCH_CHECK();
  }
  return 0;
}

struct AdamArgs {
  float* p[OPT_MAX_T];
  const float* g[OPT_MAX_T];
  float* m[OPT_MAX_T];
  float* v[OPT_MAX_T];
  int numel[OPT_MAX_T];
  int n;
  const float* step;    // DEVICE scalar: the step count t (already incremented), shared by every tensor
  float lr, beta1, beta2, eps;
};

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

__global__ __launch_bounds__(256) void adam_multi_kernel(AdamArgs a) {
  const int t = blockIdx.y;
  if (t >= a.n) return;
  adam_update(a.p[t], a.g[t], a.m[t], a.v[t], a.numel[t], a.step[0], a.lr, a.beta1, a.beta2, a.eps);
}

// AdamArgs with the learning rate behind a device address: .lr of the struct is unused, lr_dev[0] is read when the kernel runs
__global__ __launch_bounds__(256) void adam_multi_dev_kernel(AdamArgs a, const float* __restrict__ lr_dev) {
  const int t = blockIdx.y;
  if (t >= a.n) return;
  adam_update(a.p[t], a.g[t], a.m[t], a.v[t], a.numel[t], a.step[0], lr_dev[0], a.beta1, a.beta2, a.eps);
}

extern "C" int fst_adam_multi(float* const* p_host, const float* const* g_host, float* const* m_host, float* const* v_host,
                              const int64_t* numel_host, int n_tensors, const float* step_dev, float lr, float beta1, float beta2,
                              float eps, void* stream) {
  FST_REQUIRE(p_host && g_host && m_host && v_host && numel_host && step_dev && n_tensors >= 0, "fst_adam_multi: bad arguments");
  if (int rc = optim_validate("fst_adam_multi", p_host, g_host, m_host, v_host, numel_host, nullptr, n_tensors)) return rc;
  for (int base = 0; base < n_tensors; base += OPT_MAX_T) {
    AdamArgs a;
    a.n = n_tensors - base < OPT_MAX_T ? n_tensors - base : OPT_MAX_T;
    a.step = step_dev; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
    long long most = 0;
    for (int i = 0; i < a.n; ++i) {
      a.p[i] = p_host[base + i]; a.g[i] = g_host[base + i]; a.m[i] = m_host[base + i]; a.v[i] = v_host[base + i];
      a.numel[i] = (int)numel_host[base + i];
      most = most > numel_host[base + i] ? most : numel_host[base + i];
    }
    int bx = (int)((most + 1023) / 1024);
    bx = bx < 1 ? 1 : (bx > 64 ? 64 : bx);
    hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)bx, (unsigned)a.n), dim3(256), 0, (hipStream_t)stream, a);
    FST_LAUNCH_CHECK();
  }
  return 0;
}

// ---- the same two updates with the learning rates on the device (see the head of this file)
extern "C" int fst_rmsprop_multi_dev(float* const* p_host, const float* const* g_host, float* const* v_host, const int64_t* numel_host,
                                     const float* const* lr_dev_host, int n_tensors, float alpha, float eps, void* stream) {
  FST_REQUIRE(p_host && g_host && v_host && numel_host && lr_dev_host && n_tensors >= 0, "fst_rmsprop_multi_dev: bad arguments");
  if (int rc = optim_validate("fst_rmsprop_multi_dev", p_host, g_host, nullptr, v_host, numel_host, lr_dev_host, n_tensors)) return rc;
  for (int base = 0; base < n_tensors; base += OPT_MAX_T) {
    RmspropDevArgs a;
    a.n = n_tensors - base < OPT_MAX_T ? n_tensors - base : OPT_MAX_T;
    a.alpha = alpha; a.eps = eps;
    long long most = 0;
    for (int i = 0; i < a.n; ++i) {
      a.p[i] = p_host[base + i]; a.g[i] = g_host[base + i]; a.v[i] = v_host[base + i];
      a.numel[i] = (int)numel_host[base + i]; a.lr[i] = lr_dev_host[base + i];
      most = most > numel_host[base + i] ? most : numel_host[base + i];
    }
    int bx = (int)((most + 1023) / 1024);
    bx = bx < 1 ? 1 : (bx > 64 ? 64 : bx);
    hipLaunchKernelGGL(rmsprop_multi_dev_kernel, dim3((unsigned)bx, (unsigned)a.n), dim3(256), 0, (hipStream_t)stream, a);
    FST_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int fst_adam_multi_dev(float* const* p_host, const float* const* g_host, float* const* m_host, float* const* v_host,
                                  const int64_t* numel_host, int n_tensors, const float* step_dev, const float* lr_dev, float beta1,
                                  float beta2, float eps, void* stream) {
  FST_REQUIRE(p_host && g_host && m_host && v_host && numel_host && step_dev && n_tensors >= 0, "fst_adam_multi_dev: bad arguments");
  FST_REQUIRE(lr_dev, "fst_adam_multi_dev: null learning-rate address");
  if (int rc = optim_validate("fst_adam_multi_dev", p_host, g_host, m_host, v_host, numel_host, nullptr, n_tensors)) return rc;
  for (int base = 0; base < n_tensors; base += OPT_MAX_T) {
    AdamArgs a;
    a.n = n_tensors - base < OPT_MAX_T ? n_tensors - base : OPT_MAX_T;
    a.step = step_dev; a.lr = 0.0f; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
    long long most = 0;
    for (int i = 0; i < a.n; ++i) {
      a.p[i] = p_host[base + i]; a.g[i] = g_host[base + i]; a.m[i] = m_host[base + i]; a.v[i] = v_host[base + i];
      a.numel[i] = (int)numel_host[base + i];
      most = most > numel_host[base + i] ? most : numel_host[base + i];
    }
    int bx = (int)((most + 1023) / 1024);
    bx = bx < 1 ? 1 : (bx > 64 ? 64 : bx);
    hipLaunchKernelGGL(adam_multi_dev_kernel, dim3((unsigned)bx, (unsigned)a.n), dim3(256), 0, (hipStream_t)stream, a, lr_dev);
    FST_LAUNCH_CHECK();
  }
  return 0;
}

// ---- the same updates behind a device VERDICT word (anomaly guard: csrc/guard.hip writes it, fst_nonfinite_multi).  Each
// workgroup reads verdict[0] once, a uniform 4-byte load when the kernel RUNS, and returns before its first store when the word
// is non-zero: a step whose gradients hold a NaN or inf leaves parameters and moments as they were, under graph replay too.  The
// bodies are rmsprop_update / adam_update, so a clean step gives the bits of the unguarded kernels.  One entry point per
// optimiser serves both learning-rate forms: by value (lr_host / lr) or by device address (lr_dev_host / lr_dev), one of the two.
static_assert(sizeof(RmspropArgs) + sizeof(const int*) <= 4096 && sizeof(RmspropDevArgs) + sizeof(const int*) <= 4096 &&
              sizeof(AdamArgs) + 2 * sizeof(const void*) <= 4096, "kernel arguments: 4 KB at most");

__global__ __launch_bounds__(256) void rmsprop_multi_guard_kernel(RmspropArgs a, const int* __restrict__ verdict) {
  const int t = blockIdx.y;
  if (t >= a.n || verdict[0] != 0) return;
  rmsprop_update(a.p[t], a.g[t], a.v[t], a.numel[t], a.lr[t], a.alpha, a.eps);
}

__global__ __launch_bounds__(256) void rmsprop_multi_dev_guard_kernel(RmspropDevArgs a, const int* __restrict__ verdict) {
  const int t = blockIdx.y;
  if (t >= a.n || verdict[0] != 0) return;
  rmsprop_update(a.p[t], a.g[t], a.v[t], a.numel[t], a.lr[t][0], a.alpha, a.eps);
}

// lr_dev == NULL: the rate is a.lr
__global__ __launch_bounds__(256) void adam_multi_guard_kernel(AdamArgs a, const float* __restrict__ lr_dev,
                                                               const int* __restrict__ verdict) {
  const int t = blockIdx.y;
  if (t >= a.n || verdict[0] != 0) return;
  adam_update(a.p[t], a.g[t], a.m[t], a.v[t], a.numel[t], a.step[0], lr_dev ? lr_dev[0] : a.lr, a.beta1, a.beta2, a.eps);
}

extern "C" int fst_rmsprop_multi_guard(float* const* p_host, const float* const* g_host, float* const* v_host,
                                       const int64_t* numel_host, const float* lr_host, const float* const* lr_dev_host, int n_tensors,
                                       float alpha, float eps, const int32_t* verdict_dev, void* stream) {
  FST_REQUIRE(p_host && g_host && v_host && numel_host && n_tensors >= 0 && verdict_dev, "fst_rmsprop_multi_guard: bad arguments");
  FST_REQUIRE((lr_host != nullptr) != (lr_dev_host != nullptr),
              "fst_rmsprop_multi_guard: the learning rates by value or by device address, one of the two");
  if (int rc = optim_validate("fst_rmsprop_multi_guard", p_host, g_host, nullptr, v_host, numel_host, lr_dev_host, n_tensors)) return rc;
  for (int base = 0; base < n_tensors; base += OPT_MAX_T) {
    const int n = n_tensors - base < OPT_MAX_T ? n_tensors - base : OPT_MAX_T;
    long long most = 0;
    for (int i = 0; i < n; ++i) most = most > numel_host[base + i] ? most : numel_host[base + i];
    int bx = (int)((most + 1023) / 1024);
    bx = bx < 1 ? 1 : (bx > 64 ? 64 : bx);
    const dim3 grid((unsigned)bx, (unsigned)n);
    if (lr_host) {
      RmspropArgs a;
      a.n = n; a.alpha = alpha; a.eps = eps;
      for (int i = 0; i < n; ++i) {
        a.p[i] = p_host[base + i]; a.g[i] = g_host[base + i]; a.v[i] = v_host[base + i];
        a.numel[i] = (int)numel_host[base + i]; a.lr[i] = lr_host[base + i];
      }
      hipLaunchKernelGGL(rmsprop_multi_guard_kernel, grid, dim3(256), 0, (hipStream_t)stream, a, (const int*)verdict_dev);
    } else {
      RmspropDevArgs a;
      a.n = n; a.alpha = alpha; a.eps = eps;
      for (int i = 0; i < n; ++i) {
        a.p[i] = p_host[base + i]; a.g[i] = g_host[base + i]; a.v[i] = v_host[base + i];
        a.numel[i] = (int)numel_host[base + i]; a.lr[i] = lr_dev_host[base + i];
      }
      hipLaunchKernelGGL(rmsprop_multi_dev_guard_kernel, grid, dim3(256), 0, (hipStream_t)stream, a, (const int*)verdict_dev);
    }
    FST_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int fst_adam_multi_guard(float* const* p_host, const float* const* g_host, float* const* m_host, float* const* v_host,
                                    const int64_t* numel_host, int n_tensors, const float* step_dev, float lr, const float* lr_dev,
                                    float beta1, float beta2, float eps, const int32_t* verdict_dev, void* stream) {
  FST_REQUIRE(p_host && g_host && m_host && v_host && numel_host && step_dev && n_tensors >= 0 && verdict_dev,
              "fst_adam_multi_guard: bad arguments");
  if (int rc = optim_validate("fst_adam_multi_guard", p_host, g_host, m_host, v_host, numel_host, nullptr, n_tensors)) return rc;
  for (int base = 0; base < n_tensors; base += OPT_MAX_T) {
    AdamArgs a;
    a.n = n_tensors - base < OPT_MAX_T ? n_tensors - base : OPT_MAX_T;
    a.step = step_dev; a.lr = lr_dev ? 0.0f : lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
    long long most = 0;
    for (int i = 0; i < a.n; ++i) {
      a.p[i] = p_host[base + i]; a.g[i] = g_host[base + i]; a.m[i] = m_host[base + i]; a.v[i] = v_host[base + i];
      a.numel[i] = (int)numel_host[base + i];
      most = most > numel_host[base + i] ? most : numel_host[base + i];
    }
    int bx = (int)((most + 1023) / 1024);
    bx = bx < 1 ? 1 : (bx > 64 ? 64 : bx);
    hipLaunchKernelGGL(adam_multi_guard_kernel, dim3((unsigned)bx, (unsigned)a.n), dim3(256), 0, (hipStream_t)stream, a, lr_dev,
                       (const int*)verdict_dev);
    FST_LAUNCH_CHECK();
  }
  return 0;
}
