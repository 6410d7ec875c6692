// mnrf_optim.hip -- Adam over one flat parameter tensor (training.FlatAdam); SGD and RAdam in the same shape further down
// (training.FlatSGD, training.FlatRAdam).
//
// torch's fused Adam is a multi-tensor kernel that deals 65 536-element chunks to 512-thread blocks: the 595 k parameters of
// a field model are TEN blocks on a 256-CU device, 46 us per model and step, for 9.5 MB of traffic.  Here: one thread per four
// elements, float4 accesses, the same update (torch/optim/adam.py _single_tensor_adam, non-amsgrad, L2 weight decay), the same
// found_inf / grad_scale contract as GradScaler's (torch/optim/_functional + fused_adam_utils.cuh: a step with found_inf != 0
// changes nothing and does not count).  Its arithmetic: the bias corrections, 1 - beta1 and 1 - beta2 are formed in double from
// the double betas and rounded to float once (1.f - (float)0.999 is 1.3e-5 off 1 - 0.999); per element everything is float, one
// rounding per operation, and BOTH moments are updated as x + (1 - beta)(new - x).  The betas themselves are never used in
// float: (float)beta2 and (float)(1 - beta2) do not sum to one (1.3e-8 over), and exp_avg_sq of beta2 * v + (1 - beta2) g^2
// with the two rounded apart settles 1.3e-5 above g^2 -- the weights of the form used here sum to one by construction.
// Held to a float64 restatement by tests/test_hip_adam_fp64.py (tests/adam_ref.py).
// Reference: train.py:101-109 builds torch.optim.Adam through utils/__init__.py get_optimizer; this is the same update.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mnrf.h"
#include "mnrf_error.h"

namespace mnrf {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct AdamArgs {
    float* p; const float* g; float* m; float* v;
    long long n;
    float lr, eps, wd;
    double beta1, beta2;
    long long step;            // the host's count of step() calls, this one included
    int* skipped;              // device: how many of them found_inf has skipped so far
    const float* grad_scale;   // device scalars or null
    const float* found_inf;
    // mnrf_adam_step_dev: every scalar of the step comes from a device block written by adam_prep_kernel (a step captured in a hipGraph
    // must not freeze them): MNRF_ADAM_STATE_FLOATS floats [veto, lr / bias correction 1, sqrt(bias correction 2), 1 - beta1,
    // 1 - beta2, 1 / grad_scale, eps, weight_decay]
    const float* state;
};

__device__ __forceinline__ void adam_body(AdamArgs A) {
    // thread 0 reads the scalars of the step once per block and leaves what the others need in LDS
    __shared__ float sh[MNRF_ADAM_STATE_FLOATS];
    if (threadIdx.x == 0) {
        if (A.state) {
#pragma unroll
            for (int i = 0; i < MNRF_ADAM_STATE_FLOATS; ++i) sh[i] = A.state[i];
        } else {
            const bool veto = A.found_inf && *A.found_inf != 0.f;
            const long long eff = A.step - (long long)*A.skipped;      // >= 1 when the caller counts as documented
            const double t = (double)(eff < 1 ? 1 : eff);
            sh[0] = veto ? 1.f : 0.f;
            sh[1] = A.lr / (float)(1.0 - pow(A.beta1, t));
            sh[2] = (float)sqrt(1.0 - pow(A.beta2, t));
            sh[3] = (float)(1.0 - A.beta1);      // (in double, rounded once: the weights of the new gradient in the two moments)
            sh[4] = (float)(1.0 - A.beta2);
            sh[5] = A.grad_scale ? 1.f / *A.grad_scale : 1.f;
            sh[6] = A.eps;
            sh[7] = A.wd;
        }
    }
    __syncthreads();
    if (sh[0] != 0.f) {      // the whole grid leaves; one thread records that this call did not count
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(A.skipped, 1);
        return;
    }
    const float step_size = sh[1];
    const float bc2_sqrt = sh[2];
    const float omb1 = sh[3], omb2 = sh[4];
    const float inv_scale = sh[5];
    const bool scaled = sh[5] != 1.f;
    A.eps = sh[6];
    A.wd = sh[7];
    const long long i4 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= A.n) return;
    const bool full = i4 + 4 <= A.n;
    float p[4], g[4], m[4], v[4];
    if (full) {
        const f32x4 P = *(const f32x4*)(A.p + i4), G = *(const f32x4*)(A.g + i4), M = *(const f32x4*)(A.m + i4), V = *(const f32x4*)(A.v + i4);
#pragma unroll
        for (int c = 0; c < 4; ++c) { p[c] = P[c]; g[c] = G[c]; m[c] = M[c]; v[c] = V[c]; }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const bool in = i4 + c < A.n;
            p[c] = in ? A.p[i4 + c] : 0.f; g[c] = in ? A.g[i4 + c] : 0.f; m[c] = in ? A.m[i4 + c] : 0.f; v[c] = in ? A.v[i4 + c] : 0.f;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float gr = scaled ? g[c] * inv_scale : g[c];
        if (A.wd != 0.f) gr = gr + A.wd * p[c];
        m[c] = m[c] + omb1 * (gr - m[c]);                          // lerp(exp_avg, grad, 1 - beta1)
        v[c] = v[c] + omb2 * (gr * gr - v[c]);                     // exp_avg_sq * beta2 + (1 - beta2) grad^2, as a lerp too
        const float denom = sqrtf(v[c]) / bc2_sqrt + A.eps;
        p[c] = p[c] - step_size * (m[c] / denom);
    }
    if (full) {
        *(f32x4*)(A.p + i4) = f32x4{p[0], p[1], p[2], p[3]};
        *(f32x4*)(A.m + i4) = f32x4{m[0], m[1], m[2], m[3]};
        *(f32x4*)(A.v + i4) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (i4 + c < A.n) { A.p[i4 + c] = p[c]; A.m[i4 + c] = m[c]; A.v[i4 + c] = v[c]; }
    }
}


__global__ void adam_kernel(AdamArgs A) { adam_body(A); }

// the same for up to ADAM_BATCH flat tensors in one launch (blockIdx.y = tensor): a training step updates its coarse and its fine
// model behind ONE prep launch (mnrf_adam_step_dev_n)
constexpr int ADAM_BATCH = 4;
struct AdamBatch {
    AdamArgs a[ADAM_BATCH];
};
__global__ void adam_batch_kernel(AdamBatch B) { adam_body(B.a[blockIdx.y]); }

}  // namespace mnrf

extern "C" int mnrf_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, double beta1,
                              double beta2, float eps, float weight_decay, int64_t step, int32_t* skipped, const float* grad_scale,
                              const float* found_inf, void* stream) {
    using namespace mnrf;
    if (!param || !grad || !exp_avg || !exp_avg_sq || !skipped) return mnrf_fail(MNRF_ERR_ARG, "mnrf_adam_step: null pointer");
    if (n < 0 || step < 1) return mnrf_fail(MNRF_ERR_ARG, "mnrf_adam_step: n >= 0, step >= 1");
    if (n == 0) return MNRF_OK;
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_adam_step: tensors must be 16-byte aligned");
    AdamArgs A{param, grad, exp_avg, exp_avg_sq, (long long)n, lr, eps, weight_decay, beta1, beta2, (long long)step, skipped, grad_scale, found_inf,
               nullptr};
    const long long threads = (n + 3) / 4;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_adam_step");
}

// ---- the same update with every scalar in device memory (a step captured in a hipGraph must not freeze the learning rate or the
// step count).  mnrf_adam_prep: one thread -- *step += 1, then the scalars of this step -> state[MNRF_ADAM_STATE_FLOATS];
// mnrf_adam_step_dev: the update.
namespace mnrf {
struct AdamPrepArgs {
    const double* hyper; long long* step; const int* skipped; const float* grad_scale; const float* found_inf;
    const unsigned* guard[4]; int n_guard; float* state;
};
__global__ void adam_prep_kernel(AdamPrepArgs P) {
    const long long step = *P.step + 1;
    *P.step = step;
    bool veto = P.found_inf && *P.found_inf != 0.f;
    for (int i = 0; i < P.n_guard; ++i) veto |= *P.guard[i] != 0u;      // a range-guard word of this step's launches (mnrf.h MNRF_GUARD_*)
    const float lr = (float)P.hyper[0], eps = (float)P.hyper[3], wd = (float)P.hyper[4];
    const double beta1 = P.hyper[1], beta2 = P.hyper[2];
    const long long eff = step - (long long)*P.skipped;
    const double t = (double)(eff < 1 ? 1 : eff);
    P.state[0] = veto ? 1.f : 0.f;
    P.state[1] = lr / (float)(1.0 - pow(beta1, t));
    P.state[2] = (float)sqrt(1.0 - pow(beta2, t));
    P.state[3] = (float)(1.0 - beta1);
    P.state[4] = (float)(1.0 - beta2);
    P.state[5] = P.grad_scale ? 1.f / *P.grad_scale : 1.f;
    P.state[6] = eps;
    P.state[7] = wd;
}
}  // namespace mnrf

extern "C" int mnrf_adam_prep(const double* hyper, int64_t* step, const int32_t* skipped, const float* grad_scale, const float* found_inf,
                              const uint32_t* const* guard_words, int n_guard_words, float* state, void* stream) {
    using namespace mnrf;
    if (!hyper || !step || !skipped || !state) return mnrf_fail(MNRF_ERR_ARG, "mnrf_adam_prep: null pointer");
    if (n_guard_words < 0 || n_guard_words > 4 || (n_guard_words > 0 && !guard_words))
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_adam_prep: 0..4 guard words");
    AdamPrepArgs P{hyper, (long long*)step, skipped, grad_scale, found_inf, {nullptr, nullptr, nullptr, nullptr}, n_guard_words, state};
    for (int i = 0; i < n_guard_words; ++i) {
        if (!guard_words[i]) return mnrf_fail(MNRF_ERR_ARG, "mnrf_adam_prep: null guard word");
        P.guard[i] = guard_words[i];
    }
    hipLaunchKernelGGL(adam_prep_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, P);
    return mnrf_check_launch("mnrf_adam_prep");
}

extern "C" int mnrf_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* state,
                                  int32_t* skipped, void* stream) {
    using namespace mnrf;
    if (!param || !grad || !exp_avg || !exp_avg_sq || !skipped || !state) return mnrf_fail(MNRF_ERR_ARG, "mnrf_adam_step_dev: null pointer");
    if (n < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_adam_step_dev: n >= 0");
    if (n == 0) return MNRF_OK;
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_adam_step_dev: tensors must be 16-byte aligned");
    AdamArgs A{param, grad, exp_avg, exp_avg_sq, (long long)n, 0.f, 0.f, 0.f, 0.0, 0.0, 1, skipped, nullptr, nullptr, state};
    const long long threads = (n + 3) / 4;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_adam_step_dev");
}

extern "C" int mnrf_adam_step_dev_n(int n_tensors, float* const* param, const float* const* grad, float* const* exp_avg,
                                    float* const* exp_avg_sq, const int64_t* n, const float* state, int32_t* const* skipped, void* stream) {
    using namespace mnrf;
    if (n_tensors < 0 || n_tensors > ADAM_BATCH) return mnrf_fail(MNRF_ERR_ARG, "mnrf_adam_step_dev_n: 0..4 tensors per call");
    if (n_tensors == 0) return MNRF_OK;
    if (!param || !grad || !exp_avg || !exp_avg_sq || !n || !skipped || !state) return mnrf_fail(MNRF_ERR_ARG, "mnrf_adam_step_dev_n: null pointer");
    AdamBatch B{};
    long long most = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (!param[t] || !grad[t] || !exp_avg[t] || !exp_avg_sq[t] || !skipped[t]) return mnrf_fail(MNRF_ERR_ARG, "mnrf_adam_step_dev_n: null pointer");
        if (n[t] < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_adam_step_dev_n: n >= 0");
        if (((uintptr_t)param[t] | (uintptr_t)grad[t] | (uintptr_t)exp_avg[t] | (uintptr_t)exp_avg_sq[t]) & 15)
            return mnrf_fail(MNRF_ERR_ARG, "mnrf_adam_step_dev_n: tensors must be 16-byte aligned");
        B.a[t] = AdamArgs{param[t], grad[t], exp_avg[t], exp_avg_sq[t], (long long)n[t], 0.f, 0.f, 0.f, 0.0, 0.0, 1, skipped[t], nullptr, nullptr, state};
        most = n[t] > most ? n[t] : most;
    }
    if (most == 0) return MNRF_OK;
    const long long threads = (most + 3) / 4;
    hipLaunchKernelGGL(adam_batch_kernel, dim3((unsigned)((threads + 255) / 256), n_tensors), dim3(256), 0, (hipStream_t)stream, B);
    return mnrf_check_launch("mnrf_adam_step_dev_n");
}

// ---- SGD with momentum and RAdam over one flat tensor (training.FlatSGD, training.FlatRAdam): adam_body's shape -- one thread
// per four elements, float4 accesses, a ragged tail, the scalars of the step read once per block by thread 0 -- and its contract:
// a vetoed call changes nothing and adds one to *skipped, the step the scalars are made for is step - *skipped, at least 1.
// Each in two forms, as Adam: host scalars (mnrf_sgd_step, mnrf_radam_step), or every scalar from a device block that a
// one-thread launch publishes (mnrf_sgd_prep, mnrf_radam_prep) in front of one update launch for up to four tensors
// (mnrf_sgd_step_dev_n, mnrf_radam_step_dev_n).  Held to float64 restatements by tests/test_hip_optim_fp64.py (tests/optim_ref.py).
// Reference: utils/__init__.py:47-74 get_optimizer builds torch.optim.SGD and torch_optimizer.RAdam; these are torch.optim's updates.
namespace mnrf {

constexpr int OPT_BATCH = 4;

__device__ __forceinline__ void load4(const float* a, long long i4, long long n, bool full, float (&x)[4]) {
    if (full) {
        const f32x4 X = *(const f32x4*)(a + i4);
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = X[c];
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = i4 + c < n ? a[i4 + c] : 0.f;
    }
}

__device__ __forceinline__ void store4(float* a, long long i4, long long n, bool full, const float (&x)[4]) {
    if (full) {
        *(f32x4*)(a + i4) = f32x4{x[0], x[1], x[2], x[3]};
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (i4 + c < n) a[i4 + c] = x[c];
    }
}

__device__ __forceinline__ bool opt_veto(const float* found_inf, const unsigned* const* guard, int n_guard) {
    bool veto = found_inf && *found_inf != 0.f;
    for (int i = 0; i < n_guard; ++i) veto |= *guard[i] != 0u;      // a range-guard word of this step's launches (mnrf.h MNRF_GUARD_*)
    return veto;
}

// ---- SGD (torch/optim/sgd.py _single_tensor_sgd: dampening 0, no Nesterov, L2 weight decay; `grad / grad_scale` first as the fused
// path does): G = g / grad_scale + wd p, buf' = momentum buf + G, p' = p - lr buf'.  A zero-initialised buffer makes the first step
// torch's buf = G (momentum * 0 + G is G exactly).  Nothing in it depends on the step; lr, momentum and wd are floats.  G rounds
// once per operation; the two updates are one fused multiply-add each, fmaf(momentum, buf, G) and fmaf(-lr, buf', p), one rounding
// each -- as torch's fused SGD kernel computes them (the compiler contracts its a * b + c), and for the reason it matters: where
// momentum * buf cancels against G, a product rounded apart leaves its rounding error, u |momentum buf|, in a buffer that is now
// small, and the momentum carries that on (measured over twenty steps: 9577 against 1300 units of u * scale in the buffer).
// state: MNRF_SGD_STATE_FLOATS floats [veto, lr, momentum, 1 / grad_scale, weight_decay]
struct SgdArgs {
    float* p; const float* g; float* buf;
    long long n;
    float lr, momentum, wd;
    int* skipped;
    const float* grad_scale;
    const float* found_inf;
    const float* state;        // null: the scalars above; else mnrf_sgd_prep's block
};

__device__ __forceinline__ void sgd_scalars(float* out, bool veto, float lr, float momentum, float wd, const float* grad_scale) {
    out[0] = veto ? 1.f : 0.f;
    out[1] = lr;
    out[2] = momentum;
    out[3] = grad_scale ? 1.f / *grad_scale : 1.f;
    out[4] = wd;
}

__device__ __forceinline__ void sgd_body(SgdArgs A) {
    __shared__ float sh[MNRF_SGD_STATE_FLOATS];
    if (threadIdx.x == 0) {
        if (A.state) {
#pragma unroll
            for (int i = 0; i < MNRF_SGD_STATE_FLOATS; ++i) sh[i] = A.state[i];
        } else {
            sgd_scalars(sh, opt_veto(A.found_inf, nullptr, 0), A.lr, A.momentum, A.wd, A.grad_scale);
        }
    }
    __syncthreads();
    if (sh[0] != 0.f) {      // the whole grid leaves; one thread records that this call did not count
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(A.skipped, 1);
        return;
    }
    const float lr = sh[1], mu = sh[2], inv_scale = sh[3], wd = sh[4];
    const bool scaled = inv_scale != 1.f;
    const long long i4 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= A.n) return;
    const bool full = i4 + 4 <= A.n;
    float p[4], g[4], b[4];
    load4(A.p, i4, A.n, full, p);
    load4(A.g, i4, A.n, full, g);
    load4(A.buf, i4, A.n, full, b);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float gr = scaled ? g[c] * inv_scale : g[c];
        if (wd != 0.f) gr = gr + wd * p[c];
        b[c] = fmaf(mu, b[c], gr);              // one rounding: where momentum * buf cancels against G nothing of the product's is left
        p[c] = fmaf(-lr, b[c], p[c]);
    }
    store4(A.p, i4, A.n, full, p);
    store4(A.buf, i4, A.n, full, b);
}

struct SgdBatch {
    SgdArgs a[OPT_BATCH];
};
__global__ void sgd_kernel(SgdArgs A) { sgd_body(A); }
__global__ void sgd_batch_kernel(SgdBatch B) { sgd_body(B.a[blockIdx.y]); }

struct OptPrepArgs {
    const double* hyper; long long* step; const int* skipped; const float* grad_scale; const float* found_inf;
    const unsigned* guard[4]; int n_guard; float* state;
};

__global__ void sgd_prep_kernel(OptPrepArgs P) {
    *P.step = *P.step + 1;
    sgd_scalars(P.state, opt_veto(P.found_inf, P.guard, P.n_guard), (float)P.hyper[0], (float)P.hyper[1], (float)P.hyper[2], P.grad_scale);
}

// ---- RAdam (torch/optim/radam.py _single_tensor_radam, decoupled_weight_decay=False), for the effective step t:
//     G = g / grad_scale + wd p,  m' = m + (1 - beta1)(G - m),  v' = v + (1 - beta2)(G^2 - v)
//     rho_inf = 2 / (1 - beta2) - 1,  rho_t = rho_inf - 2 t beta2^t / (1 - beta2^t)
//     rho_t > 5:  p' = p - lr / (1 - beta1^t) * sqrt(1 - beta2^t) r_t * m' / (sqrt(v') + eps),
//                 r_t = sqrt((rho_t - 4)(rho_t - 2) rho_inf / ((rho_inf - 4)(rho_inf - 2) rho_t))
//     else:       p' = p - lr / (1 - beta1^t) * m'
// Every step-dependent scalar is formed in double and rounded to float once: 1 - beta1^t (lr, a float, is divided by it in
// float, as Adam's step size is), the product sqrt(1 - beta2^t) r_t, 1 - beta1, 1 - beta2; rho_t > 5 is decided in double, by the
// thread that forms the scalars -- on the device count in the prep launch, so a captured step changes branch by itself.  Per
// element: a = (lr / bc1) * (sqrt(bc2) r_t) (the same two floats in every thread), p' = p - a * (m' / (sqrt(v') + eps)), or
// p' = p - (lr / bc1) * m'; one rounding per operation.
// state: MNRF_RADAM_STATE_FLOATS floats [veto, lr / bias correction 1, sqrt(bias correction 2) r_t (0 where not rectified),
// 1 - beta1, 1 - beta2, 1 / grad_scale, eps, weight_decay, rectified (1 or 0)]
struct RadamArgs {
    float* p; const float* g; float* m; float* v;
    long long n;
    float lr, eps, wd;
    double beta1, beta2;
    long long step;
    int* skipped;
    const float* grad_scale;
    const float* found_inf;
    const float* state;
};

__device__ __forceinline__ void radam_scalars(float* out, bool veto, float lr, double beta1, double beta2, float eps, float wd, long long step,
                                              int skipped, const float* grad_scale) {
    const long long eff = step - (long long)skipped;
    const double t = (double)(eff < 1 ? 1 : eff);
    const double b2t = pow(beta2, t);
    const double bc2 = 1.0 - b2t;
    const double rho_inf = 2.0 / (1.0 - beta2) - 1.0;
    const double rho_t = rho_inf - 2.0 * t * b2t / bc2;
    const bool rect = rho_t > 5.0;
    out[0] = veto ? 1.f : 0.f;
    out[1] = lr / (float)(1.0 - pow(beta1, t));
    out[2] = rect ? (float)(sqrt(bc2) * sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t))) : 0.f;
    out[3] = (float)(1.0 - beta1);
    out[4] = (float)(1.0 - beta2);
    out[5] = grad_scale ? 1.f / *grad_scale : 1.f;
    out[6] = eps;
    out[7] = wd;
    out[8] = rect ? 1.f : 0.f;
}

__device__ __forceinline__ void radam_body(RadamArgs A) {
    __shared__ float sh[MNRF_RADAM_STATE_FLOATS];
    if (threadIdx.x == 0) {
        if (A.state) {
#pragma unroll
            for (int i = 0; i < MNRF_RADAM_STATE_FLOATS; ++i) sh[i] = A.state[i];
        } else {
            radam_scalars(sh, opt_veto(A.found_inf, nullptr, 0), A.lr, A.beta1, A.beta2, A.eps, A.wd, A.step, *A.skipped, A.grad_scale);
        }
    }
    __syncthreads();
    if (sh[0] != 0.f) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(A.skipped, 1);
        return;
    }
    const float step_size = sh[1];
    const float a = step_size * sh[2];
    const float omb1 = sh[3], omb2 = sh[4];
    const float inv_scale = sh[5], eps = sh[6], wd = sh[7];
    const bool scaled = inv_scale != 1.f;
    const bool rect = sh[8] != 0.f;
    const long long i4 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= A.n) return;
    const bool full = i4 + 4 <= A.n;
    float p[4], g[4], m[4], v[4];
    load4(A.p, i4, A.n, full, p);
    load4(A.g, i4, A.n, full, g);
    load4(A.m, i4, A.n, full, m);
    load4(A.v, i4, A.n, full, v);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float gr = scaled ? g[c] * inv_scale : g[c];
        if (wd != 0.f) gr = gr + wd * p[c];
        m[c] = m[c] + omb1 * (gr - m[c]);
        v[c] = v[c] + omb2 * (gr * gr - v[c]);
        p[c] = rect ? p[c] - a * (m[c] / (sqrtf(v[c]) + eps)) : p[c] - step_size * m[c];
    }
    store4(A.p, i4, A.n, full, p);
    store4(A.m, i4, A.n, full, m);
    store4(A.v, i4, A.n, full, v);
}

struct RadamBatch {
    RadamArgs a[OPT_BATCH];
};
__global__ void radam_kernel(RadamArgs A) { radam_body(A); }
__global__ void radam_batch_kernel(RadamBatch B) { radam_body(B.a[blockIdx.y]); }

// hyper = [lr, beta1, beta2, eps, weight_decay], FlatAdam's block
__global__ void radam_prep_kernel(OptPrepArgs P) {
    const long long step = *P.step + 1;
    *P.step = step;
    radam_scalars(P.state, opt_veto(P.found_inf, P.guard, P.n_guard), (float)P.hyper[0], P.hyper[1], P.hyper[2], (float)P.hyper[3],
                  (float)P.hyper[4], step, *P.skipped, P.grad_scale);
}

static int opt_fail(const char* what, const char* msg) {
    char text[160];
    snprintf(text, sizeof(text), "%s: %s", what, msg);
    return mnrf_fail(MNRF_ERR_ARG, text);
}

// the checks and the launch of a prep kernel (what), shared by the two
template <class K>
static int opt_prep(K kernel, const char* what, const double* hyper, int64_t* step, const int32_t* skipped, const float* grad_scale,
                    const float* found_inf, const uint32_t* const* guard_words, int n_guard_words, float* state, void* stream) {
    if (!hyper || !step || !skipped || !state) return opt_fail(what, "null pointer");
    if (n_guard_words < 0 || n_guard_words > 4 || (n_guard_words > 0 && !guard_words)) return opt_fail(what, "0..4 guard words");
    OptPrepArgs P{hyper, (long long*)step, skipped, grad_scale, found_inf, {nullptr, nullptr, nullptr, nullptr}, n_guard_words, state};
    for (int i = 0; i < n_guard_words; ++i) {
        if (!guard_words[i]) return opt_fail(what, "null guard word");
        P.guard[i] = guard_words[i];
    }
    hipLaunchKernelGGL(kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, P);
    return mnrf_check_launch(what);
}

static inline dim3 opt_grid(long long n, int n_tensors) { return dim3((unsigned)(((n + 3) / 4 + 255) / 256), (unsigned)n_tensors); }

}  // namespace mnrf

extern "C" int mnrf_sgd_step(float* param, const float* grad, float* momentum_buffer, int64_t n, float lr, float momentum, float weight_decay,
                             int64_t step, int32_t* skipped, const float* grad_scale, const float* found_inf, void* stream) {
    using namespace mnrf;
    if (!param || !grad || !momentum_buffer || !skipped) return mnrf_fail(MNRF_ERR_ARG, "mnrf_sgd_step: null pointer");
    if (n < 0 || step < 1) return mnrf_fail(MNRF_ERR_ARG, "mnrf_sgd_step: n >= 0, step >= 1");
    if (n == 0) return MNRF_OK;
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)momentum_buffer) & 15)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_sgd_step: tensors must be 16-byte aligned");
    SgdArgs A{param, grad, momentum_buffer, (long long)n, lr, momentum, weight_decay, skipped, grad_scale, found_inf, nullptr};
    hipLaunchKernelGGL(sgd_kernel, opt_grid(n, 1), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_sgd_step");
}

extern "C" int mnrf_sgd_prep(const double* hyper, int64_t* step, const int32_t* skipped, const float* grad_scale, const float* found_inf,
                             const uint32_t* const* guard_words, int n_guard_words, float* state, void* stream) {
    return mnrf::opt_prep(mnrf::sgd_prep_kernel, "mnrf_sgd_prep", hyper, step, skipped, grad_scale, found_inf, guard_words, n_guard_words, state,
                          stream);
}

extern "C" int mnrf_sgd_step_dev_n(int n_tensors, float* const* param, const float* const* grad, float* const* momentum_buffer,
                                   const int64_t* n, const float* state, int32_t* const* skipped, void* stream) {
    using namespace mnrf;
    if (n_tensors < 0 || n_tensors > OPT_BATCH) return mnrf_fail(MNRF_ERR_ARG, "mnrf_sgd_step_dev_n: 0..4 tensors per call");
    if (n_tensors == 0) return MNRF_OK;
    if (!param || !grad || !momentum_buffer || !n || !skipped || !state) return mnrf_fail(MNRF_ERR_ARG, "mnrf_sgd_step_dev_n: null pointer");
    SgdBatch B{};
    long long most = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (!param[t] || !grad[t] || !momentum_buffer[t] || !skipped[t]) return mnrf_fail(MNRF_ERR_ARG, "mnrf_sgd_step_dev_n: null pointer");
        if (n[t] < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_sgd_step_dev_n: n >= 0");
        if (((uintptr_t)param[t] | (uintptr_t)grad[t] | (uintptr_t)momentum_buffer[t]) & 15)
            return mnrf_fail(MNRF_ERR_ARG, "mnrf_sgd_step_dev_n: tensors must be 16-byte aligned");
        B.a[t] = SgdArgs{param[t], grad[t], momentum_buffer[t], (long long)n[t], 0.f, 0.f, 0.f, skipped[t], nullptr, nullptr, state};
        most = n[t] > most ? n[t] : most;
    }
    if (most == 0) return MNRF_OK;
    hipLaunchKernelGGL(sgd_batch_kernel, opt_grid(most, n_tensors), dim3(256), 0, (hipStream_t)stream, B);
    return mnrf_check_launch("mnrf_sgd_step_dev_n");
}

extern "C" int mnrf_radam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, double beta1,
                               double beta2, float eps, float weight_decay, int64_t step, int32_t* skipped, const float* grad_scale,
                               const float* found_inf, void* stream) {
    using namespace mnrf;
    if (!param || !grad || !exp_avg || !exp_avg_sq || !skipped) return mnrf_fail(MNRF_ERR_ARG, "mnrf_radam_step: null pointer");
    if (n < 0 || step < 1) return mnrf_fail(MNRF_ERR_ARG, "mnrf_radam_step: n >= 0, step >= 1");
    if (n == 0) return MNRF_OK;
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_radam_step: tensors must be 16-byte aligned");
    RadamArgs A{param, grad, exp_avg, exp_avg_sq, (long long)n, lr, eps, weight_decay, beta1, beta2, (long long)step, skipped, grad_scale, found_inf,
                nullptr};
    hipLaunchKernelGGL(radam_kernel, opt_grid(n, 1), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_radam_step");
}

extern "C" int mnrf_radam_prep(const double* hyper, int64_t* step, const int32_t* skipped, const float* grad_scale, const float* found_inf,
                               const uint32_t* const* guard_words, int n_guard_words, float* state, void* stream) {
    return mnrf::opt_prep(mnrf::radam_prep_kernel, "mnrf_radam_prep", hyper, step, skipped, grad_scale, found_inf, guard_words, n_guard_words,
                          state, stream);
}

extern "C" int mnrf_radam_step_dev_n(int n_tensors, float* const* param, const float* const* grad, float* const* exp_avg,
                                     float* const* exp_avg_sq, const int64_t* n, const float* state, int32_t* const* skipped, void* stream) {
    using namespace mnrf;
    if (n_tensors < 0 || n_tensors > OPT_BATCH) return mnrf_fail(MNRF_ERR_ARG, "mnrf_radam_step_dev_n: 0..4 tensors per call");
    if (n_tensors == 0) return MNRF_OK;
    if (!param || !grad || !exp_avg || !exp_avg_sq || !n || !skipped || !state) return mnrf_fail(MNRF_ERR_ARG, "mnrf_radam_step_dev_n: null pointer");
    RadamBatch B{};
    long long most = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (!param[t] || !grad[t] || !exp_avg[t] || !exp_avg_sq[t] || !skipped[t]) return mnrf_fail(MNRF_ERR_ARG, "mnrf_radam_step_dev_n: null pointer");
        if (n[t] < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_radam_step_dev_n: n >= 0");
        if (((uintptr_t)param[t] | (uintptr_t)grad[t] | (uintptr_t)exp_avg[t] | (uintptr_t)exp_avg_sq[t]) & 15)
            return mnrf_fail(MNRF_ERR_ARG, "mnrf_radam_step_dev_n: tensors must be 16-byte aligned");
        B.a[t] = RadamArgs{param[t], grad[t], exp_avg[t], exp_avg_sq[t], (long long)n[t], 0.f, 0.f, 0.f, 0.0, 0.0, 1, skipped[t], nullptr, nullptr, state};
        most = n[t] > most ? n[t] : most;
    }
    if (most == 0) return MNRF_OK;
    hipLaunchKernelGGL(radam_batch_kernel, opt_grid(most, n_tensors), dim3(256), 0, (hipStream_t)stream, B);
    return mnrf_check_launch("mnrf_radam_step_dev_n");
}
