// The optimizer step behind the encoder/decoder path, as a gfx950 kernel:
//   * fused Adam step over one flat parameter arena (torch.optim.Adam, nn/trainer.py:162-172)
// Bandwidth-bound: no MFMA here.  (The guarded step — clip by global norm, skip bad steps — is gpe_adam_guard.hip.)
#include "gpe_common.h"
#include <math.h>

// =====================================================================================================================
// Adam over a flat arena (torch.optim.Adam semantics, amsgrad off, maximize off):
//   g' = g*gscale + wd*p ; m = b1 m + (1-b1) g' ; v = b2 v + (1-b2) g'^2 ;
//   p -= (lr / bc1) * m / (sqrt(v)/sqrt(bc2) + eps)            bc1 = 1-b1^t, bc2 = 1-b2^t
// zero_grad != 0 also clears g (the next backward writes or accumulates into it).
// =====================================================================================================================
__global__ __launch_bounds__(256) void gpe_adam_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, long n, float lr_over_bc1, float b1,
                                                       float b2, float eps, float wd, float rsqrt_bc2, float gscale,
                                                       int zero_grad, const float* __restrict__ hyper)
{
    const long i4 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= n) return;
    // gpe_adam_step_dev: the two step-dependent scalars come from device memory (a captured launch is replayed with new values)
    if (hyper) { lr_over_bc1 = hyper[0]; rsqrt_bc2 = hyper[1]; }
    if (i4 + 3 < n) {
        float4 pv = *reinterpret_cast<float4*>(p + i4), gv = *reinterpret_cast<float4*>(g + i4);
        float4 mv = *reinterpret_cast<float4*>(m + i4), vv = *reinterpret_cast<float4*>(v + i4);
        float* pp = &pv.x; float* gg = &gv.x; float* mm = &mv.x; float* vq = &vv.x;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float gr = gg[t] * gscale + wd * pp[t];
            mm[t] = b1 * mm[t] + (1.f - b1) * gr;
            vq[t] = b2 * vq[t] + (1.f - b2) * gr * gr;
            pp[t] -= lr_over_bc1 * mm[t] / (sqrtf(vq[t]) * rsqrt_bc2 + eps);
        }
        *reinterpret_cast<float4*>(p + i4) = pv;
        *reinterpret_cast<float4*>(m + i4) = mv;
        *reinterpret_cast<float4*>(v + i4) = vv;
        if (zero_grad) *reinterpret_cast<float4*>(g + i4) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        for (long i = i4; i < n; ++i) {
            const float gr = g[i] * gscale + wd * p[i];
            m[i] = b1 * m[i] + (1.f - b1) * gr;
            v[i] = b2 * v[i] + (1.f - b2) * gr * gr;
            p[i] -= lr_over_bc1 * m[i] / (sqrtf(v[i]) * rsqrt_bc2 + eps);
            if (zero_grad) g[i] = 0.f;
        }
    }
}

extern "C" int gpe_adam_step(float* p, float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                             float eps, float weight_decay, long step, float gscale, int zero_grad, void* stream)
{
    if (!p || !g || !m || !v || n <= 0 || step <= 0 || (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15))
        return GPE_EINVAL;
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    const float lr_over_bc1 = (float)((double)lr / bc1);
    const float rsqrt_bc2 = (float)(1.0 / sqrt(bc2));
    hipLaunchKernelGGL(gpe_adam_kernel, dim3(gpe_cdiv(gpe_cdiv(n, 4), 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n,
                       lr_over_bc1, beta1, beta2, eps, weight_decay, rsqrt_bc2, gscale, zero_grad, (const float*)nullptr);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// the same step with its two step-dependent scalars read from DEVICE memory: hyper[0] = lr / (1 - beta1^step),
// hyper[1] = 1 / sqrt(1 - beta2^step) (gpe_adam_hyper computes them on the host).  For steps replayed from a captured hipGraph,
// where kernel arguments are frozen (gpe_amd/graph.py).
extern "C" int gpe_adam_step_dev(float* p, float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2,
                                 float eps, float weight_decay, float gscale, int zero_grad, void* stream)
{
    if (!p || !g || !m || !v || !hyper || n <= 0 || (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) || (((uintptr_t)hyper) & 3))
        return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_adam_kernel, dim3(gpe_cdiv(gpe_cdiv(n, 4), 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n,
                       0.f, beta1, beta2, eps, weight_decay, 1.f, gscale, zero_grad, hyper);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_adam_hyper(float lr, float beta1, float beta2, long step, float* out_host)
{
    if (!out_host || step <= 0) return GPE_EINVAL;
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    out_host[0] = (float)((double)lr / bc1);
    out_host[1] = (float)(1.0 / sqrt(bc2));
    return GPE_OK;
}
