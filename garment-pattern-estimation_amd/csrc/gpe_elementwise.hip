// Small element-wise helpers of the path for gfx950: scale (factor on the host or on the device), add, the sum over an inner
// axis, and the input standardisation (nn/data/transforms.py:35-50).
// Reference lines each one replaces are listed in include/gpe_hip.h.
#include "gpe_common.h"
#include <math.h>

// ---------------------------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------------------------
__global__ void gpe_reduce_inner_kernel(const float* __restrict__ x, long x_so, long x_si, int T, int R, int C,
                                        float* __restrict__ y, int ldy, int accumulate)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)R * C) return;
    const long r = e / C;
    const int c = (int)(e - r * C);
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += x[r * x_so + t * x_si + c];
    float* d = y + r * ldy + c;
    *d = accumulate ? (*d + s) : s;
}

extern "C" int gpe_reduce_inner(const float* x, long x_so, long x_si, int T, int R, int C, float* y, int ldy,
                                int accumulate, void* stream)
{
    if (!x || !y || T <= 0 || R <= 0 || C <= 0) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_reduce_inner_kernel, dim3(gpe_cdiv((long)R * C, 256)), dim3(256), 0, (hipStream_t)stream,
                       x, x_so, x_si, T, R, C, y, ldy, accumulate);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// out = alpha[0] * x with alpha on the device (the upstream gradient of a scalar loss term: no host read-back)
__global__ void gpe_scale_dev_kernel(const float* __restrict__ x, const float* __restrict__ alpha, float* __restrict__ out, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = alpha[0] * x[i];
}

extern "C" int gpe_scale_dev(const float* x, const float* alpha, float* out, long n, void* stream)
{
    if (!x || !alpha || !out || n < 0) return GPE_EINVAL;
    if (n == 0) return GPE_OK;
    hipLaunchKernelGGL(gpe_scale_dev_kernel, dim3((unsigned)gpe_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, alpha, out, n);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

__global__ void gpe_add_kernel(const float* a, const float* b, float* out, long n)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) out[e] = a[e] + b[e];
}

__global__ void gpe_scale_kernel(const float* x, float alpha, float* out, long n)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) out[e] = alpha * x[e];
}

extern "C" int gpe_scale(const float* x, float alpha, float* out, long n, void* stream)
{
    if (!x || !out || n < 0) return GPE_EINVAL;
    if (n == 0) return GPE_OK;
    hipLaunchKernelGGL(gpe_scale_kernel, dim3(gpe_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, alpha, out, n);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_add(const float* a, const float* b, float* out, long n, void* stream)
{
    if (!a || !b || !out || n < 0) return GPE_EINVAL;
    if (n == 0) return GPE_OK;
    hipLaunchKernelGGL(gpe_add_kernel, dim3(gpe_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, a, b, out, n);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// =====================================================================================================================
// input standardisation: out[r][c] = (x[r][c] - shift[c]) / scale[c]    (nn/data/transforms.py:35-50), C <= 8
// =====================================================================================================================
__global__ void gpe_standardize_kernel(const float* __restrict__ x, long n, int C, float s0, float s1, float s2, float s3,
                                       float s4, float s5, float s6, float s7, float d0, float d1, float d2, float d3,
                                       float d4, float d5, float d6, float d7, float* __restrict__ out)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const float sh[8] = {s0, s1, s2, s3, s4, s5, s6, s7}, sc[8] = {d0, d1, d2, d3, d4, d5, d6, d7};
    const int c = (int)(e % C);
    out[e] = (x[e] - sh[c]) / sc[c];
}

extern "C" int gpe_standardize(const float* x, long rows, int C, const float* shift_host, const float* scale_host,
                               float* out, void* stream)
{
    if (!x || !out || !shift_host || !scale_host || rows <= 0 || C <= 0 || C > 8) return GPE_EINVAL;
    float s[8] = {0}, d[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    for (int c = 0; c < C; ++c) { s[c] = shift_host[c]; d[c] = scale_host[c]; }
    const long n = rows * C;
    hipLaunchKernelGGL(gpe_standardize_kernel, dim3(gpe_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, n, C, s[0], s[1],
                       s[2], s[3], s[4], s[5], s[6], s[7], d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], out);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
