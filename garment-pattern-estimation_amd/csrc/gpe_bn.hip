// Bandwidth-bound kernels of the path for gfx950: BN finalisation (forward + backward coefficient algebra), the sums for an inner
// BN from the centred product of the reduce-GEMM, and BatchNorm applied to a stored post-ReLU activation.
// Reference lines each one replaces are listed in include/gpe_hip.h.
#include "gpe_common.h"
#include <math.h>

// ---------------------------------------------------------------------------------------------------------
// BatchNorm finalisation
// ---------------------------------------------------------------------------------------------------------
#define BNF_WAVES 16
#define BNF_CPW 16                    // channels per workgroup: a quarter wave per partial row, 4 rows per wave and load
#define BNF_SUB (64 / BNF_CPW)
__global__ __launch_bounds__(64 * BNF_WAVES) void gpe_bn_finalize_kernel(const double* __restrict__ part, int nblk, int C,
                                                              double count, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps,
                                                              float momentum, float* running_mean,
                                                              float* running_var, int64_t* num_batches,
                                                              float* __restrict__ stats)
{
    // one workgroup per 16 channels (round 6: 64 before — four workgroups read the 1.6 MB of partials of a 200-channel block, 13 do
    // now: 9.2 -> 6.5 us per launch; more load chains per wave did not help: scripts/bn_finalize_bench.py); a wave takes four partial
    // rows per load (lane = (row slot, channel)), its 16 waves x 4 slots split the blocks; combined in a fixed order: chains, then
    // row slots, then waves
    __shared__ double red[BNF_WAVES][2][BNF_CPW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ch = lane & (BNF_CPW - 1), sub = lane / BNF_CPW;
    const int c = blockIdx.x * BNF_CPW + ch;
    if (blockIdx.x == 0 && threadIdx.x == 0 && num_batches) *num_batches += 1;
    double s = 0, q = 0;
    if (c < C) {
        // four independent chains: the loads of a chain's next block do not wait for its add
        constexpr int RS = BNF_WAVES * BNF_SUB;              // row slots of the workgroup
        double s4[4] = {0, 0, 0, 0}, q4[4] = {0, 0, 0, 0};
        int b = wave * BNF_SUB + sub;
        for (; b + 3 * RS < nblk; b += 4 * RS) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                s4[u] += part[(size_t)(b + u * RS) * 2 * C + c];
                q4[u] += part[(size_t)(b + u * RS) * 2 * C + C + c];
            }
        }
        for (; b < nblk; b += RS) {
            s4[0] += part[(size_t)b * 2 * C + c];
            q4[0] += part[(size_t)b * 2 * C + C + c];
        }
        s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        q = (q4[0] + q4[1]) + (q4[2] + q4[3]);
    }
    // the row slots of a wave (lanes ch, ch + 16, ch + 32, ch + 48), in a fixed order
#pragma unroll
    for (int o = BNF_CPW; o < 64; o <<= 1) {
        s += __shfl_xor(s, o);
        q += __shfl_xor(q, o);
    }
    if (sub == 0) { red[wave][0][ch] = s; red[wave][1][ch] = q; }
    __syncthreads();
    if (wave != 0 || sub != 0 || c >= C) return;
    s = 0; q = 0;
    for (int w_ = 0; w_ < BNF_WAVES; ++w_) { s += red[w_][0][ch]; q += red[w_][1][ch]; }
    const double mean = s / count;
    double var = q / count - mean * mean;
    if (var < 0) var = 0;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    const float sc = (float)((double)gamma[c] * rstd);
    stats[c] = (float)mean;
    stats[C + c] = (float)rstd;
    stats[2 * C + c] = sc;
    stats[3 * C + c] = (float)((double)beta[c] - mean * (double)sc);
    if (running_mean) {
        const double unbiased = (count > 1) ? var * count / (count - 1) : var;
        running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * mean);
        running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * unbiased);
    }
}

extern "C" int gpe_bn_finalize(const double* part, int nblk, int C, double count, const float* gamma,
                               const float* beta, float eps, float momentum, float* running_mean,
                               float* running_var, int64_t* num_batches, float* stats_out, void* stream)
{
    if (!part || !gamma || !beta || !stats_out || nblk <= 0 || C <= 0 || count <= 0) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_bn_finalize_kernel, dim3(gpe_cdiv(C, BNF_CPW)), dim3(64 * BNF_WAVES), 0, (hipStream_t)stream, part, nblk,
                       C, count, gamma, beta, eps, momentum, running_mean, running_var, num_batches, stats_out);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

__global__ void gpe_bn_from_running_kernel(const float* rm, const float* rv, int C, const float* gamma,
                                           const float* beta, float eps, float* stats)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const double rstd = 1.0 / sqrt((double)rv[c] + (double)eps);
    const float sc = (float)((double)gamma[c] * rstd);
    stats[c] = rm[c];
    stats[C + c] = (float)rstd;
    stats[2 * C + c] = sc;
    stats[3 * C + c] = (float)((double)beta[c] - (double)rm[c] * (double)sc);
}

extern "C" int gpe_bn_from_running(const float* running_mean, const float* running_var, int C, const float* gamma,
                                   const float* beta, float eps, float* stats_out, void* stream)
{
    if (!running_mean || !running_var || !gamma || !beta || !stats_out || C <= 0) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_bn_from_running_kernel, dim3(gpe_cdiv(C, 64)), dim3(64), 0, (hipStream_t)stream,
                       running_mean, running_var, C, gamma, beta, eps, stats_out);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// (one thread per channel walking all partial blocks was a 128-deep dependent load chain: 38 us; now 16 waves split the
// blocks and meet in LDS, combined in a fixed order)
#define BNC_WAVES 16
__global__ __launch_bounds__(64 * BNC_WAVES) void gpe_bn_bwd_coef_kernel(const double* __restrict__ part, int nblk,
                                                                        const float* __restrict__ stats, int C, double count,
                                                                        float* __restrict__ coef, float* dgamma, float* dbeta)
{
    __shared__ double red[BNC_WAVES][2][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    double s1 = 0, s2 = 0;
    if (c < C) {
        for (int b = wave; b < nblk; b += BNC_WAVES) {
            s1 += part[(size_t)b * 2 * C + c];
            s2 += part[(size_t)b * 2 * C + C + c];
        }
    }
    red[wave][0][lane] = s1;
    red[wave][1][lane] = s2;
    __syncthreads();
    if (wave != 0 || c >= C) return;
    s1 = 0; s2 = 0;
    for (int w_ = 0; w_ < BNC_WAVES; ++w_) { s1 += red[w_][0][lane]; s2 += red[w_][1][lane]; }
    const double mean = stats[c], rstd = stats[C + c], s = stats[2 * C + c];
    const double m1 = s1 / count, m2 = s2 / count;
    const double k2 = s * rstd * m2;
    coef[c] = (float)s;
    coef[C + c] = (float)(s * m1);
    coef[2 * C + c] = (float)k2;
    coef[3 * C + c] = (float)mean;
    if (dgamma) dgamma[c] = (float)s2;
    if (dbeta) dbeta[c] = (float)s1;
}

extern "C" int gpe_bn_bwd_coef(const double* part, int nblk, const float* stats, int C, double count, float* coef,
                               float* dgamma, float* dbeta, void* stream)
{
    if (!part || !stats || !coef || nblk <= 0 || C <= 0 || count <= 0) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_bn_bwd_coef_kernel, dim3(gpe_cdiv(C, 64)), dim3(64 * BNC_WAVES), 0, (hipStream_t)stream, part, nblk,
                       stats, C, count, coef, dgamma, dbeta);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// sums for an inner BN + true weight gradient of the next Linear, from the CENTRED product
// Gc = dz_next^T (a - mean)  (accumulated without cancellation by the reduce-GEMM) and db = colsum(dz_next):
//   sum dy     = sum_f w[f][c] * db[f]
//   sum dy*xhat = rstd_c * sum_f w[f][c] * Gc[f][c]
//   dW_next[f][c] = Gc[f][c]*s_c + db[f]*beta_c          (since mean*s + t = beta)
#define BNG_FQ 16           // f-lanes per column: 64 columns x 16 f-lanes = one 1024-thread workgroup (Cn = 200: 13 rows each)
__global__ __launch_bounds__(64 * BNG_FQ) void gpe_bn_bwd_from_G_kernel(
    const float* __restrict__ G, int ldG, const float* __restrict__ db, const float* __restrict__ w, int ldw, int Cn,
    int C, const float* __restrict__ stats, double* __restrict__ sums, float* __restrict__ dw, int lddw)
{
    // (one thread per column looping over all Cn rows was a 200-deep dependent load chain: 77 us for 120 KB of data)
    __shared__ double red[BNG_FQ][2][64];
    const int lane = threadIdx.x & 63, fq = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    double a = 0, b = 0;
    if (c < C) {
        const double s = stats[2 * C + c], t = stats[3 * C + c], mean = stats[c];
        const double beta = t + mean * s;
        double a2[2] = {0, 0}, b2[2] = {0, 0};
        int f = fq;
        for (; f + BNG_FQ < Cn; f += 2 * BNG_FQ) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int ff = f + BNG_FQ * u;
                const double wf = w[(size_t)ff * ldw + c], gf = G[(size_t)ff * ldG + c], dbf = db[ff];
                a2[u] += wf * dbf;
                b2[u] += wf * gf;
                if (dw) dw[(size_t)ff * lddw + c] = (float)(gf * s + dbf * beta);
            }
        }
        if (f < Cn) {
            const double wf = w[(size_t)f * ldw + c], gf = G[(size_t)f * ldG + c], dbf = db[f];
            a2[0] += wf * dbf;
            b2[0] += wf * gf;
            if (dw) dw[(size_t)f * lddw + c] = (float)(gf * s + dbf * beta);
        }
        a = a2[0] + a2[1];
        b = b2[0] + b2[1];
    }
    red[fq][0][lane] = a;
    red[fq][1][lane] = b;
    __syncthreads();
    if (fq != 0 || c >= C) return;
    a = 0; b = 0;
    for (int q = 0; q < BNG_FQ; ++q) { a += red[q][0][lane]; b += red[q][1][lane]; }
    sums[c] = a;
    sums[C + c] = b * (double)stats[C + c];
}

extern "C" int gpe_bn_bwd_from_G(const float* G, int ldG, const float* db, const float* w_next, int ldw, int Cn,
                                 int C, const float* stats, double* sums, float* dw, int lddw, void* stream)
{
    if (!G || !db || !w_next || !stats || !sums || Cn <= 0 || C <= 0 || ldG < C || ldw < C) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_bn_bwd_from_G_kernel, dim3(gpe_cdiv(C, 64)), dim3(64 * BNG_FQ), 0, (hipStream_t)stream, G, ldG, db,
                       w_next, ldw, Cn, C, stats, sums, dw, lddw);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// y[r][c] = s[c]*a[r][c] + t[c]   (BatchNorm applied to a stored post-ReLU activation; dense-MLP last layer)
__global__ void gpe_bn_apply_kernel(const float* __restrict__ a, int lda, const float* __restrict__ stats, long rows,
                                    int C, float a_scale, float t_scale, float* __restrict__ y, int ldy)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * C) return;
    const long r = e / C;
    const int c = (int)(e - r * C);
    y[r * ldy + c] = stats[2 * C + c] * (a[r * lda + c] * a_scale) + stats[3 * C + c] * t_scale;
}

extern "C" int gpe_bn_apply_scaled(const float* a, int lda, const float* stats, long rows, int C, float a_scale,
                                   float t_scale, float* y, int ldy, void* stream)
{
    if (!a || !stats || !y || rows < 0 || C <= 0 || lda < C || ldy < C) return GPE_EINVAL;
    if (rows == 0) return GPE_OK;
    hipLaunchKernelGGL(gpe_bn_apply_kernel, dim3(gpe_cdiv(rows * C, 256)), dim3(256), 0, (hipStream_t)stream, a, lda,
                       stats, rows, C, a_scale, t_scale, y, ldy);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_bn_apply(const float* a, int lda, const float* stats, long rows, int C, float* y, int ldy,
                            void* stream)
{
    return gpe_bn_apply_scaled(a, lda, stats, rows, C, 1.f, 1.f, y, ldy, stream);
}
