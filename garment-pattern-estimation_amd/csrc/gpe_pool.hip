// Pooling over the points of a cloud, as gfx950 kernels:
//   * segment mean pool (equal-sized segments: every cloud has N points)
//   * global max / add pooling (torch_geometric global_max_pool / global_add_pool, nn/net_blocks.py:145-150)
//   * attention pooling over the per-point panel scores (nn/nets.py:263-276) for mean / add / max pooling
//   * sparsemax over the scores (sparsemax.Sparsemax(dim=1), nn/nets.py:225), forward and backward
// All of it is bandwidth- or latency-bound small work: no MFMA here.  Reductions run in fp64 with a fixed order, so
// results are run-to-run deterministic; there are no float atomics.
// Reference lines of the segment mean and of sparsemax are listed in include/gpe_hip.h.
#include "gpe_device.h"
#include <math.h>

// ---------------------------------------------------------------------------------------------------------
// segment mean pool (equal-sized segments: every cloud has N points)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void gpe_segment_mean_fwd_kernel(const float* __restrict__ x, int ldx, int N,
                                                                    int C, float* __restrict__ y, int ldy)
{
    __shared__ double red[4][256];
    const int c = threadIdx.x & 255, rg = threadIdx.x >> 8;
    const int b = blockIdx.x;
    for (int c0 = 0; c0 < C; c0 += 256) {
        double s = 0;
        if (c0 + c < C) {
            // 8 rows in flight per thread (one load per dependent fp64 add was a 512-deep latency chain: 150 us)
            const float* px = x + ((size_t)b * N) * ldx + c0 + c;
            double sa[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int n = rg;
            for (; n + 28 < N; n += 32) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = px[(size_t)(n + 4 * u) * ldx];
#pragma unroll
                for (int u = 0; u < 8; ++u) sa[u] += (double)v[u];
            }
            for (; n < N; n += 4) sa[0] += (double)px[(size_t)n * ldx];
            s = ((sa[0] + sa[1]) + (sa[2] + sa[3])) + ((sa[4] + sa[5]) + (sa[6] + sa[7]));
        }
        red[rg][c] = s;
        __syncthreads();
        if (rg == 0 && c0 + c < C)
            y[(size_t)b * ldy + c0 + c] = (float)((red[0][c] + red[1][c] + red[2][c] + red[3][c]) / (double)N);
        __syncthreads();
    }
}

extern "C" int gpe_segment_mean_fwd(const float* x, int ldx, int B, int N, int C, float* y, int ldy, void* stream)
{
    if (!x || !y || B <= 0 || N <= 0 || C <= 0 || ldx < C || ldy < C) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_segment_mean_fwd_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, x, ldx, N, C, y,
                       ldy);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

__global__ void gpe_segment_mean_bwd_kernel(const float* __restrict__ gy, int ldgy, int N, int C, long rows,
                                            float* __restrict__ gx, int ldgx, int accumulate)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * C) return;
    const long r = e / C;
    const int c = (int)(e - r * C);
    const float v = gy[(r / N) * ldgy + c] / (float)N;
    float* d = gx + r * ldgx + c;
    *d = accumulate ? (*d + v) : v;
}

extern "C" int gpe_segment_mean_bwd(const float* gy, int ldgy, int B, int N, int C, float* gx, int ldgx,
                                    int accumulate, void* stream)
{
    if (!gy || !gx || B <= 0 || N <= 0 || C <= 0) return GPE_EINVAL;
    const long rows = (long)B * N;
    hipLaunchKernelGGL(gpe_segment_mean_bwd_kernel, dim3(gpe_cdiv(rows * C, 256)), dim3(256), 0,
                       (hipStream_t)stream, gy, ldgy, N, C, rows, gx, ldgx, accumulate);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// =====================================================================================================================
// global max / add pooling over equal-sized clouds (mean: above)
// =====================================================================================================================
__global__ __launch_bounds__(1024) void gpe_segment_pool_fwd_kernel(const float* __restrict__ x, int ldx, int N, int C,
                                                                    int mode, float* __restrict__ y, int ldy,
                                                                    int32_t* __restrict__ arg)
{
    __shared__ float rv[16][64];
    __shared__ int ri[16][64];
    __shared__ double rs[16][64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    float best = -INFINITY;
    int ba = 0;
    double s = 0;
    if (c < C) {
        for (int n = wave; n < N; n += 16) {
            const float v = x[((long)b * N + n) * ldx + c];
            if (mode == 1) { if (v > best) { best = v; ba = n; } }
            else s += (double)v;
        }
    }
    rv[wave][lane] = best; ri[wave][lane] = ba; rs[wave][lane] = s;
    __syncthreads();
    if (wave != 0 || c >= C) return;
    if (mode == 1) {
        for (int w_ = 1; w_ < 16; ++w_) {
            const float v = rv[w_][lane];
            const int a = ri[w_][lane];
            if (v > best || (v == best && a < ba)) { best = v; ba = a; }      // first maximum
        }
        y[(long)b * ldy + c] = best;
        arg[(long)b * C + c] = ba;
    } else {
        double t = 0;
        for (int w_ = 0; w_ < 16; ++w_) t += rs[w_][lane];
        y[(long)b * ldy + c] = (float)t;
    }
}

__global__ void gpe_segment_pool_bwd_kernel(const float* __restrict__ gy, int ldgy, const int32_t* __restrict__ arg, int N,
                                            int C, int mode, long rows, float* __restrict__ gx, int ldgx)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * C) return;
    const long r = e / C;
    const int c = (int)(e - r * C);
    const long b = r / N;
    const int n = (int)(r - b * N);
    const float g = gy[b * ldgy + c];
    gx[r * ldgx + c] = (mode == 1) ? ((arg[b * C + c] == n) ? g : 0.f) : g;
}

extern "C" int gpe_segment_pool_fwd(const float* x, int ldx, int B, int N, int C, int mode, float* y, int ldy,
                                    int32_t* arg, void* stream)
{
    if (!x || !y || B <= 0 || N <= 0 || C <= 0 || ldx < C || ldy < C || (mode != 1 && mode != 2) || (mode == 1 && !arg))
        return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_segment_pool_fwd_kernel, dim3(B, gpe_cdiv(C, 64)), dim3(1024), 0, (hipStream_t)stream, x, ldx, N,
                       C, mode, y, ldy, arg);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_segment_pool_bwd(const float* gy, int ldgy, const int32_t* arg, int B, int N, int C, int mode,
                                    float* gx, int ldgx, void* stream)
{
    if (!gy || !gx || B <= 0 || N <= 0 || C <= 0 || (mode != 1 && mode != 2) || (mode == 1 && !arg)) return GPE_EINVAL;
    const long rows = (long)B * N;
    hipLaunchKernelGGL(gpe_segment_pool_bwd_kernel, dim3(gpe_cdiv(rows * C, 256)), dim3(256), 0, (hipStream_t)stream, gy, ldgy,
                       arg, N, C, mode, rows, gx, ldgx);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// =====================================================================================================================
// attention pooling: pooled[b][p][c] = pool_n ( w[b*N+n][p] * feat[b*N+n][c] )      (nn/nets.py:263-276)
//   mode 0 mean (1/N sum), 1 max, 2 add.  Workgroup = (cloud, 256-point slab); thread = a set of (p, c) outputs held in
//   registers; the slab's w / feat rows are staged in LDS.  Partials [B][nslab][P][C] are combined in slab order by the
//   second kernel (deterministic).  max keeps the argmax point for the backward pass.
// =====================================================================================================================
#define AP_ROWS 64
#define AP_TPT 2         // 4 x 4 output tiles per thread: ceil(P/4) * ceil(C/4) <= 256 * AP_TPT
__global__ __launch_bounds__(256) void gpe_attn_pool_part_kernel(const float* __restrict__ w, int ldw,
                                                                 const float* __restrict__ feat, int ldf, int N, int P,
                                                                 int C, int mode, int nslab, float* __restrict__ part,
                                                                 int32_t* __restrict__ part_arg)
{
    // register tiling: a thread owns 4 heads x 4 channels, so a slab row costs two ds_read_b128 per 16 products (one
    // (p, c) output per register with two ds_read_b32 per product was LDS-issue bound: 0.72 ms at cfg 4)
    extern __shared__ __align__(16) float sm[];
    const int Pp = (P + 3) & ~3, Cp = (C + 3) & ~3;
    float* ws = sm;                       // [AP_ROWS][Pp]  (pad columns zero)
    float* fs = sm + AP_ROWS * Pp;        // [AP_ROWS][Cp]
    const int b = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = slab * AP_ROWS;
    const int nr = (N - n0 < AP_ROWS) ? (N - n0) : AP_ROWS;
    for (int r = wave; r < nr; r += 4) {
        const long row = (long)b * N + n0 + r;
        for (int c = lane; c < Pp; c += 64) ws[r * Pp + c] = (c < P) ? w[row * ldw + c] : 0.f;
        for (int c = lane; c < Cp; c += 64) fs[r * Cp + c] = (c < C) ? feat[row * ldf + c] : 0.f;
    }
    __syncthreads();
    const int pq = Pp >> 2, cqn = Cp >> 2, tiles = pq * cqn;
    float acc[AP_TPT][4][4];
    int arg[AP_TPT][4][4];
    int tp[AP_TPT], tc[AP_TPT];
#pragma unroll
    for (int q = 0; q < AP_TPT; ++q) {
        const int t = tid + 256 * q;
        const int tt = (t < tiles) ? t : 0;
        tp[q] = tt / cqn; tc[q] = tt - tp[q] * cqn;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) { acc[q][i][k] = (mode == 1) ? -INFINITY : 0.f; arg[q][i][k] = 0; }
    }
    const int ntq = (tiles + 255) >> 8;       // tile slots in use (uniform)
    for (int r = 0; r < nr; ++r) {
#pragma unroll
        for (int q = 0; q < AP_TPT; ++q) {
            if (q < ntq) {
                const float4 wv = *reinterpret_cast<const float4*>(&ws[r * Pp + 4 * tp[q]]);
                const float4 fv = *reinterpret_cast<const float4*>(&fs[r * Cp + 4 * tc[q]]);
                const float wa[4] = {wv.x, wv.y, wv.z, wv.w}, fa[4] = {fv.x, fv.y, fv.z, fv.w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float v = wa[i] * fa[k];
                        if (mode == 1) { if (v > acc[q][i][k]) { acc[q][i][k] = v; arg[q][i][k] = n0 + r; } }
                        else acc[q][i][k] += v;
                    }
            }
        }
    }
    const int total = P * C;
#pragma unroll
    for (int q = 0; q < AP_TPT; ++q) {
        if (tid + 256 * q < tiles) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int p_ = 4 * tp[q] + i, c = 4 * tc[q] + k;
                    if (p_ < P && c < C) {
                        const size_t dst = ((size_t)b * nslab + slab) * total + (size_t)p_ * C + c;
                        part[dst] = acc[q][i][k];
                        if (mode == 1) part_arg[dst] = arg[q][i][k];
                    }
                }
        }
    }
}

__global__ void gpe_attn_pool_final_kernel(const float* __restrict__ part, const int32_t* __restrict__ part_arg, int N,
                                           int total, int mode, int nslab, float* __restrict__ out,
                                           int32_t* __restrict__ arg)
{
    const int b = blockIdx.y;
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total) return;
    if (mode == 1) {
        float best = -INFINITY;
        int ba = 0;
        for (int s = 0; s < nslab; ++s) {
            const size_t src = ((size_t)b * nslab + s) * total + o;
            const float v = part[src];
            if (v > best) { best = v; ba = part_arg[src]; }       // earlier slab wins ties: first maximum
        }
        out[(size_t)b * total + o] = best;
        arg[(size_t)b * total + o] = ba;
    } else {
        double s_ = 0;
        for (int s = 0; s < nslab; ++s) s_ += (double)part[((size_t)b * nslab + s) * total + o];
        out[(size_t)b * total + o] = (float)(mode == 0 ? s_ / N : s_);
    }
}

extern "C" long gpe_attn_pool_ws(int B, int N, int P, int C) { return (long)B * gpe_cdiv(N, AP_ROWS) * P * C; }

extern "C" int gpe_attn_pool_fwd(const float* w, int ldw, const float* feat, int ldf, int B, int N, int P, int C,
                                 int mode, float* out, int32_t* arg, float* part, int32_t* part_arg, void* stream)
{
    if (!w || !feat || !out || !part || B <= 0 || N <= 0 || P <= 0 || C <= 0 || ldw < P || ldf < C || mode < 0 ||
        mode > 2 || (long)gpe_cdiv(P, 4) * gpe_cdiv(C, 4) > 256L * AP_TPT)
        return GPE_EINVAL;
    if (mode == 1 && (!arg || !part_arg)) return GPE_EINVAL;
    const int nslab = gpe_cdiv(N, AP_ROWS);
    const size_t lds = (size_t)AP_ROWS * (gpe_round_up(P, 4) + gpe_round_up(C, 4)) * sizeof(float);
    if (lds > 150 * 1024) return GPE_EINVAL;
    GPE_ENSURE_MAX_LDS_N((gpe_attn_pool_part_kernel), 150 * 1024);
    hipLaunchKernelGGL(gpe_attn_pool_part_kernel, dim3(nslab, B), dim3(256), lds, (hipStream_t)stream, w, ldw, feat, ldf, N,
                       P, C, mode, nslab, part, part_arg);
    hipLaunchKernelGGL(gpe_attn_pool_final_kernel, dim3(gpe_cdiv(P * C, 256), B), dim3(256), 0, (hipStream_t)stream, part,
                       part_arg, N, P * C, mode, nslab, out, arg);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// backward, mean / add: gw[n][p] = sc * sum_c feat[n][c] g[b][p][c] ; gf[n][c] = sc * sum_p w[n][p] g[b][p][c]
// (sc = 1/N or 1).  Workgroup = 64 points of a cloud; the cloud's (scaled) g matrix [P][C] and the 64 w / feat rows sit in
// LDS, outputs are register tiles (gf: 4 points x 4 channels, p ascending; gw: 2 points x 4 heads, c ascending — the same
// summation order as a plain per-output loop, so the result does not depend on the tiling).
#define APB_ROWS 64
__global__ __launch_bounds__(256) void gpe_attn_pool_bwd_kernel(const float* __restrict__ w, int ldw,
                                                                const float* __restrict__ feat, int ldf,
                                                                const float* __restrict__ g, int N, int P, int C,
                                                                float sc, float* __restrict__ gw, int ldgw,
                                                                float* __restrict__ gf, int ldgf)
{
    extern __shared__ __align__(16) float sm[];
    const int Pp = (P + 3) & ~3, Cp = (C + 3) & ~3;
    float* gs = sm;                          // [Pp][Cp]   (pad rows / columns zero)
    float* ws = gs + Pp * Cp;                // [APB_ROWS][Pp]
    float* fs = ws + APB_ROWS * Pp;          // [APB_ROWS][Cp]
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * APB_ROWS;
    const int nr = (N - n0 < APB_ROWS) ? (N - n0) : APB_ROWS;
    for (int p_ = wave; p_ < Pp; p_ += 4)
        for (int c = lane; c < Cp; c += 64) gs[p_ * Cp + c] = (p_ < P && c < C) ? g[((size_t)b * P + p_) * C + c] * sc : 0.f;
    for (int r = wave; r < APB_ROWS; r += 4) {
        const long row = (long)b * N + n0 + (r < nr ? r : nr - 1);
        for (int c = lane; c < Pp; c += 64) ws[r * Pp + c] = (c < P && r < nr) ? w[row * ldw + c] : 0.f;
        for (int c = lane; c < Cp; c += 64) fs[r * Cp + c] = (c < C && r < nr) ? feat[row * ldf + c] : 0.f;
    }
    __syncthreads();
    // gf: tiles of 4 points x 4 channels
    const int cqn = Cp >> 2;
    for (int t = tid; t < (APB_ROWS / 4) * cqn; t += 256) {
        const int ng = t / cqn, cq = t - ng * cqn;
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[i][k] = 0.f;
        for (int p_ = 0; p_ < P; ++p_) {
            const float4 gv = *reinterpret_cast<const float4*>(&gs[p_ * Cp + 4 * cq]);
            const float ga[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float wv = ws[(4 * ng + i) * Pp + p_];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[i][k] = __builtin_fmaf(wv, ga[k], acc[i][k]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * ng + i;
            if (r < nr) {
                float* dst = gf + ((long)b * N + n0 + r) * ldgf + 4 * cq;
#pragma unroll
                for (int k = 0; k < 4; ++k) if (4 * cq + k < C) dst[k] = acc[i][k];
            }
        }
    }
    // gw: tiles of 2 points x 4 heads, channels four at a time in ascending order
    const int pq = Pp >> 2;
    for (int t = tid; t < (APB_ROWS / 2) * pq; t += 256) {
        const int ng = t / pq, pg = t - ng * pq;
        float acc[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[i][k] = 0.f;
        for (int c4 = 0; c4 < Cp; c4 += 4) {
            float4 fv[2], gv[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) fv[i] = *reinterpret_cast<const float4*>(&fs[(2 * ng + i) * Cp + c4]);
#pragma unroll
            for (int k = 0; k < 4; ++k) gv[k] = *reinterpret_cast<const float4*>(&gs[(4 * pg + k) * Cp + c4]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float s_ = acc[i][k];
                    s_ = __builtin_fmaf(fv[i].x, gv[k].x, s_);
                    s_ = __builtin_fmaf(fv[i].y, gv[k].y, s_);
                    s_ = __builtin_fmaf(fv[i].z, gv[k].z, s_);
                    s_ = __builtin_fmaf(fv[i].w, gv[k].w, s_);
                    acc[i][k] = s_;
                }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = 2 * ng + i;
            if (r < nr) {
                float* dst = gw + ((long)b * N + n0 + r) * ldgw + 4 * pg;
#pragma unroll
                for (int k = 0; k < 4; ++k) if (4 * pg + k < P) dst[k] = acc[i][k];
            }
        }
    }
}

// backward, max: only the argmax point of each (b, p, c) receives gradient.  gw / gf must be ZERO on entry.
//   pass 0: thread (b, p) walks c sequentially:  gw[arg][p] += g * feat[arg][c]   (distinct p per thread: no collisions)
//   pass 1: thread (b, c) walks p sequentially:  gf[arg][c] += g * w[arg][p]      (distinct c per thread)
__global__ void gpe_attn_pool_bwd_max_kernel(const float* __restrict__ w, int ldw, const float* __restrict__ feat,
                                             int ldf, const float* __restrict__ g, const int32_t* __restrict__ arg,
                                             int N, int P, int C, float* __restrict__ gw, int ldgw,
                                             float* __restrict__ gf, int ldgf)
{
    const int b = blockIdx.y;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const float* gb = g + (size_t)b * P * C;
    const int32_t* ab = arg + (size_t)b * P * C;
    if (t < P) {
        for (int c = 0; c < C; ++c) {
            const long row = (long)b * N + ab[t * C + c];
            gw[row * ldgw + t] += gb[t * C + c] * feat[row * ldf + c];
        }
    } else if (t < P + C) {
        const int c = t - P;
        for (int p_ = 0; p_ < P; ++p_) {
            const long row = (long)b * N + ab[p_ * C + c];
            gf[row * ldgf + c] += gb[p_ * C + c] * w[row * ldw + p_];
        }
    }
}

extern "C" int gpe_attn_pool_bwd(const float* w, int ldw, const float* feat, int ldf, const float* g,
                                 const int32_t* arg, int B, int N, int P, int C, int mode, float* gw, int ldgw,
                                 float* gf, int ldgf, void* stream)
{
    if (!w || !feat || !g || !gw || !gf || B <= 0 || N <= 0 || P <= 0 || C <= 0 || mode < 0 || mode > 2 || ldgw < P ||
        ldgf < C)
        return GPE_EINVAL;
    if (mode == 1) {
        if (!arg) return GPE_EINVAL;
        if (hipMemsetAsync(gw, 0, (size_t)B * N * ldgw * sizeof(float), (hipStream_t)stream) != hipSuccess ||
            hipMemsetAsync(gf, 0, (size_t)B * N * ldgf * sizeof(float), (hipStream_t)stream) != hipSuccess)
            return GPE_ELAUNCH;
        hipLaunchKernelGGL(gpe_attn_pool_bwd_max_kernel, dim3(gpe_cdiv(P + C, 64), B), dim3(64), 0, (hipStream_t)stream, w,
                           ldw, feat, ldf, g, arg, N, P, C, gw, ldgw, gf, ldgf);
    } else {
        const int Pp = gpe_round_up(P, 4), Cp = gpe_round_up(C, 4);
        const size_t lds = ((size_t)Pp * Cp + (size_t)APB_ROWS * (Pp + Cp)) * sizeof(float);
        if (lds > 150 * 1024) return GPE_EINVAL;
        GPE_ENSURE_MAX_LDS_N((gpe_attn_pool_bwd_kernel), 150 * 1024);
        hipLaunchKernelGGL(gpe_attn_pool_bwd_kernel, dim3(gpe_cdiv(N, APB_ROWS), B), dim3(256), lds, (hipStream_t)stream, w, ldw,
                           feat, ldf, g, N, P, C, mode == 0 ? 1.f / N : 1.f, gw, ldgw, gf, ldgf);
    }
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// ---------------------------------------------------------------------------------------------------------
// sparsemax over rows of width W <= 32 (sparsemax.Sparsemax(dim=1), /root/reference/nn/nets.py:225; Martins &
// Astudillo 2016): out = max((z - max) - tau, 0), tau from the sorted-cumsum support rule on the max-shifted row (as the
// published implementation does); backward nz*(g - mean_nz(g)).
// One row per lane, the row sorted in registers by a fully unrolled odd-even transposition network.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpe_sparsemax_fwd_kernel(const float* __restrict__ z, int ldz, long rows, int W,
                                                                float* __restrict__ out, int ldo)
{
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    float v[SPX_W];
#pragma unroll
    for (int i = 0; i < SPX_W; ++i) v[i] = (i < W) ? z[r * ldz + i] : -INFINITY;
#pragma unroll
    for (int pass = 0; pass < SPX_W; ++pass) {
#pragma unroll
        for (int i = (pass & 1); i + 1 < SPX_W; i += 2) {
            const float a = v[i], b = v[i + 1];
            v[i] = fmaxf(a, b); v[i + 1] = fminf(a, b);          // descending
        }
    }
    // sparsemax(z) = sparsemax(z - c): the rule runs on z - max, where the cumulative sum and tau keep their fp32 precision
    // whatever the magnitude of the scores (on raw scores near 1e3 the 1e-4 of a support decision is below one ulp of cs)
    const float mx = v[0];
    float cs = 0.f, tau = 0.f;
#pragma unroll
    for (int i = 0; i < SPX_W; ++i) {
        if (i < W) {
            const float vi = v[i] - mx;
            cs += vi;
            if (1.f + (float)(i + 1) * vi > cs) tau = (cs - 1.f) / (float)(i + 1);   // support grows monotonically
        }
    }
    for (int i = 0; i < W; ++i) out[r * ldo + i] = fmaxf((z[r * ldz + i] - mx) - tau, 0.f);
}

__global__ __launch_bounds__(256) void gpe_sparsemax_bwd_kernel(const float* __restrict__ out, int ldo,
                                                                const float* __restrict__ g, int ldg, long rows, int W,
                                                                float* __restrict__ gz, int ldgz)
{
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    float s = 0.f, n = 0.f;
    for (int i = 0; i < W; ++i)
        if (out[r * ldo + i] > 0.f) { s += g[r * ldg + i]; n += 1.f; }
    const float m = (n > 0.f) ? s / n : 0.f;
    for (int i = 0; i < W; ++i) gz[r * ldgz + i] = (out[r * ldo + i] > 0.f) ? g[r * ldg + i] - m : 0.f;
}

extern "C" int gpe_sparsemax_fwd(const float* z, int ldz, long rows, int W, float* out, int ldo, void* stream)
{
    if (!z || !out || rows < 0 || W <= 0 || W > SPX_W || ldz < W || ldo < W) return GPE_EINVAL;
    if (rows == 0) return GPE_OK;
    hipLaunchKernelGGL(gpe_sparsemax_fwd_kernel, dim3(gpe_cdiv(rows, 256)), dim3(256), 0, (hipStream_t)stream, z, ldz,
                       rows, W, out, ldo);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_sparsemax_bwd(const float* out, int ldo, const float* g, int ldg, long rows, int W, float* gz,
                                 int ldgz, void* stream)
{
    if (!out || !g || !gz || rows < 0 || W <= 0 || ldo < W || ldg < W || ldgz < W) return GPE_EINVAL;
    if (rows == 0) return GPE_OK;
    hipLaunchKernelGGL(gpe_sparsemax_bwd_kernel, dim3(gpe_cdiv(rows, 256)), dim3(256), 0, (hipStream_t)stream, out,
                       ldo, g, ldg, rows, W, gz, ldgz);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
