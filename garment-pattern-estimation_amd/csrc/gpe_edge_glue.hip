// Bandwidth-bound kernels of the path for gfx950, the EdgeConv glue: the EdgeConv neighbourhood gather with fp64 BN statistics,
// max-aggregation finish, sum over the k messages of a point (EdgeConv aggr = 'add' / 'mean', nn/net_blocks.py:129), the per-point
// sums and dz3 of the backward pass, kNN graph transposition + deterministic pull-style scatter, the W1 split of the first edge-MLP
// Linear, and the explicit EdgeConv message inputs (nn/net_blocks.py:124-135).
// Reference lines each one replaces are listed in include/gpe_hip.h.
#include "gpe_common.h"
#include <math.h>

__device__ __forceinline__ float4 pw_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void pw_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// ---------------------------------------------------------------------------------------------------------
// EdgeConv neighbourhood gather + fp64 statistics of a1 = relu(P_i + Q_j)
//   one wave per point at a time: lanes span the H channels as float4, the k neighbour rows are fetched with
//   wave-uniform (shuffle-broadcast) row bases and all k loads in flight before the first use.
// ---------------------------------------------------------------------------------------------------------
#define GS_BLOCKS 512
#ifndef GS_KU
#define GS_KU 8               // neighbour rows in flight per wave
#endif
#ifndef GS_WAVES
#define GS_WAVES 8            // waves per workgroup (GS_BLOCKS workgroups: 4 waves per SIMD; round 6: 4 before — the pass is a chain of
                              // L2 round trips per wave, more waves in flight: 85 -> 61 us per launch at cfg 2; 16: 63)
#endif
template <int KU>
__global__ __launch_bounds__(64 * GS_WAVES) void gpe_gather_stats_kernel(const float* __restrict__ pq, int ldpq, int H,
                                                               const int32_t* __restrict__ jg, int k,
                                                               int B, int N, int pin, double* __restrict__ part)
{
    __shared__ double red[GS_WAVES][2][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = 4 * lane;
    const bool active = c < H;
    double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
    // pin: the waves of XCD x (blocks x, x+8, ...) walk the points of clouds x, x+8, ... only, one cloud at a time, so a
    // cloud's Q table (N x H floats, gathered k-fold) is served by that XCD's L2 alone (gpe_common.h)
    GpePointWalk wk = gpe_point_walk(B, N, pin);
    if (GS_WAVES != 4) {                                   // (gpe_point_walk counts four waves per workgroup)
        wk.first = (long)(pin ? (blockIdx.x >> 3) : blockIdx.x) * GS_WAVES + wave;
        wk.stride = (long)(pin ? (gridDim.x >> 3) : gridDim.x) * GS_WAVES;
    }
    for (long u = wk.first; u < wk.count; u += wk.stride) {
        const long i = gpe_walk_point(wk, u, N);
        const int myidx = (lane < k) ? jg[i * k + lane] : 0;
        float4 p4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (active) p4 = pw_ld4(pq + i * ldpq + c);
        // a point's k messages are summed in fp32 (k <= 64 terms: 1e-7 relative, the same partial sums the fused edge kernels keep per
        // tile), the points in fp64: the fp64 conversions and adds per ELEMENT (round 1 - 4) were this pass's whole run time
        float s32[4] = {0.f, 0.f, 0.f, 0.f}, q32[4] = {0.f, 0.f, 0.f, 0.f};
        for (int s0 = 0; s0 < k; s0 += KU) {
            float4 nb[KU];
#pragma unroll
            for (int u = 0; u < KU; ++u) {
                nb[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (s0 + u < k) {
                    const long jrow = __shfl(myidx, s0 + u);
                    if (active) nb[u] = pw_ld4(pq + jrow * ldpq + H + c);
                }
            }
#pragma unroll
            for (int u = 0; u < KU; ++u) {
                if (s0 + u < k) {
                    const float a0 = fmaxf(p4.x + nb[u].x, 0.f), a1 = fmaxf(p4.y + nb[u].y, 0.f);
                    const float a2 = fmaxf(p4.z + nb[u].z, 0.f), a3 = fmaxf(p4.w + nb[u].w, 0.f);
                    s32[0] += a0; q32[0] = __builtin_fmaf(a0, a0, q32[0]);
                    s32[1] += a1; q32[1] = __builtin_fmaf(a1, a1, q32[1]);
                    s32[2] += a2; q32[2] = __builtin_fmaf(a2, a2, q32[2]);
                    s32[3] += a3; q32[3] = __builtin_fmaf(a3, a3, q32[3]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) { s[t] += (double)s32[t]; q[t] += (double)q32[t]; }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) { red[wave][0][c + t] = s[t]; red[wave][1][c + t] = q[t]; }
    __syncthreads();
    if (tid < H) {
        double a = 0, b = 0;
        for (int w = 0; w < GS_WAVES; ++w) { a += red[w][0][tid]; b += red[w][1][tid]; }
        part[(size_t)blockIdx.x * 2 * H + tid] = a;
        part[(size_t)blockIdx.x * 2 * H + H + tid] = b;
    }
}

extern "C" int gpe_edge_gather_stats(const float* pq, int ldpq, int H, const int32_t* jg, int B, int N, int k,
                                     double* part, void* stream)
{
    if (!pq || !jg || !part || B <= 0 || N <= 0 || k <= 0 || k > 64 || H <= 0 || H > 256 || (H & 3) || (ldpq & 3) ||
        ldpq < 2 * H)
        return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_gather_stats_kernel<GS_KU>, dim3(GS_BLOCKS), dim3(64 * GS_WAVES), 0, (hipStream_t)stream, pq, ldpq, H,
                       jg, k, B, N, gpe_pin_clouds(B) ? 1 : 0, part);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// ---------------------------------------------------------------------------------------------------------
// max aggregation finish: y = s*(s>=0 ? max : min) + t
// ---------------------------------------------------------------------------------------------------------
__global__ void gpe_edge_finish_kernel(const float* __restrict__ mx, const float* __restrict__ mn, int ldagg,
                                       const float* __restrict__ stats, long rows, int C, float* __restrict__ y,
                                       int ldy)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * C) return;
    const long r = e / C;
    const int c = (int)(e - r * C);
    const float s = stats[2 * C + c], t = stats[3 * C + c];
    const float v = (s >= 0.f) ? mx[r * ldagg + c] : mn[r * ldagg + c];
    y[r * ldy + c] = s * v + t;
}

extern "C" int gpe_edge_finish(const float* mx, const float* mn, int ldagg, const float* stats, long rows, int C,
                               float* y, int ldy, void* stream)
{
    if (!mx || !mn || !stats || !y || rows < 0 || C <= 0 || ldagg < C || ldy < C) return GPE_EINVAL;
    if (rows == 0) return GPE_OK;
    hipLaunchKernelGGL(gpe_edge_finish_kernel, dim3(gpe_cdiv(rows * C, 256)), dim3(256), 0, (hipStream_t)stream, mx,
                       mn, ldagg, stats, rows, C, y, ldy);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// sum over the k messages of every point: out[i][c] = sum_s a[(i*k+s)][c]   (EdgeConv aggr 'add' / 'mean')
__global__ __launch_bounds__(256) void gpe_edge_sum_k_kernel(const float* __restrict__ a, int lda, long npts, int k, int F,
                                                             float* __restrict__ out, int ldo)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.y * 64 + lane;
    if (c0 >= F) return;
    const long nw = (long)gridDim.x * 4;
    for (long i = (long)blockIdx.x * 4 + wave; i < npts; i += nw) {
        float s = 0.f;
        for (int s_ = 0; s_ < k; ++s_) s += a[(i * k + s_) * lda + c0];
        out[i * ldo + c0] = s;
    }
}

extern "C" int gpe_edge_sum_k(const float* a, int lda, long npts, int k, int F, float* out, int ldo, void* stream)
{
    if (!a || !out || npts <= 0 || k <= 0 || F <= 0 || lda < F || ldo < F) return GPE_EINVAL;
    const int bx = (int)((npts + 3) / 4 < 2048 ? (npts + 3) / 4 : 2048);
    hipLaunchKernelGGL(gpe_edge_sum_k_kernel, dim3(bx, gpe_cdiv(F, 64)), dim3(256), 0, (hipStream_t)stream, a, lda, npts, k,
                       F, out, ldo);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// ---------------------------------------------------------------------------------------------------------
// EdgeConv backward: per-point sums for the last BN (partials [PS_BLOCKS][2][C] fp64)
// ---------------------------------------------------------------------------------------------------------
#define PS_BLOCKS 512          // (128 left half the CUs without a workgroup: 47 us for 118 MB)
__global__ __launch_bounds__(256) void gpe_point_sums_kernel(const float* __restrict__ g, int ldg,
                                                             const float* __restrict__ mx,
                                                             const float* __restrict__ mn, int ldagg,
                                                             const float* __restrict__ stats, long rows, int C,
                                                             double* __restrict__ part, unsigned* __restrict__ amax_sg)
{
    // amax_sg (may be NULL): receives max |s_c g_ic| — the data term of the bound of a lazily formed dz3 (gpe_edge_dz3_bound)
    const int c = blockIdx.y * 256 + threadIdx.x;
    double s1 = 0, s2 = 0;
    float gm = 0.f, sabs = 0.f;
    if (c < C) {
        const float mean = stats[c], rstd = stats[C + c], s = stats[2 * C + c];
        // 8 rows in flight per thread (a load per dependent fp64 add was a 512-deep latency chain: 0.4 TB/s)
        const float* sp = (s >= 0.f) ? mx : mn;
        const long st = gridDim.x;
        long r = blockIdx.x;
        for (; r + 7 * st < rows; r += 8 * st) {
            float gv[8], sv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { gv[u] = g[(r + u * st) * ldg + c]; sv[u] = sp[(r + u * st) * ldagg + c]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s1 += (double)gv[u];
                s2 += (double)gv[u] * (double)((sv[u] - mean) * rstd);
                gm = fmaxf(gm, fabsf(gv[u]));
            }
        }
        for (; r < rows; r += st) {
            const float gv = g[r * ldg + c];
            const float sel = sp[r * ldagg + c];
            s1 += (double)gv;
            s2 += (double)gv * (double)((sel - mean) * rstd);
            gm = fmaxf(gm, fabsf(gv));
        }
        part[(size_t)blockIdx.x * 2 * C + c] = s1;
        part[(size_t)blockIdx.x * 2 * C + C + c] = s2;
        sabs = fabsf(s);
    }
    if (amax_sg) {                                   // uniform branch; every wave of the block arrives here
        float m = gm * sabs;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if ((threadIdx.x & 63) == 0) atomicMax(amax_sg, __float_as_uint(m * 1.0000002f));   // |s| * max|g| rounds once more than |s g|
    }
}

extern "C" int gpe_point_sums_blocks(void) { return PS_BLOCKS; }

extern "C" int gpe_edge_bwd_point_sums(const float* g, int ldg, const float* mx, const float* mn, int ldagg,
                                       const float* stats, long rows, int C, double* part, uint32_t* amax_sg, void* stream)
{
    if (!g || !mx || !mn || !stats || !part || rows <= 0 || C <= 0) return GPE_EINVAL;
    if (amax_sg && hipMemsetAsync(amax_sg, 0, sizeof(uint32_t), (hipStream_t)stream) != hipSuccess) return GPE_ELAUNCH;
    hipLaunchKernelGGL(gpe_point_sums_kernel, dim3(PS_BLOCKS, gpe_cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, g, ldg, mx, mn,
                       ldagg, stats, rows, C, part, amax_sg);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// dz3 = (a3>0) ? [slot==argsel]*s*g - c1 - (a3-mean)*k2 : 0, written IN PLACE over the stored activation
// a3 [E][lda3].  One wave per POINT (lanes = column quads): the point's selectors and upstream gradient are loaded once,
// its k message rows are streamed DZ3_RB at a time so that a wave always has DZ3_RB independent 16-B loads in flight
// (one row per wave-iteration was latency-bound at 3.5 TB/s of read+write traffic).
#define DZ3_RB 8
__global__ __launch_bounds__(256) void gpe_dz3_kernel(float* __restrict__ a3, int lda3, const float* __restrict__ g,
                                                      int ldg, const uint8_t* __restrict__ amx,
                                                      const uint8_t* __restrict__ amn, int ldagg,
                                                      const float* __restrict__ coef, long npts, int k, int F,
                                                      float gscale, unsigned* __restrict__ amax_out)
{
    // amax_out (f16x3 mode, else NULL): receives the largest |dz3| written, as the bit pattern of a non-negative float
    __shared__ unsigned amax_red[4];
    if (threadIdx.x < 4) amax_red[threadIdx.x] = 0u;
    __syncthreads();
    float amax_run = 0.f;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = (blockIdx.y * 64 + lane) << 2;
    if (c >= F) return;
    const bool all_slots = amx == nullptr;             // aggr 'add' / 'mean': every message carries the point's gradient
    float cs_[4], c1_[4], k2_[4], mu_[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int cc = (c + t < F) ? c + t : c;
        cs_[t] = coef[cc]; c1_[t] = coef[F + cc]; k2_[t] = coef[2 * F + cc]; mu_[t] = coef[3 * F + cc];
    }
    const long nw = (long)gridDim.x * 4;
    for (long i = (long)blockIdx.x * 4 + wave; i < npts; i += nw) {
        uint8_t mxv[4] = {0, 0, 0, 0}, mnv[4] = {0, 0, 0, 0};
        if (!all_slots) {
            const uchar4 smx = *reinterpret_cast<const uchar4*>(amx + i * ldagg + c);
            const uchar4 smn = *reinterpret_cast<const uchar4*>(amn + i * ldagg + c);
            mxv[0] = smx.x; mxv[1] = smx.y; mxv[2] = smx.z; mxv[3] = smx.w;
            mnv[0] = smn.x; mnv[1] = smn.y; mnv[2] = smn.z; mnv[3] = smn.w;
        }
        int sel[4];
        float sg[4];                                   // s * g of this point, per column of the quad
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int cc = (c + t < F) ? c + t : c;
            sel[t] = (cs_[t] >= 0.f) ? mxv[t] : mnv[t];
            sg[t] = cs_[t] * g[i * ldg + cc] * gscale;
        }
        float* base = a3 + i * k * lda3 + c;
        for (int s0 = 0; s0 < k; s0 += DZ3_RB) {
            float4 a[DZ3_RB];
#pragma unroll
            for (int u = 0; u < DZ3_RB; ++u) {
                const int s_ = (s0 + u < k) ? s0 + u : k - 1;          // clamped: unconditional loads
                a[u] = pw_ld4(base + (long)s_ * lda3);
            }
#pragma unroll
            for (int u = 0; u < DZ3_RB; ++u) {
                if (s0 + u < k) {
                    const float av[4] = {a[u].x, a[u].y, a[u].z, a[u].w};
                    float o[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float hit = (all_slots || sel[t] == s0 + u) ? sg[t] : 0.f;
                        o[t] = (c + t < F && av[t] > 0.f) ? hit - c1_[t] - (av[t] - mu_[t]) * k2_[t] : 0.f;
                    }
                    pw_st4(base + (long)(s0 + u) * lda3, make_float4(o[0], o[1], o[2], o[3]));
                    amax_run = fmaxf(fmaxf(amax_run, fmaxf(fabsf(o[0]), fabsf(o[1]))), fmaxf(fabsf(o[2]), fabsf(o[3])));
                }
            }
        }
    }
    if (amax_out) {                                    // uniform; lanes past F have left, the barrier counts live waves only
        atomicMax(&amax_red[wave], __float_as_uint(amax_run));
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned a = amax_red[0] > amax_red[1] ? amax_red[0] : amax_red[1];
            const unsigned b = amax_red[2] > amax_red[3] ? amax_red[2] : amax_red[3];
            atomicMax(amax_out, a > b ? a : b);
        }
    }
}

static int dz3_launch(float* a3, int lda3, const float* g, int ldg, const uint8_t* amx, const uint8_t* amn, int ldagg,
                      const float* coef, int B, int N, int k, int F, float gscale, unsigned* amax_out, hipStream_t stream)
{
    if (!a3 || !g || !coef || B <= 0 || N <= 0 || k <= 0 || F <= 0 || (lda3 & 3) || lda3 < F) return GPE_EINVAL;
    if (amx && (!amn || (ldagg & 3) || ldagg < F)) return GPE_EINVAL;
    const long E = (long)B * N * k;
    if (E >= (1L << 31)) return GPE_EINVAL;
    const long npts = (long)B * N;
    const int blocks = (int)((npts + 3) / 4 < 4096 ? (npts + 3) / 4 : 4096);
    // amax_out (may be NULL): the caller's word for the largest |dz3| written — the f16x3 scale of the edge GEMMs that read dz3
    if (amax_out && hipMemsetAsync(amax_out, 0, sizeof(unsigned), stream) != hipSuccess) return GPE_ELAUNCH;
    hipLaunchKernelGGL(gpe_dz3_kernel, dim3(blocks, gpe_cdiv(F, 256)), dim3(256), 0, stream, a3, lda3, g, ldg, amx, amn,
                       ldagg, coef, npts, k, F, gscale, amax_out);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_edge_dz3(float* a3, int lda3, const float* g, int ldg, const uint8_t* amx, const uint8_t* amn,
                            int ldagg, const float* coef, int B, int N, int k, int F, uint32_t* amax_out, void* stream)
{
    if (!amx || !amn) return GPE_EINVAL;
    return dz3_launch(a3, lda3, g, ldg, amx, amn, ldagg, coef, B, N, k, F, 1.f, amax_out, (hipStream_t)stream);
}

extern "C" int gpe_edge_dz3_all(float* a3, int lda3, const float* g, int ldg, float gscale, const float* coef, int B,
                                int N, int k, int F, uint32_t* amax_out, void* stream)
{
    return dz3_launch(a3, lda3, g, ldg, nullptr, nullptr, 0, coef, B, N, k, F, gscale, amax_out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------
// kNN graph transposition (one workgroup per cloud) and the pull-style scatter it enables
// ---------------------------------------------------------------------------------------------------------
// LDS_EDGES: the cloud's edge list is scattered and sorted in LDS and written out once, coalesced (it fits up to
// N*k = 32 k edges, the benchmark shape); otherwise the buckets are sorted in place in global memory.
template <bool LDS_EDGES>
__global__ __launch_bounds__(1024) void gpe_knn_reverse_kernel(const int32_t* __restrict__ idx, int N, int k,
                                                               int32_t* __restrict__ rev_off,
                                                               int32_t* __restrict__ rev_edge)
{
    extern __shared__ int sm[];
    int* cnt = sm;                 // [N]
    int* off = sm + N;             // [N+1]
    __shared__ int wsum[16];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int32_t* id = idx + (size_t)b * N * k;
    int32_t* ro = rev_off + (size_t)b * (N + 1);
    int32_t* const re_g = rev_edge + (size_t)b * N * k;
    int32_t* const re = LDS_EDGES ? reinterpret_cast<int32_t*>(sm + 2 * N + 1) : re_g;
    const int E = N * k;
    for (int i = tid; i < N; i += 1024) cnt[i] = 0;
    __syncthreads();
    for (int e = tid; e < E; e += 1024) atomicAdd(&cnt[id[e]], 1);
    __syncthreads();
    // exclusive scan of cnt: each thread owns a contiguous run of `per` entries
    const int per = (N + 1023) / 1024;
    const int beg = tid * per;
    int local = 0;
    for (int i = 0; i < per; ++i) if (beg + i < N) local += cnt[beg + i];
    // block scan of `local` (wave scan + cross-wave)
    int x = local;
    const int lane = tid & 63, wv = tid >> 6;
    for (int d = 1; d < 64; d <<= 1) { int y = __shfl_up(x, d); if (lane >= d) x += y; }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    if (tid == 0) { int a = 0; for (int w = 0; w < 16; ++w) { int t = wsum[w]; wsum[w] = a; a += t; } }
    __syncthreads();
    int run = x - local + wsum[wv];
    for (int i = 0; i < per; ++i) if (beg + i < N) { off[beg + i] = run; run += cnt[beg + i]; }
    if (tid == 1023) off[N] = E;
    __syncthreads();
    for (int i = tid; i <= N; i += 1024) ro[i] = off[i];
    for (int i = tid; i < N; i += 1024) cnt[i] = 0;
    __syncthreads();
    for (int e = tid; e < E; e += 1024) {
        const int jn = id[e];
        const int pos = atomicAdd(&cnt[jn], 1);
        re[off[jn] + pos] = e;
    }
    __threadfence_block();
    __syncthreads();
    // deterministic order inside each bucket: ascending edge id
    for (int jn = tid; jn < N; jn += 1024) {
        const int a = off[jn], z = off[jn + 1];
        for (int i = a + 1; i < z; ++i) {
            const int v = re[i];
            int h = i - 1;
            while (h >= a && re[h] > v) { re[h + 1] = re[h]; --h; }
            re[h + 1] = v;
        }
    }
    if (LDS_EDGES) {
        __syncthreads();
        for (int e = tid; e < E; e += 1024) re_g[e] = re[e];
    }
}

extern "C" int gpe_knn_reverse(const int32_t* idx, int B, int N, int k, int32_t* rev_off, int32_t* rev_edge,
                               void* stream)
{
    if (!idx || !rev_off || !rev_edge || B <= 0 || N <= 0 || k <= 0) return GPE_EINVAL;
    const size_t lds = (size_t)(2 * N + 1) * sizeof(int);
    if (lds > 150 * 1024) return GPE_EINVAL;
    const size_t lds_e = lds + (size_t)N * k * sizeof(int);
    if (lds_e <= 150 * 1024) {
        GPE_ENSURE_MAX_LDS_N((gpe_knn_reverse_kernel<true>), 150 * 1024);
        hipLaunchKernelGGL(gpe_knn_reverse_kernel<true>, dim3(B), dim3(1024), lds_e, (hipStream_t)stream, idx, N, k, rev_off,
                           rev_edge);
    } else {
        GPE_ENSURE_MAX_LDS_N((gpe_knn_reverse_kernel<false>), 150 * 1024);
        hipLaunchKernelGGL(gpe_knn_reverse_kernel<false>, dim3(B), dim3(1024), lds, (hipStream_t)stream, idx, N, k, rev_off,
                           rev_edge);
    }
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

__global__ __launch_bounds__(256) void gpe_pull_dq_kernel(const float* __restrict__ dz, int lddz,
                                                          const int32_t* __restrict__ rev_off,
                                                          const int32_t* __restrict__ rev_edge, int B, int N, int k, int H,
                                                          int pin, float* __restrict__ dQ, int lddq)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = 4 * lane;
    const bool active = c < H;
    // pin: a cloud's dz rows (N*k x H, each read once here, right after the kernel that wrote them) stay on one XCD
    const GpePointWalk wk = gpe_point_walk(B, N, pin);
    for (long u = wk.first; u < wk.count; u += wk.stride) {
        int bi, jn;
        gpe_walk_split(wk, u, N, bi, jn);
        const long b = bi;
        const long pt = b * N + jn;
        const int32_t* ro = rev_off + b * (N + 1);
        const int32_t* re = rev_edge + b * (long)N * k;
        const long e0 = b * (long)N * k;
        const int a = ro[jn], z = ro[jn + 1];
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = a; i < z; i += 4) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (i + u < z && active) v[u] = pw_ld4(dz + (e0 + re[i + u]) * lddz + c);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
        }
        if (active) pw_st4(dQ + pt * lddq + c, acc);
    }
}

extern "C" int gpe_edge_pull_dq(const float* dz, int lddz, const int32_t* rev_off, const int32_t* rev_edge, int B,
                                int N, int k, int H, float* dQ, int lddq, void* stream)
{
    if (!dz || !rev_off || !rev_edge || !dQ || B <= 0 || N <= 0 || k <= 0 || H <= 0 || H > 256 || (H & 3) ||
        (lddz & 3) || (lddq & 3))
        return GPE_EINVAL;
    const long pts = (long)B * N;
    const int pin = gpe_pin_clouds(B) ? 1 : 0;
    int blocks = (int)((pts + 3) / 4 < 2048 ? (pts + 3) / 4 : 2048);
    if (pin) blocks = gpe_round_up(blocks, GPE_NXCD);
    hipLaunchKernelGGL(gpe_pull_dq_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dz, lddz, rev_off,
                       rev_edge, B, N, k, H, pin, dQ, lddq);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

__global__ void gpe_w1_split_kernel(const float* __restrict__ w1, int ldw1, const float* __restrict__ b1, int H,
                                    int C, float* __restrict__ wpq, int ldwpq, float* __restrict__ bias_pq)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < H * C) {
        const int h = e / C, c = e - h * C;
        const float wa = w1[(size_t)h * ldw1 + c], wb = w1[(size_t)h * ldw1 + C + c];
        wpq[(size_t)h * ldwpq + c] = wa - wb;
        wpq[(size_t)(H + h) * ldwpq + c] = wb;
    }
    if (e < 2 * H) bias_pq[e] = (e < H) ? b1[e] : 0.f;
}

extern "C" int gpe_w1_split(const float* w1, int ldw1, const float* b1, int H, int C, float* wpq, int ldwpq,
                            float* bias_pq, void* stream)
{
    if (!w1 || !b1 || !wpq || !bias_pq || H <= 0 || C <= 0 || ldw1 < 2 * C || ldwpq < C) return GPE_EINVAL;
    const int total = (H * C > 2 * H) ? H * C : 2 * H;
    hipLaunchKernelGGL(gpe_w1_split_kernel, dim3(gpe_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w1, ldw1,
                       b1, H, C, wpq, ldwpq, bias_pq);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

__global__ void gpe_w1_grad_kernel(const float* __restrict__ dwpq, int ld, int H, int C, float* __restrict__ dw1,
                                   int lddw1)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= H * C) return;
    const int h = e / C, c = e - h * C;
    const float dp = dwpq[(size_t)h * ld + c], dq = dwpq[(size_t)(H + h) * ld + c];
    dw1[(size_t)h * lddw1 + c] = dp;
    dw1[(size_t)h * lddw1 + C + c] = dq - dp;
}

extern "C" int gpe_w1_grad_from_pq(const float* dwpq, int ld, int H, int C, float* dw1, int lddw1, void* stream)
{
    if (!dwpq || !dw1 || H <= 0 || C <= 0 || ld < C || lddw1 < 2 * C) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_w1_grad_kernel, dim3(gpe_cdiv(H * C, 256)), dim3(256), 0, (hipStream_t)stream, dwpq, ld,
                       H, C, dw1, lddw1);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// ---------------------------------------------------------------------------------------------------------
// explicit EdgeConv message inputs — the general formulation behind DynamicEdgeConv (nn/net_blocks.py:124-135):
//   out[e][0:C] = x_i, out[e][C:2C] = x_j - x_i   for edge e = i*k + s, j = jg[e]  (row pitch ldo >= 2C, pad columns zeroed)
// Used only for first-block widths the fused P|Q path does not take (EConv_hidden not a multiple of 4, or > 256): the edge MLP
// then runs as a dense MLP over the E message rows.  Backward: gx_i = sum_s (g1 - g2)[i*k+s] + sum_{e : jg[e] = i} g2[e],
// the second sum pulled through the transposed graph in ascending edge order (deterministic, no atomics).
// ---------------------------------------------------------------------------------------------------------
__global__ void gpe_edge_inputs_fwd_kernel(const float* __restrict__ x, int ldx, int C, const int32_t* __restrict__ jg, int k,
                                           long E, float* __restrict__ out, int ldo)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= E * ldo) return;
    const long e = t / ldo;
    const int c = (int)(t - e * ldo);
    float v = 0.f;
    if (c < 2 * C) {
        const long i = e / k;
        const float xi = x[i * ldx + (c < C ? c : c - C)];
        v = (c < C) ? xi : x[(long)jg[e] * ldx + (c - C)] - xi;
    }
    out[t] = v;
}

extern "C" int gpe_edge_inputs_fwd(const float* x, int ldx, int C, const int32_t* jg, long npts, int k, float* out, int ldo,
                                   void* stream)
{
    if (!x || !jg || !out || C <= 0 || ldx < C || npts <= 0 || k <= 0 || ldo < 2 * C) return GPE_EINVAL;
    const long total = npts * k * ldo;
    hipLaunchKernelGGL(gpe_edge_inputs_fwd_kernel, dim3((unsigned)gpe_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx,
                       C, jg, k, npts * k, out, ldo);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// rev_off [B][N+1], rev_edge [B][N*k]: the transposed graph of gpe_knn_reverse (edge numbers LOCAL to the cloud)
__global__ void gpe_edge_inputs_bwd_kernel(const float* __restrict__ g, int ldg, int C, const int32_t* __restrict__ rev_off,
                                           const int32_t* __restrict__ rev_edge, int N, int k, long npts,
                                           float* __restrict__ gx, int ldgx)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= npts * C) return;
    const long i = t / C;
    const int c = (int)(t - i * C);
    const long b = i / N;
    const int il = (int)(i - b * N);
    float s = 0.f;
    for (int sl = 0; sl < k; ++sl) {
        const float* row = g + (i * k + sl) * ldg;
        s += row[c] - row[C + c];
    }
    const int32_t* off = rev_off + b * (N + 1);
    const int32_t* ed = rev_edge + b * (long)N * k;
    const long ebase = b * (long)N * k;
    for (int q = off[il]; q < off[il + 1]; ++q) s += g[(ebase + ed[q]) * ldg + C + c];
    gx[i * ldgx + c] = s;
}

extern "C" int gpe_edge_inputs_bwd(const float* g, int ldg, int C, const int32_t* rev_off, const int32_t* rev_edge, int B,
                                   int N, int k, float* gx, int ldgx, void* stream)
{
    if (!g || !rev_off || !rev_edge || !gx || C <= 0 || ldg < 2 * C || B <= 0 || N <= 0 || k <= 0 || ldgx < C) return GPE_EINVAL;
    const long total = (long)B * N * C;
    hipLaunchKernelGGL(gpe_edge_inputs_bwd_kernel, dim3((unsigned)gpe_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, g, ldg,
                       C, rev_off, rev_edge, N, k, (long)B * N, gx, ldgx);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
