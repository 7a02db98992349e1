// DynamicASAPool (nn/net_blocks.py:194-218): PyG ASAPooling on the kNN graph of the node features, forward and backward.
// The graph comes from gpe_knn (k = min(10, N)) and gpe_knn_reverse: target c receives from every query q with c in kNN(q)
// (torch_cluster's [query, neighbour] rows, not flipped), plus one self-loop (add_remaining_self_loops), so
//   cluster(c) = {c} + {q != c : c in kNN(q)}      members in this order: c first, then the reverse bucket (ascending edge id q*k+s)
// Query branch folded: att_q(lin(x_q)) = u . x_q + s0 with u = W_lin^T w_q, s0 = w_q . b_lin + b_att (no F x F GEMM).
// All arithmetic is fp32 (weight-gradient sums in fp64), whatever the arithmetic mode of the edge kernels; no atomics anywhere,
// and every launch grid is a function of (B, N, F) only, so results are bit-identical run to run and across devices.
#include "gpe_device.h"
#include <math.h>

namespace {

constexpr int ASAP_WAVES = 4;                 // waves per workgroup of the per-node kernels
constexpr int ASAP_THREADS = 64 * ASAP_WAVES;
constexpr int ASAP_FMAX = 512;
constexpr int ASAP_FPL = ASAP_FMAX / 64;      // channels per lane at most
constexpr int ASAP_NMAX = 8192;
constexpr int ASAP_HEAD = 1024;               // state words in front of the per-node arrays: u [512], s0
constexpr int ASAP_NBLK_MAX = 1024;           // weight-gradient partial rows at most = workgroups of the per-source pull

__device__ __forceinline__ float wave_sum(float v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}

// state layout (4-byte words; include/gpe_hip.h gpe_asap_fwd)
struct AsapState {
    float* u; float* s0; float* xp; int32_t* win; float* alpha; float* aself; float* t; float* s;
    float* A; float* Bv; float* L3; float* fit; int32_t* deg;       // L3: lin3(x'), then the fitness pre-activation
};
__host__ __device__ inline AsapState asap_state(float* st, long BN, int F, int k)
{
    AsapState o;
    o.u = st;
    o.s0 = st + 512;
    float* p = st + ASAP_HEAD;
    o.xp = p; p += BN * F;
    o.win = reinterpret_cast<int32_t*>(p); p += BN * F;
    o.alpha = p; p += BN * k;
    o.aself = p; p += BN;
    o.t = p; p += BN;
    o.s = p; p += BN;
    o.A = p; p += BN;
    o.Bv = p; p += BN;
    o.L3 = p; p += BN;
    o.fit = p; p += BN;
    o.deg = reinterpret_cast<int32_t*>(p);
    return o;
}

struct AsapParams {
    const float* w_lin; const float* b_lin; const float* w_att; const float* b_att;
    const float* w1; const float* b1; const float* w2; const float* w3; const float* b3;
};

// ---- forward ------------------------------------------------------------------------------------------------------------
// t[n] = w_x . x[n] (one wave per node); the last workgroup also folds the query branch: u = W_lin^T w_q, s0.
__global__ __launch_bounds__(ASAP_THREADS) void asap_prep_kernel(const float* __restrict__ x, int ldx, long BN, int F,
                                                                 AsapParams P, float* __restrict__ st, int k)
{
    AsapState S = asap_state(st, BN, F, k);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (blockIdx.x == gridDim.x - 1) {
        for (int j = threadIdx.x; j < F; j += ASAP_THREADS) {
            float a = 0.f;
            for (int i = 0; i < F; ++i) a = fmaf(P.w_lin[(long)i * F + j], P.w_att[i], a);
            S.u[j] = a;
        }
        if (wid == 0) {
            float a = 0.f;
            for (int i = lane; i < F; i += 64) a = fmaf(P.w_att[i], P.b_lin[i], a);
            a = wave_sum(a);
            if (lane == 0) S.s0[0] = a + P.b_att[0];
        }
        return;
    }
    const long n = (long)blockIdx.x * ASAP_WAVES + wid;
    if (n >= BN) return;
    const float* xr = x + n * ldx;
    float a = 0.f;
    for (int f = lane; f < F; f += 64) a = fmaf(P.w_att[F + f], xr[f], a);
    a = wave_sum(a);
    if (lane == 0) S.t[n] = a;
}

// one wave per target c: channel max over cluster(c) (+ winners), score, softmax, x'_c, the three LEConv node dots
__global__ __launch_bounds__(ASAP_THREADS) void asap_cluster_kernel(const float* __restrict__ x, int ldx, int B, int N, int F,
                                                                    int k, const int32_t* __restrict__ rev_off,
                                                                    const int32_t* __restrict__ rev_edge, AsapParams P,
                                                                    float* __restrict__ st)
{
    const long BN = (long)B * N;
    AsapState S = asap_state(st, BN, F, k);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long gc = (long)blockIdx.x * ASAP_WAVES + wid;
    if (gc >= BN) return;
    const int b = (int)(gc / N), c = (int)(gc - (long)b * N);
    const long base = (long)b * N;
    const int32_t* ro = rev_off + (long)b * (N + 1);
    const int32_t* re = rev_edge + (long)b * N * k;
    const int e0 = ro[c], cnt = ro[c + 1] - e0;
    const int nf = (F + 63) >> 6;

    // pass 1 (lanes over channels): channel max, lowest source index on ties
    float mx[ASAP_FPL];
    int wn[ASAP_FPL];
#pragma unroll
    for (int j = 0; j < ASAP_FPL; ++j) {
        const int f = lane + 64 * j;
        mx[j] = (j < nf && f < F) ? x[gc * ldx + f] : 0.f;
        wn[j] = c;
    }
    for (int m = 0; m < cnt; ++m) {
        const int q = re[e0 + m] / k;
        if (q == c) continue;
        const float* xr = x + (base + q) * ldx;
#pragma unroll
        for (int j = 0; j < ASAP_FPL; ++j) {
            const int f = lane + 64 * j;
            if (j < nf && f < F) {
                const float v = xr[f];
                if (v > mx[j] || (v == mx[j] && q < wn[j])) { mx[j] = v; wn[j] = q; }
            }
        }
    }
    float sc = 0.f;
#pragma unroll
    for (int j = 0; j < ASAP_FPL; ++j) {
        const int f = lane + 64 * j;
        if (j < nf && f < F) {
            sc = fmaf(S.u[f], mx[j], sc);
            S.win[gc * F + f] = base + wn[j];
        }
    }
    sc = wave_sum(sc) + S.s0[0];
    if (lane == 0) S.s[gc] = sc;

    // pass 2 (lanes over members; member 0 = the self-loop): softmax statistics of leaky_relu(s_c + t_q, 0.2)
    const int nm = cnt + 1;
    float emax = -INFINITY;
    for (int m0 = 0; m0 < nm; m0 += 64) {
        const int m = m0 + lane;
        if (m < nm) {
            const int q = m == 0 ? c : re[e0 + m - 1] / k;
            if (m == 0 || q != c) {
                const float z = sc + S.t[base + q];
                emax = fmaxf(emax, z > 0.f ? z : 0.2f * z);
            }
        }
    }
    emax = wave_max(emax);
    float esum = 0.f;
    int deg = 0;
    for (int m0 = 0; m0 < nm; m0 += 64) {
        const int m = m0 + lane;
        if (m < nm) {
            const int q = m == 0 ? c : re[e0 + m - 1] / k;
            if (m == 0 || q != c) {
                const float z = sc + S.t[base + q];
                esum += expf((z > 0.f ? z : 0.2f * z) - emax);
                ++deg;
            }
        }
    }
    esum = wave_sum(esum);
    for (int d = 32; d >= 1; d >>= 1) deg += __shfl_xor(deg, d);
    const float den = esum + 1e-16f;

    // pass 3: alpha (stored in the SOURCE's slot layout; the q == c slot holds 0) and x'_c = sum alpha x_q
    float acc[ASAP_FPL];
#pragma unroll
    for (int j = 0; j < ASAP_FPL; ++j) acc[j] = 0.f;
    for (int m0 = 0; m0 < nm; m0 += 64) {
        const int m = m0 + lane;
        int q = -1;
        float al = 0.f;
        if (m < nm) {
            const int e = m == 0 ? -1 : re[e0 + m - 1];
            q = m == 0 ? c : e / k;
            if (m == 0 || q != c) {
                const float z = sc + S.t[base + q];
                al = expf((z > 0.f ? z : 0.2f * z) - emax) / den;
            } else {
                q = -1;
            }
            if (m == 0) S.aself[gc] = al;
            else S.alpha[base * k + e] = al;
        }
        const int lim = min(64, nm - m0);
        for (int jj = 0; jj < lim; ++jj) {
            const int qq = __shfl(q, jj);
            const float aa = __shfl(al, jj);
            if (qq < 0) continue;
            const float* xr = x + (base + qq) * ldx;
#pragma unroll
            for (int j = 0; j < ASAP_FPL; ++j) {
                const int f = lane + 64 * j;
                if (j < nf && f < F) acc[j] = fmaf(aa, xr[f], acc[j]);
            }
        }
    }
    float dA = 0.f, dB = 0.f, d3 = 0.f;
#pragma unroll
    for (int j = 0; j < ASAP_FPL; ++j) {
        const int f = lane + 64 * j;
        if (j < nf && f < F) {
            S.xp[gc * F + f] = acc[j];
            dA = fmaf(P.w1[f], acc[j], dA);
            dB = fmaf(P.w2[f], acc[j], dB);
            d3 = fmaf(P.w3[f], acc[j], d3);
        }
    }
    dA = wave_sum(dA);
    dB = wave_sum(dB);
    d3 = wave_sum(d3);
    if (lane == 0) {
        S.A[gc] = dA + P.b1[0];
        S.Bv[gc] = dB;
        S.L3[gc] = d3 + P.b3[0];
        S.deg[gc] = deg;
    }
}

__device__ __forceinline__ unsigned long long asap_key(float fit, int c)
{
    // ascending key = fitness descending, then index ascending (order-preserving map of the float's bits)
    unsigned u = __float_as_uint(fit);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)(~u) << 32) | (unsigned)c;
}

// one workgroup per cloud: fitness = sigmoid(LEConv), bitonic sort of (fitness desc, index asc), the first M rows -> out
__global__ __launch_bounds__(1024) void asap_select_kernel(int N, int F, int k, int M, int P2, const int32_t* __restrict__ rev_off,
                                                           const int32_t* __restrict__ rev_edge, float* __restrict__ st, long BN,
                                                           float* __restrict__ out, int32_t* __restrict__ perm,
                                                           int32_t* __restrict__ rank)
{
    extern __shared__ unsigned long long keys[];
    AsapState S = asap_state(st, BN, F, k);
    const int b = blockIdx.x, tid = threadIdx.x;
    const long base = (long)b * N;
    const int32_t* ro = rev_off + (long)b * (N + 1);
    const int32_t* re = rev_edge + (long)b * N * k;
    for (int c = tid; c < P2; c += 1024) {
        if (c >= N) { keys[c] = ~0ull; continue; }
        float pre = S.A[base + c];
        for (int e = ro[c]; e < ro[c + 1]; ++e) {
            const int q = re[e] / k;
            if (q != c) pre += S.A[base + q];
        }
        pre = pre - (float)S.deg[base + c] * S.Bv[base + c] + S.L3[base + c];
        const float fit = gpe_sigmoid(pre);
        S.fit[base + c] = fit;
        S.L3[base + c] = pre;                // the L3 slot keeps the pre-activation from here on (for the backward)
        rank[base + c] = -1;
        keys[c] = asap_key(fit, c);
    }
    __syncthreads();
    for (int size = 2; size <= P2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < P2; i += 1024) {
                const int j = i ^ stride;
                if (j > i) {
                    const unsigned long long a = keys[i], z = keys[j];
                    const bool up = (i & size) == 0;
                    if ((a > z) == up) { keys[i] = z; keys[j] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int r = tid; r < M; r += 1024) {
        const int c = (int)(keys[r] & 0xffffffffu);
        perm[(long)b * M + r] = (int32_t)(base + c);
        rank[base + c] = (int32_t)((long)b * M + r);
    }
    for (long i = tid; i < (long)M * F; i += 1024) {
        const int r = (int)(i / F), f = (int)(i - (long)r * F);
        const long gc = base + (long)(keys[r] & 0xffffffffu);
        out[((long)b * M + r) * F + f] = S.xp[gc * F + f] * S.fit[gc];
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------
struct AsapBws { double* part; double* red; float* dpre; float* dA; float* ds; float* G; float* dz; float* dzself; };
__host__ __device__ inline int asap_nblk(long BN) { long n = (BN + 15) / 16; return (int)(n < ASAP_NBLK_MAX ? n : ASAP_NBLK_MAX); }
__host__ __device__ inline AsapBws asap_bws(void* ws, long BN, int F, int k)
{
    AsapBws o;
    const long R = 5L * F + 3;
    o.part = static_cast<double*>(ws);
    o.red = o.part + (long)asap_nblk(BN) * R;
    float* p = reinterpret_cast<float*>(o.red + R);
    o.dpre = p; p += BN;
    o.dA = p; p += BN;
    o.ds = p; p += BN;
    o.G = p; p += BN * F;
    o.dz = p; p += BN * k;
    o.dzself = p;
    return o;
}

// dpre_c = (dout_r . x'_c) sigmoid'(pre_c) for a kept node (row r), else 0
__global__ __launch_bounds__(ASAP_THREADS) void asap_dpre_kernel(const float* __restrict__ dout, long BN, int F, int k,
                                                                 const int32_t* __restrict__ rank, float* __restrict__ st,
                                                                 void* ws)
{
    AsapState S = asap_state(st, BN, F, k);
    AsapBws W = asap_bws(ws, BN, F, k);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long gc = (long)blockIdx.x * ASAP_WAVES + wid;
    if (gc >= BN) return;
    const int r = rank[gc];
    if (r < 0) {
        if (lane == 0) W.dpre[gc] = 0.f;
        return;
    }
    float a = 0.f;
    for (int f = lane; f < F; f += 64) a = fmaf(dout[(long)r * F + f], S.xp[gc * F + f], a);
    a = wave_sum(a);
    // sigmoid' = sigmoid(pre) sigmoid(-pre): no cancellation in 1 - fit where the fitness saturates
    const float pre = S.L3[gc];
    if (lane == 0) W.dpre[gc] = a * (S.fit[gc] * gpe_sigmoid(-pre));
}

// one wave per target c: G_c = dL/dx'_c, then the attention backward over cluster(c) -> dz per edge, ds_c
__global__ __launch_bounds__(ASAP_THREADS) void asap_node_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ x,
                                                                     int ldx, int B, int N, int F, int k,
                                                                     const int32_t* __restrict__ idx,
                                                                     const int32_t* __restrict__ rev_off,
                                                                     const int32_t* __restrict__ rev_edge,
                                                                     const int32_t* __restrict__ rank, AsapParams P,
                                                                     float* __restrict__ st, void* ws)
{
    const long BN = (long)B * N;
    AsapState S = asap_state(st, BN, F, k);
    AsapBws W = asap_bws(ws, BN, F, k);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long gc = (long)blockIdx.x * ASAP_WAVES + wid;
    if (gc >= BN) return;
    const int b = (int)(gc / N), c = (int)(gc - (long)b * N);
    const long base = (long)b * N;
    const int nf = (F + 63) >> 6;
    // dA_c: dpre over every target c sends to = itself + its forward kNN list (without c)
    const float dp = W.dpre[gc];
    float dA = dp;
    for (int s = 0; s < k; ++s) {
        const int t = idx[gc * k + s];
        if (t != c) dA += W.dpre[base + t];
    }
    const float dB = -(float)S.deg[gc] * dp;
    const int r = rank[gc];
    const float fit = S.fit[gc];
    float G[ASAP_FPL];
#pragma unroll
    for (int j = 0; j < ASAP_FPL; ++j) {
        const int f = lane + 64 * j;
        G[j] = 0.f;
        if (j < nf && f < F) {
            float g = r >= 0 ? dout[(long)r * F + f] * fit : 0.f;
            g = fmaf(dA, P.w1[f], g);
            g = fmaf(dB, P.w2[f], g);
            g = fmaf(dp, P.w3[f], g);
            G[j] = g;
            W.G[gc * F + f] = g;
        }
    }
    if (lane == 0) W.dA[gc] = dA;

    const int32_t* ro = rev_off + (long)b * (N + 1);
    const int32_t* re = rev_edge + (long)b * N * k;
    const int e0 = ro[c], nm = ro[c + 1] - e0 + 1;
    const float sc = S.s[gc];
    // pass A: sum over members of alpha * dalpha, dalpha_cq = G_c . x_q
    float sad = 0.f;
    for (int m = 0; m < nm; ++m) {
        const int e = m == 0 ? -1 : re[e0 + m - 1];
        const int q = m == 0 ? c : e / k;
        if (m > 0 && q == c) continue;
        const float* xr = x + (base + q) * ldx;
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < ASAP_FPL; ++j) {
            const int f = lane + 64 * j;
            if (j < nf && f < F) d = fmaf(G[j], xr[f], d);
        }
        d = wave_sum(d);
        const float al = m == 0 ? S.aself[gc] : S.alpha[base * k + e];
        sad = fmaf(al, d, sad);
    }
    // pass B, chunks of 64 members: dalpha again (lane m0 + jj keeps its own), then softmax and leaky_relu backward
    float dsum = 0.f;
    for (int m0 = 0; m0 < nm; m0 += 64) {
        const int lim = min(64, nm - m0);
        float mine = 0.f;
        for (int jj = 0; jj < lim; ++jj) {
            const int m = m0 + jj;
            const int q = m == 0 ? c : re[e0 + m - 1] / k;
            if (m > 0 && q == c) continue;
            const float* xr = x + (base + q) * ldx;
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < ASAP_FPL; ++j) {
                const int f = lane + 64 * j;
                if (j < nf && f < F) d = fmaf(G[j], xr[f], d);
            }
            d = wave_sum(d);
            if (lane == jj) mine = d;
        }
        const int m = m0 + lane;
        if (m < nm) {
            const int e = m == 0 ? -1 : re[e0 + m - 1];
            const int q = m == 0 ? c : e / k;
            float dzv = 0.f;
            if (m == 0 || q != c) {
                const float al = m == 0 ? S.aself[gc] : S.alpha[base * k + e];
                const float z = sc + S.t[base + q];
                const float de = al * (mine - sad);
                dzv = z > 0.f ? de : 0.2f * de;
            }
            dsum += dzv;
            if (m == 0) W.dzself[gc] = dzv;
            else W.dz[base * k + e] = dzv;
        }
    }
    dsum = wave_sum(dsum);
    if (lane == 0) W.ds[gc] = dsum;
}

// one wave per source q (grid-stride, fixed grid): dx_q = sum_c alpha_cq G_c + (sum_c dz_cq) w_x + sum_c [winner_c == q] ds_c u,
// plus the fp64 partial sums of the parameter gradients, combined per workgroup in wave order
__global__ __launch_bounds__(ASAP_THREADS) void asap_src_bwd_kernel(const float* __restrict__ x, int ldx, int B, int N, int F, int k,
                                                                    const int32_t* __restrict__ idx, AsapParams P,
                                                                    float* __restrict__ st, void* ws, float* __restrict__ dx,
                                                                    int lddx)
{
    __shared__ double red[5 * ASAP_FMAX + 3];
    const long BN = (long)B * N;
    AsapState S = asap_state(st, BN, F, k);
    AsapBws W = asap_bws(ws, BN, F, k);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int nf = (F + 63) >> 6;
    double pv[ASAP_FPL], px[ASAP_FPL], p1[ASAP_FPL], p2[ASAP_FPL], p3[ASAP_FPL];
#pragma unroll
    for (int j = 0; j < ASAP_FPL; ++j) pv[j] = px[j] = p1[j] = p2[j] = p3[j] = 0.0;
    double sg = 0.0, sb1 = 0.0, sb3 = 0.0;
    const long nw = (long)gridDim.x * ASAP_WAVES;
    for (long gq = (long)blockIdx.x * ASAP_WAVES + wid; gq < BN; gq += nw) {
        const int b = (int)(gq / N), q = (int)(gq - (long)b * N);
        const long base = (long)b * N;
        float acc[ASAP_FPL];
        float al = S.aself[gq];
        float dt = W.dzself[gq];
        {
            const float dsq = W.ds[gq];
#pragma unroll
            for (int j = 0; j < ASAP_FPL; ++j) {
                const int f = lane + 64 * j;
                acc[j] = 0.f;
                if (j < nf && f < F) {
                    acc[j] = al * W.G[gq * F + f];
                    if (S.win[gq * F + f] == gq) acc[j] = fmaf(dsq, S.u[f], acc[j]);
                }
            }
        }
        for (int s = 0; s < k; ++s) {
            const int c = idx[gq * k + s];
            if (c == q) continue;
            const long gc = base + c;
            const float a = S.alpha[gq * k + s];
            const float dsc = W.ds[gc];
            dt += W.dz[gq * k + s];
#pragma unroll
            for (int j = 0; j < ASAP_FPL; ++j) {
                const int f = lane + 64 * j;
                if (j < nf && f < F) {
                    acc[j] = fmaf(a, W.G[gc * F + f], acc[j]);
                    if (S.win[gc * F + f] == gq) acc[j] = fmaf(dsc, S.u[f], acc[j]);
                }
            }
        }
        const float dsq = W.ds[gq], dAq = W.dA[gq], dp = W.dpre[gq];
        const float dBq = -(float)S.deg[gq] * dp;
#pragma unroll
        for (int j = 0; j < ASAP_FPL; ++j) {
            const int f = lane + 64 * j;
            if (j < nf && f < F) {
                dx[gq * lddx + f] = fmaf(dt, P.w_att[F + f], acc[j]);
                const float xq = x[(long)S.win[gq * F + f] * ldx + f];
                const float xpf = S.xp[gq * F + f];
                pv[j] += (double)dsq * xq;
                px[j] += (double)dt * x[gq * ldx + f];
                p1[j] += (double)dAq * xpf;
                p2[j] += (double)dBq * xpf;
                p3[j] += (double)dp * xpf;
            }
        }
        sg += dsq;
        sb1 += dAq;
        sb3 += dp;
    }
    // workgroup combine in wave order, then one partial row per workgroup
    for (int w = 0; w < ASAP_WAVES; ++w) {
        if (wid == w) {
#pragma unroll
            for (int j = 0; j < ASAP_FPL; ++j) {
                const int f = lane + 64 * j;
                if (j < nf && f < F) {
                    red[f] = (w ? red[f] : 0.0) + pv[j];
                    red[F + f] = (w ? red[F + f] : 0.0) + px[j];
                    red[2 * F + f] = (w ? red[2 * F + f] : 0.0) + p1[j];
                    red[3 * F + f] = (w ? red[3 * F + f] : 0.0) + p2[j];
                    red[4 * F + f] = (w ? red[4 * F + f] : 0.0) + p3[j];
                }
            }
            if (lane == 0) {
                red[5 * F] = (w ? red[5 * F] : 0.0) + sg;
                red[5 * F + 1] = (w ? red[5 * F + 1] : 0.0) + sb1;
                red[5 * F + 2] = (w ? red[5 * F + 2] : 0.0) + sb3;
            }
        }
        __syncthreads();
    }
    const int R = 5 * F + 3;
    for (int i = threadIdx.x; i < R; i += ASAP_THREADS) W.part[(long)blockIdx.x * R + i] = red[i];
}

// column sums of the partial rows (rows in ascending order, per wave a fixed stripe, stripes combined in wave order)
__global__ __launch_bounds__(ASAP_THREADS) void asap_red_kernel(long BN, int F, int k, void* ws)
{
    __shared__ double sm[ASAP_WAVES][64];
    AsapBws W = asap_bws(ws, BN, F, k);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int R = 5 * F + 3, nblk = asap_nblk(BN);
    const int col = blockIdx.x * 64 + lane;
    double a = 0.0;
    if (col < R)
        for (int r = wid; r < nblk; r += ASAP_WAVES) a += W.part[(long)r * R + col];
    sm[wid][lane] = a;
    __syncthreads();
    if (wid == 0 && col < R) W.red[col] = ((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane];
}

// the nine parameter gradients from the reduced sums (v, dw_x, dw1, dw2, dw3, sigma, db1, db3)
__global__ __launch_bounds__(1024) void asap_finalize_kernel(long BN, int F, int k, AsapParams P, void* ws, float* g_wlin,
                                                             float* g_blin, float* g_watt, float* g_batt, float* g_w1, float* g_b1,
                                                             float* g_w2, float* g_w3, float* g_b3)
{
    AsapBws W = asap_bws(ws, BN, F, k);
    const double* v = W.red;
    const double sig = W.red[5 * F];
    for (long i = threadIdx.x; i < (long)F * F; i += 1024) {
        const int r = (int)(i / F), cc = (int)(i - (long)r * F);
        g_wlin[i] = (float)((double)P.w_att[r] * v[cc]);
    }
    for (int i = threadIdx.x; i < F; i += 1024) {
        double a = 0.0;
        for (int j = 0; j < F; ++j) a += (double)P.w_lin[(long)i * F + j] * v[j];
        g_blin[i] = (float)(sig * P.w_att[i]);
        g_watt[i] = (float)(a + sig * P.b_lin[i]);
        g_watt[F + i] = (float)W.red[F + i];
        g_w1[i] = (float)W.red[2 * F + i];
        g_w2[i] = (float)W.red[3 * F + i];
        g_w3[i] = (float)W.red[4 * F + i];
    }
    if (threadIdx.x == 0) {
        g_batt[0] = (float)sig;
        g_b1[0] = (float)W.red[5 * F + 1];
        g_b3[0] = (float)W.red[5 * F + 2];
    }
}

inline bool asap_dims_ok(int B, int N, int F, int k, int ldx)
{
    return B > 0 && N > 0 && N <= ASAP_NMAX && F >= 1 && F <= ASAP_FMAX && k >= 1 && k <= N && k <= 64 && ldx >= F &&
           (long)B * N * k < (1L << 31) && (long)B * N * F < (1L << 31);
}

}  // namespace

extern "C" int gpe_asap_fwd(const float* x, int ldx, int B, int N, int F, int k, const int32_t* rev_off, const int32_t* rev_edge,
                            const float* w_lin, const float* b_lin, const float* w_att, const float* b_att, const float* w1,
                            const float* b1, const float* w2, const float* w3, const float* b3, int M, float* out, int32_t* perm,
                            int32_t* rank, float* state, void* stream)
{
    if (!x || !rev_off || !rev_edge || !w_lin || !b_lin || !w_att || !b_att || !w1 || !b1 || !w2 || !w3 || !b3 || !out ||
        !perm || !rank || !state || !asap_dims_ok(B, N, F, k, ldx) || M < 1 || M > N)
        return GPE_EINVAL;
    const AsapParams P = {w_lin, b_lin, w_att, b_att, w1, b1, w2, w3, b3};
    const long BN = (long)B * N;
    hipStream_t s = (hipStream_t)stream;
    const int nb = gpe_cdiv(BN, ASAP_WAVES);
    hipLaunchKernelGGL(asap_prep_kernel, dim3(nb + 1), dim3(ASAP_THREADS), 0, s, x, ldx, BN, F, P, state, k);
    GPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(asap_cluster_kernel, dim3(nb), dim3(ASAP_THREADS), 0, s, x, ldx, B, N, F, k, rev_off, rev_edge, P, state);
    GPE_CHECK_LAUNCH();
    int P2 = 1;
    while (P2 < N) P2 <<= 1;
    const size_t lds = (size_t)P2 * sizeof(unsigned long long);
    GPE_ENSURE_MAX_LDS_N(asap_select_kernel, 64 * 1024);
    hipLaunchKernelGGL(asap_select_kernel, dim3(B), dim3(1024), lds, s, N, F, k, M, P2, rev_off, rev_edge, state, BN, out, perm,
                       rank);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_asap_bwd(const float* dout, const float* x, int ldx, int B, int N, int F, int k, const int32_t* idx,
                            const int32_t* rev_off, const int32_t* rev_edge, const float* w_lin, const float* b_lin,
                            const float* w_att, const float* b_att, const float* w1, const float* b1, const float* w2,
                            const float* w3, const float* b3, const int32_t* rank, const float* state, float* dx, int lddx,
                            float* g_wlin, float* g_blin, float* g_watt, float* g_batt, float* g_w1, float* g_b1, float* g_w2,
                            float* g_w3, float* g_b3, void* ws, void* stream)
{
    if (!dout || !x || !idx || !rev_off || !rev_edge || !w_lin || !b_lin || !w_att || !b_att || !w1 || !b1 || !w2 || !w3 || !b3 ||
        !rank || !state || !dx || !g_wlin || !g_blin || !g_watt || !g_batt || !g_w1 || !g_b1 || !g_w2 || !g_w3 || !g_b3 || !ws ||
        !asap_dims_ok(B, N, F, k, ldx) || lddx < F || (((uintptr_t)ws) & 15))
        return GPE_EINVAL;
    const AsapParams P = {w_lin, b_lin, w_att, b_att, w1, b1, w2, w3, b3};
    const long BN = (long)B * N;
    hipStream_t s = (hipStream_t)stream;
    float* st = const_cast<float*>(state);
    const int nb = gpe_cdiv(BN, ASAP_WAVES);
    hipLaunchKernelGGL(asap_dpre_kernel, dim3(nb), dim3(ASAP_THREADS), 0, s, dout, BN, F, k, rank, st, ws);
    GPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(asap_node_bwd_kernel, dim3(nb), dim3(ASAP_THREADS), 0, s, dout, x, ldx, B, N, F, k, idx, rev_off, rev_edge,
                       rank, P, st, ws);
    GPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(asap_src_bwd_kernel, dim3(asap_nblk(BN)), dim3(ASAP_THREADS), 0, s, x, ldx, B, N, F, k, idx, P, st, ws, dx,
                       lddx);
    GPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(asap_red_kernel, dim3(gpe_cdiv(5L * F + 3, 64)), dim3(ASAP_THREADS), 0, s, BN, F, k, ws);
    GPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(asap_finalize_kernel, dim3(1), dim3(1024), 0, s, BN, F, k, P, ws, g_wlin, g_blin, g_watt, g_batt, g_w1, g_b1,
                       g_w2, g_w3, g_b3);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
