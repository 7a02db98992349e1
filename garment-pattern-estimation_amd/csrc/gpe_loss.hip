// The losses behind the encoder/decoder path, as gfx950 kernels:
//   * pattern loss (MSE shape / rotation / translation + panel loop loss) value and gradient, and the ground-truth
//     pre-processing in front of it (panel-origin matching, greedy panel-order matching)
//       nn/metrics/composed_loss.py:294-334,530-570,656-703  and  nn/metrics/losses.py:19-51
//   * entmax.SparsemaxLoss() as the reference calls it (nn/metrics/composed_loss.py:4,196,323-332)
// All of it is bandwidth- or latency-bound small work: no MFMA here.  Reductions run in fp64 with a fixed order, so
// results are run-to-run deterministic; there are no float atomics.
#include "gpe_device.h"
#include <math.h>

// =====================================================================================================================
// pattern loss
// =====================================================================================================================
// Predictions are strided views (the output dict holds slices of one [B,P,L,8] and one [B*P,7] tensor):
//   outlines element (b,p,l,c) at ol + b*ol_sb + p*ol_sp + l*ol_sl + c           (c < 4)
//   rotations (b,p,c) at rot + (b*P+p)*rot_s + c  (c < R);  translations likewise (c < T)
// Ground truth is dense: gt_ol [B,P,L,4], gt_rot [B,P,R], gt_tr [B,P,T], num_edges int32 [B*P].
// flags: bit0 shape, bit1 loop, bit2 rotation, bit3 translation.
//   shape = mean (ol-gt)^2 ; rotation / translation likewise ; loop = sum_panels |sum_{l<n} (ol[l,:2]-pad)|^2 / (2*B*P),
//   panels with n < 3 skipped (nn/metrics/losses.py:36-51).
struct LossParams {
    const float* ol; long ol_sb, ol_sp, ol_sl;
    const float* rot; long rot_s;
    const float* tr; long tr_s;
    const float* gt_ol; const float* gt_rot; const float* gt_tr; const int32_t* num_edges;
    int B, P, L, R, T, flags;
    float pad0, pad1, loop_w;
};

#define LOSS_TPB 256
__global__ __launch_bounds__(LOSS_TPB) void gpe_loss_fwd_kernel(LossParams p, double* __restrict__ part /* [B][4] */,
                                                                float* __restrict__ loop_sums /* [B*P][2] */)
{
    __shared__ double red[4][LOSS_TPB];
    const int b = blockIdx.x, tid = threadIdx.x;
    double s_shape = 0, s_loop = 0, s_rot = 0, s_tr = 0;
    if (p.flags & 1) {
        const int n = p.P * p.L * 4;
        for (int e = tid; e < n; e += LOSS_TPB) {
            const int c = e & 3, l = (e >> 2) % p.L, pp = (e >> 2) / p.L;
            const float d = p.ol[b * p.ol_sb + pp * p.ol_sp + l * p.ol_sl + c] - p.gt_ol[(size_t)b * n + e];
            s_shape += (double)d * d;
        }
    }
    if (p.flags & 2) {
        // thread (panel, coordinate): sequential sum over the panel's first n edges
        for (int e = tid; e < p.P * 2; e += LOSS_TPB) {
            const int pp = e >> 1, c = e & 1;
            const int n = p.num_edges[b * p.P + pp];
            float s = 0.f;
            if (n >= 3) {
                const float pad = c ? p.pad1 : p.pad0;
                const int nn = n < p.L ? n : p.L;
                for (int l = 0; l < nn; ++l) s += p.ol[b * p.ol_sb + pp * p.ol_sp + l * p.ol_sl + c] - pad;
            }
            loop_sums[((size_t)b * p.P + pp) * 2 + c] = s;
            s_loop += (double)s * s;
        }
    }
    if (p.flags & 4) {
        for (int e = tid; e < p.P * p.R; e += LOSS_TPB) {
            const int pp = e / p.R, c = e - pp * p.R;
            const float d = p.rot[((long)b * p.P + pp) * p.rot_s + c] - p.gt_rot[(size_t)b * p.P * p.R + e];
            s_rot += (double)d * d;
        }
    }
    if (p.flags & 8) {
        for (int e = tid; e < p.P * p.T; e += LOSS_TPB) {
            const int pp = e / p.T, c = e - pp * p.T;
            const float d = p.tr[((long)b * p.P + pp) * p.tr_s + c] - p.gt_tr[(size_t)b * p.P * p.T + e];
            s_tr += (double)d * d;
        }
    }
    red[0][tid] = s_shape; red[1][tid] = s_loop; red[2][tid] = s_rot; red[3][tid] = s_tr;
    __syncthreads();
    for (int st = LOSS_TPB / 2; st > 0; st >>= 1) {
        if (tid < st)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + st];
        __syncthreads();
    }
    if (tid < 4) part[(size_t)b * 4 + tid] = red[tid][0];
}

// out[0] = total, out[1..4] = shape, loop, rotation, translation (each already divided by its element count)
__global__ void gpe_loss_final_kernel(const double* __restrict__ part, LossParams p, float* __restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s[4] = {0, 0, 0, 0};
    for (int b = 0; b < p.B; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += part[(size_t)b * 4 + q];
    const double nb = (double)p.B * p.P;
    const double shape = s[0] / (nb * p.L * 4), loop = s[1] / (nb * 2), rot = s[2] / (nb * p.R), tr = s[3] / (nb * p.T);
    double total = 0;
    if (p.flags & 1) total += shape;
    if (p.flags & 2) total += (double)p.loop_w * loop;
    if (p.flags & 4) total += rot;
    if (p.flags & 8) total += tr;
    out[0] = (float)total;
    out[1] = (p.flags & 1) ? (float)shape : 0.f;
    out[2] = (p.flags & 2) ? (float)loop : 0.f;
    out[3] = (p.flags & 4) ? (float)rot : 0.f;
    out[4] = (p.flags & 8) ? (float)tr : 0.f;
}

// gradients of the TOTAL loss w.r.t. the three prediction views, scaled by the upstream gradient *gscale (device scalar):
//   g_ol [B,P,L,4] dense, g_rot [B,P,R], g_tr [B,P,T]
__global__ __launch_bounds__(LOSS_TPB) void gpe_loss_bwd_kernel(LossParams p, const float* __restrict__ loop_sums,
                                                                const float* __restrict__ gscale,
                                                                float* __restrict__ g_ol, float* __restrict__ g_rot,
                                                                float* __restrict__ g_tr)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const float gs = gscale ? gscale[0] : 1.f;
    const double nb = (double)p.B * p.P;
    const float k_shape = (p.flags & 1) ? (float)(2.0 / (nb * p.L * 4)) * gs : 0.f;
    const float k_loop = (p.flags & 2) ? (float)(2.0 * p.loop_w / (nb * 2)) * gs : 0.f;
    const float k_rot = (float)(2.0 / (nb * p.R)) * gs, k_tr = (float)(2.0 / (nb * p.T)) * gs;
    {
        const int n = p.P * p.L * 4;
        for (int e = tid; e < n; e += LOSS_TPB) {
            const int c = e & 3, l = (e >> 2) % p.L, pp = (e >> 2) / p.L;
            float g = 0.f;
            if (p.flags & 1)
                g = k_shape * (p.ol[b * p.ol_sb + pp * p.ol_sp + l * p.ol_sl + c] - p.gt_ol[(size_t)b * n + e]);
            if ((p.flags & 2) && c < 2) {
                const int ne = p.num_edges[b * p.P + pp];
                if (ne >= 3 && l < ne) g += k_loop * loop_sums[((size_t)b * p.P + pp) * 2 + c];
            }
            g_ol[(size_t)b * n + e] = g;
        }
    }
    if (g_rot)
        for (int e = tid; e < p.P * p.R; e += LOSS_TPB) {
            const int pp = e / p.R, c = e - pp * p.R;
            g_rot[(size_t)b * p.P * p.R + e] = (p.flags & 4)
                ? k_rot * (p.rot[((long)b * p.P + pp) * p.rot_s + c] - p.gt_rot[(size_t)b * p.P * p.R + e]) : 0.f;
        }
    if (g_tr)
        for (int e = tid; e < p.P * p.T; e += LOSS_TPB) {
            const int pp = e / p.T, c = e - pp * p.T;
            g_tr[(size_t)b * p.P * p.T + e] = (p.flags & 8)
                ? k_tr * (p.tr[((long)b * p.P + pp) * p.tr_s + c] - p.gt_tr[(size_t)b * p.P * p.T + e]) : 0.f;
        }
}

static int loss_params(LossParams& p, const float* ol, long ol_sb, long ol_sp, long ol_sl, const float* rot, long rot_s,
                       const float* tr, long tr_s, const float* gt_ol, const float* gt_rot, const float* gt_tr,
                       const int32_t* num_edges, int B, int P, int L, int R, int T, int flags, float pad0, float pad1,
                       float loop_w)
{
    if (B <= 0 || P <= 0 || L <= 0 || (flags & ~15)) return GPE_EINVAL;
    if ((flags & 3) && (!ol || !gt_ol)) return GPE_EINVAL;
    if ((flags & 2) && !num_edges) return GPE_EINVAL;
    if ((flags & 4) && (!rot || !gt_rot || R <= 0)) return GPE_EINVAL;
    if ((flags & 8) && (!tr || !gt_tr || T <= 0)) return GPE_EINVAL;
    p.ol = ol; p.ol_sb = ol_sb; p.ol_sp = ol_sp; p.ol_sl = ol_sl;
    p.rot = rot; p.rot_s = rot_s; p.tr = tr; p.tr_s = tr_s;
    p.gt_ol = gt_ol; p.gt_rot = gt_rot; p.gt_tr = gt_tr; p.num_edges = num_edges;
    p.B = B; p.P = P; p.L = L; p.R = R > 0 ? R : 1; p.T = T > 0 ? T : 1; p.flags = flags;
    p.pad0 = pad0; p.pad1 = pad1; p.loop_w = loop_w;
    return GPE_OK;
}

extern "C" int gpe_pattern_loss_fwd(const float* ol, long ol_sb, long ol_sp, long ol_sl, const float* rot, long rot_s,
                                    const float* tr, long tr_s, const float* gt_ol, const float* gt_rot,
                                    const float* gt_tr, const int32_t* num_edges, int B, int P, int L, int R, int T,
                                    int flags, float pad0, float pad1, float loop_w, double* part, float* loop_sums,
                                    float* out5, void* stream)
{
    LossParams p;
    const int rc = loss_params(p, ol, ol_sb, ol_sp, ol_sl, rot, rot_s, tr, tr_s, gt_ol, gt_rot, gt_tr, num_edges, B, P, L,
                               R, T, flags, pad0, pad1, loop_w);
    if (rc != GPE_OK || !part || !loop_sums || !out5) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_loss_fwd_kernel, dim3(B), dim3(LOSS_TPB), 0, (hipStream_t)stream, p, part, loop_sums);
    hipLaunchKernelGGL(gpe_loss_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, part, p, out5);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_pattern_loss_bwd(const float* ol, long ol_sb, long ol_sp, long ol_sl, const float* rot, long rot_s,
                                    const float* tr, long tr_s, const float* gt_ol, const float* gt_rot,
                                    const float* gt_tr, const int32_t* num_edges, int B, int P, int L, int R, int T,
                                    int flags, float pad0, float pad1, float loop_w, const float* loop_sums,
                                    const float* gscale, float* g_ol, float* g_rot, float* g_tr, void* stream)
{
    LossParams p;
    const int rc = loss_params(p, ol, ol_sb, ol_sp, ol_sl, rot, rot_s, tr, tr_s, gt_ol, gt_rot, gt_tr, num_edges, B, P, L,
                               R, T, flags, pad0, pad1, loop_w);
    if (rc != GPE_OK || !loop_sums || !g_ol) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_loss_bwd_kernel, dim3(B), dim3(LOSS_TPB), 0, (hipStream_t)stream, p, loop_sums, gscale, g_ol,
                       g_rot, g_tr);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// panel-origin matching (composed_loss.py:656-703): for every panel try each of its n cyclic edge shifts of the GT loop
// and keep the FIRST one with the smallest squared distance to the prediction.  One wave per panel: lane r evaluates
// shift r (r < n <= 64).  gt_out [B*P][L][D] = the chosen rotation; lead [B*P] = the chosen leading edge.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpe_origin_match_kernel(const float* __restrict__ ol, long ol_sb, long ol_sp,
                                                               long ol_sl, const float* __restrict__ gt, int D,
                                                               const int32_t* __restrict__ num_edges, int panels, int P,
                                                               int L, float* __restrict__ gt_out,
                                                               int32_t* __restrict__ lead)
{
    const int lane = threadIdx.x & 63;
    const int el = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (el >= panels) return;
    const int b = el / P, pp = el - b * P;
    const float* pr = ol + b * ol_sb + pp * ol_sp;
    const float* g = gt + (size_t)el * L * D;
    int n = num_edges[el];
    if (n > L) n = L;
    if (n < 0) n = 0;
    // shift r: gt_r[l] = gt[(l + r) mod n] for l < n, gt[l] beyond (padding stays in place)
    float dist = INFINITY;
    if (lane < (n > 1 ? n : 1)) {
        float s = 0.f;
        for (int l = 0; l < L; ++l) {
            int src = l;
            if (l < n) { src = l + lane; if (src >= n) src -= n; }
            for (int c = 0; c < D; ++c) {
                const float d = pr[l * ol_sl + c] - g[src * D + c];
                s = __builtin_fmaf(d, d, s);
            }
        }
        dist = s;
    }
    // first minimum over lanes: (dist, lane) lexicographic
    float best = dist;
    int bl = lane;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float od = __shfl_xor(best, off);
        const int ol_ = __shfl_xor(bl, off);
        if (od < best || (od == best && ol_ < bl)) { best = od; bl = ol_; }
    }
    const int r = bl;
    if (lane == 0) lead[el] = r;
    for (int e = lane; e < L * D; e += 64) {
        const int l = e / D, c = e - l * D;
        int src = l;
        if (l < n) { src = l + r; if (src >= n) src -= n; }
        gt_out[(size_t)el * L * D + e] = g[src * D + c];
    }
}

extern "C" int gpe_origin_match(const float* ol, long ol_sb, long ol_sp, long ol_sl, const float* gt_ol, int D,
                                const int32_t* num_edges, int B, int P, int L, float* gt_out, int32_t* lead,
                                void* stream)
{
    if (!ol || !gt_ol || !num_edges || !gt_out || !lead || B <= 0 || P <= 0 || L <= 0 || L > 64 || D <= 0)
        return GPE_EINVAL;
    const int panels = B * P;
    hipLaunchKernelGGL(gpe_origin_match_kernel, dim3(gpe_cdiv(panels, 4)), dim3(256), 0, (hipStream_t)stream, ol, ol_sb,
                       ol_sp, ol_sl, gt_ol, D, num_edges, panels, P, L, gt_out, lead);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// greedy panel-order matching (composed_loss.py:530-570): distance matrix dist[i][j] = |pred_i - gt_j|_2 (P x P), then P
// rounds of "take the global minimum (first in row-major order on ties), fix perm[row] = col, strike row and column".
// One workgroup per pattern; P <= 64.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpe_order_match_kernel(const float* __restrict__ pf, const float* __restrict__ gf,
                                                              int P, int D, int64_t* __restrict__ perm,
                                                              int32_t* __restrict__ fail)
{
    extern __shared__ float dm[];            // [P*P] + reduction scratch
    __shared__ float rv[256];
    __shared__ int ri[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* pb = pf + (size_t)b * P * D;
    const float* gb = gf + (size_t)b * P * D;
    for (int e = tid; e < P * P; e += 256) {
        const int i = e / P, j = e - i * P;
        float s = 0.f;
        for (int c = 0; c < D; ++c) {
            const float d = pb[i * D + c] - gb[j * D + c];
            s = __builtin_fmaf(d, d, s);
        }
        dm[e] = sqrtf(s);
    }
    if (tid < P) perm[(size_t)b * P + tid] = -1;
    __syncthreads();
    for (int round = 0; round < P; ++round) {
        float best = INFINITY;
        int bi = 0x7fffffff;
        for (int e = tid; e < P * P; e += 256) {
            const float v = dm[e];
            if (v < best || (v == best && e < bi)) { best = v; bi = e; }
        }
        rv[tid] = best; ri[tid] = bi;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (tid < st) {
                const float ov = rv[tid + st];
                const int oi = ri[tid + st];
                if (ov < rv[tid] || (ov == rv[tid] && oi < ri[tid])) { rv[tid] = ov; ri[tid] = oi; }
            }
            __syncthreads();
        }
        int sel = ri[0];
        if (sel == 0x7fffffff) sel = 0;      // everything +inf already (NaN inputs): torch's argmin returns 0 as well
        const int row = sel / P, col = sel - row * P;
        __syncthreads();
        if (tid == 0) perm[(size_t)b * P + row] = col;
        for (int e = tid; e < P; e += 256) { dm[row * P + e] = INFINITY; dm[e * P + col] = INFINITY; }
        __syncthreads();
    }
    // the reference raises if a finite entry is left (composed_loss.py:567-568)
    int bad = 0;
    for (int e = tid; e < P * P; e += 256) bad |= isfinite(dm[e]) ? 1 : 0;
    if (bad) fail[0] = 1;
    // Degenerate input (NaN / inf predictions: every distance +inf, the rounds above keep hitting entry 0): rows would stay
    // at -1 and the gathers that consume `perm` would index out of bounds (a device-side assert that poisons the context,
    // where the reference raises a clean ValueError).  Keep the output in bounds — unmatched rows take the unused columns
    // in ascending order — and report the failure through `fail` (thread 0 wrote every perm entry itself).
    if (tid == 0) {
        unsigned long long used = 0ull;
        bool open_rows = false;
        for (int r = 0; r < P; ++r) {
            const int64_t c = perm[(size_t)b * P + r];
            if (c >= 0) used |= 1ull << c; else open_rows = true;
        }
        if (open_rows) {
            fail[0] = 1;
            int c = 0;
            for (int r = 0; r < P; ++r) {
                if (perm[(size_t)b * P + r] >= 0) continue;
                while (c < P - 1 && ((used >> c) & 1ull)) ++c;
                perm[(size_t)b * P + r] = c;
                used |= 1ull << c;
            }
        }
    }
}

extern "C" int gpe_order_match(const float* pred_feat, const float* gt_feat, int B, int P, int D, int64_t* perm,
                               int32_t* fail, void* stream)
{
    if (!pred_feat || !gt_feat || !perm || !fail || B <= 0 || P <= 0 || P > 64 || D <= 0) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_order_match_kernel, dim3(B), dim3(256), (size_t)P * P * sizeof(float), (hipStream_t)stream,
                       pred_feat, gt_feat, P, D, perm, fail);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// ---------------------------------------------------------------------------------------------------------
// entmax.SparsemaxLoss() as the reference calls it (nn/metrics/composed_loss.py:4,196,323-332; entmax is third-party and
// un-vendored: the published Fenchel-Young sparsemax loss, Martins & Astudillo 2016 / Blondel et al. 2019, restated):
//   p = sparsemax(x);  L_r = (1 - |p|^2)/2 + <p - e_t, x>;  loss = mean_r L_r (reduction 'elementwise_mean', nothing ignored);
//   dL_r/dx = p - e_t.   One row per lane (same in-register sort as the forward, gpe_pool.hip); gx receives (p - e_t)/rows,
// part[blockIdx] the block's fp64 sum of L_r; gpe_sparsemax_loss_finish adds the partials in index order.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpe_sparsemax_loss_kernel(const float* __restrict__ x, int ldx,
                                                                 const int32_t* __restrict__ target, long rows, int W,
                                                                 float* __restrict__ gx, int ldg, double* __restrict__ part,
                                                                 int* __restrict__ bad)
{
    __shared__ double red[256];
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    double L = 0.0;
    if (r < rows) {
        float v[SPX_W];
#pragma unroll
        for (int i = 0; i < SPX_W; ++i) v[i] = (i < W) ? x[r * ldx + i] : -INFINITY;
#pragma unroll
        for (int pass = 0; pass < SPX_W; ++pass) {
#pragma unroll
            for (int i = (pass & 1); i + 1 < SPX_W; i += 2) {
                const float a = v[i], b = v[i + 1];
                v[i] = fmaxf(a, b); v[i + 1] = fminf(a, b);
            }
        }
        const float mx = v[0];                                   // max-shifted scores, as in the forward (gpe_pool.hip)
        float cs = 0.f, tau = 0.f;
#pragma unroll
        for (int i = 0; i < SPX_W; ++i) {
            if (i < W) {
                const float vi = v[i] - mx;
                cs += vi;
                if (1.f + (float)(i + 1) * vi > cs) tau = (cs - 1.f) / (float)(i + 1);
            }
        }
        int t = target[r];
        if (t < 0 || t >= W) { atomicOr(bad, 1); t = 0; }
        const float inv = 1.f / (float)rows;
        float pp = 0.f, dot = 0.f;
        for (int i = 0; i < W; ++i) {
            const float xi = x[r * ldx + i] - mx;                // <p - e_t, x> == <p - e_t, x - max>: sum(p - e_t) = 0
            const float p = fmaxf(xi - tau, 0.f);
            const float d = p - (i == t ? 1.f : 0.f);
            pp += p * p;
            dot += d * xi;
            gx[r * ldg + i] = d * inv;
        }
        L = (double)((1.f - pp) * 0.5f + dot);
    }
    red[threadIdx.x] = L;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(64) void gpe_sparsemax_loss_finish_kernel(const double* __restrict__ part, int nblk, long rows,
                                                                       float* __restrict__ loss)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < nblk; ++i) s += part[i];
    loss[0] = (float)(s / (double)rows);
}

// part: >= ceil(rows/256) doubles; bad: one int, set to 1 when a target is outside [0, W) (the caller raises)
extern "C" int gpe_sparsemax_loss(const float* x, int ldx, const int32_t* target, long rows, int W, float* gx, int ldg,
                                  double* part, float* loss, int* bad, void* stream)
{
    if (!x || !target || !gx || !part || !loss || !bad || rows <= 0 || W <= 0 || W > SPX_W || ldx < W || ldg < W) return GPE_EINVAL;
    const int nblk = (int)gpe_cdiv(rows, 256);
    hipLaunchKernelGGL(gpe_sparsemax_loss_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, x, ldx, target, rows, W, gx,
                       ldg, part, bad);
    GPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(gpe_sparsemax_loss_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, part, nblk, rows, loss);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
