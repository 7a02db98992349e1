// The quality metrics of ComposedPatternLoss (nn/metrics/composed_loss.py:268-277,365-424) as gfx950 kernels:
//   * discrete     NumbersInPanelsAccuracies                                   nn/metrics/metrics.py:95-182
//   * shape        PanelVertsL2 (vertex outline incl. curvature points)        nn/metrics/metrics.py:185-281
//   * rotation / translation   UniversalL2                                     nn/metrics/metrics.py:284-325
//   * stitch       PatternStitchPrecisionRecall + tags_to_stitches (greedy)    nn/metrics/metrics.py:13-79, nn/data/datasets.py:917-968
//   * free_class   free-edge accuracy                                          nn/metrics/composed_loss.py:419-424
// The reference walks every panel / edge / stitch in Python.  Here: one workgroup per pattern writes per-pattern partials to a
// caller-owned fp64 workspace (panel kernel, stitch kernel), and a single-thread finalise kernel combines them IN PATTERN ORDER,
// with the reference's own number types per slot (fp32 sums where the reference sums fp32 tensors, fp64 where it sums Python
// floats), so the result vector is bit-reproducible run to run.  At most three launches per call, no host reads.
#include "gpe_stitch_greedy.h"   // QM_TPB (one wave per pattern, both kernels), QM_MAXD, QM_MAXE and the pairing itself
#include <math.h>

// (every product / sum below is rounded on its own, in the reference's order: the header switches FMA contraction off)
#include "gpe_quality_fold.h"    // QM_* flags, QM_PART, and the fold of the per-pattern records (shared with csrc/gpe_eval.hip)

#define QM_MAXP 64           // panels per pattern (shipped: 23)
#define QM_MAXL 64           // edges per panel (shipped: 14)

// host-array layout of `stats` (include/gpe_hip.h gpe_quality_panels / gpe_quality_stitches)
enum { QS_OL_SHIFT = 0, QS_OL_SCALE = 4, QS_PAD = 8, QS_PAD_TOL = 12, QS_LOOP_THR = 16, QS_ROT_SHIFT = 24, QS_ROT_SCALE = 32,
       QS_TR_SHIFT = 40, QS_TR_SCALE = 48, QS_TAG_SHIFT = 56, QS_TAG_SCALE = 64, QS_N = 72 };

struct QmStats { float v[QS_N]; };

// (the slots of a pattern's workspace record: gpe_quality_fold.h)
struct QmPanelParams {
    const float* ol; long ol_sb, ol_sp, ol_sl;          // predicted outlines (b,p,l,c<4) at ol + b*ol_sb + p*ol_sp + l*ol_sl + c
    const float* gt_ol;                                 // dense [B,P,L,4]
    const int32_t* num_edges;                           // [B*P] ground truth (after order matching)
    const int32_t* num_panels;                          // [B]
    const float* rot; long rot_s; const float* gt_rot; int R;    // predicted row (b,p) at rot + (b*P + p)*rot_s; gt dense [B,P,R]
    const float* tr; long tr_s; const float* gt_tr; int T;
    int B, P, L, flags;
};

// ---------------------------------------------------------------------------------------------------------------------
// panel metrics: one lane per panel, sequential over its edges
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void qm_unstd(const float* e, const QmStats& s, float* u)
{
    for (int c = 0; c < 4; ++c) u[c] = e[c] * s.v[QS_OL_SCALE + c] + s.v[QS_OL_SHIFT + c];
}

// mean distance of matching vertices of the centred vertex outlines of a predicted and a ground-truth panel (first n edges).
// The outline of n un-standardised edges: the origin, then per edge its curvature point prev + c0*e + c1*perp(e) and the next
// vertex prev + e (metrics.py:262-281); the walk is done twice (means, then distances) instead of storing 2n + 1 vertices.
__device__ __forceinline__ void qm_panel_l2(const float* pred, long p_sl, const float* gt, int n, const QmStats& s,
                                            double* out)
{
    // pass 1: vertex means of both outlines
    float mg[2] = {0.f, 0.f}, mp[2] = {0.f, 0.f};
    float gv[2] = {0.f, 0.f}, pv[2] = {0.f, 0.f};
    for (int k = 0; k < n; ++k) {
        float eg[4], ep[4];
        qm_unstd(gt + (size_t)k * 4, s, eg);
        qm_unstd(pred + k * p_sl, s, ep);
        const float cg0 = (gv[0] + eg[2] * eg[0]) + eg[3] * -eg[1], cg1 = (gv[1] + eg[2] * eg[1]) + eg[3] * eg[0];
        const float cp0 = (pv[0] + ep[2] * ep[0]) + ep[3] * -ep[1], cp1 = (pv[1] + ep[2] * ep[1]) + ep[3] * ep[0];
        gv[0] = gv[0] + eg[0]; gv[1] = gv[1] + eg[1];
        pv[0] = pv[0] + ep[0]; pv[1] = pv[1] + ep[1];
        mg[0] += cg0; mg[0] += gv[0]; mg[1] += cg1; mg[1] += gv[1];
        mp[0] += cp0; mp[0] += pv[0]; mp[1] += cp1; mp[1] += pv[1];
    }
    const float nv = (float)(2 * n + 1);
    mg[0] /= nv; mg[1] /= nv; mp[0] /= nv; mp[1] /= nv;
    // pass 2: mean distance of matching centred vertices (the origin first)
    auto vd = [&](float g0, float g1, float p0, float p1) {
        const float d0 = (g0 - mg[0]) - (p0 - mp[0]), d1 = (g1 - mg[1]) - (p1 - mp[1]);
        return sqrtf(d0 * d0 + d1 * d1);
    };
    float acc = vd(0.f, 0.f, 0.f, 0.f);
    gv[0] = gv[1] = pv[0] = pv[1] = 0.f;
    for (int k = 0; k < n; ++k) {
        float eg[4], ep[4];
        qm_unstd(gt + (size_t)k * 4, s, eg);
        qm_unstd(pred + k * p_sl, s, ep);
        const float cg0 = (gv[0] + eg[2] * eg[0]) + eg[3] * -eg[1], cg1 = (gv[1] + eg[2] * eg[1]) + eg[3] * eg[0];
        const float cp0 = (pv[0] + ep[2] * ep[0]) + ep[3] * -ep[1], cp1 = (pv[1] + ep[2] * ep[1]) + ep[3] * ep[0];
        gv[0] = gv[0] + eg[0]; gv[1] = gv[1] + eg[1];
        pv[0] = pv[0] + ep[0]; pv[1] = pv[1] + ep[1];
        acc += vd(cg0, cg1, cp0, cp1);
        acc += vd(gv[0], gv[1], pv[0], pv[1]);
    }
    *out = (double)(acc / nv);
}

__device__ __forceinline__ double qm_row_l2(const float* p, const float* g, int C, const float* shift, const float* scale)
{
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
        const float d = (g[c] * scale[c] + shift[c]) - (p[c] * scale[c] + shift[c]);
        s += d * d;
    }
    return (double)sqrtf(s);
}

__global__ __launch_bounds__(QM_TPB) void gpe_quality_panel_kernel(QmPanelParams q, QmStats s, double* __restrict__ part)
{
    __shared__ int cnt_sh[QM_MAXP];         // predicted edge count of the panel (< 3: empty)
    __shared__ double l2_sh[3][QM_MAXP];    // shape / rotation / translation per panel
    __shared__ int shape_sh[QM_MAXP];       // panel enters the shape mean
    const int b = blockIdx.x, p = threadIdx.x;
    if (p < q.P) {
        const float* pan = q.ol + b * q.ol_sb + p * q.ol_sp;
        const size_t gp = (size_t)b * q.P + p;
        if (q.flags & QM_DISCRETE) {
            // rows that are not padding (all 4 features isclose to the pad vector), + 1 if the loop stays open by > 3 cm
            int cnt = 0;
            float sx = 0.f, sy = 0.f;
            for (int l = 0; l < q.L; ++l) {
                const float* e = pan + l * q.ol_sl;
                bool pad = true;
                for (int c = 0; c < 4; ++c) pad = pad && (fabsf(e[c] - s.v[QS_PAD + c]) <= s.v[QS_PAD_TOL + c]);
                cnt += !pad;
                sx += e[0]; sy += e[1];
            }
            if (fabsf(sx) > s.v[QS_LOOP_THR] || fabsf(sy) > s.v[QS_LOOP_THR + 1]) ++cnt;
            cnt_sh[p] = cnt;
        }
        shape_sh[p] = 0;
        l2_sh[0][p] = 0.0;
        if (q.flags & QM_SHAPE) {
            int n = q.num_edges[gp];
            if (n >= 3) {
                n = n > q.L ? q.L : n;
                qm_panel_l2(pan, q.ol_sl, q.gt_ol + gp * q.L * 4, n, s, &l2_sh[0][p]);
                shape_sh[p] = 1;
            }
        }
        l2_sh[1][p] = (q.flags & QM_ROT) ? qm_row_l2(q.rot + gp * q.rot_s, q.gt_rot + gp * q.R, q.R, s.v + QS_ROT_SHIFT,
                                                     s.v + QS_ROT_SCALE) : 0.0;
        l2_sh[2][p] = (q.flags & QM_TR) ? qm_row_l2(q.tr + gp * q.tr_s, q.gt_tr + gp * q.T, q.T, s.v + QS_TR_SHIFT,
                                                    s.v + QS_TR_SCALE) : 0.0;
    }
    __syncthreads();
    if (p != 0) return;
    double* o = part + (size_t)b * QM_PART;
    // panel order, like the reference's loops
    int npan = 0, nok = 0, nsh = 0;
    double ssh = 0, srot = 0, str = 0;
    for (int k = 0; k < q.P; ++k) {
        if (q.flags & QM_DISCRETE) {
            const int c = cnt_sh[k];
            if (c >= 3) { ++npan; nok += c == q.num_edges[(size_t)b * q.P + k]; }
        }
        if (shape_sh[k]) { ssh += l2_sh[0][k]; ++nsh; }
        srot += l2_sh[1][k];
        str += l2_sh[2][k];
    }
    const int gtn = q.flags & QM_DISCRETE ? q.num_panels[b] : 0;
    o[0] = (q.flags & QM_DISCRETE) ? (double)(npan == gtn) : 0.0;
    o[1] = (q.flags & QM_DISCRETE) ? (double)((float)nok / (float)gtn) : 0.0;     // fp32, as the reference's tensor division
    o[2] = ssh;
    o[3] = nsh;
    o[4] = srot;
    o[5] = str;
}

// ---------------------------------------------------------------------------------------------------------------------
// stitch detection (greedy pairing of the non-free edges' tags) + precision / recall + free-edge accuracy: one wave per pattern
// ---------------------------------------------------------------------------------------------------------------------
struct QmStitchParams {
    QmEdgeViews v;                                      // predicted tags / free-edge logits (gpe_stitch_greedy.h)
    const int64_t* stitches; const int64_t* nums; int S; // ground truth [B][2][S] (after the matchings' re-numbering), [B]
    const float* gt_mask;                               // ground-truth free-edge mask [B,P,L] (1 = free)
    int B, P, L, flags;
};

__global__ __launch_bounds__(QM_TPB) void gpe_quality_stitch_kernel(QmStitchParams q, QmStats s, double* __restrict__ part)
{
    __shared__ QmGreedyLds g;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int PL = q.P * q.L;
    // pass 1: decisions, their count, the edge an odd count drops, free-edge accuracy
    int nfree_ok = 0, drop;
    int m = qm_count_nonfree(q.v, b, PL, q.L, lane, &drop, [&](int e, float sg) {
        if (q.flags & QM_FREE) {
            const float cls = sg != sg ? sg : (sg > 0.5f ? 1.f : 0.f);
            nfree_ok += cls == q.gt_mask[(size_t)b * PL + e];
        }
    });
    for (int o = 32; o > 0; o >>= 1) nfree_ok += __shfl_xor(nfree_ok, o);
    double* o = part + (size_t)b * QM_PART;
    if (!(q.flags & QM_STITCH) || m < 2) {                   // no stitches: the pattern adds 0 and joins no corr_ list
        if (lane == 0) { o[8] = 0.0; o[9] = 0.0; o[10] = 0.0; o[11] = (double)nfree_ok; }
        return;
    }
    // pass 2 and the greedy rounds (gpe_stitch_greedy.h)
    const bool ts = q.flags & QM_TAG_STATS;
    m = qm_stage_tags(q.v, b, PL, q.L, lane, drop, ts ? s.v + QS_TAG_SHIFT : nullptr, ts ? s.v + QS_TAG_SCALE : nullptr, g);
    const int npairs = qm_greedy_rounds(m, q.v.D, lane, g);
    const short* pa = g.pa;
    const short* pb = g.pb;
    // scoring: a detected pair is correct if it equals a ground-truth stitch in either order (each counted once)
    long n = q.nums[b];
    const int ncmp = (int)(n < 0 ? 0 : (n > q.S ? q.S : n));
    const int64_t* st = q.stitches + (size_t)b * 2 * q.S;
    int good = 0;
    for (int k = lane; k < npairs; k += QM_TPB) {
        const int64_t a = pa[k], c = pb[k];
        for (int i = 0; i < ncmp; ++i) {
            const int64_t u = st[i], v = st[q.S + i];
            if ((a == u && c == v) || (a == v && c == u)) { ++good; break; }
        }
    }
    for (int sh = 32; sh > 0; sh >>= 1) good += __shfl_xor(good, sh);
    if (lane == 0) {
        o[8] = npairs > 0 ? 1.0 : 0.0;
        o[9] = npairs > 0 ? (double)good / (double)npairs : 0.0;
        // the reference divides a Python float by a 0-d integer tensor, which torch evaluates as c * (1 / n) in fp32
        o[10] = n != 0 ? (double)((float)good * (1.0f / (float)n)) : 0.0;
        o[11] = (double)nfree_ok;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// finalise: one thread, pattern order
// ---------------------------------------------------------------------------------------------------------------------
__global__ void gpe_quality_final_kernel(const double* __restrict__ part, int B, int P, int L, int flags, float* __restrict__ out,
                                         int32_t* __restrict__ counts)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    QmFold f;
    for (int b = 0; b < B; ++b) f.add(part + (size_t)b * QM_PART, flags);
    f.finish(B, P, L, flags, out, counts);
}

static int qm_stats(const float* stats_host, QmStats* s)
{
    if (!stats_host) return GPE_EINVAL;
    for (int k = 0; k < QS_N; ++k) s->v[k] = stats_host[k];
    return GPE_OK;
}

extern "C" int gpe_quality_panels(const float* ol, long ol_sb, long ol_sp, long ol_sl, const float* gt_ol,
                                  const int32_t* num_edges, const int32_t* num_panels, const float* rot, long rot_s,
                                  const float* gt_rot, int R, const float* tr, long tr_s, const float* gt_tr, int T, int B,
                                  int P, int L, int flags, const float* stats_host, double* part, void* stream)
{
    if (B <= 0 || P <= 0 || P > QM_MAXP || L <= 0 || L > QM_MAXL || !part || (flags & ~127)) return GPE_EINVAL;
    if ((flags & (QM_DISCRETE | QM_SHAPE)) && (!ol || !num_edges)) return GPE_EINVAL;
    if ((flags & QM_DISCRETE) && !num_panels) return GPE_EINVAL;
    if ((flags & QM_SHAPE) && !gt_ol) return GPE_EINVAL;
    if ((flags & QM_ROT) && (!rot || !gt_rot || R <= 0 || R > QM_MAXD)) return GPE_EINVAL;
    if ((flags & QM_TR) && (!tr || !gt_tr || T <= 0 || T > QM_MAXD)) return GPE_EINVAL;
    QmStats s;
    if (qm_stats(stats_host, &s) != GPE_OK) return GPE_EINVAL;
    QmPanelParams q{ol, ol_sb, ol_sp, ol_sl, gt_ol, num_edges, num_panels, rot, rot_s, gt_rot, R, tr, tr_s, gt_tr, T, B, P, L,
                    flags};
    hipLaunchKernelGGL(gpe_quality_panel_kernel, dim3(B), dim3(QM_TPB), 0, (hipStream_t)stream, q, s, part);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_quality_stitches(const float* tags, long t_sb, long t_sp, long t_sl, int D, const float* logit, long m_sb,
                                    long m_sp, long m_sl, const int64_t* stitches, const int64_t* nums, int S,
                                    const float* gt_mask, int B, int P, int L, int flags, const float* stats_host,
                                    double* part, void* stream)
{
    if (B <= 0 || P <= 0 || L <= 0 || P * L > QM_MAXE || !part || !logit || (flags & ~127)) return GPE_EINVAL;
    if ((flags & QM_STITCH) && (!tags || !stitches || !nums || S <= 0 || D <= 0 || D > QM_MAXD)) return GPE_EINVAL;
    if ((flags & QM_FREE) && !gt_mask) return GPE_EINVAL;
    QmStats s;
    if (qm_stats(stats_host, &s) != GPE_OK) return GPE_EINVAL;
    QmStitchParams q{{tags, t_sb, t_sp, t_sl, D, logit, m_sb, m_sp, m_sl}, stitches, nums, S, gt_mask, B, P, L, flags};
    hipLaunchKernelGGL(gpe_quality_stitch_kernel, dim3(B), dim3(QM_TPB), 0, (hipStream_t)stream, q, s, part);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_quality_finalize(const double* part, int B, int P, int L, int flags, float* out, int32_t* counts,
                                    void* stream)
{
    if (!part || !out || !counts || B <= 0 || P <= 0 || L <= 0 || (flags & ~127)) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_quality_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, part, B, P, L, flags, out,
                       counts);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
