// A prediction decoded to a sewing pattern (Garment3DPatternFullDataset._pred_to_pattern, nn/data/datasets.py:731-767, with
// tags_to_stitches :917-968 and NNSewingPattern.pattern_from_tensors / panel_from_numeric / _edge_dict,
// nn/data/pattern_converter.py:118-187, 228-271, 510-515) as one gfx950 kernel: one workgroup of one wave per garment.
// The reference walks every panel, edge and stitch of every garment in Python after a .cpu() per tensor.  Here, per garment:
//   1. every panel on its own lane: un-standardise in fp64 (a product and a sum, each rounded: numpy on float64), drop the padding
//      rows, walk the kept rows to vertices in the reference's order, decide closure and curvature;
//   2. number the non-empty panels (ballot prefix);
//   3. the stitches: tags_to_stitches of gpe_stitch_greedy.h (shared with the quality metrics), or the caller's list;
//   4. every stitch checked against the panels it names.
// No atomics, nothing between workgroups, every output element written by exactly one thread: bit-reproducible.
#include "gpe_stitch_greedy.h"
#include <math.h>

// every product / sum below is rounded on its own (numpy's `pred * scale + shift` is two operations)
#pragma clang fp contract(off)

// host-array layout of `stats` (include/gpe_hip.h gpe_pattern_decode): shift then scale of each group, QM_MAXD wide
enum { PD_OL_SHIFT = 0, PD_OL_SCALE = 8, PD_ROT_SHIFT = 16, PD_ROT_SCALE = 24, PD_TR_SHIFT = 32, PD_TR_SCALE = 40, PD_TAG_SHIFT = 48,
       PD_TAG_SCALE = 56, PD_N = 64 };
enum { PD_TAG_STATS = 1 };

struct PdStats { double v[PD_N]; };

struct PdParams {
    const float* ol; long ol_sb, ol_sp, ol_sl;          // predicted outlines (b,p,l,c<4) at ol + b*ol_sb + p*ol_sp + l*ol_sl + c
    const float* rot; long rot_s; int R;                // predicted row (b,p) at rot + (b*P + p)*rot_s
    const float* tr; long tr_s; int T;
    QmEdgeViews v;                                      // tags / free-edge logits
    const int32_t* given; const int32_t* given_num;     // caller's stitches [B][2][S] (NULL: pair the tags), their count [B] (NULL: S)
    int B, P, L, S, flags;
    int32_t *num_edges, *edge_slot, *num_verts, *closed, *new_panel_id, *num_panels, *curved;
    double *vertices, *curvature, *rotations, *translations;
    int32_t *stitches, *num_stitches, *stitch_flags, *first_invalid;
};

__device__ __forceinline__ double pd_unstd(float x, double scale, double shift) { return (double)x * scale + shift; }
// np.isclose(x, 0, atol = a): |x| <= a; false for NaN and inf
__device__ __forceinline__ bool pd_close(double x, double a) { return fabs(x) <= a; }

__global__ __launch_bounds__(QM_TPB) void gpe_pattern_decode_kernel(PdParams q, PdStats s)
{
    __shared__ QmGreedyLds g;
    __shared__ unsigned char kept[QM_MAXE];             // the slot's row is an edge of its panel
    __shared__ short pid[QM_MAXE];                      // new_panel_id (P <= P * L <= QM_MAXE)
    __shared__ float tag_stats[2 * QM_MAXD];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int P = q.P, L = q.L, PL = P * L, S = q.S;
    const unsigned long long below = (1ull << lane) - 1ull;
    if (lane < QM_MAXD) {
        tag_stats[lane] = (float)s.v[PD_TAG_SHIFT + lane];
        tag_stats[QM_MAXD + lane] = (float)s.v[PD_TAG_SCALE + lane];
    }
    // ---- 1. panels: one lane each ---------------------------------------------------------------------------------------
    for (int p = lane; p < P; p += QM_TPB) {
        const size_t gp = (size_t)b * P + p;
        const float* pan = q.ol + b * q.ol_sb + p * q.ol_sp;
        int32_t* slot = q.edge_slot + gp * L;
        int32_t* crv = q.curved + gp * L;
        double* vert = q.vertices + gp * (L + 1) * 2;
        double* cur = q.curvature + gp * L * 2;
        for (int c = 0; c < q.R; ++c)
            q.rotations[gp * q.R + c] = pd_unstd(q.rot[gp * q.rot_s + c], s.v[PD_ROT_SCALE + c], s.v[PD_ROT_SHIFT + c]);
        for (int c = 0; c < q.T; ++c)
            q.translations[gp * q.T + c] = pd_unstd(q.tr[gp * q.tr_s + c], s.v[PD_TR_SCALE + c], s.v[PD_TR_SHIFT + c]);
        // kept rows: not all four values within 1.5 of 0
        int n = 0;
        for (int l = 0; l < L; ++l) {
            const float* e = pan + l * q.ol_sl;
            bool pad = true;
            for (int c = 0; c < 4; ++c) pad = pad && pd_close(pd_unstd(e[c], s.v[PD_OL_SCALE + c], s.v[PD_OL_SHIFT + c]), 1.5);
            kept[p * L + l] = !pad;
            n += !pad;
        }
        const bool real = n >= 3;
        // the walk: vertex 0 at the origin, vertex k + 1 = vertex k + edge k (sequential fp64 sums, the reference's order)
        double vx = 0.0, vy = 0.0;
        int k = 0;
        vert[0] = 0.0; vert[1] = 0.0;
        if (real) {
            for (int l = 0; l < L; ++l) {
                if (!kept[p * L + l]) continue;
                const float* e = pan + l * q.ol_sl;
                double u[4];
                for (int c = 0; c < 4; ++c) u[c] = pd_unstd(e[c], s.v[PD_OL_SCALE + c], s.v[PD_OL_SHIFT + c]);
                vx = vx + u[0]; vy = vy + u[1];
                slot[k] = l;
                cur[2 * k] = u[2]; cur[2 * k + 1] = u[3];
                crv[k] = !(pd_close(u[2], 0.01) && pd_close(u[3], 0.01));
                ++k;
                if (k < n) { vert[2 * k] = vx; vert[2 * k + 1] = vy; }
            }
        }
        // the last edge returns to vertex 0 if its end is within 3 of the origin in both coordinates; else one more vertex
        const bool cl = real && pd_close(vx, 3.0) && pd_close(vy, 3.0);
        int nv = real ? n : 0;
        if (real && !cl) { vert[2 * n] = vx; vert[2 * n + 1] = vy; nv = n + 1; }
        for (int j = (nv > 0 ? nv : 1); j <= L; ++j) { vert[2 * j] = 0.0; vert[2 * j + 1] = 0.0; }
        for (int j = k; j < L; ++j) { slot[j] = -1; crv[j] = 0; cur[2 * j] = 0.0; cur[2 * j + 1] = 0.0; }
        q.num_edges[gp] = real ? n : 0;
        q.num_verts[gp] = nv;
        q.closed[gp] = cl;
        pid[p] = real ? 0 : -1;
    }
    __syncthreads();
    // ---- 2. new ids of the non-empty panels, in panel order ----------------------------------------------------------------
    int npan = 0;
    for (int p0 = 0; p0 < P; p0 += QM_TPB) {
        const int p = p0 + lane;
        const bool real = p < P && pid[p] == 0;
        const unsigned long long bal = __ballot(real);
        if (p < P) {
            const int id = real ? npan + __builtin_popcountll(bal & below) : -1;
            pid[p] = (short)id;
            q.new_panel_id[(size_t)b * P + p] = id;
        }
        npan += __builtin_popcountll(bal);
    }
    if (lane == 0) q.num_panels[b] = npan;
    __syncthreads();
    // ---- 3. stitches: found from the tags, or the caller's --------------------------------------------------------------------
    int32_t* st = q.stitches + (size_t)b * 2 * S;
    int32_t* sf = q.stitch_flags + (size_t)b * S;
    int ns = 0;
    if (q.given) {
        // entries (0, 0) are padding and are skipped; the others keep their order
        const int32_t* gs = q.given + (size_t)b * 2 * S;
        int cnt = q.given_num ? q.given_num[b] : S;
        cnt = cnt < 0 ? 0 : (cnt > S ? S : cnt);
        for (int k0 = 0; k0 < cnt; k0 += QM_TPB) {
            const int k = k0 + lane;
            int a = 0, c = 0;
            if (k < cnt) { a = gs[k]; c = gs[S + k]; }
            const bool use = k < cnt && !(a == 0 && c == 0);
            const unsigned long long bal = __ballot(use);
            if (use) { const int o = ns + __builtin_popcountll(bal & below); st[o] = a; st[S + o] = c; }
            ns += __builtin_popcountll(bal);
        }
    } else {
        int drop;
        int m = qm_count_nonfree(q.v, b, PL, L, lane, &drop, [](int, float) {});
        if (m >= 2) {
            const bool ts = q.flags & PD_TAG_STATS;
            m = qm_stage_tags(q.v, b, PL, L, lane, drop, ts ? tag_stats : nullptr, ts ? tag_stats + QM_MAXD : nullptr, g);
            ns = qm_greedy_rounds(m, q.v.D, lane, g);
            ns = ns > S ? S : ns;
            for (int k = lane; k < ns; k += QM_TPB) { st[k] = g.pa[k]; st[S + k] = g.pb[k]; }
        }
    }
    __syncthreads();
    // ---- 4. validity of every stitch ---------------------------------------------------------------------------------------------
    int first = 0x7fffffff;
    for (int k = lane; k < S; k += QM_TPB) {
        int f = 0;
        if (k < ns) {
            for (int side = 0; side < 2; ++side) {
                const int id = st[side * S + k];
                const int pp = id < 0 ? -1 : id / L;                   // a negative id names no panel
                if (pp < 0 || pp >= P || pid[pp] < 0) f |= 1;
                if (id >= 0 && id < PL && !kept[id]) f |= 2;
            }
            if ((f & 1) && k < first) first = k;
        } else {
            st[k] = 0; st[S + k] = 0;
        }
        sf[k] = f;
    }
    for (int sh = 32; sh > 0; sh >>= 1) { const int o = __shfl_xor(first, sh); first = o < first ? o : first; }
    if (lane == 0) {
        q.num_stitches[b] = ns;
        q.first_invalid[b] = first == 0x7fffffff ? -1 : first;
    }
}

// tags_to_stitches alone, batched: the pairs in the order they are taken, zero tails
__global__ __launch_bounds__(QM_TPB) void gpe_tags_to_stitches_kernel(QmEdgeViews v, int P, int L, int S, int32_t* __restrict__ stitches,
                                                                      int32_t* __restrict__ num_stitches)
{
    __shared__ QmGreedyLds g;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int PL = P * L;
    int32_t* st = stitches + (size_t)b * 2 * S;
    int drop, ns = 0;
    int m = qm_count_nonfree(v, b, PL, L, lane, &drop, [](int, float) {});
    if (m >= 2) {
        m = qm_stage_tags(v, b, PL, L, lane, drop, nullptr, nullptr, g);
        ns = qm_greedy_rounds(m, v.D, lane, g);
        ns = ns > S ? S : ns;
    }
    for (int k = lane; k < S; k += QM_TPB) { st[k] = k < ns ? g.pa[k] : 0; st[S + k] = k < ns ? g.pb[k] : 0; }
    if (lane == 0) num_stitches[b] = ns;
}

extern "C" int gpe_tags_to_stitches(const float* tags, long t_sb, long t_sp, long t_sl, int D, const float* logit, long m_sb,
                                    long m_sp, long m_sl, int B, int P, int L, int32_t* stitches, int32_t* num_stitches,
                                    void* stream)
{
    if (B <= 0 || P <= 0 || L <= 0 || (long)P * L > QM_MAXE || !tags || !logit || D <= 0 || D > QM_MAXD || !num_stitches)
        return GPE_EINVAL;
    const int S = P * L / 2;
    if (S > 0 && !stitches) return GPE_EINVAL;
    QmEdgeViews v{tags, t_sb, t_sp, t_sl, D, logit, m_sb, m_sp, m_sl};
    hipLaunchKernelGGL(gpe_tags_to_stitches_kernel, dim3(B), dim3(QM_TPB), 0, (hipStream_t)stream, v, P, L, S, stitches,
                       num_stitches);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_pattern_decode(const float* ol, long ol_sb, long ol_sp, long ol_sl, const float* rot, long rot_s, int R,
                                  const float* tr, long tr_s, int T, const float* tags, long t_sb, long t_sp, long t_sl, int D,
                                  const float* logit, long m_sb, long m_sp, long m_sl, const int32_t* given,
                                  const int32_t* given_num, int B, int P, int L, int S, int flags, const double* stats_host,
                                  int32_t* num_edges, int32_t* edge_slot, int32_t* num_verts, int32_t* closed,
                                  int32_t* new_panel_id, int32_t* num_panels, double* vertices, double* curvature,
                                  double* rotations, double* translations, int32_t* curved, int32_t* stitches,
                                  int32_t* num_stitches, int32_t* stitch_flags, int32_t* first_invalid, void* stream)
{
    if (B <= 0 || P <= 0 || L <= 0 || (long)P * L > QM_MAXE || (flags & ~PD_TAG_STATS) || !stats_host) return GPE_EINVAL;
    if (R <= 0 || R > QM_MAXD || T <= 0 || T > QM_MAXD || !ol || !rot || !tr) return GPE_EINVAL;
    if (S < 0 || (!given && S != P * L / 2)) return GPE_EINVAL;
    if (!given && (!tags || !logit || D <= 0 || D > QM_MAXD)) return GPE_EINVAL;
    if (!num_edges || !edge_slot || !num_verts || !closed || !new_panel_id || !num_panels || !vertices || !curvature || !rotations ||
        !translations || !curved || !num_stitches || !first_invalid)
        return GPE_EINVAL;
    if (S > 0 && (!stitches || !stitch_flags)) return GPE_EINVAL;
    PdStats s;
    for (int k = 0; k < PD_N; ++k) s.v[k] = stats_host[k];
    PdParams q{ol, ol_sb, ol_sp, ol_sl, rot, rot_s, R, tr, tr_s, T, {tags, t_sb, t_sp, t_sl, D, logit, m_sb, m_sp, m_sl},
               given, given_num, B, P, L, S, flags,
               num_edges, edge_slot, num_verts, closed, new_panel_id, num_panels, curved,
               vertices, curvature, rotations, translations, stitches, num_stitches, stitch_flags, first_invalid};
    hipLaunchKernelGGL(gpe_pattern_decode_kernel, dim3(B), dim3(QM_TPB), 0, (hipStream_t)stream, q, s);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
