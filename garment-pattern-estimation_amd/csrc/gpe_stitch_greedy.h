// tags_to_stitches (nn/data/datasets.py:917-968) for one garment on one wave: the free-edge decision, the odd-count drop and the
// greedy pairing of the non-free edges' stitch tags by global minimum distance.  The ONE implementation of it: included by
// gpe_quality.hip (stitch precision / recall) and gpe_pattern_decode.hip (the stitches themselves).
//
// All of it runs on QM_TPB = 64 threads (one wave) of a workgroup, every lane calling every function (they hold barriers and
// wave shuffles).  Order of calls: qm_count_nonfree -> (m >= 2) -> qm_stage_tags -> qm_greedy_rounds.
#ifndef GPE_STITCH_GREEDY_H
#define GPE_STITCH_GREEDY_H
#include "gpe_device.h"
#include <math.h>

// every product / sum below is rounded on its own, in the reference's order (no contraction into FMAs)
#pragma clang fp contract(off)

#define QM_TPB 64            // one wave per pattern
#define QM_MAXD 8            // rotation / translation / stitch-tag width
#define QM_MAXE 1024         // edges per pattern P*L (shipped: 322)

// predicted stitch tags (b,p,l,d) at tags + b*t_sb + p*t_sp + l*t_sl + d and free-edge logits (b,p,l) at logit + b*m_sb + p*m_sp +
// l*m_sl: the strided views of the panel decoder's output
struct QmEdgeViews {
    const float* tags; long t_sb, t_sp, t_sl; int D;
    const float* logit; long m_sb, m_sp, m_sl;
};

// the pairing's working set in LDS (43 KB)
struct QmGreedyLds {
    float T[QM_MAXE * QM_MAXD];         // staged tags of non-free edge k
    short ids[QM_MAXE];                 // pattern-level edge id of non-free edge k (edge order)
    float bd[QM_MAXE];                  // row k's best remaining distance ...
    short bj[QM_MAXE];                  // ... and the column that has it (-1: none)
    unsigned char alive[QM_MAXE];
    short pa[QM_MAXE / 2], pb[QM_MAXE / 2];     // the pairs, in the order they were taken
};

__device__ __forceinline__ float qm_logit(const QmEdgeViews& v, int b, int e, int L)
{
    const int pp = e / L, l = e - pp * L;
    return v.logit[b * v.m_sb + pp * v.m_sp + l * v.m_sl];
}

// torch.round(torch.sigmoid(x)) == 0 on the device: gpe_sigmoid (fp32 expf, IEEE division) and round half to even, so exactly
// 0.5 is a non-free edge.  NaN rounds to NaN, which is "free" (the reference casts it to True).
__device__ __forceinline__ bool qm_nonfree(float sg) { return sg <= 0.5f; }

__device__ __forceinline__ float qm_dist(const float* T, int i, int j, int D)
{
    float s = 0.f;
    for (int d = 0; d < D; ++d) { const float v = T[i * QM_MAXD + d] - T[j * QM_MAXD + d]; s += v * v; }
    return sqrtf(s);
}

// best remaining partner of row r: smallest distance over alive columns c > r, the smallest c on ties (-1: none)
__device__ __forceinline__ void qm_row_best(const float* T, const unsigned char* alive, int r, int m, int D, float* bd, short* bj)
{
    float best = INFINITY;
    int bc = -1;
    for (int c = r + 1; c < m; ++c) {
        if (!alive[c]) continue;
        const float d = qm_dist(T, r, c, D);
        if (d < best) { best = d; bc = c; }
    }
    bd[r] = best;
    bj[r] = (short)bc;
}

// pass 1: the decisions and their count.  Returns the number of non-free edges; *drop = the edge an odd count leaves out (the
// non-free edge with the largest logit, the first on ties: the one closest to "free"), -1 for an even count.  visit(e, sg) sees
// every edge e < PL once with its sigmoid, on the lane that owns it.
template <class Visit>
__device__ __forceinline__ int qm_count_nonfree(const QmEdgeViews& v, int b, int PL, int L, int lane, int* drop, Visit visit)
{
    int m = 0;
    float xmax = -INFINITY;
    int emax = 0x7fffffff;
    for (int e0 = 0; e0 < PL; e0 += QM_TPB) {
        const int e = e0 + lane;
        bool nonfree = false;
        if (e < PL) {
            const float x = qm_logit(v, b, e, L);
            const float sg = gpe_sigmoid(x);
            nonfree = qm_nonfree(sg);
            visit(e, sg);
            if (nonfree && (x > xmax || (x == xmax && e < emax))) { xmax = x; emax = e; }
        }
        m += __builtin_popcountll(__ballot(nonfree));
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float xo = __shfl_xor(xmax, o);
        const int eo = __shfl_xor(emax, o);
        if (xo > xmax || (xo == xmax && eo < emax)) { xmax = xo; emax = eo; }
    }
    *drop = (m & 1) ? emax : -1;
    return m;
}

// pass 2: compact the non-free edges but `drop` in edge order and stage their tags, un-standardised in fp32 with tag_scale /
// tag_shift when those are given (data_config['explicit_stitch_tags']).  Returns their count.  Ends with a barrier.
__device__ __forceinline__ int qm_stage_tags(const QmEdgeViews& v, int b, int PL, int L, int lane, int drop, const float* tag_shift,
                                             const float* tag_scale, QmGreedyLds& g)
{
    const unsigned long long below = (1ull << lane) - 1ull;
    int m = 0;
    for (int e0 = 0; e0 < PL; e0 += QM_TPB) {
        const int e = e0 + lane;
        bool nonfree = false;
        int pp = 0, l = 0;
        if (e < PL && e != drop) {
            pp = e / L; l = e - pp * L;
            nonfree = qm_nonfree(gpe_sigmoid(v.logit[b * v.m_sb + pp * v.m_sp + l * v.m_sl]));
        }
        const unsigned long long bal = __ballot(nonfree);
        if (nonfree) {
            const int k = m + __builtin_popcountll(bal & below);
            g.ids[k] = (short)e;
            g.alive[k] = 1;
            const float* t = v.tags + b * v.t_sb + pp * v.t_sp + l * v.t_sl;
            for (int d = 0; d < v.D; ++d) g.T[k * QM_MAXD + d] = tag_scale ? t[d] * tag_scale[d] + tag_shift[d] : t[d];
        }
        m += __builtin_popcountll(bal);
    }
    __syncthreads();
    return m;
}

// greedy rounds over the m staged edges: the global minimum over (row, best column), ties to the smallest row (row-major argmin
// of the reference's upper-triangular matrix); then only the rows whose best partner was just taken are re-scanned.  Returns the
// number of pairs, g.pa / g.pb hold their pattern-level edge ids.  Stops when only non-finite distances are left (NaN / inf tags).
__device__ __forceinline__ int qm_greedy_rounds(int m, int D, int lane, QmGreedyLds& g)
{
    for (int r = lane; r < m; r += QM_TPB) qm_row_best(g.T, g.alive, r, m, D, g.bd, g.bj);
    __syncthreads();
    int npairs = 0;
    for (int round = 0; round < m / 2; ++round) {
        float dmin = INFINITY;
        int rmin = 0x7fffffff;
        for (int r = lane; r < m; r += QM_TPB)
            if (g.alive[r] && g.bj[r] >= 0 && g.bd[r] < dmin) { dmin = g.bd[r]; rmin = r; }
        for (int sh = 32; sh > 0; sh >>= 1) {
            const float dq = __shfl_xor(dmin, sh);
            const int rq = __shfl_xor(rmin, sh);
            if (dq < dmin || (dq == dmin && rq < rmin)) { dmin = dq; rmin = rq; }
        }
        if (rmin == 0x7fffffff) break;
        const int cmin = g.bj[rmin];
        __syncthreads();
        if (lane == 0) { g.pa[npairs] = g.ids[rmin]; g.pb[npairs] = g.ids[cmin]; g.alive[rmin] = 0; g.alive[cmin] = 0; }
        ++npairs;
        __syncthreads();
        for (int r = lane; r < m; r += QM_TPB)
            if (g.alive[r] && (g.bj[r] == rmin || g.bj[r] == cmin)) qm_row_best(g.T, g.alive, r, m, D, g.bd, g.bj);
        __syncthreads();
    }
    return npairs;
}

#endif
