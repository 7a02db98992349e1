// Kernel template + launch plumbing of the single-role fused edge GEMM (see gpe_edgegemm_sr.hip for the design notes).
// Included by TWO translation units that are compiled with different scheduling strategies (build.py EXTRA_FLAGS):
//   gpe_edgegemm_sr.hip        default scheduler   — the gather forward (A_GATHER) and the gathered-activation backward
//   gpe_edgegemm_sr_dense.hip  -amdgpu-sched-strategy=max-ilp — the dense-A forward and the in-place backward
// (A/B in one session, scripts/sr_probe.py + GPE_HIP_LIB, us per launch at cfg 2: in-place backward 723 -> 676 under max-ilp,
// dense forward 729 -> 712; the gather forward 790 -> 825 and the gathered backward unchanged, hence the split.)
#pragma once
#include "gpe_edge_dispatch.h"
#include <math.h>

// K16: k == 16 (the benchmark configuration): every wave owns exactly ONE point per tile, so the slot index of a row is
// its compile-time position u, a point completes exactly at u == 15, and row validity is one per-tile predicate — the
// per-row bookkeeping (and the register copies its branches cost) disappears from the epilogue.
// HALF: K ends within the first 8 columns of the last 16-k chunk (K = 200, 150).  That chunk then runs as TWO k4
// steps over its lower half — lane group g supplies k = 2g, 2g+1 instead of 4g..4g+3, for A and for the resident weights alike —
// instead of four steps of which half the products multiply the zero padding (3.8-5 % of a tile's MFMAs).
// KC: compile-time rows per (pseudo-)point — 16 (above), 4 (k = 20, 24, ... as pseudo-points of four rows: four points per
// wave and tile, slot = u % 4, P row = the (u / 4)-th of the wave's four — no per-row selects or counters), or 0 = generic.
// AGG >= 0 (k == 16 instances of the forward / gathered-backward variants): STRAIGHT-LINE slices.  The memory / epilogue slice of
// a chunk then contains no branch and no exec-masked region, so it shares a basic block with the chunk's MFMAs and the
// scheduler weaves the two (measured: 171 non-MFMA runs of <= 14 instructions instead of 11 runs of 47-268, and fewer of
// them — 511 VALU + 260 SALU per tile instead of 813 + 410 on the gather forward; 5-6 % per launch):
//   * `do_stage`: the rows of the next tile are always committed (their loads are clamped anyway; a tile past the end is
//     never multiplied);
//   * `do_epi` / a wave whose rows lie past the end of a partial last tile: the epilogue always runs, but its global stores
//     are redirected to a 64 KB dummy image (p.dummy) and its statistics are not flushed;
//   * lanes past the last column quad repeat the last valid quad (same addresses, same data) instead of being masked;
//   * AGG = the compile-time value of p.agg (the per-point max / min / arg tracking of the aggregated last block).
template <int AQ, int BQ, int KCH, int AMODE, int EMODE, int KC, bool HALF = false, int AGG = -1>
__global__ __launch_bounds__(256, 1) void gpe_edgegemm_sr_kernel(RgParams p, int stats_nblk)
{
    constexpr bool K16 = KC == 16;
    // (in place: the woven schedule measured 1.5x SLOWER; KC = 4: the host only picks these instances when no tile is partial)
    constexpr bool SL = (K16 || KC == 4) && AGG >= 0 && EMODE != E_BWD_INPLACE;
    constexpr int NT = 4 * AQ + BQ;
    constexpr int LDA = 16 * KCH + 4, LDC = 16 * NT + 4;
    // chunk schedule.  Chunk 0 issues every global load of the iteration.  The staged rows are committed to LDS FIRST
    // (chunks CM_START.., CMC rows each) and the epilogue runs in the LAST chunks (EPC rows each): the other way round the
    // commit's s_waitcnt vmcnt(N) would also wait for the epilogue's just-issued global stores (vmcnt counts stores too
    // and retires in order), ~1-2 us of HBM write latency per tile.
    constexpr int CM_START = 2;
    constexpr int CM_CH = (KCH >= 13) ? 4 : 3;
    constexpr int CMC = (RG_PB + CM_CH - 1) / CM_CH;
    constexpr int EPC = (KCH >= 13) ? 2 : 3;
    constexpr int EP_CH = (RG_PB + EPC - 1) / EPC;
    constexpr int EP_START = KCH - EP_CH;
    static_assert(EP_START >= 2, "K too short for the chunk schedule");
    constexpr bool GATHER_ACT = (EMODE == E_BWD_GATHER);

    extern __shared__ __align__(16) float smem[];
    float* const Abuf0 = smem;
    float* const Abuf1 = smem + RG_BM * LDA;
    float* const Cs = smem + 2 * RG_BM * LDA;            // [64][LDC]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int rows_w = p.R >> 2;                         // rows of a tile this wave stages / finishes (<= RG_PB)
    const int rb = wave * rows_w;
    const int rk16 = (65536 + p.k - 1) / p.k;            // u / k == (u * rk16) >> 16 for u < 64
    const int PT = p.R / p.k, npw = PT >> 2;             // points per tile / per wave: first point of this wave's
                                                         // share of tile t is t*PT + wave*npw — no per-tile division
    const int c = lane << 2;                             // this lane's column quad
    const bool k_real = c < p.K, n_real = c < p.N;
    const bool k_on = SL || k_real, n_on = SL || n_real; // SL: no lane is masked, lanes past the end repeat the last quad
    const bool track_agg = (AGG >= 0) ? (AGG != 0) : (p.agg != 0);   // wave-uniform (compile-time for AGG >= 0)
    // clamped quads for the unconditional loads; SL: also for the stores (the last valid quad: same address, same data)
    const int ck = k_real ? c : (SL ? ((p.K - 1) & ~3) : 0), cn = n_real ? c : (SL ? ((p.N - 1) & ~3) : 0);
    const int cs_k = SL ? ck : c, cs_n = SL ? cn : c;    // column quad of the LDS commit / of the global stores

    for (int e = tid; e < 2 * RG_BM * LDA; e += 256) smem[e] = 0.f;

    // ---- weights: resident MFMA B fragments -------------------------------------------------------------------------
    float4 wA[AQ][KCH], wL[BQ > 0 ? BQ : 1][KCH];
    {
        // all KCH fragment loads of an N-tile are issued before the first one is pinned (the pin is an asm statement that
        // needs its operand, so load-pin-load-pin would serialise ~200 dependent round trips in the prologue)
        auto load_tile = [&](int col, float4 (&dst)[KCH]) {
            const int cc = (col < p.Npad) ? col : p.Npad - 1;
            float4 t[KCH];
#pragma unroll
            for (int kc = 0; kc < KCH; ++kc) {
                if (HALF && kc == KCH - 1) {
                    // k = 16 kc + 2g + {0, 1}: packed element (plane (2g + t) / 4, component (2g + t) % 4)
                    const int k0 = 2 * g, k1 = 2 * g + 1;
                    t[kc].x = p.wp[(((long)(kc * 4 + (k0 >> 2))) * p.Npad + cc) * 4 + (k0 & 3)];
                    t[kc].y = p.wp[(((long)(kc * 4 + (k1 >> 2))) * p.Npad + cc) * 4 + (k1 & 3)];
                    t[kc].z = 0.f; t[kc].w = 0.f;
                } else
                    t[kc] = ld4(p.wp + (((long)(kc * 4 + g)) * p.Npad + cc) * 4);
            }
#pragma unroll
            for (int kc = 0; kc < KCH; ++kc)
                dst[kc] = rg_pin_agpr4((col < p.Npad) ? t[kc] : make_float4(0.f, 0.f, 0.f, 0.f));
        };
#pragma unroll
        for (int i = 0; i < AQ; ++i) load_tile(16 * (AQ * wave + i) + j, wA[i]);
#pragma unroll
        for (int b = 0; b < BQ; ++b) load_tile(16 * (4 * AQ + b) + j, wL[b]);
    }

    // ---- epilogue constants + running state ---------------------------------------------------------------------------
    double stS[4] = {0, 0, 0, 0}, stQ[4] = {0, 0, 0, 0};
    float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 cs4 = bias4, c14 = bias4, k24 = bias4, mu4 = bias4;
    if (n_on) {
        if (EMODE == E_EDGE_FWD) {
            if (p.bias) {
                bias4.x = p.bias[cs_n];
                if (cs_n + 1 < p.N) bias4.y = p.bias[cs_n + 1];
                if (cs_n + 2 < p.N) bias4.z = p.bias[cs_n + 2];
                if (cs_n + 3 < p.N) bias4.w = p.bias[cs_n + 3];
            }
        } else {                                         // N % 4 == 0 guaranteed by the dispatcher
            cs4 = ld4(p.coef_out + cs_n); c14 = ld4(p.coef_out + p.N + cs_n);
            k24 = ld4(p.coef_out + 2 * p.N + cs_n); mu4 = ld4(p.coef_out + 3 * p.N + cs_n);
        }
    }
    float s32[4], q32[4], vmx[4], vmn[4];
    int imx[4], imn[4];
    float4 dp;
    int es = 0, ept = 0;                                 // row inside the current point, point inside this wave's share
    long e_row0 = 0, e_pt0 = 0; int e_rv = 0;            // tile being finished
    // SL: where the epilogue of the tile being finished stores — the real rows, or the dummy image when this wave has nothing
    // valid to finish (first iteration, rows past the end of a partial last tile)
    bool e_live = true;
    float* e_out = p.out;                                // row r of the tile at e_out + r * ldo
    float *e_mx = p.mx, *e_mn = p.mn, *e_dp = p.dP;      // the wave's point of the tile
    uint8_t *e_amx = p.oamx, *e_amn = p.oamn;

    float4 v[RG_PB];                                     // rows staged for the next tile
    float4 pvs0, pvs1, pvs2, pvs3;                       // P rows of the points being staged (gather)
    pvs0 = pvs1 = pvs2 = pvs3 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 act[(EMODE != E_EDGE_FWD) ? RG_PB : 1];       // stored activations of the tile being finished (backward)
    float4 pve0, pve1, pve2, pve3;                       // P rows of the points being finished (E_BWD_GATHER)
    pve0 = pve1 = pve2 = pve3 = make_float4(0.f, 0.f, 0.f, 0.f);
    int s_rv = 0;                                        // valid rows of the tile being staged

    // Row addressing of the gathers stays in VGPRs: 16 rows x 64-bit scalar addresses (plus their clamps) do not fit the
    // SGPR file next to this kernel's ~60 live scalars, and SGPR spills go to scratch memory (every reload is a
    // scratch_load + s_waitcnt vmcnt(0) in the middle of the load pipeline).  So a tile's neighbour rows are loaded
    // lane-distributed ONE ITERATION AHEAD (lane L <-> row rb + min(L, rows_w-1)), a row's value is broadcast with
    // ds_bpermute, and `vz` (an opaque zero) keeps the point indices per-lane as well.
    int vz;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
    // LICM would hoist ~250 per-row scalars (row numbers, LDS offsets, point indices — all functions of rb, rows_w and
    // rk16) out of the persistent tile loop and the register allocator would then spill them to scratch; re-deriving them
    // from an opaque per-iteration zero keeps them transient.
    int rbl = rb, rwl = rows_w, rkl = rk16;
#define SR_REFRESH_SCALARS()                                   \
    {                                                          \
        int sz_;                                               \
        asm volatile("s_mov_b32 %0, 0" : "=s"(sz_));           \
        rbl = rb + sz_; rwl = rows_w + sz_; rkl = rk16 + sz_;  \
    }
    auto load_jgv = [&](int tile) -> int {
        const long row0 = (long)tile * p.R;
        const int rv = (int)((p.M - row0 < p.R) ? (p.M - row0) : p.R);
        int r = rbl + ((lane < rwl) ? lane : rwl - 1);
        r = (r < rv - 1) ? r : rv - 1;
        return p.jg[row0 + r];
    };
    int jgv_s = 0, jgv_e = 0;            // neighbour rows for the NEXT stage (A_GATHER) / the NEXT epilogue (E_BWD_GATHER)

    // ---- VMEM issue: everything this iteration will need --------------------------------------------------------------
    auto issue_epi_loads = [&](int tile, bool live) {
        e_row0 = (long)tile * p.R;
        e_pt0 = (long)tile * PT + wave * npw;
        e_rv = (int)((p.M - e_row0 < p.R) ? (p.M - e_row0) : p.R);
        es = 0; ept = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) { s32[t] = 0.f; q32[t] = 0.f; vmx[t] = -INFINITY; vmn[t] = INFINITY; imx[t] = 0; imn[t] = 0; }
        dp = make_float4(0.f, 0.f, 0.f, 0.f);
        if (SL) {
            e_live = live && rbl < e_rv;                 // K16: all 16 rows of the wave's point are valid or none is
            e_out = e_live ? p.out + e_row0 * p.ldo : p.dummy;
            if (EMODE == E_EDGE_FWD && track_agg) {
                e_mx = e_live ? p.mx + e_pt0 * p.oldagg : p.dummy;
                e_mn = e_live ? p.mn + e_pt0 * p.oldagg : p.dummy;
                e_amx = e_live ? p.oamx + e_pt0 * p.oldagg : reinterpret_cast<uint8_t*>(p.dummy);
                e_amn = e_live ? p.oamn + e_pt0 * p.oldagg : reinterpret_cast<uint8_t*>(p.dummy);
            }
            if (EMODE == E_BWD_GATHER) e_dp = e_live ? p.dP + e_pt0 * p.lddp : p.dummy;
        }
        if (EMODE == E_EDGE_FWD) return;
        // NOTE: every load below is unconditional (clamped rows, clamped column quad): a register that is loaded under a
        // branch needs a copy at the join, and that copy waits for the load right there — no pipelining left
        const int last = e_rv - 1;
#pragma unroll
        for (int u = 0; u < RG_PB; ++u) {
            int r = rbl + ((u < rwl) ? u : rwl - 1);
            r = (r < last) ? r : last;                                  // clamp: unconditional loads
            if (EMODE == E_BWD_INPLACE) act[u] = ld4(p.out + (e_row0 + r) * p.ldo + cn);
            else {
                const int jj = __builtin_amdgcn_ds_bpermute(u << 2, jgv_e);
                act[u] = ld4(p.pq + (long)jj * p.ldpq + p.H + cn);
            }
        }
        if (GATHER_ACT) {
            const int pt0 = tile * PT + wave * npw + vz, ptl = tile * PT + ((last * rkl) >> 16);
            pve0 = ld4(p.pq + rg_prow((pt0 + 0 < ptl) ? pt0 + 0 : ptl, p.pmagic) * p.ldpq + cn);
            pve1 = ld4(p.pq + rg_prow((pt0 + 1 < ptl) ? pt0 + 1 : ptl, p.pmagic) * p.ldpq + cn);
            pve2 = ld4(p.pq + rg_prow((pt0 + 2 < ptl) ? pt0 + 2 : ptl, p.pmagic) * p.ldpq + cn);
            pve3 = ld4(p.pq + rg_prow((pt0 + 3 < ptl) ? pt0 + 3 : ptl, p.pmagic) * p.ldpq + cn);
        }
    };
    auto issue_stage_loads = [&](int tile) {
        const long row0 = (long)tile * p.R;
        s_rv = (int)((p.M - row0 < p.R) ? (p.M - row0) : p.R);
        const int last = s_rv - 1;
#pragma unroll
        for (int u = 0; u < RG_PB; ++u) {
            int r = rbl + ((u < rwl) ? u : rwl - 1);
            r = (r < last) ? r : last;
            if (AMODE == A_GATHER) {
                const int jj = __builtin_amdgcn_ds_bpermute(u << 2, jgv_s);
                v[u] = ld4(p.pq + (long)jj * p.ldpq + p.H + ck);
            } else {
                // rows are 16-B aligned and padded to a multiple of 4 columns (checked by the dispatcher)
                v[u] = ld4(p.a.base + (row0 + r) * p.a.stride_outer + ck);
            }
        }
        if (AMODE == A_GATHER) {
            const int pt0 = tile * PT + wave * npw + vz, ptl = tile * PT + ((last * rkl) >> 16);
            pvs0 = ld4(p.pq + rg_prow((pt0 + 0 < ptl) ? pt0 + 0 : ptl, p.pmagic) * p.ldpq + ck);
            pvs1 = ld4(p.pq + rg_prow((pt0 + 1 < ptl) ? pt0 + 1 : ptl, p.pmagic) * p.ldpq + ck);
            pvs2 = ld4(p.pq + rg_prow((pt0 + 2 < ptl) ? pt0 + 2 : ptl, p.pmagic) * p.ldpq + ck);
            pvs3 = ld4(p.pq + rg_prow((pt0 + 3 < ptl) ? pt0 + 3 : ptl, p.pmagic) * p.ldpq + ck);
        }
    };
    // ---- LDS commit of staged row u (compile-time u) ------------------------------------------------------------------
    auto commit_row = [&](float* An, int u) {
        if ((!KC && u >= rwl) || !k_on) return;
        const int r = rbl + u;
        float4 o = v[u];
        if (AMODE == A_GATHER) {
            const float4 pv = K16 ? pvs0 : (KC == 4) ? ((u >> 2) == 0 ? pvs0 : (u >> 2) == 1 ? pvs1 : (u >> 2) == 2 ? pvs2 : pvs3)
                                                     : rg_sel4(pvs0, pvs1, pvs2, pvs3, (u * rkl) >> 16);
            o.x = fmaxf(o.x + pv.x, 0.f); o.y = fmaxf(o.y + pv.y, 0.f);
            o.z = fmaxf(o.z + pv.z, 0.f); o.w = fmaxf(o.w + pv.w, 0.f);
        }
        // rows past the end of a partial last tile hold a copy of the last valid row (clamped loads): every output row
        // depends on its own A row only and the epilogue skips rows >= e_rv, so they need no zeroing (4 v_cndmask per row)
        st4(&An[r * LDA + cs_k], o);
    };
    // ---- epilogue of row u (compile-time u) of the tile being finished ------------------------------------------------
    auto epi_row = [&](int u, const float4 z) {
        if (!KC && u >= rwl) return;
        const int r = rbl + u;
        if (!SL && r >= e_rv) return;        // K16: all 16 rows of the wave's point are valid or none is (uniform)
        const int slot = KC ? (u % (KC ? KC : 1)) : es;
        if (n_on) {
            if (EMODE == E_EDGE_FWD) {
                const float vv[4] = {fmaxf(z.x + bias4.x, 0.f), fmaxf(z.y + bias4.y, 0.f), fmaxf(z.z + bias4.z, 0.f),
                                     fmaxf(z.w + bias4.w, 0.f)};
                // gather variant: the activation rows stream out past L2 so that they do not evict the cloud's Q table
                // (counter fetch of this kernel 199 -> <145 MB against 109 MB compulsory, same run time: profiles/r02_b)
                float* const orow = SL ? e_out + (long)r * p.ldo + cs_n : p.out + (e_row0 + r) * p.ldo + c;
                if (AMODE == A_GATHER) st4_stream(orow, make_float4(vv[0], vv[1], vv[2], vv[3]));
                else st4(orow, make_float4(vv[0], vv[1], vv[2], vv[3]));
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    s32[t] += vv[t];
                    q32[t] = __builtin_fmaf(vv[t], vv[t], q32[t]);
                }
                // per-point max / min / argmax / argmin only where the block is aggregated (the last layer of an EdgeConv
                // MLP): 6 VALU instructions per element — a fifth of a tile's non-MFMA instructions — that the inner
                // layers never store (uniform branch)
                if (track_agg) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        if (vv[t] > vmx[t]) { vmx[t] = vv[t]; imx[t] = slot; }
                        if (vv[t] < vmn[t]) { vmn[t] = vv[t]; imn[t] = slot; }
                    }
                }
            } else {
                float4 av = act[u];
                if (GATHER_ACT) {
                    const float4 pv = K16 ? pve0 : (KC == 4) ? ((u >> 2) == 0 ? pve0 : (u >> 2) == 1 ? pve1 : (u >> 2) == 2 ? pve2 : pve3)
                                                             : rg_sel4(pve0, pve1, pve2, pve3, (u * rkl) >> 16);
                    av.x = fmaxf(av.x + pv.x, 0.f); av.y = fmaxf(av.y + pv.y, 0.f);
                    av.z = fmaxf(av.z + pv.z, 0.f); av.w = fmaxf(av.w + pv.w, 0.f);
                }
                float4 o;
                o.x = (av.x > 0.f) ? z.x * cs4.x - c14.x - (av.x - mu4.x) * k24.x : 0.f;
                o.y = (av.y > 0.f) ? z.y * cs4.y - c14.y - (av.y - mu4.y) * k24.y : 0.f;
                o.z = (av.z > 0.f) ? z.z * cs4.z - c14.z - (av.z - mu4.z) * k24.z : 0.f;
                o.w = (av.w > 0.f) ? z.w * cs4.w - c14.w - (av.w - mu4.w) * k24.w : 0.f;
                st4(SL ? e_out + (long)r * p.ldo + cs_n : p.out + (e_row0 + r) * p.ldo + c, o);
                dp.x += o.x; dp.y += o.y; dp.z += o.z; dp.w += o.w;
            }
        }
        if (KC ? ((u % (KC ? KC : 1)) == KC - 1) : (++es == p.k)) {        // a point is complete (KC: compile-time)
            if (n_on) {
                const long gpt = e_pt0 + (KC ? (u / (KC ? KC : 1)) : ept);
                if (EMODE == E_EDGE_FWD && track_agg) {
                    if (SL) {                            // the (u / KC)-th point of the wave's share of the tile
                        const long po = (long)(u / (KC ? KC : 1)) * p.oldagg + cs_n;
                        st4(e_mx + po, make_float4(vmx[0], vmx[1], vmx[2], vmx[3]));
                        st4(e_mn + po, make_float4(vmn[0], vmn[1], vmn[2], vmn[3]));
                        *reinterpret_cast<uchar4*>(e_amx + po) = make_uchar4(imx[0], imx[1], imx[2], imx[3]);
                        *reinterpret_cast<uchar4*>(e_amn + po) = make_uchar4(imn[0], imn[1], imn[2], imn[3]);
                    } else {
                        const long o = gpt * p.oldagg + c;
                        st4(p.mx + o, make_float4(vmx[0], vmx[1], vmx[2], vmx[3]));
                        st4(p.mn + o, make_float4(vmn[0], vmn[1], vmn[2], vmn[3]));
                        *reinterpret_cast<uchar4*>(p.oamx + o) = make_uchar4(imx[0], imx[1], imx[2], imx[3]);
                        *reinterpret_cast<uchar4*>(p.oamn + o) = make_uchar4(imn[0], imn[1], imn[2], imn[3]);
                    }
                }
                if (EMODE == E_BWD_GATHER) st4(SL ? e_dp + (long)(u / (KC ? KC : 1)) * p.lddp + cs_n : p.dP + gpt * p.lddp + c, dp);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) { vmx[t] = -INFINITY; vmn[t] = INFINITY; imx[t] = 0; imn[t] = 0; }
            dp = make_float4(0.f, 0.f, 0.f, 0.f);
            es = 0; ++ept;
        }
    };
    auto epi_flush_stats = [&]() {
        if (EMODE == E_EDGE_FWD) {
#pragma unroll
            for (int t = 0; t < 4; ++t) { stS[t] += (double)s32[t]; stQ[t] += (double)q32[t]; }
        }
    };

    // ---- tile sequence of this workgroup --------------------------------------------------------------------------------
    // unpinned: blockIdx.x, +gridDim.x, ...   pinned (p.pin_tpc > 0; gridDim.x % 8 == 0, B % 8 == 0, tiles never straddle
    // clouds): this workgroup sits on XCD x = blockIdx.x % 8 and takes every (gridDim.x/8)-th tile of clouds x, x+8, ... —
    // the gathered Q table of a cloud (3.3 MB at the shipped sizes) is then read through ONE 4 MiB L2 instead of eight.
    // Sequence positions past the end map to tile numbers >= num_tiles in both modes.
    const int seq_step = p.pin_tpc ? (int)(gridDim.x >> 3) : (int)gridDim.x;
    int seq_t = p.pin_tpc ? (int)(blockIdx.x >> 3) : (int)blockIdx.x;      // pinned: tile inside the cloud
    int seq_c = p.pin_tpc ? (int)(blockIdx.x & 7) : 0;                     // pinned: cloud
    auto seq_tile = [&]() -> int { return p.pin_tpc ? seq_c * p.pin_tpc + seq_t : seq_t; };
    auto seq_advance = [&]() {
        seq_t += seq_step;
        if (p.pin_tpc && seq_t >= p.pin_tpc) { seq_t -= p.pin_tpc; seq_c += GPE_NXCD; }   // host: seq_step <= pin_tpc
    };

    // ---- prologue: stage tile 0 ---------------------------------------------------------------------------------------
    __syncthreads();                                     // A buffers zeroed
    int tile = seq_tile();
    seq_advance();
    int next = seq_tile();
    seq_advance();
    int next2 = seq_tile();
    if (tile < p.num_tiles) {
        if (AMODE == A_GATHER) jgv_s = load_jgv(tile);
        if (GATHER_ACT) jgv_e = load_jgv(tile);
    }
    if (tile < p.num_tiles && !(p.dbg & 1)) {
        issue_stage_loads(tile);
#pragma unroll
        for (int u = 0; u < RG_PB; ++u) commit_row(Abuf0, u);
    }
    if (AMODE == A_GATHER && tile < p.num_tiles) jgv_s = load_jgv(next < p.num_tiles ? next : tile);
    __syncthreads();

    int buf = 0, prev = -1;
    for (; tile < p.num_tiles; tile = next, next = next2, seq_advance(), next2 = seq_tile()) {
        SR_REFRESH_SCALARS()
        const float* As = buf ? Abuf1 : Abuf0;
        float* An = buf ? Abuf0 : Abuf1;
        const bool do_epi = prev >= 0 && !(p.dbg & 2);
        const bool do_stage = SL || (next < p.num_tiles && !(p.dbg & 1));   // SL: always (clamped loads, harmless LDS rows)

        f32x4 acc[4][AQ], accL[BQ > 0 ? BQ : 1];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < AQ; ++i) acc[mt][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < (BQ > 0 ? BQ : 1); ++b) accL[b] = (f32x4){0.f, 0.f, 0.f, 0.f};

        float4 an[4], anL = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 zq[EPC];
#pragma unroll
        for (int q = 0; q < EPC; ++q) zq[q] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) an[mt] = ld4(&As[(16 * mt + j) * LDA + 4 * g]);
        if (BQ > 0) anL = ld4(&As[(16 * wave + j) * LDA + 4 * g]);

#pragma unroll
        for (int kc = 0; kc < KCH; ++kc) {
            float a[4][4], aL[4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) { a[mt][0] = an[mt].x; a[mt][1] = an[mt].y; a[mt][2] = an[mt].z; a[mt][3] = an[mt].w; }
            aL[0] = anL.x; aL[1] = anL.y; aL[2] = anL.z; aL[3] = anL.w;
            if (kc + 1 < KCH) {
                if (HALF && kc + 1 == KCH - 1) {         // half chunk: k = 2g, 2g+1 in .x, .y
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) {
                        const float2 h2 = *reinterpret_cast<const float2*>(&As[(16 * mt + j) * LDA + 16 * (kc + 1) + 2 * g]);
                        an[mt] = make_float4(h2.x, h2.y, 0.f, 0.f);
                    }
                    if (BQ > 0) {
                        const float2 h2 = *reinterpret_cast<const float2*>(&As[(16 * wave + j) * LDA + 16 * (kc + 1) + 2 * g]);
                        anL = make_float4(h2.x, h2.y, 0.f, 0.f);
                    }
                } else {
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) an[mt] = ld4(&As[(16 * mt + j) * LDA + 16 * (kc + 1) + 4 * g]);
                    if (BQ > 0) anL = ld4(&As[(16 * wave + j) * LDA + 16 * (kc + 1) + 4 * g]);
                }
            }
            // ---- this chunk's slice of the memory pipeline ----
            if (kc == 0) {
                issue_epi_loads(prev >= 0 ? prev : tile, do_epi);    // clamped: results unused when !do_epi
                issue_stage_loads(next < p.num_tiles ? next : tile); // clamped: results unused when !do_stage
                if (GATHER_ACT) jgv_e = load_jgv(tile);              // this tile is finished in the next iteration
                if (AMODE == A_GATHER) jgv_s = load_jgv(next2 < p.num_tiles ? next2 : tile);
            }
            if (kc >= CM_START && kc < CM_START + CM_CH) {
                if (do_stage) {
#pragma unroll
                    for (int q = 0; q < CMC; ++q) {
                        const int u = (kc - CM_START) * CMC + q;
                        if (u < RG_PB) commit_row(An, u);
                    }
                }
            }
            if (kc >= EP_START) {
                if (SL || do_epi) {
#pragma unroll
                    for (int q = 0; q < EPC; ++q) {
                        const int u = (kc - EP_START) * EPC + q;
                        if (u < RG_PB) epi_row(u, zq[q]);
                    }
                }
            }
            if (kc + 1 >= EP_START && kc + 1 < KCH) {            // C rows of the NEXT chunk's epilogue slice (LDS prefetch)
#pragma unroll
                for (int q = 0; q < EPC; ++q) {
                    const int u = (kc + 1 - EP_START) * EPC + q;
                    const int rr = rbl + ((u < RG_PB) ? u : RG_PB - 1);
                    zq[q] = ld4(&Cs[((rr < RG_BM) ? rr : RG_BM - 1) * LDC + cn]);
                }
            }
            // memory slice stays in front of this chunk's MFMAs — except in the in-place backward variant, where letting the
            // scheduler sink the next chunk's operand reads into the MFMA block measured faster (771 -> 729 us per launch at
            // cfg 2; the same freedom costs the other three variants 1-3 % while their slices sit in blocks of their own),
            // and in the straight-line instances, whose slice is woven into the MFMA stream: scripts/sr_probe.py, round 3
            if (EMODE != E_BWD_INPLACE && !SL) __builtin_amdgcn_sched_barrier(0);
            // gathered-activation backward: the compiler's MFMA / DS interleaving pass on top of the woven slice (849 -> 795 us per
            // launch; neutral on the two forward variants)
            if (SL && EMODE == E_BWD_GATHER) __builtin_amdgcn_iglp_opt(0);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (HALF && kc == KCH - 1 && t >= 2) continue;       // compile-time: the half chunk has two k4 steps
#pragma unroll
                for (int i = 0; i < AQ; ++i) {
                    const float bv = (t == 0) ? wA[i][kc].x : (t == 1) ? wA[i][kc].y : (t == 2) ? wA[i][kc].z : wA[i][kc].w;
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt)
                        acc[mt][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][t], bv, acc[mt][i], 0, 0, 0);
                }
#pragma unroll
                for (int b = 0; b < BQ; ++b) {
                    const float bv = (t == 0) ? wL[b][kc].x : (t == 1) ? wL[b][kc].y : (t == 2) ? wL[b][kc].z : wL[b][kc].w;
                    accL[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(aL[t], bv, accL[b], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (SL ? e_live : do_epi) epi_flush_stats();
        __syncthreads();                                 // (1) every wave is done with C (epilogue of the previous tile)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < AQ; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    Cs[(16 * mt + 4 * g + r) * LDC + 16 * (AQ * wave + i) + j] = acc[mt][i][r];
#pragma unroll
        for (int b = 0; b < BQ; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) Cs[(16 * wave + 4 * g + r) * LDC + 16 * (4 * AQ + b) + j] = accL[b][r];
        __syncthreads();                                 // (2) C complete, next A tile complete
        prev = tile;
        buf ^= 1;
    }
    // ---- tail: epilogue of the last tile -------------------------------------------------------------------------------
    if (prev >= 0 && !(p.dbg & 2)) {
        issue_epi_loads(prev, true);
#pragma unroll
        for (int u = 0; u < RG_PB; ++u) {
            const int rr = rbl + u;
            epi_row(u, ld4(&Cs[((rr < RG_BM) ? rr : RG_BM - 1) * LDC + cn]));
        }
        if (!SL || e_live) epi_flush_stats();
    }
    __syncthreads();
    if (EMODE == E_EDGE_FWD && p.stats_part) {
        double* red = reinterpret_cast<double*>(smem);          // [4 waves][2][16*NT]
        if (n_real) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                red[(wave * 2 + 0) * (16 * NT) + c + t] = stS[t];
                red[(wave * 2 + 1) * (16 * NT) + c + t] = stQ[t];
            }
        }
        __syncthreads();
        if (tid < p.N) {
            constexpr int NC = 16 * NT;
            const double ss = (red[0 * NC + tid] + red[2 * NC + tid]) + (red[4 * NC + tid] + red[6 * NC + tid]);
            const double qq = (red[1 * NC + tid] + red[3 * NC + tid]) + (red[5 * NC + tid] + red[7 * NC + tid]);
            for (int b = blockIdx.x; b < stats_nblk; b += gridDim.x) {
                double* dst = p.stats_part + (size_t)b * 2 * p.N;
                dst[tid] = (b == (int)blockIdx.x) ? ss : 0.0;
                dst[p.N + tid] = (b == (int)blockIdx.x) ? qq : 0.0;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
template <int AQ, int BQ, int KCH, int AMODE, int EMODE, int KC, bool HALF = false, int AGG = -1>
static int sr_launch_k(const RgParams& p, int stats_nblk, hipStream_t s)
{
    constexpr int NT = 4 * AQ + BQ;
    constexpr int LDA = 16 * KCH + 4, LDC = 16 * NT + 4;
    const size_t lds = (size_t)RG_BM * (2 * LDA + LDC) * sizeof(float);
    return gpe_edge_launch<gpe_edgegemm_sr_kernel<AQ, BQ, KCH, AMODE, EMODE, KC, HALF, AGG>, 256, GPE_EDGE_LDS_CAP>(p, stats_nblk, lds, s);
}

template <int AQ, int BQ, int KCH, int AMODE, int EMODE>
static int sr_launch(const RgParams& p, int stats_nblk, hipStream_t s)
{
    const bool half = p.K <= 16 * (KCH - 1) + 8 && !(p.dbg & 128);
    if (p.k == 16) {
        // the benchmark's neighbourhood size: straight-line instances (AGG = p.agg at compile time) for every variant but the
        // in-place backward; they need the dummy image for redirected stores (p.dbg & 512: the branchy form, for A/B timing)
        if (EMODE != E_BWD_INPLACE && p.dummy && !(p.dbg & 512)) {
            const bool agg = EMODE == E_EDGE_FWD && p.agg;
            if (agg) return half ? sr_launch_k<AQ, BQ, KCH, AMODE, EMODE, 16, true, 1>(p, stats_nblk, s)
                                 : sr_launch_k<AQ, BQ, KCH, AMODE, EMODE, 16, false, 1>(p, stats_nblk, s);
            return half ? sr_launch_k<AQ, BQ, KCH, AMODE, EMODE, 16, true, 0>(p, stats_nblk, s)
                        : sr_launch_k<AQ, BQ, KCH, AMODE, EMODE, 16, false, 0>(p, stats_nblk, s);
        }
        return half ? sr_launch_k<AQ, BQ, KCH, AMODE, EMODE, 16, true>(p, stats_nblk, s)
                    : sr_launch_k<AQ, BQ, KCH, AMODE, EMODE, 16>(p, stats_nblk, s);
    }
    // (the one KC = 4 instance the register allocator cannot fit without scratch runs as generic k)
    constexpr bool k4_full_ok = !(EMODE == E_BWD_GATHER && AQ == 3 && KCH == 13);
    if (p.k == 4 && !(p.dbg & 256) && (half || k4_full_ok)) {
        // four-row pseudo-points (k = 20, 24, ...): straight-line instances when no tile is partial
        if (EMODE != E_BWD_INPLACE && p.dummy && !(p.dbg & 512) && p.M % p.R == 0 && half) {
            const bool agg = EMODE == E_EDGE_FWD && p.agg;
            return agg ? sr_launch_k<AQ, BQ, KCH, AMODE, EMODE, 4, true, 1>(p, stats_nblk, s)
                       : sr_launch_k<AQ, BQ, KCH, AMODE, EMODE, 4, true, 0>(p, stats_nblk, s);
        }
        return half ? sr_launch_k<AQ, BQ, KCH, AMODE, EMODE, 4, true>(p, stats_nblk, s)
                    : sr_launch_k<AQ, BQ, KCH, AMODE, EMODE, k4_full_ok ? 4 : 0>(p, stats_nblk, s);
    }
    return half ? sr_launch_k<AQ, BQ, KCH, AMODE, EMODE, 0, true>(p, stats_nblk, s)
                : sr_launch_k<AQ, BQ, KCH, AMODE, EMODE, 0>(p, stats_nblk, s);
}

// The instances of this family, by translation unit (DENSE_TU: gpe_edgegemm_sr_dense.hip holds the dense forward and the in-place
// backward)
template <bool DENSE_TU> struct SrMenu {
    static constexpr bool has(int amode, int emode, int NT, int KCH) { return (amode == A_DENSE && emode != E_BWD_GATHER) == DENSE_TU; }
};
template <bool DENSE_TU>
static int sr_select(const RgParams& p, int amode, int emode, int NT, int KCH, int stats_nblk, hipStream_t s)
{
    return gpe_edge_select<SrMenu<DENSE_TU>>(amode, emode, NT, KCH, [&](auto m, auto t) {
        return sr_launch<decltype(t)::AQ, decltype(t)::BQ, decltype(t)::KCH, decltype(m)::amode, decltype(m)::emode>(p, stats_nblk, s);
    });
}
