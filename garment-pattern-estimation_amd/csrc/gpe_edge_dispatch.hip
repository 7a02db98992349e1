// Which fused edge GEMM kernel runs: the order of families per arithmetic mode (gpe_edgegemm_try) and the re-tiling the
// single-role families share.  Host code only; the pieces are declared in gpe_edge_dispatch.h.
#include "gpe_edge_dispatch.h"

// ---- k > 16: pseudo-points ------------------------------------------------------------------------------------------------------
// A point with k > 16 neighbours is processed as f pseudo-points of kq = k / f rows (kq <= 16, so every wave still owns whole
// pseudo-points): the divisor of k that fills most of a wave's 16 rows, the largest such on a tie.
int gpe_edge_pseudo_kq(int k)
{
    int best = 0;
    for (int kq = RG_PB; kq >= RG_PB / RG_NPW; --kq)
        if (k % kq == 0 && (RG_PB / kq) * kq > (best ? (RG_PB / best) * best : 0)) best = kq;
    return best;
}

// bytes of the pseudo-point part of an edge workspace for k neighbours, widths <= Cmax (0 for k <= 16)
size_t gpe_edge_pseudo_bytes(long npts, int k, int Cmax)
{
    const int kq = k <= RG_PB ? 0 : gpe_edge_pseudo_kq(k);
    if (!kq) return 0;
    const size_t nps = (size_t)npts * (k / kq), ld = (size_t)((Cmax + 3) & ~3);
    // forward with aggregation: mx, mn (floats) + amx, amn (bytes); gathered backward: dP (floats) — the larger of the two
    return nps * ld * (2 * sizeof(float) + 2) + 256;
}

// Re-tiles a k > 16 launch: rows that need nothing per point can be tiled any way (4 rows per "point": 64-row tiles); the per-point
// variants write one max / min / argmax / argmin row, or one dP row, per PSEUDO-point into the workspace, folded afterwards
// (gpe_edge_pseudo_fold).  False when the shape cannot run that way (no divisor, no workspace).
static bool edge_pseudo_setup(RgParams& p, bool per_point, int emode, GpeFold& fd)
{
    fd = GpeFold{};
    fd.f = 1;
    if (p.k <= RG_PB) return true;
    if (!per_point) { p.k = 4; return true; }
    const long npts = p.M / p.k;
    const int kq = gpe_edge_pseudo_kq(p.k);
    if (!kq || npts * (p.k / kq) >= (1L << 31) || (p.oldagg & 3) || (p.lddp & 3)) return false;
    fd.f = p.k / kq; fd.kq = kq; fd.npts = npts;
    const long nps = npts * fd.f;                                     // pseudo-points
    const bool want_agg = emode == E_EDGE_FWD && p.agg, want_dp = emode == E_BWD_GATHER;
    const size_t agg_f = want_agg ? (size_t)nps * p.oldagg : 0, dp_f = want_dp ? (size_t)nps * p.lddp : 0;
    const size_t bytes = (2 * agg_f + dp_f) * sizeof(float) + 2 * agg_f + 256;
    char* ws = (bytes > 256 && bytes <= p.ws.pseudo_bytes) ? p.ws.pseudo : nullptr;
    if (bytes > 256 && !ws) return false;                             // no workspace: the producer/consumer kernel runs it
    if (want_agg) {
        fd.mx = p.mx; fd.mn = p.mn; fd.amx = p.oamx; fd.amn = p.oamn;
        p.mx = (float*)ws; p.mn = p.mx + agg_f;
        p.oamx = (uint8_t*)(p.mn + agg_f); p.oamn = p.oamx + agg_f;
    }
    if (want_dp) { fd.dp = p.dP; p.dP = (float*)ws; }
    p.k = kq;
    p.pmagic = (unsigned)(((1ull << 32) + fd.f - 1) / fd.f);          // x / f == umulhi(x, pmagic) for x < 2^31 / f
    return true;
}

bool gpe_edge_retile(const RgParams& p_in, int amode, int emode, int stats_nblk, RgParams& p, GpeFold& fold)
{
    p = p_in;
    const bool per_point = amode == A_GATHER || emode == E_BWD_GATHER || (emode == E_EDGE_FWD && p.agg);
    if (!edge_pseudo_setup(p, per_point, emode, fold)) return false;
    const int npw = RG_PB / p.k;                         // points per wave per tile
    if (per_point && npw > RG_NPW) return false;
    p.R = 4 * npw * p.k;
    p.num_tiles = gpe_cdiv(p.M, p.R);
    p.pin_tpc = 0;
    if ((amode == A_GATHER || emode == E_BWD_GATHER) && p.pin_clouds > 0 && gpe_pin_clouds(p.pin_clouds) &&
        p.pin_clouds % GPE_NXCD == 0) {
        // gather variants only (dense streaming tiles have nothing to keep in L2): tiles must not straddle clouds and
        // the launcher must keep gridDim.x a multiple of 8 with gridDim.x / 8 <= tiles per cloud
        const long rows_per_cloud = p.M / p.pin_clouds;
        const int gx = gpe_num_cus();
        if (rows_per_cloud % p.R == 0 && gx % GPE_NXCD == 0 && gx <= p.num_tiles &&
            (stats_nblk <= 0 || gx <= stats_nblk) && rows_per_cloud / p.R >= gx / GPE_NXCD)
            p.pin_tpc = (int)(rows_per_cloud / p.R);
    }
    return true;
}

int gpe_edge_finish(int rc, const RgParams& p, const GpeFold& fold, hipStream_t s)
{
    if (rc != GPE_EDGE_LAUNCHED) return rc;
    rc = gpe_edge_pseudo_fold(p, fold, s);
    return rc == GPE_OK ? GPE_EDGE_LAUNCHED : rc;
}

// The register-stationary fast path of the edge entry points (gpe_rowgemm.hip): launches and returns 1 when a family has the shape
// on its menu, 0 when the caller should use the generic LDS-streamed kernel (rg_dispatch_nt), < 0 on an error.  Read top to bottom:
// the families in the order they are tried, each behind the conditions of its own.
int gpe_edgegemm_try(const RgParams& p, int amode, int emode, int stats_nblk, hipStream_t s)
{
    // (r02: a "forward-only bf16x3" mode was measured and dropped — 1785 garments/s, but first-layer weight gradients are
    // residuals of cancelling sums that amplify ANY 1e-5 perturbation of the stored activations ~1e3 times (1.5e-2 of
    // max|grad|): nothing short of ~24-bit operands is parity-grade, forward or backward.)
    const int math = gpe_math_rowgemm();                 // 0: exact fp32 MFMA, 1: bf16x3, 2: bf16x6 where it fits, 3: f16x3
    // fp16 activation rows / a lazily formed dz3 exist only in the f16x3 kernels: no other kernel may touch such buffers
    const bool f16_only = p.out_half || p.lz_g;
    if (!gpe_edge_on_menu(p, amode, emode)) return f16_only ? GPE_EINVAL : GPE_EDGE_NOT_MINE;
    const int NT = gpe_edge_chunks(p.N), KCH = gpe_edge_chunks(p.K);

    // the single-role families (math 0, 2, 3) work on a re-tiled copy: whole points per wave
    RgParams t;
    GpeFold fold;
    const bool tiled = math != 1 && p.k >= 1 && gpe_edge_retile(p, amode, emode, stats_nblk, t, fold);
    int rc;

    if (math == 2 && tiled) {                            // bf16x6: three-term split-bf16 single-role kernel where it fits
        rc = gpe_edge_finish(gpe_edge_bf16x6(t, amode, emode, NT, KCH, stats_nblk, s), t, fold, s);
        if (rc != GPE_EDGE_NOT_MINE) return rc;
    }
    // f16x3: two-term split-fp16.  Needs the scale words of the caller's workspace; below gpe_h3_min_rows() rows the scale passes
    // cost more than the kernels save; the in-call bound of a gathered operand reads the [P|Q] table in quads
    if (math == 3 && tiled && p.ws.h3 && p.M >= gpe_h3_min_rows() && !(amode == A_GATHER && !p.user_amax_a && (p.H & 3))) {
        RgParams q = t;
        rc = gpe_edge_f16x3_scales(q, p.M / p.k, amode, emode, KCH, s);
        if (rc != GPE_OK) return rc;
        rc = gpe_edge_w8(q, amode, emode, NT, KCH, stats_nblk, s);              // two waves per SIMD: k = 16 / 5 / 4 by GPE_W8
        if (rc == GPE_EDGE_NOT_MINE) rc = gpe_edge_f16x3(q, amode, emode, NT, KCH, stats_nblk, s);   // single-role, any k
        rc = gpe_edge_finish(rc, q, fold, s);
        // these kernels leave the largest magnitude they wrote to `out` (forward activations, in-place dz) in the caller's word
        if (rc == GPE_EDGE_LAUNCHED && q.amax_out && p.tracked) *p.tracked = 1;
        if (rc != GPE_EDGE_NOT_MINE) return rc;
    }
    if (f16_only) return GPE_EINVAL;

    if (math != 1 && tiled && !(p.dbg & 64)) {           // exact fp32: the single-role software-pipelined kernel
        rc = gpe_edge_finish(gpe_edge_sr(t, amode, emode, NT, KCH, stats_nblk, s), t, fold, s);
        if (rc != GPE_EDGE_NOT_MINE) return rc;
    }
    if (p.R <= 64 && p.k <= 64)                          // producer/consumer: fp32, or bf16x3 in the mixed mode
        return gpe_edge_pc(p, amode, emode, NT, KCH, math == 1, stats_nblk, s);
    return GPE_EDGE_NOT_MINE;
}
