// Selection and launch layer of the fused edge GEMM kernels (gpe_edge_mlp_fwd / gpe_edge_mlp_bwd): host code only.  Everything the
// five kernel families share on the host lives here ONCE — the menu test, the re-tiling, the chunk count, the kind index, the
// (amode, emode) and (NT, KCH) ladders and the launch tail — and gpe_edgegemm_try (gpe_edge_dispatch.hip) states which family
// is tried in which order for each arithmetic mode.  The families only instantiate and launch:
//   producer/consumer          gpe_edgegemm.hip                          gpe_edge_pc
//   single-role exact          gpe_edgegemm_sr.hip / _sr_dense.hip       gpe_edge_sr
//   split bf16x6               gpe_edgegemm_x6.hip                       gpe_edge_bf16x6
//   split f16x3                gpe_edgegemm_h3.hip                       gpe_edge_f16x3 (behind gpe_edge_f16x3_scales)
//   two waves per SIMD f16x3   gpe_edgegemm_w8.hip / _f3 / _b3 / _k5 / _k4   gpe_edge_w8
#pragma once
#include "gpe_rowgemm.h"

// ---- one result convention for every function of this layer: launched, not on my menu (the caller tries the next family), or
// an error code < 0 (GPE_EINVAL: the caller asked for something no instance serves; GPE_ELAUNCH)
#define GPE_EDGE_LAUNCHED 1
#define GPE_EDGE_NOT_MINE 0

// ---- the register-stationary fast path of the edge entry points (gpe_rowgemm.hip) for the shipped edge-MLP sizes: launched, or
// not on any family's menu (the caller runs the generic LDS-streamed kernel), or an error
int gpe_edgegemm_try(const RgParams& p, int amode, int emode, int stats_nblk, hipStream_t s);

// ---- the register-stationary menu -------------------------------------------------------------------------------------------
// widths (96, 208]: 10 or 13 tiles of 16 columns / chunks of 16 k
static inline bool gpe_edge_width_ok(int c) { return c > 96 && c <= 208; }
static inline int gpe_edge_chunks(int c) { return c <= 160 ? 10 : 13; }
// kind of an edge launch: F2 gather forward, F3 dense forward, B3 in-place backward, B2 gathered backward (the digits of GPE_W8 and
// GPE_H3_LEFT, in this order)
enum { GPE_EDGE_F2 = 0, GPE_EDGE_F3 = 1, GPE_EDGE_B3 = 2, GPE_EDGE_B2 = 3 };
constexpr int gpe_edge_kind(int amode, int emode)
{
    return emode == E_EDGE_FWD ? (amode == A_GATHER ? GPE_EDGE_F2 : GPE_EDGE_F3) : (emode == E_BWD_INPLACE ? GPE_EDGE_B3 : GPE_EDGE_B2);
}
// is this launch on the menu of the register-stationary families?  (Their own extra conditions stand in gpe_edgegemm_try.)
static inline bool gpe_edge_on_menu(const RgParams& p, int amode, int emode)
{
    if (!gpe_edge_width_ok(p.N) || !gpe_edge_width_ok(p.K)) return false;
    if (emode != E_EDGE_FWD && (p.N & 3)) return false;  // the backward epilogues use aligned 16-B coefficient loads
    if (amode == A_GATHER && (p.K & 3)) return false;
    // dense rows must be aligned + padded for plain 16-B loads
    return !(amode == A_DENSE && (p.a.inner > 0 || (p.a.stride_outer & 3) || p.a.stride_outer < ((p.K + 3) & ~3) || (((uintptr_t)p.a.base) & 15)));
}

// ---- re-tiling for the single-role families (gpe_edge_dispatch.hip) ----------------------------------------------------------
// rows per (pseudo-)point a k > 16 point is split into (0: no divisor of k fills a wave's 16 rows well enough)
int gpe_edge_pseudo_kq(int k);
size_t gpe_edge_pseudo_bytes(long npts, int k, int Cmax);
// `p_in` comes with the generic tiling (R = (64/k)*k).  Returns false when the shape cannot run on the single-role families; else
// `p` is the re-tiled copy — every wave owns whole points, R = 4 * npw * k with npw * k <= 16, cloud -> XCD pinning decided —
// and `fold` says what gpe_edge_finish folds after the launch when a k > 16 point ran as pseudo-points
bool gpe_edge_retile(const RgParams& p_in, int amode, int emode, int stats_nblk, RgParams& p, GpeFold& fold);
// behind a family's launch of a re-tiled `p`: folds the pseudo-point rows when it launched; passes `rc` through otherwise
int gpe_edge_finish(int rc, const RgParams& p, const GpeFold& fold, hipStream_t s);

// ---- the families: `p` is the re-tiled copy (gpe_edge_pc: the caller's own) ---------------------------------------------------
int gpe_edge_pc(const RgParams& p, int amode, int emode, int NT, int KCH, int bf16x3, int stats_nblk, hipStream_t s);
int gpe_edge_sr(const RgParams& p, int amode, int emode, int NT, int KCH, int stats_nblk, hipStream_t s);
// ... its dense-A variants (gpe_edgegemm_sr_dense.hip: compiled with another scheduling strategy)
int gpe_edge_sr_dense(const RgParams& p, int amode, int emode, int NT, int KCH, int stats_nblk, hipStream_t s);
int gpe_edge_bf16x6(const RgParams& p, int amode, int emode, int NT, int KCH, int stats_nblk, hipStream_t s);
// the scale passes of the f16x3 families: fills p.h3_amax_a / h3_amax_w / amax_out; GPE_OK or an error
int gpe_edge_f16x3_scales(RgParams& p, long npts, int amode, int emode, int KCH, hipStream_t s);
int gpe_edge_f16x3(const RgParams& p, int amode, int emode, int NT, int KCH, int stats_nblk, hipStream_t s);
int gpe_edge_w8(const RgParams& p, int amode, int emode, int NT, int KCH, int stats_nblk, hipStream_t s);

// ---- the two ladders: run-time values -> compile-time constants -----------------------------------------------------------------
template <int A, int E> struct GpeEdgeMode { static constexpr int amode = A, emode = E, kind = gpe_edge_kind(A, E); };
template <int AQ_, int BQ_, int KCH_> struct GpeEdgeTile { static constexpr int AQ = AQ_, BQ = BQ_, KCH = KCH_, NT = 4 * AQ_ + BQ_; };

// the four legal (amode, emode) pairs; any other is the caller's mistake
template <class F> static inline int gpe_edge_for_mode(int amode, int emode, F&& f)
{
    if (amode == A_GATHER && emode == E_EDGE_FWD) return f(GpeEdgeMode<A_GATHER, E_EDGE_FWD>{});
    if (amode == A_DENSE && emode == E_EDGE_FWD) return f(GpeEdgeMode<A_DENSE, E_EDGE_FWD>{});
    if (amode == A_DENSE && emode == E_BWD_INPLACE) return f(GpeEdgeMode<A_DENSE, E_BWD_INPLACE>{});
    if (amode == A_DENSE && emode == E_BWD_GATHER) return f(GpeEdgeMode<A_DENSE, E_BWD_GATHER>{});
    return GPE_EINVAL;
}
// (NT, KCH) -> <AQ, BQ, KCH>: AQ output tiles per wave for all rows + BQ left-over tiles shared by the waves
template <class F> static inline int gpe_edge_for_tile(int NT, int KCH, F&& f)
{
    if (NT == 13 && KCH == 13) return f(GpeEdgeTile<3, 1, 13>{});
    if (NT == 13 && KCH == 10) return f(GpeEdgeTile<3, 1, 10>{});
    if (NT == 10 && KCH == 13) return f(GpeEdgeTile<2, 2, 13>{});
    if (NT == 10 && KCH == 10) return f(GpeEdgeTile<2, 2, 10>{});
    return GPE_EDGE_NOT_MINE;
}
// Both at once for a family whose instances are MENU::has(amode, emode, NT, KCH) (constexpr: nothing else is instantiated):
// f(GpeEdgeMode<..>, GpeEdgeTile<..>) launches
template <class MENU, class F> static inline int gpe_edge_select(int amode, int emode, int NT, int KCH, F&& f)
{
    return gpe_edge_for_mode(amode, emode, [&](auto m) {
        return gpe_edge_for_tile(NT, KCH, [&](auto t) -> int {
            if constexpr (MENU::has(decltype(m)::amode, decltype(m)::emode, decltype(t)::NT, decltype(t)::KCH)) return f(m, t);
            else return GPE_EDGE_NOT_MINE;
        });
    });
}

// ---- the launch tail of every persistent edge kernel: one workgroup per CU, never more than tiles or statistics slots; the
// max-LDS attribute once per kernel instantiation and device.  LDS_CAP: 160 KB, less 64 bytes for kernels with static __shared__
#define GPE_EDGE_LDS_CAP (160 * 1024)
#define GPE_EDGE_LDS_CAP_STATIC (160 * 1024 - 64)
template <auto KERNEL, int BLOCK, int LDS_CAP> static int gpe_edge_launch(const RgParams& p, int stats_nblk, size_t lds, hipStream_t s)
{
    GPE_ENSURE_MAX_LDS_N(KERNEL, LDS_CAP);
    int gx = gpe_num_cus();
    if (gx > p.num_tiles) gx = p.num_tiles;
    if (stats_nblk > 0 && gx > stats_nblk) gx = stats_nblk;
    hipLaunchKernelGGL(KERNEL, dim3(gx), dim3(BLOCK), lds, s, p, stats_nblk);
    GPE_CHECK_LAUNCH();
    return GPE_EDGE_LAUNCHED;
}
