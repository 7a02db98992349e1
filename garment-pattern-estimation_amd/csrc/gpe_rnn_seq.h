// Stack description and selection layer of the recurrence kernels (gpe_rnn_seq_fwd / gpe_rnn_seq_bwd): host code only.  What the
// three kernel families share on the host lives here ONCE; gpe_rnn_seq.hip states which family is tried in which order (DESIGN.md
// 5.28).  The families fill their kernel's parameter struct from the description and launch:
//   persistent, K split over the waves   gpe_rnn_persist.hip      LSTM, <= 256 units, one row tile per workgroup; both directions
//   persistent, waves own row tiles      gpe_rnn_persist_mt.hip   the same with many row tiles; forward, fp16 pipe only
//   one or two launches per diagonal     gpe_rnn_wave.hip         every stack
#pragma once
#include "gpe_common.h"
#include <type_traits>

// one result convention for every family entry point (that of gpe_edge_dispatch.h): launched, not mine (the caller tries the next
// family), or an error code < 0
#define GPE_RNN_LAUNCHED 1
#define GPE_RNN_NOT_MINE 0
#define WV_MAXCELL 4              // cells of one diagonal launch

// ---- what both directions know of a stack (F: float forward, const float backward).  hs: slot 0 = the start state, slot t + 1 =
// h_t; cs likewise; saved: the activated gates of every cell
template <class F> struct GpeRnnStack {
    int G, L, T, Bn, H;                      // G: 4 LSTM (i,f,g,o), 3 GRU (r,z,n)
    F* hs; long hs_sl, hs_sb, hs_st;
    F* cs; long cs_sl, cs_st;
    F* saved; long sv_sl, sv_st;
    hipStream_t s;
    F* h(int l, int slot) const { return hs + l * hs_sl + (long)slot * hs_st; }
    F* c(int l, int slot) const { return cs + l * cs_sl + (long)slot * cs_st; }
    F* gates(int l, int t) const { return saved + l * sv_sl + (long)t * sv_st; }
};
// ---- the stack as gpe_rnn_seq_fwd received it.  whh / wih / whh_amax / wih_amax are the per-layer operand tables IN USE (host
// arrays [L] of device pointers): f16 — the fp16 plane packs (gpe_pack_multi kinds 9 + 8) and their amax words; else the
// gate-interleaved fp32 packs and no amax tables
struct GpeRnnSeq : GpeRnnStack<float> {
    const float* xproj0; long xp0_sb, xp0_st;
    const void* const* whh; const void* const* wih; const void* const* whh_amax; const void* const* wih_amax;
    const void* const* bias; const void* const* bhn;
    bool f16;
    void* ws; long ws_bytes;                 // gpe_rnn_seq_fwd_ws bytes (the persistent families)
};
// ---- ... and gpe_rnn_seq_bwd.  whh_t / wih_t: the plain TRANSPOSED packs (the diagonal launches); f16: whh_tpl / wih_tpl are the
// transposed plane packs (gpe_pack_multi kind 10) with the amax words (the persistent launch).  dgx / dgh: [L][Bn][T][G*H]
struct GpeRnnSeqBwd : GpeRnnStack<const float> {
    const float* dtop; long dt_sb, dt_st;
    const float* d_hN; const float* d_cN;
    const void* const* whh_t; const void* const* wih_t;
    const void* const* whh_tpl; const void* const* wih_tpl; const void* const* whh_amax; const void* const* wih_amax;
    bool f16;
    float* dgx; float* dgh; long dg_sl, dg_sb, dg_st;
    float* part; float* carry;               // gpe_rnn_seq_bwd_ws floats; [2][L][Bn][H]
    float* dx(int l, int t) const { return dgx + l * dg_sl + (long)t * dg_st; }
    float* dh(int l, int t) const { return dgh + l * dg_sl + (long)t * dg_st; }
    float* carry_at(int t, int l) const { return carry + ((long)(t & 1) * L + l) * Bn * H; }
};

// does the caller supply the plane pack and the amax word of every weight of the stack?  (Layer 0 has no input-side weight.)
static inline bool gpe_rnn_f16_tables(int L, const void* const* whh_pl, const void* const* wih_pl, const void* const* whh_amax,
                                      const void* const* wih_amax)
{
    if (!whh_pl || !whh_amax || (L > 1 && (!wih_pl || !wih_amax))) return false;
    for (int l = 0; l < L; ++l)
        if (!whh_pl[l] || !whh_amax[l] || (l > 0 && (!wih_pl[l] || !wih_amax[l]))) return false;
    return true;
}

// ---- the persistent families.  Workgroup (layer, row group, unit block): NB blocks of 16 units, NRT tiles of 16 rows, RG row
// groups of `per` workgroups each.  What both plans start with: an LSTM of at most `maxl` layers and 256 units, none of the
// gpe_debug_set bits `off_bits`, one row group on the usable CUs; rgmax = the row groups the chip holds (at most NRT).  The family
// settles RG and grid = per * RG by its own policy
struct GpeRnnPlan { int NB, NRT, per, rgmax, RG, KP, grid; };
static inline bool gpe_rnn_plan_begin(int gates, int L, int maxl, int T, int Bn, int H, int off_bits, GpeRnnPlan& pl)
{
    if (gates != 4 || L < 1 || L > maxl || T < 1 || Bn < 1 || H < 1 || H > 256 || (gpe_debug_get() & off_bits)) return false;
    pl.NB = gpe_cdiv(H, 16);
    pl.NRT = gpe_cdiv(Bn, 16);
    const int cus = gpe_num_cus();
    pl.per = L * pl.NB;
    if (cus <= 0 || pl.per > cus) return false;
    pl.rgmax = cus / pl.per < pl.NRT ? cus / pl.per : pl.NRT;
    return true;
}
// their workspace in bytes: arrival counters | published state planes | trace (gpe_debug_set 8192).  Each family fills it in ONE
// function (ps_ws_layout, pm_ws_layout) that its *_ws_bytes query and its launch both use
struct GpeRnnWs {
    long flags, planes, trace;
    long total() const { return flags + planes + trace; }
    bool fits(const void* ws, long bytes, int align) const { return ws && bytes >= total() && !(((uintptr_t)ws) & (align - 1)); }
    char* planes_at(void* ws) const { return (char*)ws + flags; }
    unsigned long long* trace_at(void* ws) const { return trace ? (unsigned long long*)((char*)ws + flags + planes) : nullptr; }
};
// per-layer operand tables -> the w0 / w1 / s0 / s1 (/ bias) arrays of a persistent kernel's parameter struct.  Layer l's first
// operand is t0[l]; its second is t1[m], m = l + up, for 1 <= m < L (forward, up = 0: W_ih_l; backward, up = 1: W_ih_{l+1}^T).
// Every pack must be there and 16-byte aligned; f16: every amax word too; with `bias_out`, the bias row of layer m.  False: not a
// stack for a persistent kernel
template <class P>
static inline bool gpe_rnn_fill_tables(P& p, int L, int up, const void* const* t0, const void* const* t1, const void* const* a0,
                                       const void* const* a1, bool f16, const void* const* bias = nullptr,
                                       const float** bias_out = nullptr)
{
    auto pack_ok = [](const void* w) { return w && !(((uintptr_t)w) & 15); };
    for (int l = 0, m = up; l < L; ++l, ++m) {
        if (!pack_ok(t0[l]) || (f16 && !a0[l])) return false;
        p.w0[l] = t0[l];
        if (f16) p.s0[l] = (const unsigned*)a0[l];
        if (m < 1 || m >= L) continue;
        if (!pack_ok(t1[m]) || (f16 && !a1[m]) || (bias_out && !bias[m])) return false;
        p.w1[l] = t1[m];
        if (f16) p.s1[l] = (const unsigned*)a1[m];
        if (bias_out) bias_out[l] = (const float*)bias[m];
    }
    return true;
}

// the fields of a persistent FORWARD kernel's parameter struct that come from the description and the plan
template <class P> static inline bool gpe_rnn_fill_fwd(P& p, const GpeRnnSeq& q, const GpeRnnPlan& pl)
{
    p.L = q.L; p.T = q.T; p.Bn = q.Bn; p.H = q.H; p.NB = pl.NB; p.RG = pl.RG; p.NRT = pl.NRT;
    p.xproj0 = q.xproj0; p.xp0_sb = q.xp0_sb; p.xp0_st = q.xp0_st;
    p.hs = q.hs; p.hs_sl = q.hs_sl; p.hs_sb = q.hs_sb; p.hs_st = q.hs_st;
    p.cs = q.cs; p.cs_sl = q.cs_sl; p.cs_st = q.cs_st;
    p.saved = q.saved; p.sv_sl = q.sv_sl; p.sv_st = q.sv_st;
    return gpe_rnn_fill_tables(p, q.L, 0, q.whh, q.wih, q.whh_amax, q.wih_amax, q.f16, q.bias, p.bias);
}

// ---- the numbers of a launch, as a family's PLAN STEP settles them (the checks, the plan, the LDS image) before its launch step
// runs; gpe_rnn_seq_fwd_path / gpe_rnn_seq_bwd_path (gpe_rnn_seq.hip) export them in this order.  A field a family does not have is 0
struct GpeRnnPath {
    long f16, NB, NRT, per, rgmax, RG, KP, grid, lds;      // grid: workgroups of the (largest) launch
    long ws_used;                                          // forward: bytes behind ws, backward: floats behind part the launch touches
    long ks, split, jslabs, nz, fuse, Hp, groups;          // the diagonals: K slab width, <= 32-row split mode, ..., most groups per diagonal
    void persistent(const GpeRnnPlan& pl, bool h3, int kp, size_t lds_bytes, long used)
    {
        f16 = h3; NB = pl.NB; NRT = pl.NRT; per = pl.per; rgmax = pl.rgmax; RG = pl.RG; KP = kp; grid = pl.grid; lds = (long)lds_bytes;
        ws_used = used;
    }
};
#define GPE_RNN_PATH_LEN 17

// ---- the families.  With `plan_only` a family runs its plan step alone: it answers as it would, fills *plan_only and launches nothing
long gpe_rnn_persist_ws_bytes(int gates, int L, int T, int Bn, int H, int bwd);      // 0: this stack does not run there
int gpe_rnn_persist_fwd(const GpeRnnSeq& q, GpeRnnPath* plan_only = nullptr);
int gpe_rnn_persist_bwd(const GpeRnnSeqBwd& q, GpeRnnPath* plan_only = nullptr);     // its workspace is q.part
long gpe_rnn_pm_ws_bytes(int gates, int L, int T, int Bn, int H, int bwd);
int gpe_rnn_pm_fwd(const GpeRnnSeq& q, GpeRnnPath* plan_only = nullptr);
long gpe_rnn_wave_bwd_ws_floats(int gates, int L, int T, int Bn, int H);
int gpe_rnn_wave_fwd(const GpeRnnSeq& q, GpeRnnPath* plan_only = nullptr);
int gpe_rnn_wave_bwd(const GpeRnnSeqBwd& q, GpeRnnPath* plan_only = nullptr);

// ---- the diagonal walk: cell (l, t) needs (l, t - 1) and (l - 1, t), so the cells of anti-diagonal d = l + t are independent.
// Calls f(d, l0, l_top) for every group of at most WV_MAXCELL cells l0 <= l <= l_top, t = d - l, diagonals ascending (forward) or
// descending (backward); f answers like a launch, an error ends the walk
template <class F> static inline int gpe_rnn_walk_diagonals(int L, int T, bool descending, F&& f)
{
    for (int i = 0; i < T + L - 1; ++i) {
        const int d = descending ? T + L - 2 - i : i;
        const int l_lo = (d - (T - 1) > 0) ? d - (T - 1) : 0;
        const int l_hi = (d < L - 1) ? d : L - 1;
        for (int l0 = l_lo; l0 <= l_hi; l0 += WV_MAXCELL) {
            const int rc = f(d, l0, (l_hi < l0 + WV_MAXCELL - 1) ? l_hi : l0 + WV_MAXCELL - 1);
            if (rc < 0) return rc;
        }
    }
    return GPE_RNN_LAUNCHED;
}

// ---- the launch tail.  Run-time bool / K slab width -> a compile-time constant; then the max-LDS attribute once per kernel
// instantiation and device (LDS_CAP 0: no dynamic LDS), launch, check.  LDS_CAP: 160 KB, less 64 bytes beside static __shared__
template <class F> static inline int gpe_rnn_for_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <class F> static inline int gpe_rnn_for_ks(int ks, F&& f)
{
    return ks == 256 ? f(std::integral_constant<int, 256>{}) : f(std::integral_constant<int, 128>{});
}
#define GPE_RNN_LDS_CAP (160 * 1024)
#define GPE_RNN_LDS_CAP_STATIC (160 * 1024 - 64)
template <auto KERNEL, int LDS_CAP, class P> static int gpe_rnn_launch(dim3 grid, int block, size_t lds, hipStream_t s, const P& p)
{
    if constexpr (LDS_CAP > 0) GPE_ENSURE_MAX_LDS_N(KERNEL, LDS_CAP);
    hipLaunchKernelGGL(KERNEL, grid, dim3(block), lds, s, p);
    GPE_CHECK_LAUNCH();
    return GPE_RNN_LAUNCHED;
}
