// Which recurrence kernel runs a stack of L layers over T steps: the two C entry points of the recurrent stacks and their workspace
// queries.  Host code only, no kernel; the pieces are declared in gpe_rnn_seq.h.  Each entry point reads top to bottom: validate,
// describe the stack, then the families in the order they are tried — a family answers launched, not mine or an error
// (DESIGN.md 5.28).
#include "gpe_rnn_seq.h"
#include <vector>

static bool seq_dims_ok(int gates, int L, int T, int Bn, int H) { return (gates == 3 || gates == 4) && L > 0 && T > 0 && Bn > 0 && H > 0; }
// the last family takes every stack: "not mine" from it would be a mistake of this file
static int seq_result(int rc) { return rc == GPE_RNN_LAUNCHED ? GPE_OK : (rc < 0 ? rc : GPE_EINVAL); }

// bytes of the persistent families' workspace (0: the diagonal launches run, they need none)
extern "C" long gpe_rnn_seq_fwd_ws(int gates, int L, int T, int Bn, int H)
{
    if (!seq_dims_ok(gates, L, T, Bn, H)) return GPE_EINVAL;
    const long a = gpe_rnn_persist_ws_bytes(gates, L, T, Bn, H, 0), b = gpe_rnn_pm_ws_bytes(gates, L, T, Bn, H, 0);
    return a > b ? a : b;
}

// FLOATS of `part`: the diagonal launches' partial images and counters, or the arrival counters of the persistent kernel
extern "C" long gpe_rnn_seq_bwd_ws(int gates, int L, int T, int Bn, int H)
{
    if (!seq_dims_ok(gates, L, T, Bn, H)) return GPE_EINVAL;
    const long diag = gpe_rnn_wave_bwd_ws_floats(gates, L, T, Bn, H);
    const long pers = gpe_rnn_persist_ws_bytes(gates, L, T, Bn, H, 1) / 4;
    return diag > pers ? diag : pers;
}

// ---- the two ladders, ONCE: the entry points launch through them, the path queries ask them with `plan` (nothing is launched).
// family: 1 K-split persistent, 2 multi-tile persistent, 3 diagonal launches
static int seq_fwd_ladder(const GpeRnnSeq& q, GpeRnnPath* plan, int& family)
{
    family = 1;
    int rc = gpe_rnn_persist_fwd(q, plan);                                    // one persistent launch for the whole stack when it fits the chip
    if (rc == GPE_RNN_NOT_MINE) { family = 2; rc = gpe_rnn_pm_fwd(q, plan); }   // the same with several row tiles per workgroup (fp16 pipe only)
    if (rc == GPE_RNN_NOT_MINE) { family = 3; rc = gpe_rnn_wave_fwd(q, plan); } // one launch per diagonal
    return seq_result(rc);
}
static int seq_bwd_ladder(const GpeRnnSeqBwd& q, GpeRnnPath* plan, int& family)
{
    family = 1;
    int rc = gpe_rnn_persist_bwd(q, plan);                                    // one persistent launch for the whole stack when it fits the chip
    if (rc == GPE_RNN_NOT_MINE) { family = 3; rc = gpe_rnn_wave_bwd(q, plan); } // two launches per diagonal
    return seq_result(rc);
}

// validate and describe a forward call (GPE_OK: q is the stack).  f16x3: the gate products on the fp16 pipe when the arithmetic mode
// asks for it and the caller supplies the plane packs and amax words of every weight (gpe_pack_multi kinds 9 + 8); else the exact
// fp32 instruction
static int seq_fwd_describe(int gates, int L, int T, int Bn, int H, const float* xproj0, long xp0_sb, long xp0_st,
                            const void* const* whh, const void* const* wih, const void* const* bias, const void* const* bhn, float* hs,
                            long hs_sl, long hs_sb, long hs_st, float* cs, long cs_sl, long cs_st, float* saved, long sv_sl, long sv_st,
                            const void* const* whh_pl, const void* const* wih_pl, const void* const* whh_amax,
                            const void* const* wih_amax, void* ws, long ws_bytes, void* stream, GpeRnnSeq& q)
{
    if (!seq_dims_ok(gates, L, T, Bn, H) || !xproj0 || !whh || !hs || !saved || (L > 1 && (!wih || !bias)) || (gates == 4 && !cs) ||
        (gates == 3 && !bhn) || (hs_sb & 3) || (hs_st & 3))
        return GPE_EINVAL;
    static const int dbg_f32 = gpe_dbg_env("GPE_RNN_F32", 0);        // A/B measurements: keep the exact kernels
    const bool f16 = !dbg_f32 && gpe_math_get() == 4 && gpe_rnn_f16_tables(L, whh_pl, wih_pl, whh_amax, wih_amax);
    q = {{gates, L, T, Bn, H, hs, hs_sl, hs_sb, hs_st, cs, cs_sl, cs_st, saved, sv_sl, sv_st, (hipStream_t)stream},
         xproj0, xp0_sb, xp0_st, f16 ? whh_pl : whh, f16 ? wih_pl : wih, f16 ? whh_amax : nullptr,
         f16 ? wih_amax : nullptr, bias, bhn, f16, ws, ws_bytes};
    return GPE_OK;
}
// ... and a backward call.  f16x3 (the persistent launch only): the transposed plane packs (gpe_pack_multi kind 10) and amax words
// of every weight
static int seq_bwd_describe(int gates, int L, int T, int Bn, int H, const float* dtop, long dt_sb, long dt_st, const float* d_hN,
                            const float* d_cN, const void* const* whh_t, const void* const* wih_t, const float* hs, long hs_sl,
                            long hs_sb, long hs_st, const float* cs, long cs_sl, long cs_st, const float* saved, long sv_sl, long sv_st,
                            float* dgx, float* dgh, long dg_sl, long dg_sb, long dg_st, float* part, float* carry,
                            const void* const* whh_tpl, const void* const* wih_tpl, const void* const* whh_amax,
                            const void* const* wih_amax, void* stream, GpeRnnSeqBwd& q)
{
    if (!seq_dims_ok(gates, L, T, Bn, H) || !whh_t || !hs || !saved || !dgx || !dgh || !part || !carry || (L > 1 && !wih_t) ||
        (gates == 4 && !cs) || (dg_sb & 3) || (dg_st & 3))
        return GPE_EINVAL;
    const bool f16 = gpe_math_get() == 4 && gpe_rnn_f16_tables(L, whh_tpl, wih_tpl, whh_amax, wih_amax);
    q = {{gates, L, T, Bn, H, hs, hs_sl, hs_sb, hs_st, cs, cs_sl, cs_st, saved, sv_sl, sv_st, (hipStream_t)stream},
         dtop, dt_sb, dt_st, d_hN, d_cN, whh_t, wih_t, whh_tpl, wih_tpl, whh_amax, wih_amax, f16,
         dgx, dgh, dg_sl, dg_sb, dg_st, part, carry};
    return GPE_OK;
}

// whh / wih / bias / bhn (and the _pl / _amax tables): host arrays [L] of device pointers; entry 0 of wih / bias is unused
extern "C" int gpe_rnn_seq_fwd(int gates, int L, int T, int Bn, int H, const float* xproj0, long xp0_sb, long xp0_st,
                               const void* const* whh, const void* const* wih, const void* const* bias,
                               const void* const* bhn, float* hs, long hs_sl, long hs_sb, long hs_st, float* cs, long cs_sl, long cs_st,
                               float* saved, long sv_sl, long sv_st, const void* const* whh_pl, const void* const* wih_pl,
                               const void* const* whh_amax, const void* const* wih_amax, void* ws, long ws_bytes, void* stream)
{
    GpeRnnSeq q;
    int family;
    const int rc = seq_fwd_describe(gates, L, T, Bn, H, xproj0, xp0_sb, xp0_st, whh, wih, bias, bhn, hs, hs_sl, hs_sb, hs_st, cs, cs_sl,
                                    cs_st, saved, sv_sl, sv_st, whh_pl, wih_pl, whh_amax, wih_amax, ws, ws_bytes, stream, q);
    return rc != GPE_OK ? rc : seq_fwd_ladder(q, nullptr, family);
}

// dgx / dgh: [L][Bn][T][G*H] (for LSTM pass the same buffer twice); carry: [2][L][Bn][H] scratch; part: gpe_rnn_seq_bwd_ws floats;
// whh_t / wih_t: host arrays [L] of device pointers to the plain TRANSPOSED packs (gpe_pack_weight(.., transpose = 1));
// d_hN / d_cN: gradients of the final states [L][Bn][H] or NULL.  On return carry[0] holds dc_0 / the z-gated dh_0 of every layer.
extern "C" int gpe_rnn_seq_bwd(int gates, int L, int T, int Bn, int H, const float* dtop, long dt_sb, long dt_st,
                               const float* d_hN, const float* d_cN, const void* const* whh_t, const void* const* wih_t,
                               const float* hs, long hs_sl, long hs_sb, long hs_st, const float* cs, long cs_sl, long cs_st,
                               const float* saved, long sv_sl, long sv_st, float* dgx, float* dgh, long dg_sl, long dg_sb,
                               long dg_st, float* part, float* carry, const void* const* whh_tpl, const void* const* wih_tpl,
                               const void* const* whh_amax, const void* const* wih_amax, void* stream)
{
    GpeRnnSeqBwd q;
    int family;
    const int rc = seq_bwd_describe(gates, L, T, Bn, H, dtop, dt_sb, dt_st, d_hN, d_cN, whh_t, wih_t, hs, hs_sl, hs_sb, hs_st, cs, cs_sl,
                                    cs_st, saved, sv_sl, sv_st, dgx, dgh, dg_sl, dg_sb, dg_st, part, carry, whh_tpl, wih_tpl, whh_amax,
                                    wih_amax, stream, q);
    return rc != GPE_OK ? rc : seq_bwd_ladder(q, nullptr, family);
}

// ---- which family a call would run, and the numbers of its launch (include/gpe_hip.h).  HOST ONLY: the call is described to the
// SAME describe and ladder functions with stand-in operand tables — a pointer VALUE per table entry that shows what the families look
// at (NULL, 16-byte alignment) — and the families run their plan steps alone.  packs / planes: the alignment in bytes a pack of the
// stack has at worst (16: fine, 8: one is misaligned, 0: one is missing; planes 0: the plane / amax tables are incomplete)
static void seq_path_out(const GpeRnnPath& p, long* out)
{
    const long v[GPE_RNN_PATH_LEN] = {p.f16, p.NB, p.NRT, p.per, p.rgmax, p.RG, p.KP, p.grid, p.lds, p.ws_used, p.ks, p.split, p.jslabs,
                                      p.nz, p.fuse, p.Hp, p.groups};
    for (int i = 0; i < GPE_RNN_PATH_LEN; ++i) out[i] = v[i];
}
struct SeqStandIn {
    std::vector<const void*> pack, plane, amax, row;
    SeqStandIn(int L, int packs, int planes, int rows)
        : pack(L, (const void*)(uintptr_t)packs), plane(L, (const void*)(uintptr_t)planes),
          amax(L, (const void*)(uintptr_t)(planes ? 4 : 0)), row(L, (const void*)(uintptr_t)(rows ? 4 : 0)) {}
};

extern "C" int gpe_rnn_seq_fwd_path(int gates, int L, int T, int Bn, int H, const float* hs, long hs_sl, long hs_sb, long hs_st,
                                    int packs, int planes, int bias_rows, const void* ws, long ws_bytes, long* plan_out)
{
    if (L < 1 || L > (1 << 20) || packs < 0 || planes < 0) return GPE_EINVAL;
    const SeqStandIn t(L, packs, planes, bias_rows);
    float* const there = (float*)(uintptr_t)16;                               // xproj0, cs, saved: present; never looked at further
    GpeRnnSeq q;
    int family;
    int rc = seq_fwd_describe(gates, L, T, Bn, H, there, 0, 0, t.pack.data(), t.pack.data(), t.row.data(), t.row.data(), (float*)hs,
                              hs_sl, hs_sb, hs_st, there, 0, 0, there, 0, 0, t.plane.data(), t.plane.data(), t.amax.data(),
                              t.amax.data(), (void*)ws, ws_bytes, nullptr, q);
    if (rc != GPE_OK) return rc;
    GpeRnnPath p = {};
    rc = seq_fwd_ladder(q, &p, family);
    if (rc != GPE_OK) return rc;
    if (plan_out) seq_path_out(p, plan_out);
    return family;
}

extern "C" int gpe_rnn_seq_bwd_path(int gates, int L, int T, int Bn, int H, const float* dgx, long dg_sl, long dg_sb, long dg_st,
                                    const float* part, int packs, int planes, long* plan_out)
{
    if (L < 1 || L > (1 << 20) || packs < 0 || planes < 0) return GPE_EINVAL;
    const SeqStandIn t(L, packs, planes, 0);
    float* const there = (float*)(uintptr_t)16;
    GpeRnnSeqBwd q;
    int family;
    int rc = seq_bwd_describe(gates, L, T, Bn, H, nullptr, 0, 0, nullptr, nullptr, t.pack.data(), t.pack.data(), there, 0, 0, 0,
                              there, 0, 0, there, 0, 0, (float*)dgx, (float*)dgx, dg_sl, dg_sb, dg_st, (float*)part, there,
                              t.plane.data(), t.plane.data(), t.amax.data(), t.amax.data(), nullptr, q);
    if (rc != GPE_OK) return rc;
    GpeRnnPath p = {};
    rc = seq_bwd_ladder(q, &p, family);
    if (rc != GPE_OK) return rc;
    if (plan_out) seq_path_out(p, plan_out);
    return family;
}
