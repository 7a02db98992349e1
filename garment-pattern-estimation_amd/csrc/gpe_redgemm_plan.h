// Which reduce-GEMM kernel runs (gpe_redgemm / gpe_edge_redgemm / gpe_redgemm_ws): host code only.  What the kernel
// files (gpe_redgemm.hip, and gpe_gemm_x6.hip for the bf16-pipe TN kernel) share on the host lives here ONCE:
//   the constants more than one place needs, the measurement switches, the call as received (RdParams), the three "can a 16-byte
//   loader take these rows" predicates, the edge-shape predicate, the layout of the partial image, gpe_redgemm_plan — the whole
//   selection ladder as a pure function —, the settlement of gpe_edge_redgemm's amax words in front of it, and the launchers'
//   declarations.  gpe_redgemm_path (include/gpe_hip.h) gives the plan's answer for a call at the C ABI.
// A launcher decides nothing: it turns the plan's numbers into template arguments, sizes its kernel's LDS beside the kernel,
// launches and checks.  The path, gx and the number of partials decide the fp64 summation order of gpe_redgemm_finish, so they are
// part of the result's bits (tests/test_gpu_grid_sizes.py): a change to this file is a change to those bits.
#pragma once
#include "gpe_common.h"

// ---- constants more than one place needs (a constant only one kernel uses stays beside that kernel) ---------------------------
#define RD_RT 32                          // rows per operand tile (every kernel of gpe_redgemm.hip)
#define RD_MAX_GX 256                     // big-block / producer-consumer / b3 kernels: most workgroups (= partials) along x
#define RDD_B 64                          // deep kernel: output block edge
#define RDD_MAX_GX 32                     // deep kernel: largest row split (= partials)
#define RDD_MAX_TPW 64                    // deep kernel: = the big-block kernel's tiles per workgroup at the switch (num_tiles < 64 gx)
#define RDT_GX 512                        // thin kernel: most workgroups (= partials)
#define RD_FIN_E 32                       // gpe_redgemm_finish: output elements per workgroup ...
#define RD_FIN_Q 8                        // ... and the partials summed side by side per element
#define GX_B 128                          // gpe_gemm_x6.hip: block edge (rows of A / columns of W; columns of U / of V)
#define GX_RED_MAX_S 32                   // TN kernel: largest row split (= partials)

// ---- measurement switches: GPE_RD_<FIELD>, consulted only under GPE_DEBUG=1 (gpe_dbg_env), read once per process --------------
struct GpeRdSwitches {
    int DEEP;       // default -1 = the rule.  0 never the deep kernel (its products go to the big-block kernel).  Not exact: another
                    // kernel, another summation order
    int NOPC;       // default 0.  1 keeps the edge shapes off the producer/consumer and b3 kernels (the big-block kernel runs; a lazy
                    // call is refused).  Not exact, as above
};
const GpeRdSwitches& gpe_rd_switches();                 // this process's (gpe_redgemm.hip)
// Run-time, not a switch of this struct: bit 16384 of gpe_debug_set keeps f16x3 dense products off the TN kernel (the plan takes the
// debug word as an argument); bit 32768 has the TN kernel stamp its step timeline behind the partial image.

// ---- the call as gpe_redgemm / gpe_edge_redgemm received it; also what the kernels of gpe_redgemm.hip take BY VALUE ------------
// (fields and their order are the kernels' argument layout).  The entry points fill the operands; the launch fills vec, pads,
// num_tiles, magics, pin_tpc, part and part_cs from the plan.  The host never sets `rev` here: the reduce-GEMMs walk up.
enum { V_GATHER = 0, V_DENSE = 1 };
struct RdParams {
    long rows;
    int Mg, Ng, MgPad, NgPad;
    int num_tiles;
    GpeRows u;
    GpeRows v;                                   // V_DENSE
    const float* pq; int ldpq; int H; const int32_t* jg; int k; double rcp_k;   // V_GATHER (global neighbour rows)
    unsigned kmagic;                             // ceil(2^32 / k): row / k == umulhi(row, kmagic) while row * k < 2^32 (pc kernel)
    unsigned umagic, vmagic;                     // the same for u.inner / v.inner (2-level rows of the deep kernel)
    int pin_clouds;                              // B when the rows are B equal clouds (gpe_edge_redgemm), else 0
    const float* v_shift;                        // optional [Ng]: V := V - shift on valid rows (BN centring)
    int vec;                                     // rows aligned to 16 B and padded to 4 columns: plain 16-B loads
    int pin_tpc;                                 // gather variants of the pc/b3 kernels: tiles per cloud when pinned (gpe_common.h)
    int rev;                                     // walk the tile sequence from the far end (gpe_common.h GpeTileSeq)
    float* part;                                 // [gridDim.x][MgPad][NgPad]
    double* part_cs;                             // [gridDim.x][MgPad]
    // f16x3 variant of the b3 kernel: bit patterns of the largest magnitudes of U and of V - shift (device memory)
    const unsigned* amax_u;
    const unsigned* amax_v;
    // LAZY dz3 (f16x3, k = 16, dense V): U is the stored activation a3 of the aggregated block and the producers form dz3 from it
    // (gpe_edge_dz3's arithmetic; RgParams::lz_* of the edge kernels has the same fields).  NULL = off.
    const float* lz_g; int lz_ldg;
    const uint8_t* lz_amx; const uint8_t* lz_amn; int lz_ldagg;
    const float* lz_coef;                        // [4][Mg] = {s, c1, k2, mean}
};

// ---- "can a 16-byte loader take these rows": three predicates, one per loader, NOT interchangeable ----------------------------
//                      levels          pitch                                     base
//   gpe_rd_rows_pc     single only     outer % 4 == 0, outer >= round4(cols)     16-B aligned (NULL passes)
//   gpe_rd_rows_deep   one or two      outer (and inner) % 4 == 0;               16-B aligned (NULL passes)
//                                      row pitch >= round4(cols) OR cols % 4 == 0
//   gpe_rd_rows_x6     one or two      outer (and inner) % 4 == 0;               16-B aligned and not NULL
//                                      row pitch >= round4(cols)
// (row pitch = stride_inner of two-level rows, else stride_outer)
// producer/consumer, b3, big-block and thin loaders: RdParams::vec; false only costs the guarded scalar-tail loader
static inline bool gpe_rd_rows_pc(const GpeRows& r, int cols)
{
    return r.inner <= 0 && !(r.stride_outer & 3) && r.stride_outer >= ((cols + 3) & ~3) && !(((uintptr_t)r.base) & 15);
}
// deep kernel, through the 2-level descriptor: U must pass; V chooses the <VVEC> instance
static inline bool gpe_rd_rows_deep(const GpeRows& r, int cols)
{
    const long pitch = r.inner > 0 ? r.stride_inner : r.stride_outer;
    if ((((uintptr_t)r.base) & 15) || (r.stride_outer & 3)) return false;
    if (r.inner > 0 && (r.stride_inner & 3)) return false;
    return pitch >= ((cols + 3) & ~3) || (cols & 3) == 0;
}
// bf16-pipe kernels of gpe_gemm_x6.hip (TN: both operands must pass; NT: the A rows)
static inline bool gpe_rd_rows_x6(const GpeRows& r, int cols)
{
    if (!r.base || (((uintptr_t)r.base) & 15) || (r.stride_outer & 3)) return false;
    if (r.inner > 0) return !(r.stride_inner & 3) && r.stride_inner >= ((cols + 3) & ~3);
    return r.stride_outer >= ((cols + 3) & ~3);
}

// ---- the partial image: ONE function behind gpe_redgemm_ws and every launch ----------------------------------------------------
//   [nblk][MgPad][NgPad] floats | rounded up to an even count (8-B alignment) | [nblk][MgPad] fp64 column sums of U, if wanted
// Offsets and sizes in floats from the workspace pointer.
struct GpeRdLayout { long cs_off, total; };
static inline GpeRdLayout gpe_rd_layout(long nblk, long MgPad, long NgPad, bool want_colsum)
{
    GpeRdLayout l;
    l.cs_off = (nblk * MgPad * NgPad + 1) & ~1L;
    l.total = l.cs_off + (want_colsum ? 2 * nblk * MgPad : 0);
    return l;
}

// ---- geometry ------------------------------------------------------------------------------------------------------------------
static inline int gpe_rd_pick(int need, const int* opts, int n)
{
    for (int i = 0; i < n; ++i) if (opts[i] >= need) return opts[i];
    return -1;
}
// big-block kernel: M / N half-blocks per wave off its menu (-1: off the menu), M blocks, pads.  No device query: gpe_redgemm_ws
// must be computable on a CPU-only box.  The same pads serve the producer/consumer and b3 kernels (gy == 1 there).
static inline void gpe_rd_geometry(int Mg, int Ng, int* MH, int* NH, int* gy, int* MgPad, int* NgPad)
{
    const int MH_OPTS[3] = {2, 5, 7}, NH_OPTS[4] = {1, 5, 7, 8};
    // (64-row output blocks for the row-poor LSTM weight gradients were tried and measured slower: 2.43 vs 1.95 ms per
    // step — only 16 of 64 staging lanes carry U columns)
    const int mt = gpe_cdiv(Mg, 16), nt = gpe_cdiv(Ng, 16);
    const int mtb = mt < 14 ? mt : 14;
    // (r02: for the row-poor LSTM weight gradients — 10 k rows against a 1000 x 250 output — a narrower M block with fewer
    // row splits was tried: partials 52 -> 16 MB, but the reduce-GEMM time went UP, 1.85 -> 2.56 ms per step: with 2 M-tiles
    // per wave the V operand is re-read 3.5x as often from LDS and the MFMA stream is too short to hide it.)
    *MH = gpe_rd_pick(gpe_cdiv(mtb, 2), MH_OPTS, 3);
    *NH = gpe_rd_pick(gpe_cdiv(nt, 2), NH_OPTS, 4);
    *gy = gpe_cdiv(mt, 2 * (*MH));
    *MgPad = (*gy) * 32 * (*MH);
    *NgPad = gpe_round_up(Ng, 16);
}
// row split of the deep kernel: ~3 workgroups per CU, but enough of them for at most RDD_MAX_TPW row tiles each as far as the
// RDD_MAX_GX partial images allow (every workgroup sums its tiles in one fp32 accumulator chain, whose rounding grows with its length:
// sized by the CU count alone, 64 usable CUs put 8 k rows into one chain just below the deep-kernel switch, 3.1e-6 of max|G| against
// fp64), and at least 4 row tiles each
static inline int gpe_rdd_gx(int Mg, int Ng, long num_tiles, int cus)
{
    const long blocks = (long)gpe_cdiv(Mg, RDD_B) * gpe_cdiv(Ng, RDD_B);
    long gx = gpe_cdiv(3L * cus, blocks);
    if (gx < gpe_cdiv(num_tiles, (long)RDD_MAX_TPW)) gx = gpe_cdiv(num_tiles, (long)RDD_MAX_TPW);
    if (gx > RDD_MAX_GX) gx = RDD_MAX_GX;
    if (gx > num_tiles / 4) gx = num_tiles / 4;
    return gx < 1 ? 1 : (int)gx;
}
// TN kernel's menu: also the row-poor products (32 .. 736 rows: the exact kernels run those on ONE workgroup per column block —
// 39 - 53 us for 2 - 90 MFLOP): here they are a handful of 128 x 128 blocks of one to six steps
static inline bool gpe_rd_x6_menu(const GpeRows& u, const GpeRows& v, long rows, int Mg, int Ng)
{
    if (rows < 32 || rows >= (1L << 31) || Mg < 48 || Ng < 48 || 2.0 * rows * Mg * Ng < 2.0e6) return false;
    return gpe_rd_rows_x6(u, Mg) && gpe_rd_rows_x6(v, Ng);
}
// ... and its row split: one workgroup per CU and output block, >= 4 steps (128 rows) each, pieces of a multiple of 32 rows
static inline int gpe_rd_x6_split(long rows, int Mg, int Ng, int cus, long* rows_per_split)
{
    int S = cus / (gpe_cdiv(Mg, GX_B) * gpe_cdiv(Ng, GX_B));
    if (S > GX_RED_MAX_S) S = GX_RED_MAX_S;
    if (S > rows / 128) S = (int)(rows / 128);
    if (S < 1) S = 1;
    *rows_per_split = ((rows + S - 1) / S + 31) & ~31L;
    return (int)((rows + *rows_per_split - 1) / *rows_per_split);
}

// ---- gpe_redgemm_ws: the largest partial image any path may write, + 8 floats of slack -----------------------------------------
// Each term is gpe_rd_layout at the path's largest nblk; the launch's nblk never exceeds it because
//   big-block / pc / b3   gx = min(cus, RD_MAX_GX) / gy, at least 1, at most num_tiles          <= max(RD_MAX_GX / gy, 1)
//   deep                  gpe_rdd_gx clamps to RDD_MAX_GX
//   thin                  gx = min(rows / 64, RDT_GX); taken only when Ng <= 4
//   TN                    gpe_rd_x6_split clamps to GX_RED_MAX_S, and its second step (pieces rounded up) only lowers S
// and the pads of each path depend on (Mg, Ng) alone.  The TN term carries 1024 floats more: the step timeline of
// gpe_debug_set(32768), which the launch puts at gpe_rd_x6_ws_floats - 1024.
static inline long gpe_rd_x6_ws_floats(int Mg, int Ng)
{
    return gpe_rd_layout(GX_RED_MAX_S, gpe_round_up(Mg, GX_B), gpe_round_up(Ng, GX_B), true).total + 8 + 1024;
}
static inline long gpe_rd_ws_floats(int Mg, int Ng)
{
    int MH, NH, gy, MgPad, NgPad;
    gpe_rd_geometry(Mg, Ng, &MH, &NH, &gy, &MgPad, &NgPad);
    if (NH < 0 || gy < 1) return -1;             // Ng > 256; Mg <= 0 (no M block: the entry points refuse it)
    long m = gpe_rd_layout(RD_MAX_GX / gy > 0 ? RD_MAX_GX / gy : 1, MgPad, NgPad, true).total + 8;
    const long deep = gpe_rd_layout(RDD_MAX_GX, gpe_round_up(Mg, RDD_B), gpe_round_up(Ng, RDD_B), true).total + 8;
    const long thin = Ng <= 4 ? gpe_rd_layout(RDT_GX, gpe_round_up(Mg, 4), 4, true).total + 8 : 0;
    const long x6 = gpe_rd_x6_ws_floats(Mg, Ng);
    if (deep > m) m = deep;
    if (thin > m) m = thin;
    return x6 > m ? x6 : m;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------
enum GpeRdPath {
    GPE_RD_NOTHING,       // nothing is launched: the entry point returns rc
    GPE_RD_THIN,          // 1  gpe_redgemm_thin_kernel<ql>: Ng <= 4, streams U once
    GPE_RD_X6_TN,         // 2  gpe_gemm_x6_tn_kernel (gpe_gemm_x6.hip): f16x3 mode, dense, on the bf16 pipe
    GPE_RD_DEEP,          // 3  gpe_redgemm_deep_kernel<vvec>: row-poor dense products, 64 x 64 output blocks
    GPE_RD_B3_LAZY,       // 4  gpe_redgemm_b3_kernel<MT, 13, dense, F16, LAZY>: forms U = dz3 on the fly
    GPE_RD_B3_F16,        // 5  gpe_redgemm_b3_kernel<MT, 13, vmode, F16>: edge shape, f16x3 with both amax words
    GPE_RD_B3_BF16,       // 6  gpe_redgemm_b3_kernel<MT, 13, vmode>: edge shape, bf16x3
    GPE_RD_PC,            // 7  gpe_redgemm_pc_kernel<MT, 13, vmode>: edge shape, exact fp32
    GPE_RD_BIG            // 8  gpe_redgemm_kernel<MH, NH, vmode>: everything else
};
struct GpeRdPlan {
    GpeRdPath path; int rc;
    int vmode;                            // V_DENSE / V_GATHER, as received
    int gx, gy, gz;                       // grid of the path's kernel (TN: gx = S row pieces)
    long rows_per_split;                  // TN: rows per piece
    int MH, NH;                           // big-block: half-blocks per wave
    int MT;                               // pc / b3: 16-column tiles of U, 13 or 10 (V: 13)
    int MgPad, NgPad, nblk, num_tiles;    // partial image: pads, partials (= gx); RD_RT-row tiles of the product
    int vec; bool vvec; int ql;           // RdParams::vec; deep: V rows 16-B loadable; thin: column quads per lane
    int pin_tpc;                          // gathered pc / b3: tiles per cloud when clouds are pinned to XCDs, else 0
    unsigned umagic, vmagic;              // deep: ceil(2^32 / inner) of two-level rows, else 0
    bool cs;                              // the kernel writes partial column sums (part_cs is set)
    long cs_off, floats;                  // gpe_rd_layout of this launch
    long trace_off;                       // TN: where the step timeline of gpe_debug_set(32768) goes, -1 = off
};

// The edge weight-gradient shape: 13 x {13, 10} column tiles (<= 208 x 208 outputs) in one M block.  Three rungs ask for it, each
// with a tail of its own — the differences are meant as far as anyone knows, and each rung keeps its truth table:
//   TN exclusion     + both amax words (only then a b3 F16 kernel can take the call; rows and tiles unchecked)
//   deep exclusion   + gpe_rd_rows_pc on BOTH operands, num_tiles >= 4 gx   (dense only; no words, no NOPC)
//   pc_ok            + !NOPC, gpe_rd_rows_pc on U and on a dense V (a gathered V is unchecked), num_tiles >= 4 gx,
//                      gathered: k > 1 and rows * k < 2^32 (umulhi row / k by kmagic)
static inline bool gpe_rd_edge_shape(int Mg, int Ng, int gy)
{
    return gpe_cdiv(Ng, 16) == 13 && (gpe_cdiv(Mg, 16) == 13 || gpe_cdiv(Mg, 16) == 10) && gy == 1;
}

static inline GpeRdPlan gpe_rd_refuse(GpeRdPlan p, int rc) { p.path = GPE_RD_NOTHING; p.rc = rc; return p; }
static inline GpeRdPlan gpe_rd_image(GpeRdPlan p, GpeRdPath path, int nblk, int MgPad, int NgPad, bool cs)
{
    const GpeRdLayout l = gpe_rd_layout(nblk, MgPad, NgPad, cs);
    p.path = path; p.nblk = nblk; p.MgPad = MgPad; p.NgPad = NgPad; p.cs = cs; p.cs_off = l.cs_off; p.floats = l.total;
    return p;
}

// The ladder (DESIGN.md 5.33 has it as a table).  Pure: no HIP call, no environment, no static, no launch.
//   c       the call (operands, sizes, words, lazy fields, k, pin_clouds);  vmode  V_DENSE / V_GATHER
//   math    0 exact fp32, 1 bf16x3, 2 f16x3 (gpe_math_redgemm);  debug  gpe_debug_get();  cus  usable compute units (gpe_num_cus)
static inline GpeRdPlan gpe_redgemm_plan(const RdParams& c, int vmode, bool want_colsum, int math, int debug, const GpeRdSwitches& sw, int cus)
{
    GpeRdPlan p = {};
    p.rc = GPE_OK;
    p.vmode = vmode;
    p.trace_off = -1;
    // aligned, 4-padded rows take the plain unconditional 16-B loader (all RQ loads in flight); anything else the
    // guarded scalar-tail loader
    p.vec = gpe_rd_rows_pc(c.u, c.Mg) && (vmode == V_GATHER || gpe_rd_rows_pc(c.v, c.Ng));
    int gy, MgPad, NgPad;
    gpe_rd_geometry(c.Mg, c.Ng, &p.MH, &p.NH, &gy, &MgPad, &NgPad);
    if (p.MH < 0 || p.NH < 0) return gpe_rd_refuse(p, GPE_EINVAL);
    p.num_tiles = gpe_cdiv(c.rows, RD_RT);
    const int cusx = cus > RD_MAX_GX ? RD_MAX_GX : cus;
    int gx = cusx / gy;
    if (gx < 1) gx = 1;
    if (gx > p.num_tiles) gx = p.num_tiles > 0 ? p.num_tiles : 1;
    const bool dense = vmode == V_DENSE, lazy = c.lz_g != nullptr, words = c.amax_u && c.amax_v;
    // 1  thin products: stream U once (Ng <= 4, plain 16-B loadable U rows, single-level rows on both sides).  Partial column sums
    //    only when the caller wants the column sum
    if (dense && !lazy && c.Ng <= 4 && c.Mg <= 1024 && c.rows >= 4096 && c.u.inner <= 0 && c.v.inner <= 0 && gpe_rd_rows_pc(c.u, c.Mg)) {
        p = gpe_rd_image(p, GPE_RD_THIN, (int)(c.rows / 64 < RDT_GX ? c.rows / 64 : RDT_GX), gpe_round_up(c.Mg, 4), 4, want_colsum);
        p.gx = p.nblk; p.gy = p.gz = 1;
        p.ql = gpe_cdiv(p.MgPad, 256);
        return p;
    }
    // 2  f16x3 mode: row-rich dense products off the edge kernels' menu (the decoders' weight gradients, 10304 rows x 1000 x 250; the
    //    [P|Q] projection's, 65536 x 400 x 150) on the bf16 pipe, three-term splits (gpe_gemm_x6.hip): same partial image, same
    //    finish.  A call the kernel's own menu refuses goes on down the ladder
    if (dense && math == 2 && !lazy && !(debug & 16384) && !(gpe_rd_edge_shape(c.Mg, c.Ng, gy) && words) &&
        gpe_rd_x6_menu(c.u, c.v, c.rows, c.Mg, c.Ng)) {
        const int S = gpe_rd_x6_split(c.rows, c.Mg, c.Ng, cus, &p.rows_per_split);
        p = gpe_rd_image(p, GPE_RD_X6_TN, S, gpe_round_up(c.Mg, GX_B), gpe_round_up(c.Ng, GX_B), want_colsum);
        p.gx = S; p.gy = p.MgPad / GX_B; p.gz = p.NgPad / GX_B;
        if (debug & 32768) p.trace_off = gpe_rd_x6_ws_floats(c.Mg, c.Ng) - 1024;
        return p;
    }
    // 3  row-poor dense products (fewer than 64 row tiles per workgroup of the big-block grid) with a 16-B loadable U; closed to
    //    bf16x3.  The edge weight-gradient shapes with >= 4 row tiles per workgroup stay on the producer/consumer kernels below at
    //    every size: measured (profiles/r04_h_rd_paths.md, dense V, 150 x 200) 48 / 64 / 106 / 206 us against the deep kernel's
    //    70 / 107 / 204 / 403 us at E = 41 k / 66 k / 131 k / 262 k rows (f16x3: 46 / 53 / 70 / 127 us); the deep kernel keeps the
    //    row-poor decoder products it was built for (10 k rows x 1000 x 250: 79 against 154 us)
    const long in_max = (c.u.inner > c.v.inner ? c.u.inner : c.v.inner) > 1 ? (c.u.inner > c.v.inner ? c.u.inner : c.v.inner) : 1;
    const bool edge_deep = gpe_rd_edge_shape(c.Mg, c.Ng, gy) && gpe_rd_rows_pc(c.u, c.Mg) && gpe_rd_rows_pc(c.v, c.Ng) && p.num_tiles >= 4L * gx;
    if (dense && math != 1 && !lazy && !edge_deep && sw.DEEP != 0 && p.num_tiles > 0 && p.num_tiles < 64L * gx && c.rows * in_max < (1L << 32) &&
        c.rows < (1L << 31) && gpe_rd_rows_deep(c.u, c.Mg)) {
        p = gpe_rd_image(p, GPE_RD_DEEP, gpe_rdd_gx(c.Mg, c.Ng, p.num_tiles, cusx), gpe_round_up(c.Mg, RDD_B), gpe_round_up(c.Ng, RDD_B), want_colsum);
        p.gx = p.nblk; p.gy = p.MgPad / RDD_B; p.gz = p.NgPad / RDD_B;
        p.umagic = c.u.inner > 1 ? (unsigned)(((1ull << 32) + c.u.inner - 1) / c.u.inner) : 0;
        p.vmagic = c.v.inner > 1 ? (unsigned)(((1ull << 32) + c.v.inner - 1) / c.v.inner) : 0;
        p.vvec = gpe_rd_rows_deep(c.v, c.Ng);
        return p;
    }
    // 4 - 8  one partial per workgroup of a (gx, gy) grid; these kernels always write partial column sums
    p = gpe_rd_image(p, GPE_RD_BIG, gx, MgPad, NgPad, true);
    p.gx = gx; p.gy = gy; p.gz = 1;
    p.MT = gpe_cdiv(c.Mg, 16);
    const bool pc_ok = !sw.NOPC && gpe_rd_edge_shape(c.Mg, c.Ng, gy) && gpe_rd_rows_pc(c.u, c.Mg) && (!dense || gpe_rd_rows_pc(c.v, c.Ng)) &&
                       p.num_tiles >= 4 * gx && (dense || (c.k > 1 && c.rows * c.k < (1L << 32)));   // umulhi row / k (kmagic)
    if (pc_ok && !dense && c.pin_clouds > 0 && gpe_pin_clouds(c.pin_clouds) && c.pin_clouds % GPE_NXCD == 0) {
        const long rows_per_cloud = c.rows / c.pin_clouds;
        if (rows_per_cloud % RD_RT == 0 && gx % GPE_NXCD == 0 && rows_per_cloud / RD_RT >= gx / GPE_NXCD)
            p.pin_tpc = (int)(rows_per_cloud / RD_RT);
    }
    if (lazy) {
        // 4  lazy dz3: only the f16x3 dense-V kernel forms U on the fly; the caller asked gpe_edge_lazy_dz3_ok first
        if (!(pc_ok && math == 2 && words && dense && c.k == 16 && (c.rows & 15) == 0)) return gpe_rd_refuse(p, GPE_EINVAL);
        p.path = GPE_RD_B3_LAZY;
    } else if (pc_ok && math == 2 && words) p.path = GPE_RD_B3_F16;     // 5
    else if (pc_ok && math == 1) p.path = GPE_RD_B3_BF16;               // 6
    else if (pc_ok) p.path = GPE_RD_PC;                                 // 7
    return p;                                                           // 8
}

// ---- gpe_edge_redgemm's amax words, settled in front of the plan -----------------------------------------------------------------
// f16x3: the operand scales must be known without a pass over an E-row tensor — U (a dz tensor) through the caller's amax word of
// it, V through the caller's word (dense: the amax the forward kernel measured; gathered: a bound of relu(P_i + Q_j),
// gpe_edge_pq_amax) or, for the gathered operand only, the bound passes run in the caller's workspace; else exact fp32.
//   give     the plan sees both words (RdParams::amax_u / amax_v), or neither
//   passes   V's word is the one gpe_h3_pq_passes writes into the workspace; the entry point launches them (if that launch fails the
//            plan sees neither word)
struct GpeRdWords { bool give, passes; };
static inline GpeRdWords gpe_rd_settle_words(int math, long rows, long min_rows, bool has_u, bool has_v, bool gathered, bool has_ws)
{
    GpeRdWords w = {false, false};
    if (math != 2 || !has_u || rows < min_rows) return w;
    w.passes = !has_v && gathered && has_ws;
    w.give = has_v || w.passes;
    return w;
}

// ---- the launchers, each beside its kernel ---------------------------------------------------------------------------------------
// every one: GPE_OK or an error code; p carries the plan's numbers already (rd_run); writes plan.nblk partials for gpe_redgemm_finish
int gpe_gemm_x6_launch_redgemm(const RdParams& p, const GpeRdPlan& plan, hipStream_t s);     // gpe_gemm_x6.hip
// gpe_redgemm.hip (file-local): rd_launch_thin, rd_launch_deep, rd_launch_b3_lazy, rd_launch_b3_f16, rd_launch_b3_bf16, rd_launch_pc,
// rd_launch_big, and rd_finish after whichever ran
