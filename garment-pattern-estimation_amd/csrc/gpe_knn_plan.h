// Which graph-search kernel runs (gpe_knn / gpe_knn_ws_bytes / gpe_knn_path): host code only.  What the three kernel files
// (gpe_knn.hip, gpe_knn3.hip, gpe_knn_ft.hip) and the entry points (gpe_knn_search.hip) share on the host lives here ONCE:
//   the constants more than one file needs, the measurement switches, the call as received, the workspace layout,
//   gpe_knn_plan — the whole selection ladder as a pure function — and the launchers' declarations.
// A launcher decides nothing: it turns the plan's numbers into template arguments, sizes its kernel's LDS beside the kernel,
// launches and checks.
#pragma once
#include "gpe_common.h"

// ---- constants shared between files (a constant only one kernel file uses stays there) --------------------------------------
#define KNN_TQ 64                         // queries per workgroup of the all-pairs and the list kernels
#define KNN_TC 64                         // candidates per tile (every kernel)
#define KNN_MF_MINC 16                    // narrowest rows the matrix-pipe filters serve
#define KNN_H3_MAXC 256                   // widest rows of the fp16-pipe filters (wider: the fp32 matrix-pipe filter)
#define KNN_FT_NBMAX 5                    // threshold scan: 32-channel blocks, C <= 160
#define KNN_FT_MAXK 32                    // threshold scan: largest k
#define KNN_FT_CAP 64                     // threshold scan: keys per query it hands to the recheck
#define K3_MINN 128                       // sorted-cloud search: cloud sizes it takes
#define K3_MAXN 8192
#ifndef K3_QW
#define K3_QW 4                           // sorted-cloud search: queries per wave
#endif
#define KNN_FILTER_MAXK 48                // largest k a filter serves (K2 = k + 8 <= 64 entries of a lane-distributed list)

// ---- measurement switches: GPE_KNN_<FIELD>, consulted only under GPE_DEBUG=1 (gpe_dbg_env), read once per process ---------
struct GpeKnnSwitches {
    int PROBE;      // default 0.  Timing aid, WRONG RESULTS: bit 0 selection on the first tile only, bit 1 no staging after the
                    // first step, bit 2 no distance arithmetic (all-pairs kernel: its probe instance; the filters: an argument)
    int PIN;        // default -1 = the rule (B >= 8).  0 never pins clouds to XCDs, 1 pins when B >= 8.  Exact
    int VEC;        // default 0 = widest the rows allow.  1 / 2 / 4 caps the staging vector width of the all-pairs kernel and
                    // of the fp32 filter.  Exact
    int SPLIT;      // default 0 = the rule.  n forces n candidate pieces per query tile where n * k (all-pairs) or n * K2
                    // (filters) <= 64, n <= tiles and the workspace holds the lists; a forced split keeps the list kernels
                    // (the threshold scan has no pieces).  Exact
    int EXACT;      // default 0.  1 sends every search to the all-pairs group, whatever C and k.  Exact
    int F32FILTER;  // default 0.  1 filters with the fp32 matrix-pipe kernel also for C <= 256.  Exact
    int SORTED;     // default 1.  0 keeps xyz clouds off the sorted-cloud search (the all-pairs kernel runs).  Exact
    int NOORDER;    // default 0.  1 ignores the caller's order hint (planes in point order, scans from tile 0).  Exact
    int FT;         // default 1.  0 keeps the ordered-list kernels where the threshold scan would run; 4 / 8 force its
                    // 64- / 128-query workgroup.  Exact
    int RR2;        // default 1.  0 rechecks a threshold scan one query per wave (the list recheck in its unsorted mode).  Exact
};
const GpeKnnSwitches& gpe_knn_switches();               // this process's (gpe_knn_search.hip)

// ---- the search as gpe_knn received it -----------------------------------------------------------------------------------
struct GpeKnnCall {
    const float* x; int B, N, C, ldx, k;
    int32_t* idx; int32_t* idx_glob;
    const int32_t* order_in; int32_t* order_out;
    void* ws; long ws_bytes;
    hipStream_t stream;
};

// ---- workspace layout: ONE function behind gpe_knn_ws_bytes and the launch ----------------------------------------------
//   [lists | norms | cmax | planes | iscale | slack]        byte offsets from the (16-byte aligned) workspace pointer
//   lists   64 keys per query: the filters' candidate lists (nsplit * K2 <= 64; the threshold scan: KNN_FT_CAP)
//   norms   |x|^2 per point;  cmax  its maximum per cloud (bit pattern)
//   planes  the two fp16 planes of the table, C rounded up to 32 (KNN_MF_MINC <= C <= KNN_H3_MAXC only);  iscale  1 / row scale
// Two more users ALIAS the list region, from offset 0 (their paths build no filter list):
//   the all-pairs kernel's split lists   nsplit * k <= 64 keys per query (gpe_knn_plan grants no other split)
//   the sorted-cloud search              xs: one float4 per point, then tb: 8 floats per tile of 64 sorted points
// Both fit a workspace of the queried size: the first by the plan's rule, the second because a cloud has no more tiles than points:
static_assert(sizeof(float4) + 8 * sizeof(float) <= 64 * sizeof(unsigned long long), "sorted cloud + tile boxes must fit the list region");
struct GpeKnnWs {
    size_t lists_bytes;                   // region at offset 0
    size_t norms, cmax, planes, iscale;   // offsets
    size_t tb, sorted_bytes;              // aliases of the list region: xs at 0, tb behind it; what both take
    size_t need_f32;                      // what a filter launch needs without planes / iscale ...
    size_t need_h3;                       // ... and with them
    size_t total;                         // gpe_knn_ws_bytes: need_h3 where the fp16-pipe filters serve C, else need_f32; + 256
};
static inline size_t gpe_knn_up256(size_t b) { return (b + 255) & ~(size_t)255; }
static inline GpeKnnWs gpe_knn_ws_layout(int B, int N, int C)
{
    GpeKnnWs w;
    const size_t nq = (size_t)B * N;
    const size_t norm_bytes = gpe_knn_up256(nq * sizeof(float)), cmax_bytes = gpe_knn_up256((size_t)B * sizeof(int));
    const size_t CP = ((size_t)C + 31) & ~(size_t)31;
    const size_t pl_bytes = gpe_knn_up256(nq * 2 * CP * sizeof(_Float16));
    w.lists_bytes = nq * 64 * sizeof(unsigned long long);                 // a multiple of 256
    w.norms = w.lists_bytes;
    w.cmax = w.norms + norm_bytes;
    w.planes = w.cmax + cmax_bytes;
    w.iscale = w.planes + pl_bytes;
    w.tb = nq * sizeof(float4);
    w.sorted_bytes = w.tb + (size_t)B * gpe_cdiv(N, 64) * 8 * sizeof(float);
    w.need_f32 = w.planes + 256;
    w.need_h3 = w.need_f32 + pl_bytes + norm_bytes;
    w.total = ((C >= KNN_MF_MINC && C <= KNN_H3_MAXC) ? w.need_h3 : w.need_f32) + 256;
    return w;
}
// ... and the all-pairs kernel's split lists, also from offset 0
static inline size_t gpe_knn_split_bytes(int B, int N, int nsplit, int k) { return (size_t)B * N * nsplit * k * sizeof(unsigned long long); }

// ---- the plan ------------------------------------------------------------------------------------------------------------
#define GPE_KNN_PLAN_FIELDS 24             // numbers gpe_knn_path writes to plan_out (include/gpe_hip.h fixes their order)
enum GpeKnnPath {         // the values are gpe_knn_path's return codes (include/gpe_hip.h): they do not change
    GPE_KNN_NOTHING = 0,  // nothing is launched: gpe_knn returns rc (bad arguments, B == 0, a grid past 2^31 workgroups)
    GPE_KNN_SORTED3 = 1,  // 1a  xyz cloud, sorted along a Morton curve, tile pruning (gpe_knn3.hip); writes order_out itself
    GPE_KNN_ALLPAIRS = 2, // 1b / 2a  every distance by the defined chain
    GPE_KNN_SCAN = 3,     // 2b  fp16-pipe threshold scan (gpe_knn_ft.hip) + recheck
    GPE_KNN_LISTS = 4,    // 2c  fp16-pipe ordered-list kernel <2> / <5> / <8> + one-query recheck
    GPE_KNN_F32FILTER = 5 // 2d  fp32 matrix-pipe filter + one-query recheck
};
struct GpeKnnPlan {
    GpeKnnPath path; int rc;
    bool identity;                        // order_out gets the identity, first of all launches
    int pin, tiles, nsplit, vec;          // clouds pinned to XCDs; KNN_TQ-query tiles per cloud; candidate pieces; staging vector floats
    long nblocks;                         // workgroups of the path's main kernel
    int probe; bool smallc;               // all-pairs kernel: its probe / C <= 4 instance
    int K2, CP, NB; float ce;             // filters: keys kept per query, padded plane width, its 32-channel blocks, error-bound factor
    bool wide; int qtiles;                // scan: 128-query workgroups; query tiles per cloud (sorted cloud: workgroups per cloud)
    bool rerank2; int unsorted;           // recheck: two queries per wave, else one (unsorted = 1: keys as the scan leaves them)
    const int32_t* order;                 // the order hint in use (planes, scan start), NULL = point order
    unsigned long long* part;             // workspace regions in use, NULL = unused
    float* norms; int* cmax; _Float16* planes; float* iscale;
    float4* xs; float* tb;
};

// what a filter keeps per query: the K2 best candidates by the matrix-pipe distance
static inline int gpe_knn_k2(int k, int N)
{
    int K2 = (2 * k < 32) ? 2 * k : 32;
    if (K2 < k + 8) K2 = k + 8;
    if (K2 > 64) K2 = 64;
    if (K2 > N) K2 = N;
    return K2;
}
static inline bool gpe_knn_valid(const GpeKnnCall& c)
{
    return c.x && c.idx && c.B >= 0 && c.N > 0 && c.C > 0 && c.ldx >= c.C && c.k > 0 && c.k <= 64 && c.k <= c.N &&
           (long)c.B * c.N * c.k < (1L << 31);
}
static inline bool gpe_knn_ws_holds(const GpeKnnCall& c, size_t bytes) { return c.ws && !(((uintptr_t)c.ws) & 15) && (size_t)c.ws_bytes >= bytes; }
static inline long gpe_knn_tile_blocks(int pin, int B, int tiles) { return pin ? (long)GPE_NXCD * gpe_cdiv(B, GPE_NXCD) * tiles : (long)B * tiles; }
static inline GpeKnnPlan gpe_knn_refuse(GpeKnnPlan p, int rc) { p.path = GPE_KNN_NOTHING; p.rc = rc; p.identity = false; return p; }

// steps 1b / 2a: the all-pairs kernel.  with_ws = false: the filter group's fall-back, one piece whatever the workspace would hold
static inline GpeKnnPlan gpe_knn_plan_allpairs(GpeKnnPlan p, const GpeKnnCall& c, int usable_cus, const GpeKnnSwitches& sw, bool with_ws)
{
    p.path = GPE_KNN_ALLPAIRS;
    // Candidate split.  With every workgroup resident (4 per CU) an XCD works on 128 items at a time = 128 / (tiles * nsplit)
    // clouds, whose tables (N x ldx floats each) are streamed once per item: they must fit the XCD's 4 MiB L2 together or the
    // cyclic stream evicts every line before its next use (measured at cfg 2, layer 2: 4 x 1.25 MB -> 396-475 MB fetched for
    // 39 MB; 3 tables -> 36 MB).  nsplit pieces per query tile put nsplit x fewer clouds in flight.
    p.nsplit = 1;
    if (p.pin) {
        const double table = (double)c.N * c.ldx * sizeof(float), l2_budget = 3.2 * 1024 * 1024;
        const int resident = 4 * usable_cus / GPE_NXCD;                    // items in flight per XCD
        for (;;) {
            const double clouds = (double)resident / ((double)p.tiles * p.nsplit);
            if (table * (clouds > 1.0 ? clouds : 1.0) <= l2_budget) break;  // the tables in flight fit
            if (clouds <= 1.0) break;                                      // one table alone is too big: no split helps
            if (p.nsplit >= 4 || 2 * p.nsplit * c.k > 64 || 2 * p.nsplit > p.tiles) break;
            p.nsplit *= 2;
        }
    }
    if (sw.SPLIT > 0 && sw.SPLIT * c.k <= 64 && sw.SPLIT <= p.tiles) p.nsplit = sw.SPLIT;
    if (p.nsplit > 1) {
        if (with_ws && gpe_knn_ws_holds(c, gpe_knn_split_bytes(c.B, c.N, p.nsplit, c.k))) p.part = (unsigned long long*)c.ws;
        else p.nsplit = 1;                                                 // no workspace: one piece, more HBM traffic
    }
    p.nblocks = gpe_knn_tile_blocks(p.pin, c.B, p.tiles) * p.nsplit;
    if (p.nblocks >= (1L << 31)) return gpe_knn_refuse(p, GPE_EINVAL);
    // rule A, the widest staging copy the rows allow: a vector is valid or padding as a whole, so C must divide as well as the
    // pitch and the base address (a C < 32 chunk is staged ((C + 3) & ~3) floats wide, so it must divide too)
    const uintptr_t xa = (uintptr_t)c.x;
    p.vec = (c.C % 4 == 0 && c.ldx % 4 == 0 && xa % 16 == 0) ? 4 : (c.C % 2 == 0 && c.ldx % 2 == 0 && xa % 8 == 0) ? 2 : 1;
    if (sw.VEC > 0 && sw.VEC < p.vec) p.vec = sw.VEC;
    p.probe = sw.PROBE;
    p.smallc = !p.probe && p.vec == 1 && c.C <= 4;
    return p;
}

// The ladder (DESIGN.md 5.32 has it as a table).  Pure: no HIP call, no environment, no static, no launch.
static inline GpeKnnPlan gpe_knn_plan(const GpeKnnCall& c, int usable_cus, const GpeKnnSwitches& sw)
{
    GpeKnnPlan p = {};
    p.path = GPE_KNN_NOTHING;
    p.rc = GPE_OK;
    // step 0
    if (!gpe_knn_valid(c)) return gpe_knn_refuse(p, GPE_EINVAL);
    if (c.B == 0) return p;
    p.tiles = gpe_cdiv(c.N, KNN_TQ);
    p.pin = (sw.PIN >= 0) ? (sw.PIN && c.B >= GPE_NXCD) : (gpe_pin_clouds(c.B) ? 1 : 0);
    p.nsplit = 1;
    const GpeKnnWs w = gpe_knn_ws_layout(c.B, c.N, c.C);
    // step 1: every distance by the defined chain
    if (c.C < KNN_MF_MINC || c.k > KNN_FILTER_MAXK || sw.EXACT) {
        // 1a: the workspace must hold the sorted cloud and its tile boxes, the query kernel's grid must fit
        if (c.C == 3 && sw.SORTED != 0 && c.N >= K3_MINN && c.N <= K3_MAXN && gpe_knn_ws_holds(c, w.sorted_bytes) &&
            (long)c.B * gpe_cdiv(c.N, 4 * K3_QW) < (1L << 31)) {
            p.path = GPE_KNN_SORTED3;
            p.tiles = gpe_cdiv(c.N, 64);
            p.qtiles = gpe_cdiv(c.N, 4 * K3_QW);
            p.nblocks = (long)c.B * p.qtiles;
            p.xs = reinterpret_cast<float4*>(c.ws);
            p.tb = reinterpret_cast<float*>(reinterpret_cast<char*>(c.ws) + w.tb);
            return p;
        }
        p.identity = c.order_out != nullptr;           // no curve order on this path: the identity is a valid (locality-free) answer
        return gpe_knn_plan_allpairs(p, c, usable_cus, sw, true);
    }
    // step 2: matrix-pipe filter + exact recheck
    p.identity = c.order_out != nullptr;               // (only the xyz search produces an order; a filter-path caller gets the identity)
    p.K2 = gpe_knn_k2(c.k, c.N);
    // No candidate split here.  The all-pairs kernel cuts the candidate range in pieces so that the tables in flight fit an L2; for
    // this group every piece would pay its own first-tile ranking and its own list build-up (selection work x 1.7 at two pieces)
    // plus a 64-key merge per query in the recheck: measured at cfg 2, layer 2: 0.99 ms with two pieces, 0.86 ms with one (the
    // extra ~360 MB of L2 misses per launch are 0.5 TB/s of HBM traffic under a kernel that is not memory-bound).  GPE_KNN_SPLIT
    // still forces pieces (the merge code stays tested).
    if (sw.SPLIT > 0 && sw.SPLIT * p.K2 <= 64 && sw.SPLIT <= p.tiles) p.nsplit = sw.SPLIT;
    // the fp16-pipe filters (default for C <= 256; GPE_KNN_F32FILTER=1 keeps the exact-product filter for A/B measurements)
    bool h3 = !sw.F32FILTER && c.C <= KNN_H3_MAXC;
    if (h3 && (!c.ws || (size_t)c.ws_bytes < w.need_h3)) h3 = false;                        // workspace sized by an older query
    // 2a
    if (!gpe_knn_ws_holds(c, h3 ? w.need_h3 : w.need_f32)) return gpe_knn_plan_allpairs(p, c, usable_cus, sw, false);
    char* const scratch = (char*)c.ws;
    p.part = (unsigned long long*)scratch;
    p.norms = (float*)(scratch + w.norms);
    p.cmax = (int*)(scratch + w.cmax);
    p.CP = (c.C + 31) & ~31;
    p.NB = p.CP >> 5;
    // (6C + 16) * 2^-24, the bound in gpe_knn.hip; + 16 * 2^-24 for the two-term fp16 products of the fp16-pipe filters
    p.ce = (6.f * c.C + (h3 ? 32.f : 16.f)) * 5.9604645e-8f;
    p.probe = sw.PROBE;
    p.nblocks = gpe_knn_tile_blocks(p.pin, c.B, p.tiles) * p.nsplit;
    if (p.nblocks >= (1L << 31)) return gpe_knn_refuse(p, GPE_EINVAL);
    if (!h3) {
        // 2d.  Rule B, the widest staging copy: a vector may run into the row's pad columns (the kernel replaces their contents
        // by zeros), so only the pitch and the base address have to allow it — unlike rule A, C itself need not divide
        p.path = GPE_KNN_F32FILTER;
        const uintptr_t xa = (uintptr_t)c.x;
        p.vec = (c.ldx % 4 == 0 && xa % 16 == 0 && ((c.C + 3) & ~3) <= c.ldx) ? 4
              : (c.ldx % 2 == 0 && xa % 8 == 0 && ((c.C + 1) & ~1) <= c.ldx) ? 2 : 1;
        if (sw.VEC > 0 && sw.VEC < p.vec) p.vec = sw.VEC;
        return p;
    }
    p.planes = (_Float16*)(scratch + w.planes);
    p.iscale = (float*)(scratch + w.iscale);
    p.order = sw.NOORDER ? nullptr : c.order_in;
    if (sw.FT && p.NB <= KNN_FT_NBMAX && c.k <= KNN_FT_MAXK && p.nsplit == 1) {
        // 2b: 128 queries per workgroup when that still fills the chip, 64 otherwise
        p.path = GPE_KNN_SCAN;
        p.wide = sw.FT == 8 || (sw.FT != 4 && (long)c.B * gpe_cdiv(c.N, 128) >= usable_cus);
        p.qtiles = gpe_cdiv(c.N, p.wide ? 128 : 64);
        p.nblocks = gpe_knn_tile_blocks(p.pin, c.B, p.qtiles);
        p.rerank2 = sw.RR2 != 0;
        p.unsorted = 1;
        return p;
    }
    p.path = GPE_KNN_LISTS;                             // 2c
    return p;
}

// ---- the launchers, each beside its kernels ------------------------------------------------------------------------------
// every one: GPE_OK or an error code; runs on c.stream
int gpe_knn_launch_prologue(const GpeKnnCall& c, const GpeKnnPlan& p);     // gpe_knn.hip: identity order, norms + maxima, planes — what the plan names
int gpe_knn_launch_allpairs(const GpeKnnCall& c, const GpeKnnPlan& p);     // gpe_knn.hip: + the merge of the pieces
int gpe_knn_launch_lists(const GpeKnnCall& c, const GpeKnnPlan& p);        // gpe_knn.hip
int gpe_knn_launch_f32filter(const GpeKnnCall& c, const GpeKnnPlan& p);    // gpe_knn.hip
int gpe_knn_launch_recheck(const GpeKnnCall& c, const GpeKnnPlan& p);      // gpe_knn.hip
int gpe_knn_launch_sorted(const GpeKnnCall& c, const GpeKnnPlan& p);       // gpe_knn3.hip
int gpe_knn_launch_scan(const GpeKnnCall& c, const GpeKnnPlan& p);         // gpe_knn_ft.hip
