// gpe_knn / gpe_knn_ws_bytes: validate, build the call, ask gpe_knn_plan (gpe_knn_plan.h) which kernels run with
// which numbers, run the launchers the plan names.  No kernel here: they live with their launchers in gpe_knn.hip (all-pairs,
// list and fp32 filters, recheck), gpe_knn3.hip (sorted cloud) and gpe_knn_ft.hip (threshold scan).
#include "gpe_knn_plan.h"
#include <string.h>

const GpeKnnSwitches& gpe_knn_switches()
{
    static const GpeKnnSwitches sw = {gpe_dbg_env("GPE_KNN_PROBE", 0),  gpe_dbg_env("GPE_KNN_PIN", -1),  gpe_dbg_env("GPE_KNN_VEC", 0),
                                      gpe_dbg_env("GPE_KNN_SPLIT", 0),  gpe_dbg_env("GPE_KNN_EXACT", 0), gpe_dbg_env("GPE_KNN_F32FILTER", 0),
                                      gpe_dbg_env("GPE_KNN_SORTED", 1), gpe_dbg_env("GPE_KNN_NOORDER", 0), gpe_dbg_env("GPE_KNN_FT", 1),
                                      gpe_dbg_env("GPE_KNN_RR2", 1)};
    return sw;
}

// bytes of the caller's workspace (layout: gpe_knn_plan.h)
extern "C" long gpe_knn_ws_bytes(int B, int N, int C, int k)
{
    if (B < 0 || N <= 0 || C <= 0 || k <= 0 || k > 64) return GPE_EINVAL;
    return (long)gpe_knn_ws_layout(B, N, C).total;
}

// the plan of a call under this process's state: gpe_knn and gpe_knn_path both ask here, nowhere else
static GpeKnnPlan knn_plan(const GpeKnnCall& c, const GpeKnnSwitches& sw)
{
    GpeKnnPlan none = {};
    if (!gpe_knn_valid(c)) return gpe_knn_refuse(none, GPE_EINVAL);     // (the plan's step 0 too; here it keeps a refused call off the HIP runtime)
    return gpe_knn_plan(c, c.B ? gpe_num_cus() : 0, sw);
}

extern "C" int gpe_knn(const float* x, int B, int N, int C, int ldx, int k, int32_t* idx, int32_t* idx_glob, const int32_t* order_in,
                       int32_t* order_out, void* ws, long ws_bytes, void* stream)
{
    const GpeKnnCall c = {x, B, N, C, ldx, k, idx, idx_glob, order_in, order_out, ws, ws_bytes, (hipStream_t)stream};
    const GpeKnnPlan p = knn_plan(c, gpe_knn_switches());
    if (p.path == GPE_KNN_NOTHING) return p.rc;
    int rc = gpe_knn_launch_prologue(c, p);
    if (rc != GPE_OK) return rc;
    switch (p.path) {
    case GPE_KNN_SORTED3: return gpe_knn_launch_sorted(c, p);
    case GPE_KNN_ALLPAIRS: return gpe_knn_launch_allpairs(c, p);
    case GPE_KNN_SCAN: rc = gpe_knn_launch_scan(c, p); break;
    case GPE_KNN_LISTS: rc = gpe_knn_launch_lists(c, p); break;
    default: rc = gpe_knn_launch_f32filter(c, p); break;
    }
    return rc != GPE_OK ? rc : gpe_knn_launch_recheck(c, p);
}

// Which kernels a gpe_knn call runs, and the numbers of its plan (include/gpe_hip.h).  Host only: the pointers are looked at, never
// followed; the stand-ins below only have to be non-NULL.
extern "C" int gpe_knn_path(const float* x, int B, int N, int C, int ldx, int k, int has_idx_glob, int has_order_in, int has_order_out,
                            const void* ws, long ws_bytes, const int* switches, long* plan_out)
{
    static int32_t out_standin = 0;
    static const int32_t in_standin = 0;
    GpeKnnSwitches sw = gpe_knn_switches();
    if (switches)
        sw = GpeKnnSwitches{switches[0], switches[1], switches[2], switches[3], switches[4], switches[5], switches[6], switches[7], switches[8],
                            switches[9]};
    const GpeKnnCall c = {x, B, N, C, ldx, k, &out_standin, has_idx_glob ? &out_standin : nullptr, has_order_in ? &in_standin : nullptr,
                          has_order_out ? &out_standin : nullptr, const_cast<void*>(ws), ws_bytes, nullptr};
    const GpeKnnPlan p = knn_plan(c, sw);
    if (p.path == GPE_KNN_NOTHING) return p.rc;
    if (plan_out) {
        const char* const base = static_cast<const char*>(ws);
        auto off = [base](const void* r) { return r ? (long)(static_cast<const char*>(r) - base) : -1L; };
        uint32_t ce_bits;
        memcpy(&ce_bits, &p.ce, sizeof ce_bits);
        const long out[GPE_KNN_PLAN_FIELDS] = {p.identity, p.pin, p.tiles, p.nsplit, p.vec, p.nblocks, p.probe, p.smallc, p.K2, p.CP, p.NB,
                                               (long)ce_bits, p.wide, p.qtiles, p.rerank2, p.unsorted, p.order != nullptr,
                                               off(p.part), off(p.norms), off(p.cmax), off(p.planes), off(p.iscale), off(p.xs), off(p.tb)};
        for (int i = 0; i < GPE_KNN_PLAN_FIELDS; ++i) plan_out[i] = out[i];
    }
    return (int)p.path;
}
