// gpe_knn / gpe_knn_ws_bytes: validate, build the call, ask gpe_knn_plan (gpe_knn_plan.h) which kernels run with
// which numbers, run the launchers the plan names.  No kernel here: they live with their launchers in gpe_knn.hip (all-pairs,
// list and fp32 filters, recheck), gpe_knn3.hip (sorted cloud) and gpe_knn_ft.hip (threshold scan).
#include "gpe_knn_plan.h"

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

extern "C" int gpe_knn(const float* x, int B, int N, int C, int ldx, int k, int32_t* idx, int32_t* idx_glob, const int32_t* order_in,
                       int32_t* order_out, void* ws, long ws_bytes, void* stream)
{
    const GpeKnnCall c = {x, B, N, C, ldx, k, idx, idx_glob, order_in, order_out, ws, ws_bytes, (hipStream_t)stream};
    if (!gpe_knn_valid(c)) return GPE_EINVAL;           // (the plan's step 0 too; here it keeps a refused call off the HIP runtime)
    const GpeKnnPlan p = gpe_knn_plan(c, B ? gpe_num_cus() : 0, gpe_knn_switches());
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
