// Evaluating a model over a data set without a host read per batch (include/gpe_hip_eval.h; the reference's
// nn/metrics/eval_utils.py:35-76 `_eval_metrics_per_loader`):
//   * gpe_eval_add   the reference's "append the batch's value unless it is None" as one wave per batch: lane k adds key k's value
//                    into its fp32 running sum (ONE rounded add per batch, batch order = stream order) and counts it, where the key's
//                    gate lets it through.  The row of the accumulators is read from a device word, so a captured launch serves
//                    every data folder.
//   * gpe_eval_pool  the per-garment records of the whole set (the `part` rows of csrc/gpe_quality.hip, kept in one table) folded
//                    per group and overall, bit for bit as gpe_quality_finalize folds one batch: the same QmFold.
#include "gpe_common.h"
#include "gpe_quality_fold.h"

struct EvKeys { int32_t k[GPE_EVAL_MAX_KEYS]; };
struct EvSources { const float* p[GPE_EVAL_MAX_SOURCES]; };

__global__ __launch_bounds__(64) void gpe_eval_add_kernel(EvSources src, const int32_t* __restrict__ counts, EvKeys keys, int K,
                                                          float* __restrict__ sum, int32_t* __restrict__ cnt,
                                                          int32_t* __restrict__ batches, const int32_t* __restrict__ slot, int slots,
                                                          int32_t* __restrict__ status)
{
    const int k = threadIdx.x;
    const int s = slot[0];
    if (s < 0 || s >= slots) {
        if (k == 0) status[0] = 1;
        return;
    }
    if (k == 0) batches[s] = batches[s] + 1;
    if (k >= K) return;
    const int key = keys.k[k];
    const int gate = (key >> 16) & 7;
    if (gate && counts[gate - 1] <= 0) return;          // the reference's None: the batch joins neither the sum nor the count
    const float v = src.p[(key >> 8) & 3][key & 255];
    const size_t at = (size_t)s * K + k;
    sum[at] = sum[at] + v;
    cnt[at] = cnt[at] + 1;
}

extern "C" int gpe_eval_add(const float* src0, int n0, const float* src1, int n1, const float* src2, int n2, const float* src3,
                            int n3, int n_sources, const int32_t* counts, const int32_t* keys_host, int K, float* sum, int32_t* cnt,
                            int32_t* batches, const int32_t* slot, int slots, int32_t* status, void* stream)
{
    if (K < 1 || K > GPE_EVAL_MAX_KEYS || n_sources < 0 || n_sources > GPE_EVAL_MAX_SOURCES || slots < 1) return GPE_EINVAL;
    if (!keys_host || !sum || !cnt || !batches || !slot || !status) return GPE_EINVAL;
    const float* p[GPE_EVAL_MAX_SOURCES] = {src0, src1, src2, src3};
    const int n[GPE_EVAL_MAX_SOURCES] = {n0, n1, n2, n3};
    for (int i = 0; i < n_sources; ++i)
        if (n[i] < 0 || n[i] > 256 || (n[i] > 0 && !p[i])) return GPE_EINVAL;
    EvKeys keys;
    EvSources src;
    for (int i = 0; i < GPE_EVAL_MAX_SOURCES; ++i) src.p[i] = i < n_sources ? p[i] : nullptr;
    for (int k = 0; k < GPE_EVAL_MAX_KEYS; ++k) keys.k[k] = 0;
    for (int k = 0; k < K; ++k) {
        const int key = keys_host[k];
        const int idx = key & 255, s = (key >> 8) & 3, gate = (key >> 16) & 7;
        if ((key & ~0x703ff) || s >= n_sources || idx >= n[s] || gate > 4 || (gate && !counts)) return GPE_EINVAL;
        keys.k[k] = key;
    }
    hipLaunchKernelGGL(gpe_eval_add_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, src, counts, keys, K, sum, cnt, batches,
                       slot, slots, status);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// pooling: one wave per output row.  The wave fetches 64 records (8 KB) at a time, coalesced, into registers — one fetch ahead of
// the one in use — and hands them on through LDS; lane 0 folds the row's members in table order, reading record j + 1 from LDS
// while it folds record j.  The loads are not part of the order contract; QmFold::add is.
// ---------------------------------------------------------------------------------------------------------------------
#define EV_FETCH 64
#define EV_USED 12          // leading doubles of a record that the fold reads (gpe_quality_fold.h)

// lane `lane`'s share of the records g0 .. g0 + 63 (doubles lane, lane + 64, ...: coalesced) and the group id of record g0 + lane;
// past the end of the table: nothing is loaded
__device__ __forceinline__ void ev_fetch(const double* __restrict__ table, const int32_t* __restrict__ group, long G, long g0,
                                         int lane, double* pre, int& gid)
{
    const long left = G - g0;
    const int n = left < EV_FETCH ? (left > 0 ? (int)left : 0) : EV_FETCH;
    const double* src = table + (size_t)g0 * QM_PART;
    for (int t = 0; t < QM_PART; ++t) {
        const int i = lane + EV_FETCH * t;
        pre[t] = i < n * QM_PART ? src[i] : 0.0;
    }
    gid = (group && lane < n) ? group[g0 + lane] : -1;
}

__global__ __launch_bounds__(64) void gpe_eval_pool_kernel(const double* __restrict__ table, const int32_t* __restrict__ group,
                                                           long G, int n_groups, int P, int L, int flags, float* __restrict__ out,
                                                           int32_t* __restrict__ counts)
{
    __shared__ double rec[EV_FETCH * QM_PART];
    const int row = blockIdx.x, lane = threadIdx.x;
    const bool all = row == n_groups;
    QmFold f;
    int members = 0;
    double pre[QM_PART];
    int gid;
    ev_fetch(table, group, G, 0, lane, pre, gid);
    for (long g0 = 0; g0 < G; g0 += EV_FETCH) {
        const int n = (int)(G - g0 < EV_FETCH ? G - g0 : EV_FETCH);
        // which of the 64 garments belong to this row: a fetch without a member is skipped by the whole wave
        const unsigned long long mine = __ballot(lane < n && (all || gid == row));
        if (mine != 0ull)
            for (int t = 0; t < QM_PART; ++t) rec[lane + EV_FETCH * t] = pre[t];
        ev_fetch(table, group, G, g0 + EV_FETCH, lane, pre, gid);          // in flight while this fetch is folded
        if (mine == 0ull) continue;
        __syncthreads();
        if (lane == 0) {
            // the record after the current one is read from LDS while the current one is folded: the adds wait for no load
            double cur[EV_USED], nxt[EV_USED];
            for (int i = 0; i < EV_USED; ++i) nxt[i] = rec[i];
            for (int j = 0; j < n; ++j) {
                for (int i = 0; i < EV_USED; ++i) cur[i] = nxt[i];
                const int jn = j + 1 < n ? j + 1 : j;
                for (int i = 0; i < EV_USED; ++i) nxt[i] = rec[jn * QM_PART + i];
                if ((mine >> j) & 1ull) f.add(cur, flags);
            }
        }
        members += __popcll(mine);
        __syncthreads();
    }
    if (lane == 0) f.finish(members, P, L, flags, out + (size_t)row * 14, counts + (size_t)row * 4);
}

extern "C" int gpe_eval_pool(const double* table, const int32_t* group, long G, int n_groups, int P, int L, int flags, float* out,
                             int32_t* counts, void* stream)
{
    if (!table || !out || !counts || G < 1 || G > 0x7fffffffL || n_groups < 0 || n_groups > 65535 || P <= 0 || L <= 0 ||
        (flags & ~127))
        return GPE_EINVAL;
    if (n_groups > 0 && !group) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_eval_pool_kernel, dim3(n_groups + 1), dim3(64), 0, (hipStream_t)stream, table, group, G, n_groups, P, L,
                       flags, out, counts);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
