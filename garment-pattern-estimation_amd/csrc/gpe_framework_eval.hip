// Scoring the edge-pair classifier on predicted patterns over a whole data set without a host read per batch
// (include/gpe_hip_framework.h; the reference's nn/data/datasets.py:1134-1159 `_clean_datapoint_list` and
// nn/metrics/eval_utils.py:35-76 `_eval_metrics_per_loader` with one garment per batch):
//   * gpe_framework_eval_add   one wave per batch.  64 garments at a time: lane b decides garment b's state, forms its seven fp32
//                              values and writes its record; then lane k adds key k of set 0, lane 8 + k key k of set 1, in garment
//                              order (ONE rounded fp32 add per counted garment), and lanes 16 .. 21 count.  The running sums live in
//                              registers for the launch: loaded once, stored once.
//   * gpe_framework_eval_pool  one wave per output row over the table of records: the integer totals per lane (order-free), the
//                              fp64 loss sums by one lane in table order.
// Both are latency-bound single-wave kernels: plain loads and stores, no atomics.
#include "gpe_common.h"

#define FW_KEYS GPE_FRAMEWORK_KEYS
#define FW_REC GPE_FRAMEWORK_RECORD
#define FW_CHUNK 64

__device__ __forceinline__ float fw_ratio(int num, int den) { return den ? (float)num / (float)den : 0.f; }

__global__ __launch_bounds__(64) void gpe_framework_eval_add_kernel(
    const int32_t* __restrict__ counts, const double* __restrict__ loss_sum, const int32_t* __restrict__ num_selected,
    const int32_t* __restrict__ num_stitches, const int32_t* __restrict__ first_invalid, const int32_t* __restrict__ num_panels,
    const int32_t* __restrict__ gt_num_panels, const int32_t* __restrict__ num_edges, const int32_t* __restrict__ place_flags, int B,
    int P, float* __restrict__ sum, int32_t* __restrict__ cnt, int32_t* __restrict__ skipped, double* __restrict__ records,
    const int32_t* __restrict__ slot, int slots, int32_t* __restrict__ status)
{
    __shared__ float s_val[FW_CHUNK][FW_KEYS + 1];
    __shared__ int s_state[FW_CHUNK];          // state | corr flag << 8
    const int lane = threadIdx.x;
    const int s = slot[0];
    if (s < 0 || s >= slots) {
        if (lane == 0) status[0] = 1;
        return;
    }
    // this lane's accumulator: lanes 0 .. 6 the sums of set 0, 8 .. 14 those of set 1; 16 / 17 the garments of the sets; 18 .. 21 skipped
    const int set = lane >> 3, key = lane & 7;
    const bool adds = lane < 16 && key < FW_KEYS;
    const size_t sum_at = ((size_t)set * slots + s) * FW_KEYS + key;
    float acc = adds ? sum[sum_at] : 0.f;
    int32_t* word = lane == 16 ? cnt + s : lane == 17 ? cnt + slots + s : (lane >= 18 && lane < 22) ? skipped + (size_t)s * 4 + (lane - 18)
                                                                                                     : nullptr;
    int n = word ? word[0] : 0;

    for (int b0 = 0; b0 < B; b0 += FW_CHUNK) {
        const int m = B - b0 < FW_CHUNK ? B - b0 : FW_CHUNK;
        if (lane < m) {
            const size_t b = (size_t)b0 + lane;
            int bad = 0;
            for (int p = 0; p < P; ++p) bad |= (num_edges[b * P + p] > 0 && place_flags[b * P + p] != 0) ? 1 : 0;
            const int first = first_invalid[b];
            const int n_labels = first >= 0 ? first : num_stitches[b];
            const int32_t* c = counts + b * 6;
            const int pairs = c[0], correct = c[1], tp = c[2], pred = c[3], gtp = c[4], sel_tp = c[5], n_sel = num_selected[b];
            const double ls = loss_sum[b];
            const int state = bad ? 1 : n_labels == 0 ? 2 : pairs == 0 ? 3 : 0;
            const int corr = num_panels[b] == gt_num_panels[b] ? 1 : 0;
            float v[FW_KEYS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (state == 0) {
                v[0] = v[1] = (float)(ls / (double)pairs);
                v[2] = fw_ratio(correct, pairs);
                v[3] = fw_ratio(tp, pred);
                v[4] = fw_ratio(tp, gtp);
                v[5] = fw_ratio(sel_tp, n_sel);
                v[6] = fw_ratio(sel_tp, gtp);
            }
            for (int k = 0; k < FW_KEYS; ++k) s_val[lane][k] = v[k];
            s_state[lane] = state | (corr << 8);
            double* r = records + b * FW_REC;
            r[0] = (double)state;
            r[1] = (double)corr;
            r[2] = ls;
            r[3] = (double)pairs;
            r[4] = (double)correct;
            r[5] = (double)tp;
            r[6] = (double)pred;
            r[7] = (double)gtp;
            r[8] = (double)sel_tp;
            r[9] = (double)n_sel;
        }
        __syncthreads();
        if (lane < 22) {
            for (int j = 0; j < m; ++j) {
                const int st = s_state[j];
                const int state = st & 255, corr = st >> 8;
                const bool in_set = state == 0 && (set == 0 || corr);
                if (adds) {
                    if (in_set) acc = acc + s_val[j][key];
                } else if (lane == 16) {
                    n += state == 0;
                } else if (lane == 17) {
                    n += state == 0 && corr;
                } else if (lane >= 18) {
                    const int r = lane - 18;
                    n += r < 3 ? state == r + 1 : (state == 0 && !corr);
                }
            }
        }
        __syncthreads();
    }
    if (adds) sum[sum_at] = acc;
    if (word) word[0] = n;
}

extern "C" int gpe_framework_eval_add(const int32_t* counts, const double* loss_sum, const int32_t* num_selected,
                                      const int32_t* num_stitches, const int32_t* first_invalid, const int32_t* num_panels,
                                      const int32_t* gt_num_panels, const int32_t* num_edges, const int32_t* place_flags, int B, int P,
                                      float* sum, int32_t* cnt, int32_t* skipped, double* records, const int32_t* slot, int slots,
                                      int32_t* status, void* stream)
{
    if (B < 1 || P < 1 || P > GPE_FRAMEWORK_MAX_PANELS || slots < 1) return GPE_EINVAL;
    if (!counts || !loss_sum || !num_selected || !num_stitches || !first_invalid || !num_panels || !gt_num_panels || !num_edges ||
        !place_flags || !sum || !cnt || !skipped || !records || !slot || !status)
        return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_framework_eval_add_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counts, loss_sum, num_selected,
                       num_stitches, first_invalid, num_panels, gt_num_panels, num_edges, place_flags, B, P, sum, cnt, skipped,
                       records, slot, slots, status);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// pooling: one wave per output row
// ---------------------------------------------------------------------------------------------------------------------
#define FW_TOT 8          // the six counts, num_selected, garments

__global__ __launch_bounds__(64) void gpe_framework_eval_pool_kernel(const double* __restrict__ table,
                                                                     const int32_t* __restrict__ group, long G, int n_groups,
                                                                     long long* __restrict__ totals, double* __restrict__ loss,
                                                                     float* __restrict__ ratios)
{
    __shared__ double rec[FW_CHUNK * FW_REC];
    const int row = blockIdx.x, lane = threadIdx.x;
    const bool all = row == n_groups;
    long long tot[2][FW_TOT];
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < FW_TOT; ++k) tot[t][k] = 0;
    double l0 = 0.0, l1 = 0.0;
    for (long g0 = 0; g0 < G; g0 += FW_CHUNK) {
        const int n = (int)(G - g0 < FW_CHUNK ? G - g0 : FW_CHUNK);
        const double* src = table + (size_t)g0 * FW_REC;
        for (int t = 0; t < FW_REC; ++t) {
            const int i = lane + FW_CHUNK * t;                      // coalesced: doubles lane, lane + 64, ...
            if (i < n * FW_REC) rec[i] = src[i];
        }
        const int gid = (group && lane < n) ? group[g0 + lane] : -1;
        __syncthreads();
        bool in0 = false, in1 = false;
        if (lane < n && (all || gid == row)) {
            const double* r = rec + lane * FW_REC;
            in0 = r[0] == 0.0;
            in1 = in0 && r[1] != 0.0;
            if (in0) {
                for (int k = 0; k < 7; ++k) {
                    const long long v = (long long)r[3 + k];
                    tot[0][k] += v;
                    if (in1) tot[1][k] += v;
                }
                tot[0][7] += 1;
                if (in1) tot[1][7] += 1;
            }
        }
        const unsigned long long m0 = __ballot(in0), m1 = __ballot(in1);
        if (lane == 0 && m0 != 0ull) {
            for (int j = 0; j < n; ++j) {
                if ((m0 >> j) & 1ull) {
                    const double v = rec[j * FW_REC + 2];
                    l0 += v;
                    if ((m1 >> j) & 1ull) l1 += v;
                }
            }
        }
        __syncthreads();
    }
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < FW_TOT; ++k)
            for (int o = 32; o > 0; o >>= 1) tot[t][k] += __shfl_xor(tot[t][k], o);
    if (lane == 0) {
        for (int t = 0; t < 2; ++t) {
            const long long* c = tot[t];
            const double total = t ? l1 : l0;
            const size_t at = (size_t)row * 2 + t;
            for (int k = 0; k < FW_TOT; ++k) totals[at * FW_TOT + k] = c[k];
            loss[at] = total;
            float* out = ratios + at * 6;
            // gpe_stitch_eval_finalize's metrics (csrc/gpe_stitch_pairs.hip): pairs, correct, tp, predicted, gt, selected_tp, selected
            out[0] = c[0] ? (float)(total / (double)c[0]) : 0.f;
            out[1] = c[0] ? (float)c[1] / (float)c[0] : 0.f;
            out[2] = c[3] ? (float)c[2] / (float)c[3] : 0.f;
            out[3] = c[4] ? (float)c[2] / (float)c[4] : 0.f;
            out[4] = c[6] ? (float)c[5] / (float)c[6] : 0.f;
            out[5] = c[4] ? (float)c[5] / (float)c[4] : 0.f;
        }
    }
}

extern "C" int gpe_framework_eval_pool(const double* table, const int32_t* group, long G, int n_groups, int64_t* totals, double* loss,
                                       float* ratios, void* stream)
{
    if (!table || !totals || !loss || !ratios || G < 1 || G > 0x7fffffffL || n_groups < 0 || n_groups > 65535) return GPE_EINVAL;
    if (n_groups > 0 && !group) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_framework_eval_pool_kernel, dim3(n_groups + 1), dim3(64), 0, (hipStream_t)stream, table, group, G,
                       n_groups, reinterpret_cast<long long*>(totals), loss, ratios);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
