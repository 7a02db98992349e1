/* Feature additions to the C ABI of libgpe_hip.so (include/gpe_hip.h; gpe_abi_version() stays 7): scoring the edge-pair classifier
 * on PREDICTED patterns over a whole data set without a host read per batch (csrc/gpe_framework_eval.hip) — step 3 of the
 * reference's nn/evaluation_scripts/on_test_set.py -st ... -corr: GarmentStitchPairsDataset._clean_datapoint_list
 * (nn/data/datasets.py:1134-1159) decides which garments count, _eval_metrics_per_loader (nn/metrics/eval_utils.py:35-76) folds
 * them one garment per batch.  The conventions are those of include/gpe_hip_eval.h: caller-owned memory, every entry point returns
 * 0 / -22 (bad argument, checked before any launch and before any pointer is touched) / -5 (launch failure) and takes the HIP
 * stream as its last argument; no atomics and no allocation, so both calls are legal inside a stream capture.  Bound by
 * gpe_amd/_lib.py (FRAMEWORK_HEADERS) and seen by every definition (csrc/gpe_common.h).
 *
 * ---- which garments count ----------------------------------------------------------------------------------------------------------
 * Every garment of a batch gets a STATE, the first rule that matches:
 *     1  bad rotation   a place_flags bit is set on a panel with num_edges > 0 (the reference's scipy call raises there, uncaught:
 *                       the one deviation)
 *     2  no stitches    n_labels == 0, n_labels = first_invalid >= 0 ? first_invalid : num_stitches (datasets.py:1149, after
 *                       _pred_to_pattern :756-765 kept the stitches before the first invalid one)
 *     3  no pairs       counts.pairs == 0 (all_edge_pairs raises InvalidPatternDefError, eval_utils.py:49 skips the batch)
 *     0  counted
 * A counted garment is also in the CORR set iff num_panels == gt_num_panels (datasets.py:1152-1156).
 *
 * ---- the fold ------------------------------------------------------------------------------------------------------------------------
 * A counted garment has seven fp32 values, GPE_FRAMEWORK_KEYS in this order:
 *     0 full_loss              the same value as 1
 *     1 edge_pair_class_loss   (float)(loss_sum / pairs)                  (the fp64 quotient rounded once)
 *     2 edge_pair_class_acc    (float)correct / (float)pairs
 *     3 stitch_precision       tp / predicted positives
 *     4 stitch_recall          tp / gt positives
 *     5 selected_precision     selected_tp / num_selected
 *     6 selected_recall        selected_tp / gt positives
 * 2 .. 6 are ONE IEEE fp32 division of two exactly representable integers each; a ratio whose denominator is 0 is 0 and still
 * counted (nn/metrics/composed_loss.py:123-124).  For set 0 (all counted garments) and set 1 (the corr set), in garment order:
 *     sum[set, slot, key] = sum[set, slot, key] + value_key      (one individually rounded fp32 add per garment)
 *     cnt[set, slot] += 1
 * and skipped[slot, r] += 1 with r = 0, 1, 2 for the states 1, 2, 3 and r = 3 for "counted, but the wrong number of panels".  This
 * is the reference's append with a batch size of 1; the division float32(sum) / float32(cnt) is the caller's, after its one read.
 * The row `slot` is read from DEVICE memory (one row per data folder, as in gpe_eval_add); a slot word outside 0 .. slots-1 sets
 * status[0] = 1, adds nothing and writes no record.
 *
 * ---- the record ----------------------------------------------------------------------------------------------------------------------
 * One record of GPE_FRAMEWORK_RECORD doubles per garment, every value exact:
 *     0 state   1 corr flag (num_panels == gt_num_panels, whatever the state)   2 loss_sum
 *     3 pairs   4 correct   5 true positives   6 predicted positives   7 gt positives   8 selected_tp   9 num_selected
 *
 * ---- pooling the records of a whole set ----------------------------------------------------------------------------------------------
 * gpe_framework_eval_pool folds a table of records per group and overall, independent of how the set was cut into batches: row g of
 * the result covers the garments of group g, row n_groups all garments; per row and set (0 all counted, 1 corr)
 *     totals  int64 [8]: the six counts in the order of the record, num_selected, garments in the set
 *     loss    fp64: the sum of loss_sum in table order
 *     ratios  fp32 [6] as gpe_stitch_eval_finalize defines its metrics: loss / pairs rounded once, then (float)num / (float)den for
 *             acc, precision, recall, selected precision, selected recall; 0 on a zero denominator (so an empty group gives zeros)
 * One wave per output row: 64 records at a time are fetched coalesced into LDS, the integers are added per lane and reduced at the
 * end, and one lane adds the losses in table order.
 */
#ifndef GPE_HIP_FRAMEWORK_H
#define GPE_HIP_FRAMEWORK_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GPE_FRAMEWORK_KEYS 7
#define GPE_FRAMEWORK_RECORD 10
#define GPE_FRAMEWORK_MAX_PANELS 64

/*   counts, loss_sum            int32 [B, 6], fp64 [B]: gpe_stitch_eval_finalize's per-garment outputs
 *   num_selected                int32 [B]: num_stitches of gpe_stitch_select
 *   num_stitches, first_invalid int32 [B]: the decode's
 *   num_panels, gt_num_panels   int32 [B]: the decode's, the ground truth's
 *   num_edges, place_flags      int32 [B, P]: the decode's, the placement's
 *   B >= 1, 1 <= P <= 64
 *   sum     fp32 [2, slots, 7];  cnt int32 [2, slots];  skipped int32 [slots, 4];  slots >= 1
 *   records fp64 [B, 10]: the rows of the caller's table that belong to this batch
 *   slot    int32 [1] (device): the row this batch belongs to
 *   status  int32 [1] (device): set to 1 when the slot word is out of range, untouched otherwise */
int gpe_framework_eval_add(const int32_t* counts, const double* loss_sum, const int32_t* num_selected, const int32_t* num_stitches,
                           const int32_t* first_invalid, const int32_t* num_panels, const int32_t* gt_num_panels,
                           const int32_t* num_edges, const int32_t* place_flags, int B, int P, float* sum, int32_t* cnt,
                           int32_t* skipped, double* records, const int32_t* slot, int slots, int32_t* status, void* stream);

/*   table      fp64 [G, 10] (device), 1 <= G < 2^31
 *   group      int32 [G] (device) or NULL (then n_groups must be 0); an id outside 0 .. n_groups-1 belongs to no group but still
 *              counts in the last row
 *   n_groups   0 .. 65535
 *   totals     int64 [n_groups + 1, 2, 8];  loss fp64 [n_groups + 1, 2];  ratios fp32 [n_groups + 1, 2, 6] */
int gpe_framework_eval_pool(const double* table, const int32_t* group, long G, int n_groups, int64_t* totals, double* loss,
                            float* ratios, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPE_HIP_FRAMEWORK_H */
