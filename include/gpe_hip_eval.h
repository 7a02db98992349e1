/* Feature additions to the C ABI of libgpe_hip.so (include/gpe_hip.h; gpe_abi_version() stays 7): evaluating a model over a data
 * set without a host read per batch (csrc/gpe_eval.hip; the reference's nn/metrics/eval_utils.py:35-76).  The conventions are those
 * of include/gpe_hip_fit.h: caller-owned memory, every entry point returns 0 / -22 (bad argument, checked before any launch and before
 * any pointer is touched) / -5 (launch failure) and takes the HIP stream as its last argument.  Bound by gpe_amd/_lib.py
 * (EVAL_HEADERS) and seen by every definition (csrc/gpe_common.h).
 *
 * ---- the reference's aggregation rule --------------------------------------------------------------------------------------------
 * _eval_metrics_per_loader keeps one Python list per key, appends a batch's value unless it is None, and returns
 * sum(list) / len(list), or None for an empty list.  The values are 0-d float32 numpy arrays, so the sum is a sequential fp32 add in
 * batch order.  gpe_eval_add is that append: one launch per batch, one wave, lane k owns key k —
 *     sum[slot, k] = sum[slot, k] + value_k       (one individually rounded fp32 add; a NaN or inf is added like any value)
 *     cnt[slot, k] += 1
 * both only where the key is COUNTED, and batches[slot] += 1.  Plain loads and stores, no atomics: launches on one stream are the
 * batch order.  The division is the caller's, on the host, after its one read: float32(sum) / float32(cnt), None where cnt == 0.
 *
 * A KEY is a packed int32 of the host array `keys_host` (copied into the launch's arguments: the array may be reused at once):
 *     bits 0..7    index of the value inside its source vector
 *     bits 8..9    source vector 0..3
 *     bits 16..18  gate: 0 = always counted; j + 1 = counted iff counts[j] > 0 (counts: the int32 [4] contributor counts of
 *                  gpe_quality_finalize; a gated key needs counts != NULL)
 * The row `slot` is read from DEVICE memory, so that one captured launch serves every row (one row per data folder).  A slot word
 * outside 0 .. slots-1 sets status[0] = 1 and adds nothing.
 *
 * ---- pooling the per-garment records of a whole set ------------------------------------------------------------------------------
 * gpe_eval_pool folds a table of the quality kernels' per-pattern records (16 doubles per garment, the layout gpe_quality_panels /
 * gpe_quality_stitches write) per group and overall.  Row g of the result is BIT FOR BIT what gpe_quality_finalize returns for the
 * garments of group g alone, in table order, as one batch; row n_groups is that for all G garments.  The order of the adds and the
 * number type of every sum are those of gpe_quality_final_kernel (csrc/gpe_quality_fold.h holds the one statement of both).
 * One wave per output row: the wave fetches 64 records at a time, coalesced, into LDS, and one lane consumes them in order.  A group
 * without garments gives zero counts and the float slots of a 0 / 0 (NaN where the finalise kernel divides by a count).
 */
#ifndef GPE_HIP_EVAL_H
#define GPE_HIP_EVAL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GPE_EVAL_MAX_KEYS 64
#define GPE_EVAL_MAX_SOURCES 4

/*   src0..3, n0..3   the source vectors (fp32, device) and their lengths; sources n_sources .. 3 are ignored; a source no key
 *                    refers to may be NULL with length 0; 0 <= n_sources <= 4, lengths 0 .. 256
 *   counts           int32 [4] (device) or NULL when no key is gated
 *   keys_host, K     K packed keys (HOST memory), 1 <= K <= 64; every key's source < n_sources, index < that source's length
 *   sum, cnt         fp32 / int32 [slots, K];  batches int32 [slots];  slots >= 1
 *   slot             int32 [1] (device): the row this batch belongs to
 *   status           int32 [1] (device): set to 1 when the slot word is out of range, untouched otherwise */
int gpe_eval_add(const float* src0, int n0, const float* src1, int n1, const float* src2, int n2, const float* src3, int n3,
                 int n_sources, const int32_t* counts, const int32_t* keys_host, int K, float* sum, int32_t* cnt, int32_t* batches,
                 const int32_t* slot, int slots, int32_t* status, void* stream);

/*   table      fp64 [G, 16] (device), G >= 1
 *   group      int32 [G] (device) or NULL (then n_groups must be 0); an id outside 0 .. n_groups-1 belongs to no group but still
 *              counts in the last row
 *   n_groups   0 .. 65535
 *   P, L       panels per pattern, edges per panel (> 0): the denominators of the finalise kernel
 *   flags      the QM_* component bits of gpe_quality_finalize (0 .. 127)
 *   out        fp32 [n_groups + 1, 14];  counts int32 [n_groups + 1, 4] */
int gpe_eval_pool(const double* table, const int32_t* group, long G, int n_groups, int P, int L, int flags, float* out,
                  int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPE_HIP_EVAL_H */
