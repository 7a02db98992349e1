/* Feeding training epochs from the device: additions to the C ABI of libgpe_hip.so (include/gpe_hip.h; gpe_abi_version() stays 7),
 * kept in a header of their own like include/gpe_hip_fit.h and with the same conventions: caller-owned memory, every compute entry
 * point returns 0 / -22 (bad argument, checked before any launch) / -5 (launch failure) and takes the HIP stream as its last
 * argument.  Bound by gpe_amd/_lib.py (FEED_HEADERS) and seen by every definition (csrc/gpe_common.h).  csrc/gpe_epoch_feed.hip.
 *
 * ---- the balanced batch schedule of one epoch (BalancedBatchSampler.__iter__, nn/data/utils.py:54-89) ------------------------------
 * The G garments of a split belong to C classes (garment types), given in CSR form: class c owns the positions class_off[c] ..
 * class_off[c + 1] - 1 of `ids`.  gpe_batch_schedule_draw writes the batches of one epoch as the rows of `table`; the image is a
 * function of (seed, epoch, class lists, quotas, B, drop_last) alone — bit-identical for every grid size and CU reservation.  No
 * workgroup waits for another: there are no arrival counters, no spinning and no atomics; what one launch hands to the next goes
 * through the workspace in stream order.
 *
 * Random numbers: one Philox4x32-10 block per decision, keyed by the seed, with the counter layout of every sampler of the library
 * (item | kind << 28, attempt | b << 8, epoch lo, epoch hi), attempt = 0.  A 64-bit KEY is word 0 of the block << 32 | word 1.
 *   kind 10  ORDER   item = position p of the garment in `ids`, b = 0            -> key of the garment
 *   kind 11  FILL    item = batch t, b = pre-shuffle slot j                      -> word 0 chooses the class of a free slot
 *   kind 12  SLOT    item = batch t, b = pre-shuffle slot s                      -> key of the slot
 * below(word, n) = (uint64(word) * n) >> 32, an integer in [0, n).
 *
 *   order inside a class   the garments of a class sorted ascending by (key, position); the class is consumed from the front (the
 *                          reference pops from the end of a uniform shuffle: the same distribution)
 *   batch t < G / B        the classes are visited in order and class c gives min(quota[c], what it has left) garments (the
 *                          reference's `break` on an exhausted class); then each free slot j = len .. B - 1, in order, takes the
 *                          next garment of the class number below(word, n) among the n classes that still have garments, counted
 *                          in class order
 *   slot shuffle           pre-shuffle slot s goes to the rank of (key, s) among the slots of the batch
 *   kept remainder         drop_last == 0 and G % B != 0: one more row holds every garment left, in class order, shuffled by the
 *                          same rule among its G % B slots and padded with -1
 * Quotas are the caller's: the reference's int((len_c / G) * B), evaluated in double on the host (it differs from len_c * B / G in
 * integers: 13 of 23 garments at B = 23 give 12).
 *
 * Launches per epoch: three.  (1) ranking: a thread per garment counts the smaller keys of its class, the keys of 256 positions at
 * a time recomputed into LDS (quadratic in the largest class: meant for data sets of tens of thousands of garments);
 * (2) the walk over the batches, which keeps the per-class fill counts: ONE wave; it reads {seed, epoch}, leaves a copy in the
 * workspace for (3) and, as its last store, writes epoch + 1 — nothing else runs then, so the update cannot race with a reader;
 * (3) the slot shuffle, a workgroup per row.
 *
 * ---- the per-step feed ---------------------------------------------------------------------------------------------------------------
 * gpe_feed_next hands the next row of the schedule to the step and gathers the ground truth of its garments from resident tables.
 * Legal in a stream capture: everything a replay needs is read from device memory.  Two launches per step:
 *   prologue   ONE workgroup reads cursor, copies row cursor % rows of `table` to index_out, counts the entries outside 0 .. G - 1
 *              (-1 pads a kept remainder) into status[0] and, as its last store, writes cursor + 1.  It is the only reader and the
 *              only writer of cursor, so the update cannot race.
 *   gather     workgroup (b, j) copies row index_out[b] of resident table j to row b of that table's output: 16-byte vector copies
 *              when row_bytes and both addresses are multiples of 16, 4-byte copies otherwise; a row of zeros for an entry outside
 *              0 .. G - 1.
 * The tables are described by a JOB ARRAY in device memory, built once on the host by gpe_feed_jobs (which checks it) and uploaded
 * by the caller: per table three int64 words {src, dst, row_bytes}.
 */
#ifndef GPE_HIP_FEED_H
#define GPE_HIP_FEED_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GPE_FEED_MAX_TABLES 16
#define GPE_SCHEDULE_MAX_GARMENTS (1 << 20)
#define GPE_SCHEDULE_MAX_BATCH 1024

/* host only: the rows of a schedule = G / B, plus one when drop_last == 0 and G % B != 0; -22 unless 1 <= G <= 2^20 and
 * 1 <= B <= 1024 */
long gpe_batch_schedule_rows(long G, int B, int drop_last);

/* host only: the bytes of the workspace of gpe_batch_schedule_draw for G garments (16-byte aligned by the caller); -22 unless
 * 1 <= G <= 2^20 */
long gpe_batch_schedule_ws_bytes(long G);

/* One epoch's schedule.
 *   class_off       int32 [C + 1] on the device, class_off[0] = 0, non-decreasing, class_off[C] = G
 *   ids             int32 [G] on the device: the garments, in class order
 *   quota           int32 [C] on the device
 *   class_off_host, quota_host    the same two arrays in host memory: what the argument checks read
 *   state           int64 [2] on the device, 8-byte aligned: {seed, epoch}; epoch is advanced by one
 *   ws, ws_bytes    gpe_batch_schedule_ws_bytes(G) bytes on the device, 16-byte aligned
 *   table           int32 [rows, B], batch_len int32 [rows] on the device, rows = gpe_batch_schedule_rows(G, B, drop_last)
 * -22: a NULL pointer, G outside 1 .. 2^20, B outside 1 .. 1024, C < 1 or C > B (the reference raises NotImplementedError there),
 * class offsets that are not as above, a negative quota, a quota sum above B, drop_last not 0 / 1, a workspace that is too small
 * or misaligned. */
int gpe_batch_schedule_draw(const int32_t* class_off, const int32_t* ids, const int32_t* quota, const int32_t* class_off_host,
                            const int32_t* quota_host, int C, int G, int B, int drop_last, int64_t* state, void* ws, long ws_bytes,
                            int32_t* table, int32_t* batch_len, void* stream);

/* host only: checks the T tables of a feed and writes their job array (int64 [T, 3] = {src, dst, row_bytes}) into HOST memory at
 * jobs_host; the caller uploads it.  src[j] / dst[j]: device addresses of resident table j ([G, row_bytes[j]] bytes) and of its
 * output ([B, row_bytes[j]] bytes), 4-byte aligned.  -22: NULL, T outside 1 .. 16, a row_bytes that is not a positive multiple of 4
 * or exceeds 2^24, a NULL or misaligned table address. */
int gpe_feed_jobs(int T, const void* const* src, void* const* dst, const long* row_bytes, int64_t* jobs_host);

/* The next batch: index_out int32 [B] = row cursor % rows of table (int32 [rows, B]); output j row b = resident row index_out[b] of
 * table j; cursor (int64 [1] on the device, 8-byte aligned) advanced by one; status int32 [1] = the entries of the row outside
 * 0 .. G - 1, whose output rows are zeros.
 *   jobs            int64 [T, 3] on the device (gpe_feed_jobs), 8-byte aligned; T = 0 feeds the index alone (jobs may be NULL)
 *   max_row_bytes   the largest row_bytes of the jobs (sizes the gather's workgroups; rows above it are still copied whole)
 * -22: a NULL pointer, rows < 1, B outside 1 .. 1024, G < 1, T outside 0 .. 16, max_row_bytes not a positive multiple of 4 when
 * T > 0, a misaligned cursor or job array. */
int gpe_feed_next(const int32_t* table, long rows, int B, int64_t* cursor, int G, const int64_t* jobs, int T, long max_row_bytes,
                  int32_t* index_out, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPE_HIP_FEED_H */
