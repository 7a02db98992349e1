/* Prediction from raw scans: additions to the C ABI of libgpe_hip.so (include/gpe_hip.h; gpe_abi_version() stays 7), kept in a header
 * of their own like include/gpe_hip_feed.h and with the same conventions: caller-owned memory, every compute entry point returns
 * 0 / -22 (bad argument, checked before any launch) / -5 (launch failure) and takes the HIP stream as its last argument.  Bound by
 * gpe_amd/_lib.py (SCAN_HEADERS) and seen by every definition (csrc/gpe_common.h).  csrc/gpe_scan_sample.hip.
 *
 * What nn/evaluation_scripts/predict_per_example.py does per scan on the host (load_points, np.random.permutation(n)[:mesh_samples],
 * (p - f_shift) / f_scale, stack), for a whole batch of scans that stay in device memory.
 *
 * ---- the resident set ---------------------------------------------------------------------------------------------------------------
 * G clouds, concatenated: points4 fp32 [T, 4] = {x, y, z, 0} (16-byte aligned), off int32 [G + 1], off[0] = 0, non-decreasing,
 * off[G] = T; cloud g owns the rows off[g] .. off[g + 1] - 1, n_g of them, n_g < 2^28 (the generator's item field).  n_max: the size
 * of the largest cloud, known to the caller; it sizes the grids, and a cloud is read up to its first n_max points.
 *
 * ---- the draw rule ------------------------------------------------------------------------------------------------------------------
 *   keys         slot b of a call draws cloud g = index[b].  Point i of that cloud gets the 64-bit key (w0 << 32) | w1 of the
 *                samplers' Philox4x32-10 block (include/gpe_hip_feed.h: counter (item | kind << 28, attempt | b << 8, draw lo, draw hi),
 *                keyed by the seed) of kind 13, item i, attempt 0, under the call's {seed, draw} and slot b
 *   order        the points ordered by (key, i) ascending; output row r < N is the point of rank r.  In distribution this is
 *                np.random.permutation(n)[:N]: a uniform N-subset in uniform order
 *   short cloud  n < N: row r takes the point of rank r mod n (whole permutations repeat); status[b] = N - n, the repeated rows
 *                (0 when n >= N)
 *   bad slot     n = 0: status -1; index[b] outside 0 .. G - 1: status -2.  The slot's rows are zeros and its `picked` are -1
 *   outputs      features fp32 [B, N, 3] = (p - shift) / scale, the fp32 subtract-then-divide of gpe_standardize (p itself without
 *                statistics); picked int32 [B, N]: the point's index inside its cloud; status int32 [B]
 *   state        {seed, draw} and the ticket word as in gpe_mesh_points_sample: every call advances draw by one on the device through
 *                the last-arriver ticket, so a captured call draws anew on every replay
 * The result is a function of (seed, draw, b, data) alone: the order comes from a sort by (key, i), never from the order in which
 * atomics land, and no grid size or CU reservation shows.
 *
 * ---- the passes (a radix select on keys that are never stored: every pass recomputes them from i) -------------------------------------
 * One memset of the counters, then three launches in stream order; no workgroup waits for another.
 *   histogram    workgroup (b, c) counts the leading 11 key bits of 4096 points of its cloud in LDS and adds the bins it met to the
 *                slot's table (integer atomics); every workgroup reads the state, the last arriver advances it
 *   collect      every workgroup finds the bin T where the running count crosses N; (key, i) of every point below T is appended
 *                to the slot's candidate list, and those of bin T too when they fit (below + count(T) <= 4096 entries)
 *   finish       ONE workgroup per slot.  Candidates listed: sorts them by (key, i) in LDS.  A boundary bin too full to list: the
 *                workgroup narrows it by itself, 11 / 11 / 10 bits of (key hi, key lo, i) per pass over the cloud, until the N-th
 *                smallest (key, i) is known or the prefix holds exactly what is missing, collects the N points at or below it and
 *                sorts them — slower (one workgroup walks the cloud), never truncated.  n <= N: sorts the whole cloud.  Then
 *                gathers, standardises and writes.
 * N <= 2048 (the sort's LDS image holds 4096 entries).  The boundary bin holds n / 2048 points on average, so clouds up to about two
 * million points take the listed path at N = 2000.
 *
 * ---- labels back onto the scan ---------------------------------------------------------------------------------------------------------
 * gpe_scan_labels: for every point of every cloud named by a valid slot (index inside the set, n >= 1), the nearest of the slot's N
 * drawn points in raw coordinates — d = (dx dx + dy dy) + dz dz, each operation rounded on its own, the lexicographic minimum of
 * (d, row): the rule of gpe_mesh_points_sample's label scan — and then the arg-max over P of that row's attention weights, the first
 * maximum winning, written to labels[off[g] + i].  Rows of clouds not named by the batch are not touched; a slot with index outside
 * the set or an empty cloud writes nothing; a row whose `picked` lies outside 0 .. n - 1 is never the nearest.  If two slots name the
 * same cloud, the higher slot's labels stand (the lower slot writes nothing).  One launch.
 */
#ifndef GPE_HIP_SCAN_H
#define GPE_HIP_SCAN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GPE_SCAN_MAX_SAMPLES 2048
#define GPE_SCAN_MAX_POINTS ((1 << 28) - 1)
#define GPE_SCAN_MAX_BATCH ((1 << 24) - 1)

/* host only: the bytes of the workspace of gpe_scan_sample for B slots of N samples from clouds of at most n_max points (16-byte
 * aligned by the caller): 16 (the call's copy of the state) + 4 B rounded up to 16 (the list lengths) + B * 2048 * 4 (the tables) +
 * B * 4096 * 16 (the candidate lists {key hi, key lo, i, 0}).  -22 unless 1 <= B < 2^24, 1 <= N <= 2048, 1 <= n_max < 2^28 */
long gpe_scan_sample_ws_bytes(long B, int N, long n_max);

/* One batch of model clouds.
 *   points4, off, G, n_max     the resident set (above), on the device
 *   index                      int32 [B] on the device
 *   shift_host, scale_host     3 floats each in host memory, or both NULL
 *   narrow_above               0: the boundary bin is listed whenever it fits.  > 0: it is listed only when it holds at most that
 *                              many points as well — a smaller value sends smaller clouds down the narrowing path (what the tests
 *                              do); the result does not depend on it
 *   ws, ws_bytes               gpe_scan_sample_ws_bytes(B, N, n_max) bytes on the device, 16-byte aligned
 *   state                      uint64 [2] on the device, 8-byte aligned: {seed, draw}; draw is advanced by one
 *   ticket                     one zeroed uint32 on the device, left zero
 * -22: a NULL pointer (the statistics: one of the two), points4 or ws not 16-byte aligned, state not 8-byte aligned, G < 1,
 * B outside 1 .. 2^24 - 1, N outside 1 .. 2048, n_max outside 1 .. 2^28 - 1, narrow_above < 0, a workspace that is too small. */
int gpe_scan_sample(const float* points4, const int32_t* off, int G, long n_max, const int32_t* index, int B, int N,
                    const float* shift_host, const float* scale_host, int narrow_above, void* ws, long ws_bytes, uint64_t* state,
                    uint32_t* ticket, float* features, int32_t* picked, int32_t* status, void* stream);

/* The predicted per-point panel labels handed back to every point of the scans of a batch.
 *   picked        int32 [B, N]: the second output of gpe_scan_sample for the same index
 *   att_weights   fp32 [B, N, P], 1 <= P <= 4096
 *   labels        int32 [T], resident-sized; only the rows of the clouds named by valid slots are written
 * -22: a NULL pointer, points4 not 16-byte aligned, G < 1, B outside 1 .. 2^24 - 1, N outside 1 .. 2^28 - 1, P outside 1 .. 4096,
 * n_max outside 1 .. 2^28 - 1. */
int gpe_scan_labels(const float* points4, const int32_t* off, int G, long n_max, const int32_t* index, int B, int N,
                    const int32_t* picked, const float* att_weights, int P, int32_t* labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPE_HIP_SCAN_H */
