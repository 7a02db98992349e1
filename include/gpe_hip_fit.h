/* Feature additions to the C ABI of libgpe_hip.so (include/gpe_hip.h; gpe_abi_version() stays 7), kept in a header of their own
 * like include/gpe_hip_ext.h and with the same conventions: row-major fp32 input, caller-owned memory, every compute entry point
 * returns 0 / -22 (bad argument, checked before any launch) / -5 (launch failure) and takes the HIP stream as its last argument.
 * Bound by gpe_amd/_lib.py (FEATURE_HEADERS) and seen by every definition (csrc/gpe_common.h).
 *
 * ---- fitting the standardisation statistics of a resident data set on the device ------------------------------------------------
 * (GarmentBaseDataset._get_distribution_stats / _get_norm_stats / _unpad, nn/data/datasets.py:524-568; csrc/gpe_fit_stats.hip)
 *
 * The input is x: fp32, contiguous, [S, N, C] — S SETS of N rows with 1 <= C <= 16 columns.  A LEAF is a block of 512 consecutive
 * rows inside one set (the last leaf of a set holds the remainder); set s owns the leaves s * ceil(N / 512) + b.  The split into
 * leaves depends on (S, N) alone.  The statistics are formed in two stages, neither of which uses atomics or lets one workgroup
 * wait for another, and every sum is fp64 in a fixed order:
 *   gpe_fit_part     one RECORD per leaf, each leaf reduced by the waves of one workgroup (one wave for C <= 4, two for C <= 8, four
 *                    above): the leaf mean first, then the squared deviations from it (the leaf sits in registers, so the second
 *                    pass costs no memory traffic).  Which workgroup takes which leaf depends on the grid; what it computes does
 *                    not — the image is bit-identical for every grid size, CU reservation and chunking of the sets over calls.
 *                    Order (CP = C rounded up to a power of two, W = the leaf's waves): thread t of 64 W holds column t % CP of the
 *                    rows t / CP + k * (64 W / CP), summed in the order of k; the threads of a column are combined by a fixed
 *                    shuffle tree inside each wave (lane l with lane l + 32, 16, ... CP), the waves in wave order.
 *   gpe_fit_finish   one workgroup merges the records in a fixed order by Chan's pairwise update
 *                        d = mean_b - mean_a;  mean = mean_a + d n_b / n;  M2 = M2_a + M2_b + d^2 n_a n_b / n        (n = n_a + n_b)
 *                    and writes the RESULT BLOCK.  Order: thread t of 1024 works on column t % CP and folds the leaves t / CP,
 *                    t / CP + 1024 / CP, ... in that order; the threads of a column are combined by the same shuffle tree inside
 *                    each wave, the 16 waves in wave order.  A record with n = 0 is skipped.
 * min / max are IEEE 754-2019 minimum / maximum: a NaN is carried on and -0 < +0, so the sign of a zero extreme does not depend on
 * the order of the rows.
 *
 * RECORD (1 + 4 C doubles, leaf i at part + i * (1 + 4 C)):
 *   [0]                 n     rows of the leaf that were kept
 *   [1 + 4 c + 0]       mean  of column c over the kept rows (0 when n = 0)
 *   [1 + 4 c + 1]       M2    sum of (x - mean)^2 over the kept rows (0 when n = 0)
 *   [1 + 4 c + 2], [3]  min, max of column c over the kept rows (+inf, -inf when n = 0); both NaN when the column holds a NaN
 * skip_zero_rows != 0 drops a row iff fabsf(x) <= 1e-5f in every column: _unpad's isclose(x, 0, atol = 1e-5), whose rtol term
 * vanishes against 0.
 *
 * RESULT BLOCK (2 + 5 C doubles):
 *   [0]             n           rows kept over all leaves
 *   [1]             status      bit 0: no row left (n == 0) — every other entry but n is NaN; bit 1: a non-finite input was seen
 *   [2 + c]         mean
 *   [2 + C + c]     std         sqrt(M2 / n), the population form of :544-545; exactly 0 when min == max (the reference gives 0
 *                               there, a merged M2 may not); a negative merged M2 counts as 0
 *   [2 + 2 C + c]   min
 *   [2 + 3 C + c]   max
 *   [2 + 4 C + c]   norm_scale  the rule of :562-566 on the fp32 values tmin = min, tmax = max, evaluated in fp64:
 *                               |tmin - tmax| <= 1e-8 + 1e-5 |tmax|  ->  tmin, or 1 when |tmin| <= 1e-8;  otherwise tmax - tmin
 *                               (rounded to fp32 ONCE by the caller: the reference's fp32 subtraction, both correctly rounded)
 * A NaN in a column makes that column's mean, std, min, max and norm_scale NaN, as torch.min / torch.max propagate it.
 */
#ifndef GPE_HIP_FIT_H
#define GPE_HIP_FIT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* host only: the leaves of `sets` sets of `rows_per_set` rows = sets * ceil(rows_per_set / 512) (the records `part` must hold), or
 * -22 when an argument is not positive or the product does not fit a long. */
long gpe_fit_leaves(long sets, long rows_per_set);

/* One record per leaf of x, written at leaf index leaf0 + s * ceil(rows_per_set / 512) + b.
 *   x        fp32 [sets, rows_per_set, C], contiguous, 4-byte aligned; 1 <= C <= 16; sets * rows_per_set * C fits a long
 *   leaf0    first record of this call: a data set handed in as chunks of whole sets gives the image one call would give
 *            (leaf0 = the leaves of the sets before the chunk)
 *   part     fp64 [total_leaves, 1 + 4 C], 8-byte aligned; 0 <= leaf0 and leaf0 + gpe_fit_leaves(sets, rows_per_set) <= total_leaves.
 *            Records of other leaves are not touched. */
int gpe_fit_part(const float* x, long sets, long rows_per_set, int C, int skip_zero_rows, long leaf0, long total_leaves,
                 double* part, void* stream);

/* Merges the records 0 .. leaves - 1 of `part` (fp64 [leaves, 1 + 4 C], 8-byte aligned, leaves >= 1) and writes the result block
 * `result` (fp64 [2 + 5 C], 8-byte aligned).  One workgroup. */
int gpe_fit_finish(const double* part, long leaves, int C, double* result, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPE_HIP_FIT_H */
