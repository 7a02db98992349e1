/* Additions to the C ABI of libgpe_hip.so since version 7 (include/gpe_hip.h; gpe_abi_version() stays 7).  Same conventions as
 * the main header: row-major fp32, caller-owned memory, every compute entry point returns 0 / -22 (bad argument, checked before any
 * launch) / -5 (launch failure) and takes the HIP stream as its last argument.  The declarations here are folded into gpe_hip.h at
 * the next version bump; until then both headers are bound (gpe_amd/_lib.py) and both are seen by every definition
 * (csrc/gpe_common.h).
 *
 * ---- the guarded Adam step: clip by global norm, skip a bad step, per-parameter gradient norms — all on the device ----------------
 * (torch.nn.utils.clip_grad_norm_ + AMP's found_inf pattern for torch.optim.Adam over a flat arena; csrc/gpe_adam_guard.hip)
 *
 * The gradient arena g[0 .. n) is a sequence of nseg SEGMENTS (one per parameter), described by two device tables of int64:
 *   seg_end  [nseg]      end offset of segment j in floats; strictly increasing, every entry a multiple of 4 (so a 16-byte load never
 *                        straddles two segments; padding floats are zero), seg_end[nseg - 1] <= n.  Segment j = [seg_end[j-1], seg_end[j]).
 *   seg_slot [nseg + 1]  first SLOT of segment j.  A slot is a fixed range of 2048 floats counted from its segment's start; segment j owns
 *                        ceil(len_j / 2048) slots.  gpe_grad_norm_slots fills the host copy of this table from the host copy of seg_end.
 * The norm of a step is formed in two stages, neither of which uses atomics or lets one workgroup wait for another:
 *   gpe_grad_norm_part    one launch per RUN of live segments [seg_lo, seg_hi): part[s] = the sum of g^2 over slot s, in fp64, each
 *                         slot reduced by one workgroup in a fixed order (thread t takes the float4s t and t + 256 of the slot; lanes are
 *                         combined by a fixed shuffle tree, the four waves in wave order).  Which workgroup takes which slot depends on
 *                         the grid; what it computes does not — the result is bit-identical for every grid size and CU reservation.
 *   gpe_grad_norm_finish  one launch per step (one workgroup): the slots of every live segment are added (fixed order) to the segment's
 *                         sum of squares, the segment sums are added in segment order, and the guard block is written (below).
 * A segment that lies in none of the runs given to the finish is dead: norm 0, no contribution (torch skips parameters without .grad).
 *
 * The GUARD BLOCK is 32 bytes of caller-owned device memory, 16-byte aligned:
 *   byte  0  float   norm     the L2 norm of gscale * g over the live segments = the norm of the vector of segment norms
 *                             (clip_grad_norm_'s definition): fp64 sums, |gscale| * sqrt(sum) in fp64, rounded ONCE to fp32
 *   byte  4  float   coef     min(1, max_norm / (norm + 1e-6)) formed in fp64 from the fp32 norm and rounded to fp32; exactly 1.0f when
 *                             max_norm <= 0 (clipping off).  (A NaN quotient gives 1.0f.)
 *   byte  8  int32   skip     1 iff (nonfinite_skip != 0 and the fp32 norm is not finite) or any watched word is >= limit or NaN, else 0
 *   byte 12  int32   reserved (written as 0)
 *   byte 16  int64   steps    incremented once per finish launch
 *   byte 24  int64   skipped  incremented by `skip` per finish launch
 * Both counters are read-modify-written by one thread with ordinary vector stores: zero the block once, then leave it to the library.
 *
 * STEP NUMBERS.  A skipped step keeps its number: the caller advances its schedule slot and the bias-correction exponent as if the step
 * had been taken (the reference steps its OneCycleLR every batch regardless), and never reads the flag to rewind anything.  The step
 * after a skipped step t therefore runs with the scalars of step t + 1.
 */
#ifndef GPE_HIP_EXT_H
#define GPE_HIP_EXT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* host only: seg_slot_host[0 .. nseg] from seg_end_host[0 .. nseg) (both HOST arrays); returns the total number of slots
 * (= seg_slot_host[nseg] = the doubles `part` must hold), or -22 for NULL, nseg outside 1 .. 4096, or a table that is not
 * strictly increasing from a positive first entry in multiples of 4. */
long gpe_grad_norm_slots(const long* seg_end_host, int nseg, long* seg_slot_host);

/* part[s] = sum of g[i]^2 (fp64) over slot s, for every slot of the segments seg_lo .. seg_hi - 1.
 *   g        fp32 [n], 16-byte aligned: the WHOLE gradient arena (the tables hold absolute offsets); n > 0
 *   seg_end, seg_slot   device tables as above (8-byte aligned); 0 <= seg_lo < seg_hi <= nseg <= 4096
 *   part     fp64 [total_slots], 8-byte aligned; total_slots = what gpe_grad_norm_slots returned.  Slots of other segments are not touched.
 * Reads of g are clamped to [0, n) and writes of part to [0, total_slots) whatever the device tables hold.  A non-finite gradient gives
 * a non-finite slot sum (inf or NaN), which the finish carries into the norm. */
int gpe_grad_norm_part(const float* g, long n, const long* seg_end, const long* seg_slot, int nseg, int seg_lo, int seg_hi,
                       long total_slots, double* part, void* stream);

/* Completes the step's norm from `part` and writes the guard block.
 *   runs_host    HOST array of nruns pairs (seg_lo, seg_hi), 1 <= nruns <= 16, ascending and disjoint: the segment ranges
 *                gpe_grad_norm_part was launched on in this step (read during the call; a captured launch keeps the values)
 *   gscale       the factor the optimizer reads the gradient with (the norm is that of gscale * g)
 *   max_norm     clip threshold; <= 0 = no clipping (coef = 1.0f exactly)
 *   nonfinite_skip   0 / 1: set the skip flag when the fp32 norm is inf or NaN
 *   words_host   HOST array of nwords (0 .. 8) DEVICE pointers to 4-byte-aligned "amax words" (the fp32 bit pattern of a tensor's
 *                largest magnitude, as the f16x3 edge kernels write them; include/gpe_hip.h), may be NULL when nwords == 0;
 *                limit: the skip flag is set when a word's value is >= limit or NaN (fp16 activation storage: 65504)
 *   seg_norm     fp32 [nseg] or NULL: the L2 norm of gscale * g over each segment (0 for a dead segment), written at index j, or at
 *                nseg - 1 - j when reversed != 0 (optim.FlatArena keeps the parameters in reverse registration order)
 *   guard        the 32-byte guard block (16-byte aligned) */
int gpe_grad_norm_finish(const double* part, const long* seg_slot, int nseg, long total_slots, const int* runs_host, int nruns,
                         float gscale, float max_norm, int nonfinite_skip, const void* const* words_host, int nwords, float limit,
                         float* seg_norm, int reversed, void* guard, void* stream);

/* gpe_adam_step under a guard block (written by gpe_grad_norm_finish earlier on the same stream), same arguments otherwise:
 *   the effective gradient is g * gs + weight_decay * p with gs = gscale * coef formed once per thread — with coef == 1 the
 *   arithmetic of gpe_adam_step (p, m, v bit-equal to it, for every n and weight decay), with gscale == 1 torch's g.mul_(coef)
 *   followed by Adam;
 *   skip != 0: p, m and v are not modified; g is still cleared when zero_grad != 0.
 * `step` is the number of THIS step whether or not it is skipped (see STEP NUMBERS above). */
int gpe_adam_step_guarded(float* p, float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                          float weight_decay, long step, float gscale, int zero_grad, const void* guard, void* stream);
/* the same with the two step-dependent scalars read from the device pair `hyper` (gpe_adam_step_dev, gpe_adam_hyper) */
int gpe_adam_step_guarded_dev(float* p, float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2,
                              float eps, float weight_decay, float gscale, int zero_grad, const void* guard, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPE_HIP_EXT_H */
