/*
 * libgpe_hip.so — C ABI of the MI355X (gfx950) encoder/decoder hot path.
 *
 * The reference (maria-korosteleva/Garment-Pattern-Estimation) has no FFI: its "plugin API" is class-name
 * lookup from YAML (nn/train.py:120, nn/nets.py:100,106,116).  The Python modules in
 * garment-pattern-estimation_amd/ keep that surface; underneath them every tensor op of the path is one of the
 * entry points below.  Each entry point names the reference line(s) whose arithmetic it replaces.
 *
 * Conventions (all functions):
 *   - plain C symbols; raw DEVICE pointers + dims + a hipStream_t passed as void*; the caller owns EVERY buffer — outputs,
 *     workspaces (`part`, `ws`: sizes from the gpe_*_ws* queries) and the f16x3 scale words below; the library never allocates
 *     device memory and keeps no record of tensors between calls.  Work is enqueued on `stream` of the CURRENT device and the
 *     call returns immediately.  Calls on different streams may run concurrently as long as they share no output / workspace.
 *     Process-global state is limited to (a) the arithmetic mode (gpe_math_set, gpe_f16x3_min_rows_set), the profiling
 *     switches (gpe_debug_set) and the CU reservation (gpe_reserve_cus_set), which apply to every stream and device of the
 *     process, and (b) per-device caches of the CU count and of the >64 KB LDS opt-in (hipFuncSetAttribute), keyed by device
 *     ordinal.  The mode setters are not thread-safe against concurrent launches; everything else is.
 *   - "amax word" (f16x3 mode): a uint32 in device memory holding the bit pattern of a non-negative float that is >= the
 *     largest magnitude of a tensor (a bound is as good as the value; tighter = more precise).  An entry point that writes an
 *     activation / dz tensor fills the word passed as `amax_out` (whatever kernel ran: if it could not track the maximum while
 *     storing, one extra streaming pass measures it); an entry point that reads the tensor through the fp16 pipe takes the word
 *     as `amax_a` / `amax_u` / `amax_v`.  All of them may be NULL: nothing is measured / the operand is measured in-call (edge
 *     GEMMs) or the exact fp32 kernel runs (reduce-GEMM).  The caller vouches for the words it passes: a word that is too small
 *     for its tensor overflows fp16 silently.  Modes other than f16x3 ignore `amax_a/u/v` and honour `amax_out`.
 *   - return 0 on success, -22 (EINVAL) on bad arguments, -5 (EIO) if the launch failed;
 *   - fp32 storage and arithmetic unless stated; matrix products run on v_mfma_f32_16x16x4_f32 (exact fp32);
 *     BatchNorm statistics are accumulated in fp64;
 *   - "ld" = leading dimension in elements; "packed weight" = the layout produced by gpe_pack_weight.
 */
#ifndef GPE_HIP_H
#define GPE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* version / capability probe (host only, no GPU needed) */
int gpe_abi_version(void);
/* profiling aid: ablation switches for the fused edge kernels (0 = production behaviour; results are WRONG otherwise, except
 * bit 512, which only makes gpe_edge_lazy_dz3_ok answer 0 — the eager in-place dz3 pass, same results to rounding) */
int gpe_debug_set(int flags);
int gpe_debug_get(void);
/* Multi-GPU: leave n compute units (0 .. 192; use a multiple of 8 = whole CUs per XCD, which keeps the cloud -> XCD pinning on) out
 * of every persistent launch.  The fused edge kernels, the reduce-GEMMs and the persistent LSTM size their grids to "one workgroup
 * per CU" and hold 100 - 160 KB of LDS each for the whole launch: with nothing reserved, a collective's kernel queued on another
 * stream (RCCL's all-reduce of a gradient bucket, launched from inside backward: garment-pattern-estimation_amd/parallel.py) only
 * gets onto the chip when one of them retires — the "overlap" degenerates into waiting at kernel boundaries.  Process-global like the
 * arithmetic mode; returns the previous reservation, -22 for a bad n.  Results are not bit-identical across reservations (the
 * order of the partial sums and the choice of kernel change with the grid), but parity with the oracle holds at every reservation
 * (tests/test_gpu_grid_sizes.py). */
int gpe_reserve_cus_set(int n);
/* arithmetic of the fused per-edge GEMMs (gpe_edge_mlp_fwd / gpe_edge_mlp_bwd / gpe_edge_redgemm):
 *   0 = "f32"    exact fp32 matrix instruction (v_mfma_f32_16x16x4_f32)
 *   1 = "bf16x3" split-bf16: every fp32 operand x = hi + lo (two bf16), a*b ~= ah*bh + ah*bl + al*bh on the bf16 matrix
 *                pipe with fp32 accumulation (relative error ~1e-5 per product instead of ~1e-7).
 *   2 = "mixed"  split-bf16 for the per-edge ROW GEMMs (forward and the input-gradient half of backward, whose
 *                rounding errors are independent per element and average out), exact fp32 for the weight-gradient
 *                reduce-GEMM  G = dz^T (a - mean): G also feeds the BatchNorm-backward coefficients, residuals of large
 *                sums where a coherent 1e-5 product error would surface as a 1e-2 gradient error.
 *   3 = "bf16x6" THREE-term split x = h + m + l, six bf16 MFMAs per product (every term down to 2^-24 except m*l, l*m,
 *                l*l) for the row GEMMs whose shape fits the register file (10 output tiles; the others stay on the exact
 *                fp32 instruction); reduce-GEMM exact fp32.  PARITY-GRADE (meets the exact mode's bars in every test once the
 *                oracle stands on the build's ReLU / argmax decisions), measured 0.5 % faster than mode 0.
 *   4 = "f16x3"  TWO-term fp16 split of operands normalised per TENSOR by a power of two (largest magnitude -> [2^14, 2^15)),
 *                three fp16 MFMAs per product, fp32 accumulate: 23 mantissa bits per product, PARITY-GRADE (every test at the
 *                exact mode's bars; profiles/r03_i_f16x3_grad_errors.md).  All four shapes of the shipped edge MLPs stay
 *                resident (two weight planes); the weight-gradient reduce-GEMMs join when the caller passes both operand words.
 *                The scales come from caller-owned amax words (see Conventions): the packed weight is measured in-call (one
 *                workgroup), activations / dz tensors by the kernel that stores them, the gathered operand by a bound over the
 *                [P|Q] table (gpe_edge_pq_amax, or in-call).  Launches with fewer than gpe_f16x3_min_rows() rows run the exact
 *                kernels (the scale passes cost more than the fp16 pipe saves there).  The mode bench.py times.
 *                Mode 4 also (since round 4): the FORWARD gate products of the recurrences (gpe_rnn_seq_fwd with plane packs:
 *                state rows scaled by 2^12 — start states must stay below 16 in magnitude, the Python side checks) and, where
 *                the caller asks for it (out_half of gpe_edge_mlp_fwd), fp16 STORAGE of the aggregated block's activation:
 *                rows clamped at 65504, positives below 6e-8 flushed — the forward still reports the activation's true
 *                largest magnitude in amax_out, and a caller must not keep the fp16 copy when that word reaches 65504
 *                (gpe_amd.ops.set_half_act_guard does this on the Python side).  For k = 16 at the shipped widths (200 / 200 /
 *                150) the four edge launches run the two-waves-per-SIMD kernel (gpe_edgegemm_w8_kernel.h), else the
 *                single-role one.
 * Returns the previous mode, or -22 for an unknown one.  The kNN result is exact in every mode (its FILTER runs on fp16 planes
 * in every mode, followed by an exact fp32 recheck); BatchNorm statistics, the backward recurrences and every elementwise op
 * are fp32 (fp64 for reductions) in every mode. */
int gpe_math_set(int mode);
int gpe_math_get(void);
/* f16x3 size gate (part of the arithmetic mode): edge launches with fewer rows use the exact fp32 kernels.  Default 32768 (round 5: with the two-waves-per-SIMD kernels BASELINE cfg 1 — 40 960 edges — is faster on the fp16 pipe: kernel time 3.56 -> 3.48 ms per step; it was 65536 before);
 * the setter returns the previous value (tests set 0 to force the fp16-pipe kernels on small fixtures). */
long gpe_f16x3_min_rows(void);
long gpe_f16x3_min_rows_set(long rows);

/* ---- kNN graph: torch_cluster.knn as called by DynamicEdgeConv (nn/net_blocks.py:127-135,174) ------------
 * x [B][N][ldx>=C]; idx [B][N][k] int32, LOCAL to the cloud, ascending (dist, index); self included.
 * dist = fp32 fma chain over channels of (x_c - y_c)^2, ties -> lower index (same rules as oracle/knn_ref.c).
 * Limits: 1 <= k <= min(64, N) (the k-list of a query lives one entry per lane of its wavefront; torch_cluster's own device
 * kernel stops at k = 100, the reference's configurations use k = 5 .. 20), B*N*k < 2^31; anything else returns -22. */
long gpe_knn_ws_bytes(int B, int N, int C, int k);
int gpe_knn(const float* x, int B, int N, int C, int ldx, int k, int32_t* idx, int32_t* idx_glob, const int32_t* order_in,
            int32_t* order_out, void* ws, long ws_bytes, void* stream);
/* order_out (may be NULL) [B][N] int32: a LOCALITY ORDER of every cloud's points — position r of the order holds point
 * order_out[b][r].  The xyz search (C = 3) writes the Morton-curve order its sorted scan works in; every other path writes the
 * identity.  order_in (may be NULL): any permutation per cloud, taken as a hint by the matrix-pipe filter (16 <= C <= 256): it
 * lays its fp16 planes out in that order and starts every query tile's scan one tile before the queries' own tile — when the
 * order is spatially coherent (the second EdgeConv layer hands over the first layer's curve order: points that are close in
 * space are close in feature space) the first three tiles hold almost all true neighbours, the insertion bound is tight for
 * the rest of the scan and the ordered-list work of the filter drops (cfg 2, layer 2: 815 -> 699 us per search).  The RESULT
 * does not depend on the hint: idx is in point numbering, exact, for any permutation (tests/test_gpu_kernels.py). */
/* idx_glob (may be NULL) [B][N][k] = b*N + idx: the GLOBAL row of each neighbour, which is what the gather kernels
 * below take as `jg` (B*N*k must be < 2^31).  ws: gpe_knn_ws_bytes(B, N, C, k) bytes, 16-B aligned (squared norms, per-cloud
 * maxima, candidate lists of the matrix-pipe filter / of a split candidate range; for C = 3 the spatially sorted copy of the
 * clouds and its tile boxes); NULL or too small: the all-exact all-pairs kernel without candidate split runs (same result, slower).
 * Paths (all produce the identical, defined result): C = 3 and 128 <= N <= 8192 — the cloud sorted along a Morton curve and
 * scanned tile by tile with an exact box bound that prunes tiles (gpe_knn3.hip; GPE_KNN_SORTED=0 disables); C >= 16 and
 * k <= 48 — a matrix-pipe filter + exact recheck (C <= 256: on the fp16 pipe, as a threshold scan for C <= 160 and k <= 32, else
 * with ordered lists; C > 256: on the fp32 pipe); otherwise the all-pairs VALU kernel.  The whole ladder: csrc/gpe_knn_plan.h. */
/* Which kernels a gpe_knn call runs, and the numbers of its plan.  Added without a version bump (gpe_abi_version() stays 7): one
 * host-only query, nothing else changes.  HOST ONLY: x and ws are looked at for NULL and for their alignment and never followed, no
 * HIP call is made beyond the CU count (256 without a GPU, less gpe_reserve_cus_set) and nothing is allocated; gpe_knn takes its
 * plan from the same function.  idx counts as given; has_idx_glob / has_order_in / has_order_out: that pointer is not NULL.
 * switches: NULL = this process's GPE_KNN_* measurement switches (read under GPE_DEBUG=1), else ten ints in the order
 *   PROBE, PIN, VEC, SPLIT, EXACT, F32FILTER, SORTED, NOORDER, FT, RR2      (defaults 0, -1, 0, 0, 0, 0, 1, 0, 1, 1)
 * Returns -22 where gpe_knn refuses the call, 0 for B == 0 (nothing is launched), else the path:
 *   1 sorted cloud (xyz)   2 all-pairs   3 threshold scan + recheck   4 ordered lists + recheck   5 fp32 filter + recheck
 * plan_out (may be NULL; written only with a path) receives 24 numbers:
 *   [0] identity (order_out gets the identity)  [1] pin (clouds pinned to XCDs)  [2] tiles  [3] nsplit (candidate pieces)
 *   [4] vec (staging vector floats: all-pairs, fp32 filter)  [5] nblocks (workgroups of the main kernel)  [6] probe
 *   [7] smallc (all-pairs C <= 4 instance)  [8] K2  [9] CP  [10] NB  [11] the bit pattern of ce (filters' error-bound factor)
 *   [12] wide (scan: 128-query workgroups)  [13] qtiles  [14] rerank2  [15] unsorted  [16] an order hint is in use
 *   [17 - 23] byte offsets from ws of part, norms, cmax, planes, iscale, xs, tb; -1 = region unused
 * A field a path does not use is 0.  The thresholds are the library's to change; the codes and the positions in plan_out are not. */
int gpe_knn_path(const float* x, int B, int N, int C, int ldx, int k, int has_idx_glob, int has_order_in, int has_order_out,
                 const void* ws, long ws_bytes, const int* switches, long* plan_out);

/* reverse adjacency of the kNN graph (needed by the gather's backward = scatter-add into x_j rows):
 * rev_off [B][N+1] int32 (local offsets: the exclusive scan of the in-degrees, rev_off[N] = N*k), rev_edge [B][N*k] int32 =
 * local edge ids (i*k+s) sorted ascending inside each bucket, so the pull-style accumulation order is deterministic.
 * idx holds cloud-local neighbours; 2N + 1 ints must fit 150 KB of LDS, else -22. */
int gpe_knn_reverse(const int32_t* idx, int B, int N, int k, int32_t* rev_off, int32_t* rev_edge, void* stream);

/* ---- weight packing (+ BatchNorm folding) ------------------------------------------------------------------
 * w [N][ldw] row-major (nn.Linear layout, nn/net_blocks.py:45) or, if transpose != 0, w is [K][ldw] and the packed
 * operand is its transpose.  Optional col_scale[K]: packed(n,k) = w(n,k)*col_scale[k]  (folds the previous
 * BatchNorm's scale s=gamma*rstd into this Linear).  wp holds gpe_packed_size(N,K) floats: K in whole 16-k chunks, and a K in
 * (96, 208] filled up with zeros to the 10 or 13 chunks the register-stationary edge kernels keep resident. */
long gpe_packed_size(int N, int K);
int gpe_pack_weight(const float* w, int ldw, int N, int K, int transpose, const float* col_scale,
                    float* wp, void* stream);
/* every weight-derived operand of a model refreshed by ONE launch (after an optimizer step): `jobs_dev` is a device array
 * of njobs 64-byte records {const float* w, w2; float* out; long total, first_block; int ldw, N, K, kind, Npad, aux}
 * sorted by first_block; a job occupies gpe_pack_job_blocks(kind, total, Npad, K) 256-thread blocks (ABI version 6: row-major sources —
 * kinds 0, 2, 8 — are packed in 64 x 64 tiles, kind 9 reads 4096 elements per block, everything else writes 1024 outputs per block;
 * versions 3 - 5: 1024 outputs per block throughout).  kind 0 plain pack, 1 transposed pack, 2 gate-interleaved pack (aux = H),
 * 3 pack of [W1a-W1b ; W1b] from W1 [H][2C] (gpe_w1_split + pack; aux = H), 4 its transpose, 5 out = w + w2 (N floats),
 * 6 out = [w[0:aux] | 0] (N floats), 7 out = w + [w2[0:aux] | 0] (N floats; GRU input-side bias b_ih + [b_hr | b_hz | 0]).
 * f16x3 operands of the recurrences (ABI version 4): kind 9 = largest |w| of the [N][K] matrix, atomicMax into the uint32 word at
 * `out` (zeroed by the caller; total = N*K); kind 8 / 10 = two-term fp16 PLANES of the gate-interleaved pack (element map of
 * kind 2) / of the plain transpose (kind 1) in the B-fragment order of v_mfma_f32_16x16x32_f16 — out = [plane h | plane l], a
 * plane = [KP/8][Npad][8 halves], KP = K rounded up to 32; w * 2^sh = h + l with 2^sh from the amax word at `w2`
 * (total = 2 * (KP/8) * Npad * 4; gpe_packed_planes_size).  A kind-9 job must run in an EARLIER launch than the planes that
 * read its word. */
long gpe_packed_planes_size(int Npad, int K);        /* floats (4-byte units) of a kind-8 / kind-10 output */
long gpe_pack_job_blocks(int kind, long total, int Npad, int K);
int gpe_pack_multi(const void* jobs_dev, int njobs, long total_blocks, void* stream);
/* (ABI version 7) what a forward block of the edge MLP needs from the BatchNorm in front of it, in one launch instead of three:
 * wp = pack of w [N][K] with col_scale (gpe_pack_weight), bias_out[n] = bias[n] + sum_k w[n][k] t[k] (gpe_fold_bias) and, with the
 * caller's edge workspace `ws` (gpe_edge_ws_bytes; NULL = skip), the packed weight's largest magnitude in its f16x3 slot + the clears
 * the edge launch's own pass performs (`clear_word`: the amax_out word of the coming gpe_edge_mlp_fwd, or NULL) — that launch is then
 * told so through bit 1 of its `out_half` argument.  `ticket`: one uint32 the caller zeroes ONCE and reuses (left zero; not shared
 * by concurrent calls; only needed with `ws`).  Results bit-identical to the separate entry points.
 * Replaces nothing of the reference by itself: it is the BatchNorm fold of DESIGN.md 4 (nn/net_blocks.py:43-47). */
int gpe_pack_fold(const float* w, int ldw, int N, int K, const float* col_scale, const float* t, const float* bias, float* wp,
                  float* bias_out, void* ws, long ws_bytes, uint32_t* clear_word, uint32_t* ticket, void* stream);
/* folded bias: out[n] = bias[n] + sum_k w[n][k]*t[k]   (t = beta - mean*s of the previous BatchNorm) */
int gpe_fold_bias(const float* w, int ldw, int N, int K, const float* bias, const float* t, float* out,
                  void* stream);

/* ---- dense Linear: nn.Linear / LSTM gate projections (nn/net_blocks.py:45,158,373-376,397) -----------------
 * Y[r][n] = act( sum_k A[r][k]*W[n][k] + bias[n] + addend[r][n] ),  r<M, n<N.   A rows use 2-level addressing
 * (a_inner<=0: row r at a + r*a_so; else row r at a + (r/a_inner)*a_so + (r%a_inner)*a_si); same for Y and addend.
 * act: 0 none, 1 relu.  bias/addend may be NULL. */
int gpe_linear(const float* a, long a_so, long a_si, int a_inner,
               const float* wp, const float* bias,
               const float* addend, long ad_so, long ad_si, int ad_inner,
               float* y, long y_so, long y_si, int y_inner,
               int M, int N, int K, int act, void* stream);
/* Which kernel a gpe_linear call with these arguments runs (nn/net_blocks.py:45,158,373-376,397: the same nn.Linear).  Added without
 * a version bump (gpe_abi_version() stays 7): one host-only query, nothing else changes.  HOST ONLY: gpe_linear's arguments without the
 * stream; the pointers are looked at for NULL and for their 16-byte alignment and never followed (bias not at all), no HIP call is
 * made and nothing is allocated; the arithmetic mode (gpe_math_get) and the debug word (gpe_debug_get) are read as gpe_linear reads
 * them, and gpe_linear dispatches through the same function.  Returns -22 where gpe_linear refuses the arguments, 0 for M == 0
 * (nothing is launched), else rung * 100 + NT:
 *   100       bf16-pipe kernel, three-term splits, 128 x 128 blocks (f16x3 mode with debug bit 16384 clear, M >= 2048, N >= 48,
 *             K >= 32, 2 M N K >= 2.5e8, A rows and wp 16-byte loadable up to round4(K))
 *   200       K <= 8 streaming-store kernel (N % 4 == 0, M >= 4096, y and addend rows 16-byte aligned)
 *   301, 304  single-stage kernel with 16- / 64-column blocks (ceil(M / 64) * ceil(N / 208) < 128; 64-column blocks when
 *             ceil(M / 64) * ceil(N / 64) >= 128 and N > 16)
 *   404, 407, 410, 413, 416   streaming kernel with 16 NT-column blocks (everything else)
 * The thresholds are the library's to change; the codes are not. */
int gpe_linear_path(const float* a, long a_so, long a_si, int a_inner,
                    const float* wp, const float* bias,
                    const float* addend, long ad_so, long ad_si, int ad_inner,
                    const float* y, long y_so, long y_si, int y_inner,
                    int M, int N, int K, int act);

/* reduce-GEMM: G[m][n] (+)= sum_r U[r][m]*V[r][n]  (weight gradients, nn.Linear backward), colsum[m] = sum_r U[r][m].
 * part: workspace of gpe_redgemm_ws(Mg,Ng) floats.  accumulate != 0 adds into G / colsum. */
long gpe_redgemm_ws(int Mg, int Ng);
int gpe_redgemm(const float* u, long u_so, long u_si, int u_inner,
                const float* v, long v_so, long v_si, int v_inner, const float* v_shift,
                long rows, int Mg, int Ng, float* G, int ldg, float* colsum, float* part, int accumulate,
                void* stream);
/* v_shift (may be NULL) [Ng]: V rows are centred on the fly, G = sum_r U^T (V - shift) — used with shift = BatchNorm
 * batch mean so the BN-backward covariance term is accumulated without cancellation. */

/* ---- EdgeConv block (PyG DynamicEdgeConv.message + MLP + max aggregation; nn/net_blocks.py:43-47,124-135) ---
 * Algebra used: W1.[x_i, x_j-x_i] = (W1a-W1b).x_i + W1b.x_j = P_i + Q_j, with PQ = [P|Q] [B*N][2H] produced by
 * gpe_linear on the per-point features; every BatchNorm is folded into the next Linear once its batch statistics
 * are known (training mode needs the global reduction between layers; eval mode uses running stats).           */

/* stats of a1 = relu(P_i + Q_j) over all E=B*N*k edges: part [nblk][2][H] fp64 partial (sum, sumsq); nblk returned
 * by gpe_stats_blocks().  This is the EdgeConv neighbourhood gather. */
int gpe_stats_blocks(void);
int gpe_edge_gather_stats(const float* pq, int ldpq, int H, const int32_t* jg, int B, int N, int k,
                          double* part, void* stream);

/* BatchNorm finalisation (nn.BatchNorm1d in training mode, nn/net_blocks.py:45): from fp64 partials over `count`
 * rows -> mean, biased var; scale s = gamma/sqrt(var+eps), shift t = beta - mean*s; running stats updated with
 * `momentum` (unbiased var) and num_batches_tracked += 1 when running_mean != NULL.
 * stats_out [4][C] fp32 = {mean, rstd, s, t}. */
int gpe_bn_finalize(const double* part, int nblk, int C, double count, const float* gamma, const float* beta,
                    float eps, float momentum, float* running_mean, float* running_var, int64_t* num_batches,
                    float* stats_out, void* stream);
/* eval mode: stats_out from running stats */
int gpe_bn_from_running(const float* running_mean, const float* running_var, int C, const float* gamma,
                        const float* beta, float eps, float* stats_out, void* stream);

/* fused per-edge Linear+ReLU (+BN statistics, + max/min aggregation over the k messages of each point).
 * a_mode 0: A rows = relu(P_i+Q_j) gathered through the global neighbour rows jg (layer 2 of the edge MLP);
 * a_mode 1: A rows = a_in[e][*] dense (layer 3).
 * out [E][ldo] = relu(A.Wp^T + bias');  stats_part [nblk][2][Cout] fp64 (NULL in eval mode);
 * if agg != 0: mx,mn [B*N][ldagg] = max/min over the k rows of each point, amx/amn uint8 argmax/argmin slot. */
int gpe_edge_mlp_fwd(int a_mode, const float* pq, int ldpq, const int32_t* jg, const float* a_in, int lda,
                     int B, int N, int k, int Cin, int Cout, const float* wp, const float* bias,
                     float* out, int ldo, double* stats_part,
                     int agg, float* mx, float* mn, uint8_t* amx, uint8_t* amn, int ldagg,
                     const uint32_t* amax_a, uint32_t* amax_out, void* ws, long ws_bytes, int out_half, void* stream);
/* out_half: bit 0 (below) and bit 1 = "the packed weight's f16x3 scale is already in `ws`" (written by gpe_pack_fold on the same stream,
 * same workspace, nothing of this library in between: the launch then skips its own pass over wp).
 * out_half & 1: `out` is a _Float16 [E][ldo] tensor (ldo in halves, % 4 == 0; values rounded to nearest even, clamped at 65504) — the storage of the
 * aggregated block's activation when its backward forms dz3 lazily (below): that backward only needs the ReLU side of a3 and
 * the term (a3 - mean) * k2 with a coefficient of order 1e-3, gradients move by 2e-6 / 5e-6 of their maximum
 * (profiles/r04_h_row_g_probe.txt), and the step loses 0.96 GB of traffic per layer.  Only where gpe_edge_lazy_dz3_ok(B, N, k, Cout,
 * Cin) == 1 with a_mode 1 and agg != 0; anything else returns -22.  mx / mn, the statistics and amax_out are taken from the fp32
 * values before rounding. */
/* amax_a: amax word of the A operand (a_mode 0: of relu(P_i+Q_j), e.g. from gpe_edge_pq_amax; a_mode 1: of a_in), amax_out: word
 * that receives the largest |out| — see Conventions.  ws: gpe_edge_ws_bytes(B, N, k, ldagg) bytes, 16-B aligned: the store image
 * of the straight-line kernels, the in-call f16x3 words, the per-pseudo-point rows of a k > 16 launch.  NULL / too small: the
 * variants that need none run (slower; f16x3 falls back to exact fp32). */
long gpe_edge_ws_bytes(int B, int N, int k, int ldmax);   /* ldmax: the largest ldagg / lddp the workspace will be used with */
/* amax[0] = bits of a bound of relu(P_i + Q_j) over the [rows][ldpq >= 2H] table (max P + max Q, rounded up); ws as above */
int gpe_edge_pq_amax(const float* pq, int ldpq, int H, long rows, uint32_t* amax, void* ws, long ws_bytes, void* stream);
/* amax[0] = bits of the largest |x| over [rows][cols] (row pitch ldx, 16-B aligned rows) */
int gpe_absmax(const float* x, int ldx, long rows, int cols, uint32_t* amax, void* stream);

/* layer output: y[i][c] = s[c]*(s[c]>=0 ? mx : mn)[i][c] + t[c]  (BN applied after the max, sign-aware).  A zero scale of either sign
 * (+0.0, -0.0) selects mx here, in gpe_edge_bwd_point_sums and in gpe_edge_dz3 alike.  rows = 0 is a no-op; columns from C to the
 * pitch of y are not written. */
int gpe_edge_finish(const float* mx, const float* mn, int ldagg, const float* stats, long rows, int C,
                    float* y, int ldy, void* stream);

/* ---- EdgeConv backward ------------------------------------------------------------------------------------ */
/* per-channel sums for the last BN's backward from per-point data, as fp64 partials
 * part [gpe_point_sums_blocks()][2][C]: sum_i g, sum_i g*xhat_sel */
int gpe_point_sums_blocks(void);
int gpe_edge_bwd_point_sums(const float* g, int ldg, const float* mx, const float* mn, int ldagg,
                            const float* stats, long rows, int C, double* part, uint32_t* amax_sg, void* stream);
/* amax_sg (may be NULL): receives the bits of max |s_c * g_ic| (s = the BatchNorm scale in `stats`), measured while g is read —
 * the data term of gpe_edge_dz3_bound.  The call resets the word itself; the value is never below the true maximum and at most
 * 8 * 2^-24 relative above it.  Every one of the gpe_point_sums_blocks() partial blocks is written (zeros where a block has no row). */
/* coefficient vectors for "dz = (a>0) ? s*dy - c1 - (a-mean)*k2 : 0":  coef [4][C] = {s, c1 = s*mean(dy),
 * k2 = s*rstd*mean(dy*xhat), mean} from partial sums part [nblk][2][C]; also the BatchNorm parameter gradients
 * dgamma = sum dy*xhat, dbeta = sum dy (may be NULL) */
int gpe_bn_bwd_coef(const double* part, int nblk, const float* stats, int C, double count, float* coef,
                    float* dgamma, float* dbeta, void* stream);
/* sums for an inner BN from the next layer's CENTRED weight-gradient product: G [Cn][ldG] = dz_next^T (a - mean)
 * (gpe_edge_redgemm with v_shift = mean), db [Cn] = colsum dz_next, w_next [Cn][ldw] the UNFOLDED next Linear:
 *   sums[0][c] = sum_f w[f][c]*db[f];   sums[1][c] = rstd_c * sum_f w[f][c]*G[f][c];
 * also emits the true weight gradient dW_next[f][c] = G[f][c]*s_c + db[f]*beta_c into dw (ld lddw). */
int gpe_bn_bwd_from_G(const float* G, int ldG, const float* db, const float* w_next, int ldw, int Cn, int C,
                      const float* stats, double* sums, float* dw, int lddw, void* stream);

/* dz3 = (a3>0) ? [slot==argsel]*s*g - c1 - (a3-mean)*k2 : 0 written IN PLACE over the stored activation a3 [E][lda3]
 * (BN-after-max backward + ReLU backward of the last edge-MLP block; g [B*N][ldg] is the layer-output gradient,
 * amx/amn the argmax/argmin slots saved by gpe_edge_mlp_fwd, coef [4][F] = {s, c1, k2, mean} from gpe_bn_bwd_coef).
 * Exactly +0 wherever a3 <= 0.  Rows are handled in quads of columns: columns F .. round_up(F, 4) - 1 of a3 are read (any value,
 * NaN included) and WRITTEN 0, columns from round_up(F, 4) to lda3 are left alone (lda3 and ldagg % 4 == 0, >= F; amx / amn are
 * read up to round_up(F, 4) as well).  amax_out (may be NULL) is reset by the call and receives the bits of the largest |value|
 * written. */
int gpe_edge_dz3(float* a3, int lda3, const float* g, int ldg, const uint8_t* amx, const uint8_t* amn, int ldagg,
                 const float* coef, int B, int N, int k, int F, uint32_t* amax_out, void* stream);

/* reduce-GEMM over the E edges: G[Mg][Ng] = sum_e U[e][:]^T (V[e][:] - v_shift), colsum[Mg] = sum_e U[e][:];
 * U dense [E][ldu]; v_mode 0: V rows = relu(P_i+Q_j) gathered through jg (Ng = H) ; v_mode 1: V rows dense [E][ldv];
 * v_shift [Ng] may be NULL */
int gpe_edge_redgemm(const float* u, int ldu, int v_mode, const float* v, int ldv, const float* pq, int ldpq,
                     const int32_t* jg, const float* v_shift, int B, int N, int k, int Mg, int Ng, float* G, int ldG,
                     float* colsum, float* part, const uint32_t* amax_u, const uint32_t* amax_v, void* ws, long ws_bytes,
                     const float* lz_g, int lz_ldg, const uint8_t* lz_amx, const uint8_t* lz_amn, int lz_ldagg,
                     const float* lz_coef, void* stream);
/* amax_u / amax_v: amax words of U and of V (v_mode 0: of relu(P_i+Q_j); NULL there = the bound passes run in `ws`).  f16x3 mode
 * runs the fp16-pipe kernel only when both are known, else the exact fp32 kernel. */
/* Which kernel a reduce-GEMM call runs, and the numbers of its launch.  Added without a version bump (gpe_abi_version() stays 7): one
 * host-only query, nothing else changes.  HOST ONLY: the pointers are looked at for NULL and for their 16-byte alignment and never
 * followed, no HIP call is made beyond the CU count (256 without a GPU, less gpe_reserve_cus_set) and nothing is allocated; the
 * arithmetic mode, the debug word, the f16x3 size gate and the CU reservation are read as the entry points read them, and both
 * entry points take their plan from the same function.
 *   k == 0   a gpe_redgemm call: (u, u_so, u_si, u_inner), (v, v_so, v_si, v_inner), rows, Mg, Ng as there; v_mode must be 1,
 *            pin_clouds, the has_* flags and lazy are not looked at (lazy must be 0)
 *   k > 0    a gpe_edge_redgemm call with B = pin_clouds clouds of N = rows / (B k) points (rows must divide): single-level rows
 *            (u, ldu = u_so); v_mode 1: (v, ldv = v_so); v_mode 0: v stands for the [P|Q] table and v_so for ldpq.  has_amax_u /
 *            has_amax_v: the caller passes that word; has_ws: a workspace of gpe_edge_ws_bytes(...) bytes; lazy: the lz_* fields
 * want_colsum: colsum != NULL.  Returns -22 where the entry point refuses the call (its checks of G, ldG, part and of the lz_*
 * pitches aside), else the rung, in the order of DESIGN.md 5.33:
 *   1 thin   2 bf16-pipe TN   3 deep   4 b3 f16x3 lazy dz3   5 b3 f16x3   6 b3 bf16x3   7 producer/consumer   8 big-block
 * plan_out (may be NULL; written only with a rung) receives 17 numbers:
 *   [0] gx [1] gy [2] gz [3] nblk (partials)  [4] MgPad [5] NgPad  [6] MH [7] NH (big-block instance)  [8] MT (rungs 4 - 8)
 *   [9] vec [10] vvec (deep) [11] ql (thin)  [12] num_tiles [13] rows_per_split (TN)  [14] pin_tpc
 *   [15] floats the launch writes from `part` on (never more than gpe_redgemm_ws(Mg, Ng))  [16] partial column sums are written
 * The thresholds are the library's to change; the codes and the positions in plan_out are not. */
int gpe_redgemm_path(const float* u, long u_so, long u_si, int u_inner, const float* v, long v_so, long v_si, int v_inner,
                     long rows, int Mg, int Ng, int v_mode, int k, int pin_clouds, int has_amax_u, int has_amax_v, int has_ws,
                     int lazy, int want_colsum, long* plan_out);

/* propagate + BN/ReLU backward:  u = A.Wp^T ; dz = (act>0) ? s*u - c1 - (act-mean)*k2 : 0 ; written to dz_out
 * (A dense [E][lda]; coef_out [4][Cout] = {s,c1,k2,mean} of the BatchNorm being crossed; Wp = packed TRANSPOSE of the
 * unfolded Linear).
 * act_mode 0: act = dz_out's previous contents (in place over the stored activation);
 * act_mode 1: act = relu(P_i+Q_j) gathered, and dP[i] = sum_s dz[(i,s)] is also written (ld lddp).
 * Aliasing: act_mode 1 may run IN PLACE (dz_out == a, ldo == lda); any other overlap of dz_out with a, pq or dP — and, in
 * gpe_edge_mlp_fwd, of out with a_in, pq, mx or mn — is refused with -22 (several kernels store rows through a buffer descriptor
 * and load through plain pointers: aliased, the stores would lose their order against the loads). */
int gpe_edge_mlp_bwd(const float* a, int lda, int act_mode, const float* pq, int ldpq, const int32_t* jg,
                     int B, int N, int k, int Cin, int Cout, const float* wp, const float* coef_out,
                     float* dz_out, int ldo, float* dP, int lddp, const uint32_t* amax_a, uint32_t* amax_out, void* ws,
                     long ws_bytes, const float* lz_g, int lz_ldg, const uint8_t* lz_amx, const uint8_t* lz_amn, int lz_ldagg,
                     const float* lz_coef, void* stream);
/* ---- lazy dz3 (ABI version 4): gpe_edge_dz3's in-place pass folded into its two consumers ---------------------------------
 * With lz_g != NULL, gpe_edge_mlp_bwd (act_mode 0: `a`) and gpe_edge_redgemm (v_mode 1: `u`) take the STORED ACTIVATION a3 of the
 * block under the max aggregation — as the _Float16 [E][lda / ldu] tensor gpe_edge_mlp_fwd stored with out_half = 1 (pitch in
 * halves, % 4 == 0, rows 8-B aligned) — instead of dz3 and form dz3 = (a3>0) ? [slot==argsel]*s*g - c1 - (a3-mean)*k2 : 0 while staging
 * it: lz_g [B*N][lz_ldg] the layer-output gradient as it arrives (any pitch >= F, no alignment requirement), lz_amx / lz_amn
 * [B*N][lz_ldagg] the slots saved by gpe_edge_mlp_fwd, lz_coef [4][F] from gpe_bn_bwd_coef.  a3 is not modified.  Only where
 * gpe_edge_lazy_dz3_ok(...) == 1 (f16x3 arithmetic, k = 16, widths on the two-plane kernels' menu, above the size gate); amax_a /
 * amax_u must then be a bound of |dz3| (gpe_edge_dz3_bound) and amax_v the word of V.  Anything else returns -22. */
int gpe_edge_lazy_dz3_ok(int B, int N, int k, int F, int Cprev);
/* amax_out = bits of a bound of |dz3| = max |s*g| (amax_sg, from gpe_edge_bwd_point_sums) + max_c (|c1| + (amax(a3) + |mean|) |k2|)
 * with coef [4][F] from gpe_bn_bwd_coef and amax_a3 the word of the stored activation (gpe_edge_mlp_fwd's amax_out) */
int gpe_edge_dz3_bound(const uint32_t* amax_sg, const float* coef, int F, const uint32_t* amax_a3, uint32_t* amax_out, void* stream);

/* dQ[j] = sum over incoming edges e of dz1[e]  (deterministic pull through the reverse adjacency: fp32, from +0, in ascending
 * edge id; a point without incoming edges receives +0).  H % 4 == 0, H <= 256, lddz and lddq % 4 == 0; only columns 0 .. H - 1
 * of dQ are written, so dQ may be the right half of a [B*N][2H] buffer. */
int gpe_edge_pull_dq(const float* dz, int lddz, const int32_t* rev_off, const int32_t* rev_edge,
                     int B, int N, int k, int H, float* dQ, int lddq, void* stream);

/* ---- pooling (torch_geometric global_mean_pool, nn/net_blocks.py:148,184) --------------------------------- */
int gpe_segment_mean_fwd(const float* x, int ldx, int B, int N, int C, float* y, int ldy, void* stream);
int gpe_segment_mean_bwd(const float* gy, int ldgy, int B, int N, int C, float* gx, int ldgx, int accumulate,
                         void* stream);

/* ---- LSTM cell pointwise (nn.LSTM, gate order i,f,g,o; nn/net_blocks.py:373,393) --------------------------- */
/* gates_pre [Bn][4H] (pre-activation, overwritten with activated gates), c_prev [Bn][H] (row stride ldc_prev),
 * writes c [Bn][H] and h rows (2-level addressing via h + b*h_stride). */
int gpe_lstm_cell_fwd(float* gates, const float* c_prev, long ldc_prev, float* c, float* h, long h_stride,
                      int Bn, int H, void* stream);
/* dh_total = dh_out + sum of the n_rec partials dh_rec[z][Bn][H] (gpe_linear_splitk); computes dgates (pre-activation grads) [Bn][4H] rows at dgates + b*dg_stride,
 * dc_prev; inputs: activated gates, c (this step), c_prev. */
int gpe_lstm_cell_bwd(const float* dh_out, long dho_stride, const float* dh_rec, int n_rec, const float* dc_next,
                      const float* gates, const float* c, const float* c_prev, long ldc_prev,
                      float* dgates, long dg_stride, float* dc_prev, int Bn, int H, void* stream);

/* fused LSTM step (nn.LSTM recurrence, gate order i,f,g,o): gates = h_prev . W_hh^T + xproj (xproj = x_t . W_ih^T + b_ih
 * + b_hh, rows at xproj + b*xp_stride), then the cell update, in ONE launch.  W_hh must be packed gate-interleaved by
 * gpe_pack_weight_gates (gpe_packed_gates_size(H, K) floats).  Writes the ACTIVATED gates [Bn][4H] (for backward),
 * c_out [Bn][H] and h rows at h_out + b*h_stride. */
long gpe_packed_gates_size(int H, int K);
int gpe_pack_weight_gates(const float* w, int ldw, int H, int K, float* wp, void* stream);
int gpe_lstm_step_fwd(const float* h_prev, long hp_stride, const float* whh_gates_packed, const float* xproj,
                      long xp_stride, const float* c_prev, long ldc_prev, float* gates, float* c_out, float* h_out,
                      long h_stride, int Bn, int H, void* stream);

/* ---- GRU decoder (nn.GRU, gate order r,z,n; GRUDecoderModule, nn/net_blocks.py:457-497) ------------------------------
 * gate-interleaved packing for G gates (G = 3 here; gpe_pack_weight_gates is the G = 4 case) */
long gpe_packed_ngates_size(int H, int G, int K);
int gpe_pack_weight_ngates(const float* w, int ldw, int H, int G, int K, float* wp, void* stream);
/* fused step: r = s(xr + W_hr.h), z = s(xz + W_hz.h), n = tanh(xn + r*(W_hn.h + b_hn)), h' = (1-z)*n + z*h in ONE launch.
 * xproj rows [Bn][3H] = x.W_ih^T + b_ih (+ b_hr, b_hz); saved [Bn][4H] = {r, z, n, W_hn.h + b_hn} (for backward). */
int gpe_gru_step_fwd(const float* h_prev, long hp_stride, const float* whh_gates_packed, const float* xproj,
                     long xp_stride, const float* bhn, float* saved, float* h_out, long h_stride, int Bn, int H,
                     void* stream);
/* pointwise backward of one step: dh = dh_out + dh_dir_next + sum of the n_rec partials dh_rec[z][Bn][H];
 * dgx [..][3H] = input-side pre-activation gradients {dr, dz, dn}, dgh = recurrent-side {dr, dz, dn*r}; dh_dir_prev = dh*z */
int gpe_gru_cell_bwd(const float* dh_out, long dho_stride, const float* dh_rec, int n_rec, const float* dh_dir_next,
                     const float* saved, const float* h_prev, long hp_stride, float* dgx, float* dgh, long dg_stride,
                     float* dh_dir_prev, int Bn, int H, void* stream);

/* ---- whole recurrences, wavefront order (gpe_rnn_wave.hip) ---------------------------------------------------------------
 * A stack of L layers over T steps (nn.LSTM gates = 4 / nn.GRU gates = 3, batch_first, no dropout) executed diagonal by
 * diagonal: all cells (l, t) with l + t = d run in one launch.  Buffers (device, fp32):
 *   hs    h history, element (l, b, slot) at hs + l*hs_sl + b*hs_sb + slot*hs_st, slot 0 = h0, slot t+1 = h_t (pitches % 4 == 0)
 *   cs    LSTM c history, (l, slot) at cs + l*cs_sl + slot*cs_st, each [Bn][H]
 *   saved activated gates per cell, (l, t) at saved + l*sv_sl + t*sv_st, each [Bn][4H] (GRU: {r, z, n, W_hn.h + b_hn})
 *   xproj0  layer-0 input projection x.W_ih^T + bias, row (b, t) at xproj0 + b*xp0_sb + t*xp0_st (xp0_st = 0: same input at
 *           every step, the decoders' case)
 * whh / wih / bias / bhn are HOST arrays of L device pointers: gate-interleaved packed W_hh_l; gate-interleaved packed W_ih_l
 * (entry 0 unused); the addend row [gates*H] of layers > 0 (LSTM b_ih + b_hh; GRU b_ih + [b_hr | b_hz | 0]; entry 0 unused);
 * GRU b_hn [H] per layer (NULL for LSTM).
 * Alignment: hs (and dgx / dgh of gpe_rnn_seq_bwd) must be 16-byte aligned and hs_sl (dg_sl) a multiple of 4 floats like the
 * other pitches: every family fetches rows in 16-byte pieces.  The persistent families check both and decline; the entry points do
 * NOT (they check hs_sb, hs_st / dg_sb, dg_st only) and the diagonal launches then fetch misaligned pieces: the caller's error.
 * What is read and written of a state row (hs_st may exceed H; a row's pad columns are H .. hs_st - 1).  No element outside columns
 * 0 .. H - 1 of slots 0 .. T ever enters the arithmetic: whatever else a fetch brings in is replaced by zero (a select, not a
 * product) before any use, so pad columns, gaps and slots not yet produced need not be zero and may hold any bit pattern, NaN
 * included.  What the fetches LOAD beyond that, family by family:
 *   diagonal launches        16-byte pieces that start below column H: columns H .. round_up(H, 4) - 1 of the row
 *   persistent, K split      whole k-steps of a row: columns H .. round_up(H, 16) - 1 (fp16 pipe: round_up(H, 32) - 1) counted on from
 *                            the row's slot — past hs_st these are the row's NEXT slots, which another workgroup may be writing, the
 *                            gap behind the row or the next row — as far as they lie inside the buffer descriptor of the slot (from
 *                            the slot of row 0 to column round_up(H, 4) of the slot of row Bn - 1; beyond it the load returns zero).
 *                            Loaded and discarded, never values
 *   persistent, multi-tile   columns 0 .. H - 1 of slot 0 only (later states travel through the workspace)
 * NOTHING outside columns 0 .. H - 1 of slots 1 .. T is written: slot 0, every pad column and every gap come back as they were.
 * The same holds for cs (slot 0 read, slots 1 .. T written, [Bn][H] dense inside a slot) and saved (each [Bn][4H] dense), and in
 * gpe_rnn_seq_bwd for the dgx / dgh rows: only columns 0 .. gates*H - 1 are values or written; the diagonal launches load up to
 * round_up(gates*H, 4), the K-split kernel whole k-steps up to KP (plan_out[6]) inside its descriptor, both discarded.  The
 * backward reads of hs only columns 0 .. H - 1 of slots 0 .. T - 1 (GRU only). */
int gpe_rnn_seq_fwd(int gates, int L, int T, int Bn, int H, const float* xproj0, long xp0_sb, long xp0_st,
                    const void* const* whh, const void* const* wih, const void* const* bias, const void* const* bhn,
                    float* hs, long hs_sl, long hs_sb, long hs_st, float* cs, long cs_sl, long cs_st, float* saved,
                    long sv_sl, long sv_st, const void* const* whh_pl, const void* const* wih_pl,
                    const void* const* whh_amax, const void* const* wih_amax, void* ws, long ws_bytes, void* stream);
/* ws: gpe_rnn_seq_fwd_ws bytes of scratch (may be NULL when the query answers 0; the K-split persistent kernels take it 8-byte
 * aligned, the multi-tile one 16-byte aligned — a workspace that is missing, shorter or less aligned is no error: the next family
 * of DESIGN.md 5.28 runs, which gpe_rnn_seq_fwd_path shows).  An LSTM stack of <= 256
 * units whose 16-row tiles fit the chip (layers x ceil(H/16) x row tiles <= compute units: the pattern decoder, 32 rows x 2
 * layers) then runs as ONE persistent launch (gpe_rnn_persist.hip): every workgroup keeps its weight slices in LDS for all T
 * steps and cells hand their state rows on through arrival counters in `ws` (zeroed in-call) instead of kernel boundaries.
 * Same arithmetic per product as the diagonal launches (K is split over four waves instead of two: results agree to fp32
 * rounding, not bit for bit). */
long gpe_rnn_seq_fwd_ws(int gates, int L, int T, int Bn, int H);
/* whh_pl / wih_pl / whh_amax / wih_amax (host arrays of L device pointers, or NULL; entry 0 of the wih arrays unused): the fp16
 * plane packs (gpe_pack_multi kind 8) of W_hh_l / W_ih_l and their amax words (kind 9).  With all of them present and the f16x3
 * arithmetic selected (gpe_math_set(4)) the gate products run on the fp16 pipe: the state rows enter scaled by 2^12 and split in
 * two fp16 terms (|h| < 1 for every state a cell produces; start states must satisfy |h0| < 16), three MFMAs per product, fp32
 * accumulate — same bars as the exact kernel in every test.  Otherwise: exact fp32. */
/* backward through the same recurrence.  dtop: gradient of the top layer's outputs, row (b, t) at dtop + b*dt_sb + t*dt_st
 * (may be NULL); d_hN / d_cN [L][Bn][H]: gradients of the final states (may be NULL).  whh_t / wih_t: host arrays of the
 * plain TRANSPOSED packs (gpe_pack_weight(.., transpose = 1)).  Outputs: dgx / dgh [L][Bn][T][ld], element (l, b, t) at
 * + l*dg_sl + b*dg_sb + t*dg_st (pitches % 4 == 0): pre-activation gradients on the input side / recurrent side (LSTM: pass
 * the same buffer twice).  part: workspace of gpe_rnn_seq_bwd_ws floats; carry: [2][L][Bn][H] scratch — on return
 * carry[0][l] holds dc_0 (LSTM) / the z-gated part of dh_0 (GRU) of layer l. */
long gpe_rnn_seq_bwd_ws(int gates, int L, int T, int Bn, int H);
int gpe_rnn_seq_bwd(int gates, int L, int T, int Bn, int H, const float* dtop, long dt_sb, long dt_st, const float* d_hN,
                    const float* d_cN, const void* const* whh_t, const void* const* wih_t, const float* hs, long hs_sl,
                    long hs_sb, long hs_st, const float* cs, long cs_sl, long cs_st, const float* saved, long sv_sl,
                    long sv_st, float* dgx, float* dgh, long dg_sl, long dg_sb, long dg_st, float* part, float* carry,
                    const void* const* whh_tpl, const void* const* wih_tpl, const void* const* whh_amax,
                    const void* const* wih_amax, void* stream);
/* whh_tpl / wih_tpl / whh_amax / wih_amax (host arrays of L device pointers, or NULL; entry 0 of the wih arrays unused): the
 * TRANSPOSED fp16 plane packs (gpe_pack_multi kind 10) of W_hh_l / W_ih_l and their amax words — used by the persistent
 * backward launch (same eligibility as the forward's) in f16x3 mode: the dG rows are normalised per wave by the largest
 * magnitude the wave loaded, three fp16 MFMAs per product, fp32 accumulate.  Absent: exact fp32. */
/* Which kernel family a recurrence call runs, and the numbers of its launch.  Added without a version bump (gpe_abi_version() stays
 * 7): two host-only queries, nothing else changes.  HOST ONLY: hs / ws / dgx / part are looked at for NULL and for their alignment
 * and never followed, no HIP call is made beyond the CU count (256 without a GPU, less gpe_reserve_cus_set) and nothing is launched;
 * the arithmetic mode, the debug word and the CU reservation are read as the entry points read them, and the entry points decide by
 * the same plan steps.  The operand tables are described by what the families look at:
 *   packs      the alignment in bytes the worst fp32 pack in use has (forward: the gate packs; backward: the transposed packs):
 *              16 = every pack there and aligned, 8 = one is misaligned, 0 = one is missing
 *   planes     the same for the fp16 plane packs (forward kind 8, backward kind 10) with their amax words; 0 = the tables are
 *              incomplete, so that the exact kernels run in every arithmetic mode
 *   bias_rows  forward: 1 = the bias row of every layer > 0 is there
 * Every other pointer of the entry point counts as present.  Returns -22 where the entry point refuses the call, else the family:
 *   1 persistent, K split over the waves   2 persistent, waves own row tiles (forward)   3 diagonal launches
 * plan_out (may be NULL; written only with a family) receives 17 numbers; one a family does not have is 0:
 *   [0] fp16 pipe  [1] NB  [2] NRT  [3] per (workgroups of a row group)  [4] rgmax  [5] RG  [6] KP (diagonals forward: the padded
 *   slab extent)  [7] grid (diagonals: workgroups of the largest launch)  [8] LDS bytes  [9] what the launch touches of the
 *   workspace: bytes behind ws (forward), floats behind part (backward) — never more than gpe_rnn_seq_fwd_ws / _bwd_ws
 *   diagonals: [10] K slab width (128 / 256)  [11] the last 64-row tile holds <= 32 rows (wave-pair K split)  [12] jslabs  [13] nz
 *   [14] fuse  [15] Hp (pitch of the partial images)  [16] the most launches (groups of <= 4 cells) a diagonal takes
 * The policies are the library's to change; the codes and the positions in plan_out are not. */
int gpe_rnn_seq_fwd_path(int gates, int L, int T, int Bn, int H, const float* hs, long hs_sl, long hs_sb, long hs_st, int packs,
                         int planes, int bias_rows, const void* ws, long ws_bytes, long* plan_out);
int gpe_rnn_seq_bwd_path(int gates, int L, int T, int Bn, int H, const float* dgx, long dg_sl, long dg_sb, long dg_st,
                         const float* part, int packs, int planes, long* plan_out);

/* ---- attention variant (GarmentSegmentPattern3D, nn/nets.py:187-299) ------------------------------------------ */
/* sparsemax.Sparsemax(dim=1) over rows of width W <= 32 (nn/nets.py:225): forward and backward */
int gpe_sparsemax_fwd(const float* z, int ldz, long rows, int W, float* out, int ldo, void* stream);
int gpe_sparsemax_bwd(const float* out, int ldo, const float* g, int ldg, long rows, int W, float* gz, int ldgz,
                      void* stream);
/* entmax.SparsemaxLoss() on the attention weights (nn/metrics/composed_loss.py:196,323-332; third-party, un-vendored: the
 * published sparsemax Fenchel-Young loss restated): loss[0] = mean_r (1 - |p|^2)/2 + <p - e_t, x>, p = sparsemax(x_r), W <= 32;
 * gx [rows][ldg] = (p - e_t)/rows (the gradient of loss[0]); part: ceil(rows/256) doubles of scratch; bad[0] |= 1 when a
 * target lies outside [0, W) (the caller zeroes it before the call and raises after). */
int gpe_sparsemax_loss(const float* x, int ldx, const int32_t* target, long rows, int W, float* gx, int ldg, double* part,
                       float* loss, int* bad, void* stream);
/* y = s*a + t with {s,t} = stats rows 2,3: BatchNorm of a stored post-ReLU activation (last block of a dense MLP) */
int gpe_bn_apply(const float* a, int lda, const float* stats, long rows, int C, float* y, int ldy, void* stream);

/* y = s*(a*a_scale) + t*t_scale: BatchNorm of a SUM (t_scale = k, EdgeConv aggr 'add') or MEAN (a_scale = 1/k) over the k
 * messages of a point, applied after the aggregation (nn/net_blocks.py:129 with EConv_aggr != 'max') */
int gpe_bn_apply_scaled(const float* a, int lda, const float* stats, long rows, int C, float a_scale, float t_scale,
                        float* y, int ldy, void* stream);
/* out[i][c] = sum over the k messages of point i of a[i*k+s][c], in fp32, slots ascending from +0 */
int gpe_edge_sum_k(const float* a, int lda, long npts, int k, int F, float* out, int ldo, void* stream);
/* explicit message inputs of DynamicEdgeConv (nn/net_blocks.py:124-135: cat[x_i, x_j - x_i]) for first-block widths the fused
 * P|Q path does not take (EConv_hidden not a multiple of 4, or > 256): out [npts*k][ldo >= 2C], row e = i*k + s holds
 * [x_i | x_{jg[e]} - x_i], and EVERY column from 2C to ldo is written 0 (the dense MLP that follows reads whole rows).
 * bwd: gx [B*N][ldgx >= C] from g [B*N*k][ldg >= 2C] through the transposed graph of gpe_knn_reverse (rev_off [B][N+1], rev_edge
 * [B][N*k], edge ids local to the cloud) — a deterministic pull, no atomics, in fp32 in this order: sum over the point's slots of
 * (g1 - g2), ascending, then the g2 of the incoming edges in ascending edge id.  Columns of g past 2C are not read, columns of gx
 * past C not written. */
int gpe_edge_inputs_fwd(const float* x, int ldx, int C, const int32_t* jg, long npts, int k, float* out, int ldo,
                        void* stream);
int gpe_edge_inputs_bwd(const float* g, int ldg, int C, const int32_t* rev_off, const int32_t* rev_edge, int B, int N, int k,
                        float* gx, int ldgx, void* stream);
/* gpe_edge_dz3 for aggr 'add' / 'mean': every message of a point receives gscale * g[i] (no arg-slot selection) */
int gpe_edge_dz3_all(float* a3, int lda3, const float* g, int ldg, float gscale, const float* coef, int B, int N, int k,
                     int F, uint32_t* amax_out, void* stream);

/* ---- pooling variants (torch_geometric global_max_pool / global_add_pool, nn/net_blocks.py:145-150) -----------------
 * mode 1 = max (arg [B][C] int32 = the winning point, first maximum), 2 = add. */
int gpe_segment_pool_fwd(const float* x, int ldx, int B, int N, int C, int mode, float* y, int ldy, int32_t* arg,
                         void* stream);
int gpe_segment_pool_bwd(const float* gy, int ldgy, const int32_t* arg, int B, int N, int C, int mode, float* gx,
                         int ldgx, void* stream);

/* attention pooling (nn/nets.py:263-276: `w[:, p] * features -> global_pool`, for all P panels at once):
 * out[b][p][c] = pool_n w[b*N+n][p] * feat[b*N+n][c];  mode 0 mean, 1 max, 2 add (the encoder's global_pool).
 * part / part_arg: workspaces of gpe_attn_pool_ws(B,N,P,C) floats / int32 (part_arg and arg only for max). */
long gpe_attn_pool_ws(int B, int N, int P, int C);
int gpe_attn_pool_fwd(const float* w, int ldw, const float* feat, int ldf, int B, int N, int P, int C, int mode,
                      float* out, int32_t* arg, float* part, int32_t* part_arg, void* stream);
/* g [B][P][C] -> gw [B*N][ldgw], gf [B*N][ldgf] (both fully written) */
int gpe_attn_pool_bwd(const float* w, int ldw, const float* feat, int ldf, const float* g, const int32_t* arg, int B,
                      int N, int P, int C, int mode, float* gw, int ldgw, float* gf, int ldgf, void* stream);

/* ---- PointNet++ set abstraction (PointNetPlusPlus, nn/net_blocks.py:10-88: torch_geometric fps / radius / PointConv) ------
 * pos [B][N][ldp>=C] (C <= 8).  gpe_fps: farthest point sampling of M points per cloud starting at LOCAL point start[b] (device
 * array [B]; NULL = point 0.  PyG's fps(random_start=True) draws it at random: the host mirror draws from torch's generator),
 * idx [B][M] LOCAL indices in selection order (ties -> lower index).  gpe_radius: for centroid s = (b, m) the first `maxn`
 * points of cloud b, ascending index, with squared distance <= r^2: nbr [B*M][maxn] local indices, cnt [B*M]. */
int gpe_fps(const float* pos, int ldp, int B, int N, int C, int M, const int32_t* start, int32_t* idx, void* stream);
int gpe_radius(const float* pos, int ldp, const int32_t* cidx, int B, int N, int C, int M, float r, int maxn,
               int32_t* nbr, int32_t* cnt, void* stream);
/* PyG PointNetConv(add_self_loops=True) on that edge list (nn/net_blocks.py:17,24 use the default): remove_self_loops drops the
 * edge whose flat source point number equals the flat centroid number s (drop[s] = its slot in nbr[s], -1 if none) and
 * add_self_loops appends s -> s; cnt_out[s] = cnt[s] - (drop[s] >= 0) + 1. */
int gpe_pointconv_self_loops(const int32_t* nbr, const int32_t* cnt, int B, int N, int M, int maxn, int32_t* cnt_out,
                             int32_t* drop, void* stream);
/* PointConv message inputs over the COMPACT edge list (edges of centroid s at rows off[s]..off[s+1]-1, off = exclusive scan of
 * the edge counts, int64 [B*M+1]): msg[e] = [x_j (Cx values, optional) | pos_j - pos_centroid]; seg_of_row[e] = s.  drop == NULL:
 * the edges are the ball-query neighbours (off from cnt); drop != NULL: PyG's re-indexed list (off from cnt_out; neighbour slot
 * drop[s] skipped, last edge = the loop from flat point s). */
int gpe_ball_messages(const float* pos, int ldp, const float* x, int ldx, int Cx, const int32_t* cidx, const int32_t* nbr,
                      const int64_t* off, const int32_t* drop, int B, int N, int C, int M, int maxn, float* msg, int ldm,
                      int32_t* seg_of_row, void* stream);
/* max over each ragged segment of rows (PointConv aggr = 'max'): y [S][ldy], arg [S][C] = winning row or -1 (empty -> 0) */
int gpe_ragged_max_fwd(const float* x, int ldx, const int64_t* off, long S, int C, float* y, int ldy, int64_t* arg,
                       void* stream);
int gpe_ragged_max_bwd(const float* gy, int ldgy, const int64_t* off, const int64_t* arg, const int32_t* seg_of_row, long E,
                       int C, float* gx, int ldgx, void* stream);

/* ---- loss (nn/metrics/composed_loss.py:294-334 main terms; nn/metrics/losses.py:19-51 PanelLoopLoss) ----------------
 * Predictions are strided views of the decoder outputs: outlines (b,p,l,c<4) at ol + b*ol_sb + p*ol_sp + l*ol_sl + c,
 * rotations (b,p,c<R) at rot + (b*P+p)*rot_s + c, translations likewise.  Ground truth dense fp32; num_edges int32 [B*P].
 * flags: 1 shape | 2 loop | 4 rotation | 8 translation.  pad0/pad1: the standardised padding vector's first two entries.
 * fwd: part [B][4] fp64 and loop_sums [B*P][2] are workspaces (loop_sums is re-used by bwd);
 *      out5 = {total, shape, loop, rotation, translation} (each term a mean, total = shape + loop_w*loop + rot + tr).
 * bwd: gradients of `total`, times the device scalar *gscale (NULL = 1), dense: g_ol [B,P,L,4], g_rot [B,P,R], g_tr [B,P,T];
 *      g_rot / g_tr may be NULL (not written).  num_edges > L acts as L, a negative count as 0 (a panel under 3 edges has no
 *      loop term, value or gradient; the loop gradient reaches columns 0-1 of the first n edges only). */
int gpe_pattern_loss_fwd(const float* ol, long ol_sb, long ol_sp, long ol_sl, const float* rot, long rot_s,
                         const float* tr, long tr_s, const float* gt_ol, const float* gt_rot, const float* gt_tr,
                         const int32_t* num_edges, int B, int P, int L, int R, int T, int flags, float pad0, float pad1,
                         float loop_w, double* part, float* loop_sums, float* out5, void* stream);
int gpe_pattern_loss_bwd(const float* ol, long ol_sb, long ol_sp, long ol_sl, const float* rot, long rot_s,
                         const float* tr, long tr_s, const float* gt_ol, const float* gt_rot, const float* gt_tr,
                         const int32_t* num_edges, int B, int P, int L, int R, int T, int flags, float pad0, float pad1,
                         float loop_w, const float* loop_sums, const float* gscale, float* g_ol, float* g_rot,
                         float* g_tr, void* stream);
/* panel-origin matching (composed_loss.py:656-703): gt_out [B,P,L,D] = each GT panel's edge loop cyclically shifted (first
 * num_edges rows only) to the FIRST shift with the smallest squared distance to the prediction; lead [B*P] = that shift. */
int gpe_origin_match(const float* ol, long ol_sb, long ol_sp, long ol_sl, const float* gt_ol, int D,
                     const int32_t* num_edges, int B, int P, int L, float* gt_out, int32_t* lead, void* stream);
/* greedy panel-order matching (composed_loss.py:530-570) on feature rows [B][P][D]: perm [B][P] int64 with
 * perm[b][pred panel] = gt panel; *fail set to 1 if a finite distance is left unmatched (the reference raises). */
int gpe_order_match(const float* pred_feat, const float* gt_feat, int B, int P, int D, int64_t* perm, int32_t* fail,
                    void* stream);

/* ---- stitch terms, active from `epoch_with_stitches` on (nn/metrics/composed_loss.py:336-362; PatternStitchLoss
 * nn/metrics/losses.py:54-180) --------------------------------------------------------------------------------------------
 * tags (b,p,l,d<D) at tags + b*t_sb + p*t_sp + l*t_sl + d and free-edge logits (b,p,l) at logit + b*m_sb + p*m_sp + l*m_sl
 * are strided views of the panel decoder's [B,P,L,8] output.  stitches int64 [B][2][S]: pattern-level edge ids
 * (panel * L + edge) of the two sides of every stitch, the first nums[b] (int64 [B]) of them valid; S <= 64, D <= 8.
 * gt_mask fp32 [B,P,L] (1 = free edge), gt_tags fp32 [B,P,L,D] (supervised variant only).
 * flags: 1 stitch (similarity + negative term) | 2 HardNet negative (closest other tag only, losses.py:148-180; default:
 * every other tag, :112-146) | 4 free-edge BCE-with-logits | 8 supervised tag MSE.
 * fwd: part [B][6] fp64 workspace (re-used by bwd); out5 = {total, similarity, negative, supervised, free} with
 *      total = (similarity + negative) + sup_w * supervised + free.  A pattern without stitches gives NaN (the reference
 *      divides by its zero stitch count as well).
 * bwd: gradient of `total` times the device scalar *gscale (NULL = 1), dense: g_tags [B,P,L,D], g_mask [B,P,L]; g_tags is
 *      required under bits 1 | 8 and g_mask under bit 4, either may be NULL otherwise.
 * Conventions: nums[b] outside [0, S] is clamped; entries past nums[b] are never read; an edge id outside [0, P*L) is clamped
 * (the reference would raise or wrap).  A pair of tags at a gap of exactly 0 (margin - d == 0) is inactive: the value is the
 * reference's, the gradient is 0, where the reference's autograd sends that pair's full gradient (HardNet: Python's max(t, 0)
 * returns t) or half of it (all pairs: torch.max(a, zeros) splits at equality).  Tied HardNet minima share the gradient equally,
 * as torch's min() does.  A pattern with nums[b] = 0 makes the similarity and the total NaN, as in the reference; every
 * gradient stays finite and that pattern's gradients are 0 apart from the supervised and free terms. */
int gpe_stitch_loss_fwd(const float* tags, long t_sb, long t_sp, long t_sl, int D, const float* logit, long m_sb, long m_sp,
                        long m_sl, const int64_t* stitches, const int64_t* nums, int S, const float* gt_mask,
                        const float* gt_tags, int B, int P, int L, int flags, float margin, float sup_w, double* part,
                        float* out5, void* stream);
int gpe_stitch_loss_bwd(const float* tags, long t_sb, long t_sp, long t_sl, int D, const float* logit, long m_sb, long m_sp,
                        long m_sl, const int64_t* stitches, const int64_t* nums, int S, const float* gt_mask,
                        const float* gt_tags, int B, int P, int L, int flags, float margin, float sup_w, const double* part,
                        const float* gscale, float* g_tags, float* g_mask, void* stream);
/* stitched-edge re-numbering of the ground truth (composed_loss.py:592-620 after the panel-order permutation `perm` int64
 * [B][P], then :727-755 for the panel-origin shift `lead` int32 [B*P] with `num_edges` int32 [B*P] of the permuted panels);
 * either step is skipped when its pointer is NULL.  out int64 [B][2][S]; entries past nums[b] (clamped to [0, S]) are copied;
 * there is no limit on S.  A panel moves to the LAST slot r with perm[b][r] == panel; a panel no slot names gets slot -1, and
 * the origin step then floor-divides the negative id (a negative flat panel number reads lead[0] / num_edges[0]). */
int gpe_stitch_renumber(const int64_t* stitches, const int64_t* nums, int B, int S, int P, int L, const int64_t* perm,
                        const int32_t* lead, const int32_t* num_edges, int64_t* out, void* stream);
/* per-edge ground truth [npanels][L][D] follows its panel's new loop origin (composed_loss.py:705-725 `_per_panel_shift`):
 * rows l < n of a panel with n = min(num_edges, L) >= 3 edges and 0 < lead < n become feat[(l + lead) mod n], everything else
 * (padding rows, shorter panels, a lead outside (0, n)) is copied. */
int gpe_panel_shift(const float* feat, int D, const int32_t* lead, const int32_t* num_edges, long npanels, int L, float* out,
                    void* stream);

/* ---- quality metrics of ComposedPatternLoss (nn/metrics/composed_loss.py:365-424; nn/metrics/metrics.py:13-325;
 * nn/data/datasets.py:917-968) --------------------------------------------------------------------------------------------
 * Added without a version bump (gpe_abi_version() stays 7): three compute entry points, nothing else changes.
 * flags: 1 discrete (panel / edge counts) | 2 shape (vertex L2) | 4 rotation L2 | 8 translation L2 | 16 stitch precision /
 * recall | 32 free-edge accuracy | 64 un-standardise the stitch tags (data_config['explicit_stitch_tags']).
 * stats_host: HOST array of 72 floats — [0:4] outline shift, [4:8] outline scale, [8:12] pad vector (standardised), [12:16]
 * isclose tolerance per feature (atol + |rtol * pad|), [16:18] loop-closure threshold (3 cm / scale), [24:32] rotation shift,
 * [32:40] rotation scale, [40:48] translation shift, [48:56] translation scale, [56:64] stitch-tag shift, [64:72] its scale.
 * part: caller-owned fp64 workspace of B * 16 doubles (B * 128 bytes), written by gpe_quality_panels (flags 1-8) and
 * gpe_quality_stitches (flags 16, 32) and read by gpe_quality_finalize, all with the same flags.  Limits: P, L <= 64,
 * R, T, D <= 8, P * L <= 1024.  The finalize kernel sums the per-pattern partials in pattern order (bit-reproducible).
 * panels: predicted outlines (b,p,l,c<4) at ol + b*ol_sb + p*ol_sp + l*ol_sl + c; gt_ol fp32 [B,P,L,4] dense; num_edges
 *         int32 [B*P] and num_panels int32 [B] of the ground truth; predicted rotation row (b,p) at rot + (b*P + p)*rot_s,
 *         gt_rot fp32 [B,P,R] dense; translations alike.
 * stitches: tags / logits as gpe_stitch_loss_fwd; stitches int64 [B][2][S] / nums int64 [B] the ground truth; gt_mask fp32
 *         [B,P,L] (1 = free).  Greedy pairing of the non-free edges' tags by global minimum distance, ties to the smallest
 *         (row, column) of the upper-triangular distance matrix.
 * finalize: out fp32 [14] = {num_panels_accuracy, num_edges_accuracy, corr_num_edges_accuracy, panel_shape_l2,
 *         corr_panel_shape_l2, rotation_l2, corr_rotation_l2, translation_l2, corr_translation_l2, stitch_precision,
 *         stitch_recall, corr_stitch_precision, corr_stitch_recall, free_edge_acc}; counts int32 [4] = {patterns with the
 *         right panel count, shape panels of those, those with detected stitches, all shape panels}: the contributors of
 *         the corr_ slots (0 = the reference's None). */
int gpe_quality_panels(const float* ol, long ol_sb, long ol_sp, long ol_sl, const float* gt_ol, const int32_t* num_edges,
                       const int32_t* num_panels, const float* rot, long rot_s, const float* gt_rot, int R, const float* tr,
                       long tr_s, const float* gt_tr, int T, int B, int P, int L, int flags, const float* stats_host,
                       double* part, void* stream);
int gpe_quality_stitches(const float* tags, long t_sb, long t_sp, long t_sl, int D, const float* logit, long m_sb, long m_sp,
                         long m_sl, const int64_t* stitches, const int64_t* nums, int S, const float* gt_mask, int B, int P,
                         int L, int flags, const float* stats_host, double* part, void* stream);
int gpe_quality_finalize(const double* part, int B, int P, int L, int flags, float* out, int32_t* counts, void* stream);

/* ---- a prediction decoded to a sewing pattern (Garment3DPatternFullDataset._pred_to_pattern, nn/data/datasets.py:731-767;
 * tags_to_stitches :917-968; NNSewingPattern.pattern_from_tensors / panel_from_numeric / _edge_dict,
 * nn/data/pattern_converter.py:118-187, 228-271, 510-515) ----------------------------------------------------------------
 * Added without a version bump (gpe_abi_version() stays 7): two compute entry points, nothing else changes.  All memory is the
 * caller's; the library keeps no state.  One launch of B workgroups (one wave each), no atomics: bit-reproducible.
 * Inputs: outlines / rotation / translation rows as gpe_quality_panels, tags / logits as gpe_quality_stitches (the strided
 * views of the decoders' output).  stats_host: HOST array of 64 doubles, eight per group — [0:8] outline shift, [8:16] outline
 * scale, [16:24] rotation shift, [24:32] its scale, [32:40] translation shift, [40:48] its scale, [48:56] stitch-tag shift,
 * [56:64] its scale.  Every outline, rotation and translation value is un-standardised as fp64 (double)x * scale, then + shift,
 * each rounded (numpy on float64).  flags: 1 = un-standardise the stitch tags too (fp32, as gpe_quality_stitches flag 64).
 * given: int32 [B][2][S] caller's stitches (edge ids panel * L + edge) that replace the tag pairing, given_num int32 [B] how many
 * of the S entries count (NULL: all); given == NULL pairs the tags (tags_to_stitches: greedy by global minimum distance, ties to the
 * smallest (row, column); an odd count of non-free edges drops the one with the largest logit) and needs S == P * L / 2.
 * Menu: 1 <= P * L <= 1024, R, T, D in 1 .. 8; anything else returns -22 before any launch.
 * Panel (b,p): a row is kept unless all four values are within 1.5 of 0 (NaN / inf keep it); fewer than 3 kept rows = empty panel
 * (num_edges 0, num_verts 0, new_panel_id -1).  Else vertex 0 = origin, vertex k + 1 = vertex k + kept edge k's first two values
 * (sequential fp64 sums); closed = the end of the last edge is within 3 of 0 in both coordinates, then the last edge ends at vertex
 * 0 and num_verts = num_edges, else num_verts = num_edges + 1.  Kept edge k: edge_slot = its row, curvature = its last two values,
 * curved = not both within 0.01 of 0.
 * Outputs: num_edges, num_verts, closed, new_panel_id (rank among the non-empty panels) int32 [B][P]; edge_slot, curved int32
 * [B][P][L]; num_panels int32 [B]; vertices fp64 [B][P][L + 1][2]; curvature fp64 [B][P][L][2]; rotations fp64 [B][P][R];
 * translations fp64 [B][P][T] (the universal translation, passed through); stitches int32 [B][2][S] in the order found (given:
 * the non-(0, 0) entries in order); num_stitches, first_invalid int32 [B]; stitch_flags int32 [B][S]: bit 0 = an id names a panel
 * >= P or an empty one (first_invalid = the first such stitch, -1: none), bit 1 = an id names a row that was dropped (the reference
 * does not notice).  The reported edge of an id is id % L, the row, not the kept-edge index.  Tails are written: -1 (edge_slot) or 0.
 * gpe_tags_to_stitches: the pairing alone, tags as they are (the reference's static method, batched): stitches int32 [B][2][S] with
 * S = P * L / 2 in the order taken, zero tails; num_stitches int32 [B].  Same menu, same kernel code (csrc/gpe_stitch_greedy.h). */
int gpe_tags_to_stitches(const float* tags, long t_sb, long t_sp, long t_sl, int D, const float* logit, long m_sb, long m_sp,
                         long m_sl, int B, int P, int L, int32_t* stitches, int32_t* num_stitches, void* stream);
int gpe_pattern_decode(const float* ol, long ol_sb, long ol_sp, long ol_sl, const float* rot, long rot_s, int R, const float* tr,
                       long tr_s, int T, const float* tags, long t_sb, long t_sp, long t_sl, int D, const float* logit, long m_sb,
                       long m_sp, long m_sl, const int32_t* given, const int32_t* given_num, int B, int P, int L, int S, int flags,
                       const double* stats_host, int32_t* num_edges, int32_t* edge_slot, int32_t* num_verts, int32_t* closed,
                       int32_t* new_panel_id, int32_t* num_panels, double* vertices, double* curvature, double* rotations,
                       double* translations, int32_t* curved, int32_t* stitches, int32_t* num_stitches, int32_t* stitch_flags,
                       int32_t* first_invalid, void* stream);

/* ---- graph pooling: DynamicASAPool = PyG ASAPooling on the kNN graph of the node features (nn/net_blocks.py:194-218, used by
 * EdgeConvFeatures with graph_pooling (:113-118, :138-142, :172-176) and EdgeConvPoolingFeatures (:221-268)) -------------------
 * Added without a version bump (gpe_abi_version() stays 7): two compute entry points, nothing else changes.
 * Graph: idx [B][N][k] of gpe_knn on x with k = min(10, N) (the reference fixes k = 10, :204) and its transpose rev_off / rev_edge
 * of gpe_knn_reverse.  torch_cluster's rows are [query, neighbour] and ASAPooling sends from row 0 to row 1, so target c receives
 * from every q with c in kNN(q); add_remaining_self_loops drops a q == c edge and appends one self-loop:
 *   cluster(c) = {c} + {q != c : c in kNN(q)},  deg(c) = |cluster(c)|.
 * Forward (fp32 in every arithmetic mode): x_q[c] = channel max over cluster(c) (ties: lowest source index);
 * s_cq = leaky_relu(att([lin(x_q[c]) | x[q]]), 0.2), folded as u . x_q[c] + s0 + w_x . x[q] with u = W_lin^T w_q,
 * s0 = w_q . b_lin + b_att (att.weight = [w_q | w_x]); alpha = softmax over cluster(c) (max-subtracted, denominator + 1e-16);
 * x'_c = sum alpha_cq x[q]; fitness_c = sigmoid(sum_{q in cluster(c)} lin1(x'_q) - deg(c) lin2(x'_c) + lin3(x'_c)) (LEConv);
 * per cloud the M nodes of highest fitness, in descending fitness, ties to the lower index (PyG topk); M is the caller's
 * ceil(fp32(ratio) * fp32(N)).  out [B*M][F] = x'[perm] * fitness[perm]; perm int32 [B*M] = GLOBAL rows b*N + c; rank int32
 * [B*N] = the output row of a kept node, -1 otherwise.  The coarsened edge list of ASAPooling is not built (the reference discards
 * it).  Parameters in PyG 2.x's layout: w_lin [F][F], b_lin [F], w_att [1][2F], b_att [1], w1 [1][F], b1 [1], w2 [1][F] (no
 * bias), w3 [1][F], b3 [1] (gnn_score.lin1 / lin2 / lin3).
 * state: caller-owned, 16-B aligned, 4 * (1024 + B*N*(2F + k + 8)) bytes, written by gpe_asap_fwd and read by gpe_asap_bwd
 * (x', channel-max winners, alpha, scores, fitness, degrees).
 * Backward: dout [B*M][F] dense -> dx [B*N][lddx >= F] and the nine parameter gradients (same shapes as the parameters; written,
 * not accumulated).  No atomics: per-node pulls over the kNN lists and the reverse buckets, parameter sums in fp64 per workgroup
 * partial and combined in a fixed order (bit-reproducible).  ws: caller-owned, 16-B aligned,
 *   8 * (nblk + 1) * (5F + 3) + 4 * B*N*(F + k + 4) bytes,   nblk = min(ceil(B*N / 16), 1024).
 * Limits: 1 <= F <= 512, 1 <= N <= 8192, 1 <= k <= min(64, N), 1 <= M <= N, ldx >= F; anything else returns -22.
 * Launches: forward 3 (prep: w_x . x and the folded u, s0; cluster: one wave per target; select: one workgroup per cloud, bitonic
 * sort of 64-bit keys in LDS), backward 5 (dfitness; per-target G and attention backward; per-source pull + partials; column
 * sums; finalize). */
int gpe_asap_fwd(const float* x, int ldx, int B, int N, int F, int k, const int32_t* rev_off, const int32_t* rev_edge,
                 const float* w_lin, const float* b_lin, const float* w_att, const float* b_att, const float* w1, const float* b1,
                 const float* w2, const float* w3, const float* b3, int M, float* out, int32_t* perm, int32_t* rank, float* state,
                 void* stream);
int gpe_asap_bwd(const float* dout, const float* x, int ldx, int B, int N, int F, int k, const int32_t* idx, const int32_t* rev_off,
                 const int32_t* rev_edge, const float* w_lin, const float* b_lin, const float* w_att, const float* b_att,
                 const float* w1, const float* b1, const float* w2, const float* w3, const float* b3, const int32_t* rank,
                 const float* state, float* dx, int lddx, float* g_wlin, float* g_blin, float* g_watt, float* g_batt, float* g_w1,
                 float* g_b1, float* g_w2, float* g_w3, float* g_b3, void* ws, void* stream);

/* ---- stitch recovery from the edge-pair classifier (StitchOnEdge3DPairs at prediction time: nn/data/pattern_converter.py:411-499
 * all_edge_pairs + stitches_from_pair_classifier; forward only) ---------------------------------------------------------------------
 * Added without a version bump (gpe_abi_version() stays 7): six compute entry points, nothing else changes.
 * Garment b has P panel slots of L edge slots; num_edges int32 [B][P] (clamped to 0 .. L; 0 = panel absent).  Pattern-level edge id
 * e = panel * L + edge, E = P * L.  Pairs: (panel i, edge r) x (panel j, edge c), i < j, r < num_edges[i], c < num_edges[j]; order
 * key (i, j, r, c) lexicographic, packed as i << 13 | j << 8 | r << 4 | c.  A pair is positive iff sigmoid(logit) > 0.5 in fp32.
 * table: caller-owned uint64 [B][E], ZEROED by the caller; every positive pair does a 64-bit atomicMax of
 *   (bit pattern of its logit) << 32 | ~key   on the entries of both of its edges (positive logits order like their bit patterns, the
 * complement makes the earlier pair win a tie), so an entry ends as the edge's best pair whatever the arrival order.
 * logits (may be NULL): fp32 [B][E][E], entry (e_i, e_j) of every valid pair is written, nothing else is touched.
 * Limits: 1 <= P <= 32, 1 <= L <= 16, 1 <= B <= 65535; anything else returns -22.
 *
 * gpe_stitch_pairs_fwd, the fused store-free classifier.  The first Linear is split per edge, W1 [e_i | e_j] + b1 = A_i + Bv_j:
 *   ab [B*E][ldab] fp32 holds [A | Bv] (2 H columns, 16-B aligned rows; the standardisation folded in; gpe_linear writes it).
 *   n_layers = Linear layers in front of the output Linear (1 .. 4, all H wide: H <= 256, H % 4 == 0), each followed by ReLU and an
 *   eval-mode BatchNorm that is folded into the next Linear.  wpk (16-B aligned) holds, with NB = the smallest of {4, 8, 13, 16}
 *   >= ceil(H / 16) and ldw = 16 NB (+ 16 unless 16 NB % 32 == 16):
 *     for each of the n_layers - 1 hidden H x H layers: Wt [H][ldw] = gpe_stitch_pairs_pack(w, .., col_scale = s of the BatchNorm
 *       in front, ldo = ldw), then the folded bias (gpe_fold_bias) in a zero-filled row of ldw floats;
 *     then the output layer: H floats (gpe_stitch_pairs_pack with N = 1, ldo = 1) and its folded bias (1 float)
 *   = (n_layers - 1) * (H + 1) * ldw + H + 1 floats.  last_stats [4][1] = gpe_bn_from_running of the output block:
 *   logit = s * relu(z) + t.  A workgroup classifies 8 x 8 edges (64 pairs) on v_mfma_f32_16x16x4_f32;
 *   dynamic LDS 4 * (64 * ((H/4 | 1) * 4) + 32 * ldw) bytes.
 *   f16x3 (gpe_math_set(4), H <= 224, B * E * E / 2 >= gpe_f16x3_min_rows(), planes and w_amax given; otherwise the exact kernel):
 *   three v_mfma_f32_16x16x32_f16 per product on two-term fp16 splits, fp32 accumulate; the weights are normalised per layer,
 *   w_amax uint32 [n_layers - 1] = amax words of the hidden layers' Wt (gpe_absmax over [H][ldw]) and planes = per hidden layer
 *   KP * ldw floats written by gpe_stitch_pairs_planes (KP = H rounded up to 32), 16-B aligned; the activations are normalised per
 *   wave (32 pair rows) and layer by the maximum found in the accumulators.  A workgroup classifies 8 x 16 edges; dynamic LDS
 *   4 * (128 * (KP + 8) + 32 * ldw) bytes.  Both may be NULL.  Other modes run the exact kernel.
 * gpe_stitch_pairs_pack: out[k][n] = w[n][k] * col_scale[k] (col_scale may be NULL) for k < K, n < N, zero for N <= n < ldo.
 * gpe_stitch_pairs_planes: wt [K][ldw] (a gpe_stitch_pairs_pack output, ldw % 16 == 0) scaled by the power of two of its amax word
 *   and split in two fp16 terms, in the B-fragment order of v_mfma_f32_16x16x32_f16: per 32-k slab [hi | lo][4][ldw][8 halves].
 *
 * The generic route (any MLP): i-edge e = (panel q, edge r) owns the E - (q + 1) L rows of the edge slots of the later panels,
 * starting at row off(e) = L q E - L^2 q (q + 1) / 2 + r (E - (q + 1) L); a call handles the i-edges [c0, c1) of every garment,
 * rows_chunk >= off(c1) - off(c0) rows per garment, B * (c1 - c0) <= 65535.
 * gpe_stitch_pairs_rows writes rows [B][rows_chunk][2 Fe] = ([e_i | e_j] - shift) / scale (HOST arrays of 2 Fe floats, Fe <= 16;
 *   edges3d fp32 [B][E][Fe] dense), zero rows for edge slots that are not present;
 * gpe_stitch_pairs_reduce reads the classifier's output y (row pitch ldy) in the same order and applies the epilogue above.
 *
 * gpe_stitch_select: a pair survives iff the entries of both of its edges name it.  stitches int32 [B][2][S], S = E / 2: the edge
 * ids of the survivors (side 0 = lower panel) in ascending order key, zero-padded; num_stitches int32 [B]; scores fp32 [B][S] the
 * logits.  One workgroup per garment, no atomics on global memory: bit-reproducible. */
int gpe_stitch_pairs_pack(const float* w, int ldw, int N, int K, const float* col_scale, float* out, int ldo, void* stream);
int gpe_stitch_pairs_planes(const float* wt, int K, int ldw, const uint32_t* amax, void* out, void* stream);
int gpe_stitch_pairs_fwd(const float* ab, int ldab, int H, int n_layers, const float* wpk, const void* planes,
                         const uint32_t* w_amax, const float* last_stats, const int32_t* num_edges, int B, int P, int L,
                         uint64_t* table, float* logits, void* stream);
int gpe_stitch_pairs_rows(const float* edges3d, const int32_t* num_edges, int B, int P, int L, int Fe, const float* shift_host,
                          const float* scale_host, int c0, int c1, long rows_chunk, float* rows, void* stream);
int gpe_stitch_pairs_reduce(const float* y, long ldy, const int32_t* num_edges, int B, int P, int L, int c0, int c1,
                            long rows_chunk, uint64_t* table, float* logits, void* stream);
int gpe_stitch_select(const uint64_t* table, int B, int P, int L, int32_t* stitches, int32_t* num_stitches, float* scores,
                      void* stream);

/* ---- the same pass scored against ground-truth stitches (nn/metrics/composed_loss.py:83-126 ComposedLoss over the pairs and
 * labels of all_edge_pairs, nn/data/pattern_converter.py:458-499) ----------------------------------------------------------------
 * Added without a version bump (gpe_abi_version() stays 7): four compute entry points, nothing else changes.  Every workspace is
 * the caller's and ZEROED by the caller; sizes are the formulas below (no size query).  With W = ceil(E / 32), N8 = ceil(E / 8):
 *   mask      uint32 [B][E][W]: bit (e_j % 32) of word [e_i][e_j / 32] = pair (e_i, e_j) is a ground-truth stitch; symmetric.
 *   loss_slab fp64 [B][slots]: one slot per workgroup of the classifying launch, written (not added to) by its owner.
 *             gpe_stitch_pairs_eval_fwd: slots = N8 * N8, tile (ti, tj) of either fused kernel owns slot ti * N8 + tj;
 *             gpe_stitch_pairs_eval_reduce: slots = E, the workgroup of i-edge e owns slot e (all chunks share one slab).
 *   counters  uint64 [B][2]: word 0 = pairs | correct << 32, word 1 = true positives | predicted positives << 21 |
 *             ground-truth positives << 42 (a garment has fewer than 2^17 pairs), added by 64-bit integer atomics.
 * gpe_stitch_pairs_labels: gt_stitches int32 [B][2][S] of edge ids panel * L + edge (the layout of the stitch losses), gt_num_stitches
 *   int32 [B] clamped to 0 .. S.  Sets bits (a, b) and (b, a) of every stitch; an entry with an id outside 0 .. E - 1 is ignored,
 *   duplicates are harmless, S = 0 launches nothing.  Bits of same-panel pairs or absent edges are never read: only enumerated
 *   pairs consult the mask, as `pair_id in stitch_set or reversed in stitch_set` does over the reference's enumeration.
 * gpe_stitch_pairs_eval_fwd / gpe_stitch_pairs_eval_reduce: the operands and results of gpe_stitch_pairs_fwd / _reduce (table and
 *   logits are filled bit-identically) plus, for every pair with logit x and label y, the term relu(-x if y else x) +
 *   log1p(exp(-|x|)) (BCE with logits, both summands non-negative, fp32) accumulated in fp64, and the counters with the class
 *   sigmoid(x) > 0.5 of the selection.  Inside a workgroup the sums run in a fixed order (xor butterfly in a wave, then the waves
 *   in order through LDS); no float atomics, no workgroup waits on another: bit-reproducible, and independent of unused panel or
 *   edge slots (the rows route walks the present edges in position order, one workgroup per i-edge).
 * gpe_stitch_eval_finalize: one launch of one workgroup after gpe_stitch_select.  `group` consecutive slots form a group
 *   (slots % group == 0, at most 64 groups: group = N8 after _eval_fwd, group = L after _eval_reduce); a group is added in slot
 *   order, then the groups in order.  loss_sum fp64 [B]; counts int32 [B][6] = pairs, correct, true positives, predicted positives,
 *   ground-truth positives, selected_tp (stitches written by gpe_stitch_select whose pair is in the mask); metrics fp32 [6] pooled
 *   over the call = edge_pair_class_loss (sum of loss_sum in garment order / sum of pairs), edge_pair_class_acc, stitch_precision,
 *   stitch_recall, selected_precision (selected_tp / stitches selected), selected_recall (selected_tp / ground-truth positives).
 *   A ratio whose denominator is 0 is 0 (composed_loss.py:123-124). */
int gpe_stitch_pairs_labels(const int32_t* gt_stitches, const int32_t* gt_num_stitches, int B, int P, int L, int S, uint32_t* mask,
                            void* stream);
int gpe_stitch_pairs_eval_fwd(const float* ab, int ldab, int H, int n_layers, const float* wpk, const void* planes,
                              const uint32_t* w_amax, const float* last_stats, const int32_t* num_edges, int B, int P, int L,
                              uint64_t* table, float* logits, const uint32_t* mask, double* loss_slab, uint64_t* counters,
                              void* stream);
int gpe_stitch_pairs_eval_reduce(const float* y, long ldy, const int32_t* num_edges, int B, int P, int L, int c0, int c1,
                                 long rows_chunk, uint64_t* table, float* logits, const uint32_t* mask, double* loss_slab,
                                 uint64_t* counters, void* stream);
int gpe_stitch_eval_finalize(const double* loss_slab, long slots, int group, const uint64_t* counters, const uint32_t* mask,
                             const int32_t* stitches, const int32_t* num_stitches, int B, int P, int L, double* loss_sum,
                             int32_t* counts, float* metrics, void* stream);

/* ---- one DynamicEdgeConv layer at prediction time, nothing stored per edge (nn/net_blocks.py:43-47,124-135,174 under eval():
 * the edge MLP's [Linear -> ReLU -> BatchNorm] blocks on [x_i | x_j - x_i] of the kNN graph and the aggregation over the k messages) -
 * Added without a version bump (gpe_abi_version() stays 7): one compute entry point and one host-only query, nothing else changes.
 * The caller owns every byte; the library allocates nothing.
 * Menu: 1 <= k <= 64; H (the width of every block but the last) <= 256 and a multiple of 4 (the [P|Q] rows are read in quads); F (the
 * last block's width) 1 .. 256; n_hidden = H -> H Linears between the first block and the last, 0 .. 3 (the edge MLP has n_hidden + 2
 * blocks).  Anything else returns -22 before any
 * launch; gpe_edge_predict_ok answers the same question (1 / 0) on the host (its stream argument is ignored).
 * gpe_edge_predict_fwd, one launch per layer:
 *   pq [BN][ldpq] fp32 = [P | Q] of the first Linear (2 H columns, 16-B aligned rows, ldpq % 4 == 0; gpe_w1_split + gpe_linear write
 *   it), message (i, j) starts as relu(P_i + Q_j); jg int32 [BN * k] = global neighbour rows (gpe_knn's idx_global; values are clamped
 *   to 0 .. BN - 1); BN = B * N point rows, BN * k < 2^31.  A tile of points may span clouds: nothing depends on cloud boundaries.
 *   wpk (16-B aligned), with nb(W) = the smallest of {4, 8, 13, 16} >= ceil(W / 16) and ldw(W) = 16 nb (+ 16 unless 16 nb % 32 == 16):
 *     for each hidden layer: Wt [H][ldw(H)] = gpe_stitch_pairs_pack(w, .., col_scale = s of the BatchNorm in front, ldo = ldw(H)), then
 *       the folded bias (gpe_fold_bias with t of that BatchNorm) in a zero-filled row of ldw(H) floats;
 *     then the last layer alike: Wt [H][ldw(F)] and its bias row of ldw(F) floats
 *   = n_hidden * (H + 1) * ldw(H) + (H + 1) * ldw(F) floats.  last_stats [4][F] = gpe_bn_from_running of the last block.
 *   aggr 0 / 1 / 2 = max / mean / add; out [BN][ldo] fp32 (ldo >= F), with m = the message's last relu output:
 *     max: s_c >= 0 ? s_c max_j m + t_c : s_c min_j m + t_c (gpe_edge_finish's rule);  mean: s_c (sum_j m / k) + t_c;
 *     add: s_c sum_j m + k t_c.
 *   Exact kernel: a workgroup owns floor(64 / k) consecutive point rows and their edge rows on v_mfma_f32_16x16x4_f32; dynamic LDS
 *   4 * (64 * lda(max(H, F)) + 32 * max(ldw(H), ldw(F))) bytes, lda(W) = (ceil(W / 4) | 1) * 4.
 *   f16x3 (gpe_math_set(4), H and F <= 224, BN * k >= gpe_f16x3_min_rows(), planes and w_amax given; otherwise the exact kernel): three
 *   v_mfma_f32_16x16x32_f16 per product on two-term fp16 splits, fp32 accumulate, floor(128 / k) point rows per workgroup; w_amax uint32
 *   [n_hidden + 1] = amax words of the layers' Wt (gpe_absmax over [H][ldw]), planes = per layer KP * ldw floats written by
 *   gpe_stitch_pairs_planes (KP = H rounded up to 32), 16-B aligned; the activations are normalised per wave (32 edge rows) and layer by
 *   the maximum found in the accumulators.  Dynamic LDS max(4 * (128 * (KP + 8) + 32 * max ldw), 4 * 128 * lda(F)) bytes.
 *   Both may be NULL.  Other modes run the exact kernel.  No atomics, no workgroup waits on another: bit-reproducible. */
int gpe_edge_predict_ok(int k, int H, int F, int n_hidden, void* stream);
int gpe_edge_predict_fwd(const float* pq, int ldpq, const int32_t* jg, long BN, int k, int H, int F, int n_hidden, const float* wpk,
                         const void* planes, const uint32_t* w_amax, const float* last_stats, int aggr, float* out, int ldo,
                         void* stream);

/* ---- the training loss of the same classifier on a batch of sampled pair rows (nn/metrics/composed_loss.py:83-126 ComposedLoss as
 * StitchOnEdge3DPairs calls it in training) ------------------------------------------------------------------------------------------
 * Added without a version bump (gpe_abi_version() stays 7): two compute entry points, nothing else changes.
 * x fp32 [M] dense logits; y the labels, kind 0 = bytes (uint8 / bool), kind 1 = fp32; 0 <= M < 2^31.  All memory is the caller's.
 * gpe_pair_loss_fwd, one launch of `slots` workgroups (1 .. 256): BCEWithLogitsLoss (mean) with the terms max(x, 0) - x y +
 *   log1p(exp(-|x|)) in fp32 (for y in {0, 1}: relu(-x if y else x) + log1p(exp(-|x|)), as the evaluating kernels above) summed in
 *   fp64, and the counters of the class sigmoid(x) > 0.5 (fp32, as the selection above): correct = class == y, positive label =
 *   y == 1.  Slot s owns the rows [s * ceil(M / slots), (s + 1) * ceil(M / slots)): the result depends on `slots`, not on the device.
 *   Inside a workgroup the sums run in a fixed order (a thread's rows in order, xor butterfly in a wave, then the waves in order
 *   through LDS); the workgroup that draws the last ticket adds the slots in slot order.  Nobody waits, no float atomics:
 *   bit-reproducible.  part: slots * 32 bytes, 8-B aligned, need not be cleared; ticket: one ZEROED uint32, left zero (the word of
 *   gpe_pack_fold may be shared by calls on one stream).
 *   out fp32 [4] = edge_pair_class_loss, edge_pair_class_acc, stitch_precision, stitch_recall, the ratios as float32 quotients of
 *   the counts; a ratio whose denominator is 0 is 0 (composed_loss.py:123-124), M = 0 gives a NaN loss (the mean of nothing).
 *   counts int32 [5] = rows, correct, true positives, predicted positives, ground-truth positives.
 * gpe_pair_loss_bwd, one launch: gx[i] = gscale[0] * (sigmoid(x[i]) - y[i]) / M, gscale a DEVICE scalar (the upstream gradient of
 *   the loss); gx fp32 [M].  M = 0 launches nothing. */
int gpe_pair_loss_fwd(const float* x, const void* y, int kind, long M, int slots, void* part, uint32_t* ticket, float* out,
                      int32_t* counts, void* stream);
int gpe_pair_loss_bwd(const float* x, const void* y, int kind, long M, const float* gscale, float* gx, void* stream);

/* ---- the sampled pair rows of that training, drawn on the device (NNSewingPattern.stitches_as_3D_pairs,
 * nn/data/pattern_converter.py:321-409, then FeatureStandartization) ----------------------------------------------------------------
 * Added without a version bump (gpe_abi_version() stays 7): one compute entry point, nothing else changes.  All memory is the
 * caller's; the library keeps no state.
 * The resident set: edges3d fp32 [G][P][L][Fe] (Fe <= 16, E = P * L <= 512), num_edges int32 [G][P] (clamped to 0 .. L; 0 = panel
 * absent), gt_stitches int32 [G][2][S] of edge ids panel * L + edge and gt_num_stitches int32 [G] (clamped to 0 .. S), the operands
 * of gpe_stitch_pairs_labels; gt_stitches may be NULL when S == 0.  index int32 [B]: the garment of every batch slot, 1 <= B <= 2^24.
 * One launch of B workgroups writes, with R = n_stitched + n_non_stitched (1 .. 4096; both >= 0):
 *   rows   fp32 [B][R][2 Fe] = ([e_a | e_b] - shift) / scale, fp32 subtract then divide as gpe_stitch_pairs_rows (shift_host /
 *          scale_host: HOST arrays of 2 Fe floats); 16-byte stores when Fe is even and rows is 16-byte aligned;
 *   labels uint8 [B][R], 0 / 1 (kind 0 of gpe_pair_loss_fwd);
 *   status int32 [B]: >= 0 the rows that gave up; -1 more valid stitches than n_stitched; -2 index[b] outside 0 .. G - 1 (all rows
 *          and labels of such a slot are zero).
 * Per slot, before the shuffle: rows [0, S_v) are the valid stitches in order (both ids in 0 .. E - 1 and present), label 1; rows
 * [S_v, n_stitched) copy a uniformly chosen row below S_v as stored, label 1; the remaining rows (all R when S_v == 0) are
 * non-stitched, label 0: an attempt draws a present panel, an edge of it, and the same again, and is rejected when both sides are
 * the same edge or the pair is a valid stitch in either orientation; after 64 rejected attempts the row gives up (zeros, label 0).
 * flags bit 0 (shuffle_pairs; needs Fe == 8, the [start xyz | end xyz | cx cy] layout): every present edge is reversed with
 * probability 1/2 once per slot (endpoints swapped, cx' = cx ? 1 - cx : 0, cy' = -cy) and every valid stitch row has its halves
 * swapped with probability 1/2.  flags bit 1 (shuffle_pairs_order): row r moves to the rank of (key_r, r), key_r a 32-bit draw.
 * Random numbers: Philox4x32-10, key = (seed lo, seed hi), counter = (item | kind << 28, attempt | b << 8, draw lo, draw hi); an
 * integer in [0, n) is (uint64(word) * n) >> 32.
 *   kind 0 flip: item = edge id, bit 31 of word 0          kind 1 stitch swap: item = rank of the valid stitch, bit 31 of word 0
 *   kind 2 duplicate choice: item = row, word 0            kind 3 non-stitched attempt: item = index among the non-stitched rows,
 *   kind 4 order key: item = pre-shuffle row, word 0         attempt = 0 .. 63, words 0 - 3 = panel, edge, panel, edge
 * The result is a function of (seed, draw, b, inputs) only.  state uint64 [2] = {seed, draw} in DEVICE memory, 8-byte aligned: the
 * launch stores draw + 1 after every workgroup has read it (the last-arriver ticket of gpe_pack_fold, nobody waits), so a captured
 * launch draws anew on every replay.  ticket: one ZEROED uint32 of its own, left zero.
 * -EINVAL before any launch: a NULL pointer, Fe > 16, Fe != 8 with bit 0 set, unknown flag bits, P * L > 512, R outside 1 .. 4096,
 * B < 1. */
int gpe_stitch_sample(const float* edges3d, const int32_t* num_edges, const int32_t* gt_stitches, const int32_t* gt_num_stitches,
                      int G, int P, int L, int Fe, int S, const int32_t* index, int B, int n_stitched, int n_non_stitched,
                      int flags /* bit 0 shuffle_pairs, bit 1 shuffle_pairs_order */, const float* shift_host, const float* scale_host,
                      uint64_t* state /* device: {seed, draw} */, uint32_t* ticket, float* rows, uint8_t* labels, int32_t* status,
                      void* stream);


/* ---- the encoder's input point clouds drawn on the device from resident meshes (Garment3DPatternFullDataset._get_sample_info,
 * nn/data/datasets.py: igl.random_points_on_mesh, the barycentric -> world loop, the Gaussian noise, igl.snap_points twice,
 * FeatureStandartization) -----------------------------------------------------------------------------------------------------------
 * Added without a version bump (gpe_abi_version() stays 7): one compute entry point, nothing else changes.  All memory is the
 * caller's; the library keeps no state.
 * The resident set, ragged over G garments: verts4 fp32 [sum V][4] = {x, y, z, the bits of the int32 class id; -1 = a stitch / None
 * vertex}, 16-byte aligned; faces int32 [sum F][3], indices local to the garment (the caller has checked them against 0 .. V - 1;
 * the kernel holds them inside the garment all the same); vert_off, face_off int32 [G + 1]; face_cdf uint32 [sum F]: per garment
 * T[f] = floor(2^31 C_f / C_total), C the inclusive cumulative sum of the face areas, and T[f] = 2^31 exactly from the last face of
 * positive area onwards (a garment without one has no 2^31 at its end).  index int32 [B]: the garment of every batch slot.
 * Slot b, point n < N (one launch of B * ceil(N / 512) workgroups; a second one of the same grid when relabel != 0):
 *   face         w = word 0 >> 1 of kind 8: the first face f of the garment with T[f] > w (binary search)
 *   barycentric  iu = word 1 >> 8, iv = word 2 >> 8; iu + iv > 2^24 reflects both (i <- 2^24 - i); b1 = iu 2^-24, b2 = iv 2^-24,
 *                b0 = (2^24 - iu - iv) 2^-24; p = (b0 A + b1 B) + b2 C per axis, every product and sum rounded on its own
 *   noise        point_noise_w != 0 only, kind 9: Box-Muller with u1 = ((word >> 8) + 1) 2^-24, u2 = (word >> 8) 2^-24,
 *                r = sqrtf(-2 logf(u1)): words 0, 1 -> x += w (r cospif(2 u2)), y += w (r sinpif(2 u2)); words 2, 3 -> z += w (r
 *                cospif(2 u2)); the multiply and the add each rounded
 *   label        that of the vertex nearest to the noisy p: the lexicographic minimum of (d, vertex), d = (dx dx + dy dy) + dz dz,
 *                every operation rounded on its own
 *   re-label     relabel != 0 (needed exactly when the resident set has a -1 vertex; without it a -1 stays in the output): a point
 *                labelled -1 takes the label of the nearest point of its own cloud whose label is >= 0, the lower point winning a
 *                tie; no such point: label 0, counted in status[b].  ws: fp32 [B][N][4] of the caller's, 16-byte aligned (may be
 *                NULL when relabel == 0)
 * features fp32 [B][N][3] = (p - shift) / scale, the fp32 subtract-then-divide of gpe_standardize (shift_host / scale_host: HOST
 * arrays of 3 floats; both NULL: p itself); segmentation int64 [B][N]; status int32 [B]: >= 0 the points that fell back to label 0;
 * -1 a garment without a face of positive area; -2 index[b] outside 0 .. G - 1 (features and segmentation of such a slot are zero).
 * Random numbers: the Philox4x32-10 blocks of gpe_stitch_sample, key = (seed lo, seed hi), counter = (n | kind << 28, b << 8, draw
 * lo, draw hi), kinds 8 and 9.  The result is a function of (seed, draw, b, inputs) only.  state uint64 [2] = {seed, draw} in DEVICE
 * memory, 8-byte aligned: the first launch stores draw + 1 after every workgroup has read it (last-arriver ticket, nobody waits);
 * ticket: one ZEROED uint32 of its own, left zero.
 * -EINVAL before any launch: a NULL pointer (ws with relabel; one of shift_host / scale_host alone), a misaligned verts4 / ws /
 * state, G < 1, B < 1, B >= 2^24, N < 1, N >= 2^28, B * ceil(N / 512) >= 2^31. */
int gpe_mesh_points_sample(const float* verts4, const int32_t* faces, const int32_t* vert_off, const int32_t* face_off,
                           const uint32_t* face_cdf, int G, const int32_t* index, int B, int N, float point_noise_w,
                           const float* shift_host, const float* scale_host, int relabel, float* ws,
                           uint64_t* state /* device: {seed, draw} */, uint32_t* ticket, float* features, int64_t* segmentation,
                           int32_t* status, void* stream);

/* ---- optimizer / input side (nn/trainer.py:162-185; nn/data/transforms.py:35-50) ----------------------------------- */
/* one torch.optim.Adam step (amsgrad off) over a flat arena of n floats (16-B aligned p, g, m, v); `step` counts from 1;
 * the gradient is read as g*gscale; zero_grad != 0 clears g afterwards.  The OneCycleLR value is passed in as lr. */
int gpe_adam_step(float* p, float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, long step, float gscale, int zero_grad, void* stream);
/* the same step with the two step-dependent scalars read from DEVICE memory — hyper[0] = lr / (1 - beta1^step),
 * hyper[1] = 1 / sqrt(1 - beta2^step), as gpe_adam_hyper writes them into a HOST pair — for a step that is replayed from a
 * captured hipGraph, whose kernel arguments are frozen (gpe_amd/graph.py; nn/trainer.py:162-185 runs Adam under OneCycleLR) */
int gpe_adam_step_dev(float* p, float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                      float weight_decay, float gscale, int zero_grad, void* stream);
int gpe_adam_hyper(float lr, float beta1, float beta2, long step, float* out_host);
/* out = (x - shift) / scale per column; shift_host / scale_host are HOST arrays of C <= 8 floats */
int gpe_standardize(const float* x, long rows, int C, const float* shift_host, const float* scale_host, float* out,
                    void* stream);

/* split-K product y[z][M][N] = A[:, z*256:(z+1)*256] . W[:, z*256:...]^T for z < ceil(K/256): one K slab per workgroup
 * (latency-bound long-K shapes: the LSTM backward recurrence).  The partials are summed by the consumer. */
int gpe_linear_splitk(const float* a, long a_so, const float* wp, float* y, int M, int N, int K, void* stream);

/* ---- small helpers --------------------------------------------------------------------------------------- */
/* y[r][c] (+)= sum over inner index t of x[r][t][c]   (x rows: r*x_so + t*x_si) */
int gpe_reduce_inner(const float* x, long x_so, long x_si, int T, int R, int C, float* y, int ldy,
                     int accumulate, void* stream);
/* dW1 [H][2C] from dWpq [2H][C]:  dW1[:, :C] = dWp ; dW1[:, C:] = dWq - dWp */
int gpe_w1_grad_from_pq(const float* dwpq, int ld, int H, int C, float* dw1, int lddw1, void* stream);
/* Wpq [2H][C] from W1 [H][2C]: rows 0..H-1 = W1a - W1b, rows H..2H-1 = W1b; bias_pq = [b1 | 0] */
int gpe_w1_split(const float* w1, int ldw1, const float* b1, int H, int C, float* wpq, int ldwpq, float* bias_pq,
                 void* stream);
/* out = alpha * x (n floats; out may alias x) */
int gpe_scale(const float* x, float alpha, float* out, long n, void* stream);
/* out = alpha[0] * x, alpha a DEVICE scalar (the upstream gradient of a scalar loss term; no host read-back) */
int gpe_scale_dev(const float* x, const float* alpha, float* out, long n, void* stream);
/* out = a + b (n floats) */
int gpe_add(const float* a, const float* b, float* out, long n, void* stream);
/* inter-layer dropout of nn.LSTM / nn.GRU (nn/net_blocks.py:346,374,418-420,469): out [Bn,T,H] dense = x (strided [Bn,T,H] view:
 * element (b,t,h) at x + b*x_sb + t*x_st + h) * mask [Bn,T,H] dense (Bernoulli(1-p)/(1-p), drawn by the caller). */
int gpe_mul_rows(const float* x, long x_sb, long x_st, const float* mask, long Bn, int T, int H, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPE_HIP_H */
