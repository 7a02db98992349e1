// Stitch recovery from the edge-pair classifier (StitchOnEdge3DPairs at prediction time: nn/data/pattern_converter.py:411-499
// all_edge_pairs + stitches_from_pair_classifier), forward only.
//
//   pairs      every (panel i, edge r) x (panel j, edge c), i < j, both edges present; order key (i, j, r, c)
//   logit      eval-mode MLP([2 Fe, H x n, 1]) on the standardised row [e_i | e_j]; a pair is positive iff sigmoid(logit) > 0.5 in fp32
//   selection  a positive survives iff on BOTH of its edges it is the maximum of (score, earlier order key) over the positives
//              touching that edge  (= the reference's mark-the-weaker loop against the full initial list, lines 440-456)
//
// gpe_stitch_pairs_fwd  (fused, store-free): the first Linear splits into per-edge projections, W1 [e_i | e_j] = A_i + Bv_j (table
//   [A | Bv] from gpe_linear).  A workgroup owns 8 x 8 edges of one garment = 64 pair rows: relu(A_i + Bv_j) is formed in LDS, the
//   H x H layers run on v_mfma_f32_16x16x4_f32 (a wave = 16 rows x all columns, accumulators in registers, activations rewritten in
//   place in LDS, weights streamed through LDS in 32-row K slabs of the transposed, BatchNorm-folded pack), the H -> 1 layer +
//   ReLU + affine is a dot product in the epilogue.  Nothing is stored per pair: a positive pair issues two 64-bit vector atomicMax
//   on the per-edge table {logit bits : ~order key}, which makes the result independent of arrival order.
//   In the f16x3 arithmetic mode the same layers run on the fp16 pipe (gpe_stitch_pairs_h3_kernel below).
// gpe_stitch_pairs_rows / _reduce  (generic route): pair rows of a chunk of i-edges are materialised, classified by the dense-MLP
//   kernels (any width / depth) and fed to the same epilogue.
// gpe_stitch_select: one workgroup per garment; an edge's best pair survives iff its partner's table entry is the same word;
//   survivors are ranked by order key.
#include "gpe_device.h"
#include <math.h>

#define SP_MAXP 32
#define SP_MAXL 16
#define SP_MAXF 16          // features per edge (element_size / 2)
#define SP_T 8              // edges per tile side
#define SP_KS 32            // K rows of a weight slab
#define SP_TPB 256

// ---- layout of the fused kernel's operands (documented in include/gpe_hip.h) ----------------------------------------------------
static inline int sp_nb(int H) { const int nb = (H + 15) / 16; return nb <= 4 ? 4 : (nb <= 8 ? 8 : (nb <= 13 ? 13 : 16)); }
static inline int sp_ldw(int H) { const int np = sp_nb(H) * 16; return (np % 32 == 16) ? np : np + 16; }   // 4 K rows x 16 columns hit 64 banks
static inline int sp_lda(int H) { return ((H / 4) | 1) * 4; }                                               // 16 rows x 4 k hit 64 banks

// ---- the shared epilogue ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sp_positive(float x) { return gpe_sigmoid(x) > 0.5f; }

// ---- evaluation against ground-truth stitches (the EVAL instantiations; metrics/composed_loss.py:83-126 over all pairs) -------------
// what a thread gathers over its pairs: the BCE-with-logits terms (fp32 each, summed in fp64) and the packed counters
//   a = pairs | correct << 16        b = true positives | predicted positives << 10 | ground-truth positives << 20
// (a workgroup sees at most 512 pairs, so no field overflows before the workgroup's totals are unpacked)
struct SpEvalAcc { double loss; int a, b; };

// mask: this garment's label bits [E][ceil(E / 32)]
__device__ __forceinline__ void sp_eval_pair(float x, int ei, int ej, int E, const unsigned* mask, SpEvalAcc& ev)
{
    const bool y = (mask[(long)ei * ((E + 31) >> 5) + (ej >> 5)] >> (ej & 31)) & 1u;
    const bool pos = sp_positive(x);
    // relu(-+x) + log1p(exp(-|x|)): both summands are non-negative
    ev.loss += (double)(fmaxf(y ? -x : x, 0.f) + log1pf(expf(-fabsf(x))));
    ev.a += 1 + (pos == y ? 1 << 16 : 0);
    ev.b += (pos && y ? 1 : 0) + (pos ? 1 << 10 : 0) + (y ? 1 << 20 : 0);
}

// every thread of the workgroup calls this once.  Fixed order: xor butterfly inside a wave, then the waves in order through LDS.
// The fp64 partial goes to the workgroup's own slot; the integer counters are added to the garment's two words
//   cnt[0] = pairs | correct << 32       cnt[1] = true positives | predicted positives << 21 | ground-truth positives << 42
// by integer atomics (order-independent; a garment has fewer than 2^17 pairs).
__device__ __forceinline__ void sp_eval_commit(SpEvalAcc ev, double* slot, unsigned long long* cnt)
{
    __shared__ double s_loss[SP_TPB / 64];
    __shared__ int s_a[SP_TPB / 64], s_b[SP_TPB / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ev.loss += __shfl_xor(ev.loss, o);
        ev.a += __shfl_xor(ev.a, o);
        ev.b += __shfl_xor(ev.b, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_loss[w] = ev.loss; s_a[w] = ev.a; s_b[w] = ev.b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double l = s_loss[0];
        int a = s_a[0], b = s_b[0];
        for (int i = 1; i < SP_TPB / 64; ++i) { l += s_loss[i]; a += s_a[i]; b += s_b[i]; }
        *slot = l;
        if (a) atomicAdd(cnt, (unsigned long long)(a & 0xffff) | ((unsigned long long)(a >> 16) << 32));
        if (b) atomicAdd(cnt + 1, (unsigned long long)(b & 1023) | ((unsigned long long)((b >> 10) & 1023) << 21) |
                                      ((unsigned long long)(b >> 20) << 42));
    }
}

// tab / dense: this garment's table [E] and dense logits [E][E] (or NULL); EVAL: mask = this garment's label bits, ev = the thread's sums
template <bool EVAL>
__device__ __forceinline__ void sp_epilogue(float logit, int pi, int r, int pj, int c, int L, int E, unsigned long long* tab,
                                            float* dense, const unsigned* mask, SpEvalAcc& ev)
{
    const int ei = pi * L + r, ej = pj * L + c;
    if (dense) dense[(long)ei * E + ej] = logit;
    if (sp_positive(logit)) {            // implies logit > 0: the bit pattern orders like the value
        const unsigned key = ((unsigned)pi << 13) | ((unsigned)pj << 8) | ((unsigned)r << 4) | (unsigned)c;
        const unsigned long long v = ((unsigned long long)__float_as_uint(logit) << 32) | (unsigned long long)(~key);
        atomicMax(tab + ei, v);
        atomicMax(tab + ej, v);
    }
    if constexpr (EVAL) sp_eval_pair(logit, ei, ej, E, mask, ev);
}

__device__ __forceinline__ int sp_count(const int32_t* ne, int L)
{
    const int n = *ne;
    return n < 0 ? 0 : (n > L ? L : n);
}

// ---- weight pack: out[k][n] = w[n][k] * col_scale[k], zero for N <= n < ldo ----------------------------------------------------------
__global__ void gpe_stitch_pairs_pack_kernel(const float* w, int ldw, int N, int K, const float* cs, float* out, int ldo)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)K * ldo) return;
    const int k = (int)(idx / ldo), n = (int)(idx - (long)k * ldo);
    out[idx] = n < N ? w[(long)n * ldw + k] * (cs ? cs[k] : 1.f) : 0.f;
}

// ---- fused kernels ---------------------------------------------------------------------------------------------------------------
struct SpFwdParams {
    static constexpr bool EVAL = false;
    const float* ab; int ldab; int H; int nl;
    const float* wpk; const float* planes; const unsigned* w_amax; const float* last;
    const int32_t* ne; int B, P, L;
    unsigned long long* table; float* dense;
    int lda, nTj, KP;
};
// the evaluating instantiations carry the label mask [B][E][ceil(E / 32)], the loss slab [B][ceil(E / 8)^2] (tile (ti, tj) of
// either kernel owns slot ti * ceil(E / 8) + tj) and the counter words [B][2]
struct SpEvalParams : SpFwdParams {
    static constexpr bool EVAL = true;
    const unsigned* mask; double* slab; unsigned long long* cnt;
};
__device__ __forceinline__ const unsigned* sp_mask_of(const SpFwdParams&, int, int) { return nullptr; }
__device__ __forceinline__ const unsigned* sp_mask_of(const SpEvalParams& p, int b, int E) { return p.mask + (long)b * E * ((E + 31) >> 5); }
__device__ __forceinline__ void sp_tile_commit(const SpFwdParams&, const SpEvalAcc&, int, int, int, int) {}
__device__ __forceinline__ void sp_tile_commit(const SpEvalParams& p, const SpEvalAcc& ev, int b, int E, int ti, int tj)
{
    const int n8 = (E + 7) >> 3;
    sp_eval_commit(ev, p.slab + ((long)b * n8 + ti) * n8 + tj, p.cnt + 2 * (long)b);
}

template <int NB> struct SpLdw { static constexpr int v = (NB * 16) % 32 == 16 ? NB * 16 : NB * 16 + 16; };

// present edges of garment b in (panel, edge) order: the tile's TI i-positions and TJ j-positions -> (panel, edge), -1 past the end.
// false (block-uniform): the tile holds no pair.
template <int TI, int TJ>
__device__ __forceinline__ bool sp_tile_setup(const SpFwdParams& p, int b, int ti, int tj, int* s_off, int* s_pan, int* s_edg)
{
    const int tid = threadIdx.x, P = p.P, L = p.L;
    if (tj * TJ + TJ - 1 <= ti * TI) return false;
    if (tid == 0) {
        int o = 0;
        for (int q = 0; q < P; ++q) { s_off[q] = o; o += sp_count(p.ne + (long)b * P + q, L); }
        s_off[P] = o;
    }
    __syncthreads();
    const int nv = s_off[P];
    if (ti * TI >= nv || tj * TJ >= nv) return false;
    if (tid < TI + TJ) {
        const int pos = tid < TI ? ti * TI + tid : tj * TJ + tid - TI;
        int pan = -1, e = 0;
        if (pos < nv)
            for (int q = 0; q < P; ++q)
                if (pos >= s_off[q] && pos < s_off[q + 1]) { pan = q; e = pos - s_off[q]; }
        s_pan[tid] = pan;
        s_edg[tid] = e;
    }
    __syncthreads();
    // panels do not decrease with the position: a pair exists iff the first i panel lies below the last j panel
    int pmax = -1;
    for (int jj = 0; jj < TJ; ++jj) pmax = max(pmax, s_pan[TI + jj]);
    return s_pan[0] >= 0 && s_pan[0] < pmax;
}

// a 32-row K slab of a layer's weights travels global -> registers (in flight during the previous slab's products) -> LDS
// (named registers, not an array: the compiler kept an indexed array of them in private memory)
#define SP_PRE_DECL float4 pre0 = {}, pre1 = {}, pre2 = {}, pre3 = {}, pre4 = {}, pre5 = {}, pre6 = {}, pre7 = {}, pre8 = {}
#define SP_LD1(i, src, n4) if (NPRE > i) pre##i = reinterpret_cast<const float4*>(src)[min((int)threadIdx.x + i * SP_TPB, (n4) - 1)];
#define SP_ST1(i, dst, n4) if (NPRE > i && (int)threadIdx.x + i * SP_TPB < (n4)) reinterpret_cast<float4*>(dst)[threadIdx.x + i * SP_TPB] = pre##i;
#define SP_SLAB_LOAD(src, n4)  do { SP_LD1(0, src, n4) SP_LD1(1, src, n4) SP_LD1(2, src, n4) SP_LD1(3, src, n4) SP_LD1(4, src, n4) \
                                    SP_LD1(5, src, n4) SP_LD1(6, src, n4) SP_LD1(7, src, n4) SP_LD1(8, src, n4) } while (0)
#define SP_SLAB_STORE(dst, n4) do { SP_ST1(0, dst, n4) SP_ST1(1, dst, n4) SP_ST1(2, dst, n4) SP_ST1(3, dst, n4) SP_ST1(4, dst, n4) \
                                    SP_ST1(5, dst, n4) SP_ST1(6, dst, n4) SP_ST1(7, dst, n4) SP_ST1(8, dst, n4) } while (0)

// exact fp32: 8 x 8 edges = 64 pair rows, a wave = 16 rows x all columns
template <int NB, class PT>
__global__ __launch_bounds__(SP_TPB) void gpe_stitch_pairs_fwd_kernel(PT p)
{
    constexpr bool EVAL = PT::EVAL;
    constexpr int LDW = SpLdw<NB>::v, NPRE = (SP_KS * LDW / 4 + SP_TPB - 1) / SP_TPB;
    static_assert(NPRE <= 9, "a slab is at most 9 float4 per thread");
    extern __shared__ float sp_smem[];
    __shared__ int s_off[SP_MAXP + 1];
    __shared__ int s_pan[2 * SP_T], s_edg[2 * SP_T];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int ti = blockIdx.x / p.nTj, tj = blockIdx.x - ti * p.nTj;
    if (!sp_tile_setup<SP_T, SP_T>(p, b, ti, tj, s_off, s_pan, s_edg)) return;
    const int L = p.L, H = p.H, E = p.P * L;
    float* act = sp_smem;                       // [64][lda]
    float* Ws = sp_smem + 64 * p.lda;           // [SP_KS][LDW]
    const int lda = p.lda;
    const float* abg = p.ab + (long)b * E * p.ldab;
    const int H4 = H >> 2;
    for (int idx = tid; idx < 64 * H4; idx += SP_TPB) {
        const int row = idx / H4, q = idx - row * H4;
        const int ii = row >> 3, jj = SP_T + (row & 7);
        const int pi = s_pan[ii], pj = s_pan[jj];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pi >= 0 && pj > pi) {
            const float4 a = *reinterpret_cast<const float4*>(abg + (long)(pi * L + s_edg[ii]) * p.ldab + 4 * q);
            const float4 c = *reinterpret_cast<const float4*>(abg + (long)(pj * L + s_edg[jj]) * p.ldab + H + 4 * q);
            v = make_float4(fmaxf(a.x + c.x, 0.f), fmaxf(a.y + c.y, 0.f), fmaxf(a.z + c.z, 0.f), fmaxf(a.w + c.w, 0.f));
        }
        *reinterpret_cast<float4*>(act + row * lda + 4 * q) = v;
    }
    const int lane = tid & 63, row0 = (tid >> 6) * 16, lr = lane & 15, lq = lane >> 4;
    const float* wl = p.wpk;
    for (int l = 0; l + 1 < p.nl; ++l) {
        const float* Wt = wl;
        const float* bias = wl + (long)H * LDW;
        wl += (long)(H + 1) * LDW;
        f32x4 acc[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const float bz = bias[nb * 16 + lr];
            acc[nb] = f32x4{bz, bz, bz, bz};
        }
        SP_PRE_DECL;
        SP_SLAB_LOAD(Wt, min(SP_KS, H) * LDW / 4);
        for (int k0 = 0; k0 < H; k0 += SP_KS) {
            const int kc = min(SP_KS, H - k0);
            __syncthreads();                    // the activations are written / the previous slab has been read
            SP_SLAB_STORE(Ws, kc * LDW / 4);
            __syncthreads();
            if (k0 + SP_KS < H) SP_SLAB_LOAD(Wt + (long)(k0 + SP_KS) * LDW, min(SP_KS, H - k0 - SP_KS) * LDW / 4);
            for (int ks = 0; ks < kc; ks += 4) {
                const float a = act[(row0 + lr) * lda + k0 + ks + lq];
                const float* wr = Ws + (ks + lq) * LDW + lr;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
                    acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wr[nb * 16], acc[nb], 0, 0, 0);
            }
        }
        // a wave rewrites only its own 16 rows, and it has consumed them
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int col = nb * 16 + lr;
            if (col < H) {
#pragma unroll
                for (int r = 0; r < 4; ++r) act[(row0 + lq * 4 + r) * lda + col] = fmaxf(acc[nb][r], 0.f);
            }
        }
    }
    __syncthreads();
    // H -> 1: lane (lr, lq) sums k = lq, lq + 4, ... of row row0 + lr
    float s = 0.f;
    for (int k = lq; k < H; k += 4) s = fmaf(act[(row0 + lr) * lda + k], wl[k], s);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    SpEvalAcc ev = {0.0, 0, 0};
    if (lq == 0) {
        const int row = row0 + lr;
        const int ii = row >> 3, jj = SP_T + (row & 7);
        const int pi = s_pan[ii], pj = s_pan[jj];
        if (pi >= 0 && pj > pi) {
            const float logit = p.last[2] * fmaxf(s + wl[H], 0.f) + p.last[3];
            sp_epilogue<EVAL>(logit, pi, s_edg[ii], pj, s_edg[jj], L, E, p.table + (long)b * E,
                              p.dense ? p.dense + (long)b * E * E : nullptr, sp_mask_of(p, b, E), ev);
        }
    }
    sp_tile_commit(p, ev, b, E, ti, tj);
}

// ---- f16x3: the fp16 pipe on normalised two-term splits, fp32 accumulate ------------------------------------------------------------
// x 2^sh = h + l (two fp16 terms), a product = three v_mfma_f32_16x16x32_f16 (small terms first).  Weights: one power of two per
// layer from the largest magnitude of the folded pack (amax word), planes prepared by gpe_stitch_pairs_planes in B-fragment order.
// Activations: one power of two per WAVE (its 32 rows) and layer, from the maximum the wave finds in its own accumulators, so the
// normalisation needs no pass over memory; the planes of the activations live in LDS and are rewritten in place.
// 8 x 16 edges = 128 pair rows per workgroup, a wave = 32 rows x all columns (every B fragment feeds two row blocks).
#define SP3_TI 8
#define SP3_TJ 16
__device__ __forceinline__ float sp_wave_max(float m)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    return m;
}

__global__ void gpe_stitch_pairs_planes_kernel(const float* wt, int K, int ldw, const unsigned* amax, _Float16* out)
{
    const int KP = (K + 31) & ~31;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)KP * ldw) return;
    const int k = (int)(idx / ldw), n = (int)(idx - (long)k * ldw);
    float s, inv;
    gpe_h3_scale_of(*amax, s, inv);
    const float v = k < K ? wt[idx] * s : 0.f;
    const _Float16 h = (_Float16)v;
    const _Float16 l = (_Float16)(v - (float)h);
    const long o = (long)(k >> 5) * (64 * ldw) + ((long)((k >> 3) & 3) * ldw + n) * 8 + (k & 7);
    out[o] = h;
    out[o + 32 * ldw] = l;
}

template <int NB, class PT>
__global__ __launch_bounds__(SP_TPB) void gpe_stitch_pairs_h3_kernel(PT p)
{
    constexpr bool EVAL = PT::EVAL;
    constexpr int LDW = SpLdw<NB>::v, NPRE = (SP_KS * LDW / 4 + SP_TPB - 1) / SP_TPB, N4 = SP_KS * LDW / 4;
    static_assert(NPRE <= 9, "a slab is at most 9 float4 per thread");
    extern __shared__ float sp_smem[];
    __shared__ int s_off[SP_MAXP + 1];
    __shared__ int s_pan[SP3_TI + SP3_TJ], s_edg[SP3_TI + SP3_TJ];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int ti = blockIdx.x / p.nTj, tj = blockIdx.x - ti * p.nTj;
    if (!sp_tile_setup<SP3_TI, SP3_TJ>(p, b, ti, tj, s_off, s_pan, s_edg)) return;
    const int L = p.L, H = p.H, E = p.P * L, KP = p.KP, ldh = KP + 8;
    _Float16* hiP = reinterpret_cast<_Float16*>(sp_smem);          // [128][ldh]
    _Float16* loP = hiP + 128 * ldh;
    float* Ws = sp_smem + 128 * ldh;                                // hi [4][LDW][8 halves], lo alike
    const float* abg = p.ab + (long)b * E * p.ldab;
    const int H4 = H >> 2;
    const int lane = tid & 63, row0 = (tid >> 6) * 32, lr = lane & 15, lq = lane >> 4;
    // a0 = relu(A_i + Bv_j) of this wave's 32 rows: a pass for the maximum, a pass that stores the split
    float sa, inv_a;
    for (int pass = 0; pass < 2; ++pass) {
        float m = 0.f;
        for (int idx = lane; idx < 32 * H4; idx += 64) {
            const int r = idx / H4, q = idx - r * H4, row = row0 + r;
            const int ii = row >> 4, jj = SP3_TI + (row & 15);
            const int pi = s_pan[ii], pj = s_pan[jj];
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pi >= 0 && pj > pi) {
                const float4 a = *reinterpret_cast<const float4*>(abg + (long)(pi * L + s_edg[ii]) * p.ldab + 4 * q);
                const float4 c = *reinterpret_cast<const float4*>(abg + (long)(pj * L + s_edg[jj]) * p.ldab + H + 4 * q);
                v = make_float4(fmaxf(a.x + c.x, 0.f), fmaxf(a.y + c.y, 0.f), fmaxf(a.z + c.z, 0.f), fmaxf(a.w + c.w, 0.f));
            }
            if (pass == 0) {
                m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
            } else {
                uint2 h, l;
                gpe_split2_f16(v.x, v.y, sa, h.x, l.x);
                gpe_split2_f16(v.z, v.w, sa, h.y, l.y);
                *reinterpret_cast<uint2*>(hiP + row * ldh + 4 * q) = h;
                *reinterpret_cast<uint2*>(loP + row * ldh + 4 * q) = l;
            }
        }
        if (pass == 0) gpe_h3_scale_of(__float_as_uint(sp_wave_max(m)), sa, inv_a);
    }
    {   // K padding of the planes
        const int pad4 = (KP - H) >> 2;
        for (int idx = lane; idx < 32 * pad4; idx += 64) {
            const int r = idx / pad4, q = idx - r * pad4;
            *reinterpret_cast<uint2*>(hiP + (row0 + r) * ldh + H + 4 * q) = make_uint2(0u, 0u);
            *reinterpret_cast<uint2*>(loP + (row0 + r) * ldh + H + 4 * q) = make_uint2(0u, 0u);
        }
    }
    const float* wl = p.wpk;
    for (int l = 0; l + 1 < p.nl; ++l) {
        const float* bias = wl + (long)H * LDW;
        wl += (long)(H + 1) * LDW;
        const float* pl = p.planes + (long)l * KP * LDW;
        float sw, inv_w;
        gpe_h3_scale_of(p.w_amax[l], sw, inv_w);
        f32x4 acc[2][NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) { acc[0][nb] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[1][nb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        SP_PRE_DECL;
        SP_SLAB_LOAD(pl, N4);
        for (int k0 = 0; k0 < KP; k0 += 32) {
            __syncthreads();                    // the previous slab has been read by every wave
            SP_SLAB_STORE(Ws, N4);
            __syncthreads();
            if (k0 + 32 < KP) SP_SLAB_LOAD(pl + (long)(k0 + 32) * LDW, N4);
            gpe_u32x4 ah[2], al[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                ah[m] = *reinterpret_cast<const gpe_u32x4*>(hiP + (row0 + 16 * m + lr) * ldh + k0 + 8 * lq);
                al[m] = *reinterpret_cast<const gpe_u32x4*>(loP + (row0 + 16 * m + lr) * ldh + k0 + 8 * lq);
            }
            const float* wb = Ws + (lq * LDW + lr) * 4;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const gpe_u32x4 bh = *reinterpret_cast<const gpe_u32x4*>(wb + 64 * nb);
                const gpe_u32x4 bl = *reinterpret_cast<const gpe_u32x4*>(wb + 64 * nb + 16 * LDW);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    acc[m][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(gpe_f16x8, al[m]), __builtin_bit_cast(gpe_f16x8, bh), acc[m][nb], 0, 0, 0);
                    acc[m][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(gpe_f16x8, ah[m]), __builtin_bit_cast(gpe_f16x8, bl), acc[m][nb], 0, 0, 0);
                    acc[m][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(gpe_f16x8, ah[m]), __builtin_bit_cast(gpe_f16x8, bh), acc[m][nb], 0, 0, 0);
                }
            }
        }
        // a = relu(acc / (scales) + bias); its maximum gives the wave's next scale; the wave rewrites its own rows of the planes
        const float un = inv_a * inv_w;
        float m = 0.f;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int col = nb * 16 + lr;
            const float bz = bias[col];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = col < H ? fmaxf(fmaf(acc[mb][nb][r], un, bz), 0.f) : 0.f;
                    acc[mb][nb][r] = v;
                    m = fmaxf(m, v);
                }
        }
        gpe_h3_scale_of(__float_as_uint(sp_wave_max(m)), sa, inv_a);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int col = nb * 16 + lr;
            if (col < H) {
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = acc[mb][nb][r] * sa;
                        const _Float16 h = (_Float16)v;
                        const int o = (row0 + 16 * mb + lq * 4 + r) * ldh + col;
                        hiP[o] = h;
                        loP[o] = (_Float16)(v - (float)h);
                    }
            }
        }
    }
    __syncthreads();
    // H -> 1 on the planes of the last activation: lane (lr, lq) sums the 8-k groups lq, lq + 4, ... of rows row0 + lr, + 16
    const float* wf = wl;
    SpEvalAcc ev = {0.0, 0, 0};
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        const int row = row0 + 16 * mb + lr;
        float s = 0.f;
        for (int g = lq; g * 8 < H; g += 4) {
            const gpe_f16x8 h8 = *reinterpret_cast<const gpe_f16x8*>(hiP + row * ldh + 8 * g);
            const gpe_f16x8 l8 = *reinterpret_cast<const gpe_f16x8*>(loP + row * ldh + 8 * g);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (8 * g + j < H) s = fmaf((float)h8[j] + (float)l8[j], wf[8 * g + j], s);
        }
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        if (lq == 0) {
            const int ii = row >> 4, jj = SP3_TI + (row & 15);
            const int pi = s_pan[ii], pj = s_pan[jj];
            if (pi >= 0 && pj > pi) {
                const float logit = p.last[2] * fmaxf(fmaf(s, inv_a, wf[H]), 0.f) + p.last[3];
                sp_epilogue<EVAL>(logit, pi, s_edg[ii], pj, s_edg[jj], L, E, p.table + (long)b * E,
                                  p.dense ? p.dense + (long)b * E * E : nullptr, sp_mask_of(p, b, E), ev);
            }
        }
    }
    sp_tile_commit(p, ev, b, E, ti, tj);
}

// ---- generic route: rows of the i-edges [c0, c1) (pattern-level ids) -----------------------------------------------------------------
// i-edge e = (panel q, edge r) pairs with the E - (q + 1) L edge slots of the later panels; its rows start at sp_row_off(e)
__device__ __host__ __forceinline__ long sp_row_off(int e, int L, int E)
{
    const long q = e / L, r = e - q * L;
    return (long)L * (q * E) - (long)L * L * (q * (q + 1) / 2) + r * (E - (q + 1) * L);
}

struct SpStd { float shift[2 * SP_MAXF]; float scale[2 * SP_MAXF]; };

// grid (ceil(E / 256), B * (c1 - c0))
__global__ void gpe_stitch_pairs_rows_kernel(const float* edges, const int32_t* ne, int P, int L, int Fe, SpStd st, int c0, int c1,
                                             long rows_chunk, float* rows)
{
    const int E = P * L;
    const int b = blockIdx.y / (c1 - c0), ei = c0 + blockIdx.y - b * (c1 - c0);
    const int ej = blockIdx.x * blockDim.x + threadIdx.x;
    const int pi = ei / L, r = ei - pi * L;
    if (ej < (pi + 1) * L || ej >= E) return;
    const int pj = ej / L, c = ej - pj * L;
    const long row = sp_row_off(ei, L, E) - sp_row_off(c0, L, E) + (ej - (pi + 1) * L);
    const bool valid = r < sp_count(ne + (long)b * P + pi, L) && c < sp_count(ne + (long)b * P + pj, L);
    float* dst = rows + ((long)b * rows_chunk + row) * (2 * Fe);
    const float* xi = edges + ((long)b * E + ei) * Fe;
    const float* xj = edges + ((long)b * E + ej) * Fe;
    for (int f = 0; f < Fe; ++f) {
        dst[f] = valid ? (xi[f] - st.shift[f]) / st.scale[f] : 0.f;
        dst[Fe + f] = valid ? (xj[f] - st.shift[Fe + f]) / st.scale[Fe + f] : 0.f;
    }
}

// EVAL: one workgroup per (garment, i-edge) walks the PRESENT edges of the later panels in position order, so that the grouping of
// the fp64 sums does not depend on how many unused slots the caller's layout has; grid (1, B * (c1 - c0)), slot = the i-edge's id
template <bool EVAL>
__global__ void gpe_stitch_pairs_reduce_kernel(const float* y, long ldy, const int32_t* ne, int P, int L, int c0, int c1,
                                               long rows_chunk, unsigned long long* table, float* dense, const unsigned* mask,
                                               double* slab, unsigned long long* cnt)
{
    const int E = P * L;
    const int b = blockIdx.y / (c1 - c0), ei = c0 + blockIdx.y - b * (c1 - c0);
    const int pi = ei / L, r = ei - pi * L;
    SpEvalAcc ev = {0.0, 0, 0};
    if constexpr (EVAL) {
        __shared__ int s_off[SP_MAXP + 1];
        if (r >= sp_count(ne + (long)b * P + pi, L)) return;            // block-uniform
        if (threadIdx.x == 0) {
            int o = 0;
            for (int q = 0; q < P; ++q) { s_off[q] = o; o += sp_count(ne + (long)b * P + q, L); }
            s_off[P] = o;
        }
        __syncthreads();
        const long row0 = sp_row_off(ei, L, E) - sp_row_off(c0, L, E) - (long)(pi + 1) * L;
        for (int pos = s_off[pi + 1] + threadIdx.x; pos < s_off[P]; pos += blockDim.x) {
            int pj = pi + 1;
            while (pos >= s_off[pj + 1]) ++pj;
            const int c = pos - s_off[pj];
            sp_epilogue<true>(y[((long)b * rows_chunk + row0 + pj * L + c) * ldy], pi, r, pj, c, L, E, table + (long)b * E,
                              dense ? dense + (long)b * E * E : nullptr, mask + (long)b * E * ((E + 31) >> 5), ev);
        }
        sp_eval_commit(ev, slab + (long)b * E + ei, cnt + 2 * (long)b);
    } else {
        const int ej = blockIdx.x * blockDim.x + threadIdx.x;
        if (ej < (pi + 1) * L || ej >= E) return;
        const int pj = ej / L, c = ej - pj * L;
        if (r >= sp_count(ne + (long)b * P + pi, L) || c >= sp_count(ne + (long)b * P + pj, L)) return;
        const long row = sp_row_off(ei, L, E) - sp_row_off(c0, L, E) + (ej - (pi + 1) * L);
        sp_epilogue<false>(y[((long)b * rows_chunk + row) * ldy], pi, r, pj, c, L, E, table + (long)b * E,
                           dense ? dense + (long)b * E * E : nullptr, nullptr, ev);
    }
}

// ---- selection -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_TPB) void gpe_stitch_select_kernel(const unsigned long long* table, int P, int L, int S,
                                                                   int32_t* stitches, int32_t* nums, float* scores)
{
    __shared__ unsigned s_key[SP_MAXP * SP_MAXL];
    __shared__ int s_cnt;
    const int b = blockIdx.x, tid = threadIdx.x, E = P * L;
    const unsigned long long* tab = table + (long)b * E;
    if (tid == 0) s_cnt = 0;
    for (int e = tid; e < E; e += SP_TPB) {
        const unsigned long long v = tab[e];
        unsigned key = 0xffffffffu;
        if (v) {
            const unsigned ok = ~(unsigned)(v & 0xffffffffull);
            const int i = (ok >> 13) & 31, j = (ok >> 8) & 31, r = (ok >> 4) & 15, c = ok & 15;
            // the pair is recorded at its lower side; it survives iff both of its edges name it their best
            if ((ok >> 18) == 0 && i < P && j < P && r < L && c < L && i * L + r == e && tab[j * L + c] == v) key = ok;
        }
        s_key[e] = key;
    }
    __syncthreads();
    for (int e = tid; e < E; e += SP_TPB) {
        const unsigned key = s_key[e];
        if (key == 0xffffffffu) continue;
        int rank = 0;
        for (int o = 0; o < E; ++o) rank += s_key[o] < key ? 1 : 0;
        atomicAdd(&s_cnt, 1);
        if (rank < S) {
            const int j = (key >> 8) & 31, c = key & 15;
            stitches[((long)b * 2 + 0) * S + rank] = e;
            stitches[((long)b * 2 + 1) * S + rank] = j * L + c;
            scores[(long)b * S + rank] = __uint_as_float((unsigned)(tab[e] >> 32));
        }
    }
    __syncthreads();
    const int cnt = min(s_cnt, S);
    for (int s = cnt + tid; s < S; s += SP_TPB) {
        stitches[((long)b * 2 + 0) * S + s] = 0;
        stitches[((long)b * 2 + 1) * S + s] = 0;
        scores[(long)b * S + s] = 0.f;
    }
    if (tid == 0) nums[b] = cnt;
}

// ---- ground-truth labels and the finalisation of an evaluating pass -------------------------------------------------------------------
// mask[b][a][c / 32] bit c % 32 and its transpose for every stitch (a, c) of garment b; ids outside 0 .. E - 1 are ignored.
// grid (ceil(S / 256), B); integer atomicOr: duplicates and arrival order do not matter
__global__ void gpe_stitch_pairs_labels_kernel(const int32_t* st, const int32_t* nums, int S, int E, unsigned* mask)
{
    const int b = blockIdx.y, s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= min(nums[b], S)) return;
    const int a = st[((long)b * 2 + 0) * S + s], c = st[((long)b * 2 + 1) * S + s];
    if (a < 0 || a >= E || c < 0 || c >= E) return;
    const int W = (E + 31) >> 5;
    unsigned* m = mask + (long)b * E * W;
    atomicOr(m + (long)a * W + (c >> 5), 1u << (c & 31));
    atomicOr(m + (long)c * W + (a >> 5), 1u << (a & 31));
}

__device__ __forceinline__ float sp_ratio(long long num, long long den) { return den ? (float)num / (float)den : 0.f; }

// ONE workgroup of 16 waves: wave w takes the garments w, w + 16, ...  A garment's slab is `slots` doubles in groups of `group`
// consecutive slots (<= 64 groups): lane g adds group g in slot order, then the groups are added in order, so zero slots (tiles
// without a pair, unused edge slots) change nothing; the call's total adds loss_sum[0 .. B) in order.
#define SP_FIN_TPB 1024
__global__ __launch_bounds__(SP_FIN_TPB) void gpe_stitch_eval_finalize_kernel(const double* slab, long slots, int group,
                                                                              const unsigned long long* cnt, const unsigned* mask,
                                                                              const int32_t* stitches, const int32_t* nums, int B,
                                                                              int P, int L, double* loss_sum, int32_t* counts,
                                                                              float* metrics)
{
    __shared__ long long s_tot[SP_FIN_TPB / 64][7];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, E = P * L, S = E / 2, W = (E + 31) >> 5;
    const int ngroups = (int)(slots / group);
    long long tot[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int b = w; b < B; b += SP_FIN_TPB / 64) {
        double g = 0.0;
        if (lane < ngroups) {
            const double* src = slab + (long)b * slots + (long)lane * group;
#pragma unroll 8
            for (int i = 0; i < group; ++i) g += src[i];
        }
        double sum = 0.0;
#pragma unroll 1
        for (int q = 0; q < ngroups; ++q) sum += __shfl(g, q);
        const int n = max(0, min(nums[b], S));
        int tp = 0;
        for (int s = lane; s < n; s += 64) {
            const int a = stitches[((long)b * 2 + 0) * S + s], c = stitches[((long)b * 2 + 1) * S + s];
            if (a >= 0 && a < E && c >= 0 && c < E) tp += (mask[((long)b * E + a) * W + (c >> 5)] >> (c & 31)) & 1u;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tp += __shfl_xor(tp, o);
        if (lane == 0) {
            const unsigned long long c0 = cnt[2 * (long)b], c1 = cnt[2 * (long)b + 1];
            const int v[6] = {(int)(c0 & 0xffffffffull), (int)(c0 >> 32), (int)(c1 & 0x1fffff), (int)((c1 >> 21) & 0x1fffff),
                              (int)(c1 >> 42), tp};
            loss_sum[b] = sum;
            for (int k = 0; k < 6; ++k) { counts[(long)b * 6 + k] = v[k]; tot[k] += v[k]; }
            tot[6] += n;
        }
    }
    if (lane == 0)
        for (int k = 0; k < 7; ++k) s_tot[w][k] = tot[k];
    __threadfence_block();
    __syncthreads();
    if (w == 0) {
        // the first wave reads 64 garments at a time; every lane adds them in garment order (padding adds exact zeros)
        double total = 0.0;
        for (int b0 = 0; b0 < B; b0 += 64) {
            const double v = b0 + lane < B ? loss_sum[b0 + lane] : 0.0;
#pragma unroll 1
            for (int q = 0; q < 64; ++q) total += __shfl(v, q);
        }
        if (lane == 0) {
            long long t[7];
            for (int k = 0; k < 7; ++k) {
                t[k] = 0;
                for (int i = 0; i < SP_FIN_TPB / 64; ++i) t[k] += s_tot[i][k];
            }
            metrics[0] = t[0] ? (float)(total / (double)t[0]) : 0.f;         // edge_pair_class_loss: the mean over the concatenated pairs
            metrics[1] = sp_ratio(t[1], t[0]);                               // edge_pair_class_acc
            metrics[2] = sp_ratio(t[2], t[3]);                               // stitch_precision
            metrics[3] = sp_ratio(t[2], t[4]);                               // stitch_recall
            metrics[4] = sp_ratio(t[5], t[6]);                               // selected_precision
            metrics[5] = sp_ratio(t[5], t[4]);                               // selected_recall
        }
    }
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------------
static inline bool sp_dims_ok(int B, int P, int L) { return B > 0 && B <= 65535 && P > 0 && P <= SP_MAXP && L > 0 && L <= SP_MAXL; }

extern "C" int gpe_stitch_pairs_pack(const float* w, int ldw, int N, int K, const float* col_scale, float* out, int ldo, void* stream)
{
    if (!w || !out || N <= 0 || K <= 0 || ldw < K || ldo < N) return GPE_EINVAL;
    const long total = (long)K * ldo;
    hipLaunchKernelGGL(gpe_stitch_pairs_pack_kernel, dim3(gpe_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w, ldw, N, K,
                       col_scale, out, ldo);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_stitch_pairs_planes(const float* wt, int K, int ldw, const uint32_t* amax, void* out, void* stream)
{
    if (!wt || !amax || !out || K <= 0 || ldw <= 0 || (ldw & 15) || (((uintptr_t)out) & 15)) return GPE_EINVAL;
    const long total = (long)((K + 31) & ~31) * ldw;
    hipLaunchKernelGGL(gpe_stitch_pairs_planes_kernel, dim3(gpe_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, wt, K, ldw, amax,
                       reinterpret_cast<_Float16*>(out));
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

template <int NB, class PT>
static int sp_launch_fwd(const PT& p, bool h3, hipStream_t s)
{
    constexpr int LDW = SpLdw<NB>::v;
    if (h3) {
        const size_t lds = (size_t)(128 * (p.KP + 8) + SP_KS * LDW) * sizeof(float);
        GPE_ENSURE_MAX_LDS_N((gpe_stitch_pairs_h3_kernel<NB, PT>), 158 * 1024);
        hipLaunchKernelGGL((gpe_stitch_pairs_h3_kernel<NB, PT>), dim3(gpe_cdiv(p.P * p.L, SP3_TI) * p.nTj, p.B), dim3(SP_TPB), lds, s, p);
    } else {
        const size_t lds = (size_t)(64 * p.lda + SP_KS * LDW) * sizeof(float);
        GPE_ENSURE_MAX_LDS_N((gpe_stitch_pairs_fwd_kernel<NB, PT>), 150 * 1024);
        hipLaunchKernelGGL((gpe_stitch_pairs_fwd_kernel<NB, PT>), dim3(gpe_cdiv(p.P * p.L, SP_T) * p.nTj, p.B), dim3(SP_TPB), lds, s, p);
    }
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

template <class PT>
static int sp_dispatch_fwd(const PT& p, bool h3, hipStream_t s)
{
    switch (sp_nb(p.H)) {
    case 4: return sp_launch_fwd<4>(p, h3, s);
    case 8: return sp_launch_fwd<8>(p, h3, s);
    case 13: return sp_launch_fwd<13>(p, h3, s);
    default: return sp_launch_fwd<16>(p, h3, s);
    }
}

// checks and operands shared by the prediction and the evaluating entry point; false: bad arguments
static bool sp_fwd_params(const float* ab, int ldab, int H, int n_layers, const float* wpk, const void* planes, const uint32_t* w_amax,
                          const float* last_stats, const int32_t* num_edges, int B, int P, int L, uint64_t* table, float* logits,
                          SpFwdParams& p, bool& h3)
{
    if (!ab || !wpk || !last_stats || !num_edges || !table || !sp_dims_ok(B, P, L)) return false;
    if (H <= 0 || H > 256 || (H & 3) || n_layers < 1 || n_layers > 4 || ldab < 2 * H || (ldab & 3)) return false;
    if ((((uintptr_t)ab) | ((uintptr_t)wpk) | ((uintptr_t)planes)) & 15) return false;
    const int E = P * L;
    // f16x3: planes given, the activation planes of 128 rows fit beside a slab (H <= 224), and the call is past the mode's size gate
    h3 = planes && w_amax && gpe_math_get() == 4 && H <= 224 && (long)B * E * E / 2 >= gpe_h3_min_rows();
    p = SpFwdParams{ab, ldab, H, n_layers, wpk, static_cast<const float*>(planes), w_amax, last_stats, num_edges, B, P, L,
                    reinterpret_cast<unsigned long long*>(table), logits, sp_lda(H), gpe_cdiv(E, h3 ? SP3_TJ : SP_T), (H + 31) & ~31};
    return true;
}

extern "C" int gpe_stitch_pairs_fwd(const float* ab, int ldab, int H, int n_layers, const float* wpk, const void* planes,
                                    const uint32_t* w_amax, const float* last_stats, const int32_t* num_edges, int B, int P, int L,
                                    uint64_t* table, float* logits, void* stream)
{
    SpFwdParams p;
    bool h3;
    if (!sp_fwd_params(ab, ldab, H, n_layers, wpk, planes, w_amax, last_stats, num_edges, B, P, L, table, logits, p, h3)) return GPE_EINVAL;
    return sp_dispatch_fwd(p, h3, (hipStream_t)stream);
}

extern "C" int gpe_stitch_pairs_eval_fwd(const float* ab, int ldab, int H, int n_layers, const float* wpk, const void* planes,
                                         const uint32_t* w_amax, const float* last_stats, const int32_t* num_edges, int B, int P, int L,
                                         uint64_t* table, float* logits, const uint32_t* mask, double* loss_slab, uint64_t* counters,
                                         void* stream)
{
    SpEvalParams p;
    bool h3;
    if (!mask || !loss_slab || !counters) return GPE_EINVAL;
    if (!sp_fwd_params(ab, ldab, H, n_layers, wpk, planes, w_amax, last_stats, num_edges, B, P, L, table, logits, p, h3)) return GPE_EINVAL;
    p.mask = mask;
    p.slab = loss_slab;
    p.cnt = reinterpret_cast<unsigned long long*>(counters);
    return sp_dispatch_fwd(p, h3, (hipStream_t)stream);
}

static inline bool sp_chunk_ok(int P, int L, int c0, int c1) { return c0 >= 0 && c0 < c1 && c1 <= P * L; }

extern "C" int gpe_stitch_pairs_rows(const float* edges3d, const int32_t* num_edges, int B, int P, int L, int Fe,
                                     const float* shift_host, const float* scale_host, int c0, int c1, long rows_chunk, float* rows,
                                     void* stream)
{
    if (!edges3d || !num_edges || !shift_host || !scale_host || !rows || !sp_dims_ok(B, P, L) || Fe <= 0 || Fe > SP_MAXF) return GPE_EINVAL;
    if (!sp_chunk_ok(P, L, c0, c1) || (long)B * (c1 - c0) > 65535) return GPE_EINVAL;
    const int E = P * L;
    if (rows_chunk < sp_row_off(c1, L, E) - sp_row_off(c0, L, E) || rows_chunk <= 0) return GPE_EINVAL;
    SpStd st;
    for (int f = 0; f < 2 * Fe; ++f) { st.shift[f] = shift_host[f]; st.scale[f] = scale_host[f]; }
    for (int f = 2 * Fe; f < 2 * SP_MAXF; ++f) { st.shift[f] = 0.f; st.scale[f] = 1.f; }
    hipLaunchKernelGGL(gpe_stitch_pairs_rows_kernel, dim3(gpe_cdiv(E, 256), B * (c1 - c0)), dim3(256), 0, (hipStream_t)stream, edges3d,
                       num_edges, P, L, Fe, st, c0, c1, rows_chunk, rows);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_stitch_pairs_reduce(const float* y, long ldy, const int32_t* num_edges, int B, int P, int L, int c0, int c1,
                                       long rows_chunk, uint64_t* table, float* logits, void* stream)
{
    if (!y || ldy <= 0 || !num_edges || !table || !sp_dims_ok(B, P, L)) return GPE_EINVAL;
    if (!sp_chunk_ok(P, L, c0, c1) || (long)B * (c1 - c0) > 65535 || rows_chunk <= 0) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_stitch_pairs_reduce_kernel<false>, dim3(gpe_cdiv(P * L, 256), B * (c1 - c0)), dim3(256), 0,
                       (hipStream_t)stream, y, ldy, num_edges, P, L, c0, c1, rows_chunk, reinterpret_cast<unsigned long long*>(table),
                       logits, nullptr, nullptr, nullptr);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_stitch_pairs_eval_reduce(const float* y, long ldy, const int32_t* num_edges, int B, int P, int L, int c0, int c1,
                                            long rows_chunk, uint64_t* table, float* logits, const uint32_t* mask, double* loss_slab,
                                            uint64_t* counters, void* stream)
{
    if (!y || ldy <= 0 || !num_edges || !table || !mask || !loss_slab || !counters || !sp_dims_ok(B, P, L)) return GPE_EINVAL;
    if (!sp_chunk_ok(P, L, c0, c1) || (long)B * (c1 - c0) > 65535 || rows_chunk <= 0) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_stitch_pairs_reduce_kernel<true>, dim3(1, B * (c1 - c0)), dim3(SP_TPB), 0, (hipStream_t)stream, y, ldy,
                       num_edges, P, L, c0, c1, rows_chunk, reinterpret_cast<unsigned long long*>(table), logits, mask, loss_slab,
                       reinterpret_cast<unsigned long long*>(counters));
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_stitch_pairs_labels(const int32_t* gt_stitches, const int32_t* gt_num_stitches, int B, int P, int L, int S,
                                       uint32_t* mask, void* stream)
{
    if (!gt_num_stitches || !mask || !sp_dims_ok(B, P, L) || S < 0 || (S > 0 && !gt_stitches)) return GPE_EINVAL;
    if (S == 0) return GPE_OK;
    hipLaunchKernelGGL(gpe_stitch_pairs_labels_kernel, dim3(gpe_cdiv(S, 256), B), dim3(256), 0, (hipStream_t)stream, gt_stitches,
                       gt_num_stitches, S, P * L, mask);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_stitch_eval_finalize(const double* loss_slab, long slots, int group, const uint64_t* counters, const uint32_t* mask,
                                        const int32_t* stitches, const int32_t* num_stitches, int B, int P, int L, double* loss_sum,
                                        int32_t* counts, float* metrics, void* stream)
{
    if (!loss_slab || !counters || !mask || !stitches || !num_stitches || !loss_sum || !counts || !metrics) return GPE_EINVAL;
    if (!sp_dims_ok(B, P, L) || P * L < 2 || group <= 0 || slots <= 0 || slots % group || slots / group > 64) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_stitch_eval_finalize_kernel, dim3(1), dim3(SP_FIN_TPB), 0, (hipStream_t)stream, loss_slab, slots, group,
                       reinterpret_cast<const unsigned long long*>(counters), mask, stitches, num_stitches, B, P, L, loss_sum, counts,
                       metrics);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_stitch_select(const uint64_t* table, int B, int P, int L, int32_t* stitches, int32_t* num_stitches, float* scores,
                                 void* stream)
{
    if (!table || !stitches || !num_stitches || !scores || !sp_dims_ok(B, P, L) || P * L < 2) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_stitch_select_kernel, dim3(B), dim3(SP_TPB), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned long long*>(table), P, L, (P * L) / 2, stitches, num_stitches, scores);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
