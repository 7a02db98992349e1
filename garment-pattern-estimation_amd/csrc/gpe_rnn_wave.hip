// Wavefront execution of stacked recurrences (nn.LSTM / nn.GRU under the reference's decoders,
// /root/reference/nn/net_blocks.py:336-497) on gfx950.
//
// A stack of L layers over T steps is L*T dependent cells when run layer by layer, but cell (l, t) only needs (l, t-1)
// and (l-1, t): all cells of one anti-diagonal d = l + t are independent.  The two entry points below walk the T + L - 1
// diagonals (gpe_rnn_walk_diagonals, gpe_rnn_seq.h) and launch every cell of a diagonal TOGETHER (blockIdx.z = cell):
//   forward : one fused launch per diagonal — gates = h_{l,t-1}.W_hh^T (+ h_{l-1,t}.W_ih^T for layers > 0, a second K
//             segment) + addend, then the LSTM / GRU cell update in the epilogue (gate-interleaved packed weights, so
//             the gates of a unit sit in one accumulator row);
//   backward: two launches per diagonal — split-K products dh = dG_{l,t+1}.W_hh + dG_{l+1,t}.W_ih over all cells and
//             K slabs at once, then the pointwise cell backward of all cells.
// The shipped decoders (T = 23, L = 2 and T = 14, L = 3) drop from 88 + 176 dependent launches to 40 + 80.
// Arithmetic: exact fp32 MFMA (v_mfma_f32_16x16x4_f32), same staging scheme as gpe_smallgemm.hip: a workgroup stages a
// whole K slab (<= 256) of 64 rows and of its packed weight block, one barrier pair per slab.
#include "gpe_rowgemm.h"
#include "gpe_rnn_seq.h"
#include <math.h>
#include <stdlib.h>

struct WvFwdCell {
    const float* a0; long a0_stride; const float* w0;       // h_{l,t-1} rows, gate-packed W_hh_l
    const float* a1; long a1_stride; const float* w1;       // h_{l-1,t} rows, gate-packed W_ih_l (NULL for layer 0)
    const unsigned* s0; const unsigned* s1;                 // H3: amax words of W_hh_l / W_ih_l (w0 / w1 are then plane packs)
    const float* xproj; long xp_stride;                     // addend rows [..][G*H] (stride 0: one bias row)
    const float* c_prev; float* c_out;                      // LSTM
    const float* bhn;                                       // GRU
    float* saved; float* h_out; long h_stride;              // saved gates [Bn][4H]; h rows
};
struct WvFwdParams { int Bn, H, Npad, ncell; WvFwdCell cell[WV_MAXCELL]; };

// ---- slab staging: rows [row0, row0+64) x K columns of `a` (row pitch `stride`, 16-B aligned, padded to 4) and the packed weight
// block of this workgroup (columns n0 .. n0+16*NT of a [K/4][Npad][4] packed matrix) go into LDS, then the slab's MFMAs run — as
// fetch (global -> registers) / commit (registers -> LDS) / multiply, so that the forward kernel can keep the NEXT slab's loads in
// flight under the current slab's MFMAs (a cell is 2-4 slabs: with the loads exposed every slab cost ~2.5 us of L2 latency on top
// of ~2 us of matrix work) -------------------------------------------------------------------------------------------------------
template <int NT, int KS>
struct WvRegs {
    float4 a[RG_BM / 4];
    float4 w[(KS * NT + 63) / 64];           // (KS/4 planes) x (16*NT columns) float4 over 256 threads
};

// H3 (f16x3 arithmetic, round 4): `wp` is the fp16-PLANE pack of the weight (gpe_pack_multi kinds 8 / 10: [plane][K / 8][Npad][8
// halves]); a slab's share of it has the same number of 16-byte pieces as the fp32 slab, in the order [plane][k-group][column],
// and lands in LDS in that order — the B fragments of v_mfma_f32_16x16x32_f16 are then single ds_read_b128.  The A slab stays
// fp32 in LDS (zero-filled to a multiple of 32 columns) and is split at fragment-read time (each element is read by ONE wave).
template <int NT, int KS, bool H3 = false>
__device__ __forceinline__ void wv_fetch(WvRegs<NT, KS>& R, const float* __restrict__ a, long stride,
                                         const float* __restrict__ wp, int K, int Npad, int row0, int rv, int n0, int ks)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kslab = (K - ks < KS) ? (K - ks) : KS;
    const int kp = (kslab + 15) & ~15;
    const int c = lane << 2;
    const int cc = (c < kslab) ? c : 0;                       // clamped: every load below is unconditional
#pragma unroll
    for (int q = 0; q < RG_BM / 4; ++q) {
        const int r = wave + 4 * q;
        R.a[q] = ld4(a + (long)(row0 + (r < rv ? r : rv - 1)) * stride + ks + cc);
    }
    constexpr int per_plane = 16 * NT;
    if constexpr (H3) {
        const int kg_slab = ((kslab + 31) & ~31) >> 3;                    // k-groups of 8 in this slab (whole 32-k steps)
        const int KG = ((K + 31) & ~31) >> 3;                             // ... in the whole K extent of the pack
        const int half = kg_slab * per_plane, total = 2 * half;
#pragma unroll
        for (int u = 0; u < (KS * NT + 63) / 64; ++u) {
            const int e = tid + 256 * u;
            const int ec = (e < total) ? e : total - 1;
            const int plane = ec >= half, r2 = ec - plane * half;
            const int kg = r2 / per_plane, n = r2 - kg * per_plane;
            const int nn = (n0 + n < Npad) ? n0 + n : Npad - 1;
            R.w[u] = ld4(wp + (((long)plane * KG + (ks >> 3) + kg) * Npad + nn) * 4);      // 16-byte pieces = "4 floats"
        }
        return;
    }
    const int total = (kp >> 2) * per_plane;
    const int chunk0 = ks >> 4;
#pragma unroll
    for (int u = 0; u < (KS * NT + 63) / 64; ++u) {
        const int e = tid + 256 * u;
        const int ec = (e < total) ? e : total - 1;
        const int pl = ec / per_plane, n = ec - pl * per_plane;
        const int nn = (n0 + n < Npad) ? n0 + n : Npad - 1;
        R.w[u] = ld4(wp + (((long)(chunk0 * 4 + pl)) * Npad + nn) * 4);
    }
}

template <int NT, int KS, bool H3 = false>
__device__ __forceinline__ void wv_commit(const WvRegs<NT, KS>& R, int K, int Npad, int rv, int n0, int ks, float* As,
                                          float* Ws, int lda)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kslab = (K - ks < KS) ? (K - ks) : KS;
    const int kp = H3 ? ((kslab + 31) & ~31) : ((kslab + 15) & ~15);
    const int c = lane << 2;
    if (c < kp) {
        const int nvalid = kslab - c;
#pragma unroll
        for (int q = 0; q < RG_BM / 4; ++q) {
            const int r = wave + 4 * q;
            float4 o = R.a[q];
            if (r >= rv || nvalid <= 0) o = make_float4(0.f, 0.f, 0.f, 0.f);
            else {
                if (nvalid < 2) o.y = 0.f;
                if (nvalid < 3) o.z = 0.f;
                if (nvalid < 4) o.w = 0.f;
            }
            st4(&As[r * lda + c], o);
        }
    }
    constexpr int per_plane = 16 * NT;
    const int total = H3 ? 2 * (kp >> 3) * per_plane : (kp >> 2) * per_plane;
#pragma unroll
    for (int u = 0; u < (KS * NT + 63) / 64; ++u) {
        const int e = tid + 256 * u;
        if (e < total) {
            const int n = e % per_plane;
            st4(&Ws[e * 4], (n0 + n < Npad) ? R.w[u] : make_float4(0.f, 0.f, 0.f, 0.f));
        }
    }
}

// f16x3 products of one staged slab: A rows fp32 in LDS, scaled by the power of two `sA` (the state rows: GPE_STATE_SA,
// gpe_device.h) and split into two fp16 terms right after the read; B = the weight's planes in LDS; three MFMAs per 16 x 16 x 32
// block, small terms first.  `split` as in wv_mma (a <= 32-row tile: wave w = row tile (w & 1), K half (w >> 1)).
template <int NT>
__device__ __forceinline__ void wv_mma_h3(const float* As, const float* Ws, int lda, int kp, float sA, f32x4 (&acc)[NT],
                                          bool split = false)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int nsteps = kp >> 5;                           // kp is a multiple of 32 here
    const int rt = split ? (wave & 1) : wave;
    const int half = (nsteps + 1) >> 1;
    const int s0 = (split && (wave >> 1)) ? half : 0;
    const int s1 = (split && !(wave >> 1)) ? half : nsteps;
    const int plane_f = (kp >> 3) * 16 * NT * 4;          // floats per plane of the staged slab
    for (int st = s0; st < s1; ++st) {
        const float* ar = &As[(16 * rt + j) * lda + 32 * st + 8 * g];
        const float4 a0 = ld4(ar), a1 = ld4(ar + 4);
        gpe_u32x4 ah, al;
        { unsigned h, l; gpe_split2_f16(a0.x, a0.y, sA, h, l); ah[0] = h; al[0] = l; }
        { unsigned h, l; gpe_split2_f16(a0.z, a0.w, sA, h, l); ah[1] = h; al[1] = l; }
        { unsigned h, l; gpe_split2_f16(a1.x, a1.y, sA, h, l); ah[2] = h; al[2] = l; }
        { unsigned h, l; gpe_split2_f16(a1.z, a1.w, sA, h, l); ah[3] = h; al[3] = l; }
        const float* wb = &Ws[(((4 * st + g) * 16 * NT) + j) * 4];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const gpe_u32x4 bh = *reinterpret_cast<const gpe_u32x4*>(wb + 64 * n);
            const gpe_u32x4 bl = *reinterpret_cast<const gpe_u32x4*>(wb + 64 * n + plane_f);
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(gpe_f16x8, al), __builtin_bit_cast(gpe_f16x8, bh), acc[n], 0, 0, 0);
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(gpe_f16x8, ah), __builtin_bit_cast(gpe_f16x8, bl), acc[n], 0, 0, 0);
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(gpe_f16x8, ah), __builtin_bit_cast(gpe_f16x8, bh), acc[n], 0, 0, 0);
        }
    }
}

// split (a tile with <= 32 valid rows — the pattern decoders run Bn = 32): waves 2, 3 would only multiply zero rows, so
// instead wave w takes row tile (w & 1) and HALF of the slab's K chunks (w >> 1); the halves meet in the C tile, where
// rows 32..63 hold the second half's partial sums of rows 0..31 (the epilogues add them).
template <int NT>
__device__ __forceinline__ void wv_mma(const float* As, const float* Ws, int lda, int kp, f32x4 (&acc)[NT], bool split = false)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int nchunks = kp >> 4;
    const int rt = split ? (wave & 1) : wave;
    const int half = (nchunks + 1) >> 1;
    const int kc0 = (split && (wave >> 1)) ? half : 0;
    const int kc1 = (split && !(wave >> 1)) ? half : nchunks;
    for (int kc = kc0; kc < kc1; ++kc) {
        const float4 a4 = ld4(&As[(16 * rt + j) * lda + kc * 16 + 4 * g]);
        const float av[4] = {a4.x, a4.y, a4.z, a4.w};
        float4 b4[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) b4[n] = ld4(&Ws[(((kc * 4 + g) * 16 * NT) + 16 * n + j) * 4]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const float bv = (t == 0) ? b4[n].x : (t == 1) ? b4[n].y : (t == 2) ? b4[n].z : b4[n].w;
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], bv, acc[n], 0, 0, 0);
            }
        }
    }
}

// G = 4: LSTM (i,f,g,o)   G = 3: GRU (r,z,n).   H3: f16x3 arithmetic (gpe_math_set(4)) — weights as fp16 plane packs with their
// amax words, the state rows split on the fly, three fp16 MFMAs per product block, fp32 accumulate (wv_mma_h3).
template <int G, int KS, bool H3 = false>
__global__ __launch_bounds__(256, (KS <= 128 ? 2 : 1)) void gpe_rnn_wave_fwd_kernel(WvFwdParams p)
{
    extern __shared__ __align__(16) float smem[];
    const int kp_max = H3 ? (((p.H < KS ? p.H : KS) + 31) & ~31) : (((p.H < KS ? p.H : KS) + 15) & ~15);
    const int lda = kp_max + 4;
    constexpr int ldc = 16 * 2 * G + 4;              // GRU keeps the input-side and recurrent-side products apart
    const int a_floats = RG_BM * (lda > ldc ? lda : ldc);
    float* As = smem;
    float* Cs = smem;
    float* Ws = smem + a_floats;
    const WvFwdCell& c = p.cell[blockIdx.z];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.x * RG_BM;
    const int rv = (p.Bn - row0 < RG_BM) ? (p.Bn - row0) : RG_BM;
    const int n0 = blockIdx.y * (16 * G);

    const bool split = rv <= 32;                      // wave-pair K split (wv_mma)
    float h3_inv0 = 1.f, h3_inv1 = 1.f, h3_ratio = 1.f;
    if constexpr (H3) {
        float sw0, sw1 = 1.f;
        gpe_h3_scale_of(c.s0[0], sw0, h3_inv0);
        if (c.a1) gpe_h3_scale_of(c.s1[0], sw1, h3_inv1);
        h3_ratio = h3_inv0 * sw1;                     // = inv0 / inv1
        h3_inv0 *= GPE_STATE_INV_SA; h3_inv1 *= GPE_STATE_INV_SA;
    }
    f32x4 accH[G], accX[G];
#pragma unroll
    for (int n = 0; n < G; ++n) { accH[n] = (f32x4){0.f, 0.f, 0.f, 0.f}; accX[n] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    // epilogue operands (addend rows, c_{t-1} / h_{t-1}) are fetched FIRST: their L2 latency hides under the slab loop
    // instead of sitting between the last MFMA and the cell update
    const int u = tid & 15;
    const int unit = blockIdx.y * 16 + u;
    const int unitc = (unit < p.H) ? unit : p.H - 1;
    constexpr int IT = RG_BM / 16;
    float e0[IT], e1[IT], e2[IT], e3[IT], e4[IT];
    const float bhn = (G == 3) ? c.bhn[unitc] : 0.f;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int r = (tid >> 4) + 16 * it;
        const long gr = row0 + (r < rv ? r : rv - 1);
        const float* xp = c.xproj + gr * c.xp_stride;
        e0[it] = xp[unitc]; e1[it] = xp[p.H + unitc]; e2[it] = xp[2 * p.H + unitc];
        if (G == 4) { e3[it] = xp[3 * p.H + unitc]; e4[it] = c.c_prev[gr * p.H + unitc]; }
        else { e3[it] = c.a0[gr * c.a0_stride + unitc]; e4[it] = 0.f; }
    }
    // slab jobs: segment 0 = h_{l,t-1} x W_hh, segment 1 (layers > 0) = h_{l-1,t} x W_ih, each cdiv(H, KS) slabs
    {
        const int nslab = (p.H + KS - 1) / KS;
        const int njobs = c.a1 ? 2 * nslab : nslab;
        WvRegs<G, KS> R;
        auto job_fetch = [&](int i) {
            const int seg = (i >= nslab) ? 1 : 0, ks = (i - seg * nslab) * KS;
            wv_fetch<G, KS, H3>(R, seg ? c.a1 : c.a0, seg ? c.a1_stride : c.a0_stride, seg ? c.w1 : c.w0, p.H, p.Npad, row0, rv,
                                n0, ks);
        };
        job_fetch(0);
        for (int i = 0; i < njobs; ++i) {
            const int seg = (i >= nslab) ? 1 : 0, ks = (i - seg * nslab) * KS;
            const int kslab = (p.H - ks < KS) ? (p.H - ks) : KS;
            __syncthreads();                               // the previous slab's MFMAs are done with As / Ws
            wv_commit<G, KS, H3>(R, p.H, p.Npad, rv, n0, ks, As, Ws, lda);
            __syncthreads();
            job_fetch(i + 1 < njobs ? i + 1 : i);          // unconditional (the last one re-fetches itself): a load under
                                                           // a branch is waited for at the join
            if constexpr (H3) {
                if (G == 4 && i == nslab) {
                    // the LSTM's single accumulator crosses from W_hh's scale into W_ih's: an exact power-of-two rescale
#pragma unroll
                    for (int n = 0; n < G; ++n)
#pragma unroll
                        for (int r = 0; r < 4; ++r) accH[n][r] *= h3_ratio;
                }
                if (G == 4 || seg == 0) wv_mma_h3<G>(As, Ws, lda, (kslab + 31) & ~31, GPE_STATE_SA, accH, split);
                else wv_mma_h3<G>(As, Ws, lda, (kslab + 31) & ~31, GPE_STATE_SA, accX, split);
            } else {
                if (G == 4 || seg == 0) wv_mma<G>(As, Ws, lda, (kslab + 15) & ~15, accH, split);
                else wv_mma<G>(As, Ws, lda, (kslab + 15) & ~15, accX, split);
            }
        }
    }
    if constexpr (H3) {
        // undo the operand scales (exact: powers of two): state 2^-12, weight from its amax word.  LSTM: accH ends in the scale of
        // its last segment (W_ih for layers > 0, see the rescale above); GRU: one accumulator per segment
#pragma unroll
        for (int n = 0; n < G; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (G == 4) accH[n][r] *= (c.a1 ? h3_inv1 : h3_inv0);
                else { accH[n][r] *= h3_inv0; accX[n][r] *= h3_inv1; }
            }
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < G; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Cs[(16 * wave + 4 * g + r) * ldc + 16 * n + j] = accH[n][r];
            if (G == 3) Cs[(16 * wave + 4 * g + r) * ldc + 16 * (G + n) + j] = accX[n][r];
        }
    __syncthreads();

    // C element (row, col) of the tile; with the wave-pair K split rows 32.. carry the second half of rows 0..31
    auto cs_at = [&](int r, int col) -> float {
        const float v = Cs[r * ldc + col];
        return split ? v + Cs[(r + 32) * ldc + col] : v;
    };
    if (unit >= p.H) return;
    if (G == 4) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int r = (tid >> 4) + 16 * it;
            if (r < rv) {
                const long gr = row0 + r;
                // gpe_lstm_cell_fwd's formulas in this kernel's own order, each C-tile read right in front of its activation: through
                // the shared function the reads come first, the compiler then fuses the other product of c_t and every result of
                // the diagonal launches moves in its last bits
                const float ig = gpe_sigmoid(cs_at(r, u) + e0[it]);
                const float fg = gpe_sigmoid(cs_at(r, 16 + u) + e1[it]);
                const float gg = tanhf(cs_at(r, 32 + u) + e2[it]);
                const float og = gpe_sigmoid(cs_at(r, 48 + u) + e3[it]);
                const float cn = fg * e4[it] + ig * gg;
                float* go = c.saved + gr * 4 * p.H;
                go[unit] = ig; go[p.H + unit] = fg; go[2 * p.H + unit] = gg; go[3 * p.H + unit] = og;
                c.c_out[gr * p.H + unit] = cn;
                c.h_out[gr * c.h_stride + unit] = gpe_lstm_cell_h(og, cn);
            }
        }
    } else {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int r = (tid >> 4) + 16 * it;
            if (r < rv) {
                const long gr = row0 + r;
                const float rg = gpe_sigmoid(cs_at(r, u) + cs_at(r, 48 + u) + e0[it]);
                const float zg = gpe_sigmoid(cs_at(r, 16 + u) + cs_at(r, 64 + u) + e1[it]);
                const float hn = cs_at(r, 32 + u) + bhn;
                const float ng = tanhf(cs_at(r, 80 + u) + e2[it] + rg * hn);
                float* go = c.saved + gr * 4 * p.H;
                go[unit] = rg; go[p.H + unit] = zg; go[2 * p.H + unit] = ng; go[3 * p.H + unit] = hn;
                c.h_out[gr * c.h_stride + unit] = (1.f - zg) * ng + zg * e3[it];
            }
        }
    }
}

// K slab of the wavefront kernels: 128 -> 67 KB of LDS per workgroup, two workgroups per CU (a diagonal of the shipped
// panel decoder is 576 workgroups: with 256-wide slabs (132 KB, one per CU) it runs in three rounds).  GPE_WV_KS=256
// selects the wide slab (A/B measurements).
static int wv_ks()
{
    static int ks = 0;
    if (!ks) {
        const char* e = gpe_dbg_env_str("GPE_WV_KS");
        const int v = e ? atoi(e) : 0;
        ks = (v == 256) ? 256 : 128;
    }
    return ks;
}

// does the last (or only) 64-row tile run the wave-pair K split of wv_mma?
static int wv_split_mode(int Bn) { return Bn - RG_BM * (gpe_cdiv(Bn, RG_BM) - 1) <= 32; }
// cells of the largest launch and launches of the longest diagonal (gpe_rnn_walk_diagonals)
static void wv_groups(int L, int T, int& ncell_max, int& groups)
{
    const int longest = L < T ? L : T;
    ncell_max = longest < WV_MAXCELL ? longest : WV_MAXCELL;
    groups = gpe_cdiv(longest, WV_MAXCELL);
}

// plan step of the forward: slab width, padded slab extent and LDS image of every launch of the walk
struct WvFwdPlan { int ks, kp_max; size_t lds; };
static int wv_fwd_plan(const GpeRnnSeq& q, WvFwdPlan& w, GpeRnnPath* out)
{
    // a single row tile (the pattern decoders) is a pure latency chain: the wide slab halves its barrier pairs
    // (a 96-wide slab — 50 KB, three workgroups per CU, the 576-workgroup panel diagonal in one round — measured slower:
    // 686 vs 641 us per panel-decoder forward; three slabs per segment instead of two)
    const bool wide = wv_ks() == 256 || q.Bn <= RG_BM;
    w.ks = wide ? 256 : 128;
    w.kp_max = gpe_round_up(q.H < w.ks ? q.H : w.ks, q.f16 ? 32 : 16);
    const int lda = w.kp_max + 4, ldc = 16 * 2 * q.G + 4;
    w.lds = ((size_t)RG_BM * (lda > ldc ? lda : ldc) + (size_t)w.kp_max * 16 * q.G) * sizeof(float);
    if (w.lds > GPE_RNN_LDS_CAP) return GPE_EINVAL;
    if (out) {
        int ncell_max, groups;
        wv_groups(q.L, q.T, ncell_max, groups);
        out->f16 = q.f16; out->KP = w.kp_max; out->lds = (long)w.lds; out->ks = w.ks; out->split = wv_split_mode(q.Bn);
        out->grid = (long)gpe_cdiv(q.Bn, RG_BM) * gpe_cdiv(q.H, 16) * ncell_max; out->groups = groups;
    }
    return GPE_RNN_LAUNCHED;
}

template <int G>
static int wv_fwd_launch(const WvFwdParams& p, bool h3, const WvFwdPlan& w, hipStream_t s)
{
    return gpe_rnn_for_bool(h3, [&](auto h3c) {
        return gpe_rnn_for_ks(w.ks, [&](auto ksc) {
            constexpr bool H3 = decltype(h3c)::value;
            constexpr int KS = decltype(ksc)::value;
            return gpe_rnn_launch<gpe_rnn_wave_fwd_kernel<G, KS, H3>, GPE_RNN_LDS_CAP>(
                dim3(gpe_cdiv(p.Bn, RG_BM), gpe_cdiv(p.H, 16), p.ncell), 256, w.lds, s, p);
        });
    });
}

// one fused launch per group of a diagonal's cells; takes every stack
int gpe_rnn_wave_fwd(const GpeRnnSeq& q, GpeRnnPath* plan_only)
{
    const int G = q.G;
    WvFwdPlan w;
    const int rcp = wv_fwd_plan(q, w, plan_only);
    if (rcp < 0 || plan_only) return rcp;
    return gpe_rnn_walk_diagonals(q.L, q.T, false, [&](int d, int l0, int l_top) {
        WvFwdParams p = {};
        p.Bn = q.Bn; p.H = q.H; p.Npad = 16 * G * gpe_cdiv(q.H, 16);
        int n = 0;
        // highest layer first: workgroups are dispatched in blockIdx.z order and a 3-cell panel diagonal is 576
        // workgroups on 512 slots — the second round should be the cheap layer-0 cells (one K segment instead of two)
        for (int l = l_top; l >= l0; --l, ++n) {
            const int t = d - l;
            WvFwdCell& c = p.cell[n];
            c.a0 = q.h(l, t);                                    // h_{l,t-1} lives at time slot t
            c.a0_stride = q.hs_sb;
            c.w0 = (const float*)q.whh[l];
            c.s0 = q.f16 ? (const unsigned*)q.whh_amax[l] : nullptr;
            if (l > 0) {
                c.a1 = q.h(l - 1, t + 1);                        // h_{l-1,t} at slot t+1
                c.a1_stride = q.hs_sb;
                c.w1 = (const float*)q.wih[l];
                c.s1 = q.f16 ? (const unsigned*)q.wih_amax[l] : nullptr;
                c.xproj = (const float*)q.bias[l];
                c.xp_stride = 0;
            } else {
                c.xproj = q.xproj0 + (long)t * q.xp0_st;
                c.xp_stride = q.xp0_sb;
            }
            if (G == 4) {
                c.c_prev = q.c(l, t);
                c.c_out = q.c(l, t + 1);
            } else
                c.bhn = (const float*)q.bhn[l];
            c.saved = q.gates(l, t);
            c.h_out = q.h(l, t + 1);
            c.h_stride = q.hs_sb;
        }
        p.ncell = n;
        return (G == 4) ? wv_fwd_launch<4>(p, q.f16, w, q.s) : wv_fwd_launch<3>(p, q.f16, w, q.s);
    });
}

// =====================================================================================================================
// backward
// =====================================================================================================================
struct WvBwdCell {
    // split-K products: segment s multiplies rows a[s] [Bn][K] (pitch as[s]) with packed w[s] ([H out] x [K]); NULL = absent
    const float* a[2]; long as[2]; const float* w[2];
    float* part;                                   // [2 * nz][Bn][H] partial products of this cell
    // pointwise
    const float* dh_out; long dho_stride;          // top-layer output gradient rows or NULL
    const float* dh_extra;                         // d h_T of this layer (t == T-1) or NULL          [Bn][H]
    const float* carry_in; float* carry_out;       // dc (LSTM) / z-gated dh (GRU) of step t+1 -> of step t  [Bn][H]
    const float* saved;                            // activated gates of the cell [Bn][4H]
    const float* c; const float* c_prev;           // LSTM: c_t, c_{t-1} [Bn][H]
    const float* h_prev; long hp_stride;           // GRU
    float* dgx; float* dgh; long dg_stride;        // pre-activation gradients of the cell, rows [Bn] pitch dg_stride
    int nseg_mask;                                 // bit s: segment s present
};
// nz = K-slab GROUPS of the launch (partials per segment); a workgroup multiplies `jslabs` consecutive slabs of its group
// fuse (LSTM): the workgroup that completes an output block — the last of the block's split-K partials to arrive, by a counter per
// (cell, row tile, column block) at cnt — runs the pointwise cell backward of that block itself (no second launch per diagonal);
// Hp = row pitch of the partial images (H rounded up to 4: 16-byte write-through stores)
struct WvBwdParams { int Bn, H, K, Kpad_n, nz, jslabs, ncell, fuse, Hp; unsigned* cnt; WvBwdCell cell[WV_MAXCELL]; };

// grid (row tiles, cdiv(H, 64), ncell * 2 * nz): block z -> (cell, segment, K slab)
// (The same products on the fp16 pipe were built and measured in round 4 — dG rows scaled by a per-cell amax word that the
// pointwise kernel filled by atomicMax, transposed plane packs — and dropped: gpe_rnn_seq_bwd 1.00 -> 1.09 ms per step at cfg 2,
// the atomics + the word memset + the split of 16 short slabs per workgroup cost more than the MFMAs they replace;
// profiles/r04_e_recurrences.md.)
// pointwise LSTM cell backward of one element (shared by the stand-alone kernel and the fused epilogue): the loads and stores
// around gpe_lstm_cell_bwd
__device__ __forceinline__ void wv_lstm_cell_bwd(const WvBwdCell& c, int H, long b, int u, long e, float dh)
{
    const float* sv = c.saved + b * 4 * H;
    float* gx = c.dgx + b * c.dg_stride;
    float di, df, dg, dgo, cout;
    gpe_lstm_cell_bwd(sv[u], sv[H + u], sv[2 * H + u], sv[3 * H + u], c.c[e], c.c_prev[e], dh, c.carry_in ? c.carry_in + e : nullptr,
                      di, df, dg, dgo, cout);
    gx[u] = di; gx[H + u] = df; gx[2 * H + u] = dg; gx[3 * H + u] = dgo;
    c.carry_out[e] = cout;
}

template <int KS>
__global__ __launch_bounds__(256) void gpe_rnn_wave_splitk_kernel(WvBwdParams p)
{
    extern __shared__ __align__(16) float smem[];
    __shared__ unsigned last_sh;
    constexpr int NT = 4;
    const int lda = KS + 4;
    constexpr int ldc = 16 * NT + 4;
    float* As = smem;
    float* Cs = smem;
    float* Ws = smem + RG_BM * lda;
    const int zz = blockIdx.z;
    const int ci = zz / (2 * p.nz), rem = zz - ci * 2 * p.nz;
    const int seg = rem / p.nz, z = rem - seg * p.nz;
    const WvBwdCell& c = p.cell[ci];
    const int nsegs = (c.nseg_mask & 1) + ((c.nseg_mask >> 1) & 1);
    const bool present = (c.nseg_mask >> seg) & 1;
    // fused: a cell without any product (the top layer's last step) is finished by the workgroups of (segment 0, slab group 0)
    if (!present && !(p.fuse && nsegs == 0 && seg == 0 && z == 0)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.x * RG_BM;
    const int rv = (p.Bn - row0 < RG_BM) ? (p.Bn - row0) : RG_BM;
    const int n0 = blockIdx.y * (16 * NT);
    const int ncols = (p.H - n0 < 16 * NT) ? (p.H - n0) : 16 * NT;
    const int Hp = p.fuse ? p.Hp : p.H;
    if (present) {
        f32x4 acc[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const bool split = rv <= 32;
        // this workgroup's slabs ks = (z * jslabs + i) * KS, i < jslabs, while ks < K: the next slab's loads stay in flight
        // under the current slab's MFMAs (same pipeline as the forward)
        {
            const int ks0 = z * p.jslabs * KS;
            int njobs = (p.K - ks0 + KS - 1) / KS;
            if (njobs > p.jslabs) njobs = p.jslabs;
            WvRegs<NT, KS> R;
            auto job_fetch = [&](int i) {
                const int ks = ks0 + i * KS;
                wv_fetch<NT, KS>(R, c.a[seg] + ks, c.as[seg], c.w[seg] + (long)(ks >> 4) * 4 * p.Kpad_n * 4, p.K - ks, p.Kpad_n, row0, rv,
                                 n0, 0);
            };
            job_fetch(0);
            for (int i = 0; i < njobs; ++i) {
                const int ks = ks0 + i * KS;
                const int kslab = (p.K - ks < KS) ? (p.K - ks) : KS;
                __syncthreads();
                wv_commit<NT, KS>(R, p.K - ks, p.Kpad_n, rv, n0, 0, As, Ws, lda);
                __syncthreads();
                job_fetch(i + 1 < njobs ? i + 1 : i);
                wv_mma<NT>(As, Ws, lda, (kslab + 15) & ~15, acc, split);
            }
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) Cs[(16 * wave + 4 * g + r) * ldc + 16 * n + j] = acc[n][r];
        __syncthreads();
        const int cq = lane << 2;
        float* dst0 = c.part + ((long)(seg * p.nz + z) * p.Bn) * Hp;
        if (p.fuse) {
            // write-through (sc1) 16-byte stores: the block's last arriver reads them inside this launch.  Hp is a multiple of 4, so
            // a quad that starts inside the row may run into its pad columns
            if (cq < ((ncols + 3) & ~3)) {
                const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(dst0, 0, (unsigned)((long)p.Bn * Hp * 4), 0x00020000);
                for (int r = wave; r < rv; r += 4) {
                    float4 v = ld4(&Cs[r * ldc + cq]);
                    if (split) {
                        const float4 v2 = ld4(&Cs[(r + 32) * ldc + cq]);
                        v.x += v2.x; v.y += v2.y; v.z += v2.z; v.w += v2.w;
                    }
                    const gpe_u32x4 o = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
                    __builtin_amdgcn_raw_buffer_store_b128(o, rs, (int)(((long)(row0 + r) * Hp + n0 + cq) * 4), 0, 16);
                }
            }
        } else if (cq < ncols) {
            for (int r = wave; r < rv; r += 4) {
                float4 v = ld4(&Cs[r * ldc + cq]);
                if (split) {
                    const float4 v2 = ld4(&Cs[(r + 32) * ldc + cq]);
                    v.x += v2.x; v.y += v2.y; v.z += v2.z; v.w += v2.w;
                }
                float* dst = dst0 + (long)(row0 + r) * p.H + n0 + cq;
                const float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int t = 0; t < 4; ++t) if (cq + t < ncols) dst[t] = o[t];
            }
        }
    }
    if (!p.fuse) return;
    // ---- fused cell backward: count this workgroup in; the block's last arriver owns the pointwise pass (gpe_device.h: hand-off,
    // the last-arriver ticket; MI355X_MICROARCH.md "splitk-seam") ----
    const int nparts = nsegs * p.nz;
    if (nparts > 1) {
        gpe_drain_stores();
        __syncthreads();
        if (tid == 0) last_sh = gpe_flag_ticket(p.cnt + ((long)ci * gridDim.x + blockIdx.x) * gridDim.y + blockIdx.y);
        __syncthreads();
        if (last_sh != (unsigned)(nparts - 1)) return;
    } else if (nparts == 1) {
        gpe_drain_stores();
        __syncthreads();
    }
    const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(c.part, 0, (unsigned)((long)2 * p.nz * p.Bn * Hp * 4), 0x00020000);
    // 64 rows x 16 column quads; a thread: row tid / 16 + 16 it, quad tid % 16
    const int q4 = (tid & 15) << 2;
    if (q4 < ncols) {
#pragma unroll
        for (int it = 0; it < RG_BM / 16; ++it) {
            const int r = (tid >> 4) + 16 * it;
            if (r >= rv) break;
            const long b = row0 + r;
            float dh4[4] = {0.f, 0.f, 0.f, 0.f};
            for (int s = 0; s < 2; ++s)
                if ((c.nseg_mask >> s) & 1)
                    for (int zq = 0; zq < p.nz; ++zq) {
                        const gpe_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rp, (int)((((long)(s * p.nz + zq) * p.Bn + b) * Hp + n0 + q4) * 4), 0, 16);
                        dh4[0] += __uint_as_float(v[0]); dh4[1] += __uint_as_float(v[1]);
                        dh4[2] += __uint_as_float(v[2]); dh4[3] += __uint_as_float(v[3]);
                    }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int u = n0 + q4 + t;
                if (u >= p.H) break;
                const long e = b * p.H + u;
                float dh = dh4[t];
                if (c.dh_out) dh += c.dh_out[b * c.dho_stride + u];
                if (c.dh_extra) dh += c.dh_extra[e];
                wv_lstm_cell_bwd(c, p.H, b, u, e, dh);
            }
        }
    }
}

template <int G>
__global__ void gpe_rnn_wave_cell_bwd_kernel(WvBwdParams p)
{
    const WvBwdCell& c = p.cell[blockIdx.y];
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)p.Bn * p.H) return;
    const int H = p.H;
    const long b = e / H;
    const int u = (int)(e - b * H);
    float dh = c.dh_out ? c.dh_out[b * c.dho_stride + u] : 0.f;
    if (c.dh_extra) dh += c.dh_extra[e];
    for (int s = 0; s < 2; ++s)
        if ((c.nseg_mask >> s) & 1)
            for (int z = 0; z < p.nz; ++z) dh += c.part[((long)(s * p.nz + z) * p.Bn) * H + e];
    const float* sv = c.saved + b * 4 * H;
    float* gx = c.dgx + b * c.dg_stride;
    if (G == 4) {
        wv_lstm_cell_bwd(c, H, b, u, e, dh);
    } else {
        if (c.carry_in) dh += c.carry_in[e];
        const float rg = sv[u], zg = sv[H + u], ng = sv[2 * H + u], hn = sv[3 * H + u];
        const float hp = c.h_prev[b * c.hp_stride + u];
        const float dn_pre = dh * (1.f - zg) * (1.f - ng * ng);
        const float dz_pre = dh * (hp - ng) * zg * (1.f - zg);
        const float dr_pre = dn_pre * hn * rg * (1.f - rg);
        float* gh = c.dgh + b * c.dg_stride;
        gx[u] = dr_pre; gx[H + u] = dz_pre; gx[2 * H + u] = dn_pre;
        gh[u] = dr_pre; gh[H + u] = dz_pre; gh[2 * H + u] = dn_pre * rg;
        c.carry_out[e] = dh * zg;
    }
}

// floats of the diagonal backward's workspace: partial images (row pitch H rounded up to 4: the fused kernel stores them in 16-byte
// pieces) + one arrival counter per (diagonal, cell, row tile, column block) of the fused split-K + cell-backward launches
long gpe_rnn_wave_bwd_ws_floats(int gates, int L, int T, int Bn, int H)
{
    const int nz = gpe_cdiv(gates * H, 128);              // sized for the narrow slab (the wide one needs half)
    const int ncell = L < WV_MAXCELL ? L : WV_MAXCELL;
    return (long)ncell * 2 * nz * Bn * gpe_round_up(H, 4) + (long)(T + L) * WV_MAXCELL * gpe_cdiv(Bn, RG_BM) * gpe_cdiv(H, 64) + 64;
}

// two launches per group of a diagonal's cells (split-K products, pointwise cell backward); takes every stack.  On return
// carry slot 0 holds dc_0 / the z-gated dh_0 of every layer
//
// plan step: slab width, slabs per workgroup, partial images, the fused mode and where its counters start, the LDS image
struct WvBwdPlan { int KS, jslabs, nz, fuse, Hp, gxr, gyc, ncell_max; long cnt_off, cnt_per_launch; size_t lds; };
static void wv_bwd_plan(const GpeRnnSeqBwd& q, WvBwdPlan& w, GpeRnnPath* out)
{
    const int G = q.G, L = q.L, Bn = q.Bn, H = q.H, K = G * H;
    const int KS = wv_ks();
    // big batches: four slabs per workgroup (a 3-cell panel diagonal: 2304 single-slab workgroups in 4.5 rounds -> 480 in one,
    // a quarter of the partial images; measured 804 / 717 / 621 / 689 us per backward at 1 / 2 / 4 / 8 slabs); a single row
    // tile (the pattern decoders) stays at one slab per workgroup — it is a latency chain, not a throughput problem
    static const int dbg_bj = gpe_dbg_env("GPE_WV_BJ", 0);             // measurement override
    int jslabs = (Bn > 3 * RG_BM) ? (gpe_cdiv(K, KS) < 4 ? gpe_cdiv(K, KS) : 4) : 1;
    if (dbg_bj > 0 && Bn > 3 * RG_BM) jslabs = dbg_bj < gpe_cdiv(K, KS) ? dbg_bj : gpe_cdiv(K, KS);
    const int nz = gpe_cdiv(gpe_cdiv(K, KS), jslabs);
    // LSTM, gpe_debug_set(65536): the pointwise cell backward runs in the split-K launch itself (the last partial of an output block
    // to arrive does it): one launch per diagonal instead of two.  Built, bit-compatible (same tests), and
    // MEASURED SLOWER — cfg 2, one session, twice each: gpe_rnn_seq_bwd 0.838 ms with two launches, 1.115 / 1.117 ms fused (step
    // 9.15 -> 9.46 / 9.50 ms): the block's last arriver runs drain + ticket + write-through partial reads + a latency-bound
    // 64 x 64 pointwise pass on ONE workgroup per block at the tail of every diagonal, which costs more than the 9 us memory-parallel
    // launch it replaces.  Off by default.
    const int fuse = (G == 4) && L <= WV_MAXCELL && (gpe_debug_get() & 65536);
    const int Hp = fuse ? gpe_round_up(H, 4) : H;
    const long BHp = (long)Bn * Hp;
    const int gxr = gpe_cdiv(Bn, RG_BM), gyc = gpe_cdiv(H, 64);
    const int ncell_max = L < WV_MAXCELL ? L : WV_MAXCELL;
    w = {KS, jslabs, nz, fuse, Hp, gxr, gyc, ncell_max, ((long)ncell_max * 2 * nz * BHp + 15) & ~15L, (long)WV_MAXCELL * gxr * gyc,
         ((size_t)RG_BM * (KS + 4) + (size_t)KS * 64) * sizeof(float)};
    if (out) {
        int cells, groups;
        wv_groups(L, q.T, cells, groups);
        out->ks = KS; out->split = wv_split_mode(Bn); out->jslabs = jslabs; out->nz = nz; out->fuse = fuse; out->Hp = Hp;
        out->groups = groups; out->lds = (long)w.lds; out->grid = (long)gxr * gyc * cells * 2 * nz;
        out->ws_used = fuse ? w.cnt_off + (q.T + L) * w.cnt_per_launch : (long)ncell_max * 2 * nz * BHp;
    }
}

int gpe_rnn_wave_bwd(const GpeRnnSeqBwd& q, GpeRnnPath* plan_only)
{
    WvBwdPlan w;
    wv_bwd_plan(q, w, plan_only);
    if (plan_only) return GPE_RNN_LAUNCHED;
    const int G = q.G, L = q.L, T = q.T, Bn = q.Bn, H = q.H, K = G * H;
    const int KS = w.KS, jslabs = w.jslabs, nz = w.nz, fuse = w.fuse, Hp = w.Hp, gxr = w.gxr, gyc = w.gyc;
    const long BH = (long)Bn * H, BHp = (long)Bn * Hp;
    unsigned* cnt_base = reinterpret_cast<unsigned*>(q.part + w.cnt_off);
    const long cnt_per_launch = w.cnt_per_launch;
    int launch_no = 0;
    if (fuse && hipMemsetAsync(cnt_base, 0, (size_t)(T + L) * cnt_per_launch * sizeof(unsigned), q.s) != hipSuccess) return GPE_ELAUNCH;
    const size_t lds = w.lds;
    return gpe_rnn_walk_diagonals(L, T, true, [&](int d, int l0, int l_top) {
        WvBwdParams p = {};
        p.Bn = Bn; p.H = H; p.K = K; p.Kpad_n = gpe_round_up(H, 16); p.nz = nz; p.jslabs = jslabs;
        p.fuse = fuse; p.Hp = Hp; p.cnt = cnt_base + (long)launch_no * cnt_per_launch;
        ++launch_no;
        int n = 0, any_seg = 0;
        for (int l = l0; l <= l_top; ++l, ++n) {
            const int t = d - l;
            WvBwdCell& c = p.cell[n];
            c.part = q.part + (long)n * 2 * nz * BHp;
            if (t < T - 1) {                 // recurrent path: dGh_{l,t+1} . W_hh_l
                c.a[0] = q.dh(l, t + 1); c.as[0] = q.dg_sb; c.w[0] = (const float*)q.whh_t[l];
                c.nseg_mask |= 1;
            }
            if (l < L - 1) {                 // from the layer above: dGx_{l+1,t} . W_ih_{l+1}
                c.a[1] = q.dx(l + 1, t); c.as[1] = q.dg_sb; c.w[1] = (const float*)q.wih_t[l + 1];
                c.nseg_mask |= 2;
            }
            any_seg |= c.nseg_mask;
            if (l == L - 1 && q.dtop) { c.dh_out = q.dtop + (long)t * q.dt_st; c.dho_stride = q.dt_sb; }
            if (t == T - 1) {
                if (q.d_hN) c.dh_extra = q.d_hN + (long)l * BH;
                c.carry_in = (G == 4 && q.d_cN) ? q.d_cN + (long)l * BH : nullptr;
            } else
                c.carry_in = q.carry_at(t + 1, l);
            c.carry_out = q.carry_at(t, l);
            c.saved = q.gates(l, t);
            if (G == 4) {
                c.c = q.c(l, t + 1);
                c.c_prev = q.c(l, t);
            } else {
                c.h_prev = q.h(l, t); c.hp_stride = q.hs_sb;
            }
            c.dgx = q.dx(l, t);
            c.dgh = q.dh(l, t);
            c.dg_stride = q.dg_sb;
        }
        p.ncell = n;
        if (any_seg || fuse) {
            // (4 bytes of static __shared__ beside the dynamic image)
            const int rc = gpe_rnn_for_ks(KS, [&](auto ksc) {
                return gpe_rnn_launch<gpe_rnn_wave_splitk_kernel<decltype(ksc)::value>, GPE_RNN_LDS_CAP_STATIC>(
                    dim3(gxr, gyc, n * 2 * nz), 256, lds, q.s, p);
            });
            if (rc < 0 || fuse) return rc;
        }
        const dim3 grid(gpe_cdiv(BH, 256), n);
        return (G == 4) ? gpe_rnn_launch<gpe_rnn_wave_cell_bwd_kernel<4>, 0>(grid, 256, 0, q.s, p)
                        : gpe_rnn_launch<gpe_rnn_wave_cell_bwd_kernel<3>, 0>(grid, 256, 0, q.s, p);
    });
}
