// Persistent execution of an LSTM stack on gfx950: ONE launch per direction instead of one (forward) or two (backward)
// launches per anti-diagonal (gpe_rnn_wave.hip).  Reference: nn.LSTM under the decoders, /root/reference/nn/net_blocks.py:363-402.
//
// Why: the shipped pattern decoder (32 rows, 2 layers, 23 steps, 250 units) is a chain of 24 dependent diagonals whose
// arithmetic is ~1 us each; as launches they cost 13 us forward and 26 us backward apiece — the time goes into re-reading the
// weight slices from L2 and into kernel boundaries, not into the matrix pipe.
//
// Structure.  Workgroup (layer l, row group rg, unit block nb) owns 16 units of layer l — the 64 gate columns i|f|g|o of those
// units — for the row tiles rt = rg, rg + RG, ... (16 rows each).  Its weight slices (W_hh_l and, above layer 0, W_ih_l:
// 64 KB each at 250 units) are copied into LDS ONCE and stay there for all T steps.  A step of a row tile is
//   wait for the producers' arrival counters -> read the 16 x H state rows straight from global memory into MFMA A fragments
//   (every element is read by exactly one wave: no LDS staging, no barrier) -> 4 waves = 4 K quarters of the gate products ->
//   partial C tiles meet in LDS -> thread (row, unit) applies the cell -> h is PUBLISHED.
// Cells are ordered by data flow, not by a grid barrier: counter (l, t, rt) counts the unit blocks that have published
// h_{l,t} of row tile rt; cell (l, t, rt) waits for (l, t-1, rt) and (l-1, t, rt).  Layer 0 depends on nothing but itself and
// runs ahead; the input-side product of the layers above is issued before the recurrent one, while the recurrent operand is
// still being published.
//
// Inter-workgroup visibility: recipe R1 (gpe_device.h: hand-off), workgroup form — ONE counter increment per workgroup and cell;
// consumers read the payload with sc1 buffer loads.  Co-residency: the host sizes the grid to at most one workgroup per CU (the
// LDS image allows no second one).  Counters are zeroed by a memset node in front of every launch.
//
// The backward kernel mirrors it: workgroup (l, rg, nb) owns dh columns of 16 units; its slices of W_hh_l^T and W_ih_{l+1}^T
// (K = 4H rows x 16 columns) stay in LDS; the exchanged operand is the pre-activation gradient row dG (4H wide, torch gate
// order, written straight into the caller's dgx rows, which the weight-gradient GEMMs read afterwards).
// Arithmetic: exact fp32 MFMA, or f16x3 (gpe_math_set(4)): weights from the caller's fp16 plane packs; the forward state rows
// enter scaled by GPE_STATE_SA (gpe_device.h: |h| < 1, start states < 16); the backward dG fragments are
// normalised PER WAVE by the largest magnitude the wave just loaded (each wave owns its partial accumulator, so the scale is
// undone before the partials meet) — no amax words, no atomics.
#include "gpe_device.h"
#include "gpe_rnn_seq.h"

#define PS_MAXL 4
#define PS_LDC 68                 // forward C tile pitch (64 gate columns + 4)
#define PS_LDB 20                 // backward C tile pitch (16 units + 4)
struct PsFwdParams {
    int L, T, Bn, H, NB, RG, NRT;
    const float* xproj0; long xp0_sb, xp0_st;
    const void* w0[PS_MAXL];                 // W_hh_l: gate-interleaved pack (fp32 [K/4][Npad][4]) or its fp16 plane pack
    const void* w1[PS_MAXL];                 // W_ih_l, layers > 0
    const unsigned* s0[PS_MAXL]; const unsigned* s1[PS_MAXL];        // amax words of the plane packs
    const float* bias[PS_MAXL];              // b_ih + b_hh of layers > 0
    float* hs; long hs_sl, hs_sb, hs_st;
    float* cs; long cs_sl, cs_st;
    float* saved; long sv_sl, sv_st;
    unsigned* flags;                         // [L][T][NRT] arrival counters
    unsigned long long* trace;               // measurement aid (gpe_debug_set 8192): [grid][T][8] wall-clock stamps of lane 0, else NULL
};

struct PsBwdParams {
    int L, T, Bn, H, NB, RG, NRT, KP;        // KP: padded K (= 4H) extent of the transposed packs
    const float* dtop; long dt_sb, dt_st;
    const float* d_hN; const float* d_cN;
    const void* w0[PS_MAXL];                 // W_hh_l^T: plain transposed pack or transposed plane pack
    const void* w1[PS_MAXL];                 // W_ih_{l+1}^T for layer l < L-1
    const unsigned* s0[PS_MAXL]; const unsigned* s1[PS_MAXL];
    const float* cs; long cs_sl, cs_st;
    const float* saved; long sv_sl, sv_st;
    float* dgx; long dg_sl, dg_sb, dg_st;
    float* carry;                            // [2][L][Bn][H]
    unsigned* flags;                         // [L][T][NRT]
    unsigned long long* trace;
};

// phase stamp of the step timeline (100 MHz wall clock): [workgroup][step][8], written by lane 0 of wave 0 when tracing is on
#define PS_STAMP(i)                                                                                         \
    do {                                                                                                    \
        if (p.trace && tid == 0) p.trace[((long)blockIdx.x * T + t) * 8 + (i)] = wall_clock64();            \
    } while (0)

// zero the elements of a loaded quad whose k index is past the operand's K extent (what follows a row in memory is another row)
__device__ __forceinline__ gpe_u32x4 ps_mask4(gpe_u32x4 v, int k0, int K)
{
    v[0] = (k0 < K) ? v[0] : 0u; v[1] = (k0 + 1 < K) ? v[1] : 0u;
    v[2] = (k0 + 2 < K) ? v[2] : 0u; v[3] = (k0 + 3 < K) ? v[3] : 0u;
    return v;
}

// One K segment of a 16-row tile, in two phases so that the loads of two segments can be in flight together:
//   ps_load: A = rows [arow][K] behind `rs` (sc1 loads, row pitch `pitch` floats) -> this wave's share of the K steps, in registers;
//   ps_mma : B = the workgroup's weight slice in LDS with NT 16-column tiles; multiplies the loaded steps into acc.
// sA: power of two applied to A before the fp16 split (H3); DYN: take it from the largest magnitude this wave loaded instead and
// return its inverse.
//   H3 slice layout  [plane][KP / 8][16 NT columns][8 halves]   step = 32 k, two quads per lane
//   fp32 slice layout [KP / 4][16 NT columns][4 floats]          step = 16 k, one quad per lane
template <bool H3, int MAXS>
struct PsA { gpe_u32x4 v[H3 ? 2 * MAXS : MAXS]; };

template <bool H3, int MAXS>
__device__ __forceinline__ void ps_load(PsA<H3, MAXS>& A, __amdgpu_buffer_rsrc_t rs, int arow, long pitch, int K, int s_lo, int nsteps)
{
    const int g = (threadIdx.x & 63) >> 4;
    const int rowoff = (int)(arow * pitch) * 4;
#pragma unroll
    for (int i = 0; i < MAXS; ++i) {
        const int s = (s_lo + i < nsteps) ? s_lo + i : nsteps - 1;
        if constexpr (H3) {
            const int k0 = 32 * s + 8 * g;
            A.v[2 * i] = ps_mask4(__builtin_amdgcn_raw_buffer_load_b128(rs, rowoff + k0 * 4, 0, 16), k0, K);
            A.v[2 * i + 1] = ps_mask4(__builtin_amdgcn_raw_buffer_load_b128(rs, rowoff + k0 * 4 + 16, 0, 16), k0 + 4, K);
        } else {
            const int k0 = 16 * s + 4 * g;
            A.v[i] = ps_mask4(__builtin_amdgcn_raw_buffer_load_b128(rs, rowoff + k0 * 4, 0, 16), k0, K);
        }
    }
}

template <bool H3, int NT, int MAXS, bool DYN>
__device__ __forceinline__ float ps_mma(const PsA<H3, MAXS>& A, int KP, const char* W, int s_lo, int s_hi, float sA, f32x4 (&acc)[NT])
{
    const int lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4;
    float inv = 1.f;
    if constexpr (H3) {
        if constexpr (DYN) {
            unsigned m = 0u;
#pragma unroll
            for (int i = 0; i < 2 * MAXS; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) { const unsigned a = A.v[i][e] & 0x7fffffffu; m = m > a ? m : a; }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)m, o); m = m > t ? m : t; }
            gpe_h3_scale_of(m, sA, inv);
        }
        const int plane_b = KP * 32 * NT;                        // bytes per plane: (KP / 8) groups x 16 NT columns x 16
#pragma unroll
        for (int i = 0; i < MAXS; ++i) {
            const int s = s_lo + i;
            if (s < s_hi) {
                gpe_u32x4 ah, al;
                const gpe_u32x4 a0 = A.v[2 * i], a1 = A.v[2 * i + 1];
                { unsigned h, l; gpe_split2_f16(__uint_as_float(a0[0]), __uint_as_float(a0[1]), sA, h, l); ah[0] = h; al[0] = l; }
                { unsigned h, l; gpe_split2_f16(__uint_as_float(a0[2]), __uint_as_float(a0[3]), sA, h, l); ah[1] = h; al[1] = l; }
                { unsigned h, l; gpe_split2_f16(__uint_as_float(a1[0]), __uint_as_float(a1[1]), sA, h, l); ah[2] = h; al[2] = l; }
                { unsigned h, l; gpe_split2_f16(__uint_as_float(a1[2]), __uint_as_float(a1[3]), sA, h, l); ah[3] = h; al[3] = l; }
                const char* wb = W + ((4 * s + g) * 16 * NT + j) * 16;
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const gpe_u32x4 bh = *reinterpret_cast<const gpe_u32x4*>(wb + 256 * n);
                    const gpe_u32x4 bl = *reinterpret_cast<const gpe_u32x4*>(wb + 256 * n + plane_b);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(gpe_f16x8, al), __builtin_bit_cast(gpe_f16x8, bh), acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(gpe_f16x8, ah), __builtin_bit_cast(gpe_f16x8, bl), acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(gpe_f16x8, ah), __builtin_bit_cast(gpe_f16x8, bh), acc[n], 0, 0, 0);
                }
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < MAXS; ++i) {
            const int s = s_lo + i;
            if (s < s_hi) {
                const char* wb = W + ((4 * s + g) * 16 * NT + j) * 16;
                float4 b4[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) b4[n] = *reinterpret_cast<const float4*>(wb + 256 * n);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const float bv = (t == 0) ? b4[n].x : (t == 1) ? b4[n].y : (t == 2) ? b4[n].z : b4[n].w;
                        acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(A.v[i][t]), bv, acc[n], 0, 0, 0);
                    }
            }
        }
    }
    return inv;
}

// =====================================================================================================================
// forward
// =====================================================================================================================
template <bool H3>
__global__ __launch_bounds__(256) void gpe_rnn_persist_fwd_kernel(PsFwdParams p)
{
    extern __shared__ __align__(16) char ps_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    int bid = blockIdx.x;
    const int nb = bid % p.NB; bid /= p.NB;
    const int rg = bid % p.RG;
    const int l = bid / p.RG;
    const int H = p.H, T = p.T, Bn = p.Bn;
    const int KP = H3 ? ((H + 31) & ~31) : ((H + 15) & ~15);
    const int wbytes = KP * 256;                     // one slice: 64 columns x KP x 4 bytes in either layout
    char* W0 = ps_smem;
    char* W1 = ps_smem + wbytes;
    float* Cs = reinterpret_cast<float*>(ps_smem + (p.L > 1 ? 2 : 1) * wbytes);       // [4 waves][16][PS_LDC]

    gpe_fill<64, 256>(W0, p.w0[l], KP >> 2, 64 * p.NB, 64 * nb);
    if (l > 0) gpe_fill<64, 256>(W1, p.w1[l], KP >> 2, 64 * p.NB, 64 * nb);
    float inv0 = 1.f, inv1 = 1.f;
    if constexpr (H3) {
        float sw;
        gpe_h3_scale_of(p.s0[l][0], sw, inv0); inv0 *= GPE_STATE_INV_SA;
        if (l > 0) { gpe_h3_scale_of(p.s1[l][0], sw, inv1); inv1 *= GPE_STATE_INV_SA; }
    }
    __syncthreads();

    const int er = tid >> 4, eu = tid & 15;
    const int unit = 16 * nb + eu;
    const bool uok = unit < H;
    const int unitc = uok ? unit : H - 1;
    float bi = 0.f, bf = 0.f, bg = 0.f, bo = 0.f;
    if (l > 0) { const float* b = p.bias[l]; bi = b[unitc]; bf = b[H + unitc]; bg = b[2 * H + unitc]; bo = b[3 * H + unitc]; }

    constexpr int MAXS = H3 ? 2 : 4;                 // H <= 256: 8 steps of 32 / 16 steps of 16 over four waves
    const int nsteps = H3 ? (KP >> 5) : (KP >> 4);
    const int spw = (nsteps + 3) >> 2;
    const int s_lo = wave * spw;
    const int s_hi = (s_lo + spw < nsteps) ? s_lo + spw : nsteps;
    const unsigned need = (unsigned)p.NB;
    const unsigned nrec = (unsigned)((((long)Bn - 1) * p.hs_sb + ((H + 3) & ~3)) * 4);

    for (int t = 0; t < T; ++t) {
        for (int rt = rg; rt < p.NRT; rt += p.RG) {
            const int row = 16 * rt + er;
            const bool rok = row < Bn;
            const int rowc = rok ? row : Bn - 1;
            // epilogue operands first: their latency hides under the waits and the products
            float e0 = bi, e1 = bf, e2 = bg, e3 = bo;
            if (l == 0) {
                const float* xp = p.xproj0 + (long)rowc * p.xp0_sb + (long)t * p.xp0_st;
                e0 = xp[unitc]; e1 = xp[H + unitc]; e2 = xp[2 * H + unitc]; e3 = xp[3 * H + unitc];
            }
            const float cprev = p.cs[l * p.cs_sl + (long)t * p.cs_st + (long)rowc * H + unitc];

            PS_STAMP(0);
            const int arow = (16 * rt + j < Bn) ? 16 * rt + j : Bn - 1;
            f32x4 accH[4], accX[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) { accH[n] = (f32x4){0.f, 0.f, 0.f, 0.f}; accX[n] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
            // both flags first, then the loads of both segments back to back (one latency instead of two), then the products
            PsA<H3, MAXS> A1, A0;
            if (l > 0) gpe_flag_wait(p.flags + ((long)(l - 1) * T + t) * p.NRT + rt, need);   // h_{l-1,t}: the layer below runs ahead
            PS_STAMP(1);
            if (t > 0) gpe_flag_wait(p.flags + ((long)l * T + t - 1) * p.NRT + rt, need);     // h_{l,t-1}
            PS_STAMP(3);
            if (l > 0)                               // h_{l-1,t} (slot t+1) x W_ih_l
                ps_load<H3, MAXS>(A1, __builtin_amdgcn_make_buffer_rsrc(p.hs + (l - 1) * p.hs_sl + (long)(t + 1) * p.hs_st, 0, nrec, 0x00020000),
                                  arow, p.hs_sb, H, s_lo, nsteps);
            ps_load<H3, MAXS>(A0, __builtin_amdgcn_make_buffer_rsrc(p.hs + l * p.hs_sl + (long)t * p.hs_st, 0, nrec, 0x00020000),
                              arow, p.hs_sb, H, s_lo, nsteps);                           // h_{l,t-1} (slot t) x W_hh_l
            if (l > 0) ps_mma<H3, 4, MAXS, false>(A1, KP, W1, s_lo, s_hi, GPE_STATE_SA, accX);
            PS_STAMP(2);
            ps_mma<H3, 4, MAXS, false>(A0, KP, W0, s_lo, s_hi, GPE_STATE_SA, accH);
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    Cs[(wave * 16 + 4 * g + r) * PS_LDC + 16 * n + j] = H3 ? accH[n][r] * inv0 + accX[n][r] * inv1 : accH[n][r] + accX[n][r];
            PS_STAMP(4);
            __syncthreads();
            float z[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                z[q] = (Cs[er * PS_LDC + 16 * q + eu] + Cs[(16 + er) * PS_LDC + 16 * q + eu]) +
                       (Cs[(32 + er) * PS_LDC + 16 * q + eu] + Cs[(48 + er) * PS_LDC + 16 * q + eu]);
            if (rok && uok) {
                float ig, fg, gg, og, cn;
                gpe_lstm_cell_fwd(z[0], e0, z[1], e1, z[2], e2, z[3], e3, cprev, ig, fg, gg, og, cn);
                float* go = p.saved + l * p.sv_sl + (long)t * p.sv_st + (long)row * 4 * H;
                go[unit] = ig; go[H + unit] = fg; go[2 * H + unit] = gg; go[3 * H + unit] = og;
                p.cs[l * p.cs_sl + (long)(t + 1) * p.cs_st + (long)row * H + unit] = cn;
                __hip_atomic_store(p.hs + l * p.hs_sl + (long)row * p.hs_sb + (long)(t + 1) * p.hs_st + unit, gpe_lstm_cell_h(og, cn),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            PS_STAMP(5);
            gpe_flag_arrive_wg(p.flags + ((long)l * T + t) * p.NRT + rt,        // (its barrier also frees Cs for the next tile)
                      p.trace ? p.trace + ((long)blockIdx.x * T + t) * 8 + 6 : nullptr);
            PS_STAMP(7);
        }
    }
}

// =====================================================================================================================
// backward
// =====================================================================================================================
template <bool H3>
__global__ __launch_bounds__(256) void gpe_rnn_persist_bwd_kernel(PsBwdParams p)
{
    extern __shared__ __align__(16) char ps_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    int bid = blockIdx.x;
    const int nb = bid % p.NB; bid /= p.NB;
    const int rg = bid % p.RG;
    const int l = bid / p.RG;
    const int H = p.H, T = p.T, Bn = p.Bn, L = p.L, KP = p.KP, K4 = 4 * H;
    const long BH = (long)Bn * H;
    const int wbytes = KP * 64;                      // 16 columns x KP x 4 bytes
    char* W0 = ps_smem;
    char* W1 = ps_smem + wbytes;
    float* Cs = reinterpret_cast<float*>(ps_smem + (L > 1 ? 2 : 1) * wbytes);         // [4 waves][16][PS_LDB]
    const bool up = l < L - 1;                       // a layer above feeds dG_{l+1,t} x W_ih_{l+1}

    gpe_fill<16, 256>(W0, p.w0[l], KP >> 2, 16 * p.NB, 16 * nb);
    if (up) gpe_fill<16, 256>(W1, p.w1[l], KP >> 2, 16 * p.NB, 16 * nb);
    float invw0 = 1.f, invw1 = 1.f;
    if constexpr (H3) {
        float sw;
        gpe_h3_scale_of(p.s0[l][0], sw, invw0);
        if (up) gpe_h3_scale_of(p.s1[l][0], sw, invw1);
    }
    __syncthreads();

    const int er = tid >> 4, eu = tid & 15;
    const int unit = 16 * nb + eu;
    const bool uok = unit < H;
    const int unitc = uok ? unit : H - 1;
    constexpr int MAXS = H3 ? 8 : 16;                // KP <= 1024: 32 steps of 32 / 64 steps of 16 over four waves
    const int nsteps = H3 ? (KP >> 5) : (KP >> 4);
    const int spw = (nsteps + 3) >> 2;
    const int s_lo = wave * spw;
    const int s_hi = (s_lo + spw < nsteps) ? s_lo + spw : nsteps;
    const unsigned need = (unsigned)p.NB;
    const unsigned nrec = (unsigned)((((long)Bn - 1) * p.dg_sb + ((K4 + 3) & ~3)) * 4);

    for (int t = T - 1; t >= 0; --t) {
        for (int rt = rg; rt < p.NRT; rt += p.RG) {
            const int row = 16 * rt + er;
            const bool rok = row < Bn;
            const int rowc = rok ? row : Bn - 1;
            // pointwise operands first
            const long e = (long)rowc * H + unitc;
            float dh = 0.f;
            if (l == L - 1 && p.dtop) dh = p.dtop[(long)rowc * p.dt_sb + (long)t * p.dt_st + unitc];
            if (t == T - 1 && p.d_hN) dh += p.d_hN[(long)l * BH + e];
            float cin = 0.f;
            if (t == T - 1) { if (p.d_cN) cin = p.d_cN[(long)l * BH + e]; }
            else cin = p.carry[((long)((t + 1) & 1) * L + l) * BH + e];
            const float* sv = p.saved + l * p.sv_sl + (long)t * p.sv_st + (long)rowc * 4 * H;
            const float ig = sv[unitc], fg = sv[H + unitc], gg = sv[2 * H + unitc], og = sv[3 * H + unitc];
            const float ct = p.cs[l * p.cs_sl + (long)(t + 1) * p.cs_st + e];
            const float cp = p.cs[l * p.cs_sl + (long)t * p.cs_st + e];

            PS_STAMP(0);
            const int arow = (16 * rt + j < Bn) ? 16 * rt + j : Bn - 1;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            // both flags first, then the loads of both segments back to back (one latency instead of two), then the products
            PsA<H3, MAXS> A1, A0;
            const bool rec = t < T - 1;
            if (up) gpe_flag_wait(p.flags + ((long)(l + 1) * T + t) * p.NRT + rt, need);       // dG_{l+1,t}: the layer above runs ahead
            PS_STAMP(1);
            if (rec) gpe_flag_wait(p.flags + ((long)l * T + t + 1) * p.NRT + rt, need);        // dG_{l,t+1}
            PS_STAMP(3);
            if (up)                                  // dG_{l+1,t} x W_ih_{l+1}
                ps_load<H3, MAXS>(A1, __builtin_amdgcn_make_buffer_rsrc(p.dgx + (l + 1) * p.dg_sl + (long)t * p.dg_st, 0, nrec, 0x00020000),
                                  arow, p.dg_sb, K4, s_lo, nsteps);
            if (rec)                                 // dG_{l,t+1} x W_hh_l
                ps_load<H3, MAXS>(A0, __builtin_amdgcn_make_buffer_rsrc(p.dgx + l * p.dg_sl + (long)(t + 1) * p.dg_st, 0, nrec, 0x00020000),
                                  arow, p.dg_sb, K4, s_lo, nsteps);
            if (up) {
                f32x4 a1[1] = {{0.f, 0.f, 0.f, 0.f}};
                const float ia = ps_mma<H3, 1, MAXS, true>(A1, KP, W1, s_lo, s_hi, 1.f, a1);
                acc = a1[0] * (ia * invw1);
            }
            PS_STAMP(2);
            if (rec) {
                f32x4 a0[1] = {{0.f, 0.f, 0.f, 0.f}};
                const float ia = ps_mma<H3, 1, MAXS, true>(A0, KP, W0, s_lo, s_hi, 1.f, a0);
                acc += a0[0] * (ia * invw0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) Cs[(wave * 16 + 4 * g + r) * PS_LDB + j] = acc[r];
            PS_STAMP(4);
            __syncthreads();
            dh += (Cs[er * PS_LDB + eu] + Cs[(16 + er) * PS_LDB + eu]) + (Cs[(32 + er) * PS_LDB + eu] + Cs[(48 + er) * PS_LDB + eu]);
            if (rok && uok) {
                float di, df, dg, dgo, cout;
                gpe_lstm_cell_bwd(ig, fg, gg, og, ct, cp, dh, &cin, di, df, dg, dgo, cout);
                float* gx = p.dgx + l * p.dg_sl + (long)row * p.dg_sb + (long)t * p.dg_st;
                __hip_atomic_store(gx + unit, di, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(gx + H + unit, df, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(gx + 2 * H + unit, dg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(gx + 3 * H + unit, dgo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                p.carry[((long)(t & 1) * L + l) * BH + (long)row * H + unit] = cout;
            }
            PS_STAMP(5);
            gpe_flag_arrive_wg(p.flags + ((long)l * T + t) * p.NRT + rt, p.trace ? p.trace + ((long)blockIdx.x * T + t) * 8 + 6 : nullptr);
            PS_STAMP(7);
        }
    }
}

// =====================================================================================================================
// host side
// =====================================================================================================================
// gpe_debug_set bits (measurement aids): 1024 = never the persistent kernels; 2048 / 4096 = allow them for a stack whose row tiles
// outnumber the row groups the chip can hold (forward / backward: several row tiles per workgroup)
static bool ps_plan(int gates, int L, int T, int Bn, int H, bool bwd, GpeRnnPlan& pl)
{
    if (!gpe_rnn_plan_begin(gates, L, PS_MAXL, T, Bn, H, 1024, pl)) return false;
    pl.RG = pl.rgmax;
    if (pl.RG < pl.NRT && !(gpe_debug_get() & (bwd ? 4096 : 2048))) return false;
    pl.grid = pl.per * pl.RG;
    return true;
}

// [L][T][NRT] arrival counters | trace; zeroed as ONE image in front of every launch
static GpeRnnWs ps_ws_layout(int L, int T, const GpeRnnPlan& pl)
{
    return {(((long)L * T * pl.NRT * 4) + 255) & ~255L, 0, (gpe_debug_get() & 8192) ? (long)pl.grid * T * 8 * 8 : 0};
}

long gpe_rnn_persist_ws_bytes(int gates, int L, int T, int Bn, int H, int bwd)
{
    GpeRnnPlan pl;
    if (!ps_plan(gates, L, T, Bn, H, bwd != 0, pl)) return 0;
    return ps_ws_layout(L, T, pl).total();
}

// plan step of the forward: every check, the plan, the LDS image and the parameter struct (pointers are copied, never followed)
static bool ps_fwd_plan(const GpeRnnSeq& q, PsFwdParams& p, GpeRnnPlan& pl, GpeRnnWs& lay, size_t& lds)
{
    if (!ps_plan(q.G, q.L, q.T, q.Bn, q.H, false, pl)) return false;
    lay = ps_ws_layout(q.L, q.T, pl);
    if (!lay.fits(q.ws, q.ws_bytes, 8)) return false;
    if ((long)q.Bn * q.hs_sb * 4 >= (1L << 31) || (q.hs_sb & 3) || (q.hs_st & 3) || (((uintptr_t)q.hs) & 15)) return false;
    pl.KP = q.f16 ? gpe_round_up(q.H, 32) : gpe_round_up(q.H, 16);
    lds = (size_t)(q.L > 1 ? 2 : 1) * pl.KP * 256 + 4 * 16 * PS_LDC * 4;
    if (lds > GPE_RNN_LDS_CAP) return false;
    if (!gpe_rnn_fill_fwd(p, q, pl)) return false;
    p.flags = (unsigned*)q.ws; p.trace = lay.trace_at(q.ws);
    return true;
}

int gpe_rnn_persist_fwd(const GpeRnnSeq& q, GpeRnnPath* plan_only)
{
    GpeRnnPlan pl;
    GpeRnnWs lay;
    size_t lds;
    PsFwdParams p = {};
    if (!ps_fwd_plan(q, p, pl, lay, lds)) return GPE_RNN_NOT_MINE;
    if (plan_only) { plan_only->persistent(pl, q.f16, pl.KP, lds, lay.total()); return GPE_RNN_LAUNCHED; }
    if (hipMemsetAsync(q.ws, 0, (size_t)lay.total(), q.s) != hipSuccess) return GPE_ELAUNCH;
    return gpe_rnn_for_bool(q.f16, [&](auto h3) {
        return gpe_rnn_launch<gpe_rnn_persist_fwd_kernel<decltype(h3)::value>, GPE_RNN_LDS_CAP>(dim3(pl.grid), 256, lds, q.s, p);
    });
}

// ... and of the backward
static bool ps_bwd_plan(const GpeRnnSeqBwd& q, PsBwdParams& p, GpeRnnPlan& pl, GpeRnnWs& lay, size_t& lds)
{
    if (!ps_plan(q.G, q.L, q.T, q.Bn, q.H, true, pl)) return false;
    lay = ps_ws_layout(q.L, q.T, pl);
    if (!lay.fits(q.part, lay.total(), 8)) return false;                      // (gpe_rnn_seq_bwd_ws covers this layout)
    if ((long)q.Bn * q.dg_sb * 4 >= (1L << 31) || (q.dg_sb & 3) || (q.dg_st & 3) || (((uintptr_t)q.dgx) & 15) || (q.dg_sl & 3))
        return false;
    // padded K (= 4H) extent of the transposed packs
    const int K = 4 * q.H, KP = q.f16 ? gpe_round_up(K, 32) : (int)(gpe_packed_size(q.H, K) / gpe_round_up(q.H, 16));
    if (KP < K || KP > 1024 || (KP & (q.f16 ? 31 : 15))) return false;
    pl.KP = KP;
    lds = (size_t)(q.L > 1 ? 2 : 1) * KP * 64 + 4 * 16 * PS_LDB * 4;
    if (lds > GPE_RNN_LDS_CAP) return false;
    p.L = q.L; p.T = q.T; p.Bn = q.Bn; p.H = q.H; p.NB = pl.NB; p.RG = pl.RG; p.NRT = pl.NRT; p.KP = KP;
    p.dtop = q.dtop; p.dt_sb = q.dt_sb; p.dt_st = q.dt_st; p.d_hN = q.d_hN; p.d_cN = q.d_cN;
    if (!gpe_rnn_fill_tables(p, q.L, 1, q.f16 ? q.whh_tpl : q.whh_t, q.f16 ? q.wih_tpl : q.wih_t, q.whh_amax, q.wih_amax, q.f16))
        return false;
    p.cs = q.cs; p.cs_sl = q.cs_sl; p.cs_st = q.cs_st;
    p.saved = q.saved; p.sv_sl = q.sv_sl; p.sv_st = q.sv_st;
    p.dgx = q.dgx; p.dg_sl = q.dg_sl; p.dg_sb = q.dg_sb; p.dg_st = q.dg_st;
    p.carry = q.carry; p.flags = (unsigned*)q.part; p.trace = lay.trace_at(q.part);
    return true;
}

int gpe_rnn_persist_bwd(const GpeRnnSeqBwd& q, GpeRnnPath* plan_only)
{
    GpeRnnPlan pl;
    GpeRnnWs lay;
    size_t lds;
    PsBwdParams p = {};
    if (!ps_bwd_plan(q, p, pl, lay, lds)) return GPE_RNN_NOT_MINE;
    if (plan_only) { plan_only->persistent(pl, q.f16, pl.KP, lds, (lay.total() + 3) / 4); return GPE_RNN_LAUNCHED; }
    if (hipMemsetAsync(q.part, 0, (size_t)lay.total(), q.s) != hipSuccess) return GPE_ELAUNCH;
    return gpe_rnn_for_bool(q.f16, [&](auto h3) {
        return gpe_rnn_launch<gpe_rnn_persist_bwd_kernel<decltype(h3)::value>, GPE_RNN_LDS_CAP>(dim3(pl.grid), 256, lds, q.s, p);
    });
}
