// One DynamicEdgeConv layer at prediction time (nn/net_blocks.py:43-47,124-135,174 under model.eval()), forward only, nothing stored
// per edge.
//
//   eval-mode algebra   every BatchNorm is the affine map (s, t) of its running statistics and folds into the next Linear
//                       (W diag(s), b + W t); the first Linear splits per point, W1 [x_i | x_j - x_i] + b1 = P_i + Q_j; the last
//                       BatchNorm commutes with the aggregation (max: the sign of s picks max or min; mean / add: affine).
//   gpe_edge_predict_fwd  a workgroup owns RP = R / k consecutive global point rows and their RP k edge rows (rows past RP k are zero
//                       padding that the reduction never reads): relu(P_i + Q_j) is formed in LDS, the H -> H layers and the H -> F
//                       layer run as MFMA layers that rewrite the activations in place in LDS (a wave owns its rows x all columns,
//                       accumulators in registers, weights streamed through LDS in 32-row K slabs one slab ahead), the last layer's
//                       relu output goes to LDS, thread (point, channel) reduces over the point's k rows and stores out [B N, F].
//                       Points and neighbour rows use global numbering: a tile may span two clouds, the last tile may be ragged.
//   exact               v_mfma_f32_16x16x4_f32, R = 64, a wave = 16 rows
//   f16x3               three v_mfma_f32_16x16x32_f16 per product on two-term fp16 splits, R = 128, a wave = 32 rows; weights
//                       normalised per layer by the amax word of the folded pack, activations per wave and layer from the wave's
//                       own accumulators, planes in LDS (widths <= 224: the planes of 128 rows beside a slab)
// The slab macros, the plane layout and the per-wave normalisation restate csrc/gpe_stitch_pairs.hip's (the same kernel with another
// row -> operand map and another epilogue); the weight pack is that file's gpe_stitch_pairs_pack / gpe_stitch_pairs_planes output.
// No inter-workgroup communication, no atomics, no spin waits; every loop bound is a kernel argument or a template constant.
#include "gpe_device.h"
#include <math.h>

#define EP_KS 32            // K rows of a weight slab
#define EP_TPB 256
#define EP_R 64             // edge rows per workgroup, exact kernel
#define EP_R3 128           // edge rows per workgroup, f16x3 kernel
#define EP_MAXK 64
#define EP_H3_MAXW 224

// ---- operand layout (documented in include/gpe_hip.h) -------------------------------------------------------------------------------
static inline int ep_nb(int W) { const int nb = (W + 15) / 16; return nb <= 4 ? 4 : (nb <= 8 ? 8 : (nb <= 13 ? 13 : 16)); }
static inline int ep_ldw(int W) { const int np = ep_nb(W) * 16; return (np % 32 == 16) ? np : np + 16; }   // 4 K rows x 16 columns hit 64 banks
static inline int ep_lda(int W) { return (((W + 3) / 4) | 1) * 4; }                                             // 16 rows x 4 k hit 64 banks
template <int NB> struct EpLdw { static constexpr int v = (NB * 16) % 32 == 16 ? NB * 16 : NB * 16 + 16; };

static inline bool ep_menu_ok(int k, int H, int F, int n_hidden)
{
    return k >= 1 && k <= EP_MAXK && H > 0 && H <= 256 && !(H & 3) && F > 0 && F <= 256 && n_hidden >= 0 && n_hidden <= 3;
}

struct EpParams {
    const float* pq; int ldpq;          // [BN][ldpq]: P in columns [0, H), Q in [H, 2H)
    const int32_t* jg;                  // [BN * k] global neighbour rows
    long BN; int k, H, F, nh;
    const float* wpk; const float* planes; const unsigned* w_amax;
    const float* stats;                 // [4][F] of the last BatchNorm: rows 2, 3 = s, t
    int aggr;                           // 0 max, 1 mean, 2 add
    float* out; int ldo;
    int RP, lda, KP;
};

// a 32-row K slab of a layer's weights travels global -> registers (in flight during the previous slab's products) -> LDS
// (named registers, not an array: an indexed array of them ends up in private memory)
#define EP_PRE_DECL float4 pre0 = {}, pre1 = {}, pre2 = {}, pre3 = {}, pre4 = {}, pre5 = {}, pre6 = {}, pre7 = {}, pre8 = {}
#define EP_LD1(i, src, n4) if (NPRE > i) pre##i = reinterpret_cast<const float4*>(src)[min((int)threadIdx.x + i * EP_TPB, (n4) - 1)];
#define EP_ST1(i, dst, n4) if (NPRE > i && (int)threadIdx.x + i * EP_TPB < (n4)) reinterpret_cast<float4*>(dst)[threadIdx.x + i * EP_TPB] = pre##i;
#define EP_SLAB_LOAD(src, n4)  do { EP_LD1(0, src, n4) EP_LD1(1, src, n4) EP_LD1(2, src, n4) EP_LD1(3, src, n4) EP_LD1(4, src, n4) \
                                    EP_LD1(5, src, n4) EP_LD1(6, src, n4) EP_LD1(7, src, n4) EP_LD1(8, src, n4) } while (0)
#define EP_SLAB_STORE(dst, n4) do { EP_ST1(0, dst, n4) EP_ST1(1, dst, n4) EP_ST1(2, dst, n4) EP_ST1(3, dst, n4) EP_ST1(4, dst, n4) \
                                    EP_ST1(5, dst, n4) EP_ST1(6, dst, n4) EP_ST1(7, dst, n4) EP_ST1(8, dst, n4) } while (0)

// the tile's rows: s_nbr[row] = the neighbour's global row (-1 for padding rows and for points past the end), s_pt[row] = the row's
// point in the tile; -> points in the tile
template <int R>
__device__ __forceinline__ int ep_tile_rows(const EpParams& p, long pt0, int* s_nbr, int* s_pt)
{
    const int npts = (int)min((long)p.RP, p.BN - pt0);
    for (int row = threadIdx.x; row < R; row += EP_TPB) {
        int j = -1;
        if (row < npts * p.k) j = (int)min((long)max(p.jg[pt0 * p.k + row], 0), p.BN - 1);
        s_nbr[row] = j;
        s_pt[row] = row / p.k;
    }
    __syncthreads();
    return npts;
}

// thread (point, channel) reduces the point's k rows of z [rows][ldz] (fp32, LDS) and applies the last BatchNorm
__device__ __forceinline__ void ep_reduce_store(const EpParams& p, const float* z, int ldz, long pt0, int npts)
{
    const int F = p.F, k = p.k;
    const float* sv = p.stats + 2 * (long)F;
    const float* tv = p.stats + 3 * (long)F;
    for (int idx = threadIdx.x; idx < npts * F; idx += EP_TPB) {
        const int pt = idx / F, c = idx - pt * F;
        const float* col = z + (long)pt * k * ldz + c;
        float mx = col[0], mn = col[0], sum = col[0];
        for (int j = 1; j < k; ++j) {
            const float v = col[j * ldz];
            mx = fmaxf(mx, v);
            mn = fminf(mn, v);
            sum += v;
        }
        const float s = sv[c], t = tv[c];
        float y;
        if (p.aggr == 0) y = s * (s >= 0.f ? mx : mn) + t;
        else if (p.aggr == 1) y = s * (sum / (float)k) + t;
        else y = s * sum + (float)k * t;
        p.out[(pt0 + pt) * p.ldo + c] = y;
    }
}

// ---- exact fp32 ----------------------------------------------------------------------------------------------------------------------
// acc (preset to the bias) += act [16 rows of the wave][K] . Wt [K][LDW]
template <int NB>
__device__ __forceinline__ void ep_layer_f32(const float* act, int lda, int K, const float* Wt, float* Ws, int row0, int lr, int lq,
                                             f32x4 (&acc)[NB])
{
    constexpr int LDW = EpLdw<NB>::v, NPRE = (EP_KS * LDW / 4 + EP_TPB - 1) / EP_TPB;
    static_assert(NPRE <= 9, "a slab is at most 9 float4 per thread");
    EP_PRE_DECL;
    EP_SLAB_LOAD(Wt, min(EP_KS, K) * LDW / 4);
    for (int k0 = 0; k0 < K; k0 += EP_KS) {
        const int kc = min(EP_KS, K - k0);
        __syncthreads();                    // the activations are written / the previous slab has been read
        EP_SLAB_STORE(Ws, kc * LDW / 4);
        __syncthreads();
        if (k0 + EP_KS < K) EP_SLAB_LOAD(Wt + (long)(k0 + EP_KS) * LDW, min(EP_KS, K - k0 - EP_KS) * LDW / 4);
        for (int ks = 0; ks < kc; ks += 4) {
            const float a = act[(row0 + lr) * lda + k0 + ks + lq];
            const float* wr = Ws + (ks + lq) * LDW + lr;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
                acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wr[nb * 16], acc[nb], 0, 0, 0);
        }
    }
}

template <int NB>
__device__ __forceinline__ void ep_relu_store_f32(float* act, int lda, int W, int row0, int lr, int lq,
                                                  const f32x4 (&acc)[NB])
{
    // a wave rewrites only its own 16 rows, and it has consumed them
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int col = nb * 16 + lr;
        if (col < W) {
#pragma unroll
            for (int r = 0; r < 4; ++r) act[(row0 + lq * 4 + r) * lda + col] = fmaxf(acc[nb][r], 0.f);
        }
    }
}

template <int NBH, int NBF>
__global__ __launch_bounds__(EP_TPB) void gpe_edge_predict_f32_kernel(EpParams p)
{
    constexpr int LDWH = EpLdw<NBH>::v, LDWF = EpLdw<NBF>::v, LDWM = LDWH > LDWF ? LDWH : LDWF;
    extern __shared__ float ep_smem[];
    __shared__ int s_nbr[EP_R], s_pt[EP_R];
    const int tid = threadIdx.x;
    const long pt0 = (long)blockIdx.x * p.RP;
    const int npts = ep_tile_rows<EP_R>(p, pt0, s_nbr, s_pt);
    const int H = p.H, lda = p.lda;
    float* act = ep_smem;                       // [64][lda]
    float* Ws = ep_smem + EP_R * lda;           // [EP_KS][LDWM]
    const int H4 = H >> 2;
    for (int idx = tid; idx < EP_R * H4; idx += EP_TPB) {
        const int row = idx / H4, q = idx - row * H4;
        const int j = s_nbr[row];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j >= 0) {
            const float4 a = *reinterpret_cast<const float4*>(p.pq + (pt0 + s_pt[row]) * p.ldpq + 4 * q);
            const float4 c = *reinterpret_cast<const float4*>(p.pq + (long)j * p.ldpq + H + 4 * q);
            v = make_float4(fmaxf(a.x + c.x, 0.f), fmaxf(a.y + c.y, 0.f), fmaxf(a.z + c.z, 0.f), fmaxf(a.w + c.w, 0.f));
        }
        *reinterpret_cast<float4*>(act + row * lda + 4 * q) = v;
    }
    const int lane = tid & 63, row0 = (tid >> 6) * 16, lr = lane & 15, lq = lane >> 4;
    const float* wl = p.wpk;
    for (int l = 0; l < p.nh; ++l) {
        const float* bias = wl + (long)H * LDWH;
        f32x4 acc[NBH];
#pragma unroll
        for (int nb = 0; nb < NBH; ++nb) {
            const float bz = bias[nb * 16 + lr];
            acc[nb] = f32x4{bz, bz, bz, bz};
        }
        ep_layer_f32<NBH>(act, lda, H, wl, Ws, row0, lr, lq, acc);
        ep_relu_store_f32<NBH>(act, lda, H, row0, lr, lq, acc);
        wl += (long)(H + 1) * LDWH;
    }
    {
        const float* bias = wl + (long)H * LDWF;
        f32x4 acc[NBF];
#pragma unroll
        for (int nb = 0; nb < NBF; ++nb) {
            const float bz = bias[nb * 16 + lr];
            acc[nb] = f32x4{bz, bz, bz, bz};
        }
        ep_layer_f32<NBF>(act, lda, H, wl, Ws, row0, lr, lq, acc);
        ep_relu_store_f32<NBF>(act, lda, p.F, row0, lr, lq, acc);
    }
    __syncthreads();
    ep_reduce_store(p, act, lda, pt0, npts);
}

// ---- f16x3: the fp16 pipe on normalised two-term splits, fp32 accumulate ------------------------------------------------------------
// x 2^sh = h + l (two fp16 terms), a product = three v_mfma_f32_16x16x32_f16 (small terms first).  Weights: one power of two per
// layer from the largest magnitude of the folded pack (amax word), planes in B-fragment order (gpe_stitch_pairs_planes).
// Activations: one power of two per WAVE (its 32 rows) and layer, from the maximum the wave finds in its own accumulators; the planes
// of the activations live in LDS and are rewritten in place.
__device__ __forceinline__ float ep_wave_max(float m)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    return m;
}

// acc (zero) += planes of the wave's 32 rows [KP] . planes of Wt [KP][LDW]
template <int NB>
__device__ __forceinline__ void ep_layer_h3(const _Float16* hiP, const _Float16* loP, int ldh, int KP, const float* pl, float* Ws,
                                            int row0, int lr, int lq, f32x4 (&acc)[2][NB])
{
    constexpr int LDW = EpLdw<NB>::v, NPRE = (EP_KS * LDW / 4 + EP_TPB - 1) / EP_TPB, N4 = EP_KS * LDW / 4;
    static_assert(NPRE <= 9, "a slab is at most 9 float4 per thread");
    EP_PRE_DECL;
    EP_SLAB_LOAD(pl, N4);
    for (int k0 = 0; k0 < KP; k0 += 32) {
        __syncthreads();                    // the previous slab has been read by every wave
        EP_SLAB_STORE(Ws, N4);
        __syncthreads();
        if (k0 + 32 < KP) EP_SLAB_LOAD(pl + (long)(k0 + 32) * LDW, N4);
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
}

template <int NBH, int NBF>
__global__ __launch_bounds__(EP_TPB) void gpe_edge_predict_h3_kernel(EpParams p)
{
    constexpr int LDWH = EpLdw<NBH>::v, LDWF = EpLdw<NBF>::v;
    extern __shared__ float ep_smem[];
    __shared__ int s_nbr[EP_R3], s_pt[EP_R3];
    const int tid = threadIdx.x;
    const long pt0 = (long)blockIdx.x * p.RP;
    const int npts = ep_tile_rows<EP_R3>(p, pt0, s_nbr, s_pt);
    const int H = p.H, F = p.F, KP = p.KP, ldh = KP + 8;
    _Float16* hiP = reinterpret_cast<_Float16*>(ep_smem);          // [128][ldh]
    _Float16* loP = hiP + EP_R3 * ldh;
    float* Ws = ep_smem + EP_R3 * ldh;                              // hi [4][LDW][8 halves], lo alike
    const int H4 = H >> 2;
    const int lane = tid & 63, row0 = (tid >> 6) * 32, lr = lane & 15, lq = lane >> 4;
    // a0 = relu(P_i + Q_j) of this wave's 32 rows: a pass for the maximum, a pass that stores the split
    float sa = 1.f, inv_a = 1.f;
    for (int pass = 0; pass < 2; ++pass) {
        float m = 0.f;
        for (int idx = lane; idx < 32 * H4; idx += 64) {
            const int r = idx / H4, q = idx - r * H4, row = row0 + r;
            const int j = s_nbr[row];
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j >= 0) {
                const float4 a = *reinterpret_cast<const float4*>(p.pq + (pt0 + s_pt[row]) * p.ldpq + 4 * q);
                const float4 c = *reinterpret_cast<const float4*>(p.pq + (long)j * p.ldpq + H + 4 * q);
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
        if (pass == 0) gpe_h3_scale_of(__float_as_uint(ep_wave_max(m)), sa, inv_a);
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
    const float* pl = p.planes;
    for (int l = 0; l < p.nh; ++l) {
        const float* bias = wl + (long)H * LDWH;
        float sw, inv_w;
        gpe_h3_scale_of(p.w_amax[l], sw, inv_w);
        f32x4 acc[2][NBH];
#pragma unroll
        for (int nb = 0; nb < NBH; ++nb) { acc[0][nb] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[1][nb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        ep_layer_h3<NBH>(hiP, loP, ldh, KP, pl, Ws, row0, lr, lq, acc);
        // a = relu(acc / (scales) + bias); its maximum gives the wave's next scale; the wave rewrites its own rows of the planes
        const float un = inv_a * inv_w;
        float m = 0.f;
#pragma unroll
        for (int nb = 0; nb < NBH; ++nb) {
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
        gpe_h3_scale_of(__float_as_uint(ep_wave_max(m)), sa, inv_a);
#pragma unroll
        for (int nb = 0; nb < NBH; ++nb) {
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
        wl += (long)(H + 1) * LDWH;
        pl += (long)KP * LDWH;
    }
    {
        // H -> F: the relu output goes to LDS in fp32, over the planes and the slab once every wave is done with them
        const float* bias = wl + (long)H * LDWF;
        float sw, inv_w;
        gpe_h3_scale_of(p.w_amax[p.nh], sw, inv_w);
        f32x4 acc[2][NBF];
#pragma unroll
        for (int nb = 0; nb < NBF; ++nb) { acc[0][nb] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[1][nb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        ep_layer_h3<NBF>(hiP, loP, ldh, KP, pl, Ws, row0, lr, lq, acc);
        const float un = inv_a * inv_w;
        __syncthreads();
        float* z = ep_smem;                     // [128][lda]
        const int ldz = p.lda;
#pragma unroll
        for (int nb = 0; nb < NBF; ++nb) {
            const int col = nb * 16 + lr;
            if (col < F) {
                const float bz = bias[col];
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        z[(row0 + 16 * mb + lq * 4 + r) * ldz + col] = fmaxf(fmaf(acc[mb][nb][r], un, bz), 0.f);
            }
        }
        __syncthreads();
        ep_reduce_store(p, z, ldz, pt0, npts);
    }
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------------
static inline size_t ep_lds_f32(int H, int F)
{
    return (size_t)(EP_R * ep_lda(max(H, F)) + EP_KS * max(ep_ldw(H), ep_ldw(F))) * sizeof(float);
}
static inline size_t ep_lds_h3(int H, int F)
{
    const int KP = (H + 31) & ~31;
    const size_t gemm = (size_t)(EP_R3 * (KP + 8) + EP_KS * max(ep_ldw(H), ep_ldw(F))) * sizeof(float);
    const size_t red = (size_t)EP_R3 * ep_lda(F) * sizeof(float);
    return gemm > red ? gemm : red;
}

template <int NBH, int NBF>
static int ep_launch(const EpParams& p, bool h3, hipStream_t s)
{
    if (h3) {
        const size_t lds = ep_lds_h3(p.H, p.F);
        GPE_ENSURE_MAX_LDS_N((gpe_edge_predict_h3_kernel<NBH, NBF>), 158 * 1024);
        hipLaunchKernelGGL((gpe_edge_predict_h3_kernel<NBH, NBF>), dim3(gpe_cdiv(p.BN, p.RP)), dim3(EP_TPB), lds, s, p);
    } else {
        const size_t lds = ep_lds_f32(p.H, p.F);
        GPE_ENSURE_MAX_LDS_N((gpe_edge_predict_f32_kernel<NBH, NBF>), 150 * 1024);
        hipLaunchKernelGGL((gpe_edge_predict_f32_kernel<NBH, NBF>), dim3(gpe_cdiv(p.BN, p.RP)), dim3(EP_TPB), lds, s, p);
    }
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

template <int NBH>
static int ep_dispatch_f(const EpParams& p, bool h3, hipStream_t s)
{
    switch (ep_nb(p.F)) {
    case 4: return ep_launch<NBH, 4>(p, h3, s);
    case 8: return ep_launch<NBH, 8>(p, h3, s);
    case 13: return ep_launch<NBH, 13>(p, h3, s);
    default: return ep_launch<NBH, 16>(p, h3, s);
    }
}

static int ep_dispatch(const EpParams& p, bool h3, hipStream_t s)
{
    switch (ep_nb(p.H)) {
    case 4: return ep_dispatch_f<4>(p, h3, s);
    case 8: return ep_dispatch_f<8>(p, h3, s);
    case 13: return ep_dispatch_f<13>(p, h3, s);
    default: return ep_dispatch_f<16>(p, h3, s);
    }
}

extern "C" int gpe_edge_predict_ok(int k, int H, int F, int n_hidden, void* stream)
{
    (void)stream;
    return ep_menu_ok(k, H, F, n_hidden) ? 1 : 0;
}

extern "C" int gpe_edge_predict_fwd(const float* pq, int ldpq, const int32_t* jg, long BN, int k, int H, int F, int n_hidden,
                                    const float* wpk, const void* planes, const uint32_t* w_amax, const float* last_stats, int aggr,
                                    float* out, int ldo, void* stream)
{
    if (!ep_menu_ok(k, H, F, n_hidden)) return GPE_EINVAL;
    if (!pq || !jg || !wpk || !last_stats || !out || BN <= 0 || BN * k >= (1L << 31) || aggr < 0 || aggr > 2) return GPE_EINVAL;
    if (ldpq < 2 * H || (ldpq & 3) || ldo < F) return GPE_EINVAL;
    if ((((uintptr_t)pq) | ((uintptr_t)wpk) | ((uintptr_t)planes)) & 15) return GPE_EINVAL;
    // f16x3: planes given, the activation planes of 128 rows fit beside a slab (widths <= 224), and the call is past the mode's size gate
    const bool h3 = planes && w_amax && gpe_math_get() == 4 && H <= EP_H3_MAXW && F <= EP_H3_MAXW && BN * k >= gpe_h3_min_rows();
    EpParams p{pq, ldpq, jg, BN, k, H, F, n_hidden, wpk, static_cast<const float*>(planes), w_amax, last_stats, aggr, out, ldo,
               (h3 ? EP_R3 : EP_R) / k, h3 ? ep_lda(F) : ep_lda(max(H, F)), (H + 31) & ~31};
    return ep_dispatch(p, h3, (hipStream_t)stream);
}
