// Bandwidth-bound kernels of the path for gfx950: weight packing / BatchNorm folding.
//   * weight packing: plain and transposed packs, and the multi-pack that refreshes every weight-derived operand of a model
//     (plain / transposed / gate-interleaved packs, the P|Q split of the first edge-MLP Linear, b_ih + b_hh) in ONE launch
//   * gate-interleaved packing of the LSTM / GRU weights
//   * what a forward block of the edge MLP needs from the BatchNorm in front of it (gpe_pack_fold), and gpe_fold_bias
// Reference lines each one replaces are listed in include/gpe_hip.h.
#include "gpe_device.h"
#include <math.h>

// ---------------------------------------------------------------------------------------------------------
// weight packing: packed[(kc*4 + plane)*Npad*4 + n*4 + t] = w(n, 16*kc + 4*plane + t) * col_scale
// ---------------------------------------------------------------------------------------------------------
// K extent of a packed weight: whole 16-k chunks, and a K in (96, 208] is filled up (with zeros) to the 10 or 13 chunks the
// register-stationary edge kernels keep resident — they load their full chunk count whatever the real K is.
static int gpe_pack_kpad(int K)
{
    const int k16 = gpe_round_up(K, 16);
    return (k16 > 96 && k16 < 160) ? 160 : (k16 > 160 && k16 < 208) ? 208 : k16;
}
extern "C" long gpe_packed_size(int N, int K) { return (long)gpe_round_up(N, 16) * gpe_pack_kpad(K); }

__global__ void gpe_pack_kernel(const float* __restrict__ w, int ldw, int N, int K, int transpose,
                                const float* __restrict__ col_scale, float* __restrict__ wp, int Npad, long total)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int t = (int)(e & 3);
    const long r = e >> 2;
    const int n = (int)(r % Npad);
    const long kq = r / Npad;                 // = kc*4 + plane
    const int k = (int)(kq * 4 + t);
    float v = 0.f;
    if (n < N && k < K) {
        v = transpose ? w[(size_t)k * ldw + n] : w[(size_t)n * ldw + k];
        if (col_scale) v *= col_scale[k];
    }
    wp[e] = v;
}

extern "C" int gpe_pack_weight(const float* w, int ldw, int N, int K, int transpose, const float* col_scale,
                               float* wp, void* stream)
{
    if (!w || !wp || N <= 0 || K <= 0 || ldw < (transpose ? N : K)) return GPE_EINVAL;
    const int Npad = gpe_round_up(N, 16);
    const long total = (long)Npad * gpe_pack_kpad(K);
    hipLaunchKernelGGL(gpe_pack_kernel, dim3(gpe_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w, ldw, N, K,
                       transpose, col_scale, wp, Npad, total);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// ---------------------------------------------------------------------------------------------------------
// multi-pack: every weight-derived operand of a model (plain / transposed / gate-interleaved packs, the P|Q split of
// the first edge-MLP Linear, b_ih + b_hh) refreshed by ONE launch after an optimizer step, instead of ~45 launches
// per training step.  Job table in device memory, 64 bytes per job (mirrored by ops.PackPlan):
// ---------------------------------------------------------------------------------------------------------
struct GpePackJob {
    const float* w;         // source matrix / vector
    const float* w2;        // second source (kind 5)
    float* out;
    long total;             // output elements
    long first_block;       // first 256-thread block of this job
    int ldw, N, K, kind, Npad, aux;
};
static_assert(sizeof(GpePackJob) == 64, "job layout is part of the ABI (ops.PackPlan builds it with numpy)");

// one thread = one output quad (4 consecutive elements: the 4 k values of one packed float4); a block covers 1024 elements
__device__ __forceinline__ float gpe_pack_elem(const GpePackJob& jb, int n, int k)
{
    const float* w = jb.w;
    const int ldw = jb.ldw;
    switch (jb.kind) {
        case 0: return (n < jb.N && k < jb.K) ? w[(size_t)n * ldw + k] : 0.f;
        case 1: return (n < jb.N && k < jb.K) ? w[(size_t)k * ldw + n] : 0.f;
        case 2: {                                                   // gate-interleaved (LSTM G = 4, GRU G = 3), aux = H
            const int H = jb.aux, G = jb.N / H;
            const int b = n / (16 * G), gate = (n / 16) % G, u = (b << 4) + (n & 15);
            return (u < H && k < jb.K) ? w[(size_t)(gate * H + u) * ldw + k] : 0.f;
        }
        case 3: {                                                   // [W1a - W1b ; W1b] (N = 2H rows, K = C), aux = H
            const int H = jb.aux, C = jb.K;
            if (!(n < jb.N && k < C)) return 0.f;
            return (n < H) ? w[(size_t)n * ldw + k] - w[(size_t)n * ldw + C + k] : w[(size_t)(n - H) * ldw + C + k];
        }
        case 4: {                                                   // transpose of the above (N = C, K = 2H), aux = H
            const int H = jb.aux, C = jb.N;
            if (!(n < C && k < jb.K)) return 0.f;
            return (k < H) ? w[(size_t)k * ldw + n] - w[(size_t)k * ldw + C + n] : w[(size_t)(k - H) * ldw + C + n];
        }
    }
    return 0.f;
}

// blocks a job occupies in a gpe_pack_multi launch (ops.PackPlan builds first_block from it).  Row-major sources (kinds 0, 2, 8:
// the reduction index k is the fast index of the weight) go through 64 x 64 tiles: rows are read in whole 256-byte pieces and turned
// in LDS — read column by column (round 2 - 5) every load instruction touched 64 cache lines for 64 floats.  Kind 9: 4096 elements
// per block (a quarter of the same-word atomics).  Everything else: 1024 outputs per block.
#define GPE_PACK_TILE 64
static long gpe_pack_blocks(int kind, long total, int Npad, int K)
{
    if (kind == 0 || kind == 2) return (long)gpe_cdiv(Npad, GPE_PACK_TILE) * gpe_cdiv(total / Npad, GPE_PACK_TILE);
    if (kind == 8) return (long)gpe_cdiv(Npad, GPE_PACK_TILE) * gpe_cdiv(gpe_round_up(K, 32), GPE_PACK_TILE);
    if (kind == 9) return gpe_cdiv(total, 4096);
    return gpe_cdiv(total, 1024);
}
extern "C" long gpe_pack_job_blocks(int kind, long total, int Npad, int K)
{
    if (kind < 0 || kind > 10 || total <= 0 || ((kind == 0 || kind == 2 || kind == 8) && Npad <= 0)) return GPE_EINVAL;
    return gpe_pack_blocks(kind, total, Npad, K);
}


// kinds 0 / 2 / 8: one 64-column x 64-k tile of the output per block
__device__ __forceinline__ void gpe_pack_tile(const GpePackJob& jb, long tb)
{
    __shared__ float tile[GPE_PACK_TILE][GPE_PACK_TILE + 2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ntn = (jb.Npad + GPE_PACK_TILE - 1) / GPE_PACK_TILE;
    const int tk = (int)(tb / ntn), tn = (int)(tb - (long)tk * ntn);
    const int n0 = tn * GPE_PACK_TILE, k0 = tk * GPE_PACK_TILE;
    const bool pair = ((jb.ldw & 1) == 0) && ((((uintptr_t)jb.w) & 7) == 0);       // rows start on 8-byte boundaries
    const int H = jb.aux, G = (jb.kind == 0) ? 1 : jb.N / H;
    // phase 1: a wave reads its 16 columns' source rows two at a time, 256 bytes of each
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int c = wave * 16 + s * 2 + (lane >> 5), kk = 2 * (lane & 31);
        const int n = n0 + c, k = k0 + kk;
        long row = -1;
        if (jb.kind == 0) row = (n < jb.N) ? n : -1;
        else {
            const int b = n / (16 * G), gate = (n >> 4) % G, u = (b << 4) + (n & 15);
            row = (n < jb.Npad && u < H) ? (long)gate * H + u : -1;
        }
        float2 v = make_float2(0.f, 0.f);
        if (row >= 0) {
            const float* src = jb.w + row * jb.ldw + k;
            if (pair && k + 1 < jb.K) v = *reinterpret_cast<const float2*>(src);
            else {
                if (k < jb.K) v.x = src[0];
                if (k + 1 < jb.K) v.y = src[1];
            }
        }
        *reinterpret_cast<float2*>(&tile[c][kk]) = v;
    }
    __syncthreads();
    // phase 2: outputs in their own order (consecutive threads = consecutive columns)
    if (jb.kind != 8) {
        const int Kpad = (int)(jb.total / jb.Npad);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i, kq = q >> 6, c = q & 63;
            if (n0 + c < jb.Npad && k0 + 4 * kq < Kpad)
                *reinterpret_cast<float4*>(jb.out + ((long)((k0 >> 2) + kq) * jb.Npad + n0 + c) * 4) =
                    make_float4(tile[c][4 * kq], tile[c][4 * kq + 1], tile[c][4 * kq + 2], tile[c][4 * kq + 3]);
        }
        return;
    }
    const int KP = (jb.K + 31) & ~31, KG = KP >> 3;
    float sc, inv;
    gpe_h3_scale_of(*reinterpret_cast<const unsigned*>(jb.w2), sc, inv);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = tid + 256 * i, plane = q >> 9, r = q & 511, kg = r >> 6, c = r & 63;
        if (n0 + c < jb.Npad && k0 + 8 * kg < KP) {
            gpe_f16x8 o;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const float xs = tile[c][8 * kg + t] * sc;
                const _Float16 h = (_Float16)xs;
                o[t] = plane ? (_Float16)(xs - (float)h) : h;
            }
            *reinterpret_cast<gpe_f16x8*>(reinterpret_cast<char*>(jb.out) + ((long)(plane * KG + (k0 >> 3) + kg) * jb.Npad + n0 + c) * 16) = o;
        }
    }
}

__global__ __launch_bounds__(256) void gpe_pack_multi_kernel(const GpePackJob* __restrict__ jobs, int njobs, int tiled)
{
    // wave-uniform job lookup: jobs are sorted by first_block
    int ji = 0;
    for (int q = 1; q < njobs; ++q) ji = ((long)blockIdx.x >= jobs[q].first_block) ? q : ji;
    const GpePackJob jb = jobs[ji];
    if (tiled && (jb.kind == 0 || jb.kind == 2 || jb.kind == 8)) {
        gpe_pack_tile(jb, (long)blockIdx.x - jb.first_block);
        return;
    }
    if (jb.kind == 9) {
        // largest |w| of a [N][K] matrix (row pitch ldw) -> atomicMax into the uint32 word at jb.out (zeroed by the caller):
        // phase 1 of the fp16-plane packs below, which normalise a weight by a power of two taken from it.  4096 elements per block
        __shared__ unsigned red9[4];
        const long e9 = ((long)blockIdx.x - jb.first_block) * 4096 + threadIdx.x;
        unsigned m = 0u;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const long i = e9 + 256 * t;
            if (i < jb.total) {
                const long n = i / jb.K;
                const unsigned a = __float_as_uint(jb.w[n * jb.ldw + (i - n * jb.K)]) & 0x7fffffffu;
                m = m > a ? m : a;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned t = (unsigned)__shfl_xor((int)m, o);
            m = m > t ? m : t;
        }
        if ((threadIdx.x & 63) == 0) red9[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned a = red9[0] > red9[1] ? red9[0] : red9[1], b = red9[2] > red9[3] ? red9[2] : red9[3];
            const unsigned r = a > b ? a : b;
            if (r) atomicMax(reinterpret_cast<unsigned*>(jb.out), r);
        }
        return;
    }
    const long e = (((long)blockIdx.x - jb.first_block) * 256 + threadIdx.x) * 4;
    if (e >= jb.total) return;
    if (jb.kind == 8 || jb.kind == 10) {
        // two-term fp16 planes of a weight in the B-fragment order of v_mfma_f32_16x16x32_f16: out = [plane h | plane l], a plane =
        // [KP / 8 k-groups][Npad columns][8 halves] (KP = K rounded up to 32, zero fill): lane (j, g) of the MFMA reads ONE 16-byte
        // piece = k 8 kg .. 8 kg + 7 of column n.  Values: w * 2^sh = h + l with 2^sh from the tensor's largest magnitude (the word at
        // jb.w2, written by a kind-9 job of an earlier launch).  kind 8: gate-interleaved columns (element map of kind 2);
        // kind 10: the plain transpose (element map of kind 1).  A thread writes one piece (16 bytes = "4 floats" of `total`).
        const unsigned u = (unsigned)(e >> 2);
        const unsigned KP = ((unsigned)jb.K + 31u) & ~31u, KG = KP >> 3;
        const unsigned per_plane = KG * (unsigned)jb.Npad;
        const unsigned plane = u / per_plane, r2 = u - plane * per_plane;
        const unsigned kg = r2 / (unsigned)jb.Npad;
        const int n = (int)(r2 - kg * (unsigned)jb.Npad);
        float sc, inv;
        gpe_h3_scale_of(*reinterpret_cast<const unsigned*>(jb.w2), sc, inv);
        GpePackJob je = jb;
        je.kind = (jb.kind == 8) ? 2 : 1;
        gpe_f16x8 o;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float xs = gpe_pack_elem(je, n, (int)(8 * kg) + t) * sc;
            const _Float16 h = (_Float16)xs;
            o[t] = plane ? (_Float16)(xs - (float)h) : h;
        }
        *reinterpret_cast<gpe_f16x8*>(reinterpret_cast<char*>(jb.out) + (size_t)u * 16) = o;
        return;
    }
    if (jb.kind >= 5) {                                              // vector jobs, element-wise
        for (int t = 0; t < 4 && e + t < jb.total; ++t) {
            const long i = e + t;
            float v;
            if (jb.kind == 5) v = jb.w[i] + jb.w2[i];                                   // b_ih + b_hh
            else if (jb.kind == 6) v = (i < jb.aux) ? jb.w[i] : 0.f;                    // [b1 | 0]
            else v = jb.w[i] + ((i < jb.aux) ? jb.w2[i] : 0.f);                         // GRU: b_ih + [b_hr | b_hz | 0]
            jb.out[i] = v;
        }
        return;
    }
    // matrix jobs: total = Npad * Kpad is a multiple of 4 and e = 4 * (kq * Npad + n)
    const unsigned r = (unsigned)(e >> 2);                           // a job's output is far below 2^31 elements
    const unsigned kq = r / (unsigned)jb.Npad;
    const int n = (int)(r - kq * (unsigned)jb.Npad);
    const int k0 = (int)(kq * 4);
    float4 v;
    v.x = gpe_pack_elem(jb, n, k0); v.y = gpe_pack_elem(jb, n, k0 + 1);
    v.z = gpe_pack_elem(jb, n, k0 + 2); v.w = gpe_pack_elem(jb, n, k0 + 3);
    *reinterpret_cast<float4*>(jb.out + e) = v;
}

extern "C" long gpe_packed_planes_size(int Npad, int K)
{
    if (Npad <= 0 || K <= 0) return GPE_EINVAL;
    return 2L * (((K + 31) & ~31) >> 3) * Npad * 4;
}

extern "C" int gpe_pack_multi(const void* jobs_dev, int njobs, long total_blocks, void* stream)
{
    if (!jobs_dev || njobs <= 0 || total_blocks <= 0 || total_blocks >= (1L << 31)) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_pack_multi_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const GpePackJob*>(jobs_dev), njobs, 1);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// gate-interleaved packing of an LSTM weight [4H][ldw] (rows i|f|g|o x H, torch.nn.LSTM layout): packed row
// b*64 + gate*16 + u'  <->  original row gate*H + 16*b + u', so one 64-column block holds the four gates of 16 units.
__global__ void gpe_pack_gates_kernel(const float* __restrict__ w, int ldw, int H, int K, float* __restrict__ wp,
                                      int Npad, long total)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int t = (int)(e & 3);
    const long r = e >> 2;
    const int n = (int)(r % Npad);
    const long kq = r / Npad;
    const int k = (int)(kq * 4 + t);
    const int b = n >> 6, gate = (n >> 4) & 3, u = (b << 4) + (n & 15);
    float v = 0.f;
    if (u < H && k < K) v = w[(size_t)(gate * H + u) * ldw + k];
    wp[e] = v;
}

extern "C" long gpe_packed_gates_size(int H, int K) { return 64L * gpe_cdiv(H, 16) * gpe_round_up(K, 16); }

// the same for G gates (G = 3: nn.GRU rows r|z|n): packed row b*16G + gate*16 + u'  <->  original row gate*H + 16b + u'
__global__ void gpe_pack_ngates_kernel(const float* __restrict__ w, int ldw, int H, int G, int K, float* __restrict__ wp,
                                       int Npad, long total)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int t = (int)(e & 3);
    const long r = e >> 2;
    const int n = (int)(r % Npad);
    const long kq = r / Npad;
    const int k = (int)(kq * 4 + t);
    const int b = n / (16 * G), gate = (n / 16) % G, u = (b << 4) + (n & 15);
    float v = 0.f;
    if (u < H && k < K) v = w[(size_t)(gate * H + u) * ldw + k];
    wp[e] = v;
}

extern "C" long gpe_packed_ngates_size(int H, int G, int K) { return 16L * G * gpe_cdiv(H, 16) * gpe_round_up(K, 16); }

extern "C" int gpe_pack_weight_ngates(const float* w, int ldw, int H, int G, int K, float* wp, void* stream)
{
    if (!w || !wp || H <= 0 || K <= 0 || G <= 0 || G > 8 || ldw < K) return GPE_EINVAL;
    const int Npad = 16 * G * gpe_cdiv(H, 16);
    const long total = (long)Npad * gpe_round_up(K, 16);
    hipLaunchKernelGGL(gpe_pack_ngates_kernel, dim3(gpe_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w, ldw, H,
                       G, K, wp, Npad, total);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_pack_weight_gates(const float* w, int ldw, int H, int K, float* wp, void* stream)
{
    if (!w || !wp || H <= 0 || K <= 0 || ldw < K) return GPE_EINVAL;
    const int Npad = 64 * gpe_cdiv(H, 16);
    const long total = (long)Npad * gpe_round_up(K, 16);
    hipLaunchKernelGGL(gpe_pack_gates_kernel, dim3(gpe_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w, ldw, H,
                       K, wp, Npad, total);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// ---------------------------------------------------------------------------------------------------------
// What a forward block of the edge MLP needs from the BatchNorm in front of it, in ONE launch (round 6; three before: gpe_pack_weight
// with col_scale = s -> gpe_fold_bias(t) -> the packed weight's amax pass of the f16x3 edge launch): PF_BLOCKS workgroups share
// W' = W diag(s) in the edge kernels' order and b' = b + W t; with the caller's edge workspace every workgroup leaves the largest
// magnitude of its share in a partial slot, takes a ticket behind a release fence, and the LAST one folds the partials into the
// f16x3 weight slot and clears the A-operand slot and the caller's output word (what the edge launch's own pass would have done).
// No workgroup waits for another.  Same arithmetic, same summation orders as the separate kernels: bit-identical results.
// ---------------------------------------------------------------------------------------------------------
#define PF_BLOCKS 64
#define PF_WAVES 16
__global__ __launch_bounds__(64 * PF_WAVES) void gpe_pack_fold_kernel(const float* __restrict__ w, int ldw, int N, int K,
                                                                      const float* __restrict__ col_scale, const float* __restrict__ t,
                                                                      const float* __restrict__ bias, float* __restrict__ wp, int Npad,
                                                                      long total, float* __restrict__ bias_out, unsigned* slots,
                                                                      unsigned* clear_word, unsigned* ticket)
{
    __shared__ double fred[PF_WAVES][64];
    __shared__ unsigned mred[PF_WAVES];
    __shared__ unsigned last_sh;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // ---- W' = W diag(s), the element order of gpe_pack_kernel; its largest magnitude on the way ----
    unsigned m = 0u;
    for (long e = (long)blockIdx.x * (64 * PF_WAVES) + threadIdx.x; e < total; e += (long)gridDim.x * (64 * PF_WAVES)) {
        const int tq = (int)(e & 3);
        const long r = e >> 2;
        const int n = (int)(r % Npad);
        const long kq = r / Npad;
        const int k = (int)(kq * 4 + tq);
        float v = 0.f;
        if (n < N && k < K) v = w[(size_t)n * ldw + k] * col_scale[k];
        wp[e] = v;
        const unsigned a = __float_as_uint(v) & 0x7fffffffu;
        m = m > a ? m : a;
    }
    // ---- b' = b + W t: one wave per row, lanes stride over k, fixed-order sum of the 64 partials (gpe_fold_bias_kernel) ----
    for (int n0 = blockIdx.x * PF_WAVES; n0 < N; n0 += gridDim.x * PF_WAVES) {
        const int n = n0 + wave;
        double fs = 0.0;
        if (n < N)
            for (int k = lane; k < K; k += 64) fs += (double)w[(size_t)n * ldw + k] * (double)t[k];
        fred[wave][lane] = fs;
        __syncthreads();
        if (lane == 0 && n < N) {
            double acc = bias ? (double)bias[n] : 0.0;
            for (int l = 0; l < 64; ++l) acc += fred[wave][l];
            bias_out[n] = (float)acc;
        }
        __syncthreads();
    }
    if (!slots) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned u = (unsigned)__shfl_xor((int)m, o);
        m = m > u ? m : u;
    }
    if (lane == 0) mred[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < PF_WAVES; ++i) m = m > mred[i] ? m : mred[i];
        __hip_atomic_store(slots + 2 + blockIdx.x, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();                                     // release: the partial before the ticket
        last_sh = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last_sh) return;
    __threadfence();                                         // acquire: every workgroup's partial
    unsigned mm = 0u;
    if (threadIdx.x < gridDim.x) mm = __hip_atomic_load(slots + 2 + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (wave == 0) {                                         // (gridDim.x <= 64)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned u = (unsigned)__shfl_xor((int)mm, o);
            mm = mm > u ? mm : u;
        }
        if (lane == 0) {
            slots[1] = mm;
            slots[0] = 0u;
            if (clear_word) clear_word[0] = 0u;
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

extern "C" int gpe_pack_fold(const float* w, int ldw, int N, int K, const float* col_scale, const float* t, const float* bias,
                             float* wp, float* bias_out, void* ws, long ws_bytes, uint32_t* clear_word, uint32_t* ticket, void* stream)
{
    if (!w || !col_scale || !t || !wp || !bias_out || N <= 0 || K <= 0 || ldw < K) return GPE_EINVAL;
    unsigned* slots = nullptr;
    if (ws) {
        const GpeEdgeWs e = gpe_edge_ws(ws, ws_bytes);
        if (!e.h3 || !ticket) return GPE_EINVAL;
        slots = e.h3;
    }
    const int Npad = gpe_round_up(N, 16);
    const long total = (long)Npad * gpe_pack_kpad(K);
    hipLaunchKernelGGL(gpe_pack_fold_kernel, dim3(PF_BLOCKS), dim3(64 * PF_WAVES), 0, (hipStream_t)stream, w, ldw, N, K, col_scale, t, bias,
                       wp, Npad, total, bias_out, slots, clear_word, ticket);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// one wave per output row: lanes stride over k (coalesced), butterfly-free fixed-order reduction through LDS
__global__ __launch_bounds__(256) void gpe_fold_bias_kernel(const float* __restrict__ w, int ldw, int N, int K,
                                                            const float* __restrict__ bias, const float* __restrict__ t,
                                                            float* out)
{
    __shared__ double red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * 4 + wave;
    double s = 0.0;
    if (n < N)
        for (int k = lane; k < K; k += 64) s += (double)w[(size_t)n * ldw + k] * (double)t[k];
    red[wave][lane] = s;
    __syncthreads();
    if (lane == 0 && n < N) {
        double acc = bias ? (double)bias[n] : 0.0;
        for (int l = 0; l < 64; ++l) acc += red[wave][l];
        out[n] = (float)acc;
    }
}

extern "C" int gpe_fold_bias(const float* w, int ldw, int N, int K, const float* bias, const float* t, float* out,
                             void* stream)
{
    if (!w || !t || !out || N <= 0 || K <= 0 || ldw < K) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_fold_bias_kernel, dim3(gpe_cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, w, ldw, N, K,
                       bias, t, out);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
