// The training pairs of the edge-pair classifier drawn on the device (StitchOnEdge3DPairs with random_pairs_mode: what
// NNSewingPattern.stitches_as_3D_pairs, nn/data/pattern_converter.py:321-409, followed by FeatureStandartization does per garment
// on the host with numpy's generator), one launch per batch.
//
//   slot b      garment g = index[b] of the resident set; one 256-thread workgroup
//   stitches    the entries s < gt_num_stitches[g] whose two edge ids (panel * L + edge) name present edges, in order (a workgroup
//               prefix scan compacts them): rows [0, S_v), label 1; each also sets two bits of an E x E mask in LDS
//   duplicates  rows [S_v, n_stitched): a copy of a uniformly chosen row below S_v, as stored; label 1
//   negatives   n_non_stitched rows (all R rows when S_v == 0), label 0: a thread per row draws (panel, edge, panel, edge) among the
//               present ones until the pair is neither a self pair nor in the mask; after 64 rejected attempts the row gives up
//               (zeros) and is counted in status[b]
//   flips       bit 0 of flags: every present edge is reversed with probability 1/2, once per slot (endpoints swapped,
//               cx -> cx ? 1 - cx : 0, cy -> -cy), and each of the S_v stitch rows has its halves swapped with probability 1/2
//   order       bit 1 of flags: row r goes to the rank of (32-bit key, r) among the R rows, counted in LDS
//   rows        ([e_a | e_b] - shift) / scale, the fp32 subtract-then-divide of gpe_stitch_pairs_rows, written in output order
//
// Every decision is one Philox4x32-10 block keyed by the seed with the counter (item | kind << 28, attempt | b << 8, draw lo,
// draw hi): a pure function of (seed, draw, b, inputs), whatever the grid does.  Thread 0 of every workgroup reads {seed, draw} and
// then takes a ticket; the last one to do so stores draw + 1 and clears the ticket (gpe_pack_fold's scheme: nobody waits), so a
// captured launch draws new pairs on every replay.  Plain vector stores and integer atomics only.
#include "gpe_device.h"

#define SS_TPB 256
#define SS_MAXE 512             // edge slots of a garment, P * L
#define SS_MAXR 4096            // rows per slot
#define SS_MAXF 16              // features per edge
#define SS_ATTEMPTS 64
#define SS_GIVEUP 0xffffffffu   // a row descriptor is e_a | e_b << 16 (edge ids < 512)

enum { SS_FLIP = 0, SS_SWAP = 1, SS_DUP = 2, SS_PAIR = 3, SS_KEY = 4 };

struct SsParams {
    const float* edges; const int32_t* ne; const int32_t* gt; const int32_t* gt_num;
    int G, P, L, Fe, S;
    const int32_t* index; int n_stitched, R, flags;
    unsigned long long* state; unsigned* ticket;
    float* rows; uint8_t* labels; int32_t* status;
    float shift[2 * SS_MAXF], scale[2 * SS_MAXF];
};

// an integer in [0, n)
__device__ __forceinline__ unsigned ss_below(unsigned word, unsigned n) { return __umulhi(word, n); }

// every thread of the workgroup calls this: -> how many threads below this one raised `flag`; total = how many did.  s_w: 4 words
__device__ __forceinline__ int ss_scan(bool flag, int& total, int* s_w)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    __syncthreads();                                         // the previous call's readers are done with s_w
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();
    int below = __popcll(m & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int w = 0; w < SS_TPB / 64; ++w) {
        below += w < wave ? s_w[w] : 0;
        total += s_w[w];
    }
    return below;
}

__device__ __forceinline__ void ss_zero_slot(const SsParams& p, int b, int status)
{
    float* rows = p.rows + (long)b * p.R * (2 * p.Fe);
    for (int i = threadIdx.x; i < p.R * 2 * p.Fe; i += SS_TPB) rows[i] = 0.f;
    for (int i = threadIdx.x; i < p.R; i += SS_TPB) p.labels[(long)b * p.R + i] = 0;
    if (threadIdx.x == 0) p.status[b] = status;
}

// feature k of an edge as the row carries it, before the standardisation
__device__ __forceinline__ float ss_feature(const float* e, int k, bool flip)
{
    if (!flip) return e[k];
    if (k < 6) return e[k < 3 ? k + 3 : k - 3];
    if (k == 6) { const float cx = e[6]; return cx != 0.f ? 1.f - cx : 0.f; }
    return -e[7];
}

// V floats per store: 4 (16-byte stores; 2 Fe a multiple of 4 and rows 16-byte aligned) or 1
template <int V>
__global__ __launch_bounds__(SS_TPB) void gpe_stitch_sample_kernel(SsParams p)
{
    __shared__ unsigned s_mask[SS_MAXE * (SS_MAXE / 32)];    // bit (e_j % 32) of word [e_i][e_j / 32]: a valid stitch, symmetric
    __shared__ unsigned s_row[SS_MAXR];                      // pre-shuffle rows
    unsigned* const s_key = s_mask;                          // the order keys take the mask's place once the negatives are drawn
    __shared__ unsigned short s_inv[SS_MAXR];                // output position -> pre-shuffle row
    __shared__ unsigned short s_panel[SS_MAXE];              // the present panels, ascending
    __shared__ unsigned short s_cnt[SS_MAXE];                // edges of a panel slot
    __shared__ unsigned char s_flip[SS_MAXE];
    __shared__ unsigned long long s_state[2];
    __shared__ int s_w[SS_TPB / 64];
    __shared__ int s_give;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int P = p.P, L = p.L, Fe = p.Fe, E = P * L, R = p.R, W = (E + 31) >> 5;

    if (tid == 0) {
        const unsigned long long seed = __hip_atomic_load(p.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long draw = __hip_atomic_load(p.state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_state[0] = seed; s_state[1] = draw;
        s_give = 0;
        __threadfence();                                     // the reads before the ticket
        if (gpe_flag_ticket(p.ticket) == gridDim.x - 1) {    // every workgroup has read the state: advance it for the next launch
            __hip_atomic_store(p.state + 1, draw + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(p.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    const int g = p.index[b];
    if (g < 0 || g >= p.G) { ss_zero_slot(p, b, -2); return; }            // block-uniform
    __syncthreads();
    const gpe_rng rng = {(unsigned)s_state[0], (unsigned)(s_state[0] >> 32), (unsigned)s_state[1], (unsigned)(s_state[1] >> 32),
                         (unsigned)b << 8};
    const bool flips = p.flags & 1, shuffle = p.flags & 2;

    // ---- present panels ----
    int n_present = 0;
    for (int p0 = 0; p0 < P; p0 += SS_TPB) {
        const int q = p0 + tid;
        int n = 0;
        if (q < P) {
            n = p.ne[(long)g * P + q];
            n = n < 0 ? 0 : (n > L ? L : n);
            s_cnt[q] = (unsigned short)n;
        }
        int total;
        const int rank = n_present + ss_scan(n > 0, total, s_w);
        if (n > 0) s_panel[rank] = (unsigned short)q;
        n_present += total;
    }
    for (int i = tid; i < E * W; i += SS_TPB) s_mask[i] = 0u;
    __syncthreads();
    for (int e = tid; e < E; e += SS_TPB) {
        const int q = e / L;
        s_flip[e] = flips && e - q * L < (int)s_cnt[q] && (rng(SS_FLIP, e).x >> 31);
    }

    // ---- valid stitches, in order ----
    int nS = p.gt_num[g];
    nS = nS < 0 ? 0 : (nS > p.S ? p.S : nS);
    int Sv = 0;
    for (int s0 = 0; s0 < nS; s0 += SS_TPB) {
        const int s = s0 + tid;
        int ea = -1, eb = -1;
        bool valid = false;
        if (s < nS) {
            ea = p.gt[((long)g * 2 + 0) * p.S + s];
            eb = p.gt[((long)g * 2 + 1) * p.S + s];
            if (ea >= 0 && ea < E && eb >= 0 && eb < E) {
                const int qa = ea / L, qb = eb / L;
                valid = ea - qa * L < (int)s_cnt[qa] && eb - qb * L < (int)s_cnt[qb];
            }
        }
        int total;
        const int rank = Sv + ss_scan(valid, total, s_w);
        if (valid) {
            atomicOr(&s_mask[ea * W + (eb >> 5)], 1u << (eb & 31));
            atomicOr(&s_mask[eb * W + (ea >> 5)], 1u << (ea & 31));
            if (rank < p.n_stitched) {
                const bool swap = flips && (rng(SS_SWAP, rank).x >> 31);
                s_row[rank] = swap ? ((unsigned)eb | ((unsigned)ea << 16)) : ((unsigned)ea | ((unsigned)eb << 16));
            }
        }
        Sv += total;
    }
    __syncthreads();
    if (Sv > p.n_stitched) { ss_zero_slot(p, b, -1); return; }            // block-uniform

    // ---- duplicates and negatives ----
    const int n_pos = Sv > 0 ? p.n_stitched : 0, n_neg = R - n_pos;
    for (int r = Sv + tid; r < n_pos; r += SS_TPB) s_row[r] = s_row[ss_below(rng(SS_DUP, r).x, Sv)];
    for (int j = tid; j < n_neg; j += SS_TPB) {
        unsigned d = SS_GIVEUP;
        for (int a = 0; a < SS_ATTEMPTS && n_present > 0; ++a) {
            const gpe_u32x4 w = rng(SS_PAIR, j, a);
            const int qa = s_panel[ss_below(w.x, n_present)], qb = s_panel[ss_below(w.z, n_present)];
            const int ea = qa * L + (int)ss_below(w.y, s_cnt[qa]), eb = qb * L + (int)ss_below(w.w, s_cnt[qb]);
            if (ea != eb && !((s_mask[ea * W + (eb >> 5)] >> (eb & 31)) & 1u)) {
                d = (unsigned)ea | ((unsigned)eb << 16);
                break;
            }
        }
        s_row[n_pos + j] = d;
        if (d == SS_GIVEUP) atomicAdd(&s_give, 1);
    }
    __syncthreads();                                         // the mask has been read
    if (shuffle)
        for (int r = tid; r < R; r += SS_TPB) s_key[r] = rng(SS_KEY, r).x;
    __syncthreads();

    // ---- output order ----
    for (int r = tid; r < R; r += SS_TPB) {
        int pos = r;
        if (shuffle) {
            const unsigned k = s_key[r];
            pos = 0;
            for (int q = 0; q < R; ++q) {                    // (every lane reads the same word: an LDS broadcast)
                const unsigned kq = s_key[q];
                pos += kq < k || (kq == k && q < r) ? 1 : 0;
            }
        }
        s_inv[pos] = (unsigned short)r;
    }
    __syncthreads();

    // ---- rows, labels, status ----
    const int U = 2 * Fe / V;
    const float* edges = p.edges + (long)g * E * Fe;
    for (int i = tid; i < R * U; i += SS_TPB) {
        const int pos = i / U, u = i - pos * U;
        const int r = s_inv[pos];
        const unsigned d = s_row[r];
        float v[V];
#pragma unroll
        for (int t = 0; t < V; ++t) {
            const int f = u * V + t;
            const bool second = f >= Fe;
            const int e = second ? (int)(d >> 16) : (int)(d & 0xffffu);
            v[t] = d == SS_GIVEUP ? 0.f : (ss_feature(edges + (long)e * Fe, second ? f - Fe : f, s_flip[e]) - p.shift[f]) / p.scale[f];
        }
        float* dst = p.rows + (((long)b * R + pos) * (2 * Fe) + u * V);
        if constexpr (V == 4) *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
        else dst[0] = v[0];
        if (u == 0) p.labels[(long)b * R + pos] = r < n_pos ? 1 : 0;
    }
    if (tid == 0) p.status[b] = s_give;
}

extern "C" int gpe_stitch_sample(const float* edges3d, const int32_t* num_edges, const int32_t* gt_stitches,
                                 const int32_t* gt_num_stitches, int G, int P, int L, int Fe, int S, const int32_t* index, int B,
                                 int n_stitched, int n_non_stitched, int flags, const float* shift_host, const float* scale_host,
                                 uint64_t* state, uint32_t* ticket, float* rows, uint8_t* labels, int32_t* status, void* stream)
{
    if (!edges3d || !num_edges || !gt_num_stitches || !index || !shift_host || !scale_host || !state || !ticket || !rows || !labels ||
        !status || (((uintptr_t)state) & 7))
        return GPE_EINVAL;
    if (G < 1 || P < 1 || L < 1 || (long)P * L > SS_MAXE || Fe < 1 || Fe > SS_MAXF || S < 0 || (S > 0 && !gt_stitches)) return GPE_EINVAL;
    if ((flags & ~3) || ((flags & 1) && Fe != 8) || B < 1 || B > (1 << 24) || n_stitched < 0 || n_non_stitched < 0) return GPE_EINVAL;
    const long R = (long)n_stitched + n_non_stitched;
    if (R < 1 || R > SS_MAXR) return GPE_EINVAL;
    SsParams p;
    p.edges = edges3d; p.ne = num_edges; p.gt = gt_stitches; p.gt_num = gt_num_stitches;
    p.G = G; p.P = P; p.L = L; p.Fe = Fe; p.S = S;
    p.index = index; p.n_stitched = n_stitched; p.R = (int)R; p.flags = flags;
    p.state = reinterpret_cast<unsigned long long*>(state); p.ticket = ticket;
    p.rows = rows; p.labels = labels; p.status = status;
    for (int f = 0; f < 2 * SS_MAXF; ++f) {
        p.shift[f] = f < 2 * Fe ? shift_host[f] : 0.f;
        p.scale[f] = f < 2 * Fe ? scale_host[f] : 1.f;
    }
    if (Fe % 2 == 0 && !(((uintptr_t)rows) & 15))
        hipLaunchKernelGGL(gpe_stitch_sample_kernel<4>, dim3(B), dim3(SS_TPB), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(gpe_stitch_sample_kernel<1>, dim3(B), dim3(SS_TPB), 0, (hipStream_t)stream, p);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
