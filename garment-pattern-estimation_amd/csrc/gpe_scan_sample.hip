// The model's input clouds drawn on the device from resident raw scans, and the predicted per-point labels handed back to every point
// of a scan (what nn/evaluation_scripts/predict_per_example.py does per scan on the host: np.random.permutation(n)[:mesh_samples],
// FeatureStandartization, stack).  include/gpe_hip_scan.h holds the rule in full; in short:
//
//   slot b       cloud g = index[b] of the resident set (points4 [T, 4], off [G + 1]), n points
//   key          point i: (w0 << 32) | w1 of the samplers' block of kind 13, item i, slot b, under the call's {seed, draw}
//   order        the points by (key, i) ascending; row r < N is the point of rank r, rank r mod n when n < N (status = N - n)
//   bad slot     n = 0: status -1, index outside the set: status -2; rows of zeros, picked -1
//   output       features (p - shift) / scale, the fp32 subtract-then-divide of gpe_standardize (p itself without statistics);
//                picked: the point's index inside its cloud; status
//   labels       for every point of a cloud named by a valid slot: the row of the lexicographic minimum of (d, row) over the slot's
//                N drawn points, d = (dx dx + dy dy) + dz dz with every operation rounded on its own, then the first maximum over P
//                of that row's weights.  Two slots with the same cloud: the higher slot writes, the lower does not
//
// The selection is a radix select whose keys are never stored: every pass recomputes them from i.  A memset and three launches in
// stream order — histogram of the leading SS_HB key bits (several workgroups per slot, integer atomics), collect of everything at or
// below the bin where the count crosses N, and one workgroup per slot that sorts the survivors by (key, i) in LDS, gathers and writes.
// A boundary bin too full to list is narrowed by that workgroup alone (ss_narrow): exact for every n, no status asks for another
// try.  The order comes from the sort, never from where an atomic landed, so the result is a function of (seed, draw, b, data).  The
// state {seed, draw} and the last-arriver ticket are those of gpe_mesh_sample.hip.  Plain vector stores and integer atomics only.
#include "gpe_device.h"

#pragma clang fp contract(off)
__device__ __forceinline__ float ss_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float ss_add(float a, float b) { return a + b; }
__device__ __forceinline__ float ss_sub(float a, float b) { return a - b; }

#define SS_KIND 13
#define SS_TPB 256                      // histogram and collect passes
#define SS_IPT 16                       // points per thread there
#define SS_CHUNK (SS_TPB * SS_IPT)      // points per workgroup
#define SS_HB 11                        // leading key bits of the first level
#define SS_BINS (1 << SS_HB)
#define SS_FTPB 1024                    // the finishing workgroup
#define SS_SORT 4096                    // entries of its LDS image: N <= GPE_SCAN_MAX_SAMPLES = SS_SORT / 2
#define SL_TPB 256                      // labels: one workgroup owns SL_PPT scan points per thread
#define SL_PPT 2
#define SL_PTS (SL_TPB * SL_PPT)

struct SsParams {
    const f32x4* points; const int32_t* off; const int32_t* index;
    int G, B, N, chunks, n_max, narrow_above, standardize;
    float shift[3], scale[3];
    unsigned long long* state; unsigned* ticket;
    unsigned long long* ws_state;       // [2]: the call's {seed, draw}, left by the histogram pass for the two that follow
    unsigned* cnt;                      // [B]: entries of the candidate list
    unsigned* hist;                     // [B][SS_BINS]
    gpe_u32x4* cand;                    // [B][SS_SORT] {key hi, key lo, i, 0}
    float* features; int32_t* picked; int32_t* status;
};

// the cloud of slot b: -2 index outside the set, -1 empty, 0 fine (block-uniform)
__device__ __forceinline__ int ss_cloud(const int32_t* index, const int32_t* off, int G, int n_max, int b, int& p0, int& n)
{
    const int g = index[b];
    p0 = 0; n = 0;
    if (g < 0 || g >= G) return -2;
    p0 = off[g]; n = off[g + 1] - p0;
    if (n < 1) { n = 0; return -1; }
    n = n < n_max ? n : n_max;
    return 0;
}

__device__ __forceinline__ gpe_rng ss_rng(unsigned long long seed, unsigned long long draw, int b)
{
    return gpe_rng{(unsigned)seed, (unsigned)(seed >> 32), (unsigned)draw, (unsigned)(draw >> 32), (unsigned)b << 8};
}

// exclusive prefix sum of v over the workgroup (blockDim.x a multiple of 64, at most 1024); s_w: 17 words of LDS.  -> the prefix of
// this thread; total: the sum over all threads
__device__ __forceinline__ unsigned ss_block_scan(unsigned v, unsigned* s_w, unsigned& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    __syncthreads();                                         // s_w is free again
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    unsigned base = 0, sum = 0;
    for (int w = 0; w < waves; ++w) {
        const unsigned t = s_w[w];
        if (w < wave) base += t;
        sum += t;
    }
    total = sum;
    return base + inc - v;
}

// the bin where the running count of h[0 .. SS_BINS) reaches `need` (1 <= need <= the sum of h): -> D, below = the count of the
// bins in front of it, count = h[D].  Every thread calls it and gets the same answer; s_w: 20 words of LDS
__device__ __forceinline__ void ss_find(const unsigned* h, unsigned need, unsigned* s_w, unsigned& D, unsigned& below, unsigned& count)
{
    const int per = SS_BINS / blockDim.x;                    // 8 or 2 consecutive bins per thread
    unsigned mine = 0;
    for (int j = 0; j < per; ++j) mine += h[threadIdx.x * per + j];
    unsigned total;
    unsigned run = ss_block_scan(mine, s_w, total);
    if (threadIdx.x == 0) { s_w[17] = SS_BINS - 1; s_w[18] = 0; s_w[19] = 0; }      // (never read when need is in range)
    __syncthreads();
    if (run < need && need <= run + mine) {                  // exactly one thread
        for (int j = 0; j < per; ++j) {
            const unsigned c = h[threadIdx.x * per + j];
            if (need <= run + c) { s_w[17] = threadIdx.x * per + j; s_w[18] = run; s_w[19] = c; break; }
            run += c;
        }
    }
    __syncthreads();
    D = s_w[17]; below = s_w[18]; count = s_w[19];
}

// is the boundary bin listed by the collect pass?  (block-uniform; the same expression in both readers)
__device__ __forceinline__ bool ss_listed(const SsParams& p, unsigned below, unsigned count)
{
    return below + count <= (unsigned)SS_SORT && (p.narrow_above == 0 || count <= (unsigned)p.narrow_above);
}

__global__ __launch_bounds__(SS_TPB) void gpe_scan_hist_kernel(SsParams p)
{
    __shared__ unsigned s_hist[SS_BINS];
    __shared__ unsigned long long s_state[2];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.chunks, c = blockIdx.x - b * p.chunks;
    if (tid == 0) {
        const unsigned long long seed = __hip_atomic_load(p.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long draw = __hip_atomic_load(p.state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_state[0] = seed; s_state[1] = draw;
        if (blockIdx.x == 0) { p.ws_state[0] = seed; p.ws_state[1] = draw; }
        __threadfence();                                     // the reads before the ticket
        if (gpe_flag_ticket(p.ticket) == gridDim.x - 1) {    // every workgroup has read the state: advance it for the next call
            __hip_atomic_store(p.state + 1, draw + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(p.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    int p0, n;
    if (ss_cloud(p.index, p.off, p.G, p.n_max, b, p0, n)) return;                   // block-uniform
    if (n <= p.N || c * SS_CHUNK >= n) return;               // a short cloud is sorted whole by the finishing workgroup
    for (int j = tid; j < SS_BINS; j += SS_TPB) s_hist[j] = 0;
    __syncthreads();
    const gpe_rng rng = ss_rng(s_state[0], s_state[1], b);
#pragma unroll 4
    for (int k = 0; k < SS_IPT; ++k) {
        const int i = c * SS_CHUNK + k * SS_TPB + tid;
        if (i < n) atomicAdd(&s_hist[rng(SS_KIND, (unsigned)i).x >> (32 - SS_HB)], 1u);
    }
    __syncthreads();
    unsigned* hist = p.hist + (long)b * SS_BINS;
    for (int j = tid; j < SS_BINS; j += SS_TPB)
        if (s_hist[j]) atomicAdd(&hist[j], s_hist[j]);
}

__global__ __launch_bounds__(SS_TPB) void gpe_scan_collect_kernel(SsParams p)
{
    __shared__ unsigned s_w[20];
    __shared__ unsigned s_base;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.chunks, c = blockIdx.x - b * p.chunks;
    int p0, n;
    if (ss_cloud(p.index, p.off, p.G, p.n_max, b, p0, n)) return;
    if (n <= p.N || c * SS_CHUNK >= n) return;
    unsigned T, below, count;
    ss_find(p.hist + (long)b * SS_BINS, (unsigned)p.N, s_w, T, below, count);
    const bool listed = ss_listed(p, below, count);
    if (!listed) return;                                     // block-uniform: the finishing workgroup narrows and collects by itself
    const gpe_rng rng = ss_rng(p.ws_state[0], p.ws_state[1], b);
    unsigned take = 0, mine = 0;                             // few are taken (about N of n): their keys are recomputed below, not kept
#pragma unroll 4
    for (int k = 0; k < SS_IPT; ++k) {
        const int i = c * SS_CHUNK + k * SS_TPB + tid;
        if (i < n && (rng(SS_KIND, (unsigned)i).x >> (32 - SS_HB)) <= T) { take |= 1u << k; ++mine; }
    }
    unsigned total;
    unsigned at = ss_block_scan(mine, s_w, total);
    if (total == 0) return;                                  // block-uniform
    if (tid == 0) s_base = atomicAdd(&p.cnt[b], total);      // ONE addition per workgroup; where it lands decides no output
    __syncthreads();
    at += s_base;
    gpe_u32x4* cand = p.cand + (long)b * SS_SORT;
    while (take) {
        const int k = __ffs(take) - 1;
        take &= take - 1;
        const unsigned i = (unsigned)(c * SS_CHUNK + k * SS_TPB + tid);
        const gpe_u32x4 w = rng(SS_KIND, i);
        if (at < (unsigned)SS_SORT) cand[at] = gpe_u32x4{w.x, w.y, i, 0u};
        ++at;
    }
}

// the three words of the composite (key hi, key lo, i) are cut into digits of 11 / 11 / 10 bits, from the top: level l = 0 .. 8 is
// digit l % 3 of word l / 3
__device__ __forceinline__ void ss_digit(int level, int& word, int& shift, unsigned& mask)
{
    const int sub = level % 3;
    word = level / 3;
    shift = sub == 0 ? 21 : sub == 1 ? 10 : 0;
    mask = sub == 2 ? 1023u : 2047u;
}

// The finishing workgroup narrows a boundary bin that was not listed: from level 1 on (level 0 is bin T of the table), a pass over the
// cloud per level histograms the next digit of the points that share the prefix found so far, until the prefix holds exactly what is
// still missing (every point under it is taken) or every bit is fixed.  Then one more pass collects the points whose masked
// composite is at or below the prefix: exactly N of them, into the LDS image.  Every thread calls it.
__device__ __forceinline__ void ss_narrow(const gpe_rng& rng, int n, unsigned T, unsigned need, unsigned count, unsigned* s_hist,
                                          unsigned* s_w, unsigned* s_cnt, unsigned* s_k0, unsigned* s_k1, unsigned* s_i)
{
    const int tid = threadIdx.x;
    unsigned pre0 = T << (32 - SS_HB), pre1 = 0u, pre2 = 0u, fix0 = 2047u << (32 - SS_HB), fix1 = 0u, fix2 = 0u;
    for (int level = 1; level < 9 && count != need; ++level) {
        int word, shift; unsigned mask;
        ss_digit(level, word, shift, mask);
        __syncthreads();                                     // the previous table has been read
        for (int j = tid; j < SS_BINS; j += SS_FTPB) s_hist[j] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += SS_FTPB) {
            const gpe_u32x4 w = rng(SS_KIND, (unsigned)i);
            if ((w.x & fix0) == pre0 && (w.y & fix1) == pre1 && ((unsigned)i & fix2) == pre2)
                atomicAdd(&s_hist[((word == 0 ? w.x : word == 1 ? w.y : (unsigned)i) >> shift) & mask], 1u);
        }
        __syncthreads();
        unsigned D, below;
        ss_find(s_hist, need, s_w, D, below, count);
        need -= below;
        if (word == 0) { pre0 |= D << shift; fix0 |= mask << shift; }
        else if (word == 1) { pre1 |= D << shift; fix1 |= mask << shift; }
        else { pre2 |= D << shift; fix2 |= mask << shift; }
    }
    __syncthreads();
    for (int i = tid; i < n; i += SS_FTPB) {
        const gpe_u32x4 w = rng(SS_KIND, (unsigned)i);
        const unsigned a0 = w.x & fix0, a1 = w.y & fix1, a2 = (unsigned)i & fix2;
        const bool in = a0 < pre0 || (a0 == pre0 && (a1 < pre1 || (a1 == pre1 && a2 <= pre2)));
        if (in) {
            const unsigned at = atomicAdd(s_cnt, 1u);        // LDS; where a point lands decides no output: the sort follows
            if (at < (unsigned)SS_SORT) { s_k0[at] = w.x; s_k1[at] = w.y; s_i[at] = (unsigned)i; }
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(SS_FTPB) void gpe_scan_finish_kernel(SsParams p)
{
    __shared__ unsigned s_k0[SS_SORT], s_k1[SS_SORT], s_i[SS_SORT];
    __shared__ unsigned s_hist[SS_BINS];
    __shared__ unsigned s_w[20];
    __shared__ unsigned s_cnt;
    const int tid = threadIdx.x, b = blockIdx.x, N = p.N;
    int p0, n;
    const int bad = ss_cloud(p.index, p.off, p.G, p.n_max, b, p0, n);
    if (tid == 0) p.status[b] = bad ? bad : (n < N ? N - n : 0);
    float* feat = p.features + (long)b * N * 3;
    int32_t* picked = p.picked + (long)b * N;
    if (bad) {                                               // block-uniform
        for (int r = tid; r < N; r += SS_FTPB) {
            feat[r * 3] = 0.f; feat[r * 3 + 1] = 0.f; feat[r * 3 + 2] = 0.f;
            picked[r] = -1;
        }
        return;
    }
    const gpe_rng rng = ss_rng(p.ws_state[0], p.ws_state[1], b);
    int m;                                                   // the entries to sort; the first min(m, N) are the answer
    if (n <= N) {
        m = n;
        for (int i = tid; i < n; i += SS_FTPB) {
            const gpe_u32x4 w = rng(SS_KIND, (unsigned)i);
            s_k0[i] = w.x; s_k1[i] = w.y; s_i[i] = (unsigned)i;
        }
    } else {
        unsigned T, below, count;
        ss_find(p.hist + (long)b * SS_BINS, (unsigned)N, s_w, T, below, count);
        if (ss_listed(p, below, count)) {
            m = (int)(below + count);                        // = cnt[b]
            const gpe_u32x4* cand = p.cand + (long)b * SS_SORT;
            for (int j = tid; j < m; j += SS_FTPB) {
                const gpe_u32x4 e = cand[j];
                s_k0[j] = e.x; s_k1[j] = e.y; s_i[j] = e.z;
            }
        } else {
            if (tid == 0) s_cnt = 0;
            ss_narrow(rng, n, T, (unsigned)N - below, count, s_hist, s_w, &s_cnt, s_k0, s_k1, s_i);
            m = (int)(s_cnt < (unsigned)SS_SORT ? s_cnt : SS_SORT);                  // = N: the points in front of bin T are below the prefix too
        }
    }
    int P = 64;
    while (P < m) P <<= 1;                                   // m <= SS_SORT
    for (int j = m + tid; j < P; j += SS_FTPB) { s_k0[j] = 0xffffffffu; s_k1[j] = 0xffffffffu; s_i[j] = 0xffffffffu; }
    // bitonic sort by (key hi, key lo, i) ascending; the padding (i = 2^32 - 1 > every index) ends up behind
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int x = tid; x < P; x += SS_FTPB) {
                const int y = x ^ j;
                if (y > x) {
                    const unsigned a0 = s_k0[x], a1 = s_k1[x], a2 = s_i[x], b0 = s_k0[y], b1 = s_k1[y], b2 = s_i[y];
                    const bool gt = a0 > b0 || (a0 == b0 && (a1 > b1 || (a1 == b1 && a2 > b2)));
                    if (gt == ((x & k) == 0)) {
                        s_k0[x] = b0; s_k1[x] = b1; s_i[x] = b2;
                        s_k0[y] = a0; s_k1[y] = a1; s_i[y] = a2;
                    }
                }
            }
        }
    }
    __syncthreads();
    const int have = m < N ? m : N;                          // n when the cloud is short, N otherwise
    for (int r = tid; r < N; r += SS_FTPB) {
        unsigned i = s_i[r < have ? r : r % have];
        if (i >= (unsigned)n) i = 0;                         // (not reached: every listed index is a point of the cloud)
        const f32x4 v = p.points[(long)p0 + i];
        if (p.standardize) {
            feat[r * 3] = (v.x - p.shift[0]) / p.scale[0];
            feat[r * 3 + 1] = (v.y - p.shift[1]) / p.scale[1];
            feat[r * 3 + 2] = (v.z - p.shift[2]) / p.scale[2];
        } else {
            feat[r * 3] = v.x; feat[r * 3 + 1] = v.y; feat[r * 3 + 2] = v.z;
        }
        picked[r] = (int32_t)i;
    }
}

struct SlParams {
    const f32x4* points; const int32_t* off; const int32_t* index; const int32_t* picked; const float* att;
    int G, B, N, P, chunks, n_max;
    int32_t* labels;
};

__global__ __launch_bounds__(SL_TPB) void gpe_scan_labels_kernel(SlParams p)
{
    __shared__ f32x4 s_tile[SL_TPB];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.chunks, c = blockIdx.x - b * p.chunks, N = p.N;
    int p0, n;
    if (ss_cloud(p.index, p.off, p.G, p.n_max, b, p0, n)) return;                   // block-uniform
    if (c * SL_PTS >= n) return;
    const int g = p.index[b];
    int later = 0;                                           // a higher slot names the same cloud: its labels stand
    for (int o = b + 1 + tid; o < p.B; o += SL_TPB) later |= p.index[o] == g;
    if (__syncthreads_or(later)) return;
    const f32x4* cloud = p.points + p0;
    const int32_t* picked = p.picked + (long)b * N;

    float px[SL_PPT], py[SL_PPT], pz[SL_PPT], bd[SL_PPT];
    int best[SL_PPT];
#pragma unroll
    for (int q = 0; q < SL_PPT; ++q) {
        const int i = c * SL_PTS + q * SL_TPB + tid;
        px[q] = py[q] = pz[q] = 0.f;
        bd[q] = INFINITY; best[q] = -1;
        if (i < n) { const f32x4 v = cloud[i]; px[q] = v.x; py[q] = v.y; pz[q] = v.z; }
    }
    // the drawn points pass through LDS in tiles, in ascending row order, and each scan point keeps the first row of the smallest
    // distance: the minimum depends on no tile or grid shape.  w of a staged row: 1 when its `picked` names a point of the cloud
    for (int base = 0; base < N; base += SL_TPB) {
        __syncthreads();                                     // the previous tile has been read
        f32x4 e = {0.f, 0.f, 0.f, 0.f};
        if (base + tid < N) {
            const int k = picked[base + tid];
            if (k >= 0 && k < n) { e = cloud[k]; e.w = 1.f; }
        }
        s_tile[tid] = e;
        __syncthreads();
        const int cnt = N - base < SL_TPB ? N - base : SL_TPB;
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const f32x4 v = s_tile[j];                       // every lane reads the same element: an LDS broadcast
            const bool ok = v.w != 0.f;
#pragma unroll
            for (int q = 0; q < SL_PPT; ++q) {
                const float dx = ss_sub(v.x, px[q]), dy = ss_sub(v.y, py[q]), dz = ss_sub(v.z, pz[q]);
                const float d = ss_add(ss_add(ss_mul(dx, dx), ss_mul(dy, dy)), ss_mul(dz, dz));
                if (ok && d < bd[q]) { bd[q] = d; best[q] = base + j; }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < SL_PPT; ++q) {
        const int i = c * SL_PTS + q * SL_TPB + tid;
        if (i >= n || best[q] < 0) continue;
        const float* w = p.att + ((long)b * N + best[q]) * p.P;
        float top = w[0];
        int arg = 0;
        for (int k = 1; k < p.P; ++k) {
            const float x = w[k];
            if (x > top) { top = x; arg = k; }               // the first maximum wins
        }
        p.labels[(long)p0 + i] = arg;
    }
}

static inline long ss_round16(long v) { return (v + 15) & ~15L; }

extern "C" long gpe_scan_sample_ws_bytes(long B, int N, long n_max)
{
    if (B < 1 || B > GPE_SCAN_MAX_BATCH || N < 1 || N > GPE_SCAN_MAX_SAMPLES || n_max < 1 || n_max > GPE_SCAN_MAX_POINTS) return GPE_EINVAL;
    return 16 + ss_round16(B * 4) + B * (long)(SS_BINS * 4) + B * (long)(SS_SORT * 16);
}

extern "C" int gpe_scan_sample(const float* points4, const int32_t* off, int G, long n_max, const int32_t* index, int B, int N,
                               const float* shift_host, const float* scale_host, int narrow_above, void* ws, long ws_bytes,
                               uint64_t* state, uint32_t* ticket, float* features, int32_t* picked, int32_t* status, void* stream)
{
    static_assert(GPE_SCAN_MAX_SAMPLES * 2 == SS_SORT, "the sort's image holds N entries in front of the boundary bin and as many of it");
    if (!points4 || !off || !index || !ws || !state || !ticket || !features || !picked || !status || (!shift_host) != (!scale_host))
        return GPE_EINVAL;
    if ((((uintptr_t)points4) & 15) || (((uintptr_t)ws) & 15) || (((uintptr_t)state) & 7)) return GPE_EINVAL;
    if (G < 1 || narrow_above < 0) return GPE_EINVAL;
    const long need = gpe_scan_sample_ws_bytes(B, N, n_max);                         // checks B, N and n_max
    if (need < 0 || ws_bytes < need) return GPE_EINVAL;
    SsParams p;
    p.chunks = gpe_cdiv(n_max, SS_CHUNK);
    if ((long)B * p.chunks > 0x7fffffffL) return GPE_EINVAL;
    p.points = reinterpret_cast<const f32x4*>(points4); p.off = off; p.index = index;
    p.G = G; p.B = B; p.N = N; p.n_max = (int)n_max; p.narrow_above = narrow_above; p.standardize = shift_host ? 1 : 0;
    for (int a = 0; a < 3; ++a) {
        p.shift[a] = shift_host ? shift_host[a] : 0.f;
        p.scale[a] = scale_host ? scale_host[a] : 1.f;
    }
    p.state = reinterpret_cast<unsigned long long*>(state); p.ticket = ticket;
    char* w = static_cast<char*>(ws);
    p.ws_state = reinterpret_cast<unsigned long long*>(w);
    p.cnt = reinterpret_cast<unsigned*>(w + 16);
    p.hist = reinterpret_cast<unsigned*>(w + 16 + ss_round16((long)B * 4));
    p.cand = reinterpret_cast<gpe_u32x4*>(w + 16 + ss_round16((long)B * 4) + (long)B * SS_BINS * 4);
    p.features = features; p.picked = picked; p.status = status;
    const hipStream_t s = (hipStream_t)stream;
    // the list lengths and the tables start every call at zero
    if (hipMemsetAsync(p.cnt, 0, (size_t)(ss_round16((long)B * 4) + (long)B * SS_BINS * 4), s) != hipSuccess) return GPE_ELAUNCH;
    const dim3 grid((unsigned)((long)B * p.chunks));
    hipLaunchKernelGGL(gpe_scan_hist_kernel, grid, dim3(SS_TPB), 0, s, p);
    GPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(gpe_scan_collect_kernel, grid, dim3(SS_TPB), 0, s, p);
    GPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(gpe_scan_finish_kernel, dim3((unsigned)B), dim3(SS_FTPB), 0, s, p);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_scan_labels(const float* points4, const int32_t* off, int G, long n_max, const int32_t* index, int B, int N,
                               const int32_t* picked, const float* att_weights, int P, int32_t* labels, void* stream)
{
    if (!points4 || !off || !index || !picked || !att_weights || !labels) return GPE_EINVAL;
    if (((uintptr_t)points4) & 15) return GPE_EINVAL;
    if (G < 1 || B < 1 || B > GPE_SCAN_MAX_BATCH || N < 1 || N > GPE_SCAN_MAX_POINTS || P < 1 || P > 4096 || n_max < 1 ||
        n_max > GPE_SCAN_MAX_POINTS)
        return GPE_EINVAL;
    SlParams p;
    p.chunks = gpe_cdiv(n_max, SL_PTS);
    if ((long)B * p.chunks > 0x7fffffffL) return GPE_EINVAL;
    p.points = reinterpret_cast<const f32x4*>(points4); p.off = off; p.index = index; p.picked = picked; p.att = att_weights;
    p.G = G; p.B = B; p.N = N; p.P = P; p.n_max = (int)n_max; p.labels = labels;
    hipLaunchKernelGGL(gpe_scan_labels_kernel, dim3((unsigned)((long)B * p.chunks)), dim3(SL_TPB), 0, (hipStream_t)stream, p);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
