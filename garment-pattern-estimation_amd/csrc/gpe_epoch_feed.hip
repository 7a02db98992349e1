// Training epochs fed from the device (contract, random numbers and launch shapes: include/gpe_hip_feed.h).
//
//   gpe_batch_schedule_draw   the balanced batches of one epoch (BalancedBatchSampler.__iter__, nn/data/utils.py:54-89) in three
//                             launches: rank the garments of every class by their keys, walk over the batches (one wave: it keeps
//                             the per-class fill counts), shuffle the slots of every row
//   gpe_feed_next             the next row of the schedule -> the step's index, and the ground-truth rows of its garments gathered
//                             from resident tables: a one-workgroup prologue, which owns the cursor, and the gather
//
// Every decision is one Philox4x32-10 block keyed by the seed: a pure function of (seed, epoch, position or batch and slot), whatever
// the grid does.  No atomics, and no workgroup waits for another; what one launch leaves for the next is ordered by the stream.
#include "gpe_device.h"
#include <algorithm>

#define EF_TPB 256
#define EF_WS_HEAD 16           // bytes in front of the sorted ids: the walk's copy of {seed, epoch} for the shuffle

enum { EF_ORDER = 10, EF_FILL = 11, EF_SLOT = 12 };

__device__ __forceinline__ gpe_rng ef_rng(unsigned long long seed, unsigned long long epoch, unsigned b)
{
    return gpe_rng{(unsigned)seed, (unsigned)(seed >> 32), (unsigned)epoch, (unsigned)(epoch >> 32), b << 8};
}

__device__ __forceinline__ unsigned long long ef_key(const gpe_rng& rng, int kind, unsigned item)
{
    const gpe_u32x4 w = rng(kind, item);
    return ((unsigned long long)w.x << 32) | w.y;
}

__device__ __forceinline__ int ef_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- (1) order inside a class: sorted[class_off[c] + rank of (key, p) inside class c] = ids[p] -------------------------------------
// A workgroup takes 256 consecutive positions at a time; the keys of the classes they belong to pass through LDS in tiles of 256.
__global__ __launch_bounds__(EF_TPB) void gpe_schedule_rank_kernel(const int32_t* class_off, const int32_t* ids, int C, int G,
                                                                   const unsigned long long* state, int32_t* sorted)
{
    __shared__ unsigned long long s_key[EF_TPB];
    __shared__ int s_range[2];
    const int tid = threadIdx.x;
    const gpe_rng rng = ef_rng(state[0], state[1], 0u);
    for (int p0 = blockIdx.x * EF_TPB; p0 < G; p0 += gridDim.x * EF_TPB) {        // block-uniform
        const int p = p0 + tid, last = min(p0 + EF_TPB, G) - 1;
        int lo = 0, hi = 0;
        unsigned long long key = 0ull;
        if (p < G) {
            int a = 0, b = C;                                 // class_off[a] <= p < class_off[b]
            while (b - a > 1) {
                const int m = (a + b) >> 1;
                if (class_off[m] <= p) a = m; else b = m;
            }
            lo = ef_clamp(class_off[a], 0, p);
            hi = ef_clamp(class_off[a + 1], p + 1, G);
            key = ef_key(rng, EF_ORDER, (unsigned)p);
        }
        __syncthreads();                                      // the previous pass is done with s_range and s_key
        if (tid == 0) s_range[0] = lo;
        if (p == last) s_range[1] = hi;
        __syncthreads();
        const int qlo = s_range[0], qhi = s_range[1];
        int rank = 0;
        for (int q0 = qlo; q0 < qhi; q0 += EF_TPB) {
            if (q0 != qlo) __syncthreads();
            if (q0 + tid < qhi) s_key[tid] = ef_key(rng, EF_ORDER, (unsigned)(q0 + tid));
            __syncthreads();
            const int n = min(EF_TPB, qhi - q0);
            for (int i = 0; i < n; ++i) {                     // (every lane reads the same word: an LDS broadcast)
                const unsigned long long k = s_key[i];
                const int q = q0 + i;
                rank += (q >= lo && q < hi && (k < key || (k == key && q < p))) ? 1 : 0;
            }
        }
        if (p < G) sorted[lo + rank] = ids[p];                // rank < hi - lo: p itself is never counted
    }
}

// ---- (2) the walk over the batches: one wave ---------------------------------------------------------------------------------------
// Lane l owns the classes l, l + 64, ...: their fill counts live in LDS words that no other lane touches, so the wave needs no
// barrier; what the lanes share goes through ballots and shuffles.  Rows leave in pre-shuffle order.
__device__ __forceinline__ int ef_wave_scan(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d);
        v += lane >= d ? u : 0;
    }
    return v;
}

__global__ __launch_bounds__(64) void gpe_schedule_walk_kernel(const int32_t* class_off, const int32_t* quota, int C, int G, int B,
                                                               int nfull, int remainder, unsigned long long* state,
                                                               unsigned long long* state_copy, const int32_t* sorted, int32_t* table,
                                                               int32_t* batch_len)
{
    __shared__ int s_off[GPE_SCHEDULE_MAX_BATCH], s_size[GPE_SCHEDULE_MAX_BATCH], s_quota[GPE_SCHEDULE_MAX_BATCH],
        s_taken[GPE_SCHEDULE_MAX_BATCH];
    const int lane = threadIdx.x;
    const unsigned long long seed = state[0], epoch = state[1];
    for (int c = lane; c < C; c += 64) {
        const int off = ef_clamp(class_off[c], 0, G), end = ef_clamp(class_off[c + 1], off, G);
        s_off[c] = off; s_size[c] = end - off; s_quota[c] = max(quota[c], 0); s_taken[c] = 0;
    }
    for (int t = 0; t < nfull + remainder; ++t) {
        int32_t* row = table + (long)t * B;
        const bool rest = t == nfull;                         // the kept remainder: every garment left
        int len = 0;
        for (int c0 = 0; c0 < C; c0 += 64) {
            const int c = c0 + lane;
            int cnt = 0, from = 0;
            if (c < C) {
                const int left = s_size[c] - s_taken[c];
                cnt = rest ? left : min(s_quota[c], left);
                from = s_off[c] + s_taken[c];
                s_taken[c] += cnt;
            }
            const int incl = ef_wave_scan(cnt, lane), o = len + incl - cnt;
            for (int i = 0; i < cnt; ++i)
                if (o + i < B) row[o + i] = sorted[from + i];
            len += __shfl(incl, 63);
        }
        len = min(len, B);
        if (rest) {
            for (int j = len + lane; j < B; j += 64) row[j] = -1;
            if (lane == 0) batch_len[t] = len;
            break;
        }
        for (int j = len; j < B; ++j) {                       // the free slots, in order (wave-uniform control flow)
            int n = 0;
            for (int c0 = 0; c0 < C; c0 += 64) {
                const int c = c0 + lane;
                n += __popcll(__ballot(c < C && s_taken[c] < s_size[c]));
            }
            if (n == 0) {                                     // (G >= (t + 1) B garments: not reached with consistent arguments)
                if (lane == 0) row[j] = -1;
                continue;
            }
            int k = (int)__umulhi(ef_rng(seed, epoch, (unsigned)j)(EF_FILL, (unsigned)t).x, (unsigned)n);
            for (int c0 = 0; c0 < C; c0 += 64) {
                const int c = c0 + lane;
                const bool has = c < C && s_taken[c] < s_size[c];
                const unsigned long long m = __ballot(has);
                const int pc = __popcll(m);
                if (k < pc) {
                    if (has && __popcll(m & ((1ull << lane) - 1ull)) == k) {
                        row[j] = sorted[s_off[c] + s_taken[c]];
                        s_taken[c] += 1;
                    }
                    break;
                }
                k -= pc;
            }
        }
        if (lane == 0) batch_len[t] = B;
    }
    if (lane == 0) {
        state_copy[0] = seed;
        state_copy[1] = epoch;
        state[1] = epoch + 1ull;                              // the last store of the only workgroup that is running
    }
}

// ---- (3) slot shuffle: a workgroup per row, in place -------------------------------------------------------------------------------
__global__ __launch_bounds__(EF_TPB) void gpe_schedule_shuffle_kernel(const unsigned long long* state_copy, int B, int rows,
                                                                      const int32_t* batch_len, int32_t* table)
{
    __shared__ unsigned long long s_key[GPE_SCHEDULE_MAX_BATCH];
    __shared__ int32_t s_val[GPE_SCHEDULE_MAX_BATCH];
    const int tid = threadIdx.x;
    const unsigned long long seed = state_copy[0], epoch = state_copy[1];
    for (int t = blockIdx.x; t < rows; t += gridDim.x) {      // block-uniform
        int32_t* row = table + (long)t * B;
        const int len = ef_clamp(batch_len[t], 0, B);
        __syncthreads();                                      // the previous row's readers are done
        for (int s = tid; s < len; s += EF_TPB) {
            s_val[s] = row[s];
            s_key[s] = ef_key(ef_rng(seed, epoch, (unsigned)s), EF_SLOT, (unsigned)t);
        }
        __syncthreads();
        for (int s = tid; s < len; s += EF_TPB) {
            const unsigned long long key = s_key[s];
            int rank = 0;
            for (int q = 0; q < len; ++q) {
                const unsigned long long k = s_key[q];
                rank += (k < key || (k == key && q < s)) ? 1 : 0;
            }
            row[rank] = s_val[s];
        }
    }
}

static bool ef_range(long v, long lo, long hi) { return v >= lo && v <= hi; }

extern "C" long gpe_batch_schedule_rows(long G, int B, int drop_last)
{
    if (!ef_range(G, 1, GPE_SCHEDULE_MAX_GARMENTS) || !ef_range(B, 1, GPE_SCHEDULE_MAX_BATCH)) return GPE_EINVAL;
    return G / B + ((!drop_last && G % B) ? 1 : 0);
}

extern "C" long gpe_batch_schedule_ws_bytes(long G)
{
    if (!ef_range(G, 1, GPE_SCHEDULE_MAX_GARMENTS)) return GPE_EINVAL;
    return (EF_WS_HEAD + 4 * G + 15) & ~15L;
}

extern "C" int gpe_batch_schedule_draw(const int32_t* class_off, const int32_t* ids, const int32_t* quota, const int32_t* class_off_host,
                                       const int32_t* quota_host, int C, int G, int B, int drop_last, int64_t* state, void* ws,
                                       long ws_bytes, int32_t* table, int32_t* batch_len, void* stream)
{
    if (!class_off || !ids || !quota || !class_off_host || !quota_host || !state || !ws || !table || !batch_len) return GPE_EINVAL;
    if (!ef_range(G, 1, GPE_SCHEDULE_MAX_GARMENTS) || !ef_range(B, 1, GPE_SCHEDULE_MAX_BATCH) || C < 1 || C > B) return GPE_EINVAL;
    if ((drop_last & ~1) || (((uintptr_t)state) & 7) || (((uintptr_t)ws) & 15) || ws_bytes < gpe_batch_schedule_ws_bytes(G))
        return GPE_EINVAL;
    if (class_off_host[0] != 0 || class_off_host[C] != G) return GPE_EINVAL;
    long sum = 0;
    for (int c = 0; c < C; ++c) {
        if (class_off_host[c + 1] < class_off_host[c] || quota_host[c] < 0) return GPE_EINVAL;
        sum += quota_host[c];
    }
    if (sum > B) return GPE_EINVAL;
    const int nfull = G / B, remainder = (!drop_last && G % B) ? 1 : 0, rows = nfull + remainder;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(state);
    unsigned long long* copy = reinterpret_cast<unsigned long long*>(ws);
    int32_t* sorted = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + EF_WS_HEAD);
    const int cap = 4 * std::max(gpe_num_cus(), 1);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gpe_schedule_rank_kernel, dim3(std::min(gpe_cdiv(G, EF_TPB), cap)), dim3(EF_TPB), 0, s, class_off, ids, C, G, st, sorted);
    GPE_CHECK_LAUNCH();
    // (fewer garments than one batch and none kept: no row, but the epoch still advances)
    hipLaunchKernelGGL(gpe_schedule_walk_kernel, dim3(1), dim3(64), 0, s, class_off, quota, C, G, B, nfull, remainder, st, copy, sorted,
                       table, batch_len);
    GPE_CHECK_LAUNCH();
    if (rows > 0) {
        hipLaunchKernelGGL(gpe_schedule_shuffle_kernel, dim3(std::min(rows, cap)), dim3(EF_TPB), 0, s, copy, B, rows, batch_len, table);
        GPE_CHECK_LAUNCH();
    }
    return GPE_OK;
}

// ---- the per-step feed -------------------------------------------------------------------------------------------------------------
// prologue: the one workgroup that reads and writes the cursor
__global__ __launch_bounds__(EF_TPB) void gpe_feed_prologue_kernel(const int32_t* table, long rows, int B, long long* cursor, int G,
                                                                   int32_t* index_out, int32_t* status)
{
    __shared__ int s_bad[EF_TPB / 64];
    const int tid = threadIdx.x;
    const long long cur = *cursor;
    long r = (long)(cur % rows);
    r += r < 0 ? rows : 0;
    int bad = 0;
    for (int b = tid; b < B; b += EF_TPB) {
        const int g = table[r * B + b];
        index_out[b] = g;
        bad += (g < 0 || g >= G) ? 1 : 0;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) bad += __shfl_down(bad, d);
    if ((tid & 63) == 0) s_bad[tid >> 6] = bad;
    __syncthreads();                                          // every thread has read the cursor
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < EF_TPB / 64; ++w) total += s_bad[w];
        status[0] = total;
        *cursor = cur + 1;
    }
}

// gather: workgroup (b, j) copies one row of table j
__global__ void gpe_feed_gather_kernel(const long long* jobs, const int32_t* index, int G)
{
    const int b = blockIdx.x, j = blockIdx.y;
    const long nb = jobs[3 * j + 2];
    const int g = index[b];
    const bool ok = g >= 0 && g < G;
    const char* src = reinterpret_cast<const char*>(jobs[3 * j]) + (ok ? (long)g * nb : 0);
    char* dst = reinterpret_cast<char*>(jobs[3 * j + 1]) + (long)b * nb;
    if (!(nb & 15) && !((((uintptr_t)src) | ((uintptr_t)dst)) & 15)) {
        const gpe_u32x4* s4 = reinterpret_cast<const gpe_u32x4*>(src);
        gpe_u32x4* d4 = reinterpret_cast<gpe_u32x4*>(dst);
        for (long i = threadIdx.x; i < (nb >> 4); i += blockDim.x) d4[i] = ok ? s4[i] : gpe_u32x4{0u, 0u, 0u, 0u};
    } else {
        const unsigned* s1 = reinterpret_cast<const unsigned*>(src);
        unsigned* d1 = reinterpret_cast<unsigned*>(dst);
        for (long i = threadIdx.x; i < (nb >> 2); i += blockDim.x) d1[i] = ok ? s1[i] : 0u;
    }
}

#define EF_MAX_ROW_BYTES (1L << 24)

extern "C" int gpe_feed_jobs(int T, const void* const* src, void* const* dst, const long* row_bytes, int64_t* jobs_host)
{
    if (!src || !dst || !row_bytes || !jobs_host || T < 1 || T > GPE_FEED_MAX_TABLES) return GPE_EINVAL;
    for (int j = 0; j < T; ++j)
        if (!src[j] || !dst[j] || ((((uintptr_t)src[j]) | ((uintptr_t)dst[j])) & 3) || row_bytes[j] < 4 || (row_bytes[j] & 3) ||
            row_bytes[j] > EF_MAX_ROW_BYTES)
            return GPE_EINVAL;
    for (int j = 0; j < T; ++j) {
        jobs_host[3 * j] = (int64_t)(uintptr_t)src[j];
        jobs_host[3 * j + 1] = (int64_t)(uintptr_t)dst[j];
        jobs_host[3 * j + 2] = row_bytes[j];
    }
    return GPE_OK;
}

extern "C" int gpe_feed_next(const int32_t* table, long rows, int B, int64_t* cursor, int G, const int64_t* jobs, int T,
                             long max_row_bytes, int32_t* index_out, int32_t* status, void* stream)
{
    if (!table || !cursor || !index_out || !status || (((uintptr_t)cursor) & 7)) return GPE_EINVAL;
    if (rows < 1 || !ef_range(B, 1, GPE_SCHEDULE_MAX_BATCH) || G < 1 || T < 0 || T > GPE_FEED_MAX_TABLES) return GPE_EINVAL;
    if (T > 0 && (!jobs || (((uintptr_t)jobs) & 7) || max_row_bytes < 4 || (max_row_bytes & 3) || max_row_bytes > EF_MAX_ROW_BYTES))
        return GPE_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gpe_feed_prologue_kernel, dim3(1), dim3(EF_TPB), 0, s, table, rows, B, reinterpret_cast<long long*>(cursor), G,
                       index_out, status);
    GPE_CHECK_LAUNCH();
    if (T > 0) {
        const int tpb = (int)std::min(256L, std::max(64L, (max_row_bytes / 16 + 63) / 64 * 64));      // a thread per 16 bytes of the widest row
        hipLaunchKernelGGL(gpe_feed_gather_kernel, dim3(B, T), dim3(tpb), 0, s, reinterpret_cast<const long long*>(jobs), index_out, G);
        GPE_CHECK_LAUNCH();
    }
    return GPE_OK;
}
