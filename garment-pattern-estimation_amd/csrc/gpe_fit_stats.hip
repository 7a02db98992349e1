// Standardisation statistics of a resident data set (include/gpe_hip_fit.h): per-column mean / population std and min / max /
// norm_scale over the rows of x [S, N, C], optionally without the all-zero padding rows — what
//   GarmentBaseDataset._get_distribution_stats / _get_norm_stats / _unpad (nn/data/datasets.py:524-568)
// give on one collated batch of the whole training set on the host.
// Two stages, no atomics, no workgroup waits on another, fp64 sums in a fixed order: gpe_fit_part writes one record per LEAF of 512
// rows, gpe_fit_finish (one workgroup) merges the records with Chan's pairwise update.  Bandwidth-bound small work: no MFMA, no
// LDS beyond the reductions.  No process state: everything lives in the caller's part image and result block.
#include "gpe_common.h"
#include <math.h>

#define FIT_TPB 256
#define FIT_LEAF 512               // rows per leaf (a thread of the leaf kernel holds at most 32 values of one column)
#define FIT_MAX_C 16
#define FIT_FIN_TPB 1024
#define FIT_FIN_UNROLL 4

extern "C" long gpe_fit_leaves(long sets, long rows_per_set)
{
    if (sets <= 0 || rows_per_set <= 0) return GPE_EINVAL;
    const long per_set = (rows_per_set - 1) / FIT_LEAF + 1;
    if (sets > INT64_MAX / per_set) return GPE_EINVAL;
    return sets * per_set;
}

// min / max as IEEE 754-2019 minimum / maximum: a NaN is carried on (torch.min / torch.max; fmin / fmax would drop it) and -0 < +0, so
// that the result does not depend on the order in which the zeros of a column are met
__device__ __forceinline__ double fit_min(double a, double b)
{
    if (a != a || b != b) return (double)NAN;
    return (a < b || (a == b && signbit(a))) ? a : b;
}
__device__ __forceinline__ double fit_max(double a, double b)
{
    if (a != a || b != b) return (double)NAN;
    return (a > b || (a == b && !signbit(a))) ? a : b;
}

// Inside a leaf the extremes are kept as integer KEYS of the fp32 values: key = bits ^ ((bits >> 31) & 0x7fffffff) orders like the
// floats under a signed integer compare, with -0 below +0, a NaN with the sign bit clear above +inf and one with it set below
// -inf — so min / max are one integer instruction each, without a branch, and a NaN is found at the end from the two extremes.
#define FIT_KEY_PINF 0x7f800000                  // key(+inf): the identity of min
#define FIT_KEY_NINF ((int)0x807fffff)           // key(-inf): the identity of max
__device__ __forceinline__ int fit_key(float v)
{
    const int bits = __float_as_int(v);
    return bits ^ ((bits >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float fit_unkey(int key) { return __int_as_float(key ^ ((key >> 31) & 0x7fffffff)); }

// WPL waves per leaf, 4 / WPL leaves per workgroup at a time.  CP = C rounded up to a power of two.  Thread t of a leaf's 64 WPL holds
// column c = t % CP of the rows j + k * NSL, j = t / CP, NSL = 64 WPL / CP, k = 0 .. 512 / NSL - 1 (at most 32: one bit each in the
// row masks): for a fixed k the leaf's threads read one contiguous run of NSL rows (lanes with c >= C idle), and a wave has all
// its loads in flight before the first sum.  With WPL = 1 (C <= 4: the point clouds) a leaf is one wave's: no LDS, no barrier.
// Sums: the thread's rows in the order of k, then the threads of a column by a fixed shuffle tree inside each wave (lane l with lane
// l + 32, 16, ... CP), then the leaf's waves in wave order.
// (Three waves per SIMD: left alone the compiler takes 200 VGPRs and two waves, asked for four it spills.)
template <int CP, int WPL>
__global__ __launch_bounds__(FIT_TPB, 3) void gpe_fit_part_kernel(const float* __restrict__ x, long N, int C, long per_set,
                                                               long leaves, int skip_zero_rows, double* __restrict__ part)
{
    constexpr int WAVES = FIT_TPB / 64;
    constexpr int LPB = WAVES / WPL;               // leaves of a workgroup's turn
    constexpr int NSL = 64 * WPL / CP;             // row slices of a leaf
    constexpr int RPT = FIT_LEAF / NSL;            // rows per thread
    static_assert(RPT <= 32 && RPT * NSL == FIT_LEAF && LPB * WPL == WAVES, "one mask bit per row of a thread");
    __shared__ double red_sum[WAVES][CP], red_m2[WAVES][CP];
    __shared__ int red_min[WAVES][CP], red_max[WAVES][CP];
    __shared__ int red_cnt[WAVES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = wave / WPL, w0 = q * WPL;        // the leaf of this wave within the turn, and the leaf's first wave
    const int t = (wave - w0) * 64 + lane;
    const int c = t & (CP - 1), j = t / CP;
    const bool col = c < C;
    const unsigned off0 = (unsigned)(j * C + c), stride = (unsigned)(NSL * C);         // floats from the leaf's first (< 8192)
    for (long turn = blockIdx.x; turn * LPB < leaves; turn += gridDim.x) {
        const long leaf = turn * LPB + q;
        const bool live = leaf < leaves;           // (wave-uniform; a workgroup's waves run the same number of turns)
        int rows = 0;
        const float* base = x;
        if (live) {
            const long s = leaf / per_set, b = leaf - s * per_set;
            const long row0 = b * FIT_LEAF;
            rows = (int)(N - row0 < FIT_LEAF ? N - row0 : FIT_LEAF);
            base = x + (s * N + row0) * C;
        }
        float v[RPT];
        unsigned valid = 0, small = 0;
        // every load is issued (a lane without a value reads the leaf's first float, which exists) and sorted out afterwards: no
        // branch between the loads, a uniform base and a 32-bit byte offset per lane
        const char* bytes = reinterpret_cast<const char*>(base);
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const bool has = col && j + k * NSL < rows;
            v[k] = *reinterpret_cast<const float*>(bytes + (has ? 4u * (off0 + k * stride) : 0u));
        }
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const bool has = col && j + k * NSL < rows;
            v[k] = has ? v[k] : 0.f;
            valid |= (j + k * NSL < rows ? 1u : 0u) << k;
            small |= ((!col || fabsf(v[k]) <= 1e-5f) ? 1u : 0u) << k;
        }
        // a row is dropped iff it is small in every column: AND over the CP lanes that share the row slice
#pragma unroll
        for (int m = 1; m < CP; m <<= 1) small &= (unsigned)__shfl_xor((int)small, m);
        const unsigned keep = skip_zero_rows ? (valid & ~small) : valid;

        // branch-free: a dropped value adds an exact 0 and offers the identities
        double sum = 0.0;
        int mn = FIT_KEY_PINF, mx = FIT_KEY_NINF;
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const bool kept = (keep >> k) & 1u;
            const int key = fit_key(v[k]);
            sum += (double)(kept ? v[k] : 0.f);
            mn = min(mn, kept ? key : FIT_KEY_PINF);
            mx = max(mx, kept ? key : FIT_KEY_NINF);
        }
        int cnt = c == 0 ? __popc(keep) : 0;
#pragma unroll
        for (int off = 32; off >= CP; off >>= 1) {
            sum += __shfl_down(sum, off);
            mn = min(mn, __shfl_down(mn, off));
            mx = max(mx, __shfl_down(mx, off));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
        int n;
        double total;
        if (WPL == 1) {                                // lane c holds column c's sums
            n = __shfl(cnt, 0);
            total = __shfl(sum, c);
            mn = __shfl(mn, c);
            mx = __shfl(mx, c);
        } else {
            __syncthreads();                           // (the previous turn's reads of red_*[] are over)
            if (lane < CP) {
                red_sum[wave][c] = sum;
                red_min[wave][c] = mn;
                red_max[wave][c] = mx;
            }
            if (lane == 0) red_cnt[wave] = cnt;
            __syncthreads();
            n = red_cnt[w0];
            total = red_sum[w0][c];
            mn = red_min[w0][c];
            mx = red_max[w0][c];
#pragma unroll
            for (int w = 1; w < WPL; ++w) {
                n += red_cnt[w0 + w];
                total += red_sum[w0 + w][c];
                mn = min(mn, red_min[w0 + w][c]);
                mx = max(mx, red_max[w0 + w][c]);
            }
        }
        const double mean = n > 0 ? total / (double)n : 0.0;

        double m2 = 0.0;
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const double d = ((keep >> k) & 1u) ? (double)v[k] - mean : 0.0;
            m2 += d * d;
        }
#pragma unroll
        for (int off = 32; off >= CP; off >>= 1) m2 += __shfl_down(m2, off);
        if (WPL > 1) {
            if (lane < CP) red_m2[wave][c] = m2;
            __syncthreads();
            m2 = red_m2[w0][c];
#pragma unroll
            for (int w = 1; w < WPL; ++w) m2 += red_m2[w0 + w][c];
        }
        if (live && t < CP && col) {                   // (WPL == 1: lane c's own tree result is column c's)
            double* rec = part + leaf * (1 + 4 * C);
            if (t == 0) rec[0] = (double)n;
            rec[1 + 4 * c + 0] = mean;
            rec[1 + 4 * c + 1] = m2;
            const bool nan = mn < FIT_KEY_NINF || mx > FIT_KEY_PINF;       // a NaN marks both extremes (torch.min / torch.max)
            rec[1 + 4 * c + 2] = nan ? (double)NAN : (double)fit_unkey(mn);
            rec[1 + 4 * c + 3] = nan ? (double)NAN : (double)fit_unkey(mx);
        }
    }
}

struct FitAcc { double n, mean, m2, mn, mx; };

// Chan's pairwise update; a is the part that comes first in the leaf order.  An empty part leaves the other as it is.
__device__ __forceinline__ FitAcc fit_merge(const FitAcc a, const FitAcc b)
{
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    FitAcc o;
    o.n = a.n + b.n;
    const double d = b.mean - a.mean;
    o.mean = a.mean + d * b.n / o.n;
    o.m2 = a.m2 + b.m2 + d * d * a.n * b.n / o.n;
    o.mn = fit_min(a.mn, b.mn);
    o.mx = fit_max(a.mx, b.mx);
    return o;
}

// One workgroup.  CP = C rounded up to a power of two; thread t works on column c = t % CP for the leaf slot t / CP of 1024 / CP: the
// lanes of a slot read one record together, consecutive slots consecutive records (a thread per record and a pass per column had
// every load of a wave touch 64 cache lines: 300 us for 65536 leaves, all of it in the one CU's address unit).
// Order: a thread folds the leaves slot, slot + 1024 / CP, ... in that order; the threads of a column are combined by a fixed shuffle
// tree inside each wave (lane l with lane l + 32, 16, ... CP), the 16 waves in wave order.
template <int CP>
__global__ __launch_bounds__(FIT_FIN_TPB) void gpe_fit_finish_kernel(const double* __restrict__ part, long leaves, int C,
                                                                     double* __restrict__ result)
{
    constexpr int SLOTS = FIT_FIN_TPB / CP;
    __shared__ FitAcc sh[FIT_FIN_TPB / 64][CP];
    __shared__ int flags[CP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = tid & (CP - 1), slot = tid / CP;
    const bool col = c < C;
    const long rec = 1 + 4 * C;
    const int fc = col ? 1 + 4 * c : 1;                // (an idle lane reads column 0 and is never looked at)
    FitAcc acc = {0.0, 0.0, 0.0, INFINITY, -INFINITY};
    for (long i0 = slot; i0 < leaves; i0 += (long)SLOTS * FIT_FIN_UNROLL) {
        FitAcc b[FIT_FIN_UNROLL];                       // the loads of several records in flight, folded in leaf order
#pragma unroll
        for (int u = 0; u < FIT_FIN_UNROLL; ++u) {
            const long i = i0 + (long)u * SLOTS;
            const double* p = part + (i < leaves ? i : 0) * rec;
            b[u] = {i < leaves ? p[0] : 0.0, p[fc], p[fc + 1], p[fc + 2], p[fc + 3]};          // n = 0: skipped
        }
#pragma unroll
        for (int u = 0; u < FIT_FIN_UNROLL; ++u) acc = fit_merge(acc, b[u]);
    }
#pragma unroll
    for (int off = 32; off >= CP; off >>= 1) {
        FitAcc b;
        b.n = __shfl_down(acc.n, off);
        b.mean = __shfl_down(acc.mean, off);
        b.m2 = __shfl_down(acc.m2, off);
        b.mn = __shfl_down(acc.mn, off);
        b.mx = __shfl_down(acc.mx, off);
        acc = fit_merge(acc, b);                       // (lanes whose partner lies past the wave fold themselves: never read)
    }
    if (lane < CP) sh[wave][c] = acc;
    __syncthreads();
    if (tid < CP && col) {
        FitAcc t = sh[0][c];
        for (int w = 1; w < FIT_FIN_TPB / 64; ++w) t = fit_merge(t, sh[w][c]);
        int status = 0;
        double mean = t.mean, sd, mn = t.mn, mx = t.mx, scale;
        if (t.n == 0.0) {
            status |= 1;
            mean = sd = mn = mx = scale = (double)NAN;
        } else {
            if (!isfinite(mn) || !isfinite(mx)) status |= 2;
            const double m2 = t.m2 < 0.0 ? 0.0 : t.m2;
            sd = mn == mx ? 0.0 : sqrt(m2 / t.n);
            if (fabs(mn - mx) <= 1e-8 + 1e-5 * fabs(mx)) scale = fabs(mn) <= 1e-8 ? 1.0 : mn;
            else scale = mx - mn;
        }
        if (c == 0) result[0] = t.n;
        result[2 + c] = mean;
        result[2 + C + c] = sd;
        result[2 + 2 * C + c] = mn;
        result[2 + 3 * C + c] = mx;
        result[2 + 4 * C + c] = scale;
        flags[c] = status;
    }
    __syncthreads();
    if (tid == 0) {
        int status = 0;
        for (int k = 0; k < C; ++k) status |= flags[k];
        result[1] = (double)status;
    }
}

extern "C" int gpe_fit_part(const float* x, long sets, long rows_per_set, int C, int skip_zero_rows, long leaf0, long total_leaves,
                            double* part, void* stream)
{
    if (!x || !part || C < 1 || C > FIT_MAX_C || leaf0 < 0 || total_leaves <= 0 || (((uintptr_t)x) & 3) || (((uintptr_t)part) & 7))
        return GPE_EINVAL;
    const long leaves = gpe_fit_leaves(sets, rows_per_set);
    if (leaves <= 0 || leaves > total_leaves || leaf0 > total_leaves - leaves) return GPE_EINVAL;
    if (sets > INT64_MAX / rows_per_set || sets * rows_per_set > INT64_MAX / (4 * FIT_MAX_C)) return GPE_EINVAL;
    if (total_leaves > INT64_MAX / (8 * (1 + 4 * FIT_MAX_C))) return GPE_EINVAL;
    const int wpl = C <= 4 ? 1 : (C <= 8 ? 2 : 4);                  // waves per leaf: at most 32 values of the leaf per thread
    const long turns = (leaves - 1) / (FIT_TPB / 64 / wpl) + 1;
    const long cap = 8L * gpe_num_cus();
    const int grid = (int)(turns < cap ? turns : cap);
    const long per_set = leaves / sets;
    double* out = part + leaf0 * (1 + 4 * C);
    const dim3 g(grid > 0 ? grid : 1), t(FIT_TPB);
    const int skip = skip_zero_rows ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    if (C == 1) hipLaunchKernelGGL((gpe_fit_part_kernel<1, 1>), g, t, 0, st, x, rows_per_set, C, per_set, leaves, skip, out);
    else if (C == 2) hipLaunchKernelGGL((gpe_fit_part_kernel<2, 1>), g, t, 0, st, x, rows_per_set, C, per_set, leaves, skip, out);
    else if (C <= 4) hipLaunchKernelGGL((gpe_fit_part_kernel<4, 1>), g, t, 0, st, x, rows_per_set, C, per_set, leaves, skip, out);
    else if (C <= 8) hipLaunchKernelGGL((gpe_fit_part_kernel<8, 2>), g, t, 0, st, x, rows_per_set, C, per_set, leaves, skip, out);
    else hipLaunchKernelGGL((gpe_fit_part_kernel<16, 4>), g, t, 0, st, x, rows_per_set, C, per_set, leaves, skip, out);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_fit_finish(const double* part, long leaves, int C, double* result, void* stream)
{
    if (!part || !result || leaves <= 0 || C < 1 || C > FIT_MAX_C || (((uintptr_t)part | (uintptr_t)result) & 7) ||
        leaves > INT64_MAX / (8 * (1 + 4 * FIT_MAX_C)))
        return GPE_EINVAL;
    const dim3 g(1), t(FIT_FIN_TPB);
    hipStream_t st = (hipStream_t)stream;
    if (C == 1) hipLaunchKernelGGL(gpe_fit_finish_kernel<1>, g, t, 0, st, part, leaves, C, result);
    else if (C == 2) hipLaunchKernelGGL(gpe_fit_finish_kernel<2>, g, t, 0, st, part, leaves, C, result);
    else if (C <= 4) hipLaunchKernelGGL(gpe_fit_finish_kernel<4>, g, t, 0, st, part, leaves, C, result);
    else if (C <= 8) hipLaunchKernelGGL(gpe_fit_finish_kernel<8>, g, t, 0, st, part, leaves, C, result);
    else hipLaunchKernelGGL(gpe_fit_finish_kernel<16>, g, t, 0, st, part, leaves, C, result);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
