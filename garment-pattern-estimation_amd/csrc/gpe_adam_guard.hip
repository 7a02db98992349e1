// The guarded Adam step (include/gpe_hip_ext.h): the global L2 norm of the gradient arena and its per-segment norms in one pass,
// the clip factor, the skip flag (non-finite norm / an fp16 activation word at its limit) and two counters in a 32-byte device
// block, and a copy of the Adam kernel of gpe_adam.hip that scales the gradient by the factor and leaves p, m, v alone when the
// flag is set.  Nothing is read on the host, so the whole of it can sit inside a captured step.
//   torch.nn.utils.clip_grad_norm_ + torch.optim.Adam (nn/trainer.py:162-185; the reference itself only notices a NaN loss at the
//   end of an epoch, nn/trainer.py:220)
// Bandwidth-bound small work: no MFMA, no LDS beyond the reductions, no float atomics, no workgroup waits on another.
// STEP NUMBERS: a skipped step keeps its number — the host advances the schedule and the bias-correction exponent regardless and
// never reads the flag (the header has the full statement).
#include "gpe_common.h"
#include <math.h>

#define GN_TPB 256
#define GN_SLOT 2048               // floats per slot: two float4 per thread of a 256-thread workgroup
#define GN_MAX_SEG 4096
#define GN_MAX_RUNS 16
#define GN_MAX_WORDS 8
#define GN_FIN_TPB 1024

struct GpeAdamGuard {              // the guard block of the header
    float norm, coef;
    int skip, reserved;
    long long steps, skipped;
};
static_assert(sizeof(GpeAdamGuard) == 32, "the guard block is 32 bytes");

extern "C" long gpe_grad_norm_slots(const long* seg_end_host, int nseg, long* seg_slot_host)
{
    if (!seg_end_host || !seg_slot_host || nseg <= 0 || nseg > GN_MAX_SEG) return GPE_EINVAL;
    long prev = 0, slots = 0;
    for (int j = 0; j < nseg; ++j) {
        const long e = seg_end_host[j];
        if (e <= prev || (e & 3)) return GPE_EINVAL;
        seg_slot_host[j] = slots;
        slots += (e - prev + GN_SLOT - 1) / GN_SLOT;
        prev = e;
    }
    seg_slot_host[nseg] = slots;
    return slots;
}

// fixed-shape sum over the 256 threads of a workgroup: shuffle tree inside each wave, then the four waves in wave order
__device__ __forceinline__ double gn_block_sum(double acc, double* red /* [GN_TPB / 64] */)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                   // (the previous slot's read of red[] is over)
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ double gn_sq4(double acc, const float4 v)
{
    acc += (double)v.x * (double)v.x;
    acc += (double)v.y * (double)v.y;
    acc += (double)v.z * (double)v.z;
    acc += (double)v.w * (double)v.w;
    return acc;
}

__global__ __launch_bounds__(GN_TPB) void gpe_grad_norm_part_kernel(const float* __restrict__ g, long n,
                                                                    const long* __restrict__ seg_end,
                                                                    const long* __restrict__ seg_slot, int seg_lo, int seg_hi,
                                                                    long total_slots, double* __restrict__ part)
{
    __shared__ double red[GN_TPB / 64];
    const int tid = threadIdx.x;
    long s0 = seg_slot[seg_lo], s1 = seg_slot[seg_hi];
    if (s0 < 0) s0 = 0;                                // whatever the tables hold, part[] is written inside [0, total_slots)
    if (s1 > total_slots) s1 = total_slots;
    int j = seg_lo;
    for (long s = s0 + blockIdx.x; s < s1; s += gridDim.x) {
        // the segment of slot s: the largest j with seg_slot[j] <= s (s only grows: the search continues from the previous answer)
        int lo = j, hi = seg_hi - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (seg_slot[mid] <= s) lo = mid; else hi = mid - 1;
        }
        j = lo;
        long start = (j > 0 ? seg_end[j - 1] : 0) + (s - seg_slot[j]) * GN_SLOT;
        long end = seg_end[j];
        if (start < 0) start = 0;                      // ... and g[] is read inside [0, n)
        if (end > n) end = n;
        if (end > start + GN_SLOT) end = start + GN_SLOT;
        double acc = 0.0;
        if (end - start == GN_SLOT) {                  // a full slot (uniform): both loads in flight before the arithmetic
            const float4 a = *reinterpret_cast<const float4*>(g + start + 4 * tid);
            const float4 b = *reinterpret_cast<const float4*>(g + start + 4 * (tid + GN_TPB));
            acc = gn_sq4(gn_sq4(acc, a), b);
        } else {
#pragma unroll
            for (int q = 0; q < GN_SLOT / (4 * GN_TPB); ++q) {
                const long i = start + 4 * (long)(tid + q * GN_TPB);
                if (i + 3 < end)
                    acc = gn_sq4(acc, *reinterpret_cast<const float4*>(g + i));
                else
                    for (long e = i; e < end; ++e) acc += (double)g[e] * (double)g[e];
            }
        }
        const double tot = gn_block_sum(acc, red);
        if (tid == 0) part[s] = tot;
    }
}

struct GnFinish {
    int nruns, nwords;
    int runs[2 * GN_MAX_RUNS];
    const unsigned* words[GN_MAX_WORDS];
};

__global__ __launch_bounds__(GN_FIN_TPB) void gpe_grad_norm_finish_kernel(const double* __restrict__ part,
                                                                          const long* __restrict__ seg_slot, int nseg,
                                                                          long total_slots, GnFinish f, float gscale,
                                                                          float max_norm, int nonfinite_skip, float limit,
                                                                          float* __restrict__ seg_norm, int reversed,
                                                                          GpeAdamGuard* __restrict__ guard)
{
    __shared__ double sq[GN_MAX_SEG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double ags = fabs((double)gscale);
    // one wave per segment: lane l adds the slots l, l + 64, ... of the segment in that order, then the fixed shuffle tree
    for (int j = wave; j < nseg; j += GN_FIN_TPB / 64) {
        bool live = false;
        for (int r = 0; r < f.nruns; ++r) live = live || (j >= f.runs[2 * r] && j < f.runs[2 * r + 1]);
        double acc = 0.0;
        if (live) {
            long a = seg_slot[j], b = seg_slot[j + 1];
            if (a < 0) a = 0;
            if (b > total_slots) b = total_slots;
            for (long t = a + lane; t < b; t += 64) acc += part[t];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
        if (lane == 0) {
            sq[j] = acc;
            if (seg_norm) seg_norm[reversed ? nseg - 1 - j : j] = (float)(ags * sqrt(acc));
        }
    }
    __syncthreads();
    if (tid != 0) return;
    double total = 0.0;
    for (int j = 0; j < nseg; ++j) total += sq[j];     // segment order
    const float norm = (float)(ags * sqrt(total));
    float coef = 1.f;
    if (max_norm > 0.f) {
        const double c = (double)max_norm / ((double)norm + 1e-6);
        coef = c < 1.0 ? (float)c : 1.f;
    }
    int skip = (nonfinite_skip && !isfinite(norm)) ? 1 : 0;
    for (int w = 0; w < f.nwords; ++w) {
        const float v = __uint_as_float(*f.words[w]);
        if (!(v < limit)) skip = 1;                    // >= limit, or NaN
    }
    guard->norm = norm;
    guard->coef = coef;
    guard->skip = skip;
    guard->reserved = 0;
    guard->steps = guard->steps + 1;
    guard->skipped = guard->skipped + skip;
}

extern "C" int gpe_grad_norm_part(const float* g, long n, const long* seg_end, const long* seg_slot, int nseg, int seg_lo,
                                  int seg_hi, long total_slots, double* part, void* stream)
{
    if (!g || !seg_end || !seg_slot || !part || n <= 0 || nseg <= 0 || nseg > GN_MAX_SEG || seg_lo < 0 || seg_lo >= seg_hi ||
        seg_hi > nseg || total_slots <= 0 || (((uintptr_t)g) & 15) ||
        (((uintptr_t)seg_end | (uintptr_t)seg_slot | (uintptr_t)part) & 7))
        return GPE_EINVAL;
    // at most this many slots lie in the run (every segment ends one partly filled slot at the most)
    long slots = (n + GN_SLOT - 1) / GN_SLOT + (seg_hi - seg_lo);
    if (slots > total_slots) slots = total_slots;
    const long cap = 4L * gpe_num_cus();
    const int grid = (int)(slots < cap ? slots : cap);
    hipLaunchKernelGGL(gpe_grad_norm_part_kernel, dim3(grid > 0 ? grid : 1), dim3(GN_TPB), 0, (hipStream_t)stream, g, n, seg_end,
                       seg_slot, seg_lo, seg_hi, total_slots, part);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_grad_norm_finish(const double* part, const long* seg_slot, int nseg, long total_slots, const int* runs_host,
                                    int nruns, float gscale, float max_norm, int nonfinite_skip, const void* const* words_host,
                                    int nwords, float limit, float* seg_norm, int reversed, void* guard, void* stream)
{
    if (!part || !seg_slot || !runs_host || !guard || nseg <= 0 || nseg > GN_MAX_SEG || total_slots <= 0 || nruns <= 0 ||
        nruns > GN_MAX_RUNS || nwords < 0 || nwords > GN_MAX_WORDS || (nwords > 0 && !words_host) ||
        (((uintptr_t)part | (uintptr_t)seg_slot) & 7) || (((uintptr_t)guard) & 15) || (((uintptr_t)seg_norm) & 3))
        return GPE_EINVAL;
    GnFinish f;
    f.nruns = nruns;
    f.nwords = nwords;
    int prev = 0;
    for (int r = 0; r < GN_MAX_RUNS; ++r) {
        const int lo = r < nruns ? runs_host[2 * r] : 0, hi = r < nruns ? runs_host[2 * r + 1] : 0;
        if (r < nruns) {
            if (lo < prev || lo >= hi || hi > nseg) return GPE_EINVAL;
            prev = hi;
        }
        f.runs[2 * r] = lo;
        f.runs[2 * r + 1] = hi;
    }
    for (int w = 0; w < GN_MAX_WORDS; ++w) {
        const void* p = w < nwords ? words_host[w] : nullptr;
        if (w < nwords && (!p || (((uintptr_t)p) & 3))) return GPE_EINVAL;
        f.words[w] = static_cast<const unsigned*>(p);
    }
    hipLaunchKernelGGL(gpe_grad_norm_finish_kernel, dim3(1), dim3(GN_FIN_TPB), 0, (hipStream_t)stream, part, seg_slot, nseg,
                       total_slots, f, gscale, max_norm, nonfinite_skip ? 1 : 0, limit, seg_norm, reversed ? 1 : 0,
                       static_cast<GpeAdamGuard*>(guard));
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// =====================================================================================================================
// gpe_adam_kernel (gpe_adam.hip) under the guard block.  That kernel is compiled with the default floating-point contraction, and
// what the compiler fused there is part of its result; the roundings are therefore PINNED here — contraction off, every fused
// multiply-add written out — to the ones its gfx950 code performs:
//   gr = fma(gs, g, wd * p)        m = fma(b1, m, (1 - b1) * gr)        sq = ((1 - b2) * gr) * gr
//   fused:    v = fma(b2, v, sq)       p -= (lr' * m) / fma(rs, sqrt(v), eps)
//   unfused:  v = b2 * v + sq          p -= (lr' * m) / (rs * sqrt(v) + eps)
// The float4 body is fused.  The scalar tail (n % 4 != 0, never the case for an arena) was vectorised by two there: its pairs are
// fused, the last element of an odd tail is not.  tests/test_gpu_adam_guard.py holds the two kernels bit-equal (coef == 1) for a
// multiple of four and for every tail length, with and without weight decay.
// =====================================================================================================================
struct AdamScalars { float lr_over_bc1, b1, b2, c1, c2, eps, wd, rsqrt_bc2, gs; };

template <bool FUSED>
__device__ __forceinline__ void adam_guarded_elem(const AdamScalars& a, float& p, const float g, float& m, float& v)
{
#pragma clang fp contract(off)
    const float gr = __builtin_fmaf(a.gs, g, a.wd * p);
    m = __builtin_fmaf(a.b1, m, a.c1 * gr);
    const float sq = (a.c2 * gr) * gr;
    v = FUSED ? __builtin_fmaf(a.b2, v, sq) : a.b2 * v + sq;
    const float rt = sqrtf(v);
    const float den = FUSED ? __builtin_fmaf(a.rsqrt_bc2, rt, a.eps) : a.rsqrt_bc2 * rt + a.eps;
    p = p - (a.lr_over_bc1 * m) / den;
}

__global__ __launch_bounds__(256) void gpe_adam_guarded_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                               float* __restrict__ v, long n, float lr_over_bc1, float b1,
                                                               float b2, float eps, float wd, float rsqrt_bc2, float gscale,
                                                               int zero_grad, const float* __restrict__ hyper,
                                                               const GpeAdamGuard* __restrict__ guard)
{
#pragma clang fp contract(off)
    const long i4 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= n) return;
    if (guard->skip) {                                 // the step is not applied; the gradient is consumed all the same
        if (zero_grad) {
            if (i4 + 3 < n) *reinterpret_cast<float4*>(g + i4) = make_float4(0.f, 0.f, 0.f, 0.f);
            else for (long i = i4; i < n; ++i) g[i] = 0.f;
        }
        return;
    }
    if (hyper) { lr_over_bc1 = hyper[0]; rsqrt_bc2 = hyper[1]; }
    const AdamScalars a = {lr_over_bc1, b1, b2, 1.f - b1, 1.f - b2, eps, wd, rsqrt_bc2, gscale * guard->coef};
    if (i4 + 3 < n) {
        float4 pv = *reinterpret_cast<float4*>(p + i4), gv = *reinterpret_cast<float4*>(g + i4);
        float4 mv = *reinterpret_cast<float4*>(m + i4), vv = *reinterpret_cast<float4*>(v + i4);
        float* pp = &pv.x; float* gg = &gv.x; float* mm = &mv.x; float* vq = &vv.x;
#pragma unroll
        for (int t = 0; t < 4; ++t) adam_guarded_elem<true>(a, pp[t], gg[t], mm[t], vq[t]);
        *reinterpret_cast<float4*>(p + i4) = pv;
        *reinterpret_cast<float4*>(m + i4) = mv;
        *reinterpret_cast<float4*>(v + i4) = vv;
        if (zero_grad) *reinterpret_cast<float4*>(g + i4) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        const long pairs_end = i4 + ((n - i4) & ~1L);
        for (long i = i4; i < n; ++i) {
            float pi = p[i], mi = m[i], vi = v[i];
            if (i < pairs_end) adam_guarded_elem<true>(a, pi, g[i], mi, vi);
            else adam_guarded_elem<false>(a, pi, g[i], mi, vi);
            p[i] = pi; m[i] = mi; v[i] = vi;
            if (zero_grad) g[i] = 0.f;
        }
    }
}

static bool adam_args_bad(const float* p, const float* g, const float* m, const float* v, long n, const void* guard)
{
    return !p || !g || !m || !v || !guard || n <= 0 ||
           (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)guard) & 15);
}

extern "C" int gpe_adam_step_guarded(float* p, float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                                     float eps, float weight_decay, long step, float gscale, int zero_grad, const void* guard,
                                     void* stream)
{
    if (adam_args_bad(p, g, m, v, n, guard) || step <= 0) return GPE_EINVAL;
    float hy[2];
    if (gpe_adam_hyper(lr, beta1, beta2, step, hy) != GPE_OK) return GPE_EINVAL;       // the scalars of gpe_adam_step
    hipLaunchKernelGGL(gpe_adam_guarded_kernel, dim3(gpe_cdiv(gpe_cdiv(n, 4), 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                       n, hy[0], beta1, beta2, eps, weight_decay, hy[1], gscale, zero_grad, (const float*)nullptr,
                       static_cast<const GpeAdamGuard*>(guard));
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_adam_step_guarded_dev(float* p, float* g, float* m, float* v, long n, const float* hyper, float beta1,
                                         float beta2, float eps, float weight_decay, float gscale, int zero_grad,
                                         const void* guard, void* stream)
{
    if (adam_args_bad(p, g, m, v, n, guard) || !hyper || (((uintptr_t)hyper) & 3)) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_adam_guarded_kernel, dim3(gpe_cdiv(gpe_cdiv(n, 4), 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                       n, 0.f, beta1, beta2, eps, weight_decay, 1.f, gscale, zero_grad, hyper,
                       static_cast<const GpeAdamGuard*>(guard));
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
