// The training loss of the edge-pair classifier (StitchOnEdge3DPairs; nn/metrics/composed_loss.py:83-126 ComposedLoss on a batch of
// sampled pair rows): BCEWithLogitsLoss (mean) and the quality counters of the same rows in ONE launch, its gradient in one more.
//
//   term     max(x, 0) - x y + log1p(exp(-|x|)), fp32; for y in {0, 1} this is relu(-x if y else x) + log1p(exp(-|x|)), the
//            cancellation-free form the evaluating stitch kernels use (gpe_stitch_pairs.hip sp_eval_pair), bit for bit
//   class    sigmoid(x) > 0.5 in fp32 (sp_positive of gpe_stitch_pairs.hip); correct: class == y; positive label: y == 1
//   sums     fp64 for the loss, int32 for the counters.  The caller fixes the number of partial slots; slot s owns the rows
//            [s * chunk, (s + 1) * chunk), chunk = ceil(M / slots), whatever the device.  Inside a workgroup: a thread walks its rows
//            in order, xor butterfly within a wave, the waves in order through LDS.  The workgroup that draws the last ticket
//            (gpe_pack_fold's scheme: nobody waits, the ticket is left zero) adds the slots in slot order and writes the results.
//            No float atomics: two calls give the same bits, on any grid the chip schedules.
#include "gpe_device.h"
#include <limits.h>
#include <math.h>

#define PL_TPB 256
#define PL_MAX_SLOTS 256
#define PL_SLOT_WORDS 4              // uint64 per slot: loss bits, correct | tp << 32, predicted | labelled << 32, unused

struct PlAcc { double loss; int correct, tp, pp, gp; };

__device__ __forceinline__ bool pl_positive(float x) { return gpe_sigmoid(x) > 0.5f; }

__device__ __forceinline__ void pl_row(float x, float y, PlAcc& a)
{
    const bool pos = pl_positive(x), lab = y == 1.f;
    a.loss += (double)(fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x))));
    a.correct += (pos ? 1.f : 0.f) == y ? 1 : 0;
    a.tp += pos && lab ? 1 : 0;
    a.pp += pos ? 1 : 0;
    a.gp += lab ? 1 : 0;
}

__device__ __forceinline__ float pl_ratio(int num, int den) { return den ? (float)num / (float)den : 0.f; }

template <typename Y>
__global__ __launch_bounds__(PL_TPB) void gpe_pair_loss_fwd_kernel(const float* __restrict__ x, const Y* __restrict__ y, long M,
                                                                   long chunk, unsigned long long* part, unsigned* ticket,
                                                                   float* __restrict__ out, int* __restrict__ counts)
{
    __shared__ double s_loss[PL_MAX_SLOTS];      // the waves' sums, then (last workgroup) the slots'
    __shared__ int s_cnt[PL_MAX_SLOTS][4];
    __shared__ unsigned last_sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long lo = (long)blockIdx.x * chunk;
    const long hi = lo + chunk < M ? lo + chunk : M;
    PlAcc a = {0.0, 0, 0, 0, 0};
    for (long i = lo + tid; i < hi; i += PL_TPB) pl_row(x[i], (float)y[i], a);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a.loss += __shfl_xor(a.loss, o);
        a.correct += __shfl_xor(a.correct, o);
        a.tp += __shfl_xor(a.tp, o);
        a.pp += __shfl_xor(a.pp, o);
        a.gp += __shfl_xor(a.gp, o);
    }
    if (lane == 0) {
        s_loss[wave] = a.loss;
        s_cnt[wave][0] = a.correct; s_cnt[wave][1] = a.tp; s_cnt[wave][2] = a.pp; s_cnt[wave][3] = a.gp;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PL_TPB / 64; ++w) {
            a.loss += s_loss[w];
            a.correct += s_cnt[w][0]; a.tp += s_cnt[w][1]; a.pp += s_cnt[w][2]; a.gp += s_cnt[w][3];
        }
        unsigned long long* slot = part + (long)blockIdx.x * PL_SLOT_WORDS;
        __hip_atomic_store(slot, (unsigned long long)__double_as_longlong(a.loss), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(slot + 1, (unsigned long long)(unsigned)a.correct | ((unsigned long long)(unsigned)a.tp << 32),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(slot + 2, (unsigned long long)(unsigned)a.pp | ((unsigned long long)(unsigned)a.gp << 32),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();                                     // release: the partial before the ticket
        last_sh = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last_sh) return;
    __threadfence();                                         // acquire: every workgroup's partial
    if (tid < (int)gridDim.x) {                              // (gridDim.x <= PL_MAX_SLOTS == PL_TPB)
        const unsigned long long* slot = part + (long)tid * PL_SLOT_WORDS;
        const unsigned long long l = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long c0 = __hip_atomic_load(slot + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long c1 = __hip_atomic_load(slot + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_loss[tid] = __longlong_as_double((long long)l);
        s_cnt[tid][0] = (int)(unsigned)c0; s_cnt[tid][1] = (int)(c0 >> 32);
        s_cnt[tid][2] = (int)(unsigned)c1; s_cnt[tid][3] = (int)(c1 >> 32);
    }
    __syncthreads();
    if (tid != 0) return;
    double loss = 0.0;
    int correct = 0, tp = 0, pp = 0, gp = 0;
    for (int s = 0; s < (int)gridDim.x; ++s) {
        loss += s_loss[s];
        correct += s_cnt[s][0]; tp += s_cnt[s][1]; pp += s_cnt[s][2]; gp += s_cnt[s][3];
    }
    out[0] = (float)(loss / (double)M);                      // M == 0: 0 / 0 = NaN, torch's mean of nothing
    out[1] = pl_ratio(correct, (int)M);
    out[2] = pl_ratio(tp, pp);
    out[3] = pl_ratio(tp, gp);
    counts[0] = (int)M; counts[1] = correct; counts[2] = tp; counts[3] = pp; counts[4] = gp;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename Y>
__global__ __launch_bounds__(PL_TPB) void gpe_pair_loss_bwd_kernel(const float* __restrict__ x, const Y* __restrict__ y, long M,
                                                                   const float* __restrict__ gscale, float* __restrict__ gx)
{
    const float s = gscale[0] / (float)M;
    for (long i = (long)blockIdx.x * PL_TPB + threadIdx.x; i < M; i += (long)gridDim.x * PL_TPB)
        gx[i] = s * (gpe_sigmoid(x[i]) - (float)y[i]);
}

static inline bool pl_rows_ok(const float* x, const void* y, int kind, long M)
{
    // (no rows: the pointers are never followed, and an empty tensor's may be NULL)
    return (kind == 0 || kind == 1) && M >= 0 && M <= (long)INT_MAX && (M == 0 || (x && y));
}

extern "C" int gpe_pair_loss_fwd(const float* x, const void* y, int kind, long M, int slots, void* part, uint32_t* ticket,
                                 float* out, int32_t* counts, void* stream)
{
    if (!pl_rows_ok(x, y, kind, M) || slots < 1 || slots > PL_MAX_SLOTS || !part || (((uintptr_t)part) & 7) || !ticket || !out ||
        !counts)
        return GPE_EINVAL;
    const long chunk = (M + slots - 1) / slots;
    unsigned long long* p = static_cast<unsigned long long*>(part);
    if (kind == 0)
        hipLaunchKernelGGL((gpe_pair_loss_fwd_kernel<uint8_t>), dim3(slots), dim3(PL_TPB), 0, (hipStream_t)stream, x,
                           static_cast<const uint8_t*>(y), M, chunk, p, ticket, out, counts);
    else
        hipLaunchKernelGGL((gpe_pair_loss_fwd_kernel<float>), dim3(slots), dim3(PL_TPB), 0, (hipStream_t)stream, x,
                           static_cast<const float*>(y), M, chunk, p, ticket, out, counts);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

extern "C" int gpe_pair_loss_bwd(const float* x, const void* y, int kind, long M, const float* gscale, float* gx, void* stream)
{
    if (!pl_rows_ok(x, y, kind, M)) return GPE_EINVAL;
    if (M == 0) return GPE_OK;                               // (an empty gx may be NULL)
    if (!gscale || !gx) return GPE_EINVAL;
    const int blocks = gpe_cdiv(M, PL_TPB) < 1024 ? gpe_cdiv(M, PL_TPB) : 1024;
    if (kind == 0)
        hipLaunchKernelGGL((gpe_pair_loss_bwd_kernel<uint8_t>), dim3(blocks), dim3(PL_TPB), 0, (hipStream_t)stream, x,
                           static_cast<const uint8_t*>(y), M, gscale, gx);
    else
        hipLaunchKernelGGL((gpe_pair_loss_bwd_kernel<float>), dim3(blocks), dim3(PL_TPB), 0, (hipStream_t)stream, x,
                           static_cast<const float*>(y), M, gscale, gx);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
