// The encoder's input point clouds drawn on the device from resident meshes (what Garment3DPatternFullDataset._get_sample_info,
// nn/data/datasets.py, does per garment on the host: igl.random_points_on_mesh, the barycentric -> world loop, the optional Gaussian
// noise, igl.snap_points for the segmentation labels and for the stitch points, FeatureStandartization), at most two launches per
// batch.
//
//   slot b       garment g = index[b] of the resident set; point n < N is one item; a 256-thread workgroup owns MS_PPT points per
//                thread of one slot
//   face         kind 8, word 0: w = word >> 1, the first face of the garment whose threshold T[f] > w (binary search; T the
//                integer image of the cumulative area, T[last positive face ..] = 2^31: a zero-area face is never drawn)
//   barycentric  words 1 and 2: iu = word >> 8, iv = word >> 8, both reflected (i <- 2^24 - i) when iu + iv > 2^24;
//                b1 = iu 2^-24, b2 = iv 2^-24, b0 = (2^24 - iu - iv) 2^-24, exact in fp32; p = (b0 A + b1 B) + b2 C per axis
//   noise        kind 9, only when point_noise_w != 0: Box-Muller, words 0 and 1 -> (x, y), words 2 and 3 -> z (the cosine branch);
//                u1 = ((word >> 8) + 1) 2^-24, u2 = (word >> 8) 2^-24, r = sqrtf(-2 logf(u1)), r cospif(2 u2) / r sinpif(2 u2);
//                p <- p + w z
//   label        that of the vertex of g nearest to the noisy p: the lexicographic minimum of (d, vertex), d = (dx dx + dy dy) +
//                dz dz; the vertices pass through LDS in tiles of MS_TILE, in ascending order, so the minimum depends on no tile or
//                grid shape
//   re-label     second launch, only for a resident set that has unlabelled (-1) vertices: a point whose label is -1 takes the
//                label of the nearest point of its own cloud whose raw label is >= 0 (same distance, the lower point wins); none:
//                label 0, counted in status[b].  The first launch leaves {p, raw label} of every point in the caller's workspace,
//                and the second walks it with the same scan
//   output       features (p - shift) / scale, the fp32 subtract-then-divide of gpe_standardize (p itself without statistics);
//                segmentation int64; status
//
// Every product, sum and difference of the coordinates and distances is rounded on its own (ms_mul / ms_add / ms_sub below: no contraction), so a
// float32 restatement is bit-exact.  The state {seed, draw} and the last-arriver ticket are those of gpe_stitch_sample.hip; the
// kinds 8 and 9 keep a sampler that shares its seed apart from that one.  Plain vector stores and integer atomics only.
#include "gpe_device.h"

// (hip's __fmul_rn / __fadd_rn / __fsub_rn are the plain operators of a header compiled under the build's contraction mode, and
// the compiler fuses them: the operators below are compiled with contraction off and stay apart)
#pragma clang fp contract(off)
__device__ __forceinline__ float ms_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float ms_add(float a, float b) { return a + b; }
__device__ __forceinline__ float ms_sub(float a, float b) { return a - b; }

#define MS_TPB 256
#define MS_PPT 2                        // points per thread: one LDS read of a staged vertex serves both
#define MS_PTS (MS_TPB * MS_PPT)        // points per workgroup
#define MS_TILE MS_TPB                  // vertices (or points) per LDS tile: one 16-byte element per thread and stage

enum { MS_FACE = 8, MS_NOISE = 9 };

struct MsParams {
    const f32x4* verts; const int32_t* faces; const int32_t* vert_off; const int32_t* face_off; const uint32_t* cdf;
    int G, N, chunks;                   // chunks = workgroups per slot
    const int32_t* index;
    float noise_w; int standardize, relabel;
    float shift[3], scale[3];
    unsigned long long* state; unsigned* ticket;
    f32x4* ws;                          // [B][N] {p, raw label}: written by the first launch when relabel, read by the second
    float* features; long long* seg; int32_t* status;
};

// the garment of slot b: -2 index outside the set, -1 no face of positive area, 0 fine (block-uniform)
__device__ __forceinline__ int ms_garment(const MsParams& p, int b, int& g, int& v0, int& V, int& f0, int& F)
{
    g = p.index[b];
    if (g < 0 || g >= p.G) return -2;
    v0 = p.vert_off[g]; V = p.vert_off[g + 1] - v0;
    f0 = p.face_off[g]; F = p.face_off[g + 1] - f0;
    if (V < 1 || F < 1 || p.cdf[f0 + F - 1] != 0x80000000u) return -1;
    return 0;
}

// every thread of the workgroup calls this: the `count` elements {x, y, z, label} of src pass through LDS in tiles, in ascending
// order, and each of the thread's points keeps the first element of the smallest distance.  LABELLED: only elements whose label is
// >= 0 count (best stays -1 when there is none).
template <bool LABELLED>
__device__ __forceinline__ void ms_scan(const f32x4* __restrict__ src, int count, f32x4* s_tile, const float (&px)[MS_PPT],
                                        const float (&py)[MS_PPT], const float (&pz)[MS_PPT], int (&best)[MS_PPT])
{
    const int tid = threadIdx.x;
    float bd[MS_PPT];
#pragma unroll
    for (int q = 0; q < MS_PPT; ++q) { bd[q] = INFINITY; best[q] = LABELLED ? -1 : 0; }
    const f32x4 none = {0.f, 0.f, 0.f, 0.f};
    f32x4 next = tid < count ? src[tid] : none;
    for (int base = 0; base < count; base += MS_TILE) {
        __syncthreads();                                     // the previous tile has been read
        s_tile[tid] = next;
        __syncthreads();
        if (base + MS_TILE + tid < count) next = src[base + MS_TILE + tid];
        const int cnt = count - base < MS_TILE ? count - base : MS_TILE;
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const f32x4 v = s_tile[j];                       // every lane reads the same element: an LDS broadcast
            const bool ok = !LABELLED || __float_as_int(v.w) >= 0;
#pragma unroll
            for (int q = 0; q < MS_PPT; ++q) {
                const float dx = ms_sub(v.x, px[q]), dy = ms_sub(v.y, py[q]), dz = ms_sub(v.z, pz[q]);
                const float d = ms_add(ms_add(ms_mul(dx, dx), ms_mul(dy, dy)), ms_mul(dz, dz));
                if (ok && d < bd[q]) { bd[q] = d; best[q] = base + j; }
            }
        }
    }
}

__global__ __launch_bounds__(MS_TPB) void gpe_mesh_sample_kernel(MsParams p)
{
    __shared__ f32x4 s_tile[MS_TILE];
    __shared__ unsigned long long s_state[2];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.chunks, c = blockIdx.x - b * p.chunks, N = p.N;

    if (tid == 0) {
        const unsigned long long seed = __hip_atomic_load(p.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long draw = __hip_atomic_load(p.state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_state[0] = seed; s_state[1] = draw;
        __threadfence();                                     // the reads before the ticket
        if (gpe_flag_ticket(p.ticket) == gridDim.x - 1) {    // every workgroup has read the state: advance it for the next launch
            __hip_atomic_store(p.state + 1, draw + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(p.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    int g, v0, V, f0, F;
    const int bad = ms_garment(p, b, g, v0, V, f0, F);
    if (c == 0 && tid == 0) p.status[b] = bad;
    if (bad) {                                               // block-uniform: the slot is all zeros
        for (int i = tid; i < MS_PTS; i += MS_TPB) {
            const int n = c * MS_PTS + i;
            if (n >= N) break;
            float* f = p.features + ((long)b * N + n) * 3;
            f[0] = 0.f; f[1] = 0.f; f[2] = 0.f;
            p.seg[(long)b * N + n] = 0;
        }
        return;
    }
    __syncthreads();
    const gpe_rng rng = {(unsigned)s_state[0], (unsigned)(s_state[0] >> 32), (unsigned)s_state[1], (unsigned)(s_state[1] >> 32),
                         (unsigned)b << 8};
    const f32x4* verts = p.verts + v0;
    const uint32_t* cdf = p.cdf + f0;

    float px[MS_PPT], py[MS_PPT], pz[MS_PPT];
    int best[MS_PPT];
#pragma unroll
    for (int q = 0; q < MS_PPT; ++q) {
        const int n = c * MS_PTS + q * MS_TPB + tid;
        px[q] = py[q] = pz[q] = 0.f;
        if (n >= N) continue;
        const gpe_u32x4 w = rng(MS_FACE, (unsigned)n);
        const unsigned t = w.x >> 1;
        int lo = 0, hi = F - 1;                              // T[F - 1] = 2^31 > t: the answer lies in [0, F - 1]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cdf[mid] > t) hi = mid; else lo = mid + 1;
        }
        const int32_t* face = p.faces + ((long)f0 + lo) * 3;
        int ia = face[0], ib = face[1], ic = face[2];        // checked by the caller; held inside the garment all the same
        ia = min(max(ia, 0), V - 1); ib = min(max(ib, 0), V - 1); ic = min(max(ic, 0), V - 1);
        const f32x4 A = verts[ia], B = verts[ib], C = verts[ic];
        unsigned iu = w.y >> 8, iv = w.z >> 8;
        if (iu + iv > (1u << 24)) { iu = (1u << 24) - iu; iv = (1u << 24) - iv; }
        const float k = 1.f / 16777216.f;
        const float b1 = (float)iu * k, b2 = (float)iv * k, b0 = (float)((1u << 24) - iu - iv) * k;
        px[q] = ms_add(ms_add(ms_mul(b0, A.x), ms_mul(b1, B.x)), ms_mul(b2, C.x));
        py[q] = ms_add(ms_add(ms_mul(b0, A.y), ms_mul(b1, B.y)), ms_mul(b2, C.y));
        pz[q] = ms_add(ms_add(ms_mul(b0, A.z), ms_mul(b1, B.z)), ms_mul(b2, C.z));
        if (p.noise_w != 0.f) {
            const gpe_u32x4 z = rng(MS_NOISE, (unsigned)n);
            const float r0 = sqrtf(ms_mul(-2.f, logf((float)((z.x >> 8) + 1u) * k)));
            const float r1 = sqrtf(ms_mul(-2.f, logf((float)((z.z >> 8) + 1u) * k)));
            float s0, c0;
            sincospif(2.f * ((float)(z.y >> 8) * k), &s0, &c0);
            const float c1 = cospif(2.f * ((float)(z.w >> 8) * k));
            px[q] = ms_add(px[q], ms_mul(p.noise_w, ms_mul(r0, c0)));
            py[q] = ms_add(py[q], ms_mul(p.noise_w, ms_mul(r0, s0)));
            pz[q] = ms_add(pz[q], ms_mul(p.noise_w, ms_mul(r1, c1)));
        }
    }

    ms_scan<false>(verts, V, s_tile, px, py, pz, best);

#pragma unroll
    for (int q = 0; q < MS_PPT; ++q) {
        const int n = c * MS_PTS + q * MS_TPB + tid;
        if (n >= N) continue;
        const long at = (long)b * N + n;
        const int label = __float_as_int(verts[best[q]].w);
        if (p.relabel) p.ws[at] = f32x4{px[q], py[q], pz[q], __int_as_float(label)};
        float* f = p.features + at * 3;
        if (p.standardize) {
            f[0] = (px[q] - p.shift[0]) / p.scale[0];
            f[1] = (py[q] - p.shift[1]) / p.scale[1];
            f[2] = (pz[q] - p.shift[2]) / p.scale[2];
        } else {
            f[0] = px[q]; f[1] = py[q]; f[2] = pz[q];
        }
        p.seg[at] = label;                                   // a -1 is replaced by the second launch
    }
}

// the stitch points: same grid as the first launch, which has finished (stream order)
__global__ __launch_bounds__(MS_TPB) void gpe_mesh_relabel_kernel(MsParams p)
{
    __shared__ f32x4 s_tile[MS_TILE];
    __shared__ int s_fell;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.chunks, c = blockIdx.x - b * p.chunks, N = p.N;
    int g, v0, V, f0, F;
    if (ms_garment(p, b, g, v0, V, f0, F)) return;           // block-uniform
    if (tid == 0) s_fell = 0;
    const f32x4* cloud = p.ws + (long)b * N;

    float px[MS_PPT], py[MS_PPT], pz[MS_PPT];
    int best[MS_PPT];
    bool open[MS_PPT];
    bool any = false;
#pragma unroll
    for (int q = 0; q < MS_PPT; ++q) {
        const int n = c * MS_PTS + q * MS_TPB + tid;
        px[q] = py[q] = pz[q] = 0.f;
        open[q] = false;
        if (n >= N) continue;
        const f32x4 v = cloud[n];
        px[q] = v.x; py[q] = v.y; pz[q] = v.z;
        open[q] = __float_as_int(v.w) < 0;
        any |= open[q];
    }
    if (!__syncthreads_or(any)) return;                      // block-uniform: nothing to re-label here
    ms_scan<true>(cloud, N, s_tile, px, py, pz, best);
    int fell = 0;
#pragma unroll
    for (int q = 0; q < MS_PPT; ++q) {
        if (!open[q]) continue;
        const int n = c * MS_PTS + q * MS_TPB + tid;
        int label = 0;
        if (best[q] >= 0) label = __float_as_int(cloud[best[q]].w);
        else ++fell;
        p.seg[(long)b * N + n] = label;
    }
    if (fell) atomicAdd(&s_fell, fell);
    __syncthreads();
    if (tid == 0 && s_fell) atomicAdd(&p.status[b], s_fell); // the first launch stored 0
}

extern "C" int gpe_mesh_points_sample(const float* verts4, const int32_t* faces, const int32_t* vert_off, const int32_t* face_off,
                                      const uint32_t* face_cdf, int G, const int32_t* index, int B, int N, float point_noise_w,
                                      const float* shift_host, const float* scale_host, int relabel, float* ws, uint64_t* state,
                                      uint32_t* ticket, float* features, int64_t* segmentation, int32_t* status, void* stream)
{
    if (!verts4 || !faces || !vert_off || !face_off || !face_cdf || !index || !state || !ticket || !features || !segmentation ||
        !status || (!shift_host) != (!scale_host) || (relabel && !ws))
        return GPE_EINVAL;
    if ((((uintptr_t)verts4) & 15) || (((uintptr_t)ws) & 15) || (((uintptr_t)state) & 7) || (((uintptr_t)segmentation) & 7))
        return GPE_EINVAL;
    if (G < 1 || B < 1 || B >= (1 << 24) || N < 1 || N >= (1 << 28)) return GPE_EINVAL;
    MsParams p;
    p.chunks = gpe_cdiv(N, MS_PTS);
    if ((long)B * p.chunks > 0x7fffffffL) return GPE_EINVAL;
    p.verts = reinterpret_cast<const f32x4*>(verts4); p.faces = faces; p.vert_off = vert_off; p.face_off = face_off; p.cdf = face_cdf;
    p.G = G; p.N = N; p.index = index;
    p.noise_w = point_noise_w; p.standardize = shift_host ? 1 : 0; p.relabel = relabel ? 1 : 0;
    for (int a = 0; a < 3; ++a) {
        p.shift[a] = shift_host ? shift_host[a] : 0.f;
        p.scale[a] = scale_host ? scale_host[a] : 1.f;
    }
    p.state = reinterpret_cast<unsigned long long*>(state); p.ticket = ticket;
    p.ws = reinterpret_cast<f32x4*>(ws);
    p.features = features; p.seg = reinterpret_cast<long long*>(segmentation); p.status = status;
    const dim3 grid((unsigned)((long)B * p.chunks));
    hipLaunchKernelGGL(gpe_mesh_sample_kernel, grid, dim3(MS_TPB), 0, (hipStream_t)stream, p);
    GPE_CHECK_LAUNCH();
    if (p.relabel) {
        hipLaunchKernelGGL(gpe_mesh_relabel_kernel, grid, dim3(MS_TPB), 0, (hipStream_t)stream, p);
        GPE_CHECK_LAUNCH();
    }
    return GPE_OK;
}
