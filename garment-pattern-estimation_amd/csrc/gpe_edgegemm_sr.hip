// Single-role, software-pipelined fused row GEMM for the per-edge MLP of DynamicEdgeConv on gfx950 — the EXACT-fp32 path
// (/root/reference/nn/net_blocks.py:43-47,124-135 forward; its input-gradient half in backward).
//
// Why this shape (profiles/r01_d_coissue_ubench.md): a wave that streams v_mfma_f32_16x16x4_f32 owns its SIMD — a second
// wave on the same SIMD gets no issue slots, so a producer/consumer pair runs at T_consumer + T_producer.  What a wave CAN
// do is issue its OWN memory instructions between its MFMAs: they cost a few issue cycles each (~10 % of the MFMA time in
// total) and their latency hides under the following MFMAs.  So: ONE persistent 256-thread workgroup per CU, one wave per
// SIMD (512 VGPRs each), every wave does everything for its share, and the K loop is hand-pipelined in chunks of 16 k:
//
//   chunk 0        issue ALL global loads of this iteration: the activation rows the epilogue of the PREVIOUS tile needs
//                  (backward) and the <= 16 rows this wave stages for the NEXT tile (dense rows or gathered Q rows)
//   chunks 1..     epilogue of the previous tile, a few rows per chunk, from the C buffer in LDS (bias+ReLU, fp64 BN
//                  statistics, whole-row stores, max/min over each point's messages; or BN/ReLU backward with the stored
//                  activation and per-point sums)
//   last chunks    commit the staged rows to the other A buffer in LDS (ReLU(P_i+Q_j) applied here for the gather)
//   every chunk    prefetch the next chunk's A fragments (ds_read_b128), then 4*AQ*4 + 4*BQ MFMAs
//
// Wave w owns N-tiles [AQ*w, AQ*w+AQ) for all 64 rows plus rows 16w..16w+15 of the BQ left-over N-tiles (so all four
// SIMDs issue the same number of MFMAs), with its weights resident in VGPRs as MFMA B fragments for the whole kernel.
// It stages and finishes rows [w*R/4, (w+1)*R/4) of every tile: R = 4*npw*k rows = whole points, npw*k <= 16.
// LDS: A[2] + C (159 KB at the shipped sizes), two barriers per tile.
#include "gpe_edgegemm_sr_kernel.h"

// ---- k > 16: merging the per-pseudo-point results ------------------------------------------------------------------------
// A point with k > 16 neighbours is processed as f pseudo-points of kq = k / f rows (kq <= 16, so every wave still owns whole
// pseudo-points).  The kernels then write one max / min / argmax / argmin row, or one dP row, per PSEUDO-point into a scratch
// image; these two kernels fold the f rows of each point, in pseudo-point order (first maximum wins, fixed summation order).
__global__ void gpe_sr_fold_agg_kernel(const float* __restrict__ tmx, const float* __restrict__ tmn,
                                       const uint8_t* __restrict__ tamx, const uint8_t* __restrict__ tamn, long npts, int f,
                                       int kq, int C, int ld, float* __restrict__ mx, float* __restrict__ mn,
                                       uint8_t* __restrict__ amx, uint8_t* __restrict__ amn)
{
    const int cq = (C + 3) >> 2;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= npts * cq) return;
    const long pt = t / cq;
    const int c = (int)(t - pt * cq) << 2;
    float bx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, bn[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
    int ix[4] = {0, 0, 0, 0}, in_[4] = {0, 0, 0, 0};
    for (int q = 0; q < f; ++q) {
        const long o = (pt * f + q) * ld + c;
        const float4 vx = ld4(tmx + o), vn = ld4(tmn + o);
        const uchar4 ax = *reinterpret_cast<const uchar4*>(tamx + o), an = *reinterpret_cast<const uchar4*>(tamn + o);
        const float x4[4] = {vx.x, vx.y, vx.z, vx.w}, n4[4] = {vn.x, vn.y, vn.z, vn.w};
        const int ax4[4] = {ax.x, ax.y, ax.z, ax.w}, an4[4] = {an.x, an.y, an.z, an.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (x4[u] > bx[u]) { bx[u] = x4[u]; ix[u] = q * kq + ax4[u]; }
            if (n4[u] < bn[u]) { bn[u] = n4[u]; in_[u] = q * kq + an4[u]; }
        }
    }
    const long o = pt * ld + c;
    st4(mx + o, make_float4(bx[0], bx[1], bx[2], bx[3]));
    st4(mn + o, make_float4(bn[0], bn[1], bn[2], bn[3]));
    *reinterpret_cast<uchar4*>(amx + o) = make_uchar4(ix[0], ix[1], ix[2], ix[3]);
    *reinterpret_cast<uchar4*>(amn + o) = make_uchar4(in_[0], in_[1], in_[2], in_[3]);
}

__global__ void gpe_sr_fold_sum_kernel(const float* __restrict__ t, long npts, int f, int C, int ld, float* __restrict__ y)
{
    const int cq = (C + 3) >> 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npts * cq) return;
    const long pt = i / cq;
    const int c = (int)(i - pt * cq) << 2;
    float4 s = ld4(t + (pt * f) * ld + c);
    for (int q = 1; q < f; ++q) {
        const float4 v = ld4(t + (pt * f + q) * ld + c);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    st4(y + pt * ld + c, s);
}

// after the launch: folds the per-pseudo-point rows of the scratch image into the caller's per-point outputs
int gpe_edge_pseudo_fold(const RgParams& p, const GpeFold& fd, hipStream_t s)
{
    if (fd.f <= 1) return GPE_OK;
    const long th = fd.npts * ((p.N + 3) >> 2);
    if (fd.mx) {
        hipLaunchKernelGGL(gpe_sr_fold_agg_kernel, dim3((unsigned)gpe_cdiv(th, 256)), dim3(256), 0, s, p.mx, p.mn, p.oamx, p.oamn,
                           fd.npts, fd.f, fd.kq, p.N, p.oldagg, fd.mx, fd.mn, fd.amx, fd.amn);
        GPE_CHECK_LAUNCH();
    }
    if (fd.dp) {
        hipLaunchKernelGGL(gpe_sr_fold_sum_kernel, dim3((unsigned)gpe_cdiv(th, 256)), dim3(256), 0, s, p.dP, fd.npts, fd.f, p.N,
                           p.lddp, fd.dp);
        GPE_CHECK_LAUNCH();
    }
    return GPE_OK;
}

// The exact-fp32 single-role family.  `p` is re-tiled (gpe_edge_retile): every wave owns whole points.
int gpe_edge_sr(const RgParams& p_in, int amode, int emode, int NT, int KCH, int stats_nblk, hipStream_t s)
{
    // K = N = 200 with the in-place backward epilogue does not fit 512 VGPRs without heavy spilling (the instances exist, as they
    // always did): left to the producer/consumer kernel; no shipped layer has that shape
    if (NT == 13 && KCH == 13 && emode == E_BWD_INPLACE) return GPE_EDGE_NOT_MINE;
    RgParams p = p_in;
    // dummy image of the straight-line instances: 64 rows x 512 floats (row pitches here are <= 256 floats)
    p.dummy = (p.ldo <= 512 && p.oldagg <= 512 && p.lddp <= 512) ? p.ws.dummy : nullptr;
    return (amode == A_DENSE && emode != E_BWD_GATHER) ? gpe_edge_sr_dense(p, amode, emode, NT, KCH, stats_nblk, s)
                                                       : sr_select<false>(p, amode, emode, NT, KCH, stats_nblk, s);
}
