// Bandwidth-bound kernels of the path for gfx950: LSTM cell pointwise, the GRU cell backward, and the inter-layer dropout of
// nn.LSTM / nn.GRU (nn/net_blocks.py:346,374,418-420,469).
// Reference lines each one replaces are listed in include/gpe_hip.h.
#include "gpe_device.h"
#include <math.h>

// ---------------------------------------------------------------------------------------------------------
// LSTM cell pointwise (gate order i, f, g, o as in torch.nn.LSTM)
// ---------------------------------------------------------------------------------------------------------
__global__ void gpe_lstm_cell_fwd_kernel(float* __restrict__ gates, const float* __restrict__ c_prev, long ldc_prev,
                                         float* __restrict__ c, float* __restrict__ h, long h_stride, int Bn, int H)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)Bn * H) return;
    const long b = e / H;
    const int u = (int)(e - b * H);
    float* gr = gates + b * 4 * H;
    float ig, fg, gg, og, cn;
    gpe_lstm_cell_fwd(gr[u], gr[H + u], gr[2 * H + u], gr[3 * H + u], c_prev[b * ldc_prev + u], ig, fg, gg, og, cn);
    gr[u] = ig; gr[H + u] = fg; gr[2 * H + u] = gg; gr[3 * H + u] = og;
    c[b * H + u] = cn;
    h[b * h_stride + u] = gpe_lstm_cell_h(og, cn);
}

extern "C" int gpe_lstm_cell_fwd(float* gates, const float* c_prev, long ldc_prev, float* c, float* h,
                                 long h_stride, int Bn, int H, void* stream)
{
    if (!gates || !c_prev || !c || !h || Bn <= 0 || H <= 0) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_lstm_cell_fwd_kernel, dim3(gpe_cdiv((long)Bn * H, 256)), dim3(256), 0,
                       (hipStream_t)stream, gates, c_prev, ldc_prev, c, h, h_stride, Bn, H);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

__global__ void gpe_lstm_cell_bwd_kernel(const float* __restrict__ dh_out, long dho_stride,
                                         const float* __restrict__ dh_rec, int n_rec,
                                         const float* __restrict__ dc_next,
                                         const float* __restrict__ gates, const float* __restrict__ c,
                                         const float* __restrict__ c_prev, long ldc_prev,
                                         float* __restrict__ dgates, long dg_stride, float* __restrict__ dc_prev,
                                         int Bn, int H)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)Bn * H) return;
    const long b = e / H;
    const int u = (int)(e - b * H);
    const float* gr = gates + b * 4 * H;
    float dh = dh_out ? dh_out[b * dho_stride + u] : 0.f;
    if (dh_rec)
        for (int z = 0; z < n_rec; ++z) dh += dh_rec[(long)z * Bn * H + b * H + u];   // split-K partials
    float di, df, dgg, dgo, cout;
    gpe_lstm_cell_bwd(gr[u], gr[H + u], gr[2 * H + u], gr[3 * H + u], c[b * H + u], c_prev[b * ldc_prev + u], dh,
                      dc_next ? dc_next + b * H + u : nullptr, di, df, dgg, dgo, cout);
    float* dg = dgates + b * dg_stride;
    dg[u] = di; dg[H + u] = df; dg[2 * H + u] = dgg; dg[3 * H + u] = dgo;
    dc_prev[b * H + u] = cout;
}

extern "C" int gpe_lstm_cell_bwd(const float* dh_out, long dho_stride, const float* dh_rec, int n_rec,
                                 const float* dc_next,
                                 const float* gates, const float* c, const float* c_prev, long ldc_prev,
                                 float* dgates, long dg_stride, float* dc_prev, int Bn, int H, void* stream)
{
    if (!gates || !c || !c_prev || !dgates || !dc_prev || Bn <= 0 || H <= 0) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_lstm_cell_bwd_kernel, dim3(gpe_cdiv((long)Bn * H, 256)), dim3(256), 0,
                       (hipStream_t)stream, dh_out, dho_stride, dh_rec, n_rec, dc_next, gates, c, c_prev, ldc_prev, dgates,
                       dg_stride, dc_prev, Bn, H);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// GRU cell backward (pointwise).  dh = dh_out + dh_dir_next (the z-gated direct path of step t+1) + sum of the n_rec
// partials of dGh_{t+1}.W_hh;  saved = {r, z, n, hn} of this step (gpe_gru_step_fwd), h_prev rows.
//   dGx [.][3H] = {dr_pre, dz_pre, dn_pre}   (gradient w.r.t. the INPUT-side pre-activations: W_ih, b_ih, x)
//   dGh [.][3H] = {dr_pre, dz_pre, dn_pre*r} (w.r.t. the RECURRENT-side pre-activations: W_hh, b_hh, h_prev)
//   dh_dir_prev = dh * z
__global__ void gpe_gru_cell_bwd_kernel(const float* __restrict__ dh_out, long dho_stride,
                                        const float* __restrict__ dh_rec, int n_rec, const float* __restrict__ dh_dir_next,
                                        const float* __restrict__ saved, const float* __restrict__ h_prev, long hp_stride,
                                        float* __restrict__ dgx, float* __restrict__ dgh, long dg_stride,
                                        float* __restrict__ dh_dir_prev, int Bn, int H)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)Bn * H) return;
    const long b = e / H;
    const int u = (int)(e - b * H);
    const float* sv = saved + b * 4 * H;
    const float rg = sv[u], zg = sv[H + u], ng = sv[2 * H + u], hn = sv[3 * H + u];
    float dh = dh_out ? dh_out[b * dho_stride + u] : 0.f;
    if (dh_dir_next) dh += dh_dir_next[b * H + u];
    if (dh_rec)
        for (int z = 0; z < n_rec; ++z) dh += dh_rec[(long)z * Bn * H + b * H + u];
    const float hp = h_prev[b * hp_stride + u];
    const float dn_pre = dh * (1.f - zg) * (1.f - ng * ng);
    const float dz_pre = dh * (hp - ng) * zg * (1.f - zg);
    const float dr_pre = dn_pre * hn * rg * (1.f - rg);
    float* gx = dgx + b * dg_stride;
    float* gh = dgh + b * dg_stride;
    gx[u] = dr_pre; gx[H + u] = dz_pre; gx[2 * H + u] = dn_pre;
    gh[u] = dr_pre; gh[H + u] = dz_pre; gh[2 * H + u] = dn_pre * rg;
    dh_dir_prev[b * H + u] = dh * zg;
}

extern "C" int gpe_gru_cell_bwd(const float* dh_out, long dho_stride, const float* dh_rec, int n_rec,
                                const float* dh_dir_next, const float* saved, const float* h_prev, long hp_stride,
                                float* dgx, float* dgh, long dg_stride, float* dh_dir_prev, int Bn, int H, void* stream)
{
    if (!saved || !h_prev || !dgx || !dgh || !dh_dir_prev || Bn <= 0 || H <= 0) return GPE_EINVAL;
    hipLaunchKernelGGL(gpe_gru_cell_bwd_kernel, dim3(gpe_cdiv((long)Bn * H, 256)), dim3(256), 0, (hipStream_t)stream,
                       dh_out, dho_stride, dh_rec, n_rec, dh_dir_next, saved, h_prev, hp_stride, dgx, dgh, dg_stride,
                       dh_dir_prev, Bn, H);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}

// out[(b*T + t)*H + h] = x[b*x_sb + t*x_st + h] * mask[(b*T + t)*H + h] — the inter-layer dropout of nn.LSTM / nn.GRU
// (/root/reference/nn/net_blocks.py:346,374,418-420,469 pass `dropout` to torch's recurrent modules, which multiply the
// output sequence of every layer but the last by a Bernoulli(1-p)/(1-p) mask).  x is a strided [Bn, T, H] view (the h history
// of a recurrent stack, or a dense gradient); mask and out are dense.
__global__ void gpe_mul_rows_kernel(const float* __restrict__ x, long x_sb, long x_st, const float* __restrict__ mask, int T,
                                    int H, long n, float* __restrict__ out)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int h = (int)(e % H);
    const long q = e / H;
    const int t = (int)(q % T);
    const long b = q / T;
    out[e] = x[b * x_sb + t * x_st + h] * mask[e];
}

extern "C" int gpe_mul_rows(const float* x, long x_sb, long x_st, const float* mask, long Bn, int T, int H, float* out,
                            void* stream)
{
    if (!x || !mask || !out || Bn < 0 || T <= 0 || H <= 0) return GPE_EINVAL;
    const long n = Bn * T * H;
    if (n == 0) return GPE_OK;
    hipLaunchKernelGGL(gpe_mul_rows_kernel, dim3(gpe_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, x_sb, x_st, mask, T, H,
                       n, out);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
