// The panels of a decoded prediction placed in 3D (NNSewingPattern._3D_edges_per_panel, nn/data/pattern_converter.py:517-552, and the
// inverse of the universal translation, :281-288) as one gfx950 kernel that reads what gpe_pattern_decode wrote: one workgroup of one
// wave per garment, every panel on its own lane, as in gpe_pattern_decode.hip.  The reference does this per panel in Python through
// three functions of its external `pattern` package; include/gpe_hip_place.h states what each of them computes.  Per panel:
//   1. the rotation matrix of the normalised quaternion;
//   2. the universal point (pp_top_mid: the one rule that rests on the package's published definition);
//   3. the translation of the panel's origin;
//   4. the vertices in 3D;
//   5. the edge rows [start, end, curvature] in fp32, compact, the classifier's input.
// No atomics, nothing between lanes, every output element written by exactly one thread: bit-reproducible.  A garment has at most
// 1024 edges, so the work is a few microseconds of latency; nothing here is worth more than one lane per panel.
#include "gpe_common.h"
#include <math.h>

// every product / sum below is rounded on its own: the host restatement (numpy on float64) computes the same numbers
#pragma clang fp contract(off)

#define PP_TPB 64            // one wave per garment
#define PP_MAXE 1024         // edges per pattern P * L, the menu of gpe_pattern_decode

struct PpParams {
    const int32_t *num_edges, *num_verts;
    const double *vertices, *curvature;
    const int32_t* curved;
    const double *rotations, *translations;
    int B, P, L;
    double *rot_matrix, *translation;
    int32_t* top_mid;
    double* vertices3d;
    float* edges3d;
    int32_t* place_flags;
};

// R (row-major) of the quaternion q = (x, y, z, w) / |q|: scipy's Rotation.from_quat(q).as_matrix().  A zero or non-finite norm
// gives the identity and returns GPE_PLACE_BAD_QUAT (scipy raises there).
__device__ __forceinline__ int pp_quat_matrix(const double* q, double* R)
{
    const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(nrm > 0.0) || isinf(nrm)) {
        for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
        return GPE_PLACE_BAD_QUAT;
    }
    const double x = q[0] / nrm, y = q[1] / nrm, z = q[2] / nrm, w = q[3] / nrm;
    const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
    const double xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
    R[0] = x2 - y2 - z2 + w2; R[1] = 2.0 * (xy - zw);   R[2] = 2.0 * (xz + yw);
    R[3] = 2.0 * (xy + zw);   R[4] = -x2 + y2 - z2 + w2; R[5] = 2.0 * (yz - xw);
    R[6] = 2.0 * (xz - yw);   R[7] = 2.0 * (yz + xw);   R[8] = -x2 - y2 + z2 + w2;
    return 0;
}

// The universal point of a panel (_panel_universal_transtation of the reference's `pattern` package, by its published definition):
// of the four midpoints of the sides of the 2D bounding box [lo, hi] of the panel's vertices, in the order
//     0 top (mid_x, max_y)   1 bottom (mid_x, min_y)   2 right (max_x, mid_y)   3 left (min_x, mid_y)
// the one that lies highest in 3D: largest R[1][0] m.x + R[1][1] m.y (the translation moves all four alike); on a tie the first in
// that order (numpy's argmax).  -> its number, the point in (mx, my).
__device__ __forceinline__ int pp_top_mid(const double* R, double lox, double loy, double hix, double hiy, double& mx, double& my)
{
    const double cx = (lox + hix) / 2.0, cy = (loy + hiy) / 2.0;
    const double px[4] = {cx, cx, hix, lox}, py[4] = {hiy, loy, cy, cy};
    int best = 0;
    double ybest = R[3] * px[0] + R[4] * py[0];
    for (int k = 1; k < 4; ++k) {
        const double y3 = R[3] * px[k] + R[4] * py[k];
        if (y3 > ybest) { best = k; ybest = y3; }
    }
    mx = px[best]; my = py[best];
    return best;
}

__global__ __launch_bounds__(PP_TPB) void gpe_pattern_place_kernel(PpParams q)
{
    const int b = blockIdx.x, P = q.P, L = q.L;
    for (int p = threadIdx.x; p < P; p += PP_TPB) {
        const size_t gp = (size_t)b * P + p;
        const double* vert = q.vertices + gp * (L + 1) * 2;
        const double* cur = q.curvature + gp * L * 2;
        const int32_t* crv = q.curved + gp * L;
        double* Rout = q.rot_matrix + gp * 9;
        double* tout = q.translation + gp * 3;
        double* v3 = q.vertices3d + gp * (L + 1) * 3;
        float* e3 = q.edges3d + gp * L * 8;
        int n = q.num_edges[gp], nv = q.num_verts[gp];
        n = n < 0 ? 0 : (n > L ? L : n);
        nv = nv < 0 ? 0 : (nv > L + 1 ? L + 1 : nv);
        if (n == 0 || nv == 0) { n = 0; nv = 0; }
        int flag = 0, top = -1;
        if (n > 0) {
            double R[9], mx, my;
            flag = pp_quat_matrix(q.rotations + gp * 4, R);
            double lox = vert[0], hix = vert[0], loy = vert[1], hiy = vert[1];
            for (int v = 1; v < nv; ++v) {
                const double x = vert[2 * v], y = vert[2 * v + 1];
                lox = x < lox ? x : lox; hix = x > hix ? x : hix;
                loy = y < loy ? y : loy; hiy = y > hiy ? y : hiy;
            }
            top = pp_top_mid(R, lox, loy, hix, hiy, mx, my);
            double t[3];
            for (int r = 0; r < 3; ++r) {
                t[r] = q.translations[gp * 3 + r] - (R[3 * r] * mx + R[3 * r + 1] * my);
                tout[r] = t[r];
            }
            for (int k = 0; k < 9; ++k) Rout[k] = R[k];
            for (int v = 0; v < nv; ++v) {
                const double x = vert[2 * v], y = vert[2 * v + 1];
                for (int r = 0; r < 3; ++r) v3[3 * v + r] = (R[3 * r] * x + R[3 * r + 1] * y) + t[r];
            }
            // the rows read back what this lane has just stored (same thread, program order)
            for (int k = 0; k < n; ++k) {
                const int e = k + 1 < nv ? k + 1 : 0;
                const bool c = crv[k] != 0;
                for (int r = 0; r < 3; ++r) { e3[8 * k + r] = (float)v3[3 * k + r]; e3[8 * k + 3 + r] = (float)v3[3 * e + r]; }
                e3[8 * k + 6] = c ? (float)cur[2 * k] : 0.0f;
                e3[8 * k + 7] = c ? (float)cur[2 * k + 1] : 0.0f;
            }
        } else {
            for (int k = 0; k < 9; ++k) Rout[k] = 0.0;
            for (int r = 0; r < 3; ++r) tout[r] = 0.0;
        }
        for (int j = 3 * nv; j < 3 * (L + 1); ++j) v3[j] = 0.0;
        for (int j = 8 * n; j < 8 * L; ++j) e3[j] = 0.0f;
        q.top_mid[gp] = top;
        q.place_flags[gp] = flag;
    }
}

extern "C" int gpe_pattern_place(const int32_t* num_edges, const int32_t* num_verts, const double* vertices, const double* curvature,
                                 const int32_t* curved, const double* rotations, const double* translations, int B, int P, int L,
                                 double* rot_matrix, double* translation, int32_t* top_mid, double* vertices3d, float* edges3d,
                                 int32_t* place_flags, void* stream)
{
    if (B <= 0 || P <= 0 || L <= 0 || (long)P * L > PP_MAXE) return GPE_EINVAL;
    if (!num_edges || !num_verts || !vertices || !curvature || !curved || !rotations || !translations) return GPE_EINVAL;
    if (!rot_matrix || !translation || !top_mid || !vertices3d || !edges3d || !place_flags) return GPE_EINVAL;
    PpParams q{num_edges, num_verts, vertices, curvature, curved, rotations, translations, B, P, L,
               rot_matrix, translation, top_mid, vertices3d, edges3d, place_flags};
    hipLaunchKernelGGL(gpe_pattern_place_kernel, dim3(B), dim3(PP_TPB), 0, (hipStream_t)stream, q);
    GPE_CHECK_LAUNCH();
    return GPE_OK;
}
