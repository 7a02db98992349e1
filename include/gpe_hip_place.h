/* Feature addition to the C ABI of libgpe_hip.so (include/gpe_hip.h; gpe_abi_version() stays 7): the panels of a decoded prediction
 * placed in 3D (csrc/gpe_pattern_place.hip) — what the reference's NNSewingPattern builds on the host, per panel, before it hands a
 * predicted pattern's edges to the stitch classifier (_3D_edges_per_panel, nn/data/pattern_converter.py:517-552) and when it turns the
 * predicted "universal" translation into the translation of the panel's origin (:281-288).  The conventions are those of
 * include/gpe_hip_fit.h: caller-owned memory, 0 / -22 (bad argument, checked before any launch and before any pointer is touched) /
 * -5 (launch failure), the HIP stream as the last argument.  Bound by gpe_amd/_lib.py (PLACE_HEADERS) and seen by every definition
 * (csrc/gpe_common.h).
 *
 * ---- what is computed, per non-empty panel (num_edges > 0), everything in fp64, every product and sum rounded on its own --------------
 *   1. q = (x, y, z, w) = rotations[b, p] / |rotations[b, p]| (scalar last, as scipy takes it).  A norm that is zero or not finite sets
 *      bit 0 of place_flags[b, p] (GPE_PLACE_BAD_QUAT) and the identity is used.  R = the matrix of the unit quaternion
 *      (scipy Rotation.as_matrix); a point p2 of the panel lies at R . (p2.x, p2.y, 0) + translation in 3D (_point_in_3D).
 *   2. The universal point: of the four midpoints of the sides of the bounding box of the panel's num_verts 2D vertices, in the order
 *          0 top (mid_x, max_y)   1 bottom (mid_x, min_y)   2 right (max_x, mid_y)   3 left (min_x, mid_y)
 *      the one whose 3D image has the largest y; on a tie the first in that order (argmax).  The 3D y of a midpoint m is
 *      R[1][0] m.x + R[1][1] m.y (the translation is common to the four).  top_mid[b, p] is its number.
 *      THIS RULE is the one statement here that rests on the published definition of the reference's external `pattern` package
 *      (_panel_universal_transtation) alone; everything else is pinned by the reference's own text.
 *   3. translation[b, p] = translations[b, p] - R . (m.x, m.y, 0): the decoded translation is that of the universal point.
 *   4. vertices3d[b, p, v] = R . (v.x, v.y, 0) + translation, v < num_verts.
 *   5. edges3d[b, p, k] = [start xyz, end xyz, curvature.x, curvature.y] of kept edge k < num_edges, rounded to fp32: from vertex k to
 *      vertex k + 1, or to vertex 0 when k + 1 == num_verts (the last edge of a closed loop); the curvature is (0, 0) where
 *      curved[b, p, k] == 0.  Rows are compact (kept edge k, not the decoder's row slot): [B, P, L, 8] with num_edges is what
 *      gpe_stitch_pairs takes.
 * An empty panel gets top_mid -1, place_flags 0 and zeros; every tail (vertices past num_verts, edge rows past num_edges) is zeros.
 * One launch, one wave per garment and one lane per panel: no atomics, every output element written by exactly one thread, so the
 * results are bit-identical from run to run and for any CU reservation.  Nothing is allocated or read back: legal in a stream capture.
 */
#ifndef GPE_HIP_PLACE_H
#define GPE_HIP_PLACE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GPE_PLACE_BAD_QUAT 1

/*   num_edges, num_verts   int32 [B, P]             as gpe_pattern_decode wrote them (values outside 0 .. L / 0 .. L + 1 are clamped)
 *   vertices               fp64 [B, P, L + 1, 2]
 *   curvature, curved      fp64 [B, P, L, 2], int32 [B, P, L]
 *   rotations              fp64 [B, P, 4]           quaternions, scalar last, any non-zero length
 *   translations           fp64 [B, P, 3]           of the universal point
 *   B, P, L                B >= 1, 1 <= P * L <= 1024
 *   rot_matrix             fp64 [B, P, 3, 3]        row-major
 *   translation            fp64 [B, P, 3]           of the panel's origin
 *   top_mid                int32 [B, P]
 *   vertices3d             fp64 [B, P, L + 1, 3]
 *   edges3d                fp32 [B, P, L, 8]
 *   place_flags            int32 [B, P] */
int gpe_pattern_place(const int32_t* num_edges, const int32_t* num_verts, const double* vertices, const double* curvature,
                      const int32_t* curved, const double* rotations, const double* translations, int B, int P, int L,
                      double* rot_matrix, double* translation, int32_t* top_mid, double* vertices3d, float* edges3d,
                      int32_t* place_flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPE_HIP_PLACE_H */
