// Four-row (pseudo-)point instances of the two-waves-per-SIMD edge kernel (gpe_edgegemm_w8_kernel.h, KK = 4): BASELINE cfg 4's
// neighbourhood k = 20 (GarmentSegmentPattern3D, /root/reference/models/att/att.yaml with k_neighbors 20) runs every per-point
// launch as five pseudo-points of four rows (gpe_edge_retile: P rows through RgParams::pmagic, per-pseudo-point maxima /
// sums into the caller's workspace, folded afterwards) and the in-place backward, which needs nothing per point, simply tiled
// by four.  Rounds 2 - 4 ran these on the single-role kernel.
#include "gpe_edgegemm_w8_kernel.h"

int gpe_w8_select_k4(const RgParams& p, int amode, int emode, int NT, int KCH, int stats_nblk, hipStream_t s)
{
    return w8_select<4>(p, amode, emode, NT, KCH, stats_nblk, s);
}
