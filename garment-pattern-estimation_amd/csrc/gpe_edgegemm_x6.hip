// "bf16x6": the three-term bf16 policy of the split-precision single-role edge kernel (gpe_edgegemm_split_kernel.h).
#include "gpe_edgegemm_split_kernel.h"

// Only variants that fit the 512-register budget of a lone wave WITHOUT scratch spills are launched (checked with
// scripts/kernel_resources.py): 10 N-tiles always, 13 x 10 forward only; 13 N-tiles otherwise keep 252 + 24 weight registers
// resident, which leaves too little for the 16-row staging / epilogue state — those shapes stay on the exact-fp32 kernel.
struct Bf16x6Menu {
    static constexpr bool has(int amode, int emode, int NT, int KCH) { return NT == 10 || KCH == 10; }
};

int gpe_edge_bf16x6(const RgParams& p, int amode, int emode, int NT, int KCH, int stats_nblk, hipStream_t s)
{
    if (NT == 13 && emode != E_EDGE_FWD) return GPE_EDGE_NOT_MINE;       // (instantiated, as they always were; they spill)
    return split_select<SplitBf16x3, Bf16x6Menu>(p, amode, emode, NT, KCH, stats_nblk, s);
}
