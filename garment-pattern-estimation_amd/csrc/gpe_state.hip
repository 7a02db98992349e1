// The process-global state of libgpe_hip.so, all of it (include/gpe_hip.h, Conventions): the ABI version, the arithmetic mode with
// its f16x3 size gate, the debug mask and the CU reservation, each with its setter.  Host code only: no kernel, no device
// function.  Every other file reads this state through the accessors (gpe_math_get / gpe_debug_get of the C ABI; gpe_math_rowgemm,
// gpe_math_redgemm, gpe_h3_min_rows and gpe_num_cus of gpe_common.h) at the moment it decides a launch; nothing keeps a copy.
#include "gpe_common.h"

extern "C" int gpe_abi_version(void) { return 7; }

static int g_gpe_dbg = 0;
extern "C" int gpe_debug_set(int flags) { g_gpe_dbg = flags; return 0; }
extern "C" int gpe_debug_get(void) { return g_gpe_dbg; }

static int g_gpe_math = 0;
extern "C" int gpe_math_get(void) { return g_gpe_math; }
extern "C" int gpe_math_set(int mode)
{
    if (mode < 0 || mode > 4) return GPE_EINVAL;
    const int prev = g_gpe_math;
    g_gpe_math = mode;
    return prev;
}
// row GEMMs (forward, input-gradient half): 0 exact fp32, 1 two-term split-bf16 (modes 1, 2), 2 three-term split-bf16
// (mode 3), 3 two-term split-fp16 on tensor-normalised operands (mode 4)
int gpe_math_rowgemm()
{
    const int mode = g_gpe_math;
    return mode == 4 ? 3 : mode == 3 ? 2 : (mode != 0 ? 1 : 0);
}
// the weight-gradient reduce-GEMM: split-bf16 only in mode 1; mode 4: split-fp16 where the operand scales are known
int gpe_math_redgemm()
{
    const int mode = g_gpe_math;
    return mode == 1 ? 1 : mode == 4 ? 2 : 0;
}

static long g_h3_min_rows = GPE_H3_MIN_ROWS_DEFAULT;
long gpe_h3_min_rows() { return g_h3_min_rows; }
extern "C" long gpe_f16x3_min_rows(void) { return g_h3_min_rows; }
extern "C" long gpe_f16x3_min_rows_set(long rows)
{
    if (rows < 0) return GPE_EINVAL;
    const long prev = g_h3_min_rows;
    g_h3_min_rows = rows;
    return prev;
}

// compute units the persistent kernels may fill: the device's count minus the caller's reservation (gpe_reserve_cus_set)
static int g_reserved_cus = 0;
extern "C" int gpe_reserve_cus_set(int n)
{
    if (n < 0 || n > 192) return GPE_EINVAL;
    const int prev = g_reserved_cus;
    g_reserved_cus = n;
    return prev;
}
int gpe_num_cus()
{
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256 - g_reserved_cus;
    int& c = cus[dev & 63];
    if (!c) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess) c = prop.multiProcessorCount;
        if (c <= 0) c = 256;
    }
    const int left = c - g_reserved_cus;
    return left > 8 ? left : 8;
}
