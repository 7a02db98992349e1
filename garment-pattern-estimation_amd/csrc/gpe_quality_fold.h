// The fold of the per-pattern quality records (QM_PART doubles per pattern, written by gpe_quality_panel_kernel /
// gpe_quality_stitch_kernel) into the 14-slot result vector and its contributor counts: ONE statement of the order contract, used by
// gpe_quality_final_kernel (csrc/gpe_quality.hip: the patterns of one batch) and gpe_eval_pool_kernel (csrc/gpe_eval.hip: the
// patterns of one group of a whole data set's table).  Records are added in pattern order, with the reference's own number types
// per slot (fp32 sums where the reference sums fp32 tensors, fp64 where it sums Python floats).
#pragma once
#include <stdint.h>

// every product / sum below is rounded on its own, in the reference's order (no contraction into FMAs)
#pragma clang fp contract(off)

#define QM_PART 16           // doubles of workspace per pattern

enum { QM_DISCRETE = 1, QM_SHAPE = 2, QM_ROT = 4, QM_TR = 8, QM_STITCH = 16, QM_FREE = 32, QM_TAG_STATS = 64 };

// record slots per pattern: [0] pattern has the right panel count (0/1), [1] its fp32 share of correctly-sized panels,
// [2] sum of per-panel vertex L2, [3] panels in it, [4] sum of rotation L2, [5] sum of translation L2, [8] stitches
// detected (0/1), [9] precision (fp64), [10] recall (an fp32 value), [11] free-edge decisions equal to the ground truth
struct QmFold {
    float np_acc = 0.f, ne_acc = 0.f, ne_corr = 0.f, rec = 0.f, rec_corr = 0.f;
    double sh = 0, sh_corr = 0, rot = 0, rot_corr = 0, tr = 0, tr_corr = 0, prec = 0, prec_corr = 0;
    long nsh = 0, nsh_corr = 0, nfree = 0;
    int ncorr = 0, nst_corr = 0;

    // the next pattern's record
    __device__ __forceinline__ void add(const double* o, int flags)
    {
        const bool disc = flags & QM_DISCRETE;
        const bool corr = disc && o[0] != 0.0;
        if (disc) {
            np_acc += (float)o[0];
            ne_acc += (float)o[1];
            if (corr) { ne_corr += (float)o[1]; ++ncorr; }
        }
        if (flags & QM_SHAPE) {
            sh += o[2]; nsh += (long)o[3];
            if (corr) { sh_corr += o[2]; nsh_corr += (long)o[3]; }
        }
        if (flags & QM_ROT) { rot += o[4]; if (corr) rot_corr += o[4]; }
        if (flags & QM_TR) { tr += o[5]; if (corr) tr_corr += o[5]; }
        if (flags & QM_STITCH) {
            prec += o[9]; rec += (float)o[10];
            if (corr && o[8] != 0.0) { prec_corr += o[9]; rec_corr += (float)o[10]; ++nst_corr; }
        }
        if (flags & QM_FREE) nfree += (long)o[11];
    }

    // the means over the B patterns that were added -> out fp32 [14], counts int32 [4]
    __device__ __forceinline__ void finish(int B, int P, int L, int flags, float* __restrict__ out, int32_t* __restrict__ counts) const
    {
        const float fB = (float)B;
        for (int k = 0; k < 14; ++k) out[k] = 0.f;
        if (flags & QM_DISCRETE) { out[0] = np_acc / fB; out[1] = ne_acc / fB; out[2] = ne_corr / (float)ncorr; }   // 0 correct: 0/0 = NaN
        if (flags & QM_SHAPE) { out[3] = (float)(sh / (double)nsh); out[4] = (float)(sh_corr / (double)nsh_corr); }
        if (flags & QM_ROT) { out[5] = (float)(rot / ((double)B * P)); out[6] = (float)(rot_corr / ((double)ncorr * P)); }
        if (flags & QM_TR) { out[7] = (float)(tr / ((double)B * P)); out[8] = (float)(tr_corr / ((double)ncorr * P)); }
        if (flags & QM_STITCH) {
            out[9] = (float)(prec / (double)B);
            out[10] = rec / fB;
            out[11] = (float)(prec_corr / (double)nst_corr);
            out[12] = rec_corr / (float)nst_corr;
        }
        if (flags & QM_FREE) out[13] = (float)nfree / (float)((long)B * P * L);
        counts[0] = ncorr;
        counts[1] = (int32_t)nsh_corr;
        counts[2] = nst_corr;
        counts[3] = (int32_t)nsh;
    }
};
