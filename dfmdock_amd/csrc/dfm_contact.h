// dfm_contact.h - the backbone contact distance shared by kernels_metrics.hip (native contacts recovered) and kernels_consensus.hip
// (contacts of every residue pair of every pose).  Device code only; translation units that include it are built with
// -ffp-contract=off, so the arithmetic rounds like numpy's.
#pragma once

#include <hip/hip_runtime.h>

namespace dfm {

// minimum over the 9 atom pairs of |a_i - b_j| (a, b: one residue each, 9 floats), as metrics._min_dist_pairs
__device__ inline double min_dist9(const float *__restrict__ a, const float *__restrict__ b)
{
    double av[9], bv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { av[k] = (double)a[k]; bv[k] = (double)b[k]; }
    double best = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double dx = av[3 * i] - bv[3 * j], dy = av[3 * i + 1] - bv[3 * j + 1], dz = av[3 * i + 2] - bv[3 * j + 2];
            const double d = sqrt((dx * dx + dy * dy) + dz * dz);
            // numpy's min propagates NaN
            best = (i == 0 && j == 0) ? d : ((d < best || d != d) ? d : best);
        }
    return best;
}

}  // namespace dfm
