// dfm_walkgrid.h - the receptor's cell grid of the per-pose all-atom calls and its binning formula, in plain C++: the host builds the
// grid with them (dfm_poseprep.h), the kernels walk it (dfm_posewalk.h).  Also the bits a polar atom of the hydrogen-bond call carries
// in its float4, which the host packs and kernels_hbond.hip reads, and the padded length of the pair potential's squared edges.
#pragma once

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define DFM_HOST_DEVICE __host__ __device__
#else
#define DFM_HOST_DEVICE
#endif

namespace dfm {

// the receptor's bounding box lo / hi (= the grid's origin and extent), the rotation centre, the grid of nx x ny x nz cells of edge
// `edge`, and `grow`, by which every box test is widened
struct WalkGrid {
    double lo[3], hi[3], center[3];
    double edge, grow;
    int nx, ny, nz;
};

// cell coordinate of x along one axis, clamped to the grid: the one binning formula of host and device
DFM_HOST_DEVICE inline int cell_of(double x, double origin, double edge, int n)
{
    double c = floor((x - origin) / edge);
    c = c < 0.0 ? 0.0 : (c > (double)(n - 1) ? (double)(n - 1) : c);
    return (int)c;
}

// hydrogen bonds and salt bridges: the role bits of dfmdock_amd/hbonds.py; an atom's bits are role | compact charged-residue index <<
// HB_RES_SHIFT
constexpr uint32_t HB_DONOR = 1, HB_ACCEPTOR = 2, HB_CATION = 4, HB_ANION = 8, HB_SIDECHAIN = 16, HB_ROLE_MASK = 31;
constexpr int HB_RES_SHIFT = 8;

// slots of the pair potential's squared bin edges as the host pads them with +inf (dfm_poseprep.h: pairpot_edges2) and the bin search of
// kernels_pairpot.hip reads them: twice the largest step of the search over at most 65 edges
constexpr int PAIRPOT_E2_SLOTS = 128;

}  // namespace dfm
