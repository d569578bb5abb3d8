// dfm_poseprep.h - host preparation of the per-pose all-atom calls (api.hip: dfm_atoms_create, dfm_surface_create): argument checks, the
// cell grid of a chain, the ligand in blocks of 64 neighbours, the rounding slack.  Plain C++ without a HIP call, so that
// tests/test_pose_prep_cpu.py runs it under the sanitizers without a GPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "dfm_walkgrid.h"

namespace dfm {

constexpr int POSE_MAX_ATOMS = 1 << 24, POSE_MAX_CELLS = 1 << 24;

// the two atom sets [n][3] and the rotation centre of a creator: the message of the first argument that is wrong, or ""
inline std::string check_atom_sets(int Ar, const float *rec_atoms, int Al, const float *lig_atoms, const float *center)
{
    if (!rec_atoms) return "rec_atoms is NULL";
    if (!lig_atoms) return "lig_atoms is NULL";
    if (!center) return "center is NULL";
    if (Ar < 1 || Al < 1) return "need Ar >= 1 and Al >= 1";
    if (Ar > POSE_MAX_ATOMS || Al > POSE_MAX_ATOMS) return "Ar or Al exceeds 2^24 atoms";
    for (size_t i = 0; i < (size_t)Ar * 3; ++i)
        if (!std::isfinite(rec_atoms[i])) return "rec_atoms: atom " + std::to_string(i / 3) + " is not finite";
    for (size_t i = 0; i < (size_t)Al * 3; ++i)
        if (!std::isfinite(lig_atoms[i])) return "lig_atoms: atom " + std::to_string(i / 3) + " is not finite";
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(center[k])) return "center is not finite";
    return "";
}

// slack of the fp32 pair tests for coordinates up to maxabs (dfm_posewalk.h derives it)
inline float pose_slack(double maxabs) { return std::max(1e-3f, (float)(2.5e-7 * maxabs)); }

// the atoms of one chain sorted by cell of a grid of the given edge over their bounding box (a stable counting sort): lo / hi / dims,
// cell = (z ny + y) nx + x, start [cells + 1], order [n] = atom indices by cell.  false: more than 2^24 cells
struct CellGrid {
    double lo[3], hi[3];
    int dims[3], max_cell = 0;
    std::vector<int32_t> start, order;
};
inline bool build_cell_grid(int n, const float *xyz, double edge, CellGrid &g)
{
    for (int k = 0; k < 3; ++k) g.lo[k] = g.hi[k] = (double)xyz[k];
    for (int i = 1; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            const double v = (double)xyz[(size_t)i * 3 + k];
            g.lo[k] = std::min(g.lo[k], v);
            g.hi[k] = std::max(g.hi[k], v);
        }
    double cells = 1.0;
    for (int k = 0; k < 3; ++k) {
        const double d = std::floor((g.hi[k] - g.lo[k]) / edge) + 1.0;
        cells *= d;
        if (!(cells <= (double)POSE_MAX_CELLS)) return false;
        g.dims[k] = (int)d;
    }
    const int n_cells = g.dims[0] * g.dims[1] * g.dims[2];
    std::vector<int32_t> cell((size_t)n);
    g.start.assign((size_t)n_cells + 1, 0);
    for (int i = 0; i < n; ++i) {
        int c[3];
        for (int k = 0; k < 3; ++k) c[k] = cell_of((double)xyz[(size_t)i * 3 + k], g.lo[k], edge, g.dims[k]);
        cell[(size_t)i] = (c[2] * g.dims[1] + c[1]) * g.dims[0] + c[0];
        ++g.start[(size_t)cell[(size_t)i] + 1];
    }
    g.max_cell = 0;
    for (int c = 0; c < n_cells; ++c) {
        g.max_cell = std::max(g.max_cell, (int)g.start[(size_t)c + 1]);
        g.start[(size_t)c + 1] += g.start[(size_t)c];
    }
    g.order.resize((size_t)n);
    std::vector<int32_t> at(g.start.begin(), g.start.end() - 1);
    for (int i = 0; i < n; ++i) g.order[(size_t)at[(size_t)cell[(size_t)i]]++] = i;
    return true;
}

// atoms [order.size()] as the kernels read them: (x, y, z, radius or 0) of atom order[q] at q
inline std::vector<float> gather4(const std::vector<int32_t> &order, const float *xyz, const float *radius_or_null)
{
    std::vector<float> v(order.size() * 4, 0.f);
    for (size_t q = 0; q < order.size(); ++q) {
        for (int k = 0; k < 3; ++k) v[q * 4 + k] = xyz[(size_t)order[q] * 3 + k];
        if (radius_or_null) v[q * 4 + 3] = radius_or_null[order[q]];
    }
    return v;
}

// the grid as the kernels take it
inline WalkGrid walk_grid(const CellGrid &g, double edge, double grow, const float center[3])
{
    WalkGrid w = {};
    for (int k = 0; k < 3; ++k) { w.lo[k] = g.lo[k]; w.hi[k] = g.hi[k]; w.center[k] = (double)center[k]; }
    w.edge = edge; w.grow = grow;
    w.nx = g.dims[0]; w.ny = g.dims[1]; w.nz = g.dims[2];
    return w;
}

// 21 bits of each cell coordinate interleaved
inline uint64_t morton3(uint32_t x, uint32_t y, uint32_t z)
{
    auto spread = [](uint64_t v) {
        v &= 0x1fffff;
        v = (v | v << 32) & 0x1f00000000ffffull;
        v = (v | v << 16) & 0x1f0000ff0000ffull;
        v = (v | v << 8) & 0x100f00f00f00f00full;
        v = (v | v << 4) & 0x10c30c30c30c30c3ull;
        v = (v | v << 2) & 0x1249249249249249ull;
        return v;
    };
    return spread(x) | spread(y) << 1 | spread(z) << 2;
}

// the ligand in Morton order of its own cells (origin lig_lo = its bounding box's low corner; ties: the caller's order), so that 64
// consecutive atoms are a compact lump: index [Al] = each sorted atom's index in the caller's order, sphere [ceil(Al / 64)][4] = centre
// (relative to the rotation centre) and radius of each block of 64 sorted atoms.  finite: no sphere overflows fp32
struct LigandBlocks {
    std::vector<int32_t> index;
    std::vector<float> sphere;
    bool finite = true;
};
inline LigandBlocks build_ligand_blocks(int Al, const float *lig_atoms, const double lig_lo[3], double edge, const double center[3])
{
    std::vector<std::pair<uint64_t, int32_t>> order((size_t)Al);
    for (int i = 0; i < Al; ++i) {
        uint32_t c[3];
        for (int k = 0; k < 3; ++k) c[k] = (uint32_t)cell_of((double)lig_atoms[(size_t)i * 3 + k], lig_lo[k], edge, 1 << 21);
        order[(size_t)i] = {morton3(c[0], c[1], c[2]), i};
    }
    std::sort(order.begin(), order.end());
    const int nblk = (Al + 63) / 64;
    LigandBlocks lb;
    lb.index.resize((size_t)Al);
    lb.sphere.assign((size_t)nblk * 4, 0.f);
    for (int i = 0; i < Al; ++i) lb.index[(size_t)i] = order[(size_t)i].second;
    auto at = [&](int i, int k) { return (double)lig_atoms[(size_t)lb.index[(size_t)i] * 3 + k]; };
    for (int b = 0; b < nblk; ++b) {
        const int i0 = b * 64, i1 = std::min(Al, i0 + 64);
        double lo[3], hi[3];
        for (int k = 0; k < 3; ++k) lo[k] = hi[k] = at(i0, k);
        for (int i = i0 + 1; i < i1; ++i)
            for (int k = 0; k < 3; ++k) {
                lo[k] = std::min(lo[k], at(i, k));
                hi[k] = std::max(hi[k], at(i, k));
            }
        // the centre as the fp32 the kernel reads, the radius measured from THAT point and rounded up
        float c[3];
        for (int k = 0; k < 3; ++k) c[k] = (float)(0.5 * (lo[k] + hi[k]) - center[k]);
        double r2 = 0.0;
        for (int i = i0; i < i1; ++i) {
            double d2 = 0.0;
            for (int k = 0; k < 3; ++k) {
                const double d = (at(i, k) - center[k]) - (double)c[k];
                d2 += d * d;
            }
            r2 = std::max(r2, d2);
        }
        for (int k = 0; k < 3; ++k) lb.sphere[(size_t)b * 4 + k] = c[k];
        lb.sphere[(size_t)b * 4 + 3] = std::nextafter((float)(std::sqrt(r2) * (1.0 + 1e-6) + 1e-6), INFINITY);
    }
    for (float v : lb.sphere) lb.finite = lb.finite && std::isfinite(v);
    return lb;
}

}  // namespace dfm
