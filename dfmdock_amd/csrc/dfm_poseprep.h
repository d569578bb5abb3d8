// dfm_poseprep.h - host preparation of the per-pose all-atom calls (api_pose.hip: dfm_atoms_create, dfm_surface_create, dfm_iface_create,
// dfm_rescon_create, dfm_hbond_create, dfm_pairpot_create, dfm_density_create): argument checks, the cell grid of a chain, the ligand in blocks of 64 neighbours, the rounding
// slack, the frame of the cutoff-based creators, the interface energy's parameter limits and overflow bound, the residue contacts' limits, residue bits, class masks and chunk
// size, the hydrogen bonds' limits, role bits and charged residues, the pair potential's limits, quantised table, squared edges, pair
// bound and chunk size, the density fit's limits, interleaved grid, sum bound and chunk size.  Plain C++ without a HIP call, so that tests/test_pose_prep_cpu.py, tests/test_ifenergy_cpu.py,
// tests/test_affinity_cpu.py, tests/test_hbonds_cpu.py, tests/test_pairpot_cpu.py and tests/test_density_cpu.py run it under the sanitizers without a GPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
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

// The frame of a rigid-pose creator whose reach is a cutoff (dfm_atoms_create, dfm_iface_create, dfm_rescon_create, dfm_hbond_create):
// the receptor's grid of cells of the reach, the grid as the kernels take it, the fp32 reject threshold thr = reach * 1.0001 + slack
// (dfm_posewalk.h) with reject2 = thr^2, the ligand's low corner and the ligand in blocks.  maxabs = the largest coordinate of the
// receptor's box + 2 reach + 1.  These numbers decide which pairs the fp32 early reject may skip.
struct PoseFrame {
    CellGrid gr;
    WalkGrid g = {};
    float thr = 0.f, reject2 = 0.f;
    double lig_lo[3] = {0.0, 0.0, 0.0};
    LigandBlocks lb;
};
// `reach_name` names the reach in the refusal ("contact cutoff", "cutoff", "larger cutoff"), `lig_name` the ligand's argument; returns
// the message of the first thing that is wrong, or ""
inline std::string build_pose_frame(int Ar, const float *rec_atoms, int Al, const float *lig_atoms, const float center[3], float reach,
                                    const char *reach_name, PoseFrame &f, const char *lig_name = "lig_atoms")
{
    if (!build_cell_grid(Ar, rec_atoms, (double)reach, f.gr))
        return std::string("the receptor's bounding box needs more than 2^24 cells of the ") + reach_name;
    double maxabs = 0.0;
    for (int k = 0; k < 3; ++k) maxabs = std::max(maxabs, std::max(std::fabs(f.gr.lo[k]), std::fabs(f.gr.hi[k])));
    maxabs += 2.0 * (double)reach + 1.0;
    f.thr = reach * 1.0001f + pose_slack(maxabs);
    f.g = walk_grid(f.gr, (double)reach, (double)f.thr, center);
    f.reject2 = f.thr * f.thr;
    if (!std::isfinite(f.reject2)) return "cutoffs must be finite and > 0";
    for (int k = 0; k < 3; ++k) f.lig_lo[k] = (double)lig_atoms[k];
    for (int i = 1; i < Al; ++i)
        for (int k = 0; k < 3; ++k) f.lig_lo[k] = std::min(f.lig_lo[k], (double)lig_atoms[(size_t)i * 3 + k]);
    f.lb = build_ligand_blocks(Al, lig_atoms, f.lig_lo, f.g.edge, f.g.center);
    if (!f.lb.finite) return std::string(lig_name) + " / center: the ligand's extent about the centre overflows fp32";
    return "";
}

// Interface energy (api_pose.hip: dfm_iface_create; kernels_iface.hip).  The limits of the per-atom parameters [n] of one chain (`who`:
// "rec" or "lig") and of the call's scalars: the message of the first one that is wrong, or "".
inline std::string check_iface_atoms(const char *who, int n, const float *rmin_half, const float *sqrt_eps, const float *charge)
{
    const std::string w(who);
    if (!rmin_half) return w + "_rmin_half is NULL";
    if (!sqrt_eps) return w + "_sqrt_eps is NULL";
    if (!charge) return w + "_charge is NULL";
    for (int i = 0; i < n; ++i) {
        if (!(std::isfinite(rmin_half[i]) && rmin_half[i] > 0.f && rmin_half[i] <= 8.f))
            return w + "_rmin_half: atom " + std::to_string(i) + " is not in (0, 8]";
        if (!(std::isfinite(sqrt_eps[i]) && sqrt_eps[i] >= 0.f && sqrt_eps[i] <= 2.f))
            return w + "_sqrt_eps: atom " + std::to_string(i) + " is not in [0, 2]";
        if (!(std::isfinite(charge[i]) && std::fabs(charge[i]) <= 4.f)) return w + "_charge: atom " + std::to_string(i) + " is not in [-4, 4]";
    }
    return "";
}
inline std::string check_iface_scalars(float cutoff, float soft, float elec_min_dist, float dielectric_slope)
{
    if (!(std::isfinite(cutoff) && cutoff > 0.f && cutoff <= 16.f)) return "cutoff must be in (0, 16]";
    if (!(std::isfinite(soft) && soft >= 0.5f && soft <= 1.f)) return "soft must be in [0.5, 1]";
    if (!(std::isfinite(elec_min_dist) && elec_min_dist >= 1.f)) return "elec_min_dist must be finite and >= 1";
    if (!(std::isfinite(dielectric_slope) && dielectric_slope > 0.f)) return "dielectric_slope must be finite and > 0";
    return "";
}

// The integer sums of the interface energy can not wrap.  One quantum is 2^-20 kcal/mol.  With s2 = Rm^2 / max(r2, (soft Rm)^2) <=
// soft^-2 a pair has |rep| <= e soft^-12, |att| <= 2 e soft^-6 and |elec| <= (332.0637 / slope) |q_a q_b| / m^2, where e <= E = (largest
// sqrt_eps of the receptor) (largest of the ligand), |q_a q_b| <= Q likewise and m = elec_min_dist.  At the limits of the checks above
// (sqrt_eps <= 2, soft >= 0.5, |q| <= 4, m >= 1) that is rep <= 4 * 4096 = 2^14 kcal/mol = 2^34 quanta, att <= 2^9 kcal/mol and
// elec <= 5313.1 / slope kcal/mol, below 2^14 for slope >= 0.33; a smaller slope is allowed and raises the bound, which is why the bound
// is taken from the complex's own E, Q, soft, m and slope and not from the limits.  A ligand atom's pairs lie within the cutoff = the
// cell edge, so in the 27 cells about its own: a pose has at most pairs = Al min(Ar, 27 max_cell_atoms) of them.  Every sum the call forms
// (rep, att, elec per pose; rep + att and elec per ligand atom) is then at most
//     pairs * (max(rep + att, elec) * (1 + 2^-30) * 2^20 + 2)     quanta
// in magnitude: 2^-30 covers the rounding of the few fp64 operations of a term, + 2 the rounding of rep and att to integers.  The
// creator rejects a complex for which this is not below 2^62 (or not finite), so every partial sum - and every single term's
// conversion to int64 - is far inside the range.
struct IfaceBound {
    double term_kcal, pairs, sum_quanta;
    bool ok;
};
inline IfaceBound iface_sum_bound(int Ar, const float *rec_sqrt_eps, const float *rec_charge, int Al, const float *lig_sqrt_eps,
                                  const float *lig_charge, int max_cell_atoms, float soft, float elec_min_dist, float dielectric_slope)
{
    double er = 0.0, el = 0.0, qr = 0.0, ql = 0.0;
    for (int i = 0; i < Ar; ++i) {
        er = std::max(er, (double)rec_sqrt_eps[i]);
        qr = std::max(qr, std::fabs((double)rec_charge[i]));
    }
    for (int i = 0; i < Al; ++i) {
        el = std::max(el, (double)lig_sqrt_eps[i]);
        ql = std::max(ql, std::fabs((double)lig_charge[i]));
    }
    const double s = 1.0 / (double)soft, s6 = std::pow(s, 6.0), m = (double)elec_min_dist;
    const double vdw = er * el * (s6 * s6 + 2.0 * s6);
    const double q = qr * ql, elec = q > 0.0 ? (332.0637 / (double)dielectric_slope) * q / (m * m) : 0.0;
    IfaceBound b;
    b.term_kcal = std::max(vdw, elec);
    b.pairs = (double)Al * std::min((double)Ar, 27.0 * (double)max_cell_atoms);
    b.sum_quanta = b.pairs * (b.term_kcal * (1.0 + 9.4e-10) * 1048576.0 + 2.0);
    b.ok = std::isfinite(b.sum_quanta) && b.sum_quanta < 4611686018427387904.0;
    return b;
}

// per-atom parameters as the kernel reads them: (rmin_half, sqrt_eps, charge, 0) of atom order[q] at q
inline std::vector<float> gather_iface(const std::vector<int32_t> &order, const float *rmin_half, const float *sqrt_eps, const float *charge)
{
    std::vector<float> v(order.size() * 4, 0.f);
    for (size_t q = 0; q < order.size(); ++q) {
        v[q * 4] = rmin_half[order[q]];
        v[q * 4 + 1] = sqrt_eps[order[q]];
        v[q * 4 + 2] = charge[order[q]];
    }
    return v;
}

// Residue contacts (api_pose.hip: dfm_rescon_create; kernels_rescon.hip).  The limits: residues per chain, poses per call, and the bytes of
// bitmap [poses of a chunk][Lr][W] a call may hold, which fix the chunk.
constexpr int RESCON_MAX_RES = 4096, RESCON_MAX_POSES = 65536, RESCON_MAX_CHUNK = 32768;
constexpr size_t RESCON_SCRATCH_BYTES = (size_t)64 << 20;

// words of one bitmap row: one bit per receptor residue
inline int rescon_words(int Rr) { return (Rr + 31) / 32; }

// the residue index of every atom [n] and the class of every residue [n_res] of one chain (`who`: "rec" or "lig"): the message of the
// first thing that is wrong, or ""
inline std::string check_rescon_chain(const char *who, int n, const int32_t *res, int n_res, const uint8_t *cls)
{
    const std::string w(who);
    if (!res) return w + "_res is NULL";
    if (!cls) return w + "_class is NULL";
    if (n_res < 1 || n_res > RESCON_MAX_RES) return w + ": need 1 <= residues <= " + std::to_string(RESCON_MAX_RES);
    for (int i = 0; i < n; ++i)
        if (res[i] < 0 || res[i] >= n_res)
            return w + "_res: atom " + std::to_string(i) + " has residue " + std::to_string(res[i]) + " outside [0, " + std::to_string(n_res) + ")";
    for (int i = 0; i < n_res; ++i)
        if (cls[i] > 2) return w + "_class: residue " + std::to_string(i) + " has class " + std::to_string((int)cls[i]) + ", not 0, 1 or 2";
    return "";
}
inline std::string check_rescon_cutoff(float cutoff)
{
    if (!(std::isfinite(cutoff) && cutoff > 0.f && cutoff <= 16.f)) return "cutoff must be in (0, 16]";
    return "";
}

// atoms as k_rescon reads them: (x, y, z, the BITS of the residue index) of atom order[q] at q.  The fourth component is never used as a
// number: it travels through the staging as 32 bits
inline std::vector<float> gather4_res(const std::vector<int32_t> &order, const float *xyz, const int32_t *res)
{
    std::vector<float> v(order.size() * 4, 0.f);
    for (size_t q = 0; q < order.size(); ++q) {
        for (int k = 0; k < 3; ++k) v[q * 4 + k] = xyz[(size_t)order[q] * 3 + k];
        static_assert(sizeof(float) == sizeof(int32_t), "bits");
        std::memcpy(&v[q * 4 + 3], &res[order[q]], sizeof(int32_t));
    }
    return v;
}

// mask [3][W]: bit i & 31 of word i >> 5 of mask c is set iff receptor residue i has class c
inline std::vector<uint32_t> rescon_class_masks(int Rr, const uint8_t *cls)
{
    const int W = rescon_words(Rr);
    std::vector<uint32_t> m((size_t)3 * W, 0u);
    for (int i = 0; i < Rr; ++i) m[(size_t)cls[i] * W + (i >> 5)] |= 1u << (i & 31);
    return m;
}

// poses of one chunk of a call: as many bitmaps [Lr][W] of 32-bit words as fit `budget` bytes, at least 1, at most RESCON_MAX_CHUNK
inline int rescon_chunk_poses(int Lr, int Rr, size_t budget = RESCON_SCRATCH_BYTES)
{
    const size_t per_pose = (size_t)Lr * (size_t)rescon_words(Rr) * sizeof(uint32_t);
    return (int)std::min<size_t>((size_t)RESCON_MAX_CHUNK, std::max<size_t>(1, budget / per_pose));
}

// Hydrogen bonds and salt bridges (api_pose.hip: dfm_hbond_create; kernels_hbond.hip).  The atoms of a chain are its POLAR atoms only.  The
// limits: residues per chain, poses per call, the largest cutoff (the role bits: dfm_walkgrid.h).
constexpr int HBOND_MAX_RES = RESCON_MAX_RES, HBOND_MAX_POSES = RESCON_MAX_POSES;
constexpr float HBOND_MAX_CUTOFF = 8.f;

// the antecedent [n][3], role [n] and residue index [n] of every polar atom of one chain (`who`: "rec" or "lig"): the message of the
// first thing that is wrong, or ""
inline std::string check_hbond_chain(const char *who, int n, const float *ante, const uint8_t *role, const int32_t *res, int n_res)
{
    const std::string w(who);
    if (!ante) return w + "_ante is NULL";
    if (!role) return w + "_role is NULL";
    if (!res) return w + "_res is NULL";
    if (n_res < 1 || n_res > HBOND_MAX_RES) return w + ": need 1 <= residues <= " + std::to_string(HBOND_MAX_RES);
    for (size_t i = 0; i < (size_t)n * 3; ++i)
        if (!std::isfinite(ante[i])) return w + "_ante: atom " + std::to_string(i / 3) + " is not finite";
    for (int i = 0; i < n; ++i) {
        if (role[i] & ~HB_ROLE_MASK) return w + "_role: atom " + std::to_string(i) + " has role " + std::to_string((int)role[i]) + " outside the five bits";
        if (res[i] < 0 || res[i] >= n_res)
            return w + "_res: atom " + std::to_string(i) + " has residue " + std::to_string(res[i]) + " outside [0, " + std::to_string(n_res) + ")";
    }
    return "";
}
inline std::string check_hbond_scalars(float hb_cutoff, double min_cos2, float salt_cutoff)
{
    if (!(std::isfinite(hb_cutoff) && hb_cutoff > 0.f && hb_cutoff <= HBOND_MAX_CUTOFF)) return "hb_cutoff must be in (0, 8]";
    if (!(std::isfinite(salt_cutoff) && salt_cutoff > 0.f && salt_cutoff <= HBOND_MAX_CUTOFF)) return "salt_cutoff must be in (0, 8]";
    if (!(min_cos2 >= 0.0 && min_cos2 < 1.0)) return "min_cos2 must be in [0, 1): the squared cosine of an angle in [90, 180)";
    return "";
}

// the charged residues of one chain - those with at least one CATION or ANION atom - numbered in residue order: compact [n_res] = that
// number or -1; returns how many there are (0 is legal)
inline int hbond_charged_residues(int n, const uint8_t *role, const int32_t *res, int n_res, std::vector<int32_t> &compact)
{
    compact.assign((size_t)n_res, -1);
    for (int i = 0; i < n; ++i)
        if (role[i] & (HB_CATION | HB_ANION)) compact[(size_t)res[i]] = 0;
    int count = 0;
    for (int r = 0; r < n_res; ++r)
        if (compact[(size_t)r] == 0) compact[(size_t)r] = count++;
    return count;
}

// atoms as k_hbond reads them: (x, y, z, the BITS role | compact charged-residue index << 8) of atom order[q] at q; an atom that is
// neither cation nor anion carries index 0, which is never read
inline std::vector<float> gather4_hbond(const std::vector<int32_t> &order, const float *xyz, const uint8_t *role, const int32_t *res,
                                        const std::vector<int32_t> &compact)
{
    std::vector<float> v(order.size() * 4, 0.f);
    for (size_t q = 0; q < order.size(); ++q) {
        const int32_t a = order[q];
        for (int k = 0; k < 3; ++k) v[q * 4 + k] = xyz[(size_t)a * 3 + k];
        const bool charged = (role[a] & (HB_CATION | HB_ANION)) != 0;
        const uint32_t b = (uint32_t)role[a] | (charged ? (uint32_t)compact[(size_t)res[a]] << HB_RES_SHIFT : 0u);
        std::memcpy(&v[q * 4 + 3], &b, sizeof(b));
    }
    return v;
}

// poses of one chunk of a call: the bitmap of a pose is [Lc][ceil(Rc / 32)] words over the CHARGED residues of the two chains; a chain
// without one leaves a bitmap of one word that nothing reads
inline int hbond_chunk_poses(int Lc, int Rc, size_t budget = RESCON_SCRATCH_BYTES) { return rescon_chunk_poses(std::max(Lc, 1), std::max(Rc, 1), budget); }

// Tabulated pair potential (api_pose.hip: dfm_pairpot_create; kernels_pairpot.hip).  The limits: atom types, distance bins, the largest
// table entry in kcal/mol, poses per launch, and the bytes of counts plus per-atom output a chunk of a call may hold.
constexpr int PAIRPOT_MAX_TYPES = 256, PAIRPOT_MAX_BINS = 64, PAIRPOT_MAX_CHUNK = 32768;
constexpr float PAIRPOT_MAX_ENTRY = 1024.f, PAIRPOT_MAX_CUTOFF = 16.f;
constexpr size_t PAIRPOT_CHUNK_BYTES = (size_t)64 << 20;

// the bin edges [NB + 1]: the message of the first thing that is wrong, or ""
inline std::string check_pairpot_edges(int NB, const float *edges)
{
    if (NB < 1 || NB > PAIRPOT_MAX_BINS) return "need 1 <= NB <= " + std::to_string(PAIRPOT_MAX_BINS);
    if (!edges) return "edges is NULL";
    for (int k = 0; k <= NB; ++k)
        if (!std::isfinite(edges[k])) return "edges: edge " + std::to_string(k) + " is not finite";
    for (int k = 0; k < NB; ++k)
        if (!(edges[k] < edges[k + 1])) return "edges: edge " + std::to_string(k + 1) + " is not above edge " + std::to_string(k);
    if (!(edges[0] >= 0.f)) return "edges: edge 0 is below 0";
    if (!(edges[NB] <= PAIRPOT_MAX_CUTOFF)) return "edges: the last edge is above 16";
    return "";
}
// the table [T][T][NB], kcal/mol
inline std::string check_pairpot_table(int T, int NB, const float *table)
{
    if (T < 1 || T > PAIRPOT_MAX_TYPES) return "need 1 <= T <= " + std::to_string(PAIRPOT_MAX_TYPES);
    if (NB < 1 || NB > PAIRPOT_MAX_BINS) return "need 1 <= NB <= " + std::to_string(PAIRPOT_MAX_BINS);
    if (!table) return "table is NULL";
    const size_t n = (size_t)T * T * NB;
    for (size_t i = 0; i < n; ++i)
        if (!(std::isfinite(table[i]) && std::fabs(table[i]) <= PAIRPOT_MAX_ENTRY))
            return "table: entry " + std::to_string(i) + " is not in [-1024, 1024]";
    return "";
}
// the type [n] of every atom of one chain (`who`: "rec" or "lig")
inline std::string check_pairpot_types(const char *who, int n, const int32_t *type, int T)
{
    const std::string w(who);
    if (!type) return w + "_type is NULL";
    for (int i = 0; i < n; ++i)
        if (type[i] < 0 || type[i] >= T)
            return w + "_type: atom " + std::to_string(i) + " has type " + std::to_string(type[i]) + " outside [0, " + std::to_string(T) + ")";
    return "";
}

// table_q as the kernel reads it: (int32) rint((double) table * 2^20), ties to even, |q| <= 2^30, TRANSPOSED from the caller's [ligand
// type ta][receptor type tb][bin] to [tb][ta][bin] - the staged receptor atom is a broadcast, so the 64 gathers of one iteration fall
// inside the one slab of T NB entries of its type
inline std::vector<int32_t> quantise_pairpot(int T, int NB, const float *table)
{
    std::vector<int32_t> q((size_t)T * T * NB);
    for (int ta = 0; ta < T; ++ta)
        for (int tb = 0; tb < T; ++tb)
            for (int k = 0; k < NB; ++k)
                q[((size_t)tb * T + ta) * NB + k] = (int32_t)std::nearbyint((double)table[((size_t)ta * T + tb) * NB + k] * 1048576.0);
    return q;
}

// e2 [PAIRPOT_E2_SLOTS]: (double) edges[k] * (double) edges[k] - exact, 24 bits times 24 bits - then +inf
inline std::vector<double> pairpot_edges2(int NB, const float *edges)
{
    std::vector<double> e2((size_t)PAIRPOT_E2_SLOTS, (double)INFINITY);
    for (int k = 0; k <= NB; ++k) e2[(size_t)k] = (double)edges[k] * (double)edges[k];
    return e2;
}

// The integer results of the pair potential can not wrap.  A ligand atom's pairs lie within the cutoff = the cell edge, so in the 27 cells
// about its own: a pose has at most pairs = Al min(Ar, 27 max_cell_atoms) of them.  The creator refuses a complex for which that exceeds
// 2^31 - 1: under it every entry of counts (and their sum) fits int32, and |energy_q| <= pairs 2^30 < 2^61.
struct PairpotBound {
    double pairs;
    bool ok;
};
inline PairpotBound pairpot_pair_bound(int Ar, int Al, int max_cell_atoms)
{
    PairpotBound b;
    b.pairs = (double)Al * std::min((double)Ar, 27.0 * (double)max_cell_atoms);
    b.ok = b.pairs <= 2147483647.0;
    return b;
}

// what rides next to each receptor atom: (the BITS of its type, the BITS of its slab's offset type T NB in table_q, 0, 0) of atom
// order[q] at q
inline std::vector<float> gather4_pairpot(const std::vector<int32_t> &order, const int32_t *type, int T, int NB)
{
    std::vector<float> v(order.size() * 4, 0.f);
    for (size_t q = 0; q < order.size(); ++q) {
        const int32_t t = type[order[q]], slab = t * T * NB;
        std::memcpy(&v[q * 4], &t, sizeof(t));
        std::memcpy(&v[q * 4 + 1], &slab, sizeof(slab));
    }
    return v;
}

// poses of one chunk of a call: as many as fill `budget` bytes of counts [T][T][NB] int32 plus per-atom output [Al] int64, whichever of
// the two the call asks for; without either the launch alone bounds it
inline int pairpot_chunk_poses(int Al, int T, int NB, bool per_atom, bool counts, size_t budget = PAIRPOT_CHUNK_BYTES)
{
    const size_t per_pose = (counts ? (size_t)T * T * NB * sizeof(int32_t) : 0) + (per_atom ? (size_t)Al * sizeof(int64_t) : 0);
    if (!per_pose) return PAIRPOT_MAX_CHUNK;
    return (int)std::min<size_t>((size_t)PAIRPOT_MAX_CHUNK, std::max<size_t>(1, budget / per_pose));
}

// Density fit (api_pose.hip: dfm_density_create; kernels_density.hip).  The limits: channels, nodes per axis, the largest grid value,
// weight and voxel edge, poses per launch, and the bytes of per-atom output a chunk of a call may hold.
constexpr int DENSITY_MAX_CHANNELS = 4, DENSITY_MIN_AXIS = 2, DENSITY_MAX_AXIS = 1024, DENSITY_MAX_CHUNK = 32768;
constexpr float DENSITY_MAX_VALUE = 1024.f, DENSITY_MAX_WEIGHT = 128.f, DENSITY_MAX_VOXEL = 16.f;
constexpr size_t DENSITY_CHUNK_BYTES = (size_t)64 << 20;

// the grid [C][nz][ny][nx], its origin and voxel (x, y, z): the message of the first thing that is wrong, or ""
inline std::string check_density_grid(int nx, int ny, int nz, const float *origin, const float *voxel, int C, const float *grids)
{
    if (C < 1 || C > DENSITY_MAX_CHANNELS) return "need 1 <= C <= " + std::to_string(DENSITY_MAX_CHANNELS);
    const int n[3] = {nx, ny, nz};
    for (int k = 0; k < 3; ++k)
        if (n[k] < DENSITY_MIN_AXIS || n[k] > DENSITY_MAX_AXIS)
            return std::string("need 2 <= n") + "xyz"[k] + " <= " + std::to_string(DENSITY_MAX_AXIS);
    if (!origin) return "origin is NULL";
    if (!voxel) return "voxel is NULL";
    if (!grids) return "grids is NULL";
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(origin[k])) return "origin is not finite";
    for (int k = 0; k < 3; ++k)
        if (!(std::isfinite(voxel[k]) && voxel[k] > 0.f && voxel[k] <= DENSITY_MAX_VOXEL)) return "voxel is not in (0, 16]";
    const size_t total = (size_t)C * nz * ny * nx;
    for (size_t i = 0; i < total; ++i)
        if (!(std::isfinite(grids[i]) && std::fabs(grids[i]) <= DENSITY_MAX_VALUE))
            return "grids: value " + std::to_string(i) + " is not in [-1024, 1024]";
    return "";
}

// the ligand's atoms [Al][3], their weights [Al] and the rotation centre
inline std::string check_density_atoms(int Al, const float *lig_atoms, const float *lig_w, const float *center)
{
    if (!lig_atoms) return "lig_atoms is NULL";
    if (!lig_w) return "lig_w is NULL";
    if (!center) return "center is NULL";
    if (Al < 1) return "need Al >= 1";
    if (Al > POSE_MAX_ATOMS) return "Al exceeds 2^24 atoms";
    for (size_t i = 0; i < (size_t)Al * 3; ++i)
        if (!std::isfinite(lig_atoms[i])) return "lig_atoms: atom " + std::to_string(i / 3) + " is not finite";
    for (int i = 0; i < Al; ++i)
        if (!(std::isfinite(lig_w[i]) && std::fabs(lig_w[i]) <= DENSITY_MAX_WEIGHT))
            return "lig_w: weight " + std::to_string(i) + " is not in [-128, 128]";
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(center[k])) return "center is not finite";
    return "";
}

// The integer sums of the density fit can not wrap.  A trilinear value lies between its eight corners up to the rounding of seven
// lerps, so |w val| 2^20 <= 2^7 2^10 2^20 (1 + 2^-48) and |term_q| <= 2^37: a pose's sums are below quanta = Al 2^37 in magnitude.  The
// creator refuses a ligand for which that reaches 2^62.
struct DensityBound {
    double quanta;
    bool ok;
};
inline DensityBound density_sum_bound(int64_t Al)
{
    DensityBound b;
    b.quanta = (double)Al * 137438953472.0;      // 2^37
    b.ok = b.quanta < 4611686018427387904.0;     // 2^62
    return b;
}

// the grid as the kernel gathers it: [nz][ny][nx][4] floats, the C channels of a node side by side and zeros behind them, so that a
// corner is one 16-byte load whatever C is
inline std::vector<float> interleave_density(int nx, int ny, int nz, int C, const float *grids)
{
    const size_t nodes = (size_t)nz * ny * nx;
    std::vector<float> v(nodes * 4, 0.f);
    for (int c = 0; c < C; ++c)
        for (size_t i = 0; i < nodes; ++i) v[i * 4 + c] = grids[(size_t)c * nodes + i];
    return v;
}

// atoms [Al] as the kernel reads them: (x, y, z, w), in the caller's order
inline std::vector<float> gather4_density(int Al, const float *xyz, const float *w)
{
    std::vector<float> v((size_t)Al * 4);
    for (int i = 0; i < Al; ++i) {
        for (int k = 0; k < 3; ++k) v[(size_t)i * 4 + k] = xyz[(size_t)i * 3 + k];
        v[(size_t)i * 4 + 3] = w[i];
    }
    return v;
}

// poses of one chunk of a call: as many as fill `budget` bytes of per-atom output [Al] int64; without it the launch alone bounds it
inline int density_chunk_poses(int Al, bool per_atom, size_t budget = DENSITY_CHUNK_BYTES)
{
    if (!per_atom) return DENSITY_MAX_CHUNK;
    return (int)std::min<size_t>((size_t)DENSITY_MAX_CHUNK, std::max<size_t>(1, budget / ((size_t)Al * sizeof(int64_t))));
}

}  // namespace dfm
