// pose_harness.hip - test-only host shim around the rigid-pose launchers of libdfmdock_amd.so (tests/pose_harness.py builds it): the seven
// dfm::launch_*_pose, launch_sterics (the shared cell walk of dfm_posewalk.h, the one launcher with `exits`), launch_iface,
// launch_pairpot, launch_hbond, launch_surface (with its finish kernel), launch_rescon, launch_rescon_finish, launch_hbond_finish and
// launch_density (a gather from a grid, no cell walk: it shares the pose kernels' pose_transform and T).
//
// Host code only: no kernels here.  The one entry point takes a call record of named host buffers and an op code.  BEFORE anything is
// uploaded it checks everything a kernel would follow as an index - every array long enough for the launch it feeds, cell_start of
// nx ny nz + 1 entries, monotone, from 0 to Ar, lig_index a permutation, residue bits below Rr / Lr, W = ceil(Rr / 32), types below
// T, slab offsets type * T * NB, NB in 1 .. 64 with its `top`, e2 of 128 slots that end in +inf - and answers
// hipErrorInvalidValue without a launch when one fails: no call makes a kernel read outside its blocks.  Then the guard-band protocol of
// harness_common.h runs, with the shipped structs (WalkGrid, StericsConst / StericsAtoms, IfaceConst / IfaceAtoms, PairpotConst /
// PairpotAtoms, ResconConst / ResconAtoms, HbondAtoms, SurfaceAtoms, DensityAtoms) filled from the record.  A per-atom output the
// caller leaves out is passed as nullptr.  The density launch is checked for its array lengths (for max(., 2) nodes per axis,
// max(Al, 1) atoms and max(n, 0) poses), a finite geo with voxel > 0 and geo[10..12] == nx - 1, ny - 1, nz - 1 (the bounds the kernel
// turns into corner indices); n, nx / ny / nz < 2 and Al < 1 go through to the launcher, whose refusals they are.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../dfmdock_amd/csrc/dfm_internal.h"
#include "harness_common.h"

namespace {

using harness::GUARD;

// buffer slots of one call (tests/pose_harness.py SLOTS lists the same names in the same order)
enum Slot {
    S_ROT, S_TR, S_T, S_REC, S_LIG, S_SPHERE, S_CELL_START, S_LIG_INDEX, S_N_CLASH, S_N_CONTACT, S_MIN_BITS, S_LIG_CLASH, S_LIG_CONTACT,
    S_EXITS, S_TOT, S_BITS, S_CLASS_MASK, S_LIG_CLASS, S_REC_DEGREE, S_LIG_DEGREE, S_REC_PAR, S_LIG_PAR, S_LIG_VDW, S_LIG_ELEC, S_LIG_TYPE,
    S_TABLE_Q, S_E2, S_LIG_Q, S_COUNTS, S_REC_ANTE, S_LIG_ANTE, S_REC_INDEX, S_REC_HB, S_REC_SB, S_LIG_HB, S_LIG_SB,
    S_DIRS, S_REC_CLASS, S_REC_EXP, S_LIG_EXP, S_REC_BUR, S_LIG_BURIED, S_REC_BURIED,
    S_GRID, S_GEO, S_ATOM_Q,
    N_SLOTS
};

// OP_STERICS_CHAIN: launch_sterics_pose, then launch_sterics on the T it wrote, as dfm_pose_sterics chains them
enum Op {
    OP_POSE_STERICS, OP_POSE_SURFACE, OP_POSE_IFACE, OP_POSE_RESCON, OP_POSE_HBOND, OP_POSE_PAIRPOT, OP_STERICS, OP_STERICS_CHAIN,
    OP_RESCON, OP_RESCON_FINISH, OP_HBOND_FINISH, OP_IFACE, OP_PAIRPOT, OP_HBOND, OP_SURFACE, OP_POSE_DENSITY, OP_DENSITY
};

}  // namespace

extern "C" {

struct Call {
    harness::HarnessBuf buf[N_SLOTS];
    double lo[3], hi[3], center[3], edge, grow, clash, contact;
    double cut2, soft, min2, kc, lo2;      // IfaceConst; PairpotConst (cut2 is shared)
    double hb2, salt2, c2;                 // HbondConst
    double probe;                          // SurfaceConst (with slack and G)
    float reject2, slack;
    // n poses; Ar / Al atoms; Rr / Lr residues and W words per bitmap row (rescon); Lc rows of Wc words (hbond finish); NT types, NB bins
    // and top (pairpot); Rc / Lc charged residues (hbond: Ar / Al are its polar atoms); C channels (density: nx / ny / nz are its nodes)
    int nx, ny, nz, n, Ar, Al, Rr, Lr, W, Lc, Wc, NT, NB, top, Rc, G, C;
};

HARNESS_EXPORTS(Call)

// the checks alone (what kh_run does first): hipSuccess or hipErrorInvalidValue.  Touches no device.
int ph_check(const Call *c, int op)
{
    const long long n = c->n < 0 ? 0 : c->n, Ar = c->Ar, Al = c->Al;
    auto has = [&](int i, long long bytes) { return c->buf[i].host && c->buf[i].bytes >= bytes; };
    auto out = [&](int i, long long bytes) { return has(i, bytes) && c->buf[i].out != 0; };
    auto opt = [&](int i, long long bytes) { return !c->buf[i].host || out(i, bytes); };
    auto interior = [&](int i) { return (const char *)c->buf[i].host + (c->buf[i].out ? GUARD : 0); };
    bool ok = true;
    for (int i = 0; i < N_SLOTS; ++i) ok = ok && c->buf[i].bytes >= 0 && c->buf[i].out >= 0 && c->buf[i].out <= 2;
    if (!ok) return (int)hipErrorInvalidValue;

    if ((op >= OP_POSE_STERICS && op <= OP_POSE_PAIRPOT) || op == OP_POSE_DENSITY) {
        ok = c->n >= 1 && has(S_ROT, n * 12) && has(S_TR, n * 12) && out(S_T, n * 96);
        if (op == OP_POSE_STERICS) ok = ok && out(S_N_CLASH, n * 4) && out(S_N_CONTACT, n * 4) && out(S_MIN_BITS, n * 8);
        if (op == OP_POSE_SURFACE) ok = ok && out(S_TOT, n * 32 * 4);
        if (op == OP_POSE_IFACE) ok = ok && out(S_TOT, n * 4 * 8);
        if (op == OP_POSE_HBOND) ok = ok && out(S_TOT, n * 5 * 4);
        if (op == OP_POSE_PAIRPOT) ok = ok && out(S_TOT, n * 2 * 8);
        if (op == OP_POSE_DENSITY) ok = ok && out(S_TOT, n * dfm::DENSITY_TOT * 8);
        return ok ? (int)hipSuccess : (int)hipErrorInvalidValue;
    }
    if (op == OP_DENSITY) {
        // n, nx / ny / nz < 2 and Al < 1 are the launcher's to refuse: the arrays are checked for what a launch could touch whatever they are
        auto at_least = [](long long v, long long lo) { return v < lo ? lo : v; };
        ok = c->nx <= 1024 && c->ny <= 1024 && c->nz <= 1024 && Al <= (1 << 24) && c->n <= (1 << 20) && c->C >= 1 && c->C <= 4;
        if (!ok) return (int)hipErrorInvalidValue;
        const long long nodes = at_least(c->nx, 2) * at_least(c->ny, 2) * at_least(c->nz, 2), atoms = at_least(Al, 1);
        ok = has(S_GRID, nodes * 16) && c->buf[S_GRID].out == 0 && has(S_LIG, atoms * 16) && c->buf[S_LIG].out == 0 &&
             has(S_GEO, dfm::DENSITY_GEO_SLOTS * 8) && c->buf[S_GEO].out == 0 && has(S_T, n * 96) && out(S_TOT, n * dfm::DENSITY_TOT * 8) &&
             opt(S_ATOM_Q, n * atoms * 8);
        if (ok) {
            const double *geo = (const double *)c->buf[S_GEO].host;
            for (int k = 0; k < dfm::DENSITY_GEO_SLOTS; ++k) ok = ok && std::isfinite(geo[k]);
            ok = ok && geo[3] > 0.0 && geo[4] > 0.0 && geo[5] > 0.0 && geo[10] == (double)(c->nx - 1) && geo[11] == (double)(c->ny - 1) &&
                 geo[12] == (double)(c->nz - 1);
        }
        return ok ? (int)hipSuccess : (int)hipErrorInvalidValue;
    }
    if (op == OP_RESCON_FINISH) {
        const long long Rr = c->Rr, Lr = c->Lr, W = c->W;
        ok = c->n >= 1 && Rr >= 1 && Rr <= 4096 && Lr >= 1 && Lr <= 4096 && W == (Rr + 31) / 32 && has(S_BITS, n * Lr * W * 4) &&
             has(S_CLASS_MASK, 3 * W * 4) && c->buf[S_CLASS_MASK].out == 0 && has(S_LIG_CLASS, Lr * 4) && c->buf[S_LIG_CLASS].out == 0 &&
             out(S_TOT, n * 9 * 4) && opt(S_REC_DEGREE, n * Rr * 4) && opt(S_LIG_DEGREE, n * Lr * 4);
        if (ok) {
            const int32_t *cl = (const int32_t *)c->buf[S_LIG_CLASS].host;
            for (long long j = 0; j < Lr; ++j) ok = ok && cl[j] >= 0 && cl[j] <= 2;
        }
        return ok ? (int)hipSuccess : (int)hipErrorInvalidValue;
    }
    if (op == OP_HBOND_FINISH) {
        const long long words = (long long)c->Lc * c->Wc;
        ok = c->n >= 1 && c->Lc >= 0 && c->Lc <= 4096 && c->Wc >= 0 && c->Wc <= 128 && has(S_BITS, n * words * 4) && out(S_TOT, n * 5 * 4);
        return ok ? (int)hipSuccess : (int)hipErrorInvalidValue;
    }
    if (op != OP_STERICS && op != OP_STERICS_CHAIN && op != OP_RESCON && op != OP_IFACE && op != OP_PAIRPOT && op != OP_HBOND && op != OP_SURFACE) return (int)hipErrorInvalidValue;

    // the frame of a walk: the grid, the sorted receptor, the ligand in blocks.  n itself is the launcher's to refuse: the arrays are
    // checked for max(n, 0) poses whatever it is
    const long long nblk = (Al + 63) / 64;
    ok = Ar >= 1 && Al >= 1 && Ar <= (1 << 24) && Al <= (1 << 24) && c->nx >= 1 && c->ny >= 1 && c->nz >= 1;
    const double cells_d = (double)c->nx * (double)c->ny * (double)c->nz;
    ok = ok && cells_d <= (double)(1 << 24) && std::isfinite(c->edge) && c->edge > 0.0 && std::isfinite(c->grow) && c->grow >= 0.0;
    for (int k = 0; k < 3; ++k) ok = ok && std::isfinite(c->lo[k]) && std::isfinite(c->hi[k]) && std::isfinite(c->center[k]) && c->lo[k] <= c->hi[k];
    if (!ok) return (int)hipErrorInvalidValue;
    const long long cells = (long long)c->nx * c->ny * c->nz;
    ok = has(S_REC, Ar * 16) && has(S_LIG, Al * 16) && has(S_SPHERE, nblk * 16) && has(S_CELL_START, (cells + 1) * 4) &&
         c->buf[S_REC].out == 0 && c->buf[S_LIG].out == 0 && c->buf[S_SPHERE].out == 0 && c->buf[S_CELL_START].out == 0;
    if (op == OP_STERICS_CHAIN) ok = ok && c->n >= 1 && has(S_ROT, n * 12) && has(S_TR, n * 12) && out(S_T, n * 96);
    else ok = ok && has(S_T, n * 96);
    if (ok) {
        const int32_t *cs = (const int32_t *)c->buf[S_CELL_START].host;
        ok = cs[0] == 0 && cs[cells] == Ar;
        for (long long i = 0; i < cells && ok; ++i) ok = cs[i] <= cs[i + 1];
    }
    if (ok && (op == OP_STERICS || op == OP_STERICS_CHAIN))
        ok = out(S_N_CLASH, n * 4) && out(S_N_CONTACT, n * 4) && out(S_MIN_BITS, n * 8) && opt(S_LIG_CLASH, n * Al * 4) &&
             opt(S_LIG_CONTACT, n * Al * 4) && opt(S_EXITS, 16);
    if (ok && op != OP_RESCON) {
        ok = has(S_LIG_INDEX, Al * 4) && c->buf[S_LIG_INDEX].out == 0;
        if (ok) {
            const int32_t *ix = (const int32_t *)c->buf[S_LIG_INDEX].host;
            std::vector<char> seen((size_t)Al, 0);
            for (long long a = 0; a < Al && ok; ++a) {
                ok = ix[a] >= 0 && ix[a] < Al && !seen[(size_t)ix[a]];
                if (ok) seen[(size_t)ix[a]] = 1;
            }
        }
    }
    if (ok && op == OP_IFACE)
        ok = has(S_REC_PAR, Ar * 16) && c->buf[S_REC_PAR].out == 0 && has(S_LIG_PAR, Al * 16) && c->buf[S_LIG_PAR].out == 0 &&
             out(S_TOT, n * 4 * 8) && opt(S_LIG_VDW, n * Al * 8) && opt(S_LIG_ELEC, n * Al * 8);
    if (ok && op == OP_PAIRPOT) {
        const long long NT = c->NT, NB = c->NB;
        int top = 1;
        while (top * 2 <= NB) top *= 2;
        ok = NT >= 1 && NT <= 256 && NB >= 1 && NB <= 64 && c->top == top && has(S_REC_PAR, Ar * 16) && c->buf[S_REC_PAR].out == 0 &&
             has(S_LIG_TYPE, Al * 4) && c->buf[S_LIG_TYPE].out == 0 && has(S_TABLE_Q, NT * NT * NB * 4) && c->buf[S_TABLE_Q].out == 0 &&
             has(S_E2, dfm::PAIRPOT_E2_SLOTS * 8) && c->buf[S_E2].out == 0 && out(S_TOT, n * 2 * 8) && opt(S_LIG_Q, n * Al * 8) &&
             opt(S_COUNTS, n * NT * NT * NB * 4);
        if (ok) {
            const double *e2 = (const double *)c->buf[S_E2].host;
            ok = e2[0] == c->lo2 && e2[NB] == c->cut2 && e2[0] >= 0.0 && std::isfinite(e2[NB]);
            for (long long k = 0; k < NB; ++k) ok = ok && e2[k] < e2[k + 1];
            for (long long k = NB + 1; k < dfm::PAIRPOT_E2_SLOTS; ++k) ok = ok && std::isinf(e2[k]) && e2[k] > 0.0;
            const int32_t *rp = (const int32_t *)c->buf[S_REC_PAR].host, *lt = (const int32_t *)c->buf[S_LIG_TYPE].host;
            for (long long i = 0; i < Ar; ++i) ok = ok && rp[4 * i] >= 0 && rp[4 * i] < NT && rp[4 * i + 1] == rp[4 * i] * NT * NB;
            for (long long i = 0; i < Al; ++i) ok = ok && lt[i] >= 0 && lt[i] < NT;
        }
    }
    if (ok && op == OP_SURFACE) {
        const long long G = c->G;
        ok = G >= 1 && G <= 4 && has(S_DIRS, G * 64 * 3 * 4) && c->buf[S_DIRS].out == 0 && has(S_REC_INDEX, Ar * 4) && c->buf[S_REC_INDEX].out == 0 &&
             has(S_REC_CLASS, Ar * 4) && c->buf[S_REC_CLASS].out == 0 && has(S_LIG_CLASS, Al * 4) && c->buf[S_LIG_CLASS].out == 0 &&
             has(S_REC_EXP, Ar * G * 8) && c->buf[S_REC_EXP].out == 0 && has(S_LIG_EXP, Al * G * 8) && c->buf[S_LIG_EXP].out == 0 &&
             out(S_REC_BUR, n * Ar * G * 8) && out(S_TOT, n * 32 * 4) && opt(S_LIG_BURIED, n * Al * 4) && opt(S_REC_BURIED, n * Ar * 4) &&
             std::isfinite(c->probe) && std::isfinite(c->slack);
        if (ok) {
            const int32_t *ix = (const int32_t *)c->buf[S_REC_INDEX].host, *rc = (const int32_t *)c->buf[S_REC_CLASS].host;
            const int32_t *lc = (const int32_t *)c->buf[S_LIG_CLASS].host;
            std::vector<char> seen((size_t)Ar, 0);
            for (long long a = 0; a < Ar && ok; ++a) {
                ok = ix[a] >= 0 && ix[a] < Ar && !seen[(size_t)ix[a]] && rc[a] >= 0 && rc[a] < 16;
                if (ok) seen[(size_t)ix[a]] = 1;
            }
            for (long long a = 0; a < Al; ++a) ok = ok && lc[a] >= 0 && lc[a] < 16;
        }
    }
    if (ok && op == OP_HBOND) {
        const long long Rc = c->Rc, Lc = c->Lc, Wc = c->Wc;
        ok = Rc >= 0 && Rc <= 4096 && Lc >= 0 && Lc <= 4096 && Wc == (Rc + 31) / 32 && has(S_REC_ANTE, Ar * 16) && c->buf[S_REC_ANTE].out == 0 &&
             has(S_LIG_ANTE, Al * 16) && c->buf[S_LIG_ANTE].out == 0 && has(S_REC_INDEX, Ar * 4) && c->buf[S_REC_INDEX].out == 0 &&
             out(S_TOT, n * 5 * 4) && out(S_BITS, n * Lc * Wc * 4) && opt(S_REC_HB, n * Ar * 4) && opt(S_REC_SB, n * Ar * 4) &&
             opt(S_LIG_HB, n * Al * 4) && opt(S_LIG_SB, n * Al * 4);
        if (ok) {      // the receptor's permutation; role | compact charged-residue index << 8 rides as the bits of the fourth component
            const int32_t *ix = (const int32_t *)c->buf[S_REC_INDEX].host;
            std::vector<char> seen((size_t)Ar, 0);
            for (long long a = 0; a < Ar && ok; ++a) {
                ok = ix[a] >= 0 && ix[a] < Ar && !seen[(size_t)ix[a]];
                if (ok) seen[(size_t)ix[a]] = 1;
            }
            const uint32_t *r = (const uint32_t *)interior(S_REC), *l = (const uint32_t *)interior(S_LIG);
            const uint32_t charged = dfm::HB_CATION | dfm::HB_ANION;
            for (long long i = 0; i < Ar; ++i) {
                const uint32_t b = r[4 * i + 3];
                ok = ok && !(b & 0xffu & ~dfm::HB_ROLE_MASK) && ((b & charged) ? (long long)(b >> dfm::HB_RES_SHIFT) < Rc : (b >> dfm::HB_RES_SHIFT) == 0);
            }
            for (long long i = 0; i < Al; ++i) {
                const uint32_t b = l[4 * i + 3];
                ok = ok && !(b & 0xffu & ~dfm::HB_ROLE_MASK) && ((b & charged) ? (long long)(b >> dfm::HB_RES_SHIFT) < Lc : (b >> dfm::HB_RES_SHIFT) == 0);
            }
        }
    }
    if (ok && op == OP_RESCON) {
        const long long Rr = c->Rr, Lr = c->Lr, W = c->W;
        ok = Rr >= 1 && Rr <= 4096 && Lr >= 1 && Lr <= 4096 && W == (Rr + 31) / 32 && out(S_BITS, n * Lr * W * 4);
        if (ok) {      // the residue index rides as the bits of the fourth component
            const int32_t *r = (const int32_t *)interior(S_REC), *l = (const int32_t *)interior(S_LIG);
            for (long long i = 0; i < Ar; ++i) ok = ok && r[4 * i + 3] >= 0 && r[4 * i + 3] < Rr;
            for (long long i = 0; i < Al; ++i) ok = ok && l[4 * i + 3] >= 0 && l[4 * i + 3] < Lr;
        }
    }
    return ok ? (int)hipSuccess : (int)hipErrorInvalidValue;
}

int kh_run(const Call *c, int op)
{
    if (ph_check(c, op) != (int)hipSuccess) return (int)hipErrorInvalidValue;

    harness::Blocks<N_SLOTS> blk(c->buf);
    auto D = [&](int i) { return blk.ptr(i); };

    dfm::WalkGrid g = {};
    for (int k = 0; k < 3; ++k) { g.lo[k] = c->lo[k]; g.hi[k] = c->hi[k]; g.center[k] = c->center[k]; }
    g.edge = c->edge; g.grow = c->grow; g.nx = c->nx; g.ny = c->ny; g.nz = c->nz;
    dfm::StericsAtoms sa = {};
    sa.rec = (const float *)D(S_REC); sa.lig = (const float *)D(S_LIG); sa.sphere = (const float *)D(S_SPHERE);
    sa.cell_start = (const int32_t *)D(S_CELL_START); sa.lig_index = (const int32_t *)D(S_LIG_INDEX);
    sa.sc.g = g; sa.sc.clash = c->clash; sa.sc.contact = c->contact; sa.sc.reject2 = c->reject2;
    sa.Ar = c->Ar; sa.Al = c->Al;
    dfm::ResconAtoms ra = {};
    ra.rec = sa.rec; ra.lig = sa.lig; ra.sphere = sa.sphere; ra.cell_start = sa.cell_start;
    ra.lig_class = (const int32_t *)D(S_LIG_CLASS); ra.class_mask = (const uint32_t *)D(S_CLASS_MASK);
    ra.sc.g = g; ra.sc.cutoff = c->contact; ra.sc.reject2 = c->reject2;
    ra.Ar = c->Ar; ra.Al = c->Al; ra.Rr = c->Rr; ra.Lr = c->Lr; ra.W = c->W;
    dfm::HbondAtoms ha = {};
    ha.rec = sa.rec; ha.rec_ante = (const float *)D(S_REC_ANTE); ha.lig = sa.lig; ha.lig_ante = (const float *)D(S_LIG_ANTE);
    ha.sphere = sa.sphere; ha.cell_start = sa.cell_start; ha.rec_index = (const int32_t *)D(S_REC_INDEX); ha.lig_index = sa.lig_index;
    ha.sc.g = g; ha.sc.hb2 = c->hb2; ha.sc.salt2 = c->salt2; ha.sc.c2 = c->c2; ha.sc.reject2 = c->reject2;
    ha.Nr = c->Ar; ha.Nl = c->Al; ha.Rc = c->Rc; ha.Lc = c->Lc; ha.Wc = c->Wc;
    dfm::IfaceAtoms ia = {};
    ia.rec = sa.rec; ia.rec_par = (const float *)D(S_REC_PAR); ia.lig = sa.lig; ia.lig_par = (const float *)D(S_LIG_PAR);
    ia.sphere = sa.sphere; ia.cell_start = sa.cell_start; ia.lig_index = sa.lig_index;
    ia.sc.g = g; ia.sc.cut2 = c->cut2; ia.sc.soft = c->soft; ia.sc.min2 = c->min2; ia.sc.kc = c->kc; ia.sc.reject2 = c->reject2;
    ia.Ar = c->Ar; ia.Al = c->Al;
    dfm::PairpotAtoms pa = {};
    pa.rec = sa.rec; pa.rec_par = (const float *)D(S_REC_PAR); pa.lig = sa.lig; pa.sphere = sa.sphere; pa.cell_start = sa.cell_start;
    pa.lig_index = sa.lig_index; pa.lig_type = (const int32_t *)D(S_LIG_TYPE); pa.table_q = (const int32_t *)D(S_TABLE_Q);
    pa.e2 = (const double *)D(S_E2);
    pa.sc.g = g; pa.sc.lo2 = c->lo2; pa.sc.cut2 = c->cut2; pa.sc.reject2 = c->reject2; pa.sc.T = c->NT; pa.sc.NB = c->NB; pa.sc.top = c->top;
    pa.Ar = c->Ar; pa.Al = c->Al;

    dfm::SurfaceAtoms su = {};
    su.rec = sa.rec; su.lig = sa.lig; su.sphere = sa.sphere; su.dirs = (const float *)D(S_DIRS); su.cell_start = sa.cell_start;
    su.rec_index = (const int32_t *)D(S_REC_INDEX); su.lig_index = sa.lig_index; su.rec_class = (const int32_t *)D(S_REC_CLASS);
    su.lig_class = (const int32_t *)D(S_LIG_CLASS); su.rec_exp = (const uint64_t *)D(S_REC_EXP); su.lig_exp = (const uint64_t *)D(S_LIG_EXP);
    su.sc.g = g; su.sc.probe = c->probe; su.sc.slack = c->slack; su.sc.G = c->G;
    su.Ar = c->Ar; su.Al = c->Al;

    dfm::DensityAtoms da = {};
    da.grid = (const float *)D(S_GRID); da.lig = sa.lig; da.geo = (const double *)D(S_GEO);
    da.nx = c->nx; da.ny = c->ny; da.nz = c->nz; da.C = c->C; da.Al = c->Al;

    const float *rot = (const float *)D(S_ROT), *tr = (const float *)D(S_TR);
    double *T = (double *)D(S_T);
    int32_t *n_clash = (int32_t *)D(S_N_CLASH), *n_contact = (int32_t *)D(S_N_CONTACT);
    uint64_t *min_bits = (uint64_t *)D(S_MIN_BITS);

    hipStream_t s = nullptr;
    hipError_t e = blk.begin(&s);
    if (e == hipSuccess) switch (op) {
        case OP_POSE_STERICS: e = dfm::launch_sterics_pose(rot, tr, c->n, T, n_clash, n_contact, min_bits, s); break;
        case OP_POSE_SURFACE: e = dfm::launch_surface_pose(rot, tr, c->n, T, (int32_t *)D(S_TOT), s); break;
        case OP_POSE_IFACE: e = dfm::launch_iface_pose(rot, tr, c->n, T, (int64_t *)D(S_TOT), s); break;
        case OP_POSE_RESCON: e = dfm::launch_rescon_pose(rot, tr, c->n, T, s); break;
        case OP_POSE_HBOND: e = dfm::launch_hbond_pose(rot, tr, c->n, T, (int32_t *)D(S_TOT), s); break;
        case OP_POSE_PAIRPOT: e = dfm::launch_pairpot_pose(rot, tr, c->n, T, (int64_t *)D(S_TOT), s); break;
        case OP_POSE_DENSITY: e = dfm::launch_density_pose(rot, tr, c->n, T, (int64_t *)D(S_TOT), s); break;
        case OP_DENSITY: e = dfm::launch_density(da, T, c->n, (int64_t *)D(S_TOT), (int64_t *)D(S_ATOM_Q), s); break;
        case OP_STERICS_CHAIN:
            e = dfm::launch_sterics_pose(rot, tr, c->n, T, n_clash, n_contact, min_bits, s);
            if (e != hipSuccess) break;
            [[fallthrough]];
        case OP_STERICS:
            e = dfm::launch_sterics(sa, T, c->n, n_clash, n_contact, min_bits, (int32_t *)D(S_LIG_CLASH), (int32_t *)D(S_LIG_CONTACT),
                                    (uint64_t *)D(S_EXITS), s);
            break;
        case OP_RESCON: e = dfm::launch_rescon(ra, T, c->n, (uint32_t *)D(S_BITS), s); break;
        case OP_RESCON_FINISH:
            e = dfm::launch_rescon_finish(ra, (const uint32_t *)D(S_BITS), c->n, (int32_t *)D(S_TOT), (int32_t *)D(S_REC_DEGREE),
                                          (int32_t *)D(S_LIG_DEGREE), s);
            break;
        case OP_HBOND_FINISH: e = dfm::launch_hbond_finish(ha, (const uint32_t *)D(S_BITS), c->n, (int32_t *)D(S_TOT), s); break;
        case OP_HBOND:
            e = dfm::launch_hbond(ha, T, c->n, (int32_t *)D(S_TOT), (uint32_t *)D(S_BITS), (int32_t *)D(S_REC_HB), (int32_t *)D(S_REC_SB),
                                  (int32_t *)D(S_LIG_HB), (int32_t *)D(S_LIG_SB), s);
            if (e == hipSuccess) e = dfm::launch_hbond_finish(ha, (const uint32_t *)D(S_BITS), c->n, (int32_t *)D(S_TOT), s);
            break;
        case OP_SURFACE:
            e = dfm::launch_surface(su, T, c->n, (uint64_t *)D(S_REC_BUR), (int32_t *)D(S_LIG_BURIED), (int32_t *)D(S_REC_BURIED),
                                    (int32_t *)D(S_TOT), s);
            break;
        case OP_IFACE:
            e = dfm::launch_iface(ia, T, c->n, (int64_t *)D(S_TOT), (int64_t *)D(S_LIG_VDW), (int64_t *)D(S_LIG_ELEC), s);
            break;
        case OP_PAIRPOT:
            e = dfm::launch_pairpot(pa, T, c->n, (int64_t *)D(S_TOT), (int64_t *)D(S_LIG_Q), (int32_t *)D(S_COUNTS), s);
            break;
        default: e = hipErrorInvalidValue;
    }
    return (int)blk.finish(e);      // (a launcher's refusal still returns the blocks: they must be the prefill)
}

}  // extern "C"
