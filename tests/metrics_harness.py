"""Kernel-level harness of the docking-metrics kernels (tests/kernels/metrics_harness.hip): k_native_pairs, k_metrics_reduce,
k_metrics_solve and k_metrics_resid of kernels_metrics.hip, launch by launch.

The shim drives the shipped launchers of dfmdock_amd/libdfmdock_amd.so (dfm::launch_native_pairs, launch_metrics_reduce,
launch_metrics_finish) under the guard-band protocol of tests/kernel_harness.py, after checking that every array is large enough for
the launch it feeds.  This module binds it and holds
  * the float64 references, written from dfmdock_amd/metrics.py (SVD Kabsch with the reflection fix: find_rigid_alignment; the contact
    distance: _min_dist / _min_dist_pairs), not from the kernels, and the exactly rounded sums (math.fsum) the reduction is held to;
  * an extended-precision evaluation of the same definition (np.longdouble sums and residuals, the 3 x 3 SVD in mpmath at 50 digits),
    which tests/test_metrics_harness_cpu.py uses to show that the definition's own float64 error is below a quarter of every gate;
  * the comparisons the GPU tests use (check_pairs, check_sums, check_solve, check_rmsd, check_recovered), which the CPU tests also turn
    on seeded mutants of a numpy restatement of the kernels (restate) to show that they have power;
  * the input generators, so that the CPU tests can check the border-pair caps on the inputs the GPU tests use.

Gates.
  k_native_pairs   flags equal float64 d < cutoff exactly on lattice coordinates (multiples of 0.25 A: every squared distance is exact
                   and sqrt is correctly rounded); on generic coordinates a pair within BORDER = 1e-3 A of a cutoff may go either way.
  k_metrics_reduce each of the 24 sums within (n_atoms + 8) 2^-53 sum |p_i q_j| (S: sum |p_i|) of the exactly rounded sum of the
                   float64 products: n_atoms - 1 additions in any order, the reference's rounding of each product, the final rounding
                   of fsum - and five to spare.  The kernel's fma does not round the product.
  k_metrics_solve  |R R^T - I| <= 1e-13, |det R - 1| <= 1e-13, tr(R M) >= s1 + s2 + sign(det M) s3 - 1e-12 s1 (the optimum of a proper
                   rotation; 500 x the 1.8e-15 a numpy restatement reaches), t = T/n - R S/n to 1e-13 (|T| + |S|) / n.
  RMSDs            1e-9 A + 1e-9 rmsd against the SVD definition on the same fp32 inputs: the project's figure for an fp64 kernel against
                   float64 (tests/test_gpu_sterics.py, min_dist).  l_rmsd only where the receptor's fit is unique (second singular value
                   of its H above 1e-6 x the first).
"""
import ctypes as C
import functools
import math

import numpy as np

import kernel_harness as kh
from kernel_harness import HIP_INVALID_VALUE, HIP_SUCCESS, LIBDIR, ROOT, Out, guards_intact      # noqa: F401 (re-exported)

LAUNCHERS = ("_ZN3dfm19launch_native_pairsEPKfS1_iiddPhP12ihipStream_t",
             "_ZN3dfm21launch_metrics_reduceERKNS_12MetricsChainES2_iiRKNS_12MetricsConstEPdP12ihipStream_t",
             "_ZN3dfm21launch_metrics_finishERKNS_12MetricsChainES2_PKdiS4_RKNS_12MetricsConstEPKiiPdSA_PiP12ihipStream_t")
U64 = 2.0 ** -53                 # unit roundoff of fp64
BORDER = 1e-3                     # A: a contact decision this close to its cutoff may go either way (generic coordinates only)
BORDER_CAP = 0.005                # at most this share of a generator's decisions may be that close
RMSD_ABS, RMSD_REL = 1e-9, 1e-9
ORTHO_TOL, DET_TOL, OPT_TOL, T_TOL = 1e-13, 1e-13, 1e-12, 1e-13
UNIQUE = 1e-6

SLOTS = ("rec_nat", "lig_nat", "rec_model", "lig_model", "frec", "flig", "contacts", "rec_const", "sums", "xf", "rmsd", "recovered", "pairs")
VECS = ("T_rec", "T_lig", "T_rec_iface", "T_lig_iface", "o")
INTS = ("P", "R", "L", "chains", "n_rec", "n_lig", "n_rec_iface", "n_lig_iface", "n_contacts", "rec_moves")
OPS = ("native_pairs", "reduce", "finish", "full")

f32 = np.float32


def f64(x):
    return np.asarray(x, np.float64)


class Call(C.Structure):
    _fields_ = ([("buf", kh.Buf * len(SLOTS)), ("iface_cutoff", C.c_double), ("contact_cutoff", C.c_double)] +
                [(n, C.c_double * 3) for n in VECS] + [(n, C.c_int) for n in INTS])


compile_shim = functools.partial(kh.compile_shim, "metrics")


# ---- cases -------------------------------------------------------------------------------------------------------------------------
class Case:
    """One native and P poses of it.  nat_rec [R,3,3], nat_lig [L,3,3], lig [P,L,3,3] float32; rec [P,R,3,3] float32 or None (the native
    receptor in every pose: chains = 1, rec_moves = 0); frec [R], flig [L] uint8 interface flags; contacts [n,2] int32 (receptor,
    ligand); kinds [P] what each pose is; cutoff: the contact cutoff of `recovered`; lattice: every coordinate a multiple of 0.25 A."""

    def __init__(self, name, nat_rec, nat_lig, lig, rec, frec, flig, contacts, kinds, cutoff=5.5, lattice=False, iface_cutoff=None):
        self.name = name
        self.nat_rec, self.nat_lig = np.ascontiguousarray(nat_rec, f32), np.ascontiguousarray(nat_lig, f32)
        self.lig = np.ascontiguousarray(lig, f32)
        self.rec = None if rec is None else np.ascontiguousarray(rec, f32)
        self.frec, self.flig = np.ascontiguousarray(frec, np.uint8), np.ascontiguousarray(flig, np.uint8)
        self.contacts = np.ascontiguousarray(contacts, np.int32).reshape(-1, 2)
        self.kinds, self.cutoff, self.lattice, self.iface_cutoff = list(kinds), float(cutoff), lattice, iface_cutoff
        self.P, self.R, self.L = self.lig.shape[0], self.nat_rec.shape[0], self.nat_lig.shape[0]
        self.chains = 1 if rec is None else 2
        assert self.nat_rec.shape == (self.R, 3, 3) and self.nat_lig.shape == (self.L, 3, 3) and self.lig.shape == (self.P, self.L, 3, 3)
        assert self.rec is None or self.rec.shape == (self.P, self.R, 3, 3)
        assert self.frec.shape == (self.R,) and self.flig.shape == (self.L,) and len(self.kinds) == self.P
        c = self.contacts
        assert ((c[:, 0] >= 0) & (c[:, 0] < self.R) & (c[:, 1] >= 0) & (c[:, 1] < self.L)).all()

    def rec_of(self, p):
        return self.nat_rec if self.rec is None else self.rec[p]

    def __repr__(self):
        return self.name


def consts(case):
    """What dfm_native_create derives on the host (api_pose.hip): the shift o = the all-atom centroid rounded to fp32, the sums T of the
    native's shifted coordinates per group, the counts."""
    allq = np.concatenate([f64(case.nat_rec).reshape(-1, 3), f64(case.nat_lig).reshape(-1, 3)])
    of = allq.mean(0).astype(f32)
    o = np.where(np.isfinite(of), of, 0).astype(np.float64)
    qr, ql = f64(case.nat_rec) - o, f64(case.nat_lig) - o
    fr, fl = case.frec != 0, case.flig != 0
    return dict(o=o, T_rec=qr.reshape(-1, 3).sum(0), T_lig=ql.reshape(-1, 3).sum(0), T_rec_iface=qr[fr].reshape(-1, 3).sum(0),
                T_lig_iface=ql[fl].reshape(-1, 3).sum(0), n_rec=case.R, n_lig=case.L, n_rec_iface=int(fr.sum()), n_lig_iface=int(fl.sum()))


# ---- binding -----------------------------------------------------------------------------------------------------------------------
class Harness(kh.KernelHarness):
    check = True      # run() asserts success unless told check=False

    def __init__(self, path):
        super().__init__(path, Call, SLOTS, OPS)

    # ---- the four operations on a Case
    def native_pairs(self, rec, lig, iface_cutoff, contact_cutoff):
        R, L = len(rec), len(lig)
        r = self.run("native_pairs", dict(rec_nat=np.ascontiguousarray(rec, f32), lig_nat=np.ascontiguousarray(lig, f32),
                                          pairs=Out(np.uint8, R * L)), R=R, L=L, iface_cutoff=iface_cutoff, contact_cutoff=contact_cutoff)
        return r["pairs"].reshape(R, L)

    def _bufs(self, case):
        rec_model = case.nat_rec if case.rec is None else case.rec
        return dict(rec_nat=case.nat_rec, lig_nat=case.nat_lig, rec_model=rec_model, lig_model=case.lig, frec=case.frec, flig=case.flig,
                    contacts=case.contacts)

    def _scalars(self, case, k):
        return dict(P=case.P, R=case.R, L=case.L, chains=case.chains, rec_moves=case.chains - 1, n_contacts=len(case.contacts),
                    contact_cutoff=case.cutoff, **k)

    def reduce(self, case, k=None):
        """sums [P][chains][24]: chain 0 the ligand, chain 1 the receptor."""
        k = k or consts(case)
        r = self.run("reduce", dict(self._bufs(case), sums=Out(np.float64, case.P * case.chains * 24)), **self._scalars(case, k))
        return r["sums"].reshape(case.P, case.chains, 24)

    def rec_const(self, case, k=None):
        """The receptor's sums with the native receptor as its own model, as dfm_native_create forms them: one chain, one pose."""
        k = k or consts(case)
        r = self.run("reduce", dict(rec_nat=case.nat_rec, lig_nat=case.nat_rec, lig_model=case.nat_rec, frec=case.frec, flig=case.frec,
                                    sums=Out(np.float64, 24)), P=1, R=case.R, L=case.R, chains=1, rec_moves=0, **k)
        return r["sums"]

    def finish(self, case, sums, rec_const=None, k=None):
        """k_metrics_solve and k_metrics_resid on sums the caller supplies: xf [P][3][12], rmsd [P][3], recovered [P]."""
        k = k or consts(case)
        sums = np.ascontiguousarray(sums, np.float64)
        assert sums.shape == (case.P, case.chains, 24) and (case.chains == 2 or np.shape(rec_const) == (24,))
        r = self.run("finish", dict(self._bufs(case), sums=sums, rec_const=None if case.chains == 2 else np.ascontiguousarray(rec_const, np.float64),
                                    xf=Out(np.float64, case.P * 36), rmsd=Out(np.float64, case.P * 3), recovered=Out(np.int32, case.P)),
                     **self._scalars(case, k))
        return dict(xf=r["xf"].reshape(case.P, 3, 12), rmsd=r["rmsd"].reshape(case.P, 3), recovered=r["recovered"])

    def full(self, case, k=None):
        """reduce, then finish, as dfm_pose_metrics chains them."""
        k = k or consts(case)
        rc = None if case.chains == 2 else self.rec_const(case, k)
        r = self.run("full", dict(self._bufs(case), rec_const=rc, sums=Out(np.float64, case.P * case.chains * 24),
                                  xf=Out(np.float64, case.P * 36), rmsd=Out(np.float64, case.P * 3), recovered=Out(np.int32, case.P)),
                     **self._scalars(case, k))
        return dict(sums=r["sums"].reshape(case.P, case.chains, 24), rec_const=rc, xf=r["xf"].reshape(case.P, 3, 12),
                    rmsd=r["rmsd"].reshape(case.P, 3), recovered=r["recovered"])


# ---- generators ----------------------------------------------------------------------------------------------------------------------
FAR = np.array([9000.0, -9000.0, 9000.0])
POSE_KINDS = ("native", "small", "one", "halfturn", "shift500", "noise", "mirror")


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def rotvec_matrix(v):
    th = float(np.linalg.norm(v))
    if th == 0.0:
        return np.eye(3)
    k = f64(v) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def chain_coords(n, rng, start, shape="walk"):
    """A backbone [n,3,3] (N, CA, C) in float64: CA a random walk of 3.8 A steps from `start`, N and C 1.46 / 1.52 A off their CA.
    shape 'planar': every atom in the plane z = start z; 'collinear': every atom on one line."""
    if shape == "collinear":
        d = _unit(rng.standard_normal(3))
        ca = start + 3.8 * np.arange(n)[:, None] * d
        return np.stack([ca - 1.46 * d, ca, ca + 1.52 * d], 1)
    steps, dn, dc = (rng.standard_normal((n, 3)) for _ in range(3))
    if shape == "planar":
        steps[:, 2] = dn[:, 2] = dc[:, 2] = 0.0
    ca = start + np.cumsum(3.8 * _unit(steps), 0)
    return np.stack([ca + 1.46 * _unit(dn), ca, ca + 1.52 * _unit(dc)], 1)


def min_dist64(x1, x2):
    """[n1,n2] minimum backbone-atom distance in float64 of the fp32 coordinates: metrics._min_dist."""
    from dfmdock_amd.metrics import _min_dist
    return _min_dist(f64(np.asarray(x1, f32)), f64(np.asarray(x2, f32)))


def make_contacts(nat_rec, nat_lig, n):
    """n residue pairs: the first names the last residue of both chains, the rest are the closest pairs of the native in ascending
    distance (again from the start when the complex has fewer than n pairs)."""
    R, L = len(nat_rec), len(nat_lig)
    if n == 0:
        return np.zeros((0, 2), np.int32)
    order = np.argsort(min_dist64(nat_rec, nat_lig).reshape(-1), kind="stable")
    idx = order[np.arange(n) % len(order)]
    out = np.stack([idx // L, idx % L], 1).astype(np.int32)
    out[0] = (R - 1, L - 1)
    return out


def make_flags(kind, nat_rec, nat_lig):
    R, L = len(nat_rec), len(nat_lig)
    fr, fl = np.zeros(R, np.uint8), np.zeros(L, np.uint8)
    if kind == "all":
        fr[:], fl[:] = 1, 1
    elif kind == "third":
        fr[::3], fl[1::3] = 1, 1
        fr[0], fl[0] = 1, 1
    elif kind == "last":
        fr[-1], fl[-1] = 1, 1
    elif kind == "single":      # the closest residue pair of the native
        i, j = np.unravel_index(np.argmin(min_dist64(nat_rec, nat_lig)), (R, L))
        fr[i], fl[j] = 1, 1
    else:
        assert kind == "none"
    return fr, fl


def make_poses(nat_rec, nat_lig, kinds, moving, rng):
    """The poses of `kinds` in float32, computed in float64 from the fp32 native: the ligand moved about its centroid; with `moving` the
    whole model (receptor and ligand) then moved by one more rigid motion, or mirrored as a whole."""
    nr, nl = f64(nat_rec), f64(nat_lig)
    cen = nl.reshape(-1, 3).mean(0)
    P = len(kinds)
    lig, rec = np.zeros((P,) + nl.shape, f32), np.zeros((P,) + nr.shape, f32)
    for p, kind in enumerate(kinds):
        Rm, tr, xl, xr = np.eye(3), np.zeros(3), nl, nr
        if kind == "small":
            Rm = rotvec_matrix(1e-4 * _unit(rng.standard_normal(3)))
        elif kind == "one":
            Rm, tr = rotvec_matrix(_unit(rng.standard_normal(3)) * rng.uniform(0.7, 1.3)), 3.0 * rng.standard_normal(3)
        elif kind == "halfturn":
            Rm = np.diag([-1.0, -1.0, 1.0])
        elif kind == "shift500":
            tr = 500.0 * _unit(rng.standard_normal(3))
        if kind == "native":
            lig[p], rec[p] = nat_lig, nat_rec
            continue
        xl = (nl - cen) @ Rm.T + cen + tr
        if kind == "noise":
            xl = nl + 0.5 * rng.standard_normal(nl.shape)
            if moving:
                xr = nr + 0.5 * rng.standard_normal(nr.shape)
        if kind == "mirror":
            m = np.array([-1.0, 1.0, 1.0])
            xl = (nl - cen) * m + cen
            if moving:
                xr = (nr - cen) * m + cen
        elif moving:
            Rw, tw = rotvec_matrix(2.0 * rng.standard_normal(3)), 10.0 * rng.standard_normal(3)
            xl, xr = (xl - cen) @ Rw.T + cen + tw, (xr - cen) @ Rw.T + cen + tw
        lig[p], rec[p] = xl.astype(f32), xr.astype(f32)
    return lig, (rec if moving else None)


def make_case(name, R, L, chains, P, iface, n_contacts, far=False, shape="walk", seed=0, kinds=None, iface_cutoff=None):
    """A generic case.  iface: a make_flags kind, or with iface_cutoff (a float, 'single' or 'default') the flags and the contacts follow
    from the cutoffs as dfm_native_create derives them (the cases of the public call)."""
    rng = np.random.default_rng([seed, R, L, chains, P])
    off = FAR if far else np.zeros(3)
    nat_rec = (chain_coords(R, rng, off, shape)).astype(f32)
    nat_lig = (chain_coords(L, rng, off + 4.0 * _unit(rng.standard_normal(3)))).astype(f32)
    kinds = list(kinds) if kinds else [POSE_KINDS[(p + seed) % len(POSE_KINDS)] for p in range(P)]
    lig, rec = make_poses(nat_rec, nat_lig, kinds, chains == 2, rng)
    if iface_cutoff is None:
        fr, fl = make_flags(iface, nat_rec, nat_lig)
        contacts = make_contacts(nat_rec, nat_lig, n_contacts)
    else:
        md = min_dist64(nat_rec, nat_lig)
        if iface_cutoff == "single":      # between the smallest and the second smallest distance: one residue pair
            s = np.sort(md.reshape(-1))
            iface_cutoff = float(f32(0.5 * (s[0] + s[1]))) if len(s) > 1 else float(f32(s[0] + 1.0))
        near = md < float(f32(iface_cutoff))
        fr, fl = near.any(1).astype(np.uint8), near.any(0).astype(np.uint8)
        contacts = np.stack(np.where(md < 5.5), 1)
    return Case(name, nat_rec, nat_lig, lig, rec, fr, fl, contacts, kinds, iface_cutoff=iface_cutoff)


SHAPES = ((1, 1), (1, 65), (63, 64), (64, 1), (65, 129), (130, 300))


@functools.lru_cache(maxsize=None)
def harness_cases():
    """The cases of the kernel harness: every chain length with the receptor implied and given, P in {1, 3, 4, 5, 67}, every interface
    kind, n_contacts in {0, 1, 63, 64, 65, 200}, natives at the origin and at (9000, -9000, 9000) A, a planar and a collinear receptor."""
    return (
        make_case("1x1 implied", 1, 1, 1, 1, "all", 1, kinds=["one"]),
        make_case("1x1 given", 1, 1, 2, 3, "single", 0, seed=1),
        make_case("1x65 implied", 1, 65, 1, 3, "last", 63, seed=2),
        make_case("1x65 given far", 1, 65, 2, 4, "all", 65, far=True, seed=3),
        make_case("63x64 given", 63, 64, 2, 5, "third", 64, seed=4),
        make_case("63x64 implied", 63, 64, 1, 4, "none", 200, seed=5),
        make_case("64x1 implied far", 64, 1, 1, 5, "single", 1, far=True, seed=6),
        make_case("64x1 given", 64, 1, 2, 1, "last", 65, kinds=["one"]),
        make_case("65x129 implied", 65, 129, 1, 67, "third", 200, seed=0),
        make_case("65x129 given far", 65, 129, 2, 5, "last", 63, far=True, seed=2),
        make_case("130x300 given far", 130, 300, 2, 4, "all", 200, far=True, seed=3),
        make_case("130x300 implied", 130, 300, 1, 5, "single", 64, seed=1),
        make_case("planar receptor given", 40, 30, 2, 4, "third", 65, shape="planar", seed=1),
        make_case("planar receptor implied", 40, 30, 1, 3, "all", 64, shape="planar", seed=2),
        make_case("collinear receptor given", 20, 30, 2, 4, "third", 63, shape="collinear", seed=3),
        make_case("collinear receptor implied", 20, 30, 1, 3, "all", 1, shape="collinear", seed=4),
    )


@functools.lru_cache(maxsize=None)
def api_cases():
    """The cases of the public call (engine.Native.metrics): every chain length, the receptor implied and given, the interface none (cutoff
    0), all (cutoff 10^6), a single residue pair and the reference's 10 A; flags and contacts as the cutoffs give them."""
    cut = (10.0, 0.0, 1e6, "single", 10.0, "single")
    return tuple(make_case(f"api {R}x{L} {'given' if ch == 2 else 'implied'} iface {c}", R, L, ch, 5, None, None, far=(i % 3 == 2), seed=10 + i,
                           iface_cutoff=c) for i, ((R, L), c) in enumerate(zip(SHAPES, cut)) for ch in (1, 2))


def poison_case():
    """63x64, four poses = one workgroup, none of them the native; poisoned(case, how) puts a NaN pose / one +inf coordinate at pose 2."""
    return make_case("63x64 one workgroup", 63, 64, 2, 4, "third", 65, seed=7, kinds=["one", "noise", "small", "shift500"])


def poisoned(case, how):
    lig = case.lig.copy()
    if how == "nan":
        lig[2] = np.nan
    else:      # in an interface residue: all three fits see it
        j = np.where(case.flig != 0)[0]
        lig[2, j[len(j) // 2], 1, 1] = np.inf
    return Case(case.name + " " + how, case.nat_rec, case.nat_lig, lig, case.rec, case.frec, case.flig, case.contacts, case.kinds)


# ---- lattice ---------------------------------------------------------------------------------------------------------------------------
LATTICE_SHAPES = ((1, 1), (15, 17), (16, 16), (1, 257), (65, 63))      # R L = 1, 255, 256, 257, 65 * 63
LATTICE_CUTOFFS = (13.0, 5.0)      # interface, contact


def _residue(a, sign):
    """Three lattice atoms: `a` and two more, 1 and 2 A further along sign * z."""
    return np.stack([a, a + [0, 0, sign * 1.0], a + [0, 0, sign * 2.0]])


def lattice_native(R, L, seed=0):
    """nat_rec, nat_lig float32 with every coordinate a multiple of 0.25 A in a 24 A box, and planted pairs [(i, j, want)]: residue
    pairs whose nearest atoms are 3-4-5 (5-12-13) apart - EXACTLY on the contact (interface) cutoff, not a contact - and pairs one fp32
    ulp inside.  want = the pair's flags (bit 0: interface, bit 1: contact).  The last pair of both chains is always planted."""
    rng = np.random.default_rng([77, R, L, seed])
    nr = rng.integers(0, 97, (R, 3, 3)).astype(np.float64) * 0.25
    nl = rng.integers(0, 97, (L, 3, 3)).astype(np.float64) * 0.25
    nr, nl = nr.astype(f32), nl.astype(f32)
    plants = [((3.0, 4.0, 0.0), False, 1), ((3.0, 4.0, 0.0), True, 3), ((5.0, 12.0, 0.0), False, 0), ((5.0, 12.0, 0.0), True, 1)]
    pairs = [(R - 1, L - 1)] + [((5 * i) % R, (7 * i + 3) % L) for i in range(1, 4)]
    planted, anchor, used_l = [], {}, set()
    for (i, j), (d, inside, want) in zip(pairs, plants):
        if j in used_l:
            continue
        used_l.add(j)
        if i not in anchor:      # a receptor residue planted twice keeps its place
            anchor[i] = rng.integers(8, 41, 3).astype(np.float64) * 0.25 + [4.0, 0.0, 4.0]
            nr[i] = _residue(anchor[i], -1.0).astype(f32)
        b = (anchor[i] + d).astype(f32)
        if inside:
            b[0] = np.nextafter(b[0], f32(0))      # one fp32 ulp nearer in x
        nl[j] = np.stack([b, b + f32([0, 0, 1]), b + f32([0, 0, 2])]).astype(f32)
        planted.append((i, j, want))
    return nr, nl, planted


@functools.lru_cache(maxsize=None)
def lattice_cases():
    """One case per lattice shape: three poses (the native, the ligand moved by (0.25, 0, 0) and by (-0.5, 0.25, 0) A: still lattice
    points, except the planted atoms an ulp off them); interface flags and contacts as the cutoffs 13.0 / 5.0 give them, with the
    planted pairs added to the contact list (those exactly on the cutoff are listed and must NOT be found in the native pose)."""
    out = []
    for R, L in LATTICE_SHAPES:
        nr, nl, planted = lattice_native(R, L)
        md = min_dist64(nr, nl)
        near = md < LATTICE_CUTOFFS[0]
        act = np.stack(np.where(md < LATTICE_CUTOFFS[1]), 1)
        contacts = np.concatenate([act, np.array([(i, j) for i, j, _ in planted], np.int64).reshape(-1, 2)])
        lig = np.stack([nl, nl + f32([0.25, 0, 0]), nl + f32([-0.5, 0.25, 0])]).astype(f32)
        c = Case(f"lattice {R}x{L}", nr, nl, lig, None, near.any(1), near.any(0), contacts, ["native", "lattice", "lattice"],
                 cutoff=LATTICE_CUTOFFS[1], lattice=True, iface_cutoff=LATTICE_CUTOFFS[0])
        c.planted, c.native_contacts = planted, act.astype(np.int32)
        out.append(c)
    return tuple(out)


def generic_pair_cases():
    """(nat_rec, nat_lig) of the generic k_native_pairs comparison: the border rule applies."""
    return tuple((c.nat_rec, c.nat_lig) for c in harness_cases() if c.R * c.L > 1 and c.chains == 2)


# ---- k_native_pairs ----------------------------------------------------------------------------------------------------------------------
def pairs_ref(rec, lig, iface_cutoff, contact_cutoff, mutant=None):
    """The flags and the distances.  mutant 'le': <= at both cutoffs."""
    d = min_dist64(rec, lig)
    lt = (lambda a, b: a <= b) if mutant == "le" else (lambda a, b: a < b)
    return (lt(d, iface_cutoff).astype(np.uint8) | (lt(d, contact_cutoff).astype(np.uint8) << 1)), d


def check_pairs(flags, rec, lig, iface_cutoff, contact_cutoff, exact):
    """exact: every flag equals the float64 decision.  Otherwise a decision within BORDER of its cutoff may go either way; returns
    (decisions, borderline ones)."""
    want, d = pairs_ref(rec, lig, iface_cutoff, contact_cutoff)
    flags = np.asarray(flags, np.uint8).reshape(want.shape)
    assert (flags <= 3).all(), "a flag byte holds more than the two bits"
    if exact:
        np.testing.assert_array_equal(flags, want)
        return 2 * d.size, 0
    n_border = 0
    for bit, cut in ((0, iface_cutoff), (1, contact_cutoff)):
        border = np.abs(d - cut) < BORDER
        n_border += int(border.sum())
        np.testing.assert_array_equal(((flags >> bit) & 1)[~border], ((want >> bit) & 1)[~border])
    return 2 * d.size, n_border


# ---- k_metrics_reduce ----------------------------------------------------------------------------------------------------------------------
def _chains_of(case):
    """(model [P,n,3,3], native [n,3,3], flags) per chain in the order of the sums: the ligand, then the receptor."""
    out = [(case.lig, case.nat_lig, case.flig)]
    if case.chains == 2:
        out.append((case.rec, case.nat_rec, case.frec))
    return out


def sums_exact(model, native, flags, o):
    """model [P,n,3,3], native [n,3,3] float32 -> the exactly rounded sums [P,24] of the float64 shifted coordinates and of their float64
    products (math.fsum), and the bounds [P,24] = (n_atoms + 8) 2^-53 sum |term|."""
    P = model.shape[0]
    q = (f64(native) - o).reshape(-1, 3)
    w = np.repeat(np.asarray(flags) != 0, 3)
    ref, bound = np.zeros((P, 24)), np.zeros((P, 24))
    for p in range(P):
        if not np.isfinite(model[p]).all():      # no reference: the pose is not compared
            ref[p] = bound[p] = np.nan
            continue
        x = (f64(model[p]) - o).reshape(-1, 3)
        for g, sel in ((0, slice(None)), (12, w)):
            xs, qs = x[sel], q[sel]
            n = len(xs)
            for i in range(3):
                ref[p, g + i] = math.fsum(xs[:, i])
                bound[p, g + i] = (n + 8) * U64 * math.fsum(np.abs(xs[:, i]))
                for j in range(3):
                    t = xs[:, i] * qs[:, j]
                    ref[p, g + 3 + 3 * i + j] = math.fsum(t)
                    bound[p, g + 3 + 3 * i + j] = (n + 8) * U64 * math.fsum(np.abs(t))
    return ref, bound


@functools.lru_cache(maxsize=None)
def _sums_ref_cached(case):
    o = consts(case)["o"]
    refs = [sums_exact(m, n, f, o) for m, n, f in _chains_of(case)]
    return np.stack([r[0] for r in refs], 1), np.stack([r[1] for r in refs], 1)


def ratio_of(err, bound):
    """max err / bound with 0 / 0 = 0 and anything that is not a number = inf."""
    err, bound = np.broadcast_arrays(f64(err), f64(bound))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where((err == 0) & (bound == 0), 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def check_sums(sums, case, select=None):
    """sums [P][chains][24] against the exactly rounded ones; select: the poses compared (default: the finite ones).  Returns the
    largest error / bound."""
    ref, bound = _sums_ref_cached(case)
    sums = f64(sums).reshape(ref.shape)
    ok = np.isfinite(ref).all((1, 2)) if select is None else select
    worst = ratio_of(np.abs(sums - ref)[ok], bound[ok])
    assert worst <= 1.0, f"{case}: a sum is {worst:.3g} x its bound off the exactly rounded sum"
    return worst


# ---- k_metrics_solve ----------------------------------------------------------------------------------------------------------------------
def fit_inputs(sums, chains, rec_const, k):
    """Per fit (all | interface | receptor): n (residues), S [P,3], T [3], C [P,3,3] as k_metrics_solve combines the sums (float64)."""
    sums = f64(sums)
    sl = sums[:, 0]
    sr = sums[:, 1] if chains == 2 else np.broadcast_to(f64(rec_const), sl.shape)
    out = []
    for fit in range(3):
        g = 12 if fit == 1 else 0
        if fit == 2:
            n, S, C, T = k["n_rec"], sr[:, 0:3], sr[:, 3:12], f64(k["T_rec"])
        elif fit == 1:
            n, T = k["n_rec_iface"] + k["n_lig_iface"], f64(k["T_rec_iface"]) + f64(k["T_lig_iface"])
            S, C = sr[:, g:g + 3] + sl[:, g:g + 3], sr[:, g + 3:g + 12] + sl[:, g + 3:g + 12]
        else:
            n, T = k["n_rec"] + k["n_lig"], f64(k["T_rec"]) + f64(k["T_lig"])
            S, C = sr[:, 0:3] + sl[:, 0:3], sr[:, 3:12] + sl[:, 3:12]
        out.append((n, S, T, C.reshape(-1, 3, 3)))
    return out


def check_solve(xf, sums, chains, rec_const, k, label=""):
    """xf [P][3][12] against what defines it.  Returns {orthogonality, determinant, optimality, translation: largest error / gate}."""
    xf = f64(xf)
    P = xf.shape[0]
    worst = dict(orthogonality=0.0, determinant=0.0, optimality=0.0, translation=0.0)
    for fit, (n, S, T, Cm) in enumerate(fit_inputs(sums, chains, rec_const, k)):
        got = xf[:, fit]
        if n == 0:
            assert np.isnan(got).all(), f"{label} fit {fit}: no residue, and an entry is a number"
            continue
        inv = 1.0 / (3.0 * n)
        with np.errstate(invalid="ignore", over="ignore"):
            M = Cm - S[:, :, None] * (T * inv)[None, None, :]
        fin = np.isfinite(M).all((1, 2))
        assert np.isnan(got[~fin]).all(), f"{label} fit {fit}: M is not finite, and an entry of the fit is a number (poses {np.where(~fin)[0][:4]})"
        assert np.isfinite(got[fin]).all(), f"{label} fit {fit}: M is finite, and an entry of the fit is not (poses {np.where(fin)[0][~np.isfinite(got[fin]).all(1)][:4]})"
        if not fin.any():
            continue
        R, t, M, S = got[fin, :9].reshape(-1, 3, 3), got[fin, 9:], M[fin], S[fin]
        worst["orthogonality"] = max(worst["orthogonality"], float(np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max()) / ORTHO_TOL)
        worst["determinant"] = max(worst["determinant"], float(np.abs(np.linalg.det(R) - 1.0).max()) / DET_TOL)
        s = np.linalg.svd(M, compute_uv=False)
        opt = s[:, 0] + s[:, 1] + np.sign(np.linalg.det(M)) * s[:, 2]
        gap = opt - np.einsum("pba,pab->p", R, M)
        worst["optimality"] = max(worst["optimality"], ratio_of(np.maximum(gap, 0.0), OPT_TOL * s[:, 0]))
        t_ref = T * inv - np.einsum("pij,pj->pi", R, S) * inv
        tol = T_TOL * (np.linalg.norm(T) + np.linalg.norm(S, axis=1)) * inv
        worst["translation"] = max(worst["translation"], ratio_of(np.abs(t - t_ref).max(1), tol))
    for name, w in worst.items():
        assert w <= 1.0, f"{label}: {name} {w:.3g} x its gate"
    return worst


SOLVE_KINDS = ("generic", "rank2", "rank1", "zero", "rotation", "halfturn_x", "halfturn_y", "halfturn_z", "halfturn_axis", "reflection",
               "tie_plus", "tie_minus", "small", "big", "generic_shifted", "nan")


def _random_rotation(rng):
    return rotvec_matrix(_unit(rng.standard_normal(3)) * rng.uniform(0.0, np.pi))


def solve_matrix(kind, rng):
    """One crafted M (and whether the lane carries sums S)."""
    ints = lambda: rng.integers(-9, 10, 3).astype(np.float64)
    scale = float(rng.integers(1, 4096))
    if kind in ("generic", "generic_shifted", "nan"):
        return 1000.0 * rng.standard_normal((3, 3))
    if kind == "rank2":
        return np.outer(ints(), ints()) + np.outer(ints(), ints())
    if kind == "rank1":
        return np.outer(ints(), ints())
    if kind == "zero":
        return np.zeros((3, 3))
    if kind == "rotation":
        return scale * _random_rotation(rng)
    if kind.startswith("halfturn_") and kind != "halfturn_axis":
        d = -np.ones(3)
        d["xyz".index(kind[-1])] = 1.0
        return scale * np.diag(d)
    n = _unit(rng.standard_normal(3))
    if kind == "halfturn_axis":
        return scale * (2.0 * np.outer(n, n) - np.eye(3))
    if kind == "reflection":
        return scale * (np.diag([1.0, 1.0, -1.0]) if rng.integers(2) else np.eye(3) - 2.0 * np.outer(n, n))
    if kind in ("tie_plus", "tie_minus"):
        return scale * _random_rotation(rng) @ np.diag([1.0, 1.0, 1.0 if kind == "tie_plus" else -1.0]) @ _random_rotation(rng).T
    return 1000.0 * rng.standard_normal((3, 3)) * (1e-12 if kind == "small" else 1e12)


SOLVE_CONSTS = dict(o=np.zeros(3), T_rec=np.array([120.5, -60.25, 30.0]), T_lig=np.array([-100.0, 40.5, 10.0]),
                    T_rec_iface=np.array([12.0, 7.5, -3.25]), T_lig_iface=np.array([-8.0, 2.0, 5.5]), n_rec=50, n_lig=70, n_rec_iface=7,
                    n_lig_iface=9)


@functools.lru_cache(maxsize=None)
def solve_inputs(P=4096, seed=5):
    """Crafted sums [P][2][24] for one launch of k_metrics_solve, lane p of kind SOLVE_KINDS[p % 16] in all three fits.  The receptor
    fit reads the receptor's all-atom block, the interface fit the ligand's interface block (the receptor's is zero): their M is the
    crafted matrix to the bit where the lane carries no S.  The all-atom fit reads the sum of both all-atom blocks: a crafted matrix
    up to one rounding.  'nan' lanes hold one NaN in one of the three blocks, at a different entry from lane to lane."""
    rng = np.random.default_rng(seed)
    k = SOLVE_CONSTS
    sums = np.zeros((P, 2, 24))
    kinds = [SOLVE_KINDS[p % len(SOLVE_KINDS)] for p in range(P)]
    for p, kind in enumerate(kinds):
        shifted = kind in ("generic_shifted", "nan")
        M = [solve_matrix(kind, rng) for _ in range(3)]
        S = [50.0 * rng.standard_normal(3) * shifted for _ in range(3)]
        T = (k["T_rec"] + k["T_lig"], k["T_rec_iface"] + k["T_lig_iface"], k["T_rec"])
        n = (k["n_rec"] + k["n_lig"], k["n_rec_iface"] + k["n_lig_iface"], k["n_rec"])
        Cm = [M[f] + np.outer(S[f], T[f]) / (3.0 * n[f]) for f in range(3)]
        sums[p, 1, 0:3], sums[p, 1, 3:12] = S[2], Cm[2].reshape(-1)
        sums[p, 0, 0:3], sums[p, 0, 3:12] = S[0] - S[2], (Cm[0] - Cm[2]).reshape(-1)
        sums[p, 0, 12:15], sums[p, 0, 15:24] = S[1], Cm[1].reshape(-1)
        if kind == "nan":
            lane = p // len(SOLVE_KINDS)
            block = ((0, 3), (0, 15), (1, 3))[lane % 3]
            sums[p, block[0], block[1] + (lane // 3) % 9] = np.nan
    return sums, kinds


def solve_dummy_case(P):
    """The chains k_metrics_resid walks behind a crafted k_metrics_solve launch: one residue each, no contact."""
    z = np.zeros((1, 3, 3), f32)
    return Case("crafted sums", z, z, np.zeros((P, 1, 3, 3), f32), np.zeros((P, 1, 3, 3), f32), [1], [1], np.zeros((0, 2), np.int32), ["native"] * P)


# ---- the definition: RMSDs and recovered contacts ----------------------------------------------------------------------------------------
def _fit_sets(case, p):
    """The three (fitted model points, their native points, measured model points, their native points) of pose p in float64."""
    mr, ml = f64(case.rec_of(p)), f64(case.lig[p])
    nr, nl = f64(case.nat_rec), f64(case.nat_lig)
    fr, fl = case.frec != 0, case.flig != 0
    flat = lambda x: x.reshape(-1, 3)
    A, B = np.concatenate([flat(mr), flat(ml)]), np.concatenate([flat(nr), flat(nl)])
    Ai, Bi = np.concatenate([flat(mr[fr]), flat(ml[fl])]), np.concatenate([flat(nr[fr]), flat(nl[fl])])
    return (A, B, A, B), (Ai, Bi, Ai, Bi), (flat(mr), flat(nr), flat(ml), flat(nl))


@functools.lru_cache(maxsize=None)
def definition(case):
    """metrics.compute_metrics' three RMSDs with the case's own interface flags: rmsd [P,3] float64 (NaN: no interface residue, or a
    pose that is not finite) and unique [P]: the receptor's fit is unique (second singular value of its H above 1e-6 x the first)."""
    from dfmdock_amd.metrics import _rmsd, find_rigid_alignment
    out, unique = np.full((case.P, 3), np.nan), np.zeros(case.P, bool)
    for p in range(case.P):
        if not (np.isfinite(case.lig[p]).all() and np.isfinite(case.rec_of(p)).all()):
            continue
        for fit, (A, B, X, Y) in enumerate(_fit_sets(case, p)):
            if len(A) == 0:
                continue
            Rm, t = find_rigid_alignment(A, B)
            out[p, fit] = _rmsd(X @ Rm.T + t, Y)
            if fit == 2:
                s = np.linalg.svd((A - A.mean(0)).T @ (B - B.mean(0)), compute_uv=False)
                unique[p] = s[1] > UNIQUE * s[0]
    return out, unique


def _to_mp(x):
    import mpmath as mp
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi)))


def _from_mp(m):
    hi = float(m)
    return np.longdouble(hi) + np.longdouble(float(m - hi))


@functools.lru_cache(maxsize=None)
def definition_extended(case):
    """The same definition in extended precision: means, H and residuals in np.longdouble (64-bit significand), the SVD of H and the
    rotation in mpmath at 50 digits.  rmsd [P,3] as float64 (rounded once at the end)."""
    import mpmath as mp
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 here"
    ld = np.longdouble
    out = np.full((case.P, 3), np.nan)
    with mp.workdps(50):
        for p in range(case.P):
            if not (np.isfinite(case.lig[p]).all() and np.isfinite(case.rec_of(p)).all()):
                continue
            for fit, (A, B, X, Y) in enumerate(_fit_sets(case, p)):
                if len(A) == 0:
                    continue
                A, B, X, Y = (v.astype(ld) for v in (A, B, X, Y))
                am, bm = A.sum(0) / ld(len(A)), B.sum(0) / ld(len(B))
                H = (A - am).T @ (B - bm)
                U, _, Vt = mp.svd_r(mp.matrix([[_to_mp(H[i, j]) for j in range(3)] for i in range(3)]))
                Rm = Vt.T * U.T
                if mp.det(Rm) < 0:
                    Rm = Vt.T * mp.diag([1, 1, -1]) * U.T
                Rl = np.array([[_from_mp(Rm[i, j]) for j in range(3)] for i in range(3)], ld)
                d = (X - am) @ Rl.T + bm - Y
                out[p, fit] = float(np.sqrt((d * d).sum() / ld(len(X))))
    return out


def rmsd_gate(ref):
    return RMSD_ABS + RMSD_REL * np.abs(ref)


def check_rmsd(rmsd, case, ref=None):
    """rmsd [P][3] against the definition: c_rmsd and i_rmsd of every finite pose (i_rmsd NaN exactly where no residue is flagged), l_rmsd
    where the receptor's fit is unique; an exactly native pose has all three below 1e-9.  Returns the largest error / gate."""
    ref, unique = ref or definition(case)
    rmsd = f64(rmsd).reshape(case.P, 3)
    fin = np.isfinite(ref[:, 0])
    assert not np.isfinite(rmsd[~fin]).any(), f"{case}: a pose that is not finite has a finite RMSD"
    no_iface = not (case.frec.any() or case.flig.any())
    assert np.isnan(rmsd[:, 1]).all() if no_iface else np.isfinite(rmsd[fin, 1]).all(), f"{case}: i_rmsd is NaN exactly without an interface"
    assert np.isfinite(rmsd[fin][:, [0, 2]]).all(), f"{case}: c_rmsd and l_rmsd are finite for a finite pose"
    worst = 0.0
    for col in range(3):
        if col == 1 and no_iface:
            continue
        sel = fin & unique if col == 2 else fin
        worst = max(worst, ratio_of(np.abs(rmsd[sel, col] - ref[sel, col]), rmsd_gate(ref[sel, col])))
    for p, kind in enumerate(case.kinds):
        if kind == "native" and fin[p]:
            assert np.nanmax(rmsd[p]) <= 1e-9, f"{case} pose {p}: the native itself has an RMSD of {np.nanmax(rmsd[p]):.3g}"
    assert worst <= 1.0, f"{case}: an RMSD is {worst:.3g} x its gate off the definition"
    return worst


def recovered_ref(case, mutant=None):
    """(sure [P], border [P], evaluations): contacts surely found and the ones within BORDER of the cutoff (none on a lattice case: the
    decision is exact there).  mutant 'le': <=."""
    from dfmdock_amd.metrics import _min_dist_pairs
    sure, border = np.zeros(case.P, np.int64), np.zeros(case.P, np.int64)
    for p in range(case.P):
        with np.errstate(invalid="ignore"):
            d = _min_dist_pairs(f64(case.rec_of(p)), f64(case.lig[p]), case.contacts[:, 0], case.contacts[:, 1])
            hit = d <= case.cutoff if mutant == "le" else d < case.cutoff
            if case.lattice:
                sure[p] = int(hit.sum())
            else:
                near = np.abs(d - case.cutoff) < BORDER
                sure[p], border[p] = int((hit & ~near).sum()), int(near.sum())
    return sure, border, case.P * len(case.contacts)


def check_recovered(recovered, case):
    """Exact on a lattice case; elsewhere sure <= recovered <= sure + border.  Returns (evaluations, borderline ones)."""
    sure, border, n_eval = recovered_ref(case)
    got = np.asarray(recovered, np.int64).reshape(case.P)
    assert ((sure <= got) & (got <= sure + border)).all(), f"{case}: recovered {got.tolist()}, definition {sure.tolist()} (+ borderline {border.tolist()})"
    return n_eval, int(border.sum())


def check_full(out, case):
    """Every comparison of one reduce + finish run.  Returns {name: largest error / gate} and the contact evaluation counts."""
    k = consts(case)
    ratios = {"sums": check_sums(out["sums"], case)}
    ratios.update(check_solve(out["xf"], out["sums"], case.chains, out.get("rec_const"), k, str(case)))
    ratios["rmsd"] = check_rmsd(out["rmsd"], case)
    return ratios, check_recovered(out["recovered"], case)


# ---- a numpy restatement of the kernels, and its mutants ---------------------------------------------------------------------------------
MUTANTS = ("f32_accumulator", "two_sweeps", "no_reflection_fix", "mean_over_n", "shift_dropped", "lane_tail_lost", "lig_flags_ignored",
           "all_atom_fit_for_l", "le_at_cutoff", "rec_moves_ignored")


def restate_reduce(model, native, flags, o, mutant=None):
    """k_metrics_reduce of one chain: sums [P,24] in float64 (numpy's own summation order)."""
    model, native, flags = np.asarray(model), np.asarray(native), np.asarray(flags) != 0
    n = native.shape[0]
    if mutant == "lane_tail_lost" and n % 64:
        n -= n % 64
    if mutant == "shift_dropped":
        o = np.zeros(3)
    P = model.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        p = (f64(model[:, :n]) - o).reshape(P, -1, 3)
        q = (f64(native[:n]) - o).reshape(-1, 3)
        w = np.repeat(flags[:n], 3)
        out = np.zeros((P, 24))
        for g, sel in ((0, slice(None)), (12, w)):
            ps, qs = p[:, sel], q[sel]
            out[:, g:g + 3] = ps.sum(1)
            prod = ps[:, :, :, None] * qs[None, :, None, :]
            if mutant == "f32_accumulator" and g == 0:
                Cm = np.cumsum(prod.astype(f32), axis=1, dtype=f32)[:, -1].astype(np.float64) if prod.shape[1] else np.zeros((P, 3, 3))
            else:
                Cm = prod.sum(1)
            out[:, g + 3:g + 12] = Cm.reshape(P, 9)
    return out


def _jacobi(a, v, p, q):
    apq = a[:, p, q].copy()
    act = np.abs(apq) > 0
    z = np.where(act, apq, 1.0)
    theta = (a[:, q, q] - a[:, p, p]) / (2.0 * z)
    t = np.where(theta < 0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    t, c, s, z = np.where(act, t, 0.0), np.where(act, c, 1.0), np.where(act, s, 0.0), np.where(act, apq, 0.0)
    a[:, p, p] -= t * z
    a[:, q, q] += t * z
    a[:, p, q] = a[:, q, p] = np.where(act, 0.0, apq)
    for k in range(4):
        if k != p and k != q:
            akp, akq = a[:, k, p].copy(), a[:, k, q].copy()
            a[:, k, p] = a[:, p, k] = c * akp - s * akq
            a[:, k, q] = a[:, q, k] = s * akp + c * akq
        vkp, vkq = v[:, k, p].copy(), v[:, k, q].copy()
        v[:, k, p] = c * vkp - s * vkq
        v[:, k, q] = s * vkp + c * vkq


def horn_rotation(M, sweeps=12):
    """M [P,3,3] -> the proper rotations [P,3,3] maximising tr(R M): the dominant eigenvector of Horn's quaternion matrix by cyclic
    Jacobi, the first one on ties (kernels_metrics.hip: horn_rotation)."""
    P = M.shape[0]
    a, v = np.zeros((P, 4, 4)), np.tile(np.eye(4), (P, 1, 1))
    a[:, 0, 0] = M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]
    a[:, 1, 1] = M[:, 0, 0] - M[:, 1, 1] - M[:, 2, 2]
    a[:, 2, 2] = -M[:, 0, 0] + M[:, 1, 1] - M[:, 2, 2]
    a[:, 3, 3] = -M[:, 0, 0] - M[:, 1, 1] + M[:, 2, 2]
    a[:, 0, 1] = a[:, 1, 0] = M[:, 1, 2] - M[:, 2, 1]
    a[:, 0, 2] = a[:, 2, 0] = M[:, 2, 0] - M[:, 0, 2]
    a[:, 0, 3] = a[:, 3, 0] = M[:, 0, 1] - M[:, 1, 0]
    a[:, 1, 2] = a[:, 2, 1] = M[:, 0, 1] + M[:, 1, 0]
    a[:, 1, 3] = a[:, 3, 1] = M[:, 2, 0] + M[:, 0, 2]
    a[:, 2, 3] = a[:, 3, 2] = M[:, 1, 2] + M[:, 2, 1]
    for _ in range(sweeps):
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            _jacobi(a, v, p, q)
    best, quat = a[:, 0, 0].copy(), v[:, :, 0].copy()
    for k in range(1, 4):
        take = a[:, k, k] > best
        best = np.where(take, a[:, k, k], best)
        quat = np.where(take[:, None], v[:, :, k], quat)
    quat = quat / np.sqrt((quat * quat).sum(1))[:, None]
    w, x, y, z = quat.T
    return np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], 1).reshape(P, 3, 3)


def restate_solve(sums, chains, rec_const, k, mutant=None):
    """k_metrics_solve: xf [P,3,12].  A fit whose M is not finite is NaN throughout."""
    P = np.shape(sums)[0]
    xf = np.full((P, 3, 12), np.nan)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for fit, (n, S, T, Cm) in enumerate(fit_inputs(sums, chains, rec_const, k)):
            if n == 0:
                continue
            inv = 1.0 / ((1.0 if mutant == "mean_over_n" else 3.0) * n)
            M = Cm - S[:, :, None] * (T * inv)[None, None, :]
            fin = np.isfinite(M).all((1, 2))
            Rm = horn_rotation(np.where(fin[:, None, None], M, 0.0), 2 if mutant == "two_sweeps" else 12)
            if mutant == "no_reflection_fix":      # Kabsch without its determinant test
                U, _, Vt = np.linalg.svd(np.where(fin[:, None, None], M, 0.0))
                Rm = Vt.transpose(0, 2, 1) @ U.transpose(0, 2, 1)
            Rm = np.where(fin[:, None, None], Rm, np.nan)
            xf[:, fit, :9] = Rm.reshape(P, 9)
            xf[:, fit, 9:] = T * inv - np.einsum("pij,pj->pi", Rm, S * inv)
    return xf


def restate_resid(case, xf, k, mutant=None):
    """k_metrics_resid: rmsd [P,3] and recovered [P]."""
    o = np.zeros(3) if mutant == "shift_dropped" else k["o"]
    P = case.P
    e = np.zeros((P, 3))
    rec_model = case.rec if (case.rec is not None and mutant != "rec_moves_ignored") else np.broadcast_to(case.nat_rec, (P,) + case.nat_rec.shape)
    flig = np.ones_like(case.flig) if mutant == "lig_flags_ignored" else case.flig
    with np.errstate(invalid="ignore", over="ignore"):
        for chain, (model, native, flags) in enumerate(((case.lig, case.nat_lig, flig), (rec_model, case.nat_rec, case.frec))):
            n = native.shape[0]
            if mutant == "lane_tail_lost" and n % 64:
                n -= n % 64
            p = (f64(model[:, :n]) - o).reshape(P, -1, 3)
            q = (f64(native[:n]) - o).reshape(-1, 3)
            w = np.repeat(np.asarray(flags[:n]) != 0, 3)
            for col, fit in ((0, 0), (1, 1), (2, 0 if mutant == "all_atom_fit_for_l" else 2)):
                if col == 2 and chain == 1:
                    continue
                Rm, t = xf[:, fit, :9].reshape(P, 3, 3), xf[:, fit, 9:]
                d = np.einsum("pij,paj->pai", Rm, p) + t[:, None, :] - q
                r2 = (d * d).sum(2)
                e[:, col] += (r2[:, w] if col == 1 else r2).sum(1)
        nb = k["n_rec_iface"] + k["n_lig_iface"]
        rmsd = np.stack([np.sqrt(e[:, 0] / (3.0 * (k["n_rec"] + k["n_lig"]))),
                         np.sqrt(e[:, 1] / (3.0 * nb)) if nb else np.full(P, np.nan),
                         np.sqrt(e[:, 2] / (3.0 * k["n_lig"]))], 1)
    from dfmdock_amd.metrics import _min_dist_pairs
    found = np.zeros(P, np.int32)
    for p in range(P):
        with np.errstate(invalid="ignore"):
            d = _min_dist_pairs(f64(rec_model[p]), f64(case.lig[p]), case.contacts[:, 0], case.contacts[:, 1])
            found[p] = int((d <= case.cutoff).sum() if mutant == "le_at_cutoff" else (d < case.cutoff).sum())
    return rmsd, found


def restate(case, mutant=None):
    """reduce + finish of one case in numpy, as Harness.full returns them."""
    k = consts(case)
    flig = np.ones_like(case.flig) if mutant == "lig_flags_ignored" else case.flig
    sums = [restate_reduce(case.lig, case.nat_lig, flig, k["o"], mutant)]
    rc = None
    if case.chains == 2:
        rec = case.rec if mutant != "rec_moves_ignored" else np.broadcast_to(case.nat_rec, case.rec.shape)
        sums.append(restate_reduce(rec, case.nat_rec, case.frec, k["o"], mutant))
    else:
        rc = restate_reduce(case.nat_rec[None], case.nat_rec, case.frec, k["o"], mutant)[0]
    sums = np.stack(sums, 1)
    ks = k
    if mutant == "shift_dropped":      # the host's T without the shift as well: a consistent kernel family in unshifted coordinates
        ks = dict(k, T_rec=f64(case.nat_rec).reshape(-1, 3).sum(0), T_lig=f64(case.nat_lig).reshape(-1, 3).sum(0),
                  T_rec_iface=f64(case.nat_rec)[case.frec != 0].reshape(-1, 3).sum(0), T_lig_iface=f64(case.nat_lig)[case.flig != 0].reshape(-1, 3).sum(0))
    xf = restate_solve(sums, case.chains, rc, ks, mutant)
    rmsd, rec_n = restate_resid(case, xf, ks, mutant)
    return dict(sums=sums, rec_const=rc, xf=xf, rmsd=rmsd, recovered=rec_n)
