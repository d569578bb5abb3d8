"""Kernel-level harness of the rigid-pose kernels (tests/kernels/pose_harness.hip): all sixteen launchers of the six families that share
dfm_posewalk.h - launch_{sterics,surface,iface,rescon,hbond,pairpot}{_pose,}, launch_rescon_finish, launch_hbond_finish and
k_surface_finish inside launch_surface - launch by launch.

The shim drives the shipped launchers of dfmdock_amd/libdfmdock_amd.so under the guard-band protocol of tests/kernel_harness.py, after
checking everything a kernel would follow as an index.  This module binds it and holds
  * a frame built in numpy from the comments of dfm_poseprep.h, not by calling it (cell grid, sorted receptor, Morton-ordered ligand
    blocks, spheres, thr, reject2, grow), with knobs the host never turns: an edge that is not the reach, a padded box, a ligand in
    any order, spheres larger than needed;
  * the exact reference of every launch: float64 numpy by brute force over all P x Al x Ar pairs in the kernel's operation order, written
    elementwise as (a*b + c*d) + e*f, reading T as the kernel reads it (sterics_ref, iface_ref, pairpot_ref, rescon_bits_ref,
    rescon_finish_ref, hbond_ref, hbond_finish_ref, surface_ref), and the restatement of steps 1 to 3 of walk_front that tells which
    (pose, block) waves leave at the sphere test, which at the box test and which walk;
  * a restatement of the walk itself (the rows, the batches of 64, the fp32 reject), which tests/test_pose_harness_cpu.py holds against
    the brute force and whose seeded mutants it turns on the comparison functions below, to show that they have power;
  * the extended-precision reference of pose_transform (the rotation matrix of the fp32 axis-angle in mpmath at 200 bits);
  * the cases and the comparison functions the GPU tests use.

What is exact and what carries a gate.  Every kernel output here is an integer, a bitmap or a float64 formed by the same IEEE
operations in the same order as the restatement, so every comparison is bitwise - no pair near a cutoff is excused - but two:
  rotation entries of T   sin and cos of the device's library are not libm's.  The gate is 8 x the largest absolute error of the float64
                          numpy restatement of pose_transform against mpmath on the same inputs (pose_gate): the restatement and the
                          device run the same few operations, and the device's sin / cos are specified to a few ulp where libm's are
                          within one.  The translation entries are exact.
  min_dist                1 ulp: the one sqrt whose VALUE is returned.
"""
import copy
import ctypes as C
import functools
from fractions import Fraction

import numpy as np

import kernel_harness as kh
from kernel_harness import HIP_INVALID_VALUE, HIP_SUCCESS, LIBDIR, ROOT, Out, guards_intact, is_sentinel      # noqa: F401 (re-exported)

INF_BITS = 0x7FF0000000000000
MARKER = -77      # prefill of the per-atom outputs "written by the waves that reach the cell walk only"
POSE_GATE_FACTOR = 8.0

SLOTS = ("rot", "tr", "T", "rec", "lig", "sphere", "cell_start", "lig_index", "n_clash", "n_contact", "min_bits", "lig_clash", "lig_contact",
         "exits", "tot", "bits", "class_mask", "lig_class", "rec_degree", "lig_degree", "rec_par", "lig_par", "lig_vdw", "lig_elec", "lig_type",
         "table_q", "e2", "lig_q", "counts", "rec_ante", "lig_ante", "rec_index", "rec_hb", "rec_sb", "lig_hb", "lig_sb",
         "dirs", "rec_class", "rec_exp", "lig_exp", "rec_bur", "lig_buried", "rec_buried", "grid", "geo", "atom_q")
VECS = ("lo", "hi", "center")
DOUBLES = ("edge", "grow", "clash", "contact", "cut2", "soft", "min2", "kc", "lo2", "hb2", "salt2", "c2", "probe")
INTS = ("nx", "ny", "nz", "n", "Ar", "Al", "Rr", "Lr", "W", "Lc", "Wc", "NT", "NB", "top", "Rc", "G", "C")
OPS = ("pose_sterics", "pose_surface", "pose_iface", "pose_rescon", "pose_hbond", "pose_pairpot", "sterics", "sterics_chain", "rescon",
       "rescon_finish", "hbond_finish", "iface", "pairpot", "hbond", "surface", "pose_density", "density")
POSE_OPS = OPS[:6] + ("pose_density",)
# what each pose kernel zeroes next to T: (slot, dtype, entries per pose) - rescon has nothing
POSE_TOTALS = {"pose_sterics": None, "pose_surface": ("tot", np.int32, 32), "pose_iface": ("tot", np.int64, 4), "pose_rescon": None,
               "pose_hbond": ("tot", np.int32, 5), "pose_pairpot": ("tot", np.int64, 2), "pose_density": ("tot", np.int64, 6)}

f32 = np.float32


def f64(x):
    return np.asarray(x, np.float64)


class Call(C.Structure):
    _fields_ = ([("buf", kh.Buf * len(SLOTS))] + [(n, C.c_double * 3) for n in VECS] + [(n, C.c_double) for n in DOUBLES] +
                [("reject2", C.c_float), ("slack", C.c_float)] + [(n, C.c_int) for n in INTS])


compile_shim = functools.partial(kh.compile_shim, "pose")


# ---- binding -----------------------------------------------------------------------------------------------------------------------
class Harness(kh.KernelHarness):
    check = True      # run() asserts success unless told check=False

    def __init__(self, path):
        super().__init__(path, Call, SLOTS, OPS)
        self.lib.ph_check.argtypes = [C.POINTER(Call), C.c_int]
        self.lib.ph_check.restype = C.c_int

    def check_only(self, op, bufs, **scalars):
        """The shim's range checks alone: no device is touched."""
        call, _, keep = self.fill_call(bufs, scalars)
        return int(self.lib.ph_check(C.byref(call), OPS.index(op)))

    # ---- the operations
    def pose(self, op, rot, tr, extra=3):
        """One k_*_pose launch on n = len(rot) poses; every output block has room for `extra` more poses, which must keep the
        sentinel.  Returns T [n + extra, 12] and the totals the kernel zeroes (prefilled with the sentinel)."""
        n = len(rot)
        bufs = dict(rot=np.ascontiguousarray(rot, f32), tr=np.ascontiguousarray(tr, f32), T=Out(np.float64, (n + extra) * 12))
        if op == "pose_sterics":
            bufs.update(n_clash=Out(np.int32, n + extra), n_contact=Out(np.int32, n + extra), min_bits=Out(np.uint64, n + extra))
        elif POSE_TOTALS[op]:
            slot, dt, per = POSE_TOTALS[op]
            bufs[slot] = Out(dt, (n + extra) * per)
        r = self.run(op, bufs, n=n)
        r["T"] = r["T"].reshape(n + extra, 12)
        return r

    def _frame(self, fr):
        return (dict(rec=fr.rec4, lig=fr.lig4, sphere=fr.sphere, cell_start=fr.cell_start, lig_index=fr.lig_index),
                dict(lo=fr.lo, hi=fr.hi, center=fr.center, edge=fr.edge, grow=fr.grow, clash=fr.clash, contact=fr.contact, reject2=fr.reject2,
                     nx=fr.dims[0], ny=fr.dims[1], nz=fr.dims[2], Ar=fr.Ar, Al=fr.Al))

    def sterics(self, fr, T=None, rot=None, tr=None, per_atom=True, base=(0, 0), n=None, check=True):
        """launch_sterics on T [P,12], or with rot / tr the chain k_sterics_pose -> k_sterics.  base: what n_clash / n_contact start as
        (the chain's pose kernel zeroes them).  per_atom: lig_clash / lig_contact given, prefilled with MARKER."""
        P = len(T) if T is not None else len(rot)
        n = P if n is None else n
        bufs, sc = self._frame(fr)
        bufs.update(n_clash=Out(np.int32, init=np.full(P, base[0], np.int32)), n_contact=Out(np.int32, init=np.full(P, base[1], np.int32)),
                    min_bits=Out(np.uint64, init=np.full(P, INF_BITS, np.uint64)), exits=Out(np.uint64, init=np.zeros(2, np.uint64)))
        if per_atom:
            bufs.update(lig_clash=Out(np.int32, init=np.full(P * fr.Al, MARKER, np.int32)),
                        lig_contact=Out(np.int32, init=np.full(P * fr.Al, MARKER, np.int32)))
        if T is not None:
            r = self.run("sterics", dict(bufs, T=np.ascontiguousarray(T, np.float64)), check=check, n=n, **sc)
        else:
            r = self.run("sterics_chain", dict(bufs, rot=np.ascontiguousarray(rot, f32), tr=np.ascontiguousarray(tr, f32),
                                               T=Out(np.float64, P * 12)), check=check, n=n, **sc)
            r["T"] = r["T"].reshape(P, 12)
        r["min_dist"] = r["min_bits"].view(np.float64)
        for k in ("lig_clash", "lig_contact"):
            if k in r:
                r[k] = r[k].reshape(P, fr.Al)
        return r

    def iface(self, fr, T, par, per_atom=True, base=None):
        """launch_iface: tot [P,4] (prefilled with `base`, default 0) and, with per_atom, lig_vdw / lig_elec [P,Al] prefilled with MARKER.
        par: an IfacePar."""
        P = len(T)
        bufs, sc = self._frame(fr)
        bufs.update(T=np.ascontiguousarray(T, np.float64), rec_par=par.rec4(fr), lig_par=par.lig4(fr),
                    tot=Out(np.int64, init=np.zeros((P, 4), np.int64) if base is None else np.asarray(base, np.int64)))
        if per_atom:
            bufs.update(lig_vdw=Out(np.int64, init=np.full(P * fr.Al, MARKER, np.int64)), lig_elec=Out(np.int64, init=np.full(P * fr.Al, MARKER, np.int64)))
        r = self.run("iface", bufs, n=P, cut2=par.cut2, soft=par.soft, min2=par.min2, kc=par.kc, **sc)
        out = dict(tot=r["tot"].reshape(P, 4))
        if per_atom:
            out.update(lig_vdw=r["lig_vdw"].reshape(P, fr.Al), lig_elec=r["lig_elec"].reshape(P, fr.Al))
        return out

    def pairpot(self, fr, T, pot, per_atom=True, counts=True, base=None):
        """launch_pairpot: tot [P,2] (prefilled with `base`, default 0); with per_atom lig_q [P,Al] prefilled with MARKER; with counts
        (the other instantiation) counts [P,T,T,NB], zeroed first.  pot: a PairPot."""
        P = len(T)
        bufs, sc = self._frame(fr)
        bufs.update(T=np.ascontiguousarray(T, np.float64), rec_par=pot.rec4(fr), lig_type=pot.lig_type[fr.lig_index], table_q=pot.table_q,
                    e2=pot.e2, tot=Out(np.int64, init=np.zeros((P, 2), np.int64) if base is None else np.asarray(base, np.int64)))
        if per_atom:
            bufs["lig_q"] = Out(np.int64, init=np.full(P * fr.Al, MARKER, np.int64))
        if counts:
            bufs["counts"] = Out(np.int32, init=np.zeros(P * pot.T * pot.T * pot.NB, np.int32))
        r = self.run("pairpot", bufs, n=P, lo2=pot.e2[0], cut2=pot.e2[pot.NB], NT=pot.T, NB=pot.NB, top=pot.top, **sc)
        out = dict(tot=r["tot"].reshape(P, 2))
        if per_atom:
            out["lig_q"] = r["lig_q"].reshape(P, fr.Al)
        if counts:
            out["counts"] = r["counts"].reshape(P, pot.T, pot.T, pot.NB)
        return out

    def hbond(self, hb, T, per_atom=True, base=None, rec_base=0):
        """launch_hbond, then launch_hbond_finish, as dfm_pose_hbonds chains them: tot [P,5] (entries 0 .. 3 prefilled with `base`, default
        0; entry 4 with the sentinel), bits [P,Lc,Wc] zeroed first; with per_atom rec_hb / rec_sb [P,Nr] prefilled with rec_base (added to)
        and lig_hb / lig_sb [P,Nl] prefilled with MARKER.  hb: an HBond."""
        fr, P = hb.fr, len(T)
        bufs, sc = self._frame(fr)
        tot0 = np.zeros((P, 5), np.int32) if base is None else np.array(base, np.int32)
        tot0[:, 4] = -1
        bufs.update(T=np.ascontiguousarray(T, np.float64), rec_ante=hb.rec_ante4, lig_ante=hb.lig_ante4, rec_index=fr.order,
                    tot=Out(np.int32, init=tot0), bits=Out(np.uint32, init=np.zeros(P * hb.Lc * hb.Wc, np.uint32)))
        if per_atom:
            bufs.update(rec_hb=Out(np.int32, init=np.full(P * fr.Ar, rec_base, np.int32)), rec_sb=Out(np.int32, init=np.full(P * fr.Ar, rec_base, np.int32)),
                        lig_hb=Out(np.int32, init=np.full(P * fr.Al, MARKER, np.int32)), lig_sb=Out(np.int32, init=np.full(P * fr.Al, MARKER, np.int32)))
        r = self.run("hbond", bufs, n=P, hb2=hb.hb2, salt2=hb.salt2, c2=hb.c2, Rc=hb.Rc, Lc=hb.Lc, Wc=hb.Wc, **sc)
        out = dict(tot=r["tot"].reshape(P, 5), bits=r["bits"].reshape(P, hb.Lc, hb.Wc))
        if per_atom:
            out.update(rec_hb=r["rec_hb"].reshape(P, fr.Ar), rec_sb=r["rec_sb"].reshape(P, fr.Ar), lig_hb=r["lig_hb"].reshape(P, fr.Al),
                       lig_sb=r["lig_sb"].reshape(P, fr.Al))
        return out

    def surface(self, sf, T, per_atom=True, base=None):
        """launch_surface (k_surface, then k_surface_finish): rec_bur [P,Ar,G] uint64 zeroed first (the frame's receptor order),
        class_points [P,2,16] prefilled with `base` (default 0; added to); with per_atom lig_buried [P,Al] prefilled with MARKER and
        rec_buried [P,Ar] with the sentinel (every entry is written).  sf: a Surface."""
        fr, P, G = sf.fr, len(T), sf.G
        bufs, sc = self._frame(fr)
        bufs.update(T=np.ascontiguousarray(T, np.float64), dirs=sf.dirs, rec_index=fr.order, rec_class=sf.rec_class[fr.order],
                    lig_class=sf.lig_class[fr.lig_index], rec_exp=sf.rec_exp[fr.order], lig_exp=sf.lig_exp[fr.lig_index],
                    rec_bur=Out(np.uint64, init=np.zeros(P * fr.Ar * G, np.uint64)),
                    tot=Out(np.int32, init=np.zeros((P, 32), np.int32) if base is None else np.asarray(base, np.int32)))
        if per_atom:
            bufs.update(lig_buried=Out(np.int32, init=np.full(P * fr.Al, MARKER, np.int32)), rec_buried=Out(np.int32, P * fr.Ar))
        r = self.run("surface", bufs, n=P, probe=sf.probe, slack=sf.slack, G=G, **sc)
        out = dict(rec_bur=r["rec_bur"].reshape(P, fr.Ar, G), class_points=r["tot"].reshape(P, 2, 16))
        if per_atom:
            out.update(lig_buried=r["lig_buried"].reshape(P, fr.Al), rec_buried=r["rec_buried"].reshape(P, fr.Ar))
        return out

    def rescon(self, fr, T, Rr, Lr):
        """launch_rescon on a frame whose fourth components carry the residue bits: bits [P,Lr,W], zeroed first."""
        P, W = len(T), (Rr + 31) // 32
        bufs, sc = self._frame(fr)
        del bufs["lig_index"]
        r = self.run("rescon", dict(bufs, T=np.ascontiguousarray(T, np.float64), bits=Out(np.uint32, init=np.zeros(P * Lr * W, np.uint32))),
                     n=P, Rr=Rr, Lr=Lr, W=W, **sc)
        return r["bits"].reshape(P, Lr, W)

    def rescon_finish(self, bits, Rr, rec_class, lig_class, degrees=True):
        """launch_rescon_finish alone on bitmaps [P,Lr,W]: tot [P,9] and, with `degrees`, rec_degree [P,Rr] / lig_degree [P,Lr]."""
        P, Lr, W = bits.shape
        bufs = dict(bits=np.ascontiguousarray(bits, np.uint32), class_mask=class_masks(Rr, rec_class),
                    lig_class=np.ascontiguousarray(lig_class, np.int32), tot=Out(np.int32, P * 9))
        if degrees:
            bufs.update(rec_degree=Out(np.int32, P * Rr), lig_degree=Out(np.int32, P * Lr))
        r = self.run("rescon_finish", bufs, n=P, Rr=Rr, Lr=Lr, W=W)
        out = dict(tot=r["tot"].reshape(P, 9))
        if degrees:
            out.update(rec_degree=r["rec_degree"].reshape(P, Rr), lig_degree=r["lig_degree"].reshape(P, Lr))
        return out

    def hbond_finish(self, bits, Lc, Wc, base):
        """launch_hbond_finish alone on words [P, Lc Wc]: tot [P,5] prefilled with `base`."""
        P = len(base)
        r = self.run("hbond_finish", dict(bits=np.ascontiguousarray(bits, np.uint32), tot=Out(np.int32, init=np.asarray(base, np.int32))),
                     n=P, Lc=Lc, Wc=Wc)
        return r["tot"].reshape(P, 5)

    def density(self, dc, T, atom_q=True, base=None, extra=2, check=True, **over):
        """launch_density on the case dc (density_case) and T [P,12] float64.  tot has room for `extra` more poses and starts as `base`
        ([P + extra][6], default zeros); atom_q ([P][Al] and extra * Al entries behind) starts as MARKER.  over: scalars (n, Al, nx, ny,
        nz, C) or the geo buffer as a call that the launcher must refuse wants them."""
        P, Al = len(T), dc["Al"]
        base = np.zeros((P + extra, 6), np.int64) if base is None else np.asarray(base, np.int64)
        bufs = dict(grid=dc["grid4"], geo=over.pop("geo", dc["geo"]), lig=dc["lig4"], T=np.ascontiguousarray(T, np.float64), tot=Out(np.int64, init=base))
        if atom_q:
            bufs["atom_q"] = Out(np.int64, init=np.full((P + extra) * max(Al, 1), MARKER, np.int64))
        sc = dict(nx=dc["dims"][0], ny=dc["dims"][1], nz=dc["dims"][2], n=P, Al=Al, C=dc["C"])
        sc.update(over)
        r = self.run("density", bufs, check=check, **sc)
        r["tot"] = r["tot"].reshape(P + extra, 6)
        return r


# ---- the frame, from the comments of dfm_poseprep.h -----------------------------------------------------------------------------------
def cell_of(x, origin, edge, n):
    """dfm_walkgrid.h: floor((x - origin) / edge) clamped to 0 .. n - 1, in float64."""
    return np.clip(np.floor((f64(x) - origin) / edge), 0.0, float(n - 1)).astype(np.int64)


def morton(c):
    """21 bits of each cell coordinate interleaved, x lowest."""
    code = np.zeros(c.shape[0], np.uint64)
    for b in range(21):
        for k in range(3):
            code |= ((c[:, k].astype(np.uint64) >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + k)
    return code


def frame_numbers(lo, hi, reach):
    """slack, thr and reject2 of build_pose_frame: maxabs = the largest |coordinate| of the receptor's box + 2 reach + 1 in float64,
    slack = max(1e-3, 2.5e-7 maxabs), thr = reach * 1.0001 + slack and reject2 = thr^2 in float32, one rounding per operation."""
    maxabs = max(np.abs(lo).max(), np.abs(hi).max()) + 2.0 * float(f32(reach)) + 1.0
    slack = max(f32(1e-3), f32(2.5e-7 * maxabs))
    thr = f32(f32(reach) * f32(1.0001)) + slack
    return slack, f32(thr), f32(thr * thr)


class Frame:
    """What a cutoff-based creator leaves on the device.  rec [Ar,3], lig [Al,3], center [3] float32; the reach is the contact cutoff.
    The knobs the host never turns: edge (default: the reach), pad (the box grown beyond the atoms), lig_order (a permutation in place
    of the Morton order; the spheres follow it), sphere_scale (radii larger than needed), rec_w / lig_w (int32 bits of the fourth
    components: residue indices).  thr (and with it reject2 and grow) always comes from the atoms' own box."""

    def __init__(self, rec, lig, center, clash, contact, edge=None, pad=0.0, lig_order=None, sphere_scale=1.0, rec_w=None, lig_w=None):
        rec, lig, center = np.ascontiguousarray(rec, f32), np.ascontiguousarray(lig, f32), np.ascontiguousarray(center, f32)
        self.rec_atoms, self.lig_atoms, self.center32 = rec, lig, center
        self.Ar, self.Al = len(rec), len(lig)
        reach = f32(contact)
        self.reach = reach
        self.clash, self.contact = float(f32(clash)), float(reach)
        self.edge = float(reach) if edge is None else float(edge)
        r64 = f64(rec)
        lo0, hi0 = r64.min(0), r64.max(0)
        self.slack, self.thr, self.reject2 = frame_numbers(lo0, hi0, reach)
        self.grow = float(self.thr)
        self.lo, self.hi = lo0 - pad, hi0 + pad
        self.center = f64(center)
        self.dims = tuple(int(v) for v in np.floor((self.hi - self.lo) / self.edge) + 1.0)
        c = np.stack([cell_of(r64[:, k], self.lo[k], self.edge, self.dims[k]) for k in range(3)], 1)
        cell = (c[:, 2] * self.dims[1] + c[:, 1]) * self.dims[0] + c[:, 0]
        self.order = np.argsort(cell, kind="stable").astype(np.int32)
        counts = np.bincount(cell, minlength=int(np.prod(self.dims)))
        self.cell_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        self.max_cell = int(counts.max())
        self.rec4 = np.zeros((self.Ar, 4), f32)
        self.rec4[:, :3] = rec[self.order]
        if rec_w is not None:
            self.rec4[:, 3] = np.asarray(rec_w, np.int32)[self.order].view(f32)
        # the ligand in Morton order of its own cells (origin: its low corner, edge: the grid's), ties in the caller's order
        l64 = f64(lig)
        self.lig_lo = l64.min(0)
        if lig_order is None:
            lc = np.stack([cell_of(l64[:, k], self.lig_lo[k], self.edge, 1 << 21) for k in range(3)], 1)
            lig_order = np.argsort(morton(lc), kind="stable")
        self.lig_index = np.ascontiguousarray(lig_order, np.int32)
        self.lig4 = np.zeros((self.Al, 4), f32)
        self.lig4[:, :3] = lig[self.lig_index]
        if lig_w is not None:
            self.lig4[:, 3] = np.asarray(lig_w, np.int32)[self.lig_index].view(f32)
        # per block of 64 sorted atoms: the centre of its box relative to the rotation centre as fp32, the radius measured from THAT
        # point in float64, (1 + 1e-6) r + 1e-6 rounded to fp32 and one ulp up
        nblk = (self.Al + 63) // 64
        self.sphere = np.zeros((nblk, 4), f32)
        ls = l64[self.lig_index]
        for b in range(nblk):
            a = ls[64 * b:64 * b + 64]
            cen = (0.5 * (a.min(0) + a.max(0)) - self.center).astype(f32)
            d = (a - self.center) - f64(cen)
            r2 = (((0.0 + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max()
            rad = np.nextafter(f32(np.sqrt(r2) * (1.0 + 1e-6) + 1e-6), f32(np.inf))
            self.sphere[b, :3], self.sphere[b, 3] = cen, f32(rad * f32(sphere_scale))


# ---- pose_transform --------------------------------------------------------------------------------------------------------------------
def pose_T(rot, tr):
    """dfm_posewalk.h: pose_transform in float64 numpy, operation by operation.  rot, tr [n,3] float32 -> T [n,12]."""
    rot, tr = np.asarray(rot, f32).reshape(-1, 3), np.asarray(tr, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        x, y, z = f64(rot[:, 0]), f64(rot[:, 1]), f64(rot[:, 2])
        ang = np.sqrt((x * x + y * y) + z * z)
        s = np.where(np.abs(ang) < 1e-6, 0.5 - ang * ang / 48.0, np.sin(0.5 * ang) / ang)
        r, i, j, k = np.cos(0.5 * ang), x * s, y * s, z * s
        two_s = 2.0 / (((r * r + i * i) + j * j) + k * k)
        T = np.stack([1.0 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                      two_s * (i * j + k * r), 1.0 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                      two_s * (i * k - j * r), two_s * (j * k + i * r), 1.0 - two_s * (i * i + j * j),
                      f64(tr[:, 0]), f64(tr[:, 1]), f64(tr[:, 2])], 1)
    return T


def pose_R_mp(rot):
    """The rotation matrix of the fp32 axis-angle vectors rot [n,3] by Rodrigues' formula in mpmath at 200 bits, rounded once to float64:
    [n,9] row-major.  rot = 0 is the identity."""
    import mpmath as mp
    out = np.zeros((len(rot), 9))
    with mp.workprec(200):
        for n, v in enumerate(np.asarray(rot, f32)):
            x, y, z = (mp.mpf(float(c)) for c in v)
            th = mp.sqrt(x * x + y * y + z * z)
            if th == 0:
                out[n] = np.eye(3).reshape(-1)
                continue
            kx, ky, kz = x / th, y / th, z / th
            c, s = mp.cos(th), mp.sin(th)
            v1 = 1 - c
            R = [c + kx * kx * v1, kx * ky * v1 - kz * s, kx * kz * v1 + ky * s,
                 ky * kx * v1 + kz * s, c + ky * ky * v1, ky * kz * v1 - kx * s,
                 kz * kx * v1 - ky * s, kz * ky * v1 + kx * s, c + kz * kz * v1]
            out[n] = [float(e) for e in R]
    return out


PI32, TWO_PI32 = f32(np.pi), f32(2.0 * np.pi)


@functools.lru_cache(maxsize=None)
def pose_rotations():
    """The finite rotations of the pose-kernel tests, [m,3] float32: 0; |rot| = 1e-30, 9.9e-7, 1e-6, 1.1e-6 (the small-angle branch
    and both sides of its threshold), 0.3, pi and 2 pi each at the fp32 nearest and one ulp on either side, 50 - each along one
    generic direction and along one component only."""
    d = np.array([0.36, -0.48, 0.8])
    mags = [1e-30, 9.9e-7, 1e-6, 1.1e-6, 0.3, 50.0]
    for c in (PI32, TWO_PI32):
        mags += [float(np.nextafter(c, f32(0))), float(c), float(np.nextafter(c, f32(10)))]
    rows = [np.zeros(3)]
    for m in mags:
        rows.append(m * d)
        for k in range(3):
            e = np.zeros(3)
            e[k] = m if k != 1 else -m
            rows.append(e)
    return np.asarray(rows, f32)


def pose_inputs(n):
    """rot, tr [n,3] float32: the rotations above in turn, translations of every size and sign."""
    rots = pose_rotations()
    rng = np.random.default_rng(n)
    rot = rots[np.arange(n) % len(rots)] if n > 1 else rots[5:6]
    tr = (rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-3, 5, (n, 1))).astype(f32)
    return rot, tr


@functools.lru_cache(maxsize=None)
def pose_gate():
    """(cpu, gate): the largest absolute error of a rotation entry of the numpy restatement against mpmath on every finite rotation of
    the tests, and the device's gate = 8 x that."""
    rots = pose_rotations()
    cpu = float(np.abs(pose_T(rots, np.zeros_like(rots))[:, :9] - pose_R_mp(rots)).max())
    return cpu, POSE_GATE_FACTOR * cpu


def nonfinite_poses():
    """rot, tr [18,3]: NaN, +inf and -inf in each of the six input positions of an otherwise ordinary pose."""
    rot, tr = np.tile(f32([0.2, -0.1, 0.3]), (18, 1)), np.tile(f32([0.5, 0.25, -0.5]), (18, 1))
    for n, (pos, v) in enumerate((pos, v) for pos in range(6) for v in (np.nan, np.inf, -np.inf)):
        (rot if pos < 3 else tr)[n, pos % 3] = v
    return rot, tr


def check_pose(out, op, rot, tr, extra=3):
    """One k_*_pose launch against everything its header comment promises.  Returns the largest absolute error of a rotation entry."""
    n = len(rot)
    T = out["T"]
    ref, gate = pose_T(rot, tr), pose_gate()[1]
    assert is_sentinel(T[n:].view(np.uint32)).all(), f"{op}: T past n was written"
    assert T[:n, 9:].tobytes() == ref[:, 9:].tobytes(), f"{op}: a translation entry is not the widened fp32"
    fin = np.isfinite(ref).all(1)
    assert not np.isfinite(T[:n][~fin]).all(1).any(), f"{op}: a pose that is not finite has twelve finite entries"
    zero = (f32(rot) == 0).all(1) & fin
    assert (T[:n][zero][:, :9] == np.eye(3).reshape(-1)).all(), f"{op}: rot = 0 is not exactly the identity"
    err = float(np.abs(T[:n][fin][:, :9] - pose_R_mp(rot[fin])).max()) if fin.any() else 0.0
    assert err <= gate, f"{op}: a rotation entry is {err:.3g} off the mpmath rotation, gate {gate:.3g}"
    if op == "pose_sterics":
        assert (out["n_clash"][:n] == 0).all() and (out["n_contact"][:n] == 0).all() and (out["min_bits"][:n] == INF_BITS).all(), op
        for k in ("n_clash", "n_contact", "min_bits"):
            assert is_sentinel(out[k][n:].view(np.uint32)).all(), f"{op}: {k} past n was written"
    elif POSE_TOTALS[op]:
        slot, _, per = POSE_TOTALS[op]
        assert (out[slot][:n * per] == 0).all(), f"{op}: the totals are not zero"
        assert is_sentinel(out[slot][n * per:].view(np.uint32)).all(), f"{op}: the totals past n were written"
    return err


# ---- the exact reference: brute force over all pairs -------------------------------------------------------------------------------------
def posed(fr, T, mutant=None):
    """The ligand atoms in the frame's (sorted) order under every pose, as walk_front forms them: X, Y, Z [P,Al] float64."""
    t = f64(T)[:, None, :]
    if mutant == "T_transposed":
        t = t[:, :, [0, 3, 6, 1, 4, 7, 2, 5, 8, 9, 10, 11]]
    c = fr.center
    with np.errstate(all="ignore"):
        qx, qy, qz = f64(fr.lig4[:, 0]) - c[0], f64(fr.lig4[:, 1]) - c[1], f64(fr.lig4[:, 2]) - c[2]
        X = ((qx * t[..., 0] + qy * t[..., 1]) + qz * t[..., 2]) + c[0] + t[..., 9]
        Y = ((qx * t[..., 3] + qy * t[..., 4]) + qz * t[..., 5]) + c[1] + t[..., 10]
        Z = ((qx * t[..., 6] + qy * t[..., 7]) + qz * t[..., 8]) + c[2] + t[..., 11]
    if mutant == "f32_pose":
        X, Y, Z = (f64(v.astype(f32)) for v in (X, Y, Z))
    return X, Y, Z


def _fused(ex, ey, ez):
    """sqrt(fma(ex, ex, ey * ey) + ez * ez) of three float64 scalars: the first product of the sum not rounded."""
    s = float(Fraction(float(ex)) * Fraction(float(ex)) + Fraction(float(ey) * float(ey)))
    return float(np.sqrt(np.float64(s) + np.float64(ez) * np.float64(ez)))


def distances(fr, X, Y, Z, mutant=None, near=None):
    """d [.., Al, Ar] = sqrt((ex*ex + ey*ey) + ez*ez) on the widened fp32 receptor atom and the float64 ligand atom.  mutant 'fma': one
    product fused, recomputed exactly (fractions) for the pairs within 1e-9 A of a cutoff in `near` - no other decision can move."""
    r = f64(fr.rec4)
    with np.errstate(all="ignore"):
        ex, ey, ez = X[..., None] - r[:, 0], Y[..., None] - r[:, 1], Z[..., None] - r[:, 2]
        d = np.sqrt((ex * ex + ey * ey) + ez * ez)
    if mutant == "fma":
        for cut in near:
            for idx in zip(*np.where(np.abs(d - cut) < 1e-9)):
                d[idx] = _fused(ex[idx], ey[idx], ez[idx])
    return d


def finite_poses(T):
    return np.isfinite(f64(T)).all(1)


def sterics_ref(fr, T):
    """Every result of launch_sterics on zeroed totals by brute force: n_clash, n_contact [P] int32, min_dist [P] float64 (+inf without
    a contact), lig_clash, lig_contact [P,Al] int32 in the caller's atom order, d [P,Al,Ar] in the frame's order.  A pose whose T is
    not finite has nothing."""
    T = f64(T)
    d = distances(fr, *posed(fr, T))
    fin = finite_poses(T)[:, None, None]
    with np.errstate(invalid="ignore"):
        ct, cl = (d < fr.contact) & fin, (d < fr.clash) & (d < fr.contact) & fin
    P = len(T)
    lig_contact, lig_clash = np.zeros((P, fr.Al), np.int32), np.zeros((P, fr.Al), np.int32)
    lig_contact[:, fr.lig_index], lig_clash[:, fr.lig_index] = ct.sum(2), cl.sum(2)
    md = np.where(ct, d, np.inf).reshape(P, -1).min(1)
    return dict(n_clash=cl.sum((1, 2)).astype(np.int32), n_contact=ct.sum((1, 2)).astype(np.int32), min_dist=md, lig_clash=lig_clash,
                lig_contact=lig_contact, d=d)


def walk_front(fr, T, mutant=None):
    """Steps 1 to 3 of dfm_posewalk.h: walk_front for every (pose, block).  status [P,nblk]: 0 walks, 1 leaves at the sphere test, 2 at
    the box test, 3 the pose is not finite; cells [P,nblk,6] = cx0, cx1, cy0, cy1, cz0, cz1 of the ones that walk."""
    T = f64(T)
    P, nblk = len(T), len(fr.sphere)
    status, cells = np.zeros((P, nblk), np.int64), np.zeros((P, nblk, 6), np.int64)
    X, Y, Z = posed(fr, T, mutant)
    c, lo, hi, grow = fr.center, fr.lo, fr.hi, fr.grow
    for p in range(P):
        t = T[p]
        if not np.isfinite(t).all():
            status[p] = 3
            continue
        for b in range(nblk):
            q = f64(fr.sphere[b])
            reach = q[3] + (0.0 if mutant == "sphere_no_grow" else grow)
            cen = [((q[0] * t[3 * k] + q[1] * t[3 * k + 1]) + q[2] * t[3 * k + 2]) + c[k] + t[9 + k] for k in range(3)]
            e = [lo[k] - cen[k] if cen[k] < lo[k] else (cen[k] - hi[k] if cen[k] > hi[k] else 0.0) for k in range(3)]
            if (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] > reach * reach:
                status[p, b] = 1
                continue
            sl = slice(64 * b, 64 * b + 64)
            box = [(v[p, sl].min() - grow, v[p, sl].max() + grow) for v in (X, Y, Z)]
            if any(box[k][0] > hi[k] or box[k][1] < lo[k] for k in range(3)):
                status[p, b] = 2
                continue
            cells[p, b] = [int(cell_of(box[k][m], lo[k], fr.edge, fr.dims[k])) for k in range(3) for m in (0, 1)]
    return status, cells


def exits_ref(status):
    return np.array([(status == 1).sum(), (status == 2).sum()], np.uint64)


MUTANTS = ("f32_pose", "fma", "le", "reject_bare", "reject_factor_only", "first_64_of_a_row", "last_cell_dropped", "lanes_past_Al",
           "T_transposed", "sphere_no_grow", "min_of_last_block")


def sterics_walk(fr, T, mutant=None, base=(0, 0)):
    """The kernel restated WITH its walk: per (pose, block) walk_front, per row the batches of 64, per pair the fp32 reject against the
    fp32 copy of the posed atom, then the float64 decision.  Returns what Harness.sterics returns (per-atom outputs prefilled with MARKER,
    totals with `base`) and rows = the set of receptor atoms per visited row.  Without a mutant it must equal sterics_ref bit for bit: the
    reject and the cell range drop no pair within the contact cutoff."""
    if mutant in ("reject_bare", "reject_factor_only"):      # the same frame with another threshold: no slack and no factor | the factor only
        fr = copy.copy(fr)
        fr.thr = fr.reach if mutant == "reject_bare" else f32(fr.reach * f32(1.0001))
        fr.reject2, fr.grow = f32(fr.thr * fr.thr), float(fr.thr)
    T = f64(T)
    P, Al = len(T), fr.Al
    status, cells = walk_front(fr, T, mutant)
    X, Y, Z = posed(fr, T, mutant)
    out = dict(n_clash=np.full(P, base[0], np.int32), n_contact=np.full(P, base[1], np.int32), min_dist=np.full(P, np.inf),
               lig_clash=np.full((P, Al), MARKER, np.int32), lig_contact=np.full((P, Al), MARKER, np.int32), exits=exits_ref(status))
    rows = set()
    lt = (lambda a, b: a <= b) if mutant == "le" else (lambda a, b: a < b)
    r32 = fr.rec4[:, :3]
    for p in range(P):
        for b in range(status.shape[1]):
            if status[p, b]:
                continue
            cx0, cx1, cy0, cy1, cz0, cz1 = cells[p, b]
            if mutant == "last_cell_dropped":
                cx1 -= 1
            idx = []
            for cz in range(cz0, cz1 + 1):
                for cy in range(cy0, cy1 + 1):
                    row = (cz * fr.dims[1] + cy) * fr.dims[0]
                    b0, b1 = int(fr.cell_start[row + cx0]), int(fr.cell_start[row + cx1 + 1])
                    rows.add(b1 - b0)
                    idx.append(np.arange(b0, min(b1, b0 + 64) if mutant == "first_64_of_a_row" else b1))
            idx = np.concatenate(idx).astype(np.int64)
            lanes = np.arange(64 * b, 64 * b + 64)
            valid = lanes < Al
            lanes = np.minimum(lanes, Al - 1)
            if mutant == "lanes_past_Al":
                valid[:] = True
            x, y, z = X[p, lanes], Y[p, lanes], Z[p, lanes]
            xf, yf, zf = x.astype(f32), y.astype(f32), z.astype(f32)
            r = r32[idx]
            dx, dy, dz = r[None, :, 0] - xf[:, None], r[None, :, 1] - yf[:, None], r[None, :, 2] - zf[:, None]
            go = ~((dx * dx + dy * dy) + dz * dz > fr.reject2) & valid[:, None]
            sub = _Sub(fr, idx)
            d = distances(sub, x, y, z, mutant, (fr.contact, fr.clash))
            ct = go & lt(d, fr.contact)
            cl = ct & lt(d, fr.clash)
            real = lanes[np.arange(64) + 64 * b < Al]
            out["lig_contact"][p, fr.lig_index[real]] = ct.sum(1)[:len(real)]
            out["lig_clash"][p, fr.lig_index[real]] = cl.sum(1)[:len(real)]
            if ct.any():
                out["n_contact"][p] += ct.sum()
                out["n_clash"][p] += cl.sum()
                m = d[ct].min()
                out["min_dist"][p] = m if mutant == "min_of_last_block" else min(out["min_dist"][p], m)
    out["rows"] = rows
    return out


class _Sub:
    """The receptor atoms `idx` of a frame, as distances() reads them."""
    def __init__(self, fr, idx):
        self.rec4 = fr.rec4[idx]


def ulps(a, b):
    """|a - b| in units of the last place of float64, for non-negative finite doubles and +inf (0 where both are +inf)."""
    a, b = f64(a).view(np.int64), f64(b).view(np.int64)
    return np.abs(a - b)


def check_sterics(out, ref, status=None, base=(0, 0), per_atom=True):
    """One launch_sterics against the brute force `ref` (sterics_ref) - every integer bitwise, min_dist within 1 ulp - and, with `status`
    (walk_front), the exits and the per-atom outputs: written exactly on the atoms of the walked blocks, the MARKER everywhere else.
    Returns (decisions compared, min_dist values that are not bitwise)."""
    P, Al = ref["lig_contact"].shape
    np.testing.assert_array_equal(out["n_contact"], ref["n_contact"] + np.int32(base[1]), "n_contact")
    np.testing.assert_array_equal(out["n_clash"], ref["n_clash"] + np.int32(base[0]), "n_clash")
    u = ulps(out["min_dist"], ref["min_dist"])
    assert (u <= 1).all(), f"min_dist is {u.max()} ulp off the reference"
    if status is not None:
        np.testing.assert_array_equal(out["exits"], exits_ref(status), "exits (sphere test, box test)")
    if per_atom:
        if status is not None:
            walked = np.zeros((P, Al), bool)
            for b in range(status.shape[1]):
                walked[:, ref["index"][64 * b:64 * b + 64]] = (status[:, b] == 0)[:, None]
        else:
            walked = np.ones((P, Al), bool)
        for k in ("lig_clash", "lig_contact"):
            np.testing.assert_array_equal(out[k], np.where(walked, ref[k], MARKER), k)
            assert (ref[k][~walked] == 0).all(), f"{k}: an atom of a block that left early has a pair in the reference"
    return 2 * ref["d"].size, int((u != 0).sum())


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
class Case:
    """One frame, its poses T [P,12] (fed directly) and, cached, its brute-force reference and walk_front."""

    def __init__(self, name, fr, T, host_shaped=True, **extra):
        self.name, self.fr, self.T, self.host_shaped = name, fr, np.ascontiguousarray(T, np.float64), host_shaped
        self.__dict__.update(extra)

    @functools.cached_property
    def ref(self):
        r = sterics_ref(self.fr, self.T)
        r["index"] = self.fr.lig_index
        return r

    @functools.cached_property
    def front(self):
        return walk_front(self.fr, self.T)

    def __repr__(self):
        return self.name


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def touching_poses(rng, P, s_rot=0.4, s_tr=1.5):
    rot, tr = (s_rot * rng.standard_normal((P, 3))).astype(f32), (s_tr * rng.standard_normal((P, 3))).astype(f32)
    return rot, tr


def lump(rng, n, center, spread):
    return (spread * rng.standard_normal((n, 3)) + np.asarray(center)).astype(f32)


def centre_of(lig):
    return f64(lig).mean(0).astype(f32)


GENERIC = dict(Ar=300, Al=130, P=6, clash=3.0, contact=5.0)


@functools.lru_cache(maxsize=None)
def generic_atoms(seed=0, off=(0.0, 0.0, 0.0)):
    """The generic complex: 300 receptor atoms, 130 ligand atoms (three blocks, the last of two atoms) touching them, six poses of which
    the last is moved 60 A away (every block leaves at the sphere test) and the fifth just far enough along x that a block leaves at
    the box test."""
    rng = np.random.default_rng([5, seed])
    off = np.asarray(off)
    rec, lig = lump(rng, GENERIC["Ar"], off, 7.0), lump(rng, GENERIC["Al"], off + [6.0, 0.0, 0.0], 4.0)
    rot, tr = touching_poses(rng, GENERIC["P"])
    tr[-1] = f32([60.0, -40.0, 10.0])
    # pose 4: no rotation, pushed out along x to the first half A at which a block passes the sphere test and leaves at the box test
    cen = centre_of(lig)
    fr = Frame(rec, lig, cen, GENERIC["clash"], GENERIC["contact"])
    rot[4] = 0
    for tx in np.arange(5.0, 60.0, 0.5):
        tr[4] = f32([tx, 0.0, 0.0])
        if (walk_front(fr, pose_T(rot[4:5], tr[4:5]))[0] == 2).any():
            break
    return rec, lig, cen, rot, tr


@functools.lru_cache(maxsize=None)
def generic_case(seed=0):
    rec, lig, cen, rot, tr = generic_atoms(seed)
    return Case(f"generic {seed}", Frame(rec, lig, cen, GENERIC["clash"], GENERIC["contact"]), pose_T(rot, tr), rot=rot, tr=tr)


@functools.lru_cache(maxsize=None)
def grid_variants():
    """The generic complex under grids that are not the host's own; every integer output and min_dist must equal generic_case(0)'s."""
    rec, lig, cen, rot, tr = generic_atoms(0)
    T, k = pose_T(rot, tr), (GENERIC["clash"], GENERIC["contact"])
    perm = np.random.default_rng(9).permutation(len(lig))
    mk = lambda name, **kw: Case(name, Frame(rec, lig, cen, *k, **kw), T, host_shaped=False)
    return (mk("edge = reach / 2", edge=2.5), mk("edge = 2.5 reach", edge=12.5), mk("box padded by 7 A", pad=7.0),
            mk("1 x 1 x 1 grid", edge=1000.0), mk("ligand in random order", lig_order=perm), mk("spheres of twice the radius", sphere_scale=2.0))


@functools.lru_cache(maxsize=None)
def size_cases():
    """Al = 1, 63, 64, 65, 129 against Ar = 1, with P = 1, 2, 8."""
    out = []
    for n, (Al, P) in enumerate(zip((1, 63, 64, 65, 129), (1, 2, 8, 1, 2))):
        rng = np.random.default_rng([6, Al])
        rec, lig = f32([[0.5, -0.25, 1.0]]), lump(rng, Al, (1.0, 0.0, 0.0), 2.0)
        rot, tr = touching_poses(rng, P, 0.4, 0.5)
        out.append(Case(f"Al {Al} Ar 1 P {P}", Frame(rec, lig, centre_of(lig), 3.0, 5.0), pose_T(rot, tr)))
    return tuple(out)


ROW_COUNTS = (0, 1, 63, 64, 65, 128, 129)


@functools.lru_cache(maxsize=None)
def row_cases():
    """A receptor of three rows along y (5 A cells): N atoms in the row y = 1 spread over three cells in x, five atoms each in the rows
    y = 0 and y = 2; a ligand of 65 atoms over all of them.  The walk of its first block reads a row of exactly N atoms.  Last: one
    cell of 200 coincident atoms."""
    out = []
    for N in ROW_COUNTS:
        rng = np.random.default_rng([7, N])
        side = lambda y: np.stack([rng.uniform(0.0, 14.9, 5), np.full(5, y), rng.uniform(0.0, 4.9, 5)], 1)
        mid = np.stack([rng.uniform(0.1, 14.8, N), rng.uniform(5.1, 9.9, N), rng.uniform(0.0, 4.9, N)], 1)
        rec = np.concatenate([side(0.0), mid, side(14.9)]).astype(f32)
        rec[0], rec[-1] = (0.0, 0.0, 0.0), (14.9, 14.9, 4.9)      # the box, whatever N
        lig = np.stack([rng.uniform(1.0, 14.0, 65), rng.uniform(3.0, 12.0, 65), rng.uniform(0.0, 8.0, 65)], 1).astype(f32)
        rot, tr = touching_poses(rng, 2, 0.1, 0.3)
        out.append(Case(f"row of {N}", Frame(rec, lig, centre_of(lig), 3.0, 5.0), pose_T(rot, tr), row=N))
    rng = np.random.default_rng(8)
    rec = np.concatenate([np.tile(f32([[2.0, 2.5, 1.5]]), (200, 1)), lump(rng, 30, (6.0, 6.0, 6.0), 5.0)])
    lig = lump(rng, 65, (3.0, 3.0, 3.0), 2.5)
    rot, tr = touching_poses(rng, 2, 0.2, 0.5)
    out.append(Case("cell of 200 coincident atoms", Frame(rec, lig, centre_of(lig), 3.0, 5.0), pose_T(rot, tr), row=None))
    return tuple(out)


QUARTER_Z = np.array([0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0])


@functools.lru_cache(maxsize=None)
def tie_cases():
    """Lattice coordinates (multiples of 0.25 A), T the identity or a quarter turn about z with integer entries and lattice translations:
    every posed coordinate, every squared distance and every sqrt of a planted pair is exact in float64.  Planted: ligand atoms at
    3-4-5 from receptor atoms (d = 5 exactly: no contact at contact = 5, a contact at contact = nextafter(5, inf) in fp32), at 0-0-3
    (d = 3 = the clash cutoff: no clash) and at d = 0.  Third case: clash == contact."""
    rng = np.random.default_rng(12)
    rec = (rng.integers(0, 81, (120, 3)) * 0.25).astype(f32)
    lig = (rng.integers(0, 81, (70, 3)) * 0.25 + [4.0, 0.0, 0.0]).astype(f32)
    cen = f32([12.0, 10.0, 10.0])
    for n, (i, off) in enumerate(((3, (3.0, 4.0, 0.0)), (40, (0.0, -4.0, 3.0)), (77, (0.0, 0.0, 3.0)), (100, (0.0, 0.0, 0.0)),
                                  (119, (-4.0, 0.0, -3.0)))):
        lig[13 * n] = rec[i] + f32(off)      # under the identity pose
    T = np.zeros((4, 12))
    T[0, :9] = T[1, :9] = np.eye(3).reshape(-1)
    T[1, 9:] = (0.25, -0.5, 0.0)
    T[2, :9] = T[3, :9] = QUARTER_Z
    T[3, 9:] = (1.0, 0.25, -0.75)
    up = float(np.nextafter(f32(5.0), f32(np.inf)))
    return (Case("ties contact 5", Frame(rec, lig, cen, 3.0, 5.0), T, planted=5),
            Case("ties contact 5 + 1 ulp", Frame(rec, lig, cen, 3.0, up), T, planted=5),
            Case("ties clash = contact", Frame(rec, lig, cen, 5.0, 5.0), T, planted=5))


FAR = (((3000.0, -2500.0, 1800.0), 5.0), ((20000.0, -20000.0, 20000.0), 3.0))
FAR_PLANTED = 1500


@functools.lru_cache(maxsize=None)
def far_cases():
    """The complex, centre included, far from the origin, where the fp32 copy of a posed atom is off by up to 2^-24 |coordinate|: the
    fp32 reject must not drop one pair the float64 test counts.  Planted: FAR_PLANTED ligand atoms, each at a distance below the contact
    cutoff by 1e-7 .. 1e-2 A (log-uniform) from one receptor atom, under the identity pose; then a
    translation and a rotation of 1e-3 A or so, after which the posed atoms are no fp32 numbers any more."""
    out = []
    for off, reach in FAR:
        rng = np.random.default_rng([13, int(reach)])
        off = np.asarray(off)
        rec = lump(rng, 200, off, 6.0)
        gap = 10.0 ** rng.uniform(-7.0, -2.0, FAR_PLANTED)
        lig = (f64(rec[rng.integers(0, 200, FAR_PLANTED)]) + _unit(rng.standard_normal((FAR_PLANTED, 3))) * (reach - gap)[:, None]).astype(f32)
        lig = np.concatenate([lig, lump(rng, 36, off + [5.0, 0.0, 0.0], 3.0)])
        T = np.zeros((2, 12))
        T[:, :9] = np.eye(3).reshape(-1)
        T[1, 9:] = (0.001, -0.002, 0.0005)
        T = np.concatenate([T, pose_T(f32([[1e-4, 2e-4, -1e-4]]), f32([[0.0, 0.0, 0.0]]))])
        out.append(Case(f"far {int(off[0])} reach {int(reach)}", Frame(rec, lig, centre_of(lig), 0.6 * reach, reach), T, reach=reach))
    return tuple(out)


def last_hundredth(case):
    """Pairs of the reference in the last 1e-2 A below the contact cutoff."""
    d = case.ref["d"]
    return int(((d < case.fr.contact) & (d > case.fr.contact - 1e-2)).sum())


@functools.lru_cache(maxsize=None)
def knife_cases():
    """The generic complex with the cutoffs ON distances of its own pairs (the kernel takes the cutoffs as doubles): contact = the d
    of a pair whose distance with one product fused is SMALLER (the reference: d == contact, no pair; a contracted kernel: a pair), and
    contact = the next double above the d of a pair whose fused distance is LARGER (the reference: a pair; contracted: none)."""
    c = generic_case(0)
    fr, (X, Y, Z) = c.fr, posed(c.fr, c.T)
    d = c.ref["d"]
    r = f64(fr.rec4)
    picks = {}
    for p, a, b in zip(*np.where((d > 4.0) & (d < 6.0))):
        fd = _fused(X[p, a] - r[b, 0], Y[p, a] - r[b, 1], Z[p, a] - r[b, 2])
        if fd < d[p, a, b]:
            picks.setdefault("below", float(d[p, a, b]))
        elif fd > d[p, a, b]:
            picks.setdefault("above", float(np.nextafter(d[p, a, b], np.inf)))
        if len(picks) == 2:
            break
    out = []
    for k, cut in sorted(picks.items()):
        f = Frame(fr.rec_atoms, fr.lig_atoms, fr.center32, 3.0, 6.0)      # the frame of a 6 A reach: the cutoff lies inside it
        f.contact = cut
        out.append(Case(f"knife edge, fused {k}", f, c.T, host_shaped=False))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def nonfinite_T_case():
    """24 + 2 poses of the generic complex in one launch: each of the 12 entries of pose 0's T set to NaN, then to +inf, with the
    untouched pose before and after them."""
    c = generic_case(0)
    T = np.tile(c.T[0], (26, 1))
    for k in range(12):
        T[1 + k, k], T[13 + k, k] = np.nan, np.inf
    return Case("non-finite entries of T", c.fr, T)


def walk_cases():
    """Every case of the exact comparison of launch_sterics."""
    return (generic_case(0), generic_case(1)) + grid_variants() + size_cases() + row_cases() + tie_cases() + far_cases() + knife_cases() + \
        (nonfinite_T_case(),)


def host_shaped_cases():
    return tuple(c for c in walk_cases() if c.host_shaped)


# ---- residue contacts --------------------------------------------------------------------------------------------------------------------
def class_masks(Rr, cls):
    """mask [3][W]: bit i & 31 of word i >> 5 of mask c is set iff receptor residue i has class c."""
    W = (Rr + 31) // 32
    m = np.zeros((3, W), np.uint32)
    for i in range(Rr):
        m[int(cls[i]), i >> 5] |= np.uint32(1 << (i & 31))
    return m


def rescon_bits_ref(fr, T, rec_res, lig_res, Rr, Lr, mutant=None):
    """bits [P,Lr,W] of launch_rescon by brute force: bit (i, j) iff an atom of receptor residue i and one of ligand residue j are closer
    than the cutoff.  mutant 'last_kept': the skip of a repeated receptor residue carried over from one ligand atom to the next."""
    W = (Rr + 31) // 32
    d = distances(fr, *posed(fr, T))
    with np.errstate(invalid="ignore"):
        ct = (d < fr.contact) & finite_poses(T)[:, None, None]
    rr, lr = np.asarray(rec_res)[fr.order], np.asarray(lig_res)[fr.lig_index]
    bits = np.zeros((len(T), Lr, W), np.uint32)
    for p in range(len(T)):
        last = -1
        for a in range(fr.Al):
            if mutant != "last_kept":
                last = -1
            for b in np.where(ct[p, a])[0]:
                i = int(rr[b])
                if i != last:
                    last = i
                    bits[p, lr[a], i >> 5] |= np.uint32(1 << (i & 31))
    return bits


@functools.lru_cache(maxsize=None)
def rescon_case():
    """The generic complex with Rr = 4096 (atoms of residues 0, 31, 32, 4095 and a spread of others) and Lr = 70; ligand residues 0
    and 1 alternate atom by atom, and the receptor atoms nearest the ligand are all of residue 31: a ligand atom meets one receptor
    residue through many atoms, and consecutive ligand atoms of DIFFERENT residues meet the same one."""
    rec, lig, cen, rot, tr = generic_atoms(0)
    rng = np.random.default_rng(21)
    rec_res = rng.choice([0, 31, 32, 4095, 64, 1000, 2047, 2048], len(rec)).astype(np.int32)
    near = np.argsort(np.linalg.norm(f64(rec) - f64(cen), axis=1))[:60]
    rec_res[near] = 31
    lig_res = (np.arange(len(lig)) % 2).astype(np.int32)
    lig_res[100:] = rng.integers(2, 70, len(lig) - 100)
    fr = Frame(rec, lig, cen, 3.0, 5.0, rec_w=rec_res, lig_w=lig_res, lig_order=np.arange(len(lig)))
    return Case("rescon Rr 4096", fr, pose_T(rot, tr), host_shaped=False, rec_res=rec_res, lig_res=lig_res, Rr=4096, Lr=70)


def popcount(x):
    return np.unpackbits(np.ascontiguousarray(x, np.uint32).view(np.uint8), axis=-1).reshape(x.shape + (32,)).sum(-1).astype(np.int64)


def rescon_finish_ref(bits, Rr, rec_class, lig_class, mutant=None):
    """tot [P,9] = AA, AP, AC, PP, PC, CC, pairs, receptor residues, ligand residues and both degree arrays, from popcounts.  mutant
    'words_64_up_dropped': the second pass over the words of a row lost."""
    bits = np.asarray(bits, np.uint32)
    P, Lr, W = bits.shape
    seen = bits.copy()
    if mutant == "words_64_up_dropped":
        seen[:, :, 64:] = 0
    m, lc = class_masks(Rr, rec_class), np.asarray(lig_class)
    t = np.zeros((P, 3, 3), np.int64)
    for a in range(3):
        for c in range(3):
            t[:, a, c] = popcount(seen[:, lc == a] & m[c]).sum((1, 2))
    tot = np.stack([t[:, 0, 0], t[:, 0, 1] + t[:, 1, 0], t[:, 0, 2] + t[:, 2, 0], t[:, 1, 1], t[:, 1, 2] + t[:, 2, 1], t[:, 2, 2],
                    t.sum((1, 2)), popcount(np.bitwise_or.reduce(seen, 1)).sum(1), (popcount(bits).sum(2) != 0).sum(1)], 1).astype(np.int32)
    i = np.arange(Rr)
    rec_degree = ((bits[:, :, i >> 5] >> (i & 31).astype(np.uint32)) & 1).sum(1).astype(np.int32)
    return dict(tot=tot, rec_degree=rec_degree, lig_degree=popcount(bits).sum(2).astype(np.int32))


FINISH_RR = (1, 31, 32, 33, 2048, 2049, 4096)
FINISH_LR = (1, 63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def finish_inputs(Rr, Lr):
    """bits [3,Lr,W] made in numpy, never from poses: densities 0, 0.5 and all ones (no bit at or above Rr); random classes."""
    rng = np.random.default_rng([31, Rr, Lr])
    W = (Rr + 31) // 32
    valid = np.zeros(W * 32, np.uint8)
    valid[:Rr] = 1
    valid = np.packbits(valid, bitorder="little").view(np.uint32)
    bits = np.stack([np.zeros((Lr, W), np.uint32), rng.integers(0, 1 << 32, (Lr, W), dtype=np.uint64).astype(np.uint32),
                     np.full((Lr, W), 0xffffffff, np.uint32)]) & valid
    return bits, rng.integers(0, 3, Rr).astype(np.uint8), rng.integers(0, 3, Lr).astype(np.int32)


def check_finish(out, ref, degrees=True):
    np.testing.assert_array_equal(out["tot"], ref["tot"], "the nine totals")
    if degrees:
        np.testing.assert_array_equal(out["rec_degree"], ref["rec_degree"], "rec_degree")
        np.testing.assert_array_equal(out["lig_degree"], ref["lig_degree"], "lig_degree")


HBOND_WORDS = ((0, 0), (1, 1), (1, 63), (2, 32), (5, 13), (1000, 1))      # (Lc, Wc): 0, 1, 63, 64, 65, 1000 words


def hbond_finish_ref(bits, base, mutant=None):
    """tot [P,5]: entry 4 = the set bits of the pose's words, entries 0 .. 3 untouched.  mutant 'tail_dropped': the words past the last
    full 64 lost."""
    bits = np.asarray(bits, np.uint32).reshape(len(base), -1)
    if mutant == "tail_dropped":
        bits = bits[:, :bits.shape[1] - bits.shape[1] % 64]
    out = np.array(base, np.int32)
    out[:, 4] = popcount(bits).sum(1) if bits.shape[1] else 0
    return out


# ---- interface energy and pair potential: exact against their restatements ---------------------------------------------------------------
QUANTA = 1048576.0      # 2^20 per kcal/mol


def r2_of(fr, T):
    """r2 [P,Al,Ar] = (ex*ex + ey*ey) + ez*ez in the frame's order; NaN for a pose that is not finite."""
    X, Y, Z = posed(fr, T)
    r = f64(fr.rec4)
    with np.errstate(all="ignore"):
        ex, ey, ez = X[..., None] - r[:, 0], Y[..., None] - r[:, 1], Z[..., None] - r[:, 2]
        r2 = (ex * ex + ey * ey) + ez * ez
    return np.where(finite_poses(T)[:, None, None], r2, np.nan)


def walked_atoms(fr, status):
    """[P,Al] in the caller's atom order: the atom's block reaches the cell walk."""
    w = np.zeros((status.shape[0], fr.Al), bool)
    for b in range(status.shape[1]):
        w[:, fr.lig_index[64 * b:64 * b + 64]] = (status[:, b] == 0)[:, None]
    return w


class IfacePar:
    """The per-atom (rmin_half, sqrt_eps, charge) rows [n,3] float32 of both chains in the caller's order and the call's scalars, as
    dfm_iface_create widens them: cut2 = cutoff^2, soft, min2 = elec_min_dist^2, kc = 332.0637 / dielectric_slope."""

    def __init__(self, rec_par, lig_par, cutoff, soft=0.6, elec_min_dist=3.0, dielectric_slope=4.0):
        self.rec_par, self.lig_par = np.ascontiguousarray(rec_par, f32), np.ascontiguousarray(lig_par, f32)
        c, m = float(f32(cutoff)), float(f32(elec_min_dist))
        self.cutoff, self.cut2, self.soft, self.min2 = f32(cutoff), c * c, float(f32(soft)), m * m
        self.kc = 332.0637 / float(f32(dielectric_slope))
        self.args = (float(cutoff), float(soft), float(elec_min_dist), float(dielectric_slope))

    def rec4(self, fr):
        v = np.zeros((fr.Ar, 4), f32)
        v[:, :3] = self.rec_par[fr.order]
        return v

    def lig4(self, fr):
        v = np.zeros((fr.Al, 4), f32)
        v[:, :3] = self.lig_par[fr.lig_index]
        return v


def iface_ref(fr, T, par, mutant=None):
    """launch_iface on zeroed totals by brute force: tot [P,4] = (rep_q, att_q, elec_q, n_pairs) int64, lig_vdw / lig_elec [P,Al] in the
    caller's order; every term in the kernel's operation order, rounded to quanta ties-to-even, then integer sums."""
    r2 = r2_of(fr, T)
    rp, lp = f64(par.rec4(fr)), f64(par.lig4(fr))
    with np.errstate(all="ignore"):
        pair = r2 <= par.cut2 if mutant == "le" else r2 < par.cut2
        Rm = lp[:, None, 0] + rp[None, :, 0]
        f = par.soft * Rm
        ff = f * f
        r2v = np.where(r2 < ff, ff, r2)
        s2 = (Rm * Rm) / r2v
        s6 = (s2 * s2) * s2
        e = lp[:, None, 1] * rp[None, :, 1]
        t_rep, t_att = e * (s6 * s6), -2.0 * (e * s6)
        r2c = r2 if mutant == "no_elec_clamp" else np.where(r2 < par.min2, par.min2, r2)
        t_elec = (par.kc * (lp[:, None, 2] * rp[None, :, 2])) / r2c
        q = [np.where(pair, np.rint(np.where(pair, t, 0.0) * QUANTA), 0.0).astype(np.int64) for t in (t_rep, t_att, t_elec)]
    tot = np.stack([q[0].sum((1, 2)), q[1].sum((1, 2)), q[2].sum((1, 2)), pair.sum((1, 2))], 1).astype(np.int64)
    lig_vdw, lig_elec = np.zeros((len(T), fr.Al), np.int64), np.zeros((len(T), fr.Al), np.int64)
    lig_vdw[:, fr.lig_index], lig_elec[:, fr.lig_index] = (q[0] + q[1]).sum(2), q[2].sum(2)
    return dict(tot=tot, lig_vdw=lig_vdw, lig_elec=lig_elec, r2=r2, soft_pairs=int((pair & (r2 < ff)).sum()),
                clamped_pairs=int((pair & (r2 < par.min2)).sum()))


def check_iface(out, ref, fr, status, base=None, per_atom=True):
    want = ref["tot"] if base is None else ref["tot"] + np.asarray(base, np.int64)      # (wraps like the unsigned atomics)
    np.testing.assert_array_equal(out["tot"], want, "tot (rep_q, att_q, elec_q, n_pairs)")
    if per_atom:
        w = walked_atoms(fr, status)
        for k in ("lig_vdw", "lig_elec"):
            np.testing.assert_array_equal(out[k], np.where(w, ref[k], MARKER), k)
    return 4 * ref["r2"].size


class PairPot:
    """Types [n] int32 of both chains in the caller's order, edges [NB+1] float32, table [T,T,NB] float32 kcal/mol indexed (ligand type,
    receptor type, bin), as dfm_pairpot_create prepares them: table_q = rint(table 2^20) transposed to (receptor type, ligand type, bin),
    e2 = the exact squares of the edges in 128 slots, then +inf, top = the largest power of two <= NB."""

    def __init__(self, rec_type, lig_type, edges, table):
        self.rec_type, self.lig_type = np.ascontiguousarray(rec_type, np.int32), np.ascontiguousarray(lig_type, np.int32)
        self.edges, self.table = np.ascontiguousarray(edges, f32), np.ascontiguousarray(table, f32)
        self.T, self.NB = self.table.shape[0], self.table.shape[2]
        assert self.table.shape == (self.T, self.T, self.NB) and self.edges.shape == (self.NB + 1,)
        self.table_q = np.ascontiguousarray(np.rint(f64(self.table) * QUANTA).astype(np.int32).transpose(1, 0, 2))
        self.e2 = np.full(128, np.inf)
        self.e2[:self.NB + 1] = f64(self.edges) * f64(self.edges)
        self.top = 1
        while self.top * 2 <= self.NB:
            self.top *= 2

    def rec4(self, fr):
        v = np.zeros((fr.Ar, 4), np.int32)
        v[:, 0] = self.rec_type[fr.order]
        v[:, 1] = v[:, 0] * self.T * self.NB
        return v.view(f32)


def pairpot_ref(fr, T, pot, mutant=None):
    """launch_pairpot on zeroed totals by brute force: tot [P,2] = (energy_q, n_pairs) int64, lig_q [P,Al] in the caller's order, counts
    [P,T,T,NB] (ligand type, receptor type, bin) int32.  A pair has e2[0] <= r2 < e2[NB]; its bin is #{j : e2[j] <= r2} - 1.  mutant
    'bin_off_by_one': e2[j] < r2 (a pair ON an edge falls into the bin below)."""
    r2 = r2_of(fr, T)
    e2 = pot.e2[:pot.NB + 1]
    with np.errstate(invalid="ignore"):
        pair = (r2 >= e2[0]) & (r2 < e2[-1])
    side = "left" if mutant == "bin_off_by_one" else "right"
    k = np.clip(np.searchsorted(e2, np.where(pair, r2, e2[0]), side=side) - 1, 0, pot.NB - 1)
    ta, tb = pot.lig_type[fr.lig_index][None, :, None], pot.rec_type[fr.order][None, None, :]
    val = np.where(pair, pot.table_q[tb, ta, k].astype(np.int64), 0)
    P = len(T)
    lig_q = np.zeros((P, fr.Al), np.int64)
    lig_q[:, fr.lig_index] = val.sum(2)
    counts = np.zeros((P, pot.T, pot.T, pot.NB), np.int32)
    pp, aa, bb = np.where(pair)
    np.add.at(counts, (pp, pot.lig_type[fr.lig_index][aa], pot.rec_type[fr.order][bb], k[pp, aa, bb]), 1)
    return dict(tot=np.stack([val.sum((1, 2)), pair.sum((1, 2))], 1).astype(np.int64), lig_q=lig_q, counts=counts, r2=r2, pair=pair, k=k)


def check_pairpot(out, ref, fr, status, base=None, per_atom=True, counts=True):
    want = ref["tot"] if base is None else ref["tot"] + np.asarray(base, np.int64)
    np.testing.assert_array_equal(out["tot"], want, "tot (energy_q, n_pairs)")
    if per_atom:
        np.testing.assert_array_equal(out["lig_q"], np.where(walked_atoms(fr, status), ref["lig_q"], MARKER), "lig_q")
    if counts:
        np.testing.assert_array_equal(out["counts"], ref["counts"], "counts")
        np.testing.assert_array_equal(out["counts"].sum((1, 2, 3)), ref["tot"][:, 1], "the counts add up to n_pairs")
    return 2 * ref["r2"].size


@functools.lru_cache(maxsize=None)
def iface_cases():
    """(name, Case, IfacePar).  The generic complex at 8 A with generic parameters; the same with the parameters at their limits
    (sqrt_eps 0 and 2, charges 0 and +-4, soft = 0.5, elec_min_dist above most pairs) and the far pose; the size cases; a lattice case
    with pairs at r2 == cut2 exactly (3-4-5 at cutoff 5: no pair), one fp32 ulp of cutoff above it (a pair) and r2 = 0; a case whose
    charges are all of opposite sign and whose well is deep, so that att and elec are negative (the unsigned atomics wrap back)."""
    out = []
    rec, lig, cen, rot, tr = generic_atoms(0)
    rng = np.random.default_rng(41)
    par = lambda n, qs=1.0: np.stack([rng.uniform(1.0, 2.2, n), rng.uniform(0.05, 0.5, n), qs * rng.uniform(-1.0, 1.0, n)], 1).astype(f32)
    T = pose_T(rot, tr)
    fr8 = Frame(rec, lig, cen, 3.0, 8.0)
    out.append(("generic 8 A", Case("iface generic", fr8, T, rot=rot, tr=tr), IfacePar(par(300), par(130), 8.0)))
    rp, lp = par(300), par(130)
    rp[::3, 1], rp[1::3, 1], rp[::4, 2], rp[1::4, 2], rp[2::4, 2] = 0.0, 2.0, 0.0, 4.0, -4.0
    lp[::2, 1], lp[::5, 2], lp[1::5, 2] = 2.0, -4.0, 0.0
    out.append(("limits", Case("iface limits", fr8, T), IfacePar(rp, lp, 8.0, soft=0.5, elec_min_dist=6.0, dielectric_slope=1.0)))
    rn, ln = par(300), par(130)
    rn[:, 1], ln[:, 1], rn[:, 2], ln[:, 2] = 0.5, 0.5, np.abs(rn[:, 2]) + 0.1, -np.abs(ln[:, 2]) - 0.1
    out.append(("negative sums", Case("iface negative", fr8, T), IfacePar(rn, ln, 8.0, soft=1.0)))
    for c in size_cases():
        out.append((c.name, c, IfacePar(par(c.fr.Ar), par(c.fr.Al), 5.0)))
    t = tie_cases()
    out.append(("ties cutoff 5", t[0], IfacePar(par(t[0].fr.Ar), par(t[0].fr.Al), 5.0)))
    out.append(("ties cutoff 5 + 1 ulp", t[1], IfacePar(par(t[1].fr.Ar), par(t[1].fr.Al), np.nextafter(f32(5.0), f32(np.inf)))))
    return tuple(out)


PAIRPOT_NB = (1, 2, 3, 30, 63, 64)


@functools.lru_cache(maxsize=None)
def pairpot_cases():
    """(name, Case, PairPot).  The generic complex with NB = 1, 2, 3, 30, 63, 64 bins up to 8 A (top = 1, 2, 2, 16, 32, 64), edges[0] =
    2.5 A with pairs below it, T = 3 (T = 1 at NB = 1, T = 256 at NB = 2), entries of +-2^30 quanta; the size cases; a lattice case with
    integer edges 0 .. 8 (and 3 .. 8), where pairs sit at integer distances: r2 == e2[k] is bin k, and r2 == e2[NB] no pair."""
    out = []
    rec, lig, cen, rot, tr = generic_atoms(0)
    T = pose_T(rot, tr)
    c8 = Case("pairpot generic", Frame(rec, lig, cen, 3.0, 8.0), T, rot=rot, tr=tr)
    for NB in PAIRPOT_NB:
        rng = np.random.default_rng([43, NB])
        NT = {1: 1, 2: 256}.get(NB, 3)
        edges = np.linspace(2.5, 8.0, NB + 1).astype(f32)
        table = rng.uniform(-3.0, 3.0, (NT, NT, NB)).astype(f32)
        table.reshape(-1)[::7], table.reshape(-1)[3::7] = 1024.0, -1024.0
        out.append((f"NB {NB} T {NT}", c8, PairPot(rng.integers(0, NT, 300), rng.integers(0, NT, 130), edges, table)))
    rng = np.random.default_rng(44)
    for c in size_cases():
        out.append((c.name, c, PairPot(rng.integers(0, 3, c.fr.Ar), rng.integers(0, 3, c.fr.Al), np.linspace(0.0, 5.0, 31).astype(f32),
                                       rng.uniform(-3.0, 3.0, (3, 3, 30)).astype(f32))))
    t = tie_cases()
    lat = t[0].fr.lig_atoms.copy()
    for k in range(9):      # under the identity pose: a pair at every integer distance 0 .. 8
        lat[1 + k] = t[0].fr.rec_atoms[10 + k] + f32([0.0, k, 0.0])
    f8 = Frame(t[0].fr.rec_atoms, lat, t[0].fr.center32, 3.0, 8.0)
    for lo in (0, 3):
        NB = 8 - lo
        out.append((f"integer edges {lo} .. 8", Case(f"pairpot lattice {lo}", f8, t[0].T),
                    PairPot(rng.integers(0, 3, f8.Ar), rng.integers(0, 3, f8.Al), np.arange(lo, 9).astype(f32), rng.uniform(-3.0, 3.0, (3, 3, NB)).astype(f32))))
    return tuple(out)


# ---- hydrogen bonds and salt bridges -------------------------------------------------------------------------------------------------------
HB_D, HB_A, HB_CAT, HB_AN, HB_SIDE = 1, 2, 4, 8, 16


def charged_residues(role, res, n_res):
    """compact [n_res]: the number of each residue with a cation or an anion among those, in residue order, or -1; and how many."""
    has = np.zeros(n_res, bool)
    has[np.asarray(res)[(np.asarray(role) & (HB_CAT | HB_AN)) != 0]] = True
    compact = np.where(has, np.cumsum(has) - 1, -1)
    return compact.astype(np.int64), int(has.sum())


class HBond:
    """The polar atoms of both chains (dicts: xyz, ante [n,3] float32, role [n] uint8, res [n] int32, n_res) as dfm_hbond_create leaves
    them: a frame whose reach is the larger cutoff and whose fourth components hold role | compact charged-residue index << 8, the
    antecedents sorted like their atoms, hb2 / salt2 = the cutoffs squared, c2 = min_cos2."""

    def __init__(self, rec, lig, center, hb_cutoff, c2, salt_cutoff, **frame):
        self.rec, self.lig = rec, lig
        h, sc = float(f32(hb_cutoff)), float(f32(salt_cutoff))
        self.hb2, self.salt2, self.c2 = h * h, sc * sc, float(c2)
        self.rc, self.Rc = charged_residues(rec["role"], rec["res"], rec["n_res"])
        self.lc, self.Lc = charged_residues(lig["role"], lig["res"], lig["n_res"])
        self.Wc = (self.Rc + 31) // 32
        bits = lambda ch, compact: (ch["role"].astype(np.int64) | np.where((ch["role"] & (HB_CAT | HB_AN)) != 0, compact[ch["res"]] << 8, 0)).astype(np.int32)
        self.fr = fr = Frame(rec["xyz"], lig["xyz"], center, 1.0, max(f32(hb_cutoff), f32(salt_cutoff)), rec_w=bits(rec, self.rc),
                             lig_w=bits(lig, self.lc), **frame)
        self.rec_ante4, self.lig_ante4 = np.zeros((fr.Ar, 4), f32), np.zeros((fr.Al, 4), f32)
        self.rec_ante4[:, :3], self.lig_ante4[:, :3] = np.asarray(rec["ante"], f32)[fr.order], np.asarray(lig["ante"], f32)[fr.lig_index]


def hbond_ref(hb, T, mutant=None):
    """launch_hbond + launch_hbond_finish on zeroed outputs by brute force over all pairs, in the kernel's operation order: tot [P,5] =
    bonds with 0, 1, 2 side-chain atoms, salt-bridge atom pairs, salt bridges; bits [P,Lc,Wc]; rec_hb / rec_sb [P,Nr], lig_hb / lig_sb
    [P,Nl] in the caller's order.  mutant 'angle_lt': du < 0 for du <= 0."""
    fr, T = hb.fr, f64(T)
    P = len(T)
    X, Y, Z = posed(fr, T)
    t, c = T[:, None, :], fr.center
    la, ra, r = f64(hb.lig_ante4), f64(hb.rec_ante4), f64(fr.rec4)
    rl, rr = fr.lig4[:, 3].view(np.int32).astype(np.int64), fr.rec4[:, 3].view(np.int32).astype(np.int64)
    with np.errstate(all="ignore"):
        qx, qy, qz = la[:, 0] - c[0], la[:, 1] - c[1], la[:, 2] - c[2]
        ux = (((qx * t[..., 0] + qy * t[..., 1]) + qz * t[..., 2]) + c[0] + t[..., 9]) - X
        uy = (((qx * t[..., 3] + qy * t[..., 4]) + qz * t[..., 5]) + c[1] + t[..., 10]) - Y
        uz = (((qx * t[..., 6] + qy * t[..., 7]) + qz * t[..., 8]) + c[2] + t[..., 11]) - Z
        uu = ((ux * ux + uy * uy) + uz * uz)[..., None]
        dx, dy, dz = r[:, 0] - X[..., None], r[:, 1] - Y[..., None], r[:, 2] - Z[..., None]
        r2 = (dx * dx + dy * dy) + dz * dz
        du = (ux[..., None] * dx + uy[..., None] * dy) + uz[..., None] * dz
        wx, wy, wz = ra[:, 0] - r[:, 0], ra[:, 1] - r[:, 1], ra[:, 2] - r[:, 2]
        ww = (wx * wx + wy * wy) + wz * wz
        dw = -((wx * dx + wy * dy) + wz * dz)
        neg = (lambda v: v < 0.0) if mutant == "angle_lt" else (lambda v: v <= 0.0)
        fin = finite_poses(T)[:, None, None]
        compl_ = (((rl & HB_D) != 0)[:, None] & ((rr & HB_A) != 0)[None, :]) | (((rl & HB_A) != 0)[:, None] & ((rr & HB_D) != 0)[None, :])
        ionic = (((rl & HB_CAT) != 0)[:, None] & ((rr & HB_AN) != 0)[None, :]) | (((rl & HB_AN) != 0)[:, None] & ((rr & HB_CAT) != 0)[None, :])
        salt = fin & ionic & (r2 < hb.salt2)
        bond = fin & compl_ & (r2 < hb.hb2) & neg(du) & (du * du >= hb.c2 * (uu * r2)) & neg(dw) & (dw * dw >= hb.c2 * (ww * r2))
    kind = ((rl >> 4) & 1)[:, None] + ((rr >> 4) & 1)[None, :]
    tot = np.stack([(bond & (kind == k)).sum((1, 2)) for k in range(3)] + [salt.sum((1, 2)), np.zeros(P, np.int64)], 1).astype(np.int32)
    bits = np.zeros((P, hb.Lc, hb.Wc), np.uint32)
    for p, a, b in zip(*np.where(salt)):
        i = int(rr[b] >> 8)
        bits[p, int(rl[a] >> 8), i >> 5] |= np.uint32(1 << (i & 31))
    tot[:, 4] = popcount(bits).reshape(P, -1).sum(1) if bits.size else 0
    out = dict(tot=tot, bits=bits, r2=r2, bond=bond, salt=salt, uu=uu)
    for name, m, axis, n, idx in (("rec_hb", bond, 1, fr.Ar, fr.order), ("rec_sb", salt, 1, fr.Ar, fr.order),
                                  ("lig_hb", bond, 2, fr.Al, fr.lig_index), ("lig_sb", salt, 2, fr.Al, fr.lig_index)):
        v = np.zeros((P, n), np.int32)
        v[:, idx] = m.sum(axis)
        out[name] = v
    return out


def check_hbond(out, ref, hb, status, base=None, rec_base=0, per_atom=True):
    want = ref["tot"].copy()
    if base is not None:
        want[:, :4] += np.asarray(base, np.int32)[:, :4]
    np.testing.assert_array_equal(out["tot"], want, "tot (bonds by side-chain atoms 0 / 1 / 2, salt-bridge atom pairs, salt bridges)")
    np.testing.assert_array_equal(out["bits"], ref["bits"], "the salt-bridge bitmap")
    if per_atom:
        w = walked_atoms(hb.fr, status)
        for k in ("lig_hb", "lig_sb"):
            np.testing.assert_array_equal(out[k], np.where(w, ref[k], MARKER), k)
        for k in ("rec_hb", "rec_sb"):
            np.testing.assert_array_equal(out[k], ref[k] + np.int32(rec_base), k)
    return 2 * ref["r2"].size


def polar_lump(rng, n, n_res, center, spread):
    """n polar atoms about `center` with all five role bits drawn (1 .. 31), antecedents 1.2 to 1.6 A away, every tenth antecedent ON its
    atom (uu = 0)."""
    xyz = lump(rng, n, center, spread)
    d = _unit(rng.standard_normal((n, 3)))
    ante = (xyz + d * rng.uniform(1.2, 1.6, (n, 1))).astype(f32)
    ante[::10] = xyz[::10]
    return dict(xyz=xyz, ante=ante, role=rng.integers(1, 32, n).astype(np.uint8), res=rng.integers(0, n_res, n).astype(np.int32), n_res=n_res)


@functools.lru_cache(maxsize=None)
def hbond_cases():
    """(name, HBond, T, rot, tr).  300 receptor and 130 ligand polar atoms with every role combination on both sides (donor and acceptor,
    cation and donor, ...), side-chain kinds 0, 1, 2, antecedents coincident with their atoms, at c2 = 0 and 0.97; the same without a
    charged residue in the receptor (Rc = 0), in the ligand (Lc = 0), with exactly 33 in the receptor (two words, the second of one bit);
    Nl = 1 and 65."""
    out = []
    rng = np.random.default_rng(51)
    rec, lig = polar_lump(rng, 300, 40, (0.0, 0.0, 0.0), 7.0), polar_lump(rng, 130, 20, (6.0, 0.0, 0.0), 4.0)
    cen = centre_of(lig["xyz"])
    rot, tr = touching_poses(rng, 6)
    tr[-1] = f32([60.0, -40.0, 10.0])
    T = pose_T(rot, tr)
    strip = lambda ch: dict(ch, role=(ch["role"] & ~np.uint8(HB_CAT | HB_AN)) | np.where((ch["role"] & 3) == 0, 1, 0).astype(np.uint8))
    r33 = dict(rec, res=(np.arange(300) % 40).astype(np.int32))
    r33["role"] = np.where(r33["res"] < 33, rec["role"] | np.uint8(HB_AN), rec["role"] & ~np.uint8(HB_CAT | HB_AN) | np.uint8(HB_A)).astype(np.uint8)
    l33 = dict(lig, role=(lig["role"] | np.uint8(HB_CAT)).astype(np.uint8))
    for name, r, l, c2 in (("c2 0", rec, lig, 0.0), ("c2 0.97", rec, lig, 0.97), ("Rc 0", strip(rec), lig, 0.25), ("Lc 0", rec, strip(lig), 0.25),
                           ("Rc 33", r33, l33, 0.0)):
        out.append((name, HBond(r, l, cen, 3.5, c2, 4.0), T, rot, tr))
    for n in (1, 65):
        l = polar_lump(rng, n, 5, (3.0, 0.0, 0.0), 3.0)
        out.append((f"Nl {n}", HBond(rec, l, centre_of(l["xyz"]), 3.5, 0.0, 5.5), T[:3], rot[:3], tr[:3]))
    return tuple(out)


# ---- buried surface ----------------------------------------------------------------------------------------------------------------------------
def sphere_dirs(K):
    """The default sphere points of dfm_surface_create: the golden spiral in float64, rounded to float32.  [K,3]"""
    k = np.arange(K, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / K
    r, phi = np.sqrt(1.0 - z * z), k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(f32)


def pack_bits(b):
    """bool [.., K] -> uint64 [.., K / 64]: bit l of word g = point 64 g + l."""
    return np.ascontiguousarray(np.packbits(b, axis=-1, bitorder="little")).view(np.uint64)


def unpack_bits(m, K):
    return np.unpackbits(np.ascontiguousarray(m).view(np.uint8), axis=-1, bitorder="little")[..., :K].astype(bool)


def exposure_ref(xyz, radius, probe, dirs):
    """Isolated exposure [n,K] bool as the definition takes it: point k of atom i, c_i + R_i u_k, is exposed when no other atom j of the
    chain has d < R_j, d = sqrt((dx*dx + dy*dy) + dz*dz) in float64."""
    x, R, u = f64(xyz), f64(radius) + probe, f64(dirs)
    out = np.ones((len(x), len(u)), bool)
    for i in range(len(x)):
        q = x[i] + R[i] * u      # [K,3]
        dx, dy, dz = q[:, None, 0] - x[:, 0], q[:, None, 1] - x[:, 1], q[:, None, 2] - x[:, 2]
        held = np.sqrt((dx * dx + dy * dy) + dz * dz) < R
        held[:, i] = False
        out[i] = ~held.any(1)
    return out


class Surface:
    """Atoms [n,3] and radii [n] float32 of both chains, K = 64 G sphere points and exposure masks [n,G] uint64 in the caller's atom order
    (the host's own, exposure_ref, or any the test likes: the kernel takes what it is given), as dfm_surface_create leaves them: radius
    classes = the distinct radii of both chains in ascending order, thr = (2 Rmax) 1.0001 + slack in float32 with maxabs over both
    chains + 4 Rmax + 1, the grid's edge = grow = thr, the radius as the fourth component."""

    def __init__(self, rec, rec_radius, lig, lig_radius, center, probe, K, rec_exp=None, lig_exp=None, dirs=None, **frame):
        rec_radius, lig_radius = np.ascontiguousarray(rec_radius, f32), np.ascontiguousarray(lig_radius, f32)
        self.rec_radius, self.lig_radius = rec_radius, lig_radius
        self.K, self.G, self.probe = K, K // 64, float(f32(probe))
        self.dirs = sphere_dirs(K) if dirs is None else np.ascontiguousarray(dirs, f32)
        self.values = np.unique(np.concatenate([rec_radius, lig_radius]))
        assert len(self.values) <= 16
        self.rec_class, self.lig_class = (np.searchsorted(self.values, r).astype(np.int32) for r in (rec_radius, lig_radius))
        Rmax = float(self.values[-1]) + self.probe
        maxabs = max(np.abs(f64(rec)).max(), np.abs(f64(lig)).max()) + 4.0 * Rmax + 1.0
        self.slack = max(f32(1e-3), f32(2.5e-7 * maxabs))
        self.thr = f32(f32(2.0 * Rmax) * f32(1.0001)) + self.slack
        self.rec_exp = pack_bits(exposure_ref(rec, rec_radius, self.probe, self.dirs)) if rec_exp is None else np.ascontiguousarray(rec_exp, np.uint64)
        self.lig_exp = pack_bits(exposure_ref(lig, lig_radius, self.probe, self.dirs)) if lig_exp is None else np.ascontiguousarray(lig_exp, np.uint64)
        self.fr = fr = Frame(rec, lig, center, 1.0, 2.0, edge=frame.pop("edge", float(self.thr)), rec_w=rec_radius.view(np.int32),
                             lig_w=lig_radius.view(np.int32), **frame)
        fr.grow, fr.thr = float(self.thr), self.thr


def surface_ref(sf, T, margin=1e-2):
    """launch_surface on zeroed outputs: rec_bur [P,Ar,G] (the frame's receptor order), lig_buried [P,Al], rec_buried [P,Ar] (the caller's
    order), class_points [P,2,16] (receptor, ligand).  Every pair of atoms whose centres are closer than R_a + R_b + margin (float64:
    no other pair can hold a point, by a hundredth of an A against roundings of 1e-12) and for it every point of both atoms, in the
    kernel's operation order; a buried point is an exposed one that an atom of the other chain holds (d < R, strict).  nearest: the
    smallest |d - R| met, in A."""
    fr, T, K, G = sf.fr, f64(T), sf.K, sf.G
    P = len(T)
    X, Y, Z = posed(fr, T)
    r = f64(fr.rec4)
    Rb, Ra = r[:, 3] + sf.probe, f64(fr.lig4[:, 3]) + sf.probe
    u = f64(sf.dirs)
    lexp, rexp = unpack_bits(sf.lig_exp[fr.lig_index], K), unpack_bits(sf.rec_exp[fr.order], K)
    lig_bur, rec_bur = np.zeros((P, fr.Al, K), bool), np.zeros((P, fr.Ar, K), bool)
    n_close, nearest = np.zeros((P, len(fr.sphere)), np.int64), np.inf
    for p in np.where(finite_poses(T))[0]:
        t = T[p]
        w = np.stack([(t[3 * k] * u[:, 0] + t[3 * k + 1] * u[:, 1]) + t[3 * k + 2] * u[:, 2] for k in range(3)], 1)      # [K,3]
        ex, ey, ez = X[p][:, None] - r[:, 0], Y[p][:, None] - r[:, 1], Z[p][:, None] - r[:, 2]
        lim = Ra[:, None] + Rb[None, :] + margin
        aa, bb = np.where((ex * ex + ey * ey) + ez * ez < lim * lim)
        np.add.at(n_close[p], aa // 64, 1)
        ax, ay, az = X[p][aa][:, None], Y[p][aa][:, None], Z[p][aa][:, None]
        bx, by, bz = r[bb, 0][:, None], r[bb, 1][:, None], r[bb, 2][:, None]
        ra, rb = Ra[aa][:, None], Rb[bb][:, None]
        dx, dy, dz = (ax + ra * w[:, 0]) - bx, (ay + ra * w[:, 1]) - by, (az + ra * w[:, 2]) - bz
        d = np.sqrt((dx * dx + dy * dy) + dz * dz)
        hit = d < rb
        nearest = min(nearest, float(np.abs(d - rb).min()) if d.size else np.inf)
        np.logical_or.at(lig_bur[p], aa, hit)
        dx, dy, dz = (bx + rb * u[:, 0]) - ax, (by + rb * u[:, 1]) - ay, (bz + rb * u[:, 2]) - az
        d = np.sqrt((dx * dx + dy * dy) + dz * dz)
        hit = d < ra
        nearest = min(nearest, float(np.abs(d - ra).min()) if d.size else np.inf)
        np.logical_or.at(rec_bur[p], bb, hit)
    lig_bur &= lexp
    rec_bur &= rexp
    lig_buried, rec_buried = np.zeros((P, fr.Al), np.int32), np.zeros((P, fr.Ar), np.int32)
    lig_buried[:, fr.lig_index], rec_buried[:, fr.order] = lig_bur.sum(2), rec_bur.sum(2)
    cp = np.zeros((P, 2, 16), np.int32)
    for c in range(16):
        cp[:, 0, c], cp[:, 1, c] = rec_buried[:, sf.rec_class == c].sum(1), lig_buried[:, sf.lig_class == c].sum(1)
    return dict(rec_bur=pack_bits(rec_bur).reshape(P, fr.Ar, G), lig_buried=lig_buried, rec_buried=rec_buried, class_points=cp, n_close=n_close,
                nearest=nearest, points=2 * P * fr.Al * fr.Ar * K)


def check_surface(out, ref, sf, status, base=None, per_atom=True):
    np.testing.assert_array_equal(out["rec_bur"], ref["rec_bur"], "rec_bur: the receptor's buried masks")
    want = ref["class_points"] if base is None else ref["class_points"] + np.asarray(base, np.int32).reshape(-1, 2, 16)
    np.testing.assert_array_equal(out["class_points"], want, "class_points")
    if per_atom:
        np.testing.assert_array_equal(out["rec_buried"], ref["rec_buried"], "rec_buried")
        np.testing.assert_array_equal(out["lig_buried"], np.where(walked_atoms(sf.fr, status), ref["lig_buried"], MARKER), "lig_buried")
    return ref["points"]


@functools.lru_cache(maxsize=None)
def surface_cases():
    """(name, Surface, T, rot, tr).  The generic complex with three radii at K = 128 and the host's own exposure (the case of the public
    call); K = 64, 128, 192, 256 (G = 1 .. 4) with sixteen radius classes and random exposure masks (rows of zeros and of ones among
    them); Ar = 1, 255, 256, 257 (one block of k_surface_finish, its last lane, two blocks); a dense clump whose first block has more
    than 1000 close pairs, so that the LDS queue of 512 drains several times mid-walk."""
    out = []
    rec, lig, cen, rot, tr = generic_atoms(0)
    T = pose_T(rot, tr)
    rng = np.random.default_rng(61)
    three = lambda n: rng.choice(f32([1.5, 1.7, 1.9]), n)
    out.append(("host exposure K 128", Surface(rec, three(300), lig, three(130), cen, 1.4, 128), T, rot, tr))
    sixteen = lambda n: (f32(1.2) + f32(0.05) * rng.integers(0, 16, n).astype(f32)).astype(f32)

    def masks(n, G):
        m = rng.integers(0, 1 << 63, (n, G), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, G), dtype=np.uint64)
        m[::7], m[3::7] = 0, np.uint64(0xffffffffffffffff)
        return m
    for K in (64, 128, 192, 256):
        rr, lr = sixteen(300), sixteen(130)
        rr[:16] = f32(1.2) + f32(0.05) * np.arange(16, dtype=f32)
        out.append((f"K {K} sixteen classes", Surface(rec, rr, lig, lr, cen, 1.4, K, masks(300, K // 64), masks(130, K // 64)), T, rot, tr))
    for Ar in (1, 255, 256, 257):
        r = lump(np.random.default_rng([62, Ar]), Ar, (0.0, 0.0, 0.0), 6.0)
        out.append((f"Ar {Ar}", Surface(r, three(Ar), lig, three(130), cen, 1.4, 64, masks(Ar, 1), masks(130, 1)), T[:3], rot[:3], tr[:3]))
    drng = np.random.default_rng(63)
    drec, dlig = lump(drng, 400, (0.0, 0.0, 0.0), 2.5), lump(drng, 70, (1.0, 0.0, 0.0), 1.5)
    drot, dtr = touching_poses(drng, 2, 0.3, 0.5)
    out.append(("dense clump", Surface(drec, three(400), dlig, three(70), centre_of(dlig), 1.4, 128, masks(400, 2), masks(70, 2)), pose_T(drot, dtr), drot, dtr))
    return tuple(out)


# =====================================================================================================================================
# k_density_pose / k_density: a gather, no cell walk
# =====================================================================================================================================
DENSITY_SHAPES = ((2, 2, 2), (3, 5, 4))      # [nz, ny, nx]
DENSITY_AL = (1, 63, 64, 65, 130)
DENSITY_N = (1, 2, 5)
DENSITY_MUTANTS = {      # name -> the comparison of density_compare that rejects it
    "le_upper": "n_inside", "trunc": "n_inside", "fx_f32": "atom_q", "y_before_x": "atom_q", "stride_swapped": "atom_q", "half_away": "atom_q",
    "contracted": "atom_q", "channel1_above": "n_above", "lanes_past_Al": "n_inside", "tot_stored": "sum_q"}


def density_case(shape, C, Al, seed=0, origin=(-3.0, 2.0, -5.0), voxel=(1.5, 1.0, 2.0), threshold=0.125, center=None, lig=None, w=None, grid4=None):
    """Inputs of one launch_density: a grid [nz][ny][nx] of float4 whose FOUR channels are all non-zero whatever C is (the launcher must not
    add the ones at or above C), anisotropic voxels, a negative origin, atoms from a quarter of the extent outside to a quarter beyond."""
    rng = np.random.default_rng([71, seed, C, Al] + list(shape))
    nz, ny, nx = shape
    o, v = f32(origin), f32(voxel)
    if grid4 is None:
        grid4 = rng.uniform(-4.0, 4.0, (nz, ny, nx, 4)).astype(f32)
    ext = v * (f32([nx, ny, nz]) - 1)
    if lig is None:
        lig = (o + ext * rng.uniform(-0.25, 1.25, (max(Al, 1), 3))).astype(f32)
    if w is None:
        w = rng.uniform(-8.0, 8.0, len(lig)).astype(f32)
    cen = f32(lig.mean(0) if center is None else center)
    geo = np.concatenate([f64(o), f64(v), f64(cen), [float(f32(threshold))], [nx - 1.0, ny - 1.0, nz - 1.0], np.zeros(3)])
    return dict(grid4=np.ascontiguousarray(grid4, f32), geo=geo, lig4=np.ascontiguousarray(np.concatenate([f32(lig), f32(w)[:, None]], 1), f32),
                dims=(nx, ny, nz), C=C, Al=Al, origin=o, voxel=v, center=cen, threshold=float(f32(threshold)))


def density_poses(dc, n, seed=0, s_rot=0.3, s_tr=0.2):
    """rot, tr [n,3] float32: rotations of about s_rot rad, translations of about s_tr times the grid's smallest extent."""
    rng = np.random.default_rng([72, seed, n])
    ext = float((f64(dc["voxel"]) * dc["geo"][10:13]).min())
    return (rng.standard_normal((n, 3)) * s_rot).astype(f32), (rng.standard_normal((n, 3)) * s_tr * ext).astype(f32)


def density_base(P, extra=2, seed=0):
    """What tot starts as: values of every size and sign, [P + extra][6]."""
    rng = np.random.default_rng([73, seed, P])
    return rng.integers(-(1 << 40), 1 << 40, (P + extra, 6)).astype(np.int64)


def _two_product_error(w, val):
    """The exact error of fl(w val) for w a widened fp32 number (Veltkamp split of val: both partial products are exact)."""
    p = w * val
    bits_ = np.ascontiguousarray(val, np.float64).view(np.uint64) & np.uint64(0xFFFFFFFFF8000000)
    hi = bits_.view(np.float64)
    lo = val - hi
    return (w * hi - p) + w * lo


def density_ref(grid, geo, lig4, T, C, mutant=None, base=None):
    """k_density restated in float64 numpy from T as twelve doubles, in the kernel's operation order and parenthesisation:
    ((qx t0 + qy t1) + qz t2) + c + t9, the division by the voxel, floor, the seven lerps of every channel, rint((w val) 2^20).  grid
    [nz][ny][nx][4] float32, geo [16], lig4 [Al][4].  Returns integers only: tot [P][6] (= base + the sums where a base is given; the
    channels at or above C are not added), atom_q [P][Al], inside [P][Al].  mutant: one of DENSITY_MUTANTS -
      le_upper        u <= n - 1 at the upper face (the corner index runs into the next row, as flat addressing does)
      trunc           the cell by truncation, the inside test on it: u in (-1, 0) lands in cell 0
      fx_f32          the fraction along x rounded to fp32
      y_before_x      the lerps along y before those along x
      stride_swapped  ny for nx in the row stride
      half_away       ties away from zero in the quantisation
      contracted      the product w val not rounded before the scale (decided by its exact error at a tie)
      channel1_above  n_above from channel 1
      lanes_past_Al   the idle lanes of the last block counted (they hold the last atom)
      tot_stored      tot stored, not added to."""
    grid = np.asarray(grid, f32)
    nz, ny, nx = grid.shape[:3]
    G = grid.reshape(-1, 4)
    geo, lig4, T = f64(geo), np.asarray(lig4, f32).reshape(-1, 4), f64(T).reshape(-1, 12)
    P, Al = len(T), len(lig4)
    t = T[:, None, :]
    with np.errstate(all="ignore"):
        fin = ~np.isnan((T * 0.0).sum(1))
        q3 = f64(lig4[:, :3]) - geo[6:9]
        qx, qy, qz = q3[None, :, 0], q3[None, :, 1], q3[None, :, 2]
        X = ((qx * t[..., 0] + qy * t[..., 1]) + qz * t[..., 2]) + geo[6] + t[..., 9]
        Y = ((qx * t[..., 3] + qy * t[..., 4]) + qz * t[..., 5]) + geo[7] + t[..., 10]
        Z = ((qx * t[..., 6] + qy * t[..., 7]) + qz * t[..., 8]) + geo[8] + t[..., 11]
        u = np.stack([(X - geo[0]) / geo[3], (Y - geo[1]) / geo[4], (Z - geo[2]) / geo[5]], -1)      # [P][Al][3]
        n1 = geo[10:13]
        if mutant == "trunc":
            cell = np.trunc(u)
            inside = ((cell >= 0.0) & (cell <= n1 - 1.0)).all(-1)
        elif mutant == "le_upper":
            inside = ((u >= 0.0) & (u <= n1)).all(-1)
        else:
            inside = ((u >= 0.0) & (u < n1)).all(-1)
        inside &= fin[:, None]
        um = np.where(inside[..., None], u, 0.0)
        fl = np.trunc(um) if mutant == "trunc" else np.floor(um)
        f = um - fl
        fx, fy, fz = f[..., 0, None], f[..., 1, None], f[..., 2, None]
        if mutant == "fx_f32":
            fx = f64(fx.astype(f32))
        ix, iy, iz = (fl[..., k].astype(np.int64) for k in range(3))
        row, slab = (ny if mutant == "stride_swapped" else nx), nx * ny
        first = (iz * ny + iy) * row + ix
        c = lambda dz, dy, dx: f64(G[(first + dx + dy * row + dz * slab) % len(G)])      # [P][Al][4]; the wrap is reached by mutants only
        c000, c100, c010, c110, c001, c101, c011, c111 = c(0, 0, 0), c(0, 0, 1), c(0, 1, 0), c(0, 1, 1), c(1, 0, 0), c(1, 0, 1), c(1, 1, 0), c(1, 1, 1)
        if mutant == "y_before_x":
            a00, a10 = c000 + fy * (c010 - c000), c100 + fy * (c110 - c100)
            a01, a11 = c001 + fy * (c011 - c001), c101 + fy * (c111 - c101)
            c0, c1 = a00 + fx * (a10 - a00), a01 + fx * (a11 - a01)
        else:
            c00, c10 = c000 + fx * (c100 - c000), c010 + fx * (c110 - c010)
            c01, c11 = c001 + fx * (c101 - c001), c011 + fx * (c111 - c011)
            c0, c1 = c00 + fy * (c10 - c00), c01 + fy * (c11 - c01)
        val = c0 + fz * (c1 - c0)
        w = f64(lig4[:, 3])[None, :, None]
        s = (w * val) * QUANTA
        r = np.rint(s)
        if mutant == "half_away":
            r = np.sign(s) * np.floor(np.abs(s) + 0.5)
        elif mutant == "contracted":
            err = _two_product_error(np.broadcast_to(w, val.shape), val)
            tie = (s - np.floor(s)) == 0.5
            r = np.where(tie & (err != 0.0), np.floor(s) + (err > 0.0), r)
        q = np.where(inside[..., None], r, 0.0).astype(np.int64)
        above = inside & (val[..., 1 if mutant == "channel1_above" else 0] >= geo[9])
    tot = np.zeros((P, 6), np.int64)
    tot[:, :4], tot[:, 4], tot[:, 5] = q.sum(1), inside.sum(1), above.sum(1)
    if mutant == "lanes_past_Al":
        pad = (-Al) % 64
        tot[:, :4] += pad * q[:, -1]
        tot[:, 4] += pad * inside[:, -1]
        tot[:, 5] += pad * above[:, -1]
    tot[:, C:4] = 0
    if base is not None:
        b = np.asarray(base, np.int64)[:P]
        if mutant == "tot_stored":
            written = np.zeros((P, 6), bool)
            written[:, :C], written[:, 4], written[:, 5] = True, True, tot[:, 5] != 0
            written &= inside.any(1)[:, None]
            tot = np.where(written, tot, b)
        else:
            tot = b + tot
    return dict(tot=tot, atom_q=q[..., 0].copy(), inside=inside)


def density_compare(out, ref, P, Al, base=None, atom_q=True):
    """Every comparison of one launch against density_ref (which holds the base already), as numbers of mismatches: sum_q, n_inside,
    n_above, atom_q, `past` (a total past pose P that is not the base any more, an atom_q entry past [P][Al] that is not the marker)."""
    tot = np.asarray(out["tot"]).reshape(-1, 6)
    cmp = {"sum_q": int((tot[:P, :4] != ref["tot"][:, :4]).sum()), "n_inside": int((tot[:P, 4] != ref["tot"][:, 4]).sum()),
           "n_above": int((tot[:P, 5] != ref["tot"][:, 5]).sum()), "past": 0}
    if len(tot) > P:
        cmp["past"] += int((tot[P:] != (0 if base is None else np.asarray(base, np.int64)[P:])).sum())
    if atom_q:
        aq = np.asarray(out["atom_q"]).reshape(-1)
        cmp["atom_q"] = int((aq[:P * Al] != ref["atom_q"].reshape(-1)).sum())
        cmp["past"] += int((aq[P * Al:] != MARKER).sum())
    return cmp


def density_definition(dc, rot, tr):
    """dfmdock_amd.density.density on the case's first C channels: the package's definition."""
    from dfmdock_amd import density as DN
    grids = np.ascontiguousarray(np.moveaxis(dc["grid4"][..., :dc["C"]], -1, 0))
    return DN.density(grids, dc["origin"], dc["voxel"], dc["lig4"][:, :3], dc["lig4"][:, 3], dc["center"], rot, tr, dc["threshold"], per_atom=True)


@functools.lru_cache(maxsize=None)
def density_launches(shape, C):
    """[(dc, rot, tr, T, base)] of test_density_exact for one grid and one C: every Al of DENSITY_AL with every n of DENSITY_N."""
    out = []
    for Al in DENSITY_AL:
        dc = density_case(shape, C, Al)
        for n in DENSITY_N:
            rot, tr = density_poses(dc, n, seed=Al)
            out.append((dc, rot, tr, pose_T(rot, tr), density_base(n, seed=Al)))
    return tuple(out)


QUARTER_TURNS = {"identity": ((1, 0, 0), (0, 1, 0), (0, 0, 1)), "x90": ((1, 0, 0), (0, 0, -1), (0, 1, 0)), "y90": ((0, 0, 1), (0, 1, 0), (-1, 0, 0)),
                 "z90": ((0, -1, 0), (1, 0, 0), (0, 0, 1))}
PLANTED_TR = ((0.0, 0.0, 0.0), (0.25, -0.5, 0.125), (-0.125, 0.25, 0.5), (0.5, 0.125, -0.5))
PLANTED_KINDS = ("node", "lower", "upper", "neg_half", "far")      # and "<face>+" / "<face>-": one fp32 ulp up / down along the face's axis


@functools.lru_cache(maxsize=None)
def planted_density_case():
    """(dc, T [4][12], labels) with T of EXACT doubles - the identity and the quarter turns about x, y, z (entries 0, +-1), translations that
    are small binary fractions - on a grid whose origin and voxels are binary fractions too (voxels 0.5, 1, 2: the division is exact), so
    every X and u is exact.  For every pose p the atoms x = R^T (Y - t) whose images Y are: nodes (corners of the grid among them), a
    point on each of the six faces, and that atom moved by one fp32 ulp either way along the axis the face's normal comes from; a point
    with u = -1/2 on each axis; and, once, atoms at 1e30 and 3e38.  labels [Al] = (pose, kind).  Every atom is seen by all four poses."""
    shape, o, v = (3, 5, 4), np.array([-1.75, 2.0, -4.25]), np.array([0.5, 1.0, 2.0])      # (no face at 0: an ulp of 0 is a denormal)
    n1 = np.array([shape[2], shape[1], shape[0]], np.float64) - 1
    mid = o + 0.75 * v
    atoms, labels, T = [], [], []
    for p, (name, R) in enumerate(QUARTER_TURNS.items()):
        R, t = np.array(R, np.float64), np.array(PLANTED_TR[p])
        T.append(np.concatenate([R.reshape(-1), t]))
        pre = lambda Y: R.T @ (np.asarray(Y, np.float64) - t)

        def add(x, kind):
            assert (f64(f32(x)) == x).all(), (name, kind, x)      # the atom is an fp32 number
            atoms.append(f32(x))
            labels.append((p, kind))
        for node in ((0, 0, 0), (1, 1, 1), (2, 3, 1), (3, 0, 0), (0, 4, 0), (0, 0, 2), (3, 4, 2), (2, 3, 0)):
            add(pre(o + np.array(node) * v), "node")
        for k in range(3):
            j = int(np.nonzero(R[k])[0][0])      # the atom coordinate that moves X_k
            for kind, uk in (("lower", 0.0), ("upper", n1[k])):
                Yp = mid.copy()
                Yp[k] = o[k] + uk * v[k]
                x = pre(Yp)
                add(x, kind)
                for sgn, far in (("+", np.inf), ("-", -np.inf)):
                    xs = f32(x)
                    xs[j] = np.nextafter(xs[j], f32(far))
                    add(f64(xs), kind + sgn)
            Yp = mid.copy()
            Yp[k] = o[k] - 0.5 * v[k]
            add(pre(Yp), "neg_half")
    for far in ((1e30, 0.0, 0.0), (0.0, -3e38, 0.0), (0.0, 0.0, 3e38)):
        add(f64(f32(far)), "far")
    lig = np.asarray(atoms, f32)
    w = np.random.default_rng(74).uniform(1.0, 8.0, len(lig)).astype(f32)
    dc = density_case(shape, 2, len(lig), seed=5, origin=o, voxel=v, center=(0.0, 0.0, 0.0), lig=lig, w=w)
    return dc, np.asarray(T), tuple(labels)


def density_inside_exact(dc, T):
    """The inside decision of every (pose, atom) in exact rational arithmetic: X = R (x - c) + c + t, 0 <= (X - o) / v < n - 1."""
    geo, lig = dc["geo"], dc["lig4"]
    F = lambda a: Fraction(float(a))
    out = np.zeros((len(T), len(lig)), bool)
    for p, tp in enumerate(T):
        for a, x in enumerate(lig):
            q = [F(x[k]) - F(geo[6 + k]) for k in range(3)]
            ok = True
            for k in range(3):
                Xk = sum(q[j] * F(tp[3 * k + j]) for j in range(3)) + F(geo[6 + k]) + F(tp[9 + k])
                uk = (Xk - F(geo[k])) / F(geo[3 + k])
                ok = ok and 0 <= uk < F(geo[10 + k])
            out[p, a] = ok
    return out


def minus_zero_density_case():
    """(dc, T): u_x = -0.0.  The atom sits on the x = 0 face of a grid whose origin is 0 there, the pose shifts it by -2^-1000 and the voxel
    is 2^100 wide along x: the quotient -2^-1100 is below half the smallest denormal and rounds to -0.0, which is >= 0: inside, cell 0,
    fraction 0 (the IEEE operations are the definition; the exact quotient would be outside)."""
    dc = density_case((2, 2, 2), 1, 1, seed=6, origin=(0.0, 0.0, 0.0), voxel=(2.0 ** 100, 1.0, 1.0), center=(0.0, 0.0, 0.0),
                      lig=f32([[0.0, 0.25, 0.5]]), w=f32([3.0]))
    T = np.concatenate([np.eye(3).reshape(-1), [-2.0 ** -1000, 0.0, 0.0]])[None]
    return dc, T


def ties_density_case():
    """(half, rounded, T): quantisation ties.
    half     a grid that is 2^-21 on every node, weights 1, 3, 5, -1, -5: (w val) 2^20 = w / 2 exactly; ties to even give 0, 2, 2, -0, -2.
    rounded  ties that exist only once a product is rounded.  Channel 0 is -1, 1 on the nodes (x = 0, 1) of the row y = 0 and 0, 2 on those
             of y = 1, the same in both z planes; the atoms sit at fx = 1/2, so the lerps along x give 0 and 1 exactly and val = fy =
             fl(y / 3) (a voxel of 3 along y) with y = (k + 1/2) 2^-20, k = 2 .. 9, and w = 3: fl(3 fl(y / 3)) = y exactly, a tie, although
             3 fl(y / 3) != y.  Lerps along y first round -1 + fy and 1 + fy at 2^-53: no tie is left, and half of them fall the other way."""
    flat = np.full((2, 2, 2, 4), 2.0 ** -21, f32)
    half = density_case((2, 2, 2), 1, 5, seed=7, origin=(0.0, 0.0, 0.0), voxel=(1.0, 1.0, 1.0), center=(0.0, 0.0, 0.0),
                        lig=f32([[0.25, 0.5, 0.75], [0.5, 0.5, 0.5], [0.125, 0.25, 0.5], [0.75, 0.25, 0.5], [0.5, 0.75, 0.25]]),
                        w=f32([1, 3, 5, -1, -5]), grid4=flat)
    g = np.zeros((2, 2, 2, 4), f32)
    g[:, 0, :, 0], g[:, 1, :, 0] = (-1.0, 1.0), (0.0, 2.0)
    g[..., 1] = f32(2.0 ** -21)
    lig = f32([[0.5, (k + 0.5) * 2.0 ** -20, 0.5] for k in range(2, 10)])
    rounded = density_case((2, 2, 2), 1, len(lig), seed=8, origin=(0.0, 0.0, 0.0), voxel=(1.0, 3.0, 1.0), center=(0.0, 0.0, 0.0), lig=lig,
                           w=np.full(len(lig), 3.0, f32), grid4=g)
    T = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])[None]
    return half, rounded, T


def nonfinite_density_T(T0, T1):
    """[38][12]: T0, then T0 with NaN, +inf, -inf in each of its twelve slots, then T1."""
    out = np.tile(f64(T0), (38, 1))
    for k in range(12):
        for j, v in enumerate((np.nan, np.inf, -np.inf)):
            out[1 + 3 * k + j, k] = v
    out[37] = T1
    return out


def limit_density_case():
    """The launcher's largest n: 65535 poses of one atom on a 2 x 2 x 2 grid, pure translations about its centre, a share of them
    outside."""
    dc = density_case((2, 2, 2), 3, 1, seed=9, lig=f32([[-2.25, 2.5, -4.0]]), w=f32([5.5]))
    rng = np.random.default_rng(75)
    T = np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]), (65535, 1))
    T[:, 9:] = rng.uniform(-1.0, 1.0, (65535, 3)) * f64(dc["voxel"]) * 0.7
    return dc, T


def sum_limit_density_case():
    """Values of 2^10 on every node and weights of +-2^7 across 130 atoms: terms of exactly +-2^37 (the largest check_density_grid and
    check_density_atoms admit), every tenth atom's negative; channel 1 holds -2^10."""
    g = np.full((2, 2, 2, 4), 1024.0, f32)
    g[..., 1] = -1024.0
    rng = np.random.default_rng(76)
    lig = rng.uniform(1.0, 15.0, (130, 3)).astype(f32)
    w = np.where(np.arange(130) % 10 == 3, -128.0, 128.0).astype(f32)
    dc = density_case((2, 2, 2), 2, 130, seed=10, origin=(0.0, 0.0, 0.0), voxel=(16.0, 16.0, 16.0), threshold=1024.0, center=(8.0, 8.0, 8.0),
                      lig=lig, w=w, grid4=g)
    T = np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]), (2, 1))
    T[1, 9:] = (0.5, -0.25, 0.125)
    return dc, T
