"""Numpy-level wrapper over the C ABI: Model / Complex handles, batched score and sample calls."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .weights import HParams


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a, t=L.F32P):
    return a.ctypes.data_as(t) if a is not None else None


PRECISIONS = ("mfma16", "f16", "fp32")
_warned_bf16 = False


def precision_kwargs(precision: str) -> dict:
    """Engine selector -> keyword arguments of Complex.score / Complex.sample.

      "mfma16"  the 16-bit MFMA engine as shipped (DFM_F_MFMA16): fp16 MFMA operands, fp32 accumulation (config_string())
      "f16"     the same with fp32 A_i (DFM_F_F16)
      "fp32"    exact fp32 (the reference's own arithmetic)
      "bf16"    DEPRECATED alias of "mfma16" - the name of rounds 1-3, kept so that old command lines keep working; the
                engine it selects has computed on fp16 operands since r03, which is what the name now says
    """
    global _warned_bf16
    if precision == "bf16":
        if not _warned_bf16:
            import sys
            print('dfmdock_amd: precision "bf16" is a deprecated alias of "mfma16" (fp16 MFMA operands, fp32 accumulation)', file=sys.stderr)
            _warned_bf16 = True
        precision = "mfma16"
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS} (or the deprecated alias 'bf16'), got {precision!r}")
    return {"mfma16": precision == "mfma16", "f16": precision == "f16"}


def canonical_precision(precision: str) -> str:
    return "mfma16" if precision == "bf16" else precision


def hparams_c(hp: HParams | None = None) -> L.HParamsC:
    hp = hp or HParams()
    return L.HParamsC(**hp.as_dict())


def set_device(index: int = 0):
    L.check(L.lib().dfm_set_device(int(index)), "dfm_set_device")


def config_string() -> str:
    """The precision plan and every diagnostic switch in force in this process (dfm_config_string)."""
    return L.lib().dfm_config_string().decode()


def trim_cache(device: int = -1) -> int:
    """Hand the device blocks parked by destroyed handles back to the driver (dfm_trim_cache); returns the bytes freed."""
    return int(L.lib().dfm_trim_cache(int(device)))


def alloc_diag() -> dict:
    """What the allocator diagnostics DFM_ALLOC_POISON / DFM_ALLOC_GUARD did in this process (dfm_alloc_diag): {blocks, poisoned_bytes,
    bands_checked, bands_damaged, first_damaged_size, first_damaged_offset (both -1 while every band is intact)}."""
    n = (C.c_int64 * 6)()
    L.check(L.lib().dfm_alloc_diag(n), "dfm_alloc_diag")
    return dict(zip(("blocks", "poisoned_bytes", "bands_checked", "bands_damaged", "first_damaged_size", "first_damaged_offset"),
                    (int(v) for v in n)))


def device_count() -> int:
    n = C.c_int(0)
    rc = L.lib().dfm_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def diffusion_coef(which: int, t: float, hp: HParams | None = None):
    """(g, sigma) of the R^3 (which=0) or SO(3) (which=1) VE-SDE, float64 like the reference."""
    h = hparams_c(hp)
    g, s = C.c_double(0), C.c_double(0)
    L.check(L.lib().dfm_diffusion_coef(C.byref(h), int(which), float(t), C.byref(g), C.byref(s)), "diffusion_coef")
    return g.value, s.value


def format_selfcheck(r: dict, name: str = "") -> str:
    """One line for logs: what a checkpoint owner reads before trusting the 16-bit engine."""
    worst = {k: max(r[k]) for k in ("max_A", "max_Bm", "max_sum16", "max_pre", "max_acc")}
    top = max(worst, key=worst.get)
    return (f"selfcheck {name}: {r['precision']} vs fp32 on {r['n_eval']} graphs: f {r['dev_f']:.2e} tr {r['dev_tr_score']:.2e} "
            f"rot {r['dev_rot_score']:.2e} E {r['dev_energy']:.2e} (gates {r['gate_f']:.0e} / {r['gate_score']:.0e} / {r['gate_energy']:.0e}; "
            f"cancellation tr {r['cancel_ratio'][0]:.3f} rot {r['cancel_ratio'][1]:.3f}, pooled-vector bounds {r['score_bound'][0]:.1e} / "
            f"{r['score_bound'][1]:.1e}) | fp16 range: max|h| {max(r['max_h']):.3g}, largest stored magnitude {worst[top]:.3g} ({top[4:]}), "
            f"headroom x{r['headroom']:.3g}, saturated {r['saturated']} | {'OK' if r['ok'] else 'FAILED: ' + ('range ' if not r['range_ok'] else '') + ('deviation' if not r['dev_ok'] else '')}")


class Model:
    """Device-resident weights (dfm_model).  `blob` is the flat float32 state_dict (weights.pack_blob)."""

    def __init__(self, blob, hp: HParams | None = None):
        self.hp = hp or HParams()
        self._hp_c = hparams_c(self.hp)
        blob = _f32(blob).reshape(-1)
        self._h = L.lib().dfm_model_create(_p(blob), blob.size, C.byref(self._hp_c))
        if not self._h:
            L.check(-1 if b"blob" in L.lib().dfm_last_error() or b"unsupported" in L.lib().dfm_last_error() else -2,
                    "dfm_model_create")

    def close(self):
        if getattr(self, "_h", None):
            L.lib().dfm_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


    # ------------------------------------------------------------------
    def _poses(self, lig_pos, residues):
        lp = _f32(lig_pos)
        if lp.ndim == 4:
            lp = lp.reshape(lp.shape[0], lp.shape[1], 9)
        if lp.ndim != 3 or lp.shape[2] != 9:
            raise ValueError(f"lig_pos must be [B,L,9] or [B,L,3,3], got {np.shape(lig_pos)}")
        res = None if residues is None else np.ascontiguousarray(np.asarray(residues).reshape(-1), dtype=np.int32)
        return lp, res, 0 if res is None else res.size

    def pose_rmsd(self, lig_pos, residues=None):
        """[B,B] float32 pairwise ligand RMSD without superposition over the backbone atoms of `residues` (None: all) on the GPU
        (dfm_pose_rmsd; the float64 definition is cluster.pose_rmsd)."""
        lp, res, n_res = self._poses(lig_pos, residues)
        B, Lg = lp.shape[0], lp.shape[1]
        out = np.empty((B, B), np.float32)
        L.check(L.lib().dfm_pose_rmsd(self._h, B, Lg, _p(lp), _p(res, L.I32P), n_res, _p(out)), "dfm_pose_rmsd")
        return out

    def pose_cluster(self, lig_pos, radius, key=None, rule="energy", max_clusters=None, residues=None):
        """Cluster B poses on the GPU (dfm_pose_cluster; the definition is cluster.cluster_poses): neighbours within `radius` A ligand
        RMSD, `key` [B] lower = better (None: index order), rule "energy" (leader) or "size" (greedy), at most `max_clusters` (None: B).
        Returns {n_clusters, center, size, cluster_of} as int32 arrays."""
        from .cluster import RULES
        if rule not in RULES:
            raise ValueError(f"rule must be one of {RULES}, got {rule!r}")
        lp, res, n_res = self._poses(lig_pos, residues)
        B, Lg = lp.shape[0], lp.shape[1]
        maxc = B if max_clusters is None else int(max_clusters)
        k = None if key is None else _f32(key).reshape(-1)
        if k is not None and k.size != B:
            raise ValueError(f"key must have {B} entries")
        n = C.c_int32(0)
        cap = max(1, min(maxc, B))
        center, size, cluster_of = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(B, np.int32)
        rc = L.lib().dfm_pose_cluster(self._h, B, Lg, _p(lp), _p(res, L.I32P), n_res, _p(k), float(radius), RULES.index(rule), maxc,
                                      C.byref(n), _p(center, L.I32P), _p(size, L.I32P), _p(cluster_of, L.I32P))
        L.check(rc, "dfm_pose_cluster")
        return {"n_clusters": int(n.value), "center": center[: n.value].copy(), "size": size[: n.value].copy(), "cluster_of": cluster_of}


    def igso3_table(self, t):
        """The IGSO(3) table `refine` looks rotation angles up in at time t (dfm_igso3_table; definition: refine.sigma_index /
        refine.igso3_cdf): {sigma_idx, sigma, cdf [1000] float64}, computed on the GPU once per sigma index."""
        idx, sg = C.c_int(0), C.c_double(0)
        cdf = np.zeros(1000, np.float64)
        L.check(L.lib().dfm_igso3_table(self._h, float(t), C.byref(idx), C.byref(sg), cdf.ctypes.data_as(C.POINTER(C.c_double))),
                "dfm_igso3_table")
        return {"sigma_idx": idx.value, "sigma": sg.value, "cdf": cdf}


    def native(self, rec_pos, lig_pos, iface_cutoff=10.0, contact_cutoff=5.5):
        """The native pose (receptor [R,3,3], ligand [L,3,3]) prepared for batched docking metrics on the GPU (dfm_native_create):
        a Native whose `.metrics(lig_pos[, rec_pos])` evaluates P poses in one call.  The cutoffs are the reference's."""
        return Native(self, rec_pos, lig_pos, iface_cutoff, contact_cutoff)

    def consensus(self, rec_pos, lig_pos, cutoff=5.5, members=None, bits=False):
        """Consensus contact scoring of P poses on the GPU (dfm_pose_consensus; the float64 definition is consensus.consensus): rec_pos
        [R,3,3], lig_pos [P,L,3,3], `members` bool [P] (None: every pose).  Returns {count [R,L], rec_count [R], lig_count [L], n_contacts
        [P] (int32), score_sum [P] (int64), M, cutoff, freq = count / M, consensus [P] = score_sum / (M n_contacts), NaN without a
        contact (consensus.finish)} and, with `bits`, the contacts themselves as uint64 [P,R,ceil(L/64)] (consensus.unpack_bits)."""
        from . import consensus as CS
        rp = _f32(rec_pos).reshape(-1, 9)
        lp = _f32(lig_pos)
        if lp.ndim == 4:
            lp = lp.reshape(lp.shape[0], lp.shape[1], 9)
        if lp.ndim != 3 or lp.shape[2] != 9:
            raise ValueError(f"lig_pos must be [P,L,9] or [P,L,3,3], got {np.shape(lig_pos)}")
        P, Lg, R = lp.shape[0], lp.shape[1], rp.shape[0]
        mem = None
        if members is not None:
            mem = np.ascontiguousarray(np.asarray(members).reshape(-1).astype(bool), dtype=np.uint8)
            if mem.size != P:
                raise ValueError(f"members must have {P} entries, got {mem.size}")
        o = {"count": np.zeros((R, Lg), np.int32), "rec_count": np.zeros(R, np.int32), "lig_count": np.zeros(Lg, np.int32),
             "n_contacts": np.zeros(P, np.int32), "score_sum": np.zeros(P, np.int64)}
        out = L.ConsensusOutC()
        out.count, out.rec_count, out.lig_count, out.n_contacts = (_p(o[k], L.I32P) for k in ("count", "rec_count", "lig_count", "n_contacts"))
        out.score_sum = o["score_sum"].ctypes.data_as(C.POINTER(C.c_int64))
        if bits:
            o["bits"] = np.zeros((P, R, (Lg + 63) // 64), np.uint64)
            out.bits = o["bits"].ctypes.data_as(C.POINTER(C.c_uint64))
        L.check(L.lib().dfm_pose_consensus(self._h, P, R, Lg, _p(rp), _p(lp), _p(mem, C.POINTER(C.c_uint8)), float(cutoff), C.byref(out)),
                "dfm_pose_consensus")
        o["M"] = P if mem is None else int(mem.sum())
        o["cutoff"] = float(np.float32(cutoff))
        o["freq"] = o["count"].astype(np.float64) / o["M"]
        o["consensus"] = CS.finish(o["score_sum"], o["n_contacts"], o["M"])
        return o

    def pose_fit(self, lig_ref, lig_pos, center, rec_ref=None, rec_pos=None, chunk_poses=0):
        """Rigid pose fit of P decoys on the GPU (dfm_pose_fit; the float64 definition is fit.fit_poses): lig_ref [L,3,3] the input
        ligand, lig_pos [P,L,3,3] the decoys' ligands, center [3] the sampler's rotation centre; rec_ref [R,3,3] and rec_pos [P,R,3,3],
        both or neither, for decoys in a frame of their own.  Returns {rot [P,3], tr [P,3] float32 - the sampler's (rot_update,
        tr_update) -, rmsd [P] float64 and rec_rmsd [P] float64 or None}."""
        lr = _f32(lig_ref).reshape(-1, 9)
        Lg = lr.shape[0]
        lp = _f32(lig_pos)
        if Lg < 1 or lp.size == 0 or lp.size % (Lg * 9):
            raise ValueError(f"lig_pos must be [P,{Lg},3,3] with P >= 1, got {np.shape(lig_pos)}")
        P = lp.size // (Lg * 9)
        if (rec_ref is None) != (rec_pos is None):
            raise ValueError("rec_ref and rec_pos must be given together")
        rr = rp = None
        R = 0
        if rec_ref is not None:
            rr, rp = _f32(rec_ref).reshape(-1, 9), _f32(rec_pos)
            R = rr.shape[0]
            if R < 1 or rp.size != P * R * 9:
                raise ValueError(f"rec_pos must be [{P},{R},3,3], got {np.shape(rec_pos)}")
        cen = _center(center)
        o = {"rot": np.zeros((P, 3), np.float32), "tr": np.zeros((P, 3), np.float32), "rmsd": np.zeros(P, np.float64),
             "rec_rmsd": None if rr is None else np.zeros(P, np.float64)}
        out = L.FitOutC()
        dp = C.POINTER(C.c_double)
        out.rot, out.tr, out.rmsd = _p(o["rot"]), _p(o["tr"]), o["rmsd"].ctypes.data_as(dp)
        if rr is not None:
            out.rec_rmsd_or_null = o["rec_rmsd"].ctypes.data_as(dp)
        L.check(L.lib().dfm_pose_fit_chunked(self._h, P, Lg, _p(lr), _p(lp), R, _p(rr), _p(rp), _p(cen), int(chunk_poses), C.byref(out)),
                "dfm_pose_fit")
        return o

    def atoms(self, rec_atoms, lig_atoms, center, clash_cutoff=3.0, contact_cutoff=5.0):
        """The heavy atoms of a pair prepared for the all-atom clash / contact screen on the GPU (dfm_atoms_create): rec_atoms [Ar,3],
        lig_atoms [Al,3], center [3] = the point the sampler's (rot, tr) rotate the ligand about.  Returns an Atoms whose
        `.sterics(rot, tr)` screens P poses in one call."""
        return Atoms(self, rec_atoms, lig_atoms, center, clash_cutoff, contact_cutoff)

    def surface(self, rec_atoms, rec_radius, lig_atoms, lig_radius, center, probe=1.4, points=128):
        """The heavy atoms of a pair and their van der Waals radii prepared for the buried-surface-area call on the GPU
        (dfm_surface_create): `points` sphere points per atom (surface.sphere_points), a probe of `probe` A.  Returns a Surface whose
        `.bsa(rot, tr)` takes P poses in one call."""
        return Surface(self, rec_atoms, rec_radius, lig_atoms, lig_radius, center, probe, points)

    def interface(self, rec_atoms, rec_params, lig_atoms, lig_params, center, cutoff=8.0, soft=0.6, elec_min_dist=3.0, dielectric_slope=4.0):
        """The heavy atoms of a pair and their (rmin_half, sqrt_eps, charge) rows ([n,3], ifenergy.atom_parameters) prepared for the
        interface-energy call on the GPU (dfm_iface_create): soft Lennard-Jones plus Coulomb with eps = dielectric_slope r over the pairs
        within `cutoff` A.  Returns an Interface whose `.energy(rot, tr)` takes P poses in one call."""
        return Interface(self, rec_atoms, rec_params, lig_atoms, lig_params, center, cutoff, soft, elec_min_dist, dielectric_slope)

    def contacts(self, rec_atoms, rec_res, rec_class, lig_atoms, lig_res, lig_class, center, cutoff=5.5):
        """The heavy atoms of a pair with the residue index of every atom ([n] in [0, n_res)) and the class of every residue ([n_res]: 0
        apolar, 1 polar, 2 charged; affinity.residue_classes) prepared for the residue-contact call on the GPU (dfm_rescon_create):
        residue pairs with two heavy atoms closer than `cutoff` A.  Returns a Contacts whose `.count(rot, tr)` takes P poses in one call."""
        return Contacts(self, rec_atoms, rec_res, rec_class, lig_atoms, lig_res, lig_class, center, cutoff)

    def hbonds(self, rec, lig, center, hb_cutoff=3.5, min_angle=90.0, salt_cutoff=4.0):
        """The polar atoms of a pair (rec, lig: the dicts of hbonds.polar_atoms - xyz, ante, role, res, n_res) prepared for the hydrogen-bond
        and salt-bridge call on the GPU (dfm_hbond_create): heavy-atom criteria, a distance below `hb_cutoff` A and both antecedent angles
        at least `min_angle` degrees; cation / anion pairs below `salt_cutoff` A.  Returns an HBonds whose `.count(rot, tr)` takes P poses
        in one call."""
        return HBonds(self, rec, lig, center, hb_cutoff, min_angle, salt_cutoff)

    def pairpot(self, rec_atoms, rec_type, lig_atoms, lig_type, center, edges, table):
        """The heavy atoms of a pair with the type of every atom ([n] in [0, T); pairpot.atom_types) and a tabulated pair potential -
        edges [NB+1] in A, table [T,T,NB] in kcal/mol indexed (ligand type, receptor type, bin); pairpot.load reads both from a file -
        prepared for the pair-potential call on the GPU (dfm_pairpot_create).  The project ships no table.  Returns a PairPotential
        whose `.energy(rot, tr)` takes P poses in one call."""
        return PairPotential(self, rec_atoms, rec_type, lig_atoms, lig_type, center, edges, table)

    def density(self, grids, origin, voxel, lig_atoms, lig_w, center, threshold=1.0):
        """A density grid - grids [C,nz,ny,nx] float32, 1 to 4 channels on one orthogonal grid with `origin` and `voxel` [3] in A (x, y,
        z); density.read_mrc and density.channels make them from a map - and the ligand's atoms with their weights prepared for the
        density-fit call on the GPU (dfm_density_create); the receptor is taken to be in the map's frame.  Returns a Density whose
        `.fit(rot, tr)` takes P poses in one call."""
        return Density(self, grids, origin, voxel, lig_atoms, lig_w, center, threshold)


class _Handle:
    """What Native, Atoms, Surface, Interface, Contacts, HBonds, PairPotential and Density share: a handle `_h` made by dfm_<_kind>_create and freed by dfm_<_kind>_destroy - close(), a context
    manager, closed when collected."""
    _kind = None

    def _created(self):
        if not self._h:
            name = f"dfm_{self._kind}_create"
            L.check(-2 if L.lib().dfm_last_error().startswith((name.encode(), b"hipSetDevice")) else -1, name)      # else: bad argument

    def close(self):
        if getattr(self, "_h", None):
            getattr(L.lib(), f"dfm_{self._kind}_destroy")(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _center(center):
    """center as float32 [3]: the rotation centre of a rigid-pose handle."""
    cen = _f32(center).reshape(-1)
    if cen.size != 3:
        raise ValueError(f"center must have 3 entries, got {np.shape(center)}")
    return cen


def _grid_info(n, mx, e):
    """The first three fields of every rigid-pose handle's info(): the receptor's grid."""
    return {"n_cells": n.value, "max_cell_atoms": mx.value, "cell_edge": e.value}


def _last_ms(getter, k):
    """The k millisecond figures that `getter` (a dfm_*_last_timing or dfm_*_last_phases) returns for this thread's last call."""
    v = [C.c_double(0) for _ in range(k)]
    L.check(getattr(L.lib(), getter)(*(C.byref(x) for x in v)), getter)
    return tuple(x.value for x in v)


def _rigid_poses(rot, tr):
    """rot, tr as float32 [P,3] and P: the poses of Atoms.sterics and Surface.bsa."""
    r, t = _f32(rot).reshape(-1, 3), _f32(tr).reshape(-1, 3)
    if r.shape != t.shape or r.shape[0] < 1:
        raise ValueError(f"rot and tr must both be [P,3] with P >= 1, got {np.shape(rot)} and {np.shape(tr)}")
    return r, t, r.shape[0]


class Native(_Handle):
    """A native pose resident on the model's GPU (dfm_native): interface residues, native contacts and the receptor's share of the
    Kabsch sums, computed once.  Read-only after creation: `metrics` may be called from several threads at once."""
    _kind = "native"

    def __init__(self, model: Model, rec_pos, lig_pos, iface_cutoff=10.0, contact_cutoff=5.5):
        rp, lp = _f32(rec_pos).reshape(-1, 9), _f32(lig_pos).reshape(-1, 9)
        self.model, self.R, self.L = model, rp.shape[0], lp.shape[0]
        self._h = L.lib().dfm_native_create(model._h, _p(rp), _p(lp), self.R, self.L, float(iface_cutoff), float(contact_cutoff))
        self._created()

    def info(self):
        """{n_iface_rec, n_iface_lig, n_contacts, iface_rec, iface_lig (ascending residue indices), contacts [n,2] (receptor, ligand)}:
        what metrics.NativeContext calls r1, r2 and act."""
        n = [C.c_int32(0) for _ in range(3)]
        L.check(L.lib().dfm_native_info(self._h, C.byref(n[0]), C.byref(n[1]), C.byref(n[2]), None, None, None), "dfm_native_info")
        r1, r2, act = np.zeros(n[0].value, np.int32), np.zeros(n[1].value, np.int32), np.zeros((n[2].value, 2), np.int32)
        L.check(L.lib().dfm_native_info(self._h, None, None, None, _p(r1, L.I32P), _p(r2, L.I32P), _p(act, L.I32P)), "dfm_native_info")
        return {"n_iface_rec": n[0].value, "n_iface_lig": n[1].value, "n_contacts": n[2].value, "iface_rec": r1, "iface_lig": r2,
                "contacts": act}

    def metrics(self, lig_pos, rec_pos=None):
        """Docking metrics of P poses (dfm_pose_metrics; the float64 definition is metrics.compute_metrics): lig_pos [P,L,3,3] (or one
        [L,3,3] pose), rec_pos [P,R,3,3] or None = the native receptor in every pose.  Returns float64 arrays [P] under the reference's
        keys c_rmsd, i_rmsd, l_rmsd, fnat, DockQ, plus n_recovered (int32: the native contacts found in the pose)."""
        lp = _f32(lig_pos)
        if lp.size and lp.size == self.L * 9:
            lp = lp.reshape(1, self.L, 9)
        if lp.ndim < 2 or lp.shape[0] < 1 or lp.size != lp.shape[0] * self.L * 9:
            raise ValueError(f"lig_pos must be [P,{self.L},3,3] with P >= 1, got {np.shape(lig_pos)}")
        P = lp.shape[0]
        rp = None
        if rec_pos is not None:
            rp = _f32(rec_pos)
            if rp.size == self.R * 9 and P > 1:
                rp = np.ascontiguousarray(np.broadcast_to(rp.reshape(1, self.R, 9), (P, self.R, 9)))
            if rp.size != P * self.R * 9:
                raise ValueError(f"rec_pos must be [P,{self.R},3,3] with P = {P}, got {np.shape(rec_pos)}")
        o = {k: np.zeros(P, np.float64) for k in ("c_rmsd", "i_rmsd", "l_rmsd", "fnat", "DockQ")}
        o["n_recovered"] = np.zeros(P, np.int32)
        out = L.MetricsOutC()
        dp = C.POINTER(C.c_double)
        out.c_rmsd, out.i_rmsd, out.l_rmsd = (o[k].ctypes.data_as(dp) for k in ("c_rmsd", "i_rmsd", "l_rmsd"))
        out.fnat, out.dockq, out.n_recovered = o["fnat"].ctypes.data_as(dp), o["DockQ"].ctypes.data_as(dp), _p(o["n_recovered"], L.I32P)
        L.check(L.lib().dfm_pose_metrics(self._h, P, _p(lp), _p(rp), C.byref(out)), "dfm_pose_metrics")
        return o


class Atoms(_Handle):
    """The heavy atoms of a receptor / ligand pair resident on the model's GPU (dfm_atoms): the receptor binned into a cell grid, the
    ligand in blocks of neighbours.  Read-only after creation: `sterics` may be called from several threads at once."""
    _kind = "atoms"

    def __init__(self, model: Model, rec_atoms, lig_atoms, center, clash_cutoff=3.0, contact_cutoff=5.0):
        ra, la, cen = _f32(rec_atoms).reshape(-1, 3), _f32(lig_atoms).reshape(-1, 3), _center(center)
        self.model, self.Ar, self.Al = model, ra.shape[0], la.shape[0]
        self.clash_cutoff, self.contact_cutoff = float(np.float32(clash_cutoff)), float(np.float32(contact_cutoff))
        prm = L.StericsParamsC(float(clash_cutoff), float(contact_cutoff), 0)
        self._h = L.lib().dfm_atoms_create(model._h, self.Ar, _p(ra), self.Al, _p(la), _p(cen), C.byref(prm))
        self._created()

    def info(self):
        """{n_cells, max_cell_atoms, cell_edge} of the receptor's grid (dfm_atoms_info)."""
        n, mx, e = C.c_int32(0), C.c_int32(0), C.c_float(0)
        L.check(L.lib().dfm_atoms_info(self._h, C.byref(n), C.byref(mx), C.byref(e)), "dfm_atoms_info")
        return _grid_info(n, mx, e)

    def sterics(self, rot, tr, per_atom=False, chunk_poses=0, members=None):
        """Clash / contact screen of P poses (dfm_pose_sterics; the float64 definition is sterics.sterics): rot [P,3] axis-angle and tr
        [P,3] as rot_update / tr_update hold them.  Returns {n_clash, n_contact (int32 [P]), min_dist (float64 [P], +inf without a
        contact)}, with `per_atom` lig_clash / lig_contact (int32 [P,Al], the caller's atom order), and CAPRI's rule over `members`
        (bool [P]; None: every pose) from sterics.capri_flags: flags (bool [P]), threshold, ensemble_mean, ensemble_std."""
        from . import sterics as ST
        r, t, P = _rigid_poses(rot, tr)
        o = {"n_clash": np.zeros(P, np.int32), "n_contact": np.zeros(P, np.int32), "min_dist": np.zeros(P, np.float64)}
        out = L.StericsOutC()
        out.n_clash, out.n_contact = _p(o["n_clash"], L.I32P), _p(o["n_contact"], L.I32P)
        out.min_dist = o["min_dist"].ctypes.data_as(C.POINTER(C.c_double))
        if per_atom:
            o["lig_clash"], o["lig_contact"] = np.zeros((P, self.Al), np.int32), np.zeros((P, self.Al), np.int32)
            out.lig_clash, out.lig_contact = _p(o["lig_clash"], L.I32P), _p(o["lig_contact"], L.I32P)
        L.check(L.lib().dfm_pose_sterics_chunked(self._h, P, _p(r), _p(t), int(chunk_poses), C.byref(out)), "dfm_pose_sterics")
        o["flags"], o["threshold"], o["ensemble_mean"], o["ensemble_std"] = ST.capri_flags(o["n_clash"], members)
        return o


class Surface(_Handle):
    """The heavy atoms of a receptor / ligand pair with their isolated exposure masks resident on the model's GPU (dfm_surface).
    Read-only after creation: `bsa` may be called from several threads at once."""
    _kind = "surface"

    def __init__(self, model: Model, rec_atoms, rec_radius, lig_atoms, lig_radius, center, probe=1.4, points=128):
        from . import surface as SF
        ra, la, cen = _f32(rec_atoms).reshape(-1, 3), _f32(lig_atoms).reshape(-1, 3), _center(center)
        rr, lr = _f32(rec_radius).reshape(-1), _f32(lig_radius).reshape(-1)
        if rr.size != ra.shape[0] or lr.size != la.shape[0]:
            raise ValueError(f"one radius per atom: {ra.shape[0]} / {rr.size} receptor, {la.shape[0]} / {lr.size} ligand")
        self.model, self.Ar, self.Al = model, ra.shape[0], la.shape[0]
        self.K, self.probe = SF.check_points(points), float(np.float32(probe))
        dirs = SF.sphere_points(self.K)
        prm = L.SurfaceParamsC(float(probe), self.K, _p(dirs), 0)
        self._h = L.lib().dfm_surface_create(model._h, self.Ar, _p(ra), _p(rr), self.Al, _p(la), _p(lr), _p(cen), C.byref(prm))
        self._created()
        self.class_radius = self.info()["class_radius"]

    def info(self):
        """{sasa_rec, sasa_lig (A^2 in isolation), rec_exposed [Ar], lig_exposed [Al] (exposed points per atom), class_radius (float32,
        ascending), n_cells, max_cell_atoms, cell_edge} (dfm_surface_info)."""
        sr, sl = C.c_double(0), C.c_double(0)
        re, le = np.zeros(self.Ar, np.int32), np.zeros(self.Al, np.int32)
        nc, n, mx, e = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_float(0)
        cr = np.zeros(16, np.float32)
        L.check(L.lib().dfm_surface_info(self._h, C.byref(sr), C.byref(sl), _p(re, L.I32P), _p(le, L.I32P), C.byref(nc), _p(cr), C.byref(n),
                                         C.byref(mx), C.byref(e)), "dfm_surface_info")
        return {"sasa_rec": sr.value, "sasa_lig": sl.value, "rec_exposed": re, "lig_exposed": le, "class_radius": cr[:nc.value].copy(),
                **_grid_info(n, mx, e)}

    def bsa(self, rot, tr, per_atom=False, chunk_poses=0):
        """Buried surface of P poses (dfm_pose_bsa; the float64 definition is surface.bsa): rot [P,3] axis-angle and tr [P,3] as
        rot_update / tr_update hold them.  Returns {bsa (float64 [P], A^2, both sides), lig_points, rec_points (int32 [P]), class_points
        (int32 [P,2,16])}, with `per_atom` lig_buried [P,Al] / rec_buried [P,Ar] (int32 points, the caller's atom order), and
        bsa_rec / bsa_lig (float64 [P]): the two sides (surface.side_areas)."""
        from . import surface as SF
        r, t, P = _rigid_poses(rot, tr)
        o = {"bsa": np.zeros(P, np.float64), "lig_points": np.zeros(P, np.int32), "rec_points": np.zeros(P, np.int32),
             "class_points": np.zeros((P, 2, 16), np.int32)}
        out = L.BsaOutC()
        out.bsa = o["bsa"].ctypes.data_as(C.POINTER(C.c_double))
        out.lig_points, out.rec_points, out.class_points = (_p(o[k], L.I32P) for k in ("lig_points", "rec_points", "class_points"))
        if per_atom:
            o["lig_buried"], o["rec_buried"] = np.zeros((P, self.Al), np.int32), np.zeros((P, self.Ar), np.int32)
            out.lig_buried, out.rec_buried = _p(o["lig_buried"], L.I32P), _p(o["rec_buried"], L.I32P)
        L.check(L.lib().dfm_pose_bsa_chunked(self._h, P, _p(r), _p(t), int(chunk_poses), C.byref(out)), "dfm_pose_bsa")
        o["bsa_rec"], o["bsa_lig"] = SF.side_areas(o["class_points"], self.class_radius, self.probe, self.K)
        return o


class Interface(_Handle):
    """The heavy atoms of a receptor / ligand pair with their Lennard-Jones parameters and charges resident on the model's GPU
    (dfm_iface).  Read-only after creation: `energy` may be called from several threads at once."""
    _kind = "iface"

    def __init__(self, model: Model, rec_atoms, rec_params, lig_atoms, lig_params, center, cutoff=8.0, soft=0.6, elec_min_dist=3.0,
                 dielectric_slope=4.0):
        ra, la, cen = _f32(rec_atoms).reshape(-1, 3), _f32(lig_atoms).reshape(-1, 3), _center(center)
        rp, lp = _f32(rec_params), _f32(lig_params)
        if rp.shape != (ra.shape[0], 3) or lp.shape != (la.shape[0], 3):
            raise ValueError(f"one (rmin_half, sqrt_eps, charge) row per atom: receptor {ra.shape[0]} / {rp.shape}, ligand {la.shape[0]} / {lp.shape}")
        self.model, self.Ar, self.Al = model, ra.shape[0], la.shape[0]
        self.cutoff, self.soft, self.elec_min_dist, self.dielectric_slope = (float(np.float32(v)) for v in
                                                                             (cutoff, soft, elec_min_dist, dielectric_slope))
        rc, lc = (tuple(np.ascontiguousarray(p[:, k]) for k in range(3)) for p in (rp, lp))
        self._h = L.lib().dfm_iface_create(model._h, self.Ar, _p(ra), _p(rc[0]), _p(rc[1]), _p(rc[2]), self.Al, _p(la), _p(lc[0]), _p(lc[1]),
                                           _p(lc[2]), _p(cen), float(cutoff), float(soft), float(elec_min_dist), float(dielectric_slope))
        self._created()

    def info(self):
        """{n_cells, max_cell_atoms, cell_edge} of the receptor's grid and sum_bound_q, the creator's bound on the magnitude of every
        integer sum of a call in quanta (dfm_iface_info)."""
        n, mx, e, b = C.c_int32(0), C.c_int32(0), C.c_float(0), C.c_double(0)
        L.check(L.lib().dfm_iface_info(self._h, C.byref(n), C.byref(mx), C.byref(e), C.byref(b)), "dfm_iface_info")
        return {**_grid_info(n, mx, e), "sum_bound_q": b.value}

    def energy(self, rot, tr, per_atom=False, chunk_poses=0):
        """Interface energy of P poses (dfm_pose_iface_energy; the float64 definition is ifenergy.interface_energy): rot [P,3] axis-angle
        and tr [P,3] as rot_update / tr_update hold them.  Returns {rep_q, att_q, elec_q, n_pairs (int64 [P]; quanta of 2^-20
        kcal/mol)}, with `per_atom` lig_vdw_q / lig_elec_q (int64 [P,Al], the caller's atom order), and rep, att, elec (float64 [P],
        kcal/mol = q * 2^-20)."""
        from . import ifenergy as IE
        r, t, P = _rigid_poses(rot, tr)
        o = {k: np.zeros(P, np.int64) for k in ("rep_q", "att_q", "elec_q", "n_pairs")}
        if per_atom:
            o["lig_vdw_q"], o["lig_elec_q"] = np.zeros((P, self.Al), np.int64), np.zeros((P, self.Al), np.int64)
        out = L.IfaceOutC()
        for k, v in o.items():
            setattr(out, k, v.ctypes.data_as(C.POINTER(C.c_int64)))
        L.check(L.lib().dfm_pose_iface_energy_chunked(self._h, P, _p(r), _p(t), int(chunk_poses), C.byref(out)), "dfm_pose_iface_energy")
        o["rep"], o["att"], o["elec"] = IE.kcal(o["rep_q"]), IE.kcal(o["att_q"]), IE.kcal(o["elec_q"])
        return o


class Contacts(_Handle):
    """The heavy atoms of a receptor / ligand pair with their residue indices and the residue classes resident on the model's GPU
    (dfm_rescon).  Read-only after creation: `count` may be called from several threads at once."""
    _kind = "rescon"

    def __init__(self, model: Model, rec_atoms, rec_res, rec_class, lig_atoms, lig_res, lig_class, center, cutoff=5.5):
        from . import affinity as AF
        ra, la, cen = _f32(rec_atoms).reshape(-1, 3), _f32(lig_atoms).reshape(-1, 3), _center(center)
        rr, rc = AF.check_residues(rec_res, ra.shape[0], rec_class, "rec")
        lr, lc = AF.check_residues(lig_res, la.shape[0], lig_class, "lig")
        rr, rc, lr, lc = (np.ascontiguousarray(a) for a in (rr, rc, lr, lc))
        self.model, self.Ar, self.Al, self.Rr, self.Lr = model, ra.shape[0], la.shape[0], rc.size, lc.size
        self.W, self.cutoff = (self.Rr + 31) // 32, float(np.float32(cutoff))
        u8 = C.POINTER(C.c_uint8)
        self._h = L.lib().dfm_rescon_create(model._h, self.Ar, _p(ra), _p(rr, L.I32P), self.Rr, rc.ctypes.data_as(u8), self.Al, _p(la),
                                            _p(lr, L.I32P), self.Lr, lc.ctypes.data_as(u8), _p(cen), float(cutoff))
        self._created()

    def info(self):
        """{n_cells, max_cell_atoms, cell_edge} of the receptor's grid, row_words = W and chunk_poses, the poses one chunk of a call
        holds a bitmap for (dfm_rescon_info)."""
        n, mx, e, w, ch = C.c_int32(0), C.c_int32(0), C.c_float(0), C.c_int32(0), C.c_int32(0)
        L.check(L.lib().dfm_rescon_info(self._h, C.byref(n), C.byref(mx), C.byref(e), C.byref(w), C.byref(ch)), "dfm_rescon_info")
        return {**_grid_info(n, mx, e), "row_words": w.value, "chunk_poses": ch.value}

    def count(self, rot, tr, per_residue=False, bits=False, chunk_poses=0):
        """Residue contacts of P poses (dfm_pose_rescon; the float64 definition is affinity.residue_contacts): rot [P,3] axis-angle and
        tr [P,3] as rot_update / tr_update hold them.  Returns {ic [P,6] (AA, AP, AC, PP, PC, CC), n_pairs, n_rec_res, n_lig_res [P]}
        int32, with `per_residue` rec_degree [P,Rr] / lig_degree [P,Lr] int32, with `bits` contact_bits [P,Lr,W] uint32
        (affinity.pairs_of turns one pose's block into residue pairs)."""
        r, t, P = _rigid_poses(rot, tr)
        o = {"ic": np.zeros((P, 6), np.int32), "n_pairs": np.zeros(P, np.int32), "n_rec_res": np.zeros(P, np.int32),
             "n_lig_res": np.zeros(P, np.int32)}
        if per_residue:
            o["rec_degree"], o["lig_degree"] = np.zeros((P, self.Rr), np.int32), np.zeros((P, self.Lr), np.int32)
        out = L.ResconOutC()
        for k, v in o.items():
            setattr(out, k, _p(v, L.I32P))
        if bits:
            o["contact_bits"] = np.zeros((P, self.Lr, self.W), np.uint32)
            out.contact_bits = _p(o["contact_bits"], L.U32P)
        L.check(L.lib().dfm_pose_rescon_chunked(self._h, P, _p(r), _p(t), int(chunk_poses), C.byref(out)), "dfm_pose_rescon")
        return o


class HBonds(_Handle):
    """The polar atoms of a receptor / ligand pair with their antecedents, roles and residues resident on the model's GPU (dfm_hbond).
    Read-only after creation: `count` may be called from several threads at once."""
    _kind = "hbond"

    def __init__(self, model: Model, rec, lig, center, hb_cutoff=3.5, min_angle=90.0, salt_cutoff=4.0):
        from . import hbonds as HB
        cen = _center(center)
        self.hb_cutoff, self.salt_cutoff = HB.check_cutoffs(hb_cutoff, salt_cutoff)
        self.min_angle, self.min_cos2 = float(min_angle), HB.min_cos2(min_angle)
        rx, ra, rro, rre, self.n_rec_res = (np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a for a in HB.check_chain(rec, "rec"))
        lx, la, lro, lre, self.n_lig_res = (np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a for a in HB.check_chain(lig, "lig"))
        self.model, self.Nr, self.Nl = model, rx.shape[0], lx.shape[0]
        u8, status = C.POINTER(C.c_uint8), C.c_int(0)
        self._h = L.lib().dfm_hbond_create(model._h, self.Nr, _p(rx), _p(ra), rro.ctypes.data_as(u8), _p(rre, L.I32P), self.n_rec_res,
                                           self.Nl, _p(lx), _p(la), lro.ctypes.data_as(u8), _p(lre, L.I32P), self.n_lig_res, _p(cen),
                                           float(hb_cutoff), self.min_cos2, float(salt_cutoff), C.byref(status))
        if not self._h:
            L.check(status.value or -1, "dfm_hbond_create")

    def info(self):
        """{n_cells, max_cell_atoms, cell_edge} of the receptor's grid, n_rec_charged / n_lig_charged = the residues with a cation or an
        anion, and chunk_poses, the poses one chunk of a call holds a bitmap for (dfm_hbond_info)."""
        n, mx, e, rc, lc, ch = C.c_int32(0), C.c_int32(0), C.c_float(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        L.check(L.lib().dfm_hbond_info(self._h, C.byref(n), C.byref(mx), C.byref(e), C.byref(rc), C.byref(lc), C.byref(ch)), "dfm_hbond_info")
        return {**_grid_info(n, mx, e), "n_rec_charged": rc.value, "n_lig_charged": lc.value,
                "chunk_poses": ch.value}

    def count(self, rot, tr, per_atom=False, chunk_poses=0):
        """Hydrogen bonds and salt bridges of P poses (dfm_pose_hbonds; the float64 definition is hbonds.hbonds): rot [P,3] axis-angle and
        tr [P,3] as rot_update / tr_update hold them.  Returns {n_hbond [P], hb_kind [P,3] (backbone-backbone, mixed, side chain-side
        chain), n_salt [P] (residue pairs), n_salt_atoms [P]} int32 and, with `per_atom`, rec_hb / rec_sb [P,Nr] and lig_hb / lig_sb
        [P,Nl] int32 in the caller's polar-atom order."""
        r, t, P = _rigid_poses(rot, tr)
        o = {"n_hbond": np.zeros(P, np.int32), "hb_kind": np.zeros((P, 3), np.int32), "n_salt": np.zeros(P, np.int32),
             "n_salt_atoms": np.zeros(P, np.int32)}
        if per_atom:
            o.update(rec_hb=np.zeros((P, self.Nr), np.int32), lig_hb=np.zeros((P, self.Nl), np.int32),
                     rec_sb=np.zeros((P, self.Nr), np.int32), lig_sb=np.zeros((P, self.Nl), np.int32))
        out = L.HbondOutC()
        for k, v in o.items():
            setattr(out, k, _p(v, L.I32P))
        L.check(L.lib().dfm_pose_hbonds_chunked(self._h, P, _p(r), _p(t), int(chunk_poses), C.byref(out)), "dfm_pose_hbonds")
        return o


class PairPotential(_Handle):
    """The heavy atoms of a receptor / ligand pair with their types, the squared bin edges and the quantised table resident on the
    model's GPU (dfm_pairpot).  Read-only after creation: `energy` may be called from several threads at once."""
    _kind = "pairpot"

    def __init__(self, model: Model, rec_atoms, rec_type, lig_atoms, lig_type, center, edges, table):
        from . import pairpot as PP
        ra, la, cen = _f32(rec_atoms).reshape(-1, 3), _f32(lig_atoms).reshape(-1, 3), _center(center)
        e = np.ascontiguousarray(PP.check_edges(edges))
        tb = np.ascontiguousarray(PP.check_table(table, e.size - 1))
        self.model, self.Ar, self.Al, self.T, self.NB = model, ra.shape[0], la.shape[0], tb.shape[0], e.size - 1
        rt = np.ascontiguousarray(PP.check_types(rec_type, self.Ar, self.T, "rec_type"))
        lt = np.ascontiguousarray(PP.check_types(lig_type, self.Al, self.T, "lig_type"))
        self.cutoff = float(e[-1])
        self._h = L.lib().dfm_pairpot_create(model._h, self.Ar, _p(ra), _p(rt, L.I32P), self.Al, _p(la), _p(lt, L.I32P), _p(cen), self.T,
                                             self.NB, _p(e), _p(tb), 0)
        self._created()

    def info(self):
        """{n_cells, max_cell_atoms, cell_edge} of the receptor's grid, pair_bound = the creator's bound on the pairs of one pose, T and
        NB (dfm_pairpot_info)."""
        n, mx, e, b, T, NB = C.c_int32(0), C.c_int32(0), C.c_float(0), C.c_double(0), C.c_int32(0), C.c_int32(0)
        L.check(L.lib().dfm_pairpot_info(self._h, C.byref(n), C.byref(mx), C.byref(e), C.byref(b), C.byref(T), C.byref(NB)), "dfm_pairpot_info")
        return {**_grid_info(n, mx, e), "pair_bound": b.value, "T": T.value, "NB": NB.value}

    def energy(self, rot, tr, per_atom=False, counts=False, chunk_poses=0):
        """Pair potential of P poses (dfm_pose_pairpot; the float64 definition is pairpot.pair_potential): rot [P,3] axis-angle and tr
        [P,3] as rot_update / tr_update hold them.  Returns {energy_q, n_pairs (int64 [P]; quanta of 2^-20 kcal/mol)}, with `per_atom`
        lig_q (int64 [P,Al], the caller's atom order), with `counts` counts (int32 [P,T,T,NB]: ligand type, receptor type, bin - one
        global atomic per pair, the slow path), and energy (float64 [P], kcal/mol = energy_q * 2^-20)."""
        from . import pairpot as PP
        r, t, P = _rigid_poses(rot, tr)
        o = {"energy_q": np.zeros(P, np.int64), "n_pairs": np.zeros(P, np.int64)}
        if per_atom:
            o["lig_q"] = np.zeros((P, self.Al), np.int64)
        out = L.PairpotOutC()
        for k, v in o.items():
            setattr(out, k, v.ctypes.data_as(C.POINTER(C.c_int64)))
        if counts:
            o["counts"] = np.zeros((P, self.T, self.T, self.NB), np.int32)
            out.counts = _p(o["counts"], L.I32P)
        L.check(L.lib().dfm_pose_pairpot_chunked(self._h, P, _p(r), _p(t), int(chunk_poses), C.byref(out)), "dfm_pose_pairpot")
        o["energy"] = PP.kcal(o["energy_q"])
        return o


class Density(_Handle):
    """A density grid, channel-interleaved, and the ligand's atoms with their weights resident on the model's GPU (dfm_density).
    Read-only after creation: `fit` may be called from several threads at once."""
    _kind = "density"

    def __init__(self, model: Model, grids, origin, voxel, lig_atoms, lig_w, center, threshold=1.0):
        from . import density as DN
        g, o, v = DN.check_grid(grids, origin, voxel)
        la, cen = _f32(lig_atoms).reshape(-1, 3), _center(center)
        w = np.ascontiguousarray(DN.check_weights(lig_w, la.shape[0]))
        o, v = np.ascontiguousarray(o), np.ascontiguousarray(v)
        self.model, self.Al, self.C, self.shape, self.threshold = model, la.shape[0], g.shape[0], g.shape[1:], float(np.float32(threshold))
        err = C.c_int(0)
        self._h = L.lib().dfm_density_create(model._h, g.shape[3], g.shape[2], g.shape[1], _p(o), _p(v), self.C, _p(g), self.Al, _p(la), _p(w),
                                             _p(cen), self.threshold, C.byref(err))
        self._created()

    def info(self):
        """{nx, ny, nz, C, chunk_poses (of a call with atom_q), sum_bound (quanta a pose's sums stay below)} (dfm_density_info)."""
        v = [C.c_int32(0) for _ in range(5)]
        b = C.c_double(0)
        L.check(L.lib().dfm_density_info(self._h, *(C.byref(x) for x in v), C.byref(b)), "dfm_density_info")
        return dict(zip(("nx", "ny", "nz", "C", "chunk_poses"), (x.value for x in v)), sum_bound=b.value)

    def fit(self, rot, tr, per_atom=False, chunk_poses=0):
        """Density fit of P poses (dfm_pose_density; the float64 definition is density.density): rot [P,3] axis-angle and tr [P,3] as
        rot_update / tr_update hold them.  Returns {sum_q (int64 [P,C]; quanta of 2^-20), n_inside, n_above (int32 [P])} and, with
        `per_atom`, atom_q (int64 [P,Al]: channel 0, the caller's atom order)."""
        r, t, P = _rigid_poses(rot, tr)
        o = {"sum_q": np.zeros((P, self.C), np.int64), "n_inside": np.zeros(P, np.int32), "n_above": np.zeros(P, np.int32)}
        if per_atom:
            o["atom_q"] = np.zeros((P, self.Al), np.int64)
        out = L.DensityOutC()
        for k, a in o.items():
            setattr(out, k, a.ctypes.data_as(C.POINTER(C.c_int64 if a.dtype == np.int64 else C.c_int32)))
        L.check(L.lib().dfm_pose_density_chunked(self._h, P, _p(r), _p(t), int(chunk_poses), C.byref(out)), "dfm_pose_density")
        return o


def density_last_timing():
    """(host-to-device copy ms, kernel ms) of this thread's last Density.fit call (dfm_density_last_timing)."""
    return _last_ms("dfm_density_last_timing", 2)


def fit_last_timing():
    """(copy_ms, kernel_ms) of this thread's last Model.pose_fit, from the call's own events."""
    return _last_ms("dfm_fit_last_timing", 2)


def pairpot_last_timing():
    """(host-to-device copy ms, kernel ms) of this thread's last PairPotential.energy call (dfm_pairpot_last_timing)."""
    return _last_ms("dfm_pairpot_last_timing", 2)


def pairpot_last_phases():
    """(memsets ms, walk ms, finish ms - the call has no finishing kernel) of this thread's last PairPotential.energy call: its kernel
    time by phase (dfm_pairpot_last_phases)."""
    return _last_ms("dfm_pairpot_last_phases", 3)


def hbond_last_timing():
    """(host-to-device copy ms, kernel ms) of this thread's last HBonds.count call (dfm_hbond_last_timing)."""
    return _last_ms("dfm_hbond_last_timing", 2)


def hbond_last_phases():
    """(memsets ms, walk ms, finish ms) of this thread's last HBonds.count call: its kernel time by phase (dfm_hbond_last_phases)."""
    return _last_ms("dfm_hbond_last_phases", 3)


def rescon_last_timing():
    """(host-to-device copy ms, kernel ms) of this thread's last Contacts.count call (dfm_rescon_last_timing)."""
    return _last_ms("dfm_rescon_last_timing", 2)


def rescon_last_phases():
    """(zeroing the bitmap ms, walk ms, finish ms) of this thread's last Contacts.count call: its kernel time by phase
    (dfm_rescon_last_phases)."""
    return _last_ms("dfm_rescon_last_phases", 3)


def iface_last_timing():
    """(host-to-device copy ms, kernel ms) of this thread's last Interface.energy call (dfm_iface_last_timing)."""
    return _last_ms("dfm_iface_last_timing", 2)


def bsa_last_timing():
    """(host-to-device copy ms, kernel ms) of this thread's last Surface.bsa call (dfm_bsa_last_timing)."""
    return _last_ms("dfm_bsa_last_timing", 2)


def sterics_last_timing():
    """(host-to-device copy ms, kernel ms) of this thread's last Atoms.sterics call (dfm_sterics_last_timing)."""
    return _last_ms("dfm_sterics_last_timing", 2)


def sterics_exit_counts(enable):
    """Diagnostic (dfm_sterics_exit_counts): (waves, left at the sphere test, left at the box test) of this thread's last counted
    Atoms.sterics call; `enable` switches the counting of this thread's next calls."""
    n = (C.c_uint64 * 3)()
    L.check(L.lib().dfm_sterics_exit_counts(int(bool(enable)), n), "dfm_sterics_exit_counts")
    return int(n[0]), int(n[1]), int(n[2])


def metrics_last_timing():
    """(host-to-device copy ms, kernel ms) of this thread's last Native.metrics call (dfm_metrics_last_timing)."""
    return _last_ms("dfm_metrics_last_timing", 2)


def consensus_last_timing():
    """(host-to-device copy ms, kernel ms) of this thread's last Model.consensus call (dfm_consensus_last_timing)."""
    return _last_ms("dfm_consensus_last_timing", 2)


def consensus_chunk_poses(R: int, Lg: int) -> int:
    """Poses per chunk of a Model.consensus call on an R + L complex (dfm_consensus_chunk_poses)."""
    return int(L.lib().dfm_consensus_chunk_poses(int(R), int(Lg)))


def pose_last_timing():
    """(k_pose_dist ms, clustering kernels ms) of this thread's last pose_rmsd / pose_cluster call (dfm_pose_last_timing)."""
    return _last_ms("dfm_pose_last_timing", 2)


class Complex:
    """One receptor/ligand pair resident on the GPU (dfm_complex)."""

    def __init__(self, model: Model, rec_x, lig_x, rec_pos, lig_pos):
        self.model = model
        rec_x, lig_x = _f32(rec_x), _f32(lig_x)
        rec_pos, lig_pos = _f32(rec_pos).reshape(-1, 9), _f32(lig_pos).reshape(-1, 9)
        self.R, self.L = rec_x.shape[0], lig_x.shape[0]
        if rec_x.shape[1] != model.hp.lm_embed_dim or lig_x.shape[1] != model.hp.lm_embed_dim:
            raise ValueError("node features must be [n, lm_embed_dim]")
        if rec_pos.shape[0] != self.R or lig_pos.shape[0] != self.L:
            raise ValueError("positions must be [n, 3, 3] matching the features")
        self.N = self.R + self.L
        self._h = L.lib().dfm_complex_create(model._h, _p(rec_x), _p(lig_x), _p(rec_pos), _p(lig_pos), self.R, self.L)
        if not self._h:
            L.check(-2, "dfm_complex_create")
        self.K = L.lib().dfm_complex_degree(self._h)
        self.n_restraints = 0
        self.symmetry = 0
        self.lig_pos0 = lig_pos.reshape(self.L, 3, 3).copy()

    def close(self):
        if getattr(self, "_h", None):
            L.lib().dfm_complex_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------
    def set_pose(self, rec_pos=None, lig_pos=None):
        """Replace the resident receptor pose and / or the ligand start pose of `sample` (features stay resident)."""
        rp = None if rec_pos is None else _f32(rec_pos).reshape(-1, 9)
        lp = None if lig_pos is None else _f32(lig_pos).reshape(-1, 9)
        if (rp is not None and rp.shape[0] != self.R) or (lp is not None and lp.shape[0] != self.L):
            raise ValueError("set_pose: positions must keep the residue counts of the complex")
        L.check(L.lib().dfm_complex_set_pose(self._h, _p(rp), _p(lp)), "dfm_complex_set_pose")
        if lp is not None:
            self.lig_pos0 = lp.reshape(self.L, 3, 3).copy()

    def set_homomer(self, flag: bool):
        """Value of the 67th ("sym") position channel (positional_embed_dim = 67 models only)."""
        L.check(L.lib().dfm_complex_set_homomer(self._h, int(bool(flag))), "dfm_complex_set_homomer")

    def set_restraints(self, groups, params=None):
        """Store interface restraints (restraints.RestraintGroup list; None or [] clears them) and the step's parameters
        (restraints.RestraintParams, None: the defaults) - dfm_complex_set_restraints.  `sample(restraints=True)` applies them."""
        from .restraints import pack
        gs, pairs, up, w = pack(groups or [], self.R, self.L)
        par = None if params is None else params.to_c()
        rc = L.lib().dfm_complex_set_restraints(self._h, len(up), _p(gs, L.I32P), _p(pairs, L.I32P), _p(up), _p(w),
                                                C.byref(par) if par is not None else None)
        L.check(rc, "dfm_complex_set_restraints")
        self.n_restraints = len(up)

    def restraint_eval(self, lig_pos):
        """The stored restraints at poses lig_pos [B,L,3,3] (or [L,3,3]) on the GPU, with the sampler's own kernel
        (dfm_restraint_eval): {energy [B], n_satisfied [B], step [B,6] = dtau, domega}."""
        lp = _f32(lig_pos)
        if lp.ndim == 3:
            lp = lp[None]
        B = lp.shape[0]
        if lp.shape[1:] != (self.L, 3, 3):
            raise ValueError(f"lig_pos must be [B,{self.L},3,3]")
        o = dict(energy=np.zeros(B, np.float32), n_satisfied=np.zeros(B, np.int32), step=np.zeros((B, 6), np.float32))
        L.check(L.lib().dfm_restraint_eval(self._h, B, _p(lp), _p(o["energy"]), _p(o["n_satisfied"], L.I32P), _p(o["step"])),
                "dfm_restraint_eval")
        return o

    def set_symmetry(self, n, params=None):
        """Store the order n of a cyclic assembly (2 .. 24; 0 or None clears it) and the step's parameters (symmetry.SymmetryParams,
        None: the defaults) - dfm_complex_set_symmetry.  The ligand must be the receptor's own chain (R == L).
        `sample(symmetry=True)` / `refine(symmetry=True)` apply the symmetry step."""
        n = int(n or 0)
        par = None if params is None else params.to_c()
        rc = L.lib().dfm_complex_set_symmetry(self._h, n, C.byref(par) if par is not None else None)
        L.check(rc, "dfm_complex_set_symmetry")
        self.symmetry = n

    def symmetry_eval(self, lig_pos):
        """The stored symmetry at poses lig_pos [B,L,3,3] (or [L,3,3]) on the GPU, with the sampler's own kernel (dfm_symmetry_eval):
        float64 theta [B], screw [B], axis [B,3], axis_point [B,3], fit_rmsd [B], sym_rmsd [B]; int32 order_m [B]; float32 step [B,6] =
        dtau, domega of a non-final step.  The definition: symmetry.evaluate."""
        lp = _f32(lig_pos)
        if lp.ndim == 3:
            lp = lp[None]
        B = lp.shape[0]
        if lp.shape[1:] != (self.L, 3, 3):
            raise ValueError(f"lig_pos must be [B,{self.L},3,3]")
        o = dict(theta=np.zeros(B), screw=np.zeros(B), axis=np.zeros((B, 3)), axis_point=np.zeros((B, 3)), fit_rmsd=np.zeros(B),
                 sym_rmsd=np.zeros(B), order_m=np.zeros(B, np.int32), step=np.zeros((B, 6), np.float32))
        out = L.SymmetryOutC()
        F64P = C.POINTER(C.c_double)
        for k in ("theta", "screw", "axis", "axis_point", "fit_rmsd", "sym_rmsd"):
            setattr(out, k, _p(o[k], F64P))
        out.order_m, out.step = _p(o["order_m"], L.I32P), _p(o["step"])
        L.check(L.lib().dfm_symmetry_eval(self._h, B, _p(lp), C.byref(out)), "dfm_symmetry_eval")
        return o

    def score(self, lig_pos, t, edges=None, seed=0, mfma16=False, energy=True, debug=False, profile=False, f16=False,
              ires=False, return_edges=False, bf16_ops=False, dist=False, bf16=False, l0_table=False):
        """B score evaluations.  lig_pos [B,L,3,3] (or [L,3,3]), t [B] (or scalar).  mfma16: the 16-bit MFMA engine
        (`bf16=` is its deprecated keyword of rounds 1-3).  l0_table: layer 0 through the per-complex message table
        (DFM_F_L0_TABLE; the mfma16 and the fp32 engine, a table each - `sample` uses it by default, `score` only on request)."""
        mfma16 = mfma16 or bf16
        lig_pos = _f32(lig_pos)
        if lig_pos.ndim == 3:
            lig_pos = lig_pos[None]
        B = lig_pos.shape[0]
        t = np.broadcast_to(_f32(t).reshape(-1), (B,)).copy()
        N, Lg, K, H = self.N, self.L, self.K, self.model.hp.node_dim
        o = dict(tr_score=np.zeros((B, 3), np.float32), rot_score=np.zeros((B, 3), np.float32),
                 energy=np.zeros((B,), np.float32), num_clashes=np.zeros((B,), np.int32),
                 f=np.zeros((B, Lg, 3), np.float32), confidence=np.zeros((B,), np.float32))
        out = L.ScoreOutC()
        out.tr_score, out.rot_score = _p(o["tr_score"]), _p(o["rot_score"])
        out.energy, out.num_clashes, out.f = _p(o["energy"]), _p(o["num_clashes"], L.I32P), _p(o["f"])
        out.confidence = _p(o["confidence"])
        if ires:
            o["ires"] = np.zeros((B, N), np.float32)
            out.ires = _p(o["ires"])
        if dist:      # family 1 only: dist_logits [B,R,L,64] (egnn_net.py:447)
            o["dist_logits"] = np.zeros((B, self.R, Lg, 64), np.float32)
            out.dist_logits = _p(o["dist_logits"])
        if return_edges and not debug:      # the graph each evaluation used, without the [B,N,H] debug taps
            o["edges"] = np.zeros((B, N, K), np.int32)
            out.edges = _p(o["edges"], L.I32P)
        if debug:
            o.update(h_last=np.zeros((B, N, H), np.float32), h_first=np.zeros((B, N, H), np.float32),
                     edges=np.zeros((B, N, K), np.int32), edge_codes=np.zeros((B, N, K), np.uint32))
            out.h_last, out.h_first = _p(o["h_last"]), _p(o["h_first"])
            out.edges, out.edge_codes = _p(o["edges"], L.I32P), _p(o["edge_codes"], L.U32P)
        e = None
        if edges is not None:
            e = np.ascontiguousarray(edges, dtype=np.int32)
            if e.ndim == 2:
                e = e[None]
            if e.shape != (B, N, K):
                raise ValueError(f"edges must be [B,N,K] = {(B, N, K)}, got {e.shape}")
        flags = (L.DFM_F_MFMA16 if mfma16 else 0) | (L.DFM_F_ENERGY if energy else 0) | (L.DFM_F_PROFILE if profile else 0) | \
                (L.DFM_F_F16 if f16 else 0) | (L.DFM_F_IRES if ires else 0) | (L.DFM_F_BF16_OPS if bf16_ops else 0) | \
                (L.DFM_F_DIST if dist else 0) | (L.DFM_F_L0_TABLE if l0_table else 0)
        rc = L.lib().dfm_score(self._h, B, _p(lig_pos), _p(t), _p(e, L.I32P), int(seed), flags, C.byref(out))
        L.check(rc, "dfm_score")
        if debug:
            c = o["edge_codes"]
            o["bins"] = np.stack([c & 63, (c >> 6) & 31, (c >> 11) & 31, (c >> 16) & 15], -1).astype(np.int8)
            o["relpos"] = ((c >> 20) & 127).astype(np.int8)
        return o

    def distogram(self, lig_pos, t, edges=None, seed=0, mfma16=False, f16=False, maps=(), contact_bins=7, near_cutoff=None):
        """The distogram head (family 1) of B poses reduced on the GPU - dfm_score_distogram, definition: dfmdock_amd/distogram.py.
        lig_pos [B,L,3,3] (or [L,3,3]), t [B] (or scalar); mfma16 / f16 choose the engine of the forward as in `score`.
        Returns {nll [B], nll_near [B], n_near [B] int32, exp_contacts [B]} and, for every name in `maps` out of "pair_nll",
        "pcontact", "edist" ([B,R,L] each) and "pcontact_mean" ([R,L], mean over the B poses), that map.  near_cutoff None: the
        model's cut_off.  The [B,R,L,64] logits are never materialised (score(dist=True) returns them)."""
        lig_pos = _f32(lig_pos)
        if lig_pos.ndim == 3:
            lig_pos = lig_pos[None]
        B = lig_pos.shape[0]
        if lig_pos.shape[1:] != (self.L, 3, 3):
            raise ValueError(f"lig_pos must be [B,{self.L},3,3]")
        t = np.broadcast_to(_f32(t).reshape(-1), (B,)).copy()
        maps = (maps,) if isinstance(maps, str) else tuple(maps)
        known = ("pair_nll", "pcontact", "edist", "pcontact_mean")
        for m in maps:
            if m not in known:
                raise ValueError(f"unknown map {m!r}: one of {known}")
        N, K = self.N, self.K
        o = dict(nll=np.zeros(B, np.float32), nll_near=np.zeros(B, np.float32), n_near=np.zeros(B, np.int32),
                 exp_contacts=np.zeros(B, np.float32))
        out = L.DistogramOutC()
        out.nll, out.nll_near, out.n_near, out.exp_contacts = _p(o["nll"]), _p(o["nll_near"]), _p(o["n_near"], L.I32P), _p(o["exp_contacts"])
        for m in maps:
            o[m] = np.zeros((self.R, self.L) if m == "pcontact_mean" else (B, self.R, self.L), np.float32)
            setattr(out, m, _p(o[m]))
        e = None
        if edges is not None:
            e = np.ascontiguousarray(edges, dtype=np.int32)
            if e.ndim == 2:
                e = e[None]
            if e.shape != (B, N, K):
                raise ValueError(f"edges must be [B,N,K] = {(B, N, K)}, got {e.shape}")
        par = L.DistogramParamsC(int(contact_bins), 0.0 if near_cutoff is None else float(near_cutoff))
        flags = (L.DFM_F_MFMA16 if mfma16 else 0) | (L.DFM_F_F16 if f16 else 0)
        rc = L.lib().dfm_score_distogram(self._h, B, _p(lig_pos), _p(t), _p(e, L.I32P), int(seed), flags, C.byref(par), C.byref(out))
        L.check(rc, "dfm_score_distogram")
        return o

    def sample(self, B=1, num_steps=40, eps=1e-3, tr_noise_scale=0.5, rot_noise_scale=0.5, noise_annealing=False,
               use_clash_force=False, ode=False, seed=0, mfma16=False, inject=None, trace=False, profile=False, f16=False, bf16_ops=False,
               bf16=False, l0_table=True, graph=False, step_energy=None, restraints=False, symmetry=False):
        """B independent Euler-Maruyama trajectories (inference_base.py:390-468 batched).  l0_table=False: DFM_F_NO_L0_TABLE
        (layer 0 evaluated edge by edge even where the per-complex message table applies).  graph=True: DFM_F_GRAPH (one captured
        step replayed as a hipGraph instead of every launch enqueued by the host; bitwise the same results, no faster on MI355X).
        trace=True returns the pose after every step and the scores of every evaluation; by default it also asks for the energy
        head on every step (DFM_F_STEP_ENERGY - the step evaluations then run their last layer in full); step_energy=False keeps
        the step evaluations exactly as an untraced call runs them (ligand-only last layer, no energy in trace_scores[:, :-1]).
        restraints=True: DFM_F_RESTRAINTS (the restraint step of set_restraints after every update; nothing without a stored set).
        symmetry=True: DFM_F_SYMMETRY (the Cn symmetry step of set_symmetry as the last move of every step; nothing without a stored
        symmetry)."""
        return self._trajectories(None, B, num_steps, eps, tr_noise_scale, rot_noise_scale, noise_annealing, use_clash_force, ode, seed,
                                  mfma16 or bf16, inject, trace, profile, f16, bf16_ops, l0_table, graph, step_energy, restraints, symmetry)

    def _trajectories(self, refine, B, num_steps, eps, tr_noise_scale, rot_noise_scale, noise_annealing, use_clash_force, ode, seed, mfma16,
                      inject, trace, profile, f16, bf16_ops, l0_table, graph, step_energy, restraints, symmetry=False):
        """dfm_sample (refine None) or dfm_refine (refine = (RefineParamsC, RefineInjectC or None, arrays to keep alive))."""
        if step_energy is None:
            step_energy = bool(trace)
        Lg, N, K, S = self.L, self.N, self.K, int(num_steps)
        o = dict(lig_pos=np.zeros((B, Lg, 3, 3), np.float32), rot_update=np.zeros((B, 3), np.float32),
                 tr_update=np.zeros((B, 3), np.float32), energy=np.zeros((B,), np.float32),
                 num_clashes=np.zeros((B,), np.int32), final_scores=np.zeros((B, 6), np.float32))
        out = L.TrajOutC()
        out.lig_pos, out.rot_update, out.tr_update = _p(o["lig_pos"]), _p(o["rot_update"]), _p(o["tr_update"])
        out.energy, out.num_clashes = _p(o["energy"]), _p(o["num_clashes"], L.I32P)
        out.final_scores = _p(o["final_scores"])
        if trace:
            o.update(trace_pose=np.zeros((B, S, Lg, 3, 3), np.float32), trace_scores=np.zeros((B, S + 1, 8), np.float32),
                     init_pose=np.zeros((B, Lg, 3, 3), np.float32))
            out.trace_pose, out.trace_scores, out.init_pose = _p(o["trace_pose"]), _p(o["trace_scores"]), _p(o["init_pose"])
        inj, keep = None, []
        if inject:
            inj = L.InjectC()
            shapes = {"R0": (B, 9), "tr_draw": (B, 3), "z_rot": (B, S, 3), "z_tr": (B, S, 3)}
            for k, shp in shapes.items():
                if inject.get(k) is not None:
                    a = _f32(inject[k]).reshape(shp)
                    keep.append(a)
                    setattr(inj, k, _p(a))
            if inject.get("edges") is not None:
                a = np.ascontiguousarray(inject["edges"], dtype=np.int32).reshape(B, S + 1, N, K)
                keep.append(a)
                inj.edges = _p(a, L.I32P)
        flags = (L.DFM_F_MFMA16 if mfma16 else 0) | (L.DFM_F_NOISE_ANNEALING if noise_annealing else 0) | \
                (L.DFM_F_CLASH_FORCE if use_clash_force else 0) | (L.DFM_F_ODE if ode else 0) | \
                (L.DFM_F_PROFILE if profile else 0) | (L.DFM_F_STEP_ENERGY if step_energy else 0) | (L.DFM_F_F16 if f16 else 0) | \
                (L.DFM_F_BF16_OPS if bf16_ops else 0) | (0 if l0_table else L.DFM_F_NO_L0_TABLE) | \
                (L.DFM_F_GRAPH if graph else 0) | (L.DFM_F_RESTRAINTS if restraints else 0) | \
                (L.DFM_F_SYMMETRY if symmetry else 0)
        if refine is not None:
            par, rinj, _alive = refine
            rc = L.lib().dfm_refine(self._h, int(B), S, float(eps), float(tr_noise_scale), float(rot_noise_scale), flags, int(seed),
                                    C.byref(par), C.byref(inj) if inj is not None else None,
                                    C.byref(rinj) if rinj is not None else None, C.byref(out))
            L.check(rc, "dfm_refine")
            return o
        rc = L.lib().dfm_sample(self._h, int(B), S, float(eps), float(tr_noise_scale), float(rot_noise_scale), flags,
                                int(seed), C.byref(inj) if inj is not None else None, C.byref(out))
        L.check(rc, "dfm_sample")
        return o

    @staticmethod
    def _refine_inject(refine_inject, B):
        if not refine_inject:
            return None, []
        rinj, keep = L.RefineInjectC(), []
        for k, shp in {"u_angle": (B,), "axis_draw": (B, 3), "tr_draw": (B, 3)}.items():
            if refine_inject.get(k) is not None:
                a = _f32(refine_inject[k]).reshape(shp)
                keep.append(a)
                setattr(rinj, k, _p(a))
        return rinj, keep

    def refine(self, B=1, t_begin=0.1, start_pos=None, perturb=True, num_steps=40, eps=1e-3, tr_noise_scale=0.5, rot_noise_scale=0.5,
               noise_annealing=False, use_clash_force=False, ode=False, seed=0, mfma16=False, inject=None, refine_inject=None, trace=False,
               profile=False, f16=False, bf16_ops=False, bf16=False, l0_table=True, graph=False, step_energy=None, restraints=False,
               symmetry=False):
        """Local refinement (dfm_refine; definition: dfmdock_amd/refine.py): B trajectories that start from `start_pos` [B,L,3,3] (one
        pose per trajectory; [L,3,3]: the same for all; None: the stored ligand pose), noised with the reference's forward process at
        `t_begin` (perturb=False: the pose itself), and run `sample`'s steps over linspace(t_begin, eps, num_steps).  Keywords and the
        returned dict are `sample`'s; rot_update / tr_update map each trajectory's START pose onto its final pose.  `inject`: z_rot,
        z_tr, edges as for `sample` (R0 / tr_draw are randomize_pose's: ValueError); `refine_inject`: u_angle [B], axis_draw [B,3],
        tr_draw [B,3] of the start."""
        par, keep = L.RefineParamsC(), []
        par.t_begin, par.perturb = float(t_begin), int(bool(perturb))
        if start_pos is not None:
            sp = _f32(start_pos)
            if sp.shape in ((self.L, 3, 3), (self.L, 9)):
                sp = np.repeat(sp.reshape(1, self.L, 9), B, 0)
            if sp.size != B * self.L * 9:
                raise ValueError(f"start_pos must be [B,{self.L},3,3] (or one [{self.L},3,3] pose)")
            sp = np.ascontiguousarray(sp.reshape(B, self.L, 9))
            keep.append(sp)
            par.start_pos = _p(sp)
        rinj, k2 = self._refine_inject(refine_inject, B)
        return self._trajectories((par, rinj, keep + k2), B, num_steps, eps, tr_noise_scale, rot_noise_scale, noise_annealing,
                                  use_clash_force, ode, seed, mfma16 or bf16, inject, trace, profile, f16, bf16_ops, l0_table, graph,
                                  step_energy, restraints, symmetry)

    def forward_marginal(self, B, t, seed=0, refine_inject=None):
        """The draws `refine` starts from at t_begin = t (dfm_forward_marginal, the start kernel in evaluation mode): {rot [B,3]
        axis-angle, tr [B,3]}."""
        rinj, keep = self._refine_inject(refine_inject, B)
        o = dict(rot=np.zeros((B, 3), np.float32), tr=np.zeros((B, 3), np.float32))
        L.check(L.lib().dfm_forward_marginal(self._h, int(B), float(t), int(seed), C.byref(rinj) if rinj is not None else None,
                                             _p(o["rot"]), _p(o["tr"])), "dfm_forward_marginal")
        return o

    def selfcheck(self, n_eval=4, t=None, seed=0, precision="mfma16", bf16_ops=False):
        """dfm_complex_selfcheck: the stored pose through the fp32 engine and the 16-bit engine `precision` names on the same
        n_eval engine-drawn graphs; deviations, cancellation ratios and the fp16 range telemetry as a dict (include/dfmdock_amd.h:
        dfm_selfcheck_out).  `ok` False = do not trust the 16-bit engine on this model / complex: run precision="fp32"."""
        kw = precision_kwargs(precision)
        if not (kw["mfma16"] or kw["f16"]):
            raise ValueError("selfcheck compares a 16-bit engine with the fp32 engine: precision must be 'mfma16' or 'f16'")
        flags = (L.DFM_F_F16 if kw["f16"] else L.DFM_F_MFMA16) | (L.DFM_F_BF16_OPS if bf16_ops else 0)
        tt = None
        if t is not None:
            tt = _f32(t).reshape(-1)
            n_eval = tt.size
        out = L.SelfcheckC()
        L.check(L.lib().dfm_complex_selfcheck(self._h, int(n_eval), _p(tt), int(seed), flags, C.byref(out)), "dfm_complex_selfcheck")
        d = out.depth
        r = {k: getattr(out, k) for k in ("n_eval", "depth", "dev_f", "dev_tr_score", "dev_rot_score", "dev_energy", "gate_f", "gate_score",
                                          "gate_energy", "limit", "headroom", "saturated")}
        r.update(cancel_ratio=list(out.cancel_ratio), score_bound=list(out.score_bound), max_h=list(out.max_h)[: d + 1],
                 range_ok=bool(out.range_ok), dev_ok=bool(out.dev_ok), ok=bool(out.ok), precision=canonical_precision(precision))
        for k in ("max_A", "max_Bm", "max_tab", "max_sum16", "max_pre", "max_acc"):
            r[k] = list(getattr(out, k))[:d]
        return r

    def profile(self):
        p = L.ProfileC()
        L.check(L.lib().dfm_get_profile(self._h, C.byref(p)), "dfm_get_profile")
        return dict(edge_kernel_ms=p.edge_kernel_ms, edge_kernel_launches=p.edge_kernel_launches,
                    edge_rows=p.edge_rows, total_ms=p.total_ms, phase_cycles=list(p.phase_cycles), slot_cycles=list(p.slot_cycles),
                    l0_evals=p.l0_evals, l0_edges=p.l0_edges, l0_miss_rows=p.l0_miss_rows, l0_rows_ms=p.l0_rows_ms,
                    l0_gather_ms=p.l0_gather_ms, l0_build_ms=p.l0_build_ms, edge_lig_launches=p.edge_lig_launches, edge_lig_ms=p.edge_lig_ms,
                    edge_shader_cycles=p.edge_shader_cycles, edge_ref_ticks=p.edge_ref_ticks,
                    edge_sclk_mhz=(100.0 * p.edge_shader_cycles / p.edge_ref_ticks) if p.edge_ref_ticks > 0 else None)
