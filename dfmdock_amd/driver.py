"""Drivers around the sampling engine: the DB5-set sweep and the single-pair run.

  run_set      <- inference_mlsb.Sampler.run_sampling (src/inference_mlsb.py:188-262) over
                  PPIDataset('db5_test', training=False) (src/datasets/ppi_dataset.py:224-329): ESM || one-hot
                  features, relpos from (R, L), and the RANDOM GLOBAL ROTATION the loader applies even at test time
                  (:212-219, :309); CSV rows {id,index,c_rmsd,i_rmsd,l_rmsd,fnat,DockQ,energy,num_clashes}
                  (src/inference_base.py:495-499,:589-596)
  dock_pair    <- inference() (src/inference_base.py:601-670): num_samples trajectories, keep the minimum energy,
                  apply its (rot, tr) to the all-atom ligand, write output.pdb

Work is sharded over ranks by complexes (longest first, distributed.assign_work) - or, with fewer than two complexes per
rank, by TRAJECTORIES: every rank then samples its block of each complex's trajectories (all ranks hold all complexes: weights
7 MB + <= 3.6 MB of features per complex), so that a short list of complexes still fills every GPU with one large batch
instead of leaving ranks idle.  The energy-ranked records are gathered with the single collective of
distributed.gather_records.
"""
from __future__ import annotations

import csv
import os
from typing import Callable, NamedTuple

import numpy as np

from . import distributed as D
from . import engine, pdbio
from .cluster import rank_order, rebuild_backbone
from .metrics import NativeContext, compute_metrics

CSV_FIELDS = ["id", "index", "c_rmsd", "i_rmsd", "l_rmsd", "fnat", "DockQ", "energy", "num_clashes"]
RESTRAINT_FIELDS = ["restraint_energy", "restraints_satisfied"]      # appended to the rows only when restraints are given
CLUSTER_FIELDS = ["cluster", "is_center"]      # appended to the rows only when clustering is asked for
STEP_FIELDS = ["id", "index", "step", "t", "c_rmsd", "i_rmsd", "l_rmsd", "fnat", "DockQ"]      # the long table of run_set(step_metrics=True)
METRIC_FIELDS = ["c_rmsd", "i_rmsd", "l_rmsd", "fnat", "DockQ"]
CONSENSUS_FIELDS = ["consensus", "n_contacts"]      # appended to the rows only when consensus scoring is asked for


def rotate_complex(rec_pos, lig_pos, Rm):
    """ppi_dataset.py:212-219: rotate the whole complex about its joint CA centroid (which also centres it)."""
    pos = np.concatenate([rec_pos, lig_pos], 0).astype(np.float32)
    cen = pos[:, 1, :].mean(0)
    pos = (pos - cen) @ np.asarray(Rm, np.float32).T
    return pos[: rec_pos.shape[0]], pos[rec_pos.shape[0]:]


def random_rotation(rec_pos, lig_pos, rng):
    """The loader's test-time augmentation with a Haar-uniform rotation (scipy Rotation.random(): normalised
    Gaussian quaternion, scalar last)."""
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    x, y, z, w = q
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return rotate_complex(rec_pos, lig_pos, Rm)


def input_pose(c, rot_seed, global_rotation):
    """The (receptor, ligand) backbone a complex is sampled from: the loader's random rotation applied when `global_rotation`."""
    rec_pos, lig_pos = np.asarray(c["rec_pos"], np.float32), np.asarray(c["lig_pos"], np.float32)
    if global_rotation:
        rec_pos, lig_pos = random_rotation(rec_pos, lig_pos, np.random.default_rng(rot_seed))
    return rec_pos, lig_pos


def cluster_trajectories(model: engine.Model, lig_pos0, rot_update, tr_update, key, radius, rule="energy", max_clusters=None):
    """Cluster trajectories on the GPU (dfm_pose_cluster) by the ligand backbone rebuilt from their final (rot_update, tr_update) on
    the input backbone lig_pos0 (cluster.rebuild_backbone): a function of those records alone, so every world size and sharding gives
    the same clusters.  `key` [n]: lower = better.  Returns the dict of Model.pose_cluster."""
    poses = rebuild_backbone(lig_pos0, rot_update, tr_update, model.hp.family)
    return model.pose_cluster(poses, radius, key=key, rule=rule, max_clusters=max_clusters)


def ensemble_consensus(model: engine.Model, rec_bb, lig0, rot_update, tr_update, energy, cutoff=5.5, top=1.0):
    """Consensus contact scoring of trajectories on the GPU (dfm_pose_consensus) on the ligand backbone rebuilt from their final
    (rot_update, tr_update) on the input backbone lig0 (cluster.rebuild_backbone, as cluster_trajectories does).  Members: the best `top`
    fraction by energy (consensus.energy_members); every trajectory is scored.  Returns the dict of Model.consensus plus `members`."""
    from . import consensus as CS
    poses = rebuild_backbone(lig0, rot_update, tr_update, model.hp.family)
    members = CS.energy_members(energy, top)
    out = model.consensus(rec_bb, poses, cutoff=cutoff, members=members)
    out["members"] = members
    return out


def sterics_inputs(rec, lig, family):
    """What the all-atom screen takes from two pdbio.backbone_from_atoms dicts: the heavy atoms of both chains (sterics.heavy_atoms,
    float32 [n,3]) and the centre pdbio.apply_pose_all_atom rotates the ligand about for this model family, as float32."""
    from . import sterics as ST
    ra = np.asarray(rec["aa_coords"], np.float32)[ST.heavy_atoms(rec["atoms"])]
    la = np.asarray(lig["aa_coords"], np.float32)[ST.heavy_atoms(lig["atoms"])]
    cen = np.asarray(lig["aa_coords"], np.float64).reshape(-1, 3).mean(0) if family == 1 else np.asarray(lig["bb_coords"], np.float64)[:, 1].mean(0)
    return ra, la, cen.astype(np.float32)


def ensemble_sterics(model: engine.Model, rec, lig, rot_update, tr_update, clash_cutoff=3.0, contact_cutoff=5.0, per_atom=False):
    """All-atom clash / contact screen of trajectories on the GPU (dfm_pose_sterics) from their final (rot_update, tr_update) alone: the
    heavy atoms of the two parsed PDB chains, the ligand moved as pdbio.apply_pose_all_atom moves it.  Returns the dict of Atoms.sterics
    (n_clash, n_contact, min_dist, flags, threshold, ensemble_mean, ensemble_std) plus the cutoffs."""
    ra, la, cen = sterics_inputs(rec, lig, model.hp.family)
    with model.atoms(ra, la, cen, clash_cutoff, contact_cutoff) as at:
        out = at.sterics(np.asarray(rot_update, np.float32).reshape(-1, 3), np.asarray(tr_update, np.float32).reshape(-1, 3), per_atom=per_atom)
        out.update(clash_cutoff=at.clash_cutoff, contact_cutoff=at.contact_cutoff)
    return out


def residue_sterics(model: engine.Model, rec, lig, rot, tr, clash_cutoff=3.0, contact_cutoff=5.0):
    """Per ligand residue of ONE pose: (keys, clash pairs, contact pairs) - the per-atom counts of the screen summed over each residue's
    heavy atoms (sterics.residue_of_atoms)."""
    from . import sterics as ST
    sd = ensemble_sterics(model, rec, lig, np.asarray(rot).reshape(1, 3), np.asarray(tr).reshape(1, 3), clash_cutoff, contact_cutoff, per_atom=True)
    keys, res = ST.residue_of_atoms(lig["atoms"], ST.heavy_atoms(lig["atoms"]))
    return keys, ST.residue_counts(sd["lig_clash"][0], res, len(keys)), ST.residue_counts(sd["lig_contact"][0], res, len(keys))


def surface_inputs(rec, lig, family):
    """What the buried-surface call takes from two pdbio.backbone_from_atoms dicts: sterics_inputs plus the van der Waals radius of every
    heavy atom (surface.element_radius, float32 [n])."""
    from . import sterics as ST
    from . import surface as SF
    ra, la, cen = sterics_inputs(rec, lig, family)
    return ra, SF.atom_radii(rec["atoms"], ST.heavy_atoms(rec["atoms"])), la, SF.atom_radii(lig["atoms"], ST.heavy_atoms(lig["atoms"])), cen


def ensemble_surface(model: engine.Model, rec, lig, rot_update, tr_update, probe=1.4, sphere_points=128, per_atom=False):
    """Buried solvent-accessible surface area of trajectories on the GPU (dfm_pose_bsa) from their final (rot_update, tr_update) alone:
    the heavy atoms of the two parsed PDB chains with their element radii, the ligand moved as pdbio.apply_pose_all_atom moves it.
    Returns the dict of Surface.bsa plus probe, sphere_points and the two radius arrays and, with `per_atom`, rec_exposed / lig_exposed
    (the points of every atom that are exposed in isolation, Surface.info)."""
    ra, rr, la, lr, cen = surface_inputs(rec, lig, model.hp.family)
    with model.surface(ra, rr, la, lr, cen, probe, sphere_points) as sf:
        out = sf.bsa(np.asarray(rot_update, np.float32).reshape(-1, 3), np.asarray(tr_update, np.float32).reshape(-1, 3), per_atom=per_atom)
        out.update(probe=sf.probe, sphere_points=sf.K, rec_radius=rr, lig_radius=lr)
        if per_atom:
            info = sf.info()
            out.update(rec_exposed=info["rec_exposed"], lig_exposed=info["lig_exposed"])
    return out


def residue_surface(model: engine.Model, rec, lig, rot, tr, probe=1.4, sphere_points=128):
    """Per residue of ONE pose: ((receptor keys, ligand keys), (receptor areas, ligand areas)) - the buried points of each residue's heavy
    atoms as areas in A^2 (surface.residue_bsa)."""
    from . import sterics as ST
    from . import surface as SF
    bd = ensemble_surface(model, rec, lig, np.asarray(rot).reshape(1, 3), np.asarray(tr).reshape(1, 3), probe, sphere_points, per_atom=True)
    keys, area = [], []
    for chain, buried, radius in ((rec, bd["rec_buried"][0], bd["rec_radius"]), (lig, bd["lig_buried"][0], bd["lig_radius"])):
        k, res = ST.residue_of_atoms(chain["atoms"], ST.heavy_atoms(chain["atoms"]))
        keys.append(k)
        area.append(SF.residue_bsa(buried, radius, res, len(k), bd["probe"], bd["sphere_points"]))
    return keys, area


def _check_surface(bsa, min_bsa, probe, sphere_points):
    """None (off) or (min_bsa or None, probe, sphere points) of a pair driver's surface options; min_bsa implies bsa."""
    if not bsa and min_bsa is None:
        return None
    from . import surface as SF
    if min_bsa is not None and not np.isfinite(min_bsa):
        raise ValueError(f"min_bsa must be finite, got {min_bsa}")
    return (None if min_bsa is None else float(min_bsa)), SF.check_probe(probe), SF.check_points(sphere_points)


def _pose_bsa(bd, k):
    return {"bsa": float(bd["bsa"][k]), "bsa_rec": float(bd["bsa_rec"][k]), "bsa_lig": float(bd["bsa_lig"][k])}


def _surface_result(bd, k, opts):
    """The surface entries of a pair driver's result for the kept pose k: none without the option."""
    if bd is None:
        return {}
    out = dict(_pose_bsa(bd, k), bsa_data=bd, probe=bd["probe"], sphere_points=bd["sphere_points"], index=int(k))
    if opts[0] is not None:
        out["min_bsa"] = opts[0]
    return out


def iface_inputs(rec, lig, family):
    """What the interface-energy call takes from two pdbio.backbone_from_atoms dicts: sterics_inputs plus the (rmin_half, sqrt_eps,
    charge) row of every heavy atom (ifenergy.atom_parameters, float32 [n,3])."""
    from . import ifenergy as IE
    ra, la, cen = sterics_inputs(rec, lig, family)
    return ra, IE.atom_parameters(rec["atoms"]), la, IE.atom_parameters(lig["atoms"]), cen


def ensemble_interface_energy(model: engine.Model, rec, lig, rot_update, tr_update, cutoff=8.0, weights=None, per_atom=False):
    """Interface energy of trajectories on the GPU (dfm_pose_iface_energy) from their final (rot_update, tr_update) alone: soft
    Lennard-Jones plus Coulomb (eps = 4 r) over the heavy-atom pairs of the two parsed PDB chains within `cutoff` A.  Returns the dict of
    Interface.energy plus total (float64 [P], ifenergy.total with `weights`: None = ifenergy.WEIGHTS, starting values that are not
    fitted), weights and cutoff."""
    from . import ifenergy as IE
    w = IE.WEIGHTS if weights is None else tuple(float(v) for v in weights)
    ra, rp, la, lp, cen = iface_inputs(rec, lig, model.hp.family)
    with model.interface(ra, rp, la, lp, cen, cutoff=cutoff) as h:
        out = h.energy(np.asarray(rot_update, np.float32).reshape(-1, 3), np.asarray(tr_update, np.float32).reshape(-1, 3), per_atom=per_atom)
        out.update(total=IE.total(out["rep"], out["att"], out["elec"], w), weights=w, cutoff=h.cutoff)
    return out


def residue_interface_energy(model: engine.Model, rec, lig, rot, tr, cutoff=8.0):
    """Per ligand residue of ONE pose: (keys, vdw, elec) - the per-atom sums of the interface energy in quanta of 2^-20 kcal/mol summed
    over each residue's heavy atoms (sterics.residue_of_atoms, ifenergy.residue_energy)."""
    from . import ifenergy as IE
    from . import sterics as ST
    ed = ensemble_interface_energy(model, rec, lig, np.asarray(rot).reshape(1, 3), np.asarray(tr).reshape(1, 3), cutoff, per_atom=True)
    keys, res = ST.residue_of_atoms(lig["atoms"], ST.heavy_atoms(lig["atoms"]))
    return keys, IE.residue_energy(ed["lig_vdw_q"][0], res, len(keys)), IE.residue_energy(ed["lig_elec_q"][0], res, len(keys))


def _check_interface(interface_energy, rank, ie_weights, ie_cutoff):
    """None (off) or (rank by it, weights, cutoff) of a pair driver's interface-energy options; rank "interface" implies them."""
    if not interface_energy and rank != "interface":
        return None
    from . import ifenergy as IE
    w = IE.WEIGHTS if ie_weights is None else tuple(float(v) for v in ie_weights)
    IE.total(0.0, 0.0, 0.0, w)      # three finite numbers
    return rank == "interface", w, IE.check_scalars(cutoff=ie_cutoff)[0]


def _pose_interface(ed, k):
    return {"rep": float(ed["rep"][k]), "att": float(ed["att"][k]), "elec": float(ed["elec"][k]), "total": float(ed["total"][k]),
            "n_pairs": int(ed["n_pairs"][k])}


def _interface_result(ed, k, opts, bad=None, ranked_by="energy"):
    """The `interface_energy` entries of a pair driver's result for the FINAL kept pose k (none without the option): its terms, its
    rank by total among the poses the clash filter left, and `ranked_by` - the rule that chose k."""
    if ed is None:
        return {}
    _, weights, cutoff = opts
    tot = _nan_key(ed["total"], bad)
    summary = dict(_pose_interface(ed, k), rank=int(np.nonzero(rank_order(tot, len(tot)) == k)[0][0]) + 1, weights=list(weights),
                   cutoff=float(cutoff), ranked_by=ranked_by)
    return {"interface_energy": summary, "interface_data": ed, "index": int(k)}


def pairpot_inputs(rec, lig, family, pot):
    """What the pair-potential call takes from two pdbio.backbone_from_atoms dicts and a potential (pairpot.load's dict): the heavy
    atoms of both chains that the file's type names give a type (pairpot.atom_types; float32 [n,3] and int32 [n]), the centre of
    sterics_inputs, the indices of the ligand's typed atoms among lig["atoms"] and the number of heavy atoms of both chains that no name
    fits - those are left out of every sum."""
    from . import pairpot as PP
    _, _, cen = sterics_inputs(rec, lig, family)
    rt, rk, ru = PP.atom_types(rec["atoms"], pot["type_names"])
    lt, lk, lu = PP.atom_types(lig["atoms"], pot["type_names"])
    if not rk.size or not lk.size:
        raise ValueError("the potential's type names fit no heavy atom of " + ("the receptor" if not rk.size else "the ligand"))
    return np.asarray(rec["aa_coords"], np.float32)[rk], rt, np.asarray(lig["aa_coords"], np.float32)[lk], lt, cen, lk, ru + lu


def ensemble_pairpot(model: engine.Model, rec, lig, rot_update, tr_update, pot, per_atom=False, counts=False):
    """Tabulated pair potential of trajectories on the GPU (dfm_pose_pairpot) from their final (rot_update, tr_update) alone, over the
    typed heavy atoms of the two parsed PDB chains (pairpot_inputs); pot: pairpot.load's dict - the project ships no table.  Returns the
    dict of PairPotential.energy plus n_untyped, T, NB, cutoff and lig_kept (the ligand's typed atoms as indices into lig["atoms"])."""
    ra, rt, la, lt, cen, lk, nu = pairpot_inputs(rec, lig, model.hp.family, pot)
    with model.pairpot(ra, rt, la, lt, cen, pot["edges"], pot["table"]) as h:
        out = h.energy(np.asarray(rot_update, np.float32).reshape(-1, 3), np.asarray(tr_update, np.float32).reshape(-1, 3), per_atom=per_atom,
                       counts=counts)
        out.update(n_untyped=int(nu), T=h.T, NB=h.NB, cutoff=h.cutoff, lig_kept=lk)
    return out


def residue_pairpot(model: engine.Model, rec, lig, rot, tr, pot):
    """Per ligand residue of ONE pose: (keys, q) - the per-atom sums of the pair potential in quanta of 2^-20 kcal/mol summed over each
    residue's typed heavy atoms (sterics.residue_of_atoms over the heavy atoms, pairpot.residue_energy)."""
    from . import pairpot as PP
    from . import sterics as ST
    pd = ensemble_pairpot(model, rec, lig, np.asarray(rot).reshape(1, 3), np.asarray(tr).reshape(1, 3), pot, per_atom=True)
    heavy = ST.heavy_atoms(lig["atoms"])
    keys, res = ST.residue_of_atoms(lig["atoms"], heavy)
    of_atom = dict(zip(heavy.tolist(), res.tolist()))
    return keys, PP.residue_energy(pd["lig_q"][0], np.array([of_atom[int(i)] for i in pd["lig_kept"]], np.int64), len(keys))


def _check_pairpot(pair_potential, rank):
    """None (off) or (rank by it, the potential) of a pair driver's pair-potential options: pair_potential is pairpot.load's dict or the
    path of such a file; rank "pairpot" needs one."""
    if pair_potential is None:
        if rank == "pairpot":
            raise ValueError("rank 'pairpot' needs a pair_potential: the project ships no table")
        return None
    from . import pairpot as PP
    pot = PP.load(pair_potential) if isinstance(pair_potential, (str, os.PathLike)) else dict(pair_potential)
    pot["edges"] = PP.check_edges(pot["edges"])
    pot["table"] = PP.check_table(pot["table"], pot["edges"].size - 1)
    if len(pot["type_names"]) != pot["table"].shape[0]:
        raise ValueError(f"pair_potential: {len(pot['type_names'])} type names for {pot['table'].shape[0]} types")
    return rank == "pairpot", pot


def _pose_pairpot(pd, k):
    return {"energy": float(pd["energy"][k]), "n_pairs": int(pd["n_pairs"][k]), "n_untyped": int(pd["n_untyped"]), "T": int(pd["T"]),
            "NB": int(pd["NB"]), "cutoff": float(pd["cutoff"])}


def _pairpot_result(pd, k):
    """The `pair_potential` entries of a pair driver's result for the FINAL kept pose k: none without the option."""
    if pd is None:
        return {}
    return {"pair_potential": _pose_pairpot(pd, k), "pairpot_data": pd, "index": int(k)}


def density_inputs(rec, lig, family):
    """What the density fit takes from two pdbio.backbone_from_atoms dicts: sterics_inputs (the heavy atoms of both chains and the
    centre) plus the weight of every heavy atom - its element's atomic number (density.atom_weights) - receptor first."""
    from . import density as DN
    from . import sterics as ST
    ra, la, cen = sterics_inputs(rec, lig, family)
    return ra, DN.atom_weights(rec["atoms"], ST.heavy_atoms(rec["atoms"])), la, DN.atom_weights(lig["atoms"], ST.heavy_atoms(lig["atoms"])), cen


def ensemble_density(model: engine.Model, rec, lig, rot_update, tr_update, dmap, resolution, threshold=1.0, per_atom=False):
    """Density fit of trajectories on the GPU (dfm_pose_density) from their final (rot_update, tr_update) alone: the heavy atoms of the
    two parsed PDB chains, weighted by atomic number, against dmap (density.read_mrc's dict; the receptor is taken to sit in the map's
    frame) at `resolution` A (sigma = resolution * density.SIGMA_FACTOR).  The three grids of density.channels are gathered in one call.
    Returns the dict of Density.fit plus cc (density.correlation), neg_cc, inclusion (n_above / Al), n_outside (Al - n_inside), Al,
    scalars, resolution, sigma and threshold."""
    from . import density as DN
    ra, rw, la, lw, cen = density_inputs(rec, lig, model.hp.family)
    sigma = float(resolution) * DN.SIGMA_FACTOR
    grids, scalars = DN.channels(dmap, ra, rw, sigma, la, lw)
    with model.density(grids, dmap["origin"], dmap["voxel"], la, lw, cen, threshold) as h:
        out = h.fit(np.asarray(rot_update, np.float32).reshape(-1, 3), np.asarray(tr_update, np.float32).reshape(-1, 3), per_atom=per_atom)
    cc = DN.correlation(out["sum_q"], scalars)
    out.update(cc=cc, neg_cc=-cc, inclusion=DN.inclusion(out["n_above"], la.shape[0]), n_outside=la.shape[0] - out["n_inside"].astype(np.int64),
               Al=int(la.shape[0]), scalars=scalars, resolution=float(resolution), sigma=sigma, threshold=float(threshold))
    return out


def residue_density(model: engine.Model, rec, lig, rot, tr, dmap, resolution, threshold=1.0):
    """Per ligand residue, over the poses (rot, tr) [n,3]: (keys, mean) - the mean over the poses and over the residue's heavy atoms of
    w * val of the normalised map (channel 0), float64 [n_res] (sterics.residue_of_atoms over the heavy atoms, density.residue_density)."""
    from . import density as DN
    from . import sterics as ST
    dd = ensemble_density(model, rec, lig, np.asarray(rot).reshape(-1, 3), np.asarray(tr).reshape(-1, 3), dmap, resolution, threshold, per_atom=True)
    keys, res = ST.residue_of_atoms(lig["atoms"], ST.heavy_atoms(lig["atoms"]))
    q = DN.residue_density(dd["atom_q"], res, len(keys)).sum(0)
    return keys, DN.units(q) / (np.bincount(res, minlength=len(keys)) * dd["atom_q"].shape[0])


def _check_density(density_map, density_resolution, density_threshold, min_density_cc, rank):
    """None (off) or (rank by it, the map, resolution, threshold, min_density_cc) of a pair driver's density options: density_map is
    density.read_mrc's dict or the path of an MRC file and needs density_resolution; rank "density" needs a map."""
    if density_map is None:
        if rank == "density":
            raise ValueError("rank 'density' needs a density_map")
        if min_density_cc is not None:
            raise ValueError("min_density_cc needs a density_map")
        return None
    from . import density as DN
    dmap = DN.read_mrc(density_map) if isinstance(density_map, (str, os.PathLike)) else dict(density_map)
    g, o, v = DN.check_grid(np.zeros((1,) + tuple(np.shape(dmap["grid"])), np.float32), dmap["origin"], dmap["voxel"])      # the shape and the geometry
    if not np.isfinite(np.asarray(dmap["grid"], np.float64)).all():
        raise ValueError("density_map: the map holds a value that is not finite")
    if density_resolution is None or not (np.isfinite(density_resolution) and density_resolution > 0):
        raise ValueError("a density_map needs density_resolution, finite and > 0 (A)")
    if not np.isfinite(np.float32(density_threshold)):
        raise ValueError("density_threshold must be finite")
    if min_density_cc is not None and not np.isfinite(min_density_cc):
        raise ValueError("min_density_cc must be finite")
    return rank == "density", dmap, float(density_resolution), float(density_threshold), None if min_density_cc is None else float(min_density_cc)


def _pose_density(dd, k):
    cc = float(dd["cc"][k])
    return {"density_cc": cc if np.isfinite(cc) else None, "density_inclusion": float(dd["inclusion"][k]), "density_n_outside": int(dd["n_outside"][k])}


def _density_result(dd, k, opts, bad=None):
    """The density entries of a pair driver's result for the FINAL kept pose k: its three figures, its rank by correlation (1: the highest)
    among the poses the clash filter left, the resolution, sigma and threshold they were taken at."""
    key = _nan_key(dd["neg_cc"], bad)
    summary = dict(_pose_density(dd, k), rank=int(np.nonzero(rank_order(key, len(key)) == k)[0][0]) + 1, resolution=dd["resolution"],
                   sigma=dd["sigma"], threshold=dd["threshold"], ranked_by_density=bool(opts[0]))
    return {"density": summary, "density_data": dd, "index": int(k)}


def rescon_inputs(rec, lig, family):
    """What the residue-contact call takes from two pdbio.backbone_from_atoms dicts: sterics_inputs plus, per chain, the residue index of
    every heavy atom (sterics.residue_of_atoms) and the class of every residue by its name (affinity.IC_CLASS; a name outside the table is
    apolar).  Returns (rec_atoms, rec_res, rec_class, lig_atoms, lig_res, lig_class, center, rec_keys, lig_keys, unclassified):
    unclassified = the number of residues of (receptor, ligand) whose name is outside the table."""
    from . import affinity as AF
    from . import sterics as ST
    ra, la, cen = sterics_inputs(rec, lig, family)
    rk, rres = ST.residue_of_atoms(rec["atoms"], ST.heavy_atoms(rec["atoms"]))
    lk, lres = ST.residue_of_atoms(lig["atoms"], ST.heavy_atoms(lig["atoms"]))
    (rcls, rmiss), (lcls, lmiss) = AF.residue_classes([k[3] for k in rk], AF.IC_CLASS), AF.residue_classes([k[3] for k in lk], AF.IC_CLASS)
    return ra, rres.astype(np.int32), rcls, la, lres.astype(np.int32), lcls, cen, rk, lk, (int(rmiss), int(lmiss))


def ensemble_contacts(model: engine.Model, rec, lig, rot_update, tr_update, cutoff=5.5, per_residue=False, bits=False):
    """Residue contacts by class of trajectories on the GPU (dfm_pose_rescon) from their final (rot_update, tr_update) alone: the residue
    pairs of the two parsed PDB chains with two heavy atoms closer than `cutoff` A.  Returns the dict of Contacts.count plus cutoff,
    rec_keys and lig_keys (the residues the indices of the degree arrays and of contact_bits mean) and unclassified: the residues of
    (receptor, ligand) whose name is not one of the 20 and that count as apolar."""
    inp = rescon_inputs(rec, lig, model.hp.family)
    with model.contacts(*inp[:7], cutoff=cutoff) as h:
        out = h.count(np.asarray(rot_update, np.float32).reshape(-1, 3), np.asarray(tr_update, np.float32).reshape(-1, 3),
                      per_residue=per_residue, bits=bits)
        out.update(cutoff=h.cutoff, rec_keys=inp[7], lig_keys=inp[8], unclassified=inp[9])
    return out


def pose_affinity(model: engine.Model, rec, lig, rot, tr, cutoff=5.5, probe=1.4, sphere_points=128, coef=None, temp_c=25.0, pairs=False,
                  surface=None):
    """The contacts-based affinity estimate (IC-NIS; affinity.dg - coefficients, class tables and reference areas there are starting
    values that are not verified or calibrated, and the surface is this project's own) of the given poses: ensemble_contacts for ic, ONE
    Surface.bsa(per_atom=True) call for every residue's accessible area inside each complex (affinity.complex_residue_sasa) and from it
    the composition of the non-interacting surface (affinity.nis_percent).  Returns the dict of ensemble_contacts plus nis [P,3] (percent
    apolar, polar, charged), nis_apolar, nis_charged, dg_contacts, dg (kcal/mol), kd (M at temp_c) and, with `pairs`, pairs: per pose the
    [n,2] residue pairs (receptor, ligand) as indices into rec_keys / lig_keys.  `surface`: what ensemble_surface(per_atom=True) returned
    for these poses, to be used instead of the surface call (its probe and sphere points then hold)."""
    from . import affinity as AF
    from . import sterics as ST
    c = AF.COEF if coef is None else tuple(float(v) for v in coef)
    rot, tr = np.asarray(rot, np.float32).reshape(-1, 3), np.asarray(tr, np.float32).reshape(-1, 3)
    out = ensemble_contacts(model, rec, lig, rot, tr, cutoff, bits=pairs)
    bd = ensemble_surface(model, rec, lig, rot, tr, probe, sphere_points, per_atom=True) if surface is None else surface
    pr, K = bd["probe"], bd["sphere_points"]
    sasa = []
    for chain, side, keys in ((rec, "rec", out["rec_keys"]), (lig, "lig", out["lig_keys"])):
        res = ST.residue_of_atoms(chain["atoms"], ST.heavy_atoms(chain["atoms"]))[1]
        sasa.append(AF.complex_residue_sasa(bd[side + "_exposed"], bd[side + "_buried"], bd[side + "_radius"], res, len(keys), pr, K))
    nis = AF.nis_percent(sasa[0], sasa[1], [k[3] for k in out["rec_keys"]], [k[3] for k in out["lig_keys"]])
    dgv = AF.dg(out["ic"], nis[:, 0], nis[:, 2], c)
    out.update(nis=nis, nis_apolar=nis[:, 0], nis_charged=nis[:, 2], dg_contacts=AF.dg_contacts(out["ic"], c), dg=dgv, kd=AF.kd(dgv, temp_c),
               coef=c, probe=pr, sphere_points=K)
    if pairs:
        out["pairs"] = [AF.pairs_of(b) for b in out.pop("contact_bits")]
    return out


AFFINITY_SURFACE = (1.4, 128)      # probe and sphere points of the surface behind the affinity estimate of the pair drivers


def _check_affinity(affinity, affinity_cutoff):
    """None (off) or (cutoff,) of a pair driver's affinity options."""
    if not affinity:
        return None
    from . import affinity as AF
    return (AF.check_cutoff(affinity_cutoff),)


def _pose_affinity(ad, k):
    fin = lambda v: float(v) if np.isfinite(v) else None
    return {"ic": [int(v) for v in ad["ic"][k]], "n_pairs": int(ad["n_pairs"][k]), "n_rec_res": int(ad["n_rec_res"][k]),
            "n_lig_res": int(ad["n_lig_res"][k]), "nis_apolar": fin(ad["nis_apolar"][k]), "nis_charged": fin(ad["nis_charged"][k]),
            "dg": fin(ad["dg"][k]), "kd": fin(ad["kd"][k]), "cutoff": float(ad["cutoff"])}


def _affinity_result(ad, k):
    """The `affinity` entries of a pair driver's result for the kept pose k: none without the option."""
    if ad is None:
        return {}
    return {"affinity": _pose_affinity(ad, k), "affinity_data": ad, "index": int(k)}


def hbond_inputs(rec, lig, family):
    """What the hydrogen-bond call takes from two pdbio.backbone_from_atoms dicts: the polar atoms of both chains (hbonds.polar_atoms over
    sterics.heavy_atoms: coordinates, antecedents, roles, residues) and the centre of sterics_inputs.  Returns (rec_polar, lig_polar,
    center)."""
    from . import hbonds as HB
    return HB.polar_atoms(rec["atoms"]), HB.polar_atoms(lig["atoms"]), sterics_inputs(rec, lig, family)[2]


def ensemble_hbonds(model: engine.Model, rec, lig, rot_update, tr_update, hb_cutoff=3.5, min_angle=90.0, salt_cutoff=4.0, per_atom=False):
    """Interface hydrogen bonds and salt bridges of trajectories on the GPU (dfm_pose_hbonds) from their final (rot_update, tr_update)
    alone: heavy-atom criteria over the polar atoms of the two parsed PDB chains (hbonds.py; HIS is donor, acceptor and cation; no
    agreement with any published tool is claimed).  Returns the dict of HBonds.count plus hb_cutoff, min_angle, salt_cutoff, rec_polar /
    lig_polar (the polar_atoms dicts the per-atom arrays are in the order of) and untyped: the polar atoms of (receptor, ligand) whose
    antecedent is missing from the file and that therefore take no part."""
    rp, lp, cen = hbond_inputs(rec, lig, model.hp.family)
    with model.hbonds(rp, lp, cen, hb_cutoff, min_angle, salt_cutoff) as h:
        out = h.count(np.asarray(rot_update, np.float32).reshape(-1, 3), np.asarray(tr_update, np.float32).reshape(-1, 3), per_atom=per_atom)
        out.update(hb_cutoff=h.hb_cutoff, min_angle=h.min_angle, salt_cutoff=h.salt_cutoff, rec_polar=rp, lig_polar=lp,
                   untyped=(int(rp["untyped"]), int(lp["untyped"])))
    return out


def unsatisfied_polar(hd, bd, percent=100):
    """n_unsat [P] int32: the donors and acceptors of both chains that each pose buries completely (`percent` of the points exposed in
    isolation) and leaves without a hydrogen bond (hbonds.unsatisfied).  hd: ensemble_hbonds(per_atom=True); bd:
    ensemble_surface(per_atom=True) of the same poses."""
    from . import hbonds as HB
    n = 0
    for side in ("rec", "lig"):
        pa = hd[side + "_polar"]
        n = n + HB.unsatisfied(pa["role"], bd[side + "_exposed"][pa["index"]], bd[side + "_buried"][:, pa["index"]], hd[side + "_hb"],
                               percent)["n_unsat"]
    return n


def residue_hbonds(model: engine.Model, rec, lig, rot, tr, hb_cutoff=3.5, min_angle=90.0, salt_cutoff=4.0):
    """Per residue of ONE pose: ((receptor keys, ligand keys), (receptor bonds, ligand bonds), (receptor salt-bridge atom pairs,
    ligand ...)) - the per-atom counts summed over each residue's polar atoms (hbonds.residue_bonds)."""
    from . import hbonds as HB
    hd = ensemble_hbonds(model, rec, lig, np.asarray(rot).reshape(1, 3), np.asarray(tr).reshape(1, 3), hb_cutoff, min_angle, salt_cutoff,
                         per_atom=True)
    keys, hb, sb = [], [], []
    for side in ("rec", "lig"):
        pa = hd[side + "_polar"]
        keys.append(pa["keys"])
        hb.append(HB.residue_bonds(hd[side + "_hb"][0], pa["res"], pa["n_res"]))
        sb.append(HB.residue_bonds(hd[side + "_sb"][0], pa["res"], pa["n_res"]))
    return keys, hb, sb


def _check_hbonds(hbonds, hbond_cutoff, hbond_angle, salt_cutoff):
    """None (off) or (hb_cutoff, min_angle, salt_cutoff) of a pair driver's hydrogen-bond options."""
    if not hbonds:
        return None
    from . import hbonds as HB
    HB.min_cos2(hbond_angle)
    return HB.check_cutoffs(hbond_cutoff, salt_cutoff)[0], float(hbond_angle), HB.check_cutoffs(hbond_cutoff, salt_cutoff)[1]


def _pose_hbonds(hd, k):
    out = {"n_hbond": int(hd["n_hbond"][k]), "hb_bb_bb": int(hd["hb_kind"][k, 0]), "hb_bb_sc": int(hd["hb_kind"][k, 1]),
           "hb_sc_sc": int(hd["hb_kind"][k, 2]), "n_salt": int(hd["n_salt"][k])}
    if "n_unsat" in hd:
        out["n_unsat"] = int(hd["n_unsat"][k])
    return out


def _hbonds_result(hd, k):
    """The hydrogen-bond entries of a pair driver's result for the kept pose k."""
    return dict(_pose_hbonds(hd, k), hbond_data=hd, index=int(k))


def _check_sterics(clash_screen, clash_filter, clash_cutoff, contact_cutoff):
    """None (off) or (filter, clash cutoff, contact cutoff) of a pair driver's screen options."""
    if not (clash_screen or clash_filter):
        return None
    from .sterics import check_cutoffs
    cc, ct = check_cutoffs(clash_cutoff, contact_cutoff)
    return bool(clash_filter), cc, ct


def _screen(model, rec, lig, cols, opts):
    """The screen of a pair driver's trajectories.  Returns (sterics data, bad): bad [n] bool = the poses --clash-filter removes
    (CAPRI's flags), or None when nothing is removed - the filter is off, nothing is flagged, or every pose would go (`fallback`)."""
    filtered, clash_cutoff, contact_cutoff = opts
    sd = ensemble_sterics(model, rec, lig, cols["rot_update"], cols["tr_update"], clash_cutoff, contact_cutoff)
    sd["filtered"], sd["fallback"] = filtered, bool(filtered and sd["flags"].all())
    bad = sd["flags"].copy() if filtered and sd["flags"].any() and not sd["fallback"] else None
    return sd, bad


def _kept(pick, bad, *cols):
    """pick(*cols) -> index, over the poses that are not `bad`."""
    if bad is None:
        return int(pick(*cols))
    idx = np.nonzero(~bad)[0]
    return int(idx[int(pick(*(np.asarray(c)[idx] for c in cols)))])


def _nan_key(key, bad):
    """The clustering key with NaN on the removed poses (cluster.rank_order sorts NaN last)."""
    return key if bad is None or key is None else np.where(bad, np.nan, np.asarray(key, np.float64))


def _pose_sterics(sd, k):
    m = float(sd["min_dist"][k])
    return {"n_clash": int(sd["n_clash"][k]), "n_contact": int(sd["n_contact"][k]), "min_dist": m if np.isfinite(m) else None,
            "flagged": bool(sd["flags"][k])}


def _sterics_result(sd, k):
    """The `sterics` entries of a pair driver's result for the kept pose k: none without the screen."""
    if sd is None:
        return {}
    fin = lambda v: float(v) if np.isfinite(v) else None
    return {"sterics": dict(_pose_sterics(sd, k), threshold=fin(sd["threshold"]), ensemble_mean=fin(sd["ensemble_mean"]),
                            ensemble_std=fin(sd["ensemble_std"]), clash_cutoff=sd["clash_cutoff"], contact_cutoff=sd["contact_cutoff"],
                            filtered=sd["filtered"], fallback=sd["fallback"]),
            "sterics_data": sd, "index": int(k)}


def _remarks(sd, k):
    """The REMARK line of a written model: none without the screen."""
    if sd is None:
        return None
    return [f"dfmdock_amd sterics n_clash {int(sd['n_clash'][k])} n_contact {int(sd['n_contact'][k])} "
            f"(heavy-atom pairs below {sd['clash_cutoff']:g} / {sd['contact_cutoff']:g} A)"]


DISTOGRAM_T = 1e-3      # time of the distogram evaluation of final poses: the end of the sampler's grid


def ensemble_distogram(gx: engine.Complex, rot_update, tr_update, t=DISTOGRAM_T, precision="mfma16", max_batch=256, contact_bins=7,
                       near_cutoff=None, maps=False, seed=0):
    """The distogram head (family 1) of trajectories from their final (rot_update, tr_update) alone, on the open handle `gx`
    (Complex.distogram, dfm_score_distogram): the poses are rebuilt from the input backbone (cluster.rebuild_backbone) and evaluated at
    time `t` in chunks of max_batch.  Returns nll, nll_near, exp_contacts (float64 [P]), n_near (int [P]), t, contact_bins and, with
    `maps`, pcontact_mean [R,L] (the mean over ALL P poses, added in index order in double across the chunks) and edist [P,R,L]."""
    rot, tr = np.asarray(rot_update, np.float32).reshape(-1, 3), np.asarray(tr_update, np.float32).reshape(-1, 3)
    P, mb = rot.shape[0], max(1, int(max_batch))
    out = {k: [] for k in ("nll", "nll_near", "n_near", "exp_contacts")}
    psum, ed = np.zeros((gx.R, gx.L), np.float64), []
    for p0 in range(0, P, mb):
        poses = rebuild_backbone(gx.lig_pos0, rot[p0:p0 + mb], tr[p0:p0 + mb], gx.model.hp.family)
        r = gx.distogram(poses, t, seed=seed + p0, maps=("pcontact", "edist") if maps else (), contact_bins=contact_bins,
                         near_cutoff=near_cutoff, **engine.precision_kwargs(precision))
        for k in out:
            out[k].append(r[k])
        if maps:
            for b in range(poses.shape[0]):
                psum += r["pcontact"][b]
            ed.append(r["edist"])
    res = {k: np.concatenate(v).astype(np.int64 if k == "n_near" else np.float64) for k, v in out.items()}
    res.update(t=float(t), contact_bins=int(contact_bins))
    if maps:
        res.update(pcontact_mean=psum / P, edist=np.concatenate(ed, 0))
    return res


def _check_distogram(model, distogram, rank, distogram_t, distogram_maps, max_batch):
    """None (off) or (rank by it, t, maps, max_batch) of a pair driver's distogram options; rank "distogram" implies them.  The head
    exists in the second model family only: anything else is refused here, before a trajectory is sampled."""
    if not distogram and rank != "distogram" and not distogram_maps:
        return None
    if model.hp.family != 1:
        raise ValueError("the distogram head (distogram / rank 'distogram') needs a family-1 checkpoint: EGNN_Net has to_dist, Score_Net "
                         "does not")
    t = float(distogram_t)
    if not (0.0 < t <= 1.0):
        raise ValueError(f"distogram_t must be in (0, 1], got {distogram_t}")
    return rank == "distogram", t, bool(distogram_maps), int(max_batch)


def _pose_distogram(dd, k):
    fin = lambda v: float(v) if np.isfinite(v) else None
    return {"dist_nll": fin(dd["nll"][k]), "dist_nll_near": fin(dd["nll_near"][k]), "exp_contacts": fin(dd["exp_contacts"][k])}


def _distogram_result(dd, k, opts, bad=None):
    """The distogram entries of a pair driver's result for the FINAL kept pose k."""
    nll = _nan_key(dd["nll"], bad)
    summary = dict(_pose_distogram(dd, k), n_near=int(dd["n_near"][k]), rank=int(np.nonzero(rank_order(nll, len(nll)) == k)[0][0]) + 1,
                   t=dd["t"], contact_bins=dd["contact_bins"], ranked_by_distogram=bool(opts[0]))
    return {"distogram": summary, "distogram_data": dd, "index": int(k)}


def _check_rank(rank, consensus_top):
    if rank not in ("energy", "consensus", "interface", "distogram", "pairpot", "density"):
        raise ValueError(f"rank must be 'energy', 'consensus', 'interface', 'distogram', 'pairpot' or 'density', got {rank!r}")
    if not (0.0 < float(consensus_top) <= 1.0):
        raise ValueError(f"consensus_top must be in (0, 1], got {consensus_top}")


def _consensus_result(cd, k, opts, ranked_by="energy"):
    """The `consensus` entries of a pair driver's result for the FINAL kept pose k; `ranked_by`: the rule that chose it (`fallback`: not rank "consensus" itself)."""
    s = float(cd["consensus"][k])
    summary = {"score": None if np.isnan(s) else s, "rank": int(np.nonzero(rank_order(-cd["consensus"], len(cd["consensus"])) == k)[0][0]) + 1,
               "n_contacts": int(cd["n_contacts"][k]), "M": int(cd["M"]), "cutoff": float(cd["cutoff"]), "ranked_by": ranked_by,
               "fallback": opts[0] == "consensus" and ranked_by != "consensus"}
    return {"consensus": summary, "consensus_data": cd, "index": int(k)}


def checked_precision(gx: engine.Complex, precision: str, name: str, selfcheck=True, on_fail="fp32", log=None, seed=0):
    """Once per complex, before any trajectory: dfm_complex_selfcheck of the 16-bit engine on the complex's own pose (fp32 vs
    16-bit on the same graphs + fp16 range telemetry), printed as one line.  A failed check - activations outside the fp16 range
    or deviations beyond SURVEY 8(d)'s gates, i.e. a checkpoint this engine's precision plan does not hold for - switches the
    complex to the fp32 ENGINE (`on_fail="fp32"`: slower, the reference's own arithmetic, still the HIP path), raises
    (`"raise"`) or only warns (`"warn"`).  Returns (precision to use, the check's dict or None)."""
    import sys
    if not selfcheck or engine.canonical_precision(precision) == "fp32":
        return precision, None
    r = gx.selfcheck(precision=precision, seed=seed)
    line = engine.format_selfcheck(r, name)
    (log or (lambda m: print(m, file=sys.stderr, flush=True)))(line)
    if not r["ok"]:
        if on_fail == "raise":
            raise RuntimeError(line)
        if on_fail == "fp32":
            (log or (lambda m: print(m, file=sys.stderr, flush=True)))(f"selfcheck {name}: running this complex on the fp32 engine")
            return "fp32", r
    return precision, r


class _Prepared:
    """One complex ready to sample: its handle, the pose it was created on and everything derived from that pose alone."""
    __slots__ = ("ci", "c", "gx", "N", "rec_pos", "lig_pos", "native", "precision", "check", "ms", "restraints")


def _prepare(model, c, ci, rot_seed, global_rotation, precision, selfcheck, on_selfcheck_fail, seed, log=None,
             restraints=None) -> _Prepared:
    """Stage 1 of run_set (host + a little device work on the new handle's own stream): loader semantics, handle, self-check."""
    import time
    t0 = time.perf_counter()
    p = _Prepared()
    p.ci, p.c = ci, c
    rec_pos, lig_pos = input_pose(c, rot_seed, global_rotation)
    p.rec_pos, p.lig_pos = rec_pos, lig_pos
    p.gx = engine.Complex(model, c["rec_x"], c["lig_x"], rec_pos, lig_pos)
    p.N = p.gx.N
    p.restraints = restraints      # residue indices: unchanged by the global rotation
    if restraints is not None:
        p.gx.set_restraints(restraints)
    p.native = NativeContext((rec_pos, lig_pos))
    p.precision, p.check = checked_precision(p.gx, precision, str(c.get("id", ci)), selfcheck, on_selfcheck_fail, log=log, seed=seed)
    p.ms = {"prepare": (time.perf_counter() - t0) * 1e3}
    return p


def _sample(p: _Prepared, t_lo, t_hi, num_steps, seed, max_batch, trace, sampler_kw, keep_open=False):
    """Stage 2: the trajectories of this rank's share, in batches of at most max_batch.  The results are host arrays, so the
    handle (and its ~GB of device workspace) is released HERE, not after the host-side stage 3: however far the metrics /
    trajectory-PDB stage falls behind, the live handles are bounded by the prepare gate + the samplers."""
    import time
    t0 = time.perf_counter()
    batches, done = [], t_lo
    try:
        while done < t_hi:
            b = min(max_batch, t_hi - done)
            r = p.gx.sample(B=b, num_steps=num_steps, seed=seed * 100003 + p.ci * 1009 + done, trace=trace,
                            restraints=p.restraints is not None, **engine.precision_kwargs(p.precision), **sampler_kw)
            if p.restraints is not None:      # the restraint terms of the final poses, on the sampler's own kernel
                ev = p.gx.restraint_eval(r["lig_pos"])
                r["restraint_energy"], r["restraints_satisfied"] = ev["energy"], ev["n_satisfied"]
            batches.append((done, b, r))
            done += b
    finally:
        if not keep_open:
            p.gx.close()
    p.ms["sample"] = (time.perf_counter() - t0) * 1e3
    return batches


def _post(p: _Prepared, batches, traj_dir, model=None, metrics="host", step_metrics=False, eps=1e-3):
    """Stage 3: per-trajectory metrics against the native pose (inference_mlsb.py:232-262), trajectory PDBs, records.  metrics "host":
    one compute_metrics per final pose (numpy, the reference's arithmetic); "gpu": the final poses of the complex in ONE
    dfm_pose_metrics call, and with `step_metrics` every frame of every trace in one call per batch (returned as the third value)."""
    import time
    t0 = time.perf_counter()
    c, rows, records, steps = p.c, [], [], []
    gm = None
    if metrics == "gpu" and batches:
        with model.native(p.rec_pos, p.lig_pos) as nat:
            gm = nat.metrics(np.concatenate([r["lig_pos"] for _, _, r in batches], 0))
            if step_metrics:
                for done, b, r in batches:
                    S = r["trace_pose"].shape[1]
                    sm = nat.metrics(r["trace_pose"].reshape(b * S, -1, 3, 3))
                    ts = np.linspace(1.0, eps, S)
                    for k in range(b):
                        for st in range(S):
                            steps.append({"id": c.get("id", str(p.ci)), "index": str(done + k), "step": st, "t": float(ts[st]),
                                          **{f: float(sm[f][k * S + st]) for f in METRIC_FIELDS}})
    at = 0
    for done, b, r in batches:
        for k in range(b):
            if gm is not None:
                m = {f: float(gm[f][at + k]) for f in METRIC_FIELDS}
            else:
                m = compute_metrics((p.rec_pos, r["lig_pos"][k]), (p.rec_pos, p.lig_pos), p.native)
            rows.append({"id": c.get("id", str(p.ci)), "index": str(done + k), **m, "energy": float(r["energy"][k]),
                         "num_clashes": int(r["num_clashes"][k])})
            if p.restraints is not None:
                rows[-1].update(restraint_energy=float(r["restraint_energy"][k]), restraints_satisfied=int(r["restraints_satisfied"][k]))
            if traj_dir is not None and "rec_seq" in c:
                os.makedirs(traj_dir, exist_ok=True)
                frames = r["trace_pose"][k]
                pdbio.write_trajectory_pdb(os.path.join(traj_dir, f"{c.get('id', p.ci)}_p{done + k}.pdb"),
                                           [p.rec_pos] * len(frames), frames, c["rec_seq"], c["lig_seq"])
        at += b
        records.append(D.make_records(p.ci, np.arange(done, done + b), r))
    p.ms["post"] = (time.perf_counter() - t0) * 1e3
    if step_metrics:
        return rows, records, steps
    return rows, records


def run_set(model: engine.Model, complexes, num_samples=40, num_steps=40, seed=0, precision="mfma16", global_rotation=True,
            out_csv=None, traj_dir=None, max_batch=256, selfcheck=True, on_selfcheck_fail="fp32", checks_out=None,
            overlap=True, samplers=2, timings_out=None, log=None, canary=True, canary_out=None, restraints_by_id=None,
            cluster_radius=None, cluster_rule="energy", top_k=10, metrics="host", step_metrics=False, step_csv=None, steps_out=None,
            consensus=False, consensus_top=1.0, consensus_cutoff=5.5, **sampler_kw):
    """Sample `num_samples` trajectories for every complex dict (id, rec_x, lig_x, rec_pos, lig_pos[, rec_seq, lig_seq]);
    returns the metric rows of this rank's share; rank 0 writes the gathered CSV when `out_csv` is given.  Every complex is
    self-checked first (checked_precision); `checks_out` (a list) collects {id, precision used, check dict}.

    The reference's loop (src/inference_mlsb.py:415-439 over :188-262) is serial: load, sample, score, next.  Here the three
    stages of a complex run on three host threads (`overlap=True`): while complex k samples on its handle's stream, complex k+1
    is created and self-checked on ITS handle's stream (dfmdock_amd.h: handles are independent) and complex k-1's 40 Kabsch
    fits / CSV rows are computed on the host; `samplers` complexes sample concurrently (default 2: a B = 40 batch of a 200-400-residue
    complex does not fill 256 CUs; measured +4 ... +8 % over one sampler on the C4 set, profiles/r05_c4.txt; 3 buys nothing more).  Results do not depend on any of this: a trajectory is a pure function of (seed, complex,
    trajectory index), so the rows equal the serial driver's (`overlap=False`) bit for bit.  `timings_out` (a list) collects
    per-complex {id, N, prepare, sample, post} milliseconds; `log` receives the self-check lines
    (default: stderr).

    `canary` (overlapped driver only): r05 found - and fenced, without naming the mechanism - a silent miscompute between two handles
    running at once (profiles/r05_concurrency.txt; tests/test_gpu_concurrency.py holds the shipped build to 0 deviations).  As a
    run-time tripwire on whatever box / ROCm this runs on, the cheapest complex that sampled with others in flight is sampled AGAIN
    after the pipeline has drained, alone, and compared bit for bit; on a mismatch the whole share is re-run by the serial driver and
    those rows are returned (`canary_out`, a dict, receives {checked, id, ok, reran_serial}).

    `restraints_by_id` ({complex id: [restraints.RestraintGroup]}): the listed complexes sample with their interface restraints
    (DFM_F_RESTRAINTS; every rank holds the set, the canary re-sample uses it too) and every row gains `restraint_energy` and
    `restraints_satisfied` of its final pose (complexes without an entry: 0 groups, both 0).  Without it the rows and the CSV keep
    the reference schema.

    `cluster_radius` (A): the trajectories of every complex are clustered by ligand RMSD (cluster_trajectories; key: energy, rule
    `cluster_rule`, at most `top_k` clusters) and every row gains `cluster` (-1: in none of them) and `is_center`.  This runs where all
    trajectories of a complex are present: on the owning rank when complexes are sharded, on rank 0 after the record gather when
    trajectories are split (the assignment then reaches every rank's rows).

    `metrics`: "host" (default; one numpy compute_metrics per final pose, the CSV of every earlier version byte for byte) or "gpu" (the
    final poses of a complex in one dfm_pose_metrics call: the same definition evaluated in fp64 on the device, equal to the host's
    values to ~1e-12 relative, so the CSV differs in the last printed digits).  `step_metrics=True` (needs metrics="gpu"; takes the
    trace) evaluates the pose after EVERY step of every trajectory: the long table {id, index, step, t, c_rmsd, i_rmsd, l_rmsd, fnat,
    DockQ} (t = the time of the step taken, linspace(1, eps, num_steps)[step]) is appended to `steps_out` (a list; this rank's share)
    and written to `step_csv` by rank 0.

    `consensus`: every row gains `consensus` (the consensus contact score of the trajectory within its complex's ensemble, NaN without
    a contact) and `n_contacts` (ensemble_consensus: contacts below `consensus_cutoff` A, members = the best `consensus_top` fraction by
    energy).  Like clustering it runs where all trajectories of a complex are present."""
    if consensus:
        _check_rank("energy", consensus_top)
    if metrics not in ("host", "gpu"):
        raise ValueError(f"metrics must be 'host' or 'gpu', got {metrics!r}")
    step_metrics = bool(step_metrics) or step_csv is not None
    if step_metrics and metrics != "gpu":
        raise ValueError("step_metrics evaluates num_samples x num_steps poses per complex: it needs metrics='gpu'")
    if cluster_radius is not None and cluster_rule not in ("energy", "size"):
        raise ValueError(f"cluster_rule must be 'energy' or 'size', got {cluster_rule!r}")
    rank, _, world = D.dist_env()
    complexes = list(complexes)
    split_trajectories = world > 1 and len(complexes) < 2 * world
    if split_trajectories:      # (complex, trajectory block) work items: rank r takes block r of every complex
        share = list(range(len(complexes)))
        t_lo, t_hi = D.shard_range(num_samples, world, rank)
    else:
        # longest-first over the estimated sampling time of each complex (affine in N: a B = 40 call has a fixed cost no batch fills)
        share = D.assign_work([D.complex_cost(c["rec_x"].shape[0] + c["lig_x"].shape[0], num_samples) for c in complexes], world)[rank]
        t_lo, t_hi = 0, num_samples
    rng = np.random.default_rng(seed)
    rots = [rng.integers(0, 2 ** 31) for _ in complexes]      # per-complex streams, identical on every rank
    if t_hi <= t_lo:
        share = []
    trace = traj_dir is not None or step_metrics
    if step_metrics and traj_dir is None:      # the trace is taken for its poses alone: the step evaluations stay those of an untraced run
        sampler_kw.setdefault("step_energy", False)
    step_rows = []

    def post(p, batches):
        if metrics == "host":
            return _post(p, batches, traj_dir)      # the path of every earlier version, untouched
        out = _post(p, batches, traj_dir, model, metrics, step_metrics, float(sampler_kw.get("eps", 1e-3)))
        if step_metrics:
            step_rows.extend(out[2])
        return out[0], out[1]

    def restraints_of(ci):      # keyword arguments of _prepare: none without restraints
        if restraints_by_id is None:
            return {}
        return {"restraints": list(restraints_by_id.get(complexes[ci].get("id", str(ci)), []))}

    def prep(ci):
        return _prepare(model, complexes[ci], ci, rots[ci], global_rotation, precision, selfcheck, on_selfcheck_fail, seed, log,
                        **restraints_of(ci))

    def samp(p):
        return _sample(p, t_lo, t_hi, num_steps, seed, max_batch, trace, sampler_kw)

    done = []      # (prepared, rows, records) in share order
    if not overlap or len(share) < 2:
        for ci in share:
            p = prep(ci)
            rows_c, recs_c = post(p, samp(p))
            done.append((p, rows_c, recs_c))
    else:
        import threading
        from concurrent.futures import ThreadPoolExecutor
        ahead = threading.Semaphore(samplers + 1)      # handles prepared but not yet sampling: bounds the device memory in flight

        def prep_gated(ci):
            ahead.acquire()
            try:
                return prep(ci)
            except BaseException:
                ahead.release()
                raise

        def samp_of(fp):
            p = fp.result()
            ahead.release()
            return p, samp(p)

        # the canary complex: cheapest of those that are neither first nor last of the share (so something else was always in flight)
        inner = share[1:-1] if len(share) > 2 else share[-1:]
        canary_ci = min(inner, key=lambda ci: complexes[ci]["rec_x"].shape[0] + complexes[ci]["lig_x"].shape[0]) if canary else None
        canary_ref = {}

        def post_of(fs):
            p, batches = fs.result()
            if p.ci == canary_ci:
                canary_ref["batches"], canary_ref["precision"] = batches, p.precision
            rows_c, recs_c = post(p, batches)
            return p, rows_c, recs_c

        with ThreadPoolExecutor(1, thread_name_prefix="dfm-prep") as ex_prep, \
                ThreadPoolExecutor(max(1, int(samplers)), thread_name_prefix="dfm-sample") as ex_samp, \
                ThreadPoolExecutor(1, thread_name_prefix="dfm-post") as ex_post:
            f_prep = [ex_prep.submit(prep_gated, ci) for ci in share]
            f_samp = [ex_samp.submit(samp_of, f) for f in f_prep]
            f_post = [ex_post.submit(post_of, f) for f in f_samp]
            try:
                done = [f.result() for f in f_post]
            except BaseException:
                for f in f_prep + f_samp + f_post:
                    f.cancel()
                for _ in share:      # un-block a prepare stage parked on the gate
                    ahead.release()
                raise
        if canary_ci is not None and "batches" in canary_ref:
            again = _prepare(model, complexes[canary_ci], canary_ci, rots[canary_ci], global_rotation, canary_ref["precision"], False,
                             on_selfcheck_fail, seed, log, **restraints_of(canary_ci))
            solo = samp(again)
            same = len(solo) == len(canary_ref["batches"]) and all(
                all(np.array_equal(ra[k], rb[k]) for k in ("lig_pos", "energy", "num_clashes", "rot_update", "tr_update"))
                for (_, _, ra), (_, _, rb) in zip(solo, canary_ref["batches"]))
            info = {"checked": True, "id": complexes[canary_ci].get("id", str(canary_ci)), "ok": bool(same), "reran_serial": False}
            if not same:
                import sys
                (log or (lambda m: print(m, file=sys.stderr, flush=True)))(
                    f"run_set canary: complex {info['id']} sampled next to other handles differs from the same complex sampled alone - "
                    "concurrent handles are NOT independent on this system; re-running this rank's share serially")
                done = []
                del step_rows[:]
                for ci in share:
                    p = prep(ci)
                    rows_c, recs_c = post(p, samp(p))
                    done.append((p, rows_c, recs_c))
                info["reran_serial"] = True
            if canary_out is not None:
                canary_out.update(info)
    rows, records = [], []
    for p, rows_c, recs_c in done:
        rows += rows_c
        records += recs_c
        if checks_out is not None:
            checks_out.append({"id": p.c.get("id", str(p.ci)), "precision": p.precision, "selfcheck": p.check})
        if timings_out is not None:
            timings_out.append({"id": p.c.get("id", str(p.ci)), "N": p.N, **p.ms})
    recs = np.concatenate(records, 0) if records else np.zeros((0, D.RECORD_WIDTH), np.float32)
    gathered = D.gather_records(recs) if world > 1 or len(recs) else recs
    ranked = D.rank_by_energy(gathered) if world > 1 or len(recs) else {}

    def per_complex(fields, fn):
        """Every row's columns `fields` from fn(ci, trajectory indices, energy, rot_update, tr_update) -> one tuple of values per trajectory,
        given all trajectories of complex ci in index order.  fn runs where they are all present: on the owning rank when complexes are
        sharded, on rank 0 after the record gather when trajectories are split (the values then reach every rank's rows)."""
        mine = list(range(len(complexes))) if split_trajectories else [p.ci for p, _, _ in done]
        values = {}
        if not split_trajectories or rank == 0:
            for ci in mine:
                r = gathered[gathered[:, 0] == ci]
                if not len(r):
                    continue
                r = r[np.argsort(r[:, 1], kind="stable")]
                t = r[:, 1].astype(int)      # D.make_records: complex, trajectory, energy, num_clashes, rot_update[3], tr_update[3]
                cid = complexes[ci].get("id", str(ci))
                for ti, v in zip(t, fn(ci, t, r[:, 2], r[:, 4:7], r[:, 7:10])):
                    values[f"{cid}/{ti}"] = v
        if split_trajectories and world > 1:
            values = D.gather_objects(values)[0]
        for row in rows:
            row.update(zip(fields, values[f"{row['id']}/{row['index']}"]))

    def clusters(ci, t, energy, rot_update, tr_update):
        lig0 = input_pose(complexes[ci], rots[ci], global_rotation)[1]
        cl = cluster_trajectories(model, lig0, rot_update, tr_update, energy, cluster_radius, cluster_rule, top_k)
        centers = set(int(t[c]) for c in cl["center"])
        return [(int(k), int(ti in centers)) for ti, k in zip(t, cl["cluster_of"])]

    def consensus_scores(ci, t, energy, rot_update, tr_update):
        rec0, lig0 = input_pose(complexes[ci], rots[ci], global_rotation)
        cd = ensemble_consensus(model, rec0, lig0, rot_update, tr_update, energy, consensus_cutoff, consensus_top)
        return [(float(sc), int(nc)) for sc, nc in zip(cd["consensus"], cd["n_contacts"])]

    def write_csv(path, table, fields, order):
        """Rank 0 writes the rows of every rank in `order`."""
        table = _gather_rows(table, world)
        if rank == 0:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w", newline="") as f:
                w = csv.DictWriter(f, fieldnames=fields)
                w.writeheader()
                for row in sorted(table, key=order):
                    w.writerow(row)

    if cluster_radius is not None:
        per_complex(CLUSTER_FIELDS, clusters)
    if consensus:
        per_complex(CONSENSUS_FIELDS, consensus_scores)
    if out_csv is not None:
        write_csv(out_csv, rows, CSV_FIELDS + (RESTRAINT_FIELDS if restraints_by_id is not None else []) +
                  (CLUSTER_FIELDS if cluster_radius is not None else []) + (CONSENSUS_FIELDS if consensus else []),
                  lambda x: (x["id"], int(x["index"])))
    if steps_out is not None:
        steps_out.extend(step_rows)
    if step_csv is not None:
        write_csv(step_csv, step_rows, STEP_FIELDS, lambda x: (x["id"], int(x["index"]), x["step"]))
    return rows, ranked


def _gather_rows(rows, world):
    if world == 1:
        return rows
    return [r for part in D.gather_objects(rows) for r in part]


def native_metrics(model: engine.Model, native, rec_bb, lig_poses):
    """Docking metrics of ligand poses lig_poses [P,L,3,3] of a pair whose receptor backbone is rec_bb [R,3,3], against `native` =
    (receptor [R,3,3], ligand [L,3,3]) given in ANY frame: the pair's receptor travels with every pose (rec_pos of dfm_pose_metrics), so
    the fits take care of the frame.  The native is matched to the pair by residue order.  Returns one {c_rmsd, ..., DockQ} per pose."""
    nr, nl = (np.asarray(x, np.float32).reshape(-1, 3, 3) for x in native)
    rec_bb, lig_poses = np.asarray(rec_bb, np.float32).reshape(-1, 3, 3), np.asarray(lig_poses, np.float32)
    lig_poses = lig_poses.reshape(lig_poses.shape[0], -1, 3, 3)
    _check_native((nr, nl), rec_bb.shape[0], lig_poses.shape[1])
    with model.native(nr, nl) as nat:
        m = nat.metrics(lig_poses, np.repeat(rec_bb[None], lig_poses.shape[0], 0))
    return [{k: float(m[k][p]) for k in METRIC_FIELDS} for p in range(lig_poses.shape[0])]


def _check_native(native, n_rec, n_lig):
    """The native must have the input's residue counts (the pair drivers ask before any sampling)."""
    nr, nl = (np.asarray(x).reshape(-1, 3, 3) for x in native)
    if nr.shape[0] != n_rec or nl.shape[0] != n_lig:
        raise ValueError(f"the native has {nr.shape[0]} receptor / {nl.shape[0]} ligand residues, the input pair {n_rec} / {n_lig}: they must match residue by residue")


def _center(model):
    """The centre pdbio.apply_pose_all_atom rotates the ligand about for this model family."""
    return "all_atoms" if model.hp.family == 1 else "ca"


def _check_symmetry(rec, lig, symmetry, symmetry_params, tolerance):
    """None (no symmetry) or {n, params, tolerance, input_rmsd} of dock_pair / refine_pair's `symmetry`, checked before anything is
    sampled: the two inputs must be ONE chain each, of one sequence, and rigid images of each other within `tolerance` A (the Kabsch
    rmsd over all backbone atoms - rescore's --fit-tolerance rule)."""
    if symmetry is None:
        if symmetry_params is not None:
            raise ValueError("symmetry_params needs symmetry (the order n of the assembly)")
        return None
    from . import symmetry as SY
    n = SY.check_order(symmetry)
    if not (np.isfinite(tolerance) and tolerance >= 0):
        raise ValueError("symmetry_tolerance must be finite and >= 0")
    for side, c in (("receptor", rec), ("ligand", lig)):
        ids = pdbio._chain_ids(c["residues"])
        if len(ids) > 1:
            raise ValueError(f"symmetry: the {side} has more than one chain id ({''.join(ids)}): a Cn assembly is built from ONE chain")
    if rec["seq"] != lig["seq"]:
        raise ValueError(f"symmetry: receptor and ligand sequences differ ({len(rec['seq'])} and {len(lig['seq'])} residues): "
                         "a Cn assembly needs two copies of the same chain")
    _, _, rmsd = SY.fit_transform(rec["bb_coords"], lig["bb_coords"])
    if not rmsd <= tolerance:
        raise ValueError(f"symmetry: the two input monomers are no rigid images of each other: Kabsch rmsd {rmsd:.3g} A over the backbone "
                         f"is above symmetry_tolerance = {tolerance} A")
    return {"n": n, "params": symmetry_params, "tolerance": float(tolerance), "input_rmsd": float(rmsd)}


def _set_symmetry(model, gx, sym):
    """Stores the symmetry of a checked `sym` on the handle; a model with the 67th position channel gets its homomer flag (a 66-channel
    model has no such channel: the entry point refuses it)."""
    if model.hp.positional_embed_dim == 67:
        gx.set_homomer(True)
    gx.set_symmetry(sym["n"], sym["params"])


def _file_center(model, lig):
    """The point pdbio.apply_pose_all_atom (and every dfm_pose_* call of the drivers) rotates this ligand about, float64 [3]."""
    if model.hp.family == 1:
        return np.asarray(lig["aa_coords"], np.float64).reshape(-1, 3).mean(0)
    return np.asarray(lig["bb_coords"], np.float64)[:, 1].mean(0)


def _pose_bb(run, i):
    """A symmetric run: the ligand backbone of trajectory i's final pose as the written files hold it (None otherwise)."""
    if run.sym is None:
        return None
    from . import symmetry as SY
    return SY._pose_backbone(run.lig["bb_coords"], run.cols["rot_update"][i], run.cols["tr_update"][i], _file_center(run.model, run.lig))


def _symmetry_columns(run):
    """The symmetry record of EVERY trajectory's final pose as arrays (run.data["symmetry"]): m, theta, screw, sym_rmsd, closure."""
    from . import symmetry as SY
    recs = [SY.record(run.rec["bb_coords"], _pose_bb(run, i), run.sym["n"], _center(run.model)) for i in range(len(run.cols["energy"]))]
    run.sym["records"] = recs
    return {k: np.asarray([r[k] for r in recs]) for k in ("m", "theta", "screw", "sym_rmsd", "closure")}


def _ring_clashes(run, indices):
    """n >= 4: the heavy-atom clash count of copy 0 (the receptor) against copies k = 2 .. n // 2 of the poses `indices`, summed over k -
    one call of the all-atom screen over all of them (copy k placed by symmetry.copy_poses).  Copies 1 and n - 1 are the docked interface
    itself; a ring that closes on paper can still run copy 2 into copy 0."""
    from . import symmetry as SY
    n = run.sym["n"]
    ks = list(range(2, n // 2 + 1))
    ra, la, cen = sterics_inputs(run.rec, run.lig, run.model.hp.family)
    rot, tr = run.poses()
    rots, trs = [], []
    for i in indices:
        rk, tk = SY.copy_poses(run.rec["bb_coords"], run.lig["bb_coords"], rot[i], tr[i], _file_center(run.model, run.lig), n, _center(run.model))
        rots += [rk[k - 1] for k in ks]
        trs += [tk[k - 1] for k in ks]
    with run.model.atoms(ra, la, cen) as at:
        out = at.sterics(np.asarray(rots, np.float32).reshape(-1, 3), np.asarray(trs, np.float32).reshape(-1, 3))
    return [int(v) for v in out["n_clash"].reshape(len(indices), len(ks)).sum(1)]


def _symmetry_record(run, i, ring=None):
    return dict(run.sym["records"][i], **({} if ring is None else {"ring_clashes": ring}))


def _write_pose(run, path, lig_aa, lig_bb, remarks=None):
    """One written model: receptor + ligand at lig_aa - or, in a symmetric run, all n chains: the receptor under its own chain id, then
    the ligand (lig_aa, its backbone lig_bb) and its images under the powers of the projected transform T' (symmetry.evaluate: a pure
    rotation by theta* about the assembly's axis) under the next unused chain letters."""
    rec, lig = run.rec, run.lig
    if run.sym is None:
        return pdbio.write_complex_pdb(path, list(rec["atoms"]), lig["atoms"], lig_aa, remarks=remarks)
    from . import symmetry as SY
    n = run.sym["n"]
    ev = SY.evaluate(rec["bb_coords"], lig_bb, n, center=_center(run.model))
    if ev["m"] > 0:
        Qp = SY.axis_angle_to_matrix(ev["theta_star"] * ev["axis"])
        taup = ev["axis_point"] - Qp @ ev["axis_point"]
    else:      # no axis (or a non-finite pose): the fit's own transform
        Qp, taup = (ev["Q"], ev["tau"]) if ev["Q"] is not None else (np.full((3, 3), np.nan), np.full(3, np.nan))
    used = set(pdbio._chain_ids(rec["residues"]))
    letters = [ch for ch in "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789" if ch not in used]
    atoms, coords = [], []
    for k in range(1, n):
        Qk, tk = SY.transform_power(Qp, taup, k - 1)
        atoms += [dict(a, chain=letters[k - 1]) for a in lig["atoms"]]
        coords.append(np.asarray(lig_aa, np.float64) @ Qk.T + tk)
    pdbio.write_complex_pdb(path, list(rec["atoms"]), atoms, np.concatenate(coords, 0), remarks=remarks)


class _Run:
    """One pair-driver call after its sampling: what _finish, the analyses and _top_models pass around.  cols: every trajectory's energy, rot_update,
    tr_update (and the driver's own columns); opts[name]: the checked options of every analysis of ANALYSES that is on; data[name]: the arrays it produced;
    k, key, bad, ranked_by: the kept pose, the clustering key, the poses the clash filter removed (or None) and the rule that chose k, as they stand."""

    def __init__(self, model, gx, rec, lig, cols, precision, opts=None, selfcheck=None, out_pdb=None, native=None, seed=0):
        self.model, self.gx, self.rec, self.lig, self.lig0, self.cols = model, gx, rec, lig, gx.lig_pos0, cols
        self.precision, self.selfcheck, self.out_pdb, self.native, self.seed = precision, selfcheck, out_pdb, native, seed
        self.opts, self.data = {name: o for name, o in (opts or {}).items() if o is not None}, {}
        self.k, self.key, self.bad, self.ranked_by = None, None, None, "energy"
        self.sym = None      # a symmetric run (_check_symmetry's dict): every written model holds all n chains, every pose a `symmetry` record

    def any(self):      # is any analysis on?  Then the result also carries `index` and every trajectory, and dock_pair picks among all of them at once
        return bool(self.opts)

    def poses(self):
        return self.cols["rot_update"], self.cols["tr_update"]


def _ranked(run, name, data, column, pick=np.argmin):
    """Keeps the arrays of analysis `name` and, when its options say that the run ranks by it, makes the pose of the lowest `column` among those the clash filter
    left the kept one (ties: the lower index) and the column the clustering key, NaN on the removed poses.  With np.nanargmin a NaN never wins, and a column of NaN alone moves nothing."""
    run.data[name] = data
    if run.opts[name][0]:
        key = _nan_key(data[column], run.bad)
        run.ranked_by = name
        if pick is not np.nanargmin or not np.isnan(key).all():
            run.k, run.key = _kept(pick, run.bad, data[column]), key


def _sterics_screen(run):
    sd, bad = _screen(run.model, run.rec, run.lig, run.cols, run.opts["sterics"])
    if run.bad is not None and bad is not None:      # poses the driver removed itself (rescore_pair's rejected decoys): both masks hold
        bad = run.bad | bad
        if bad.all():      # the filter would take what the driver left: nothing more is removed
            sd["fallback"], bad = True, run.bad
    run.data["sterics"], run.bad = sd, run.bad if bad is None else bad


def _distogram_select(run):
    _, t, maps, mb = run.opts["distogram"]
    _ranked(run, "distogram", ensemble_distogram(run.gx, *run.poses(), t, run.precision, mb, maps=maps, seed=run.seed), "nll", np.nanargmin)


def _interface_select(run):
    _, weights, cutoff = run.opts["interface"]
    _ranked(run, "interface", ensemble_interface_energy(run.model, run.rec, run.lig, *run.poses(), cutoff, weights), "total")


def _pairpot_select(run):
    pd = ensemble_pairpot(run.model, run.rec, run.lig, *run.poses(), run.opts["pairpot"][1])
    pd.update(rot_update=run.cols["rot_update"], tr_update=run.cols["tr_update"])      # the poses the arrays are of (a restrained run's `trajectories` hold none)
    _ranked(run, "pairpot", pd, "energy")


def _density_select(run):
    _, dmap, resolution, threshold, _ = run.opts["density"]
    dd = ensemble_density(run.model, run.rec, run.lig, *run.poses(), dmap, resolution, threshold)
    dd.update(rot_update=run.cols["rot_update"], tr_update=run.cols["tr_update"])      # the poses the arrays are of
    _ranked(run, "density", dd, "neg_cc", np.nanargmin)      # the highest correlation; a NaN never wins


def _consensus_select(run):
    """Under rank "consensus" the kept pose becomes the one consensus.pick keeps and the key its order - unless no pose has any contact, when both stay."""
    from . import consensus as CS
    rank, cutoff, top = run.opts["consensus"]
    cd = run.data["consensus"] = ensemble_consensus(run.model, run.rec["bb_coords"], run.lig0, *run.poses(), run.cols["energy"], cutoff, top)
    if run.bad is not None:      # poses the clash filter removed: no score, so never picked and last in consensus order
        cd["consensus"] = np.where(run.bad, np.nan, cd["consensus"])
    if rank == "consensus":
        k = CS.pick(cd["consensus"], run.cols["energy"])
        if k is not None:
            run.k, run.key, run.ranked_by = k, CS.rank_positions(cd["consensus"], run.cols["energy"]), "consensus"


def _shared_surface(run):      # one surface call serves the affinity estimate too when its options are the ones that takes (probe 1.4 A, 128 points)
    surf = run.opts.get("surface")
    return surf is not None and "affinity" in run.opts and surf[1:] == _check_surface(True, None, *AFFINITY_SURFACE)[1:]


def _surface_describe(run):
    _, probe, points = run.opts["surface"]
    run.data["surface"] = ensemble_surface(run.model, run.rec, run.lig, *run.poses(), probe, points, per_atom=_shared_surface(run) or "hbonds" in run.opts)


def _affinity_describe(run):
    shared = run.data["surface"] if _shared_surface(run) else None
    run.data["affinity"] = pose_affinity(run.model, run.rec, run.lig, *run.poses(), run.opts["affinity"][0], *AFFINITY_SURFACE, surface=shared)


def _hbonds_describe(run):
    # reported, never ranked by; with the surface in the same run also the buried donors and acceptors without a bond
    bd = run.data.get("surface")
    hd = run.data["hbonds"] = ensemble_hbonds(run.model, run.rec, run.lig, *run.poses(), *run.opts["hbonds"], per_atom=bd is not None)
    hd.update(rot_update=run.cols["rot_update"], tr_update=run.cols["tr_update"])      # the poses the arrays are of
    if bd is not None:
        hd["n_unsat"] = unsatisfied_polar(hd, bd)


class _Analysis(NamedTuple):
    """One per-pose analysis of the pair drivers."""
    name: str
    defaults: dict                # its keywords of dock_pair / refine_pair
    check: Callable               # (model, rank, max_batch, **its keywords) -> its options, None: off; raises before anything is sampled
    stage: str                    # where _finish runs it: "screen", "handle", "select" or "describe"
    run: Callable                 # run -> None: fills run.data[name]; may set run.bad ("screen") or run.k, run.key, run.ranked_by ("handle", "select")
    result: Callable              # run -> its entries of the result, for the kept pose run.k
    pose: Callable = None         # (data, k) -> its summary of pose k: what every model of top_k gains ...
    model_key: str = None         # ... under this key (None: merged into the model)


# In the order a model of top_k lists them, which within a stage is also the order of the calls: interface, pairpot, density, then consensus (one
# rank is given, so at most one of them moves the kept pose); surface before affinity and hbonds, which use it.
ANALYSES = (
    _Analysis("sterics", dict(clash_screen=False, clash_filter=False, clash_cutoff=3.0, contact_cutoff=5.0), lambda model, rank, max_batch, **kw: _check_sterics(**kw),
              "screen", _sterics_screen, lambda run: _sterics_result(run.data["sterics"], run.k), _pose_sterics, "sterics"),
    _Analysis("surface", dict(bsa=False, min_bsa=None, probe=1.4, sphere_points=128), lambda model, rank, max_batch, **kw: _check_surface(**kw),
              "describe", _surface_describe, lambda run: _surface_result(run.data["surface"], run.k, run.opts["surface"]), _pose_bsa),
    # its `ranked_by`: the rule that kept the pose - but rank "distogram" is named only when the consensus object names it as well
    _Analysis("interface", dict(interface_energy=False, ie_weights=None, ie_cutoff=8.0), lambda model, rank, max_batch, **kw: _check_interface(rank=rank, **kw),
              "select", _interface_select, lambda run: _interface_result(
                  run.data["interface"], run.k, run.opts["interface"], run.bad, run.ranked_by if "consensus" in run.opts or run.ranked_by != "distogram" else "energy"),
              _pose_interface, "interface_energy"),
    _Analysis("affinity", dict(affinity=False, affinity_cutoff=5.5), lambda model, rank, max_batch, **kw: _check_affinity(**kw),
              "describe", _affinity_describe, lambda run: _affinity_result(run.data["affinity"], run.k), _pose_affinity, "affinity"),
    _Analysis("distogram", dict(distogram=False, distogram_t=DISTOGRAM_T, distogram_maps=False),
              lambda model, rank, max_batch, **kw: _check_distogram(model, rank=rank, max_batch=max_batch, **kw),
              "handle", _distogram_select, lambda run: _distogram_result(run.data["distogram"], run.k, run.opts["distogram"], run.bad), _pose_distogram),
    _Analysis("hbonds", dict(hbonds=False, hbond_cutoff=3.5, hbond_angle=90.0, salt_cutoff=4.0), lambda model, rank, max_batch, **kw: _check_hbonds(**kw),
              "describe", _hbonds_describe, lambda run: _hbonds_result(run.data["hbonds"], run.k), _pose_hbonds),
    _Analysis("pairpot", dict(pair_potential=None), lambda model, rank, max_batch, **kw: _check_pairpot(rank=rank, **kw),
              "select", _pairpot_select, lambda run: _pairpot_result(run.data["pairpot"], run.k), _pose_pairpot, "pair_potential"),
    _Analysis("density", dict(density_map=None, density_resolution=None, density_threshold=1.0, min_density_cc=None),
              lambda model, rank, max_batch, **kw: _check_density(rank=rank, **kw),
              "select", _density_select, lambda run: _density_result(run.data["density"], run.k, run.opts["density"], run.bad), _pose_density),
    _Analysis("consensus", dict(consensus=False, consensus_top=1.0, consensus_cutoff=5.5), lambda model, rank, max_batch, consensus, consensus_top, consensus_cutoff:
              (rank, float(consensus_cutoff), float(consensus_top)) if consensus or rank == "consensus" else None,      # rank "consensus" implies it
              "select", _consensus_select, lambda run: _consensus_result(run.data["consensus"], run.k, run.opts["consensus"], run.ranked_by)),
)


def _analysis_options(model, max_batch, kw):
    """{analysis name: its checked options, None when it is off} of a dock_pair / refine_pair call, before anything is sampled.  kw: what the call gave beyond
    the driver's own parameters; `rank` and the keywords of ANALYSES (their defaults where absent) are taken OUT of it - what stays goes to the sampler."""
    rank = kw.pop("rank", "energy")
    given = {a.name: {name: kw.pop(name, default) for name, default in a.defaults.items()} for a in ANALYSES}
    _check_rank(rank, given["consensus"]["consensus_top"])
    return {a.name: a.check(model, rank, max_batch, **given[a.name]) for a in ANALYSES}


def _check_refine(top_k, refine_t, refine_samples):
    """refine_t of dock_pair / rescore_pair: it needs top_k and at least one trajectory per centre."""
    if refine_t is not None and top_k is None:
        raise ValueError("refine_t refines the cluster centres: it needs top_k")
    if refine_t is not None and int(refine_samples) < 1:
        raise ValueError("refine_samples must be >= 1")


def _check_models(top_k, cluster_radius, cluster_rule):
    """None (no models) or the options of _top_models: (top_k, cluster radius, cluster rule), checked."""
    if top_k is None:
        return None
    if int(top_k) < 1:
        raise ValueError("top_k must be >= 1")
    if cluster_rule not in ("energy", "size"):
        raise ValueError(f"cluster_rule must be 'energy' or 'size', got {cluster_rule!r}")
    if not (np.isfinite(cluster_radius) and cluster_radius > 0):
        raise ValueError("cluster_radius must be finite and > 0")
    return int(top_k), float(cluster_radius), cluster_rule


def _finish(run, pick, entries, clu=None, refine=None):
    """What every pair driver does with its sampled trajectories: the kept pose, its files and the result.  pick = (rule, *column names): the driver's
    own choice, rule(*columns) -> index; run.key: the clustering key that goes with it.  entries(k): the driver's own result entries for the kept pose k.
    clu: None or the options of _top_models; refine: None or the keyword arguments of refine_models - only then does the handle outlive the post-processing."""
    model, gx, rec, lig, cols = run.model, run.gx, run.rec, run.lig, run.cols
    on = [a for a in ANALYSES if a.name in run.opts]

    def stage(name):
        for a in on:
            if a.stage == name:
                a.run(run)
    handle = refine is not None or any(a.stage == "handle" for a in on)
    if not handle:      # the columns are host arrays: the handle (and its ~GB of device workspace) goes before any post-processing
        gx.close()
    stage("screen")
    run.k = _kept(pick[0], run.bad, *(cols[c] for c in pick[1:]))
    run.key = _nan_key(run.key, run.bad)
    stage("handle")      # the model's own distogram needs the open handle (a forward per pose): the handle goes right after it
    if handle and refine is None:
        gx.close()
    stage("select")      # the kept pose is settled first - the driver's rule, then the rank that is given - and only then does anything describe it
    run.key = _nan_key(run.key, run.bad)      # again: rank "consensus" has replaced the key by consensus.rank_positions
    stage("describe")
    k = run.k
    lig_aa = pdbio.apply_pose_all_atom(lig["aa_coords"], lig["bb_coords"], cols["rot_update"][k], cols["tr_update"][k], center=_center(model))
    if run.sym is not None:
        run.data["symmetry"] = _symmetry_columns(run)
    if run.out_pdb:
        _write_pose(run, run.out_pdb, lig_aa, _pose_bb(run, k), remarks=_remarks(run.data.get("sterics"), k))
    res = {"energy": float(cols["energy"][k]), "rot_update": cols["rot_update"][k].copy(), "tr_update": cols["tr_update"][k].copy(),
           "lig_aa_coords": lig_aa, "precision": run.precision, "selfcheck": run.selfcheck, **entries(k)}
    for a in on:
        res.update(a.result(run))
    if run.any():      # these also return `index` and every trajectory - the driver's own `trajectories` if it has them
        res.setdefault("trajectories", {c: cols[c] for c in ("energy", "rot_update", "tr_update")})
    if run.native is not None:      # of the kept pose: its rot_update / tr_update on the input backbone
        pose = rebuild_backbone(run.lig0, res["rot_update"][None], res["tr_update"][None], model.hp.family)
        res["metrics"] = native_metrics(model, run.native, rec["bb_coords"], pose)[0]
    if clu is not None:
        res.update(_top_models(run, clu))
    if run.sym is not None:      # the kept pose and every model: their record; n >= 4: the ring screen of all of them in one call
        idx = [k] + [m["index"] for m in res.get("models", [])]
        ring = _ring_clashes(run, idx) if run.sym["n"] >= 4 else [None] * len(idx)
        res["symmetry"] = _symmetry_record(run, k, ring[0])
        for m, rc in zip(res.get("models", []), ring[1:]):
            m["symmetry"] = _symmetry_record(run, m["index"], rc)
        res["symmetry_data"] = dict(run.data["symmetry"], n=run.sym["n"], tolerance=run.sym["tolerance"], input_rmsd=run.sym["input_rmsd"])
        res.setdefault("index", k)
    if clu is not None:
        if refine is not None:
            refine_models(run, res["models"], **refine)
            gx.close()
    return res


def dock_pair(model: engine.Model, rec, lig, rec_x, lig_x, num_samples=120, num_steps=40, seed=0, precision="mfma16",
              out_pdb="output.pdb", max_batch=256, selfcheck=True, on_selfcheck_fail="fp32", restraints=None,
              restraint_rank="satisfied", restraint_params=None, top_k=None, cluster_radius=4.0, cluster_rule="energy", refine_t=None,
              refine_samples=8, native=None, symmetry=None, symmetry_params=None, symmetry_tolerance=0.1, **sampler_kw):
    """inference() of the reference for two parsed PDB chains (pdbio.backbone_from_atoms dicts) and their pre-computed node features; returns
    {'energy': min energy} and writes the best pose.  `sampler_kw`: `rank` and the analysis keywords described below (their names and defaults:
    ANALYSES; checked by _analysis_options before anything is sampled) and, beyond those, the sampler options the reference's pair loop passes
    (src/inference_base.py:483-491: use_clash_force, noise_annealing, tr_noise_scale, rot_noise_scale, ode).

    `restraints` ([restraints.RestraintGroup]): sample with the interface restraint step (DFM_F_RESTRAINTS, `restraint_params` or the
    defaults) and keep, by `restraint_rank`, the minimum-energy trajectory among those satisfying the most groups ("satisfied") or the
    reference's plain minimum-energy one ("energy"); the result gains `restraint_energy`, `restraints_satisfied` of the kept pose and
    `trajectories` (per-trajectory energy, restraint_energy, restraints_satisfied).

    `top_k`: also cluster the trajectories by ligand RMSD (cluster_trajectories: `cluster_radius` A, rule `cluster_rule`) with the key
    that picks output.pdb - energy, or under restraint_rank "satisfied" the most satisfied groups and then energy - and return up to
    top_k cluster centres as `models` [{rank, index, energy, cluster_size}], written as <out_pdb stem>_<rank>.pdb.  Under rule "energy"
    model 1 is the output.pdb pose.

    `refine_t` (needs top_k): the centres are then refined locally from t_begin = refine_t, `refine_samples` trajectories each, in one
    batched call (refine_models); the models gain `refined_energy` and their files hold the refined poses.  output.pdb is unchanged.

    `native` ((receptor [R,3,3], ligand [L,3,3]) backbones of the native complex, any frame, same residues as the input): the result
    gains `metrics` (c_rmsd, i_rmsd, l_rmsd, fnat, DockQ of the kept pose, on the GPU: native_metrics), every model `metrics` and, after
    refinement, `refined_metrics`.

    `consensus`: the trajectories are also scored by consensus contacts (ensemble_consensus: contacts below `consensus_cutoff` A, members =
    the best `consensus_top` fraction by energy) and the result gains `consensus` ({score, rank, n_contacts} of the kept pose - rank: its
    position in consensus order - plus M, cutoff, ranked_by, fallback), `consensus_data` (the arrays of Model.consensus and `members`),
    `index` and `trajectories` (every trajectory's energy, rot_update, tr_update, as refine_pair returns them; with restraints: the
    restrained path's own `trajectories`).  rank="consensus" (implies consensus) keeps the pose with the highest consensus instead (ties: lower energy, then lower
    index; it overrides restraint_rank) and makes that order the clustering key of `top_k`; when no trajectory has any contact the
    driver's own rule stays and `fallback` is true.

    `clash_screen`: the all-atom clash / contact screen of every trajectory (ensemble_sterics: heavy-atom pairs below `clash_cutoff` /
    `contact_cutoff` A, CAPRI's mean + 2 std rule over the ensemble).  The result gains `sterics` ({n_clash, n_contact, min_dist, flagged}
    of the kept pose, threshold, ensemble_mean, ensemble_std, the cutoffs, filtered, fallback), `sterics_data` (the arrays), `index` and
    `trajectories`; every model of `top_k` gains `sterics`, and every written file a REMARK line with its counts.  `clash_filter` (implies
    the screen): flagged poses are removed before the selection, the consensus ranking and the clustering - they can neither be kept nor
    become a model; were every pose flagged, nothing is removed and `fallback` is true.

    `bsa`: the buried solvent-accessible surface area of every trajectory (ensemble_surface: Shrake-Rupley with `sphere_points` points per
    heavy atom and a probe of `probe` A).  The result gains `bsa`, `bsa_rec`, `bsa_lig` (A^2 of the kept pose: both sides, each side),
    `bsa_data` (the arrays), `probe`, `sphere_points`, `index` and `trajectories`; every model of `top_k` gains the three areas.  `min_bsa`
    (implies bsa): cluster centres that bury less than min_bsa A^2 do not become a model of `top_k`; `bsa_dropped` counts them.  It
    composes with `clash_filter`; the kept pose is not affected.

    `interface_energy`: the soft Lennard-Jones + Coulomb interface energy of every trajectory (ensemble_interface_energy: heavy-atom
    pairs within `ie_cutoff` A).  The result gains `interface_energy` ({rep, att, elec, total, n_pairs} of the kept pose in kcal/mol, its
    rank by total, weights, cutoff, ranked_by), `interface_data` (the arrays), `index` and `trajectories`; every model of `top_k` gains
    `interface_energy`.  total = ifenergy.total with `ie_weights` (rep, att, elec; None: ifenergy.WEIGHTS - starting values, not
    fitted).  rank="interface" (implies interface_energy) keeps the pose with the lowest total instead (ties: lower index; it overrides
    restraint_rank) and makes the totals the clustering key of `top_k`; poses `clash_filter` removed get a NaN key as under rank
    "consensus".

    `affinity`: the residue contacts by class (heavy atoms within `affinity_cutoff` A) and the contacts-based affinity estimate of every
    trajectory (pose_affinity: IC-NIS with starting values that are not verified or calibrated, on this project's own surface).  The
    result gains `affinity` ({ic, n_pairs, n_rec_res, n_lig_res, nis_apolar, nis_charged, dg, kd, cutoff} of the kept pose; dg in
    kcal/mol, kd in M, None where there is no surface residue), `affinity_data` (the arrays of every trajectory, with dg_contacts),
    `index` and `trajectories`; every model of `top_k` gains `affinity`.  Nothing is ranked by it.

    `distogram` (family-1 models only; anything else raises before sampling): the model's own distogram head at every final pose
    (ensemble_distogram: one forward per pose at time `distogram_t`, in chunks of max_batch, reduced on the GPU).  The result gains
    `distogram` ({dist_nll, dist_nll_near, exp_contacts, n_near} of the kept pose, its rank by nll, t, contact_bins), `distogram_data`
    (the arrays; with `distogram_maps` also pcontact_mean [R,L] and edist [P,R,L]), `index` and `trajectories`; every model of `top_k`
    gains dist_nll, dist_nll_near and exp_contacts.  rank="distogram" (implies distogram) keeps the pose with the lowest nll instead
    (ties: lower index; it overrides restraint_rank) and makes the nll values the clustering key of `top_k`; poses `clash_filter` removed
    get a NaN key as under rank "consensus".

    `hbonds`: the interface hydrogen bonds and salt bridges of every trajectory (ensemble_hbonds: heavy-atom criteria - a distance below
    `hbond_cutoff` A and both antecedent angles at least `hbond_angle` degrees; cation / anion pairs below `salt_cutoff` A; HIS is donor,
    acceptor and cation; no agreement with any published tool is claimed).  The result gains n_hbond, hb_bb_bb, hb_bb_sc, hb_sc_sc, n_salt
    of the kept pose, `hbond_data` (the arrays), `index` and `trajectories`; with `bsa` in the same run also n_unsat, the donors and
    acceptors the pose buries completely and leaves without a bond; every model of `top_k` gains the same numbers.  Nothing is ranked or
    filtered by them.
    `pair_potential` (pairpot.load's dict, or the path of such a file - the project ships no table): the tabulated pair potential of
    every trajectory (ensemble_pairpot: the heavy atoms the file's type names fit).  The result gains `pair_potential` ({energy in
    kcal/mol, n_pairs, n_untyped, T, NB, cutoff} of the kept pose), `pairpot_data` (the arrays and the rot_update / tr_update they are of), `index` and `trajectories`; every model
    of `top_k` gains `pair_potential`.  rank="pairpot" (needs pair_potential) keeps the pose with the lowest energy instead (ties: lower
    index; it overrides restraint_rank and becomes the clustering key of top_k).
    `density_map` (density.read_mrc's dict, or the path of an MRC file; the receptor is taken to sit in the map's frame) with
    `density_resolution` (A; sigma = resolution * density.SIGMA_FACTOR) and `density_threshold` (in units of the normalised map): the
    density fit of every trajectory (ensemble_density: heavy atoms weighted by atomic number).  The result gains `density` ({density_cc,
    density_inclusion, density_n_outside, rank, resolution, sigma, threshold} of the kept pose), `density_data`, `index` and
    `trajectories`; every model of `top_k` gains density_cc, density_inclusion and density_n_outside.  rank="density" (needs density_map)
    keeps the pose with the highest correlation instead; `min_density_cc` leaves a cluster centre below it out of `models`
    (`density_dropped`).  The ligand is rigid, nothing guides the sampler, and nothing is claimed about ranking quality on real maps.

    `symmetry` (an order n in 2 .. 24): Cn symmetric docking of a homo-oligomer.  Receptor and ligand must be ONE chain each, of the same
    sequence, and rigid images of each other within `symmetry_tolerance` A (Kabsch rmsd of the backbones); anything else raises a
    ValueError that names the cause, before anything is sampled.  The sampler runs with the symmetry step (DFM_F_SYMMETRY,
    `symmetry_params`: symmetry.SymmetryParams or the defaults - starting values, not measured against a trained checkpoint); a model
    with the 67th position channel gets its homomer flag.  The result gains `symmetry` ({n, m, theta, screw, sym_rmsd, closure, axis,
    axis_point} of the kept pose; closure: the largest displacement of a receptor atom under T^n, on the host; for n >= 4 also
    ring_clashes, the heavy-atom clashes of the receptor against copies 2 .. n / 2 from the all-atom screen - reported, nothing is
    filtered by it), `symmetry_data` (m, theta, screw, sym_rmsd, closure of every trajectory) and `index`; every model of `top_k` gains
    `symmetry` (of its cluster centre) and, under `refine_t`, `refined_symmetry` (the same record without ring_clashes, of the refined pose
    its file holds; the refinement samples with the symmetry step too).  out_pdb and the model files hold all n chains: the receptor under its chain id, the copies under the next unused
    letters."""
    sym = _check_symmetry(rec, lig, symmetry, symmetry_params, symmetry_tolerance)
    opts = _analysis_options(model, max_batch, sampler_kw)
    if native is not None:
        _check_native(native, len(rec["bb_coords"]), len(lig["bb_coords"]))
    _check_refine(top_k, refine_t, refine_samples)
    if restraints is not None and restraint_rank not in ("satisfied", "energy"):
        raise ValueError(f"restraint_rank must be 'satisfied' or 'energy', got {restraint_rank!r}")
    clu = _check_models(top_k, cluster_radius, cluster_rule)
    refine = None if refine_t is None else dict(t_begin=float(refine_t), n=int(refine_samples), num_steps=num_steps,
                                                restraints=restraints is not None, **({"symmetry": True} if sym else {}), **sampler_kw)
    gx = engine.Complex(model, rec_x, lig_x, rec["bb_coords"], lig["bb_coords"])
    if sym:      # (before the self-check: the homomer channel changes what the engines compute)
        _set_symmetry(model, gx, sym)
    precision, chk = checked_precision(gx, precision, "pair", selfcheck, on_selfcheck_fail, seed=seed)
    restrained = restraints is not None
    if restrained:
        gx.set_restraints(restraints, restraint_params)
    cols = {c: [] for c in ("energy", "rot_update", "tr_update") + (("restraint_energy", "restraints_satisfied") if restrained else ())}
    best, k0, done = None, None, 0
    while done < num_samples:
        b = min(max_batch, num_samples - done)
        r = gx.sample(B=b, num_steps=num_steps, seed=seed + done, restraints=restrained, symmetry=sym is not None,
                      **engine.precision_kwargs(precision), **sampler_kw)
        if restrained:      # the restraint terms of the final poses, on the sampler's own kernel
            ev = gx.restraint_eval(r["lig_pos"])
            r["restraint_energy"], r["restraints_satisfied"] = ev["energy"], ev["n_satisfied"]
        k = int(np.argmin(r["energy"]))
        if k0 is None or r["energy"][k] < best:     # strict <: the first minimum wins, as in the reference
            best, k0 = r["energy"][k], done + k
        for c in cols:
            cols[c].append(r[c])
        done += b
    cols = {c: np.concatenate(v, 0) for c, v in cols.items()}
    run = _Run(model, gx, rec, lig, cols, precision, opts, chk, out_pdb, native, seed)
    run.sym = sym
    if not restrained:
        # the loop's own minimum; with any analysis on, the pick is among all trajectories at once (the first minimum: the same pose)
        pick = (np.argmin if run.any() else (lambda energy: k0), "energy")
        run.key, entries = cols["energy"], lambda k: {}
    else:
        from . import restraints as RS
        from .cluster import satisfied_key
        by_satisfied = restraint_rank == "satisfied"
        pick = (RS.rank_key, "energy", "restraints_satisfied") if by_satisfied else (np.argmin, "energy")
        run.key = satisfied_key(cols["energy"], cols["restraints_satisfied"]) if by_satisfied else cols["energy"]
        entries = lambda k: {"index": k, "restraints": len(restraints), "restraint_rank": restraint_rank,
                             "restraint_energy": float(cols["restraint_energy"][k]), "restraints_satisfied": int(cols["restraints_satisfied"][k]),
                             "trajectories": {c: cols[c] for c in ("energy", "restraint_energy", "restraints_satisfied")}}
    return _finish(run, pick, entries, clu, refine)


def refine_pair(model: engine.Model, rec, lig, rec_x, lig_x, t_begin=0.1, num_samples=32, num_steps=40, seed=0, precision="mfma16",
                out_pdb="output.pdb", max_batch=256, selfcheck=True, on_selfcheck_fail="fp32", perturb=True, restraints=None,
                restraint_params=None, native=None, start_shift=None, symmetry=None, symmetry_params=None, symmetry_tolerance=0.1,
                **sampler_kw):
    """Local refinement of the pose the two parsed PDB chains are in (engine.Complex.refine, dfm_refine): num_samples trajectories start from that pose
    noised with the forward process at t_begin (perturb=False: from the pose itself) and run the sampler's steps down from t_begin; like dock_pair the
    minimum-energy one is kept, applied to the all-atom ligand and written to out_pdb.  Returns dock_pair's dict plus `t_begin`, `index` and `trajectories`
    (every trajectory's energy, rot_update, tr_update).  `restraints` ([restraints.RestraintGroup]) turns the restraint step on (DFM_F_RESTRAINTS).
    `native`, `rank` and every analysis keyword: as for dock_pair (there are no models here, so min_bsa only turns bsa on); with `native` the result also
    gains `start_metrics` of the pose the refinement started from.
    `start_shift` ([num_samples,3]): trajectory i starts from the input pose translated by start_shift[i] (the engine's start_pos); the
    shift is added to its tr_update, so (rot_update, tr_update) keep mapping the INPUT pose onto the final one.
    `symmetry`, `symmetry_params`, `symmetry_tolerance`: as for dock_pair (the symmetry step fits the receptor onto every pose itself: it
    needs no reference ligand, so foreign start poses are fine)."""
    sym = _check_symmetry(rec, lig, symmetry, symmetry_params, symmetry_tolerance)
    opts = _analysis_options(model, max_batch, sampler_kw)
    if native is not None:
        _check_native(native, len(rec["bb_coords"]), len(lig["bb_coords"]))
    if start_shift is not None:
        start_shift = np.asarray(start_shift, np.float32).reshape(-1, 3)
        if start_shift.shape[0] != num_samples:
            raise ValueError(f"start_shift must be [{num_samples},3], got {start_shift.shape}")
    gx = engine.Complex(model, rec_x, lig_x, rec["bb_coords"], lig["bb_coords"])
    if sym:
        _set_symmetry(model, gx, sym)
    precision, chk = checked_precision(gx, precision, "pair", selfcheck, on_selfcheck_fail, seed=seed)
    if restraints is not None:
        gx.set_restraints(restraints, restraint_params)
    cols = {k: [] for k in ("energy", "rot_update", "tr_update")}
    done = 0
    while done < num_samples:
        b = min(max_batch, num_samples - done)
        skw = dict(sampler_kw)
        if start_shift is not None:      # a translation commutes with the rotation about the (equally translated) centre
            skw["start_pos"] = gx.lig_pos0[None] + start_shift[done:done + b, None, None, :]
        r = gx.refine(B=b, t_begin=t_begin, perturb=perturb, num_steps=num_steps, seed=seed + done, restraints=restraints is not None,
                      symmetry=sym is not None, **engine.precision_kwargs(precision), **skw)
        if start_shift is not None:
            r["tr_update"] = (r["tr_update"] + start_shift[done:done + b]).astype(np.float32)
        for c in cols:
            cols[c].append(r[c])
        done += b
    cols = {k: np.concatenate(v, 0) for k, v in cols.items()}
    run = _Run(model, gx, rec, lig, cols, precision, opts, chk, out_pdb, native, seed)
    run.sym = sym
    res = _finish(run, (np.argmin, "energy"),      # the first minimum wins, as in dock_pair
                  lambda k: {"index": k, "t_begin": float(t_begin), "trajectories": cols})
    if native is not None:
        res["start_metrics"] = native_metrics(model, native, rec["bb_coords"], run.lig0[None])[0]
    return res


class AllRejected(ValueError):
    """rescore_pair: no decoy is a rigid image of the input pair."""


RESCORE_T = 1e-3      # time of rescore_pair's energy evaluation: the last entry of the sampler's default grid, where dfm_sample takes its final energy


def fit_decoys(model: engine.Model, lig0, decoys, rec_bb=None):
    """The decoys of rescore_pair as (rot_update [P,3], tr_update [P,3] float32, rmsd [P], rec_rmsd [P] or None): coordinates
    ({"lig_pos": [P,L,3,3], "rec_pos": optional [P,R,3,3]}) fitted on the GPU (Model.pose_fit) about the backbone centre
    cluster.rebuild_backbone uses for the model's family; poses ({"rot_update", "tr_update"}) taken as they are, with an rmsd of 0."""
    if "lig_pos" in decoys:
        if "rot_update" in decoys or "tr_update" in decoys:
            raise ValueError("decoys must hold either lig_pos (and rec_pos) or rot_update and tr_update, not both")
        x0 = np.asarray(lig0, np.float32).reshape(-1, 3, 3).astype(np.float64)
        center = x0.reshape(-1, 3).mean(0) if model.hp.family == 1 else x0[:, 1].mean(0)
        rec_pos = decoys.get("rec_pos")
        if rec_pos is not None and rec_bb is None:
            raise ValueError("decoys with rec_pos need the input receptor's backbone")
        f = model.pose_fit(lig0, decoys["lig_pos"], center, None if rec_pos is None else rec_bb, rec_pos)
        return f["rot"], f["tr"], f["rmsd"], f["rec_rmsd"]
    if "rot_update" not in decoys or "tr_update" not in decoys:
        raise ValueError("decoys must hold lig_pos (and optionally rec_pos) or rot_update and tr_update")
    rot, tr = (np.array(decoys[k], np.float32).reshape(-1, 3) for k in ("rot_update", "tr_update"))
    if rot.shape != tr.shape or rot.shape[0] < 1:
        raise ValueError(f"rot_update and tr_update must both be [P,3] with P >= 1, got {rot.shape} and {tr.shape}")
    return rot, tr, np.zeros(rot.shape[0]), None


def rescore_pair(model: engine.Model, rec, lig, rec_x, lig_x, decoys, fit_tolerance=0.1, t=RESCORE_T, seed=0, precision="mfma16",
                 out_pdb="output.pdb", max_batch=256, selfcheck=True, on_selfcheck_fail="fp32", top_k=None, cluster_radius=4.0,
                 cluster_rule="energy", refine_t=None, refine_samples=8, num_steps=40, native=None, **kw):
    """Rescoring of decoys this engine did not sample: every decoy of the two parsed PDB chains becomes a pose (rot_update, tr_update)
    (fit_decoys), gets the model's energy at time `t` - Complex.score on cluster.rebuild_backbone of its pose, in chunks of max_batch, the
    chunk that starts at decoy p0 with seed + p0 as dock_pair's batches and ensemble_distogram's chunks take theirs: the energy column
    equals that call made by hand chunk by chunk, and with P <= max_batch the one call with `seed` - and
    the minimum-energy one is kept, written and described exactly as dock_pair does it (_finish): `rank`, every analysis keyword,
    `top_k` / `cluster_radius` / `cluster_rule`, `refine_t` / `refine_samples` and `native` are dock_pair's.  `num_steps` and what is
    left of `kw` go to the sampler of `refine_t`.
    A decoy whose fit leaves an rmsd (or rec_rmsd) above `fit_tolerance` A, or NaN, is no rigid image of the input: it is REJECTED - a
    NaN energy and key, never kept and never a model, like a pose the clash filter removed (the two masks add up); its pose columns hold
    the fit where that is finite and the identity where it is not, so every analysis still sees P poses.  With every decoy rejected
    the call raises AllRejected before any analysis runs.
    Returns refine_pair's dict (energy, index, trajectories, ...) plus `t`, `fit` ({rmsd, rec_rmsd, tolerance, n_rejected}, the first two
    of the kept pose) and `fit_data` ({rot_update, tr_update, rmsd, rec_rmsd, rejected}: the fit's own arrays).
    Family 1: cluster.rebuild_backbone rotates about the backbone centroid, pdbio.apply_pose_all_atom about the all-atom mean, and one
    (rot_update, tr_update) goes to both, as it always has in dock_pair."""
    opts = _analysis_options(model, max_batch, kw)
    if native is not None:
        _check_native(native, len(rec["bb_coords"]), len(lig["bb_coords"]))
    if not (np.isfinite(fit_tolerance) and fit_tolerance >= 0):
        raise ValueError("fit_tolerance must be finite and >= 0")
    _check_refine(top_k, refine_t, refine_samples)
    clu = _check_models(top_k, cluster_radius, cluster_rule)
    refine = None if refine_t is None else dict(t_begin=float(refine_t), n=int(refine_samples), num_steps=num_steps, **kw)
    lig0 = np.asarray(lig["bb_coords"], np.float32)
    rot, tr, rmsd, rec_rmsd = fit_decoys(model, lig0, decoys, np.asarray(rec["bb_coords"], np.float32))
    with np.errstate(invalid="ignore"):
        rejected = ~(rmsd <= fit_tolerance) | (False if rec_rmsd is None else ~(rec_rmsd <= fit_tolerance))
    fit_data = {"rot_update": rot.copy(), "tr_update": tr.copy(), "rmsd": rmsd, "rec_rmsd": rec_rmsd, "rejected": rejected}
    if rejected.all():
        raise AllRejected(f"every one of the {rejected.size} decoys is rejected: no fit is within fit_tolerance = {fit_tolerance} A "
                         f"(smallest rmsd {np.nanmin(rmsd) if not np.isnan(rmsd).all() else float('nan'):.3g} A) - are these decoys of this pair?")
    finite = np.isfinite(rot).all(1) & np.isfinite(tr).all(1)
    rot, tr = np.where(finite[:, None], rot, np.float32(0)), np.where(finite[:, None], tr, np.float32(0))
    gx = engine.Complex(model, rec_x, lig_x, rec["bb_coords"], lig["bb_coords"])
    precision, chk = checked_precision(gx, precision, "pair", selfcheck, on_selfcheck_fail, seed=seed)
    P, mb = rot.shape[0], max(1, int(max_batch))
    energy = np.concatenate([gx.score(rebuild_backbone(gx.lig_pos0, rot[p0:p0 + mb], tr[p0:p0 + mb], model.hp.family), t, seed=seed + p0,
                                      energy=True, **engine.precision_kwargs(precision))["energy"] for p0 in range(0, P, mb)])
    cols = {"energy": np.where(rejected, np.float32(np.nan), energy), "rot_update": rot, "tr_update": tr}
    run = _Run(model, gx, rec, lig, cols, precision, opts, chk, out_pdb, native, seed)
    run.key, run.bad = cols["energy"], rejected if rejected.any() else None
    res = _finish(run, (np.nanargmin, "energy"), lambda k: {"index": k, "t": float(t), "trajectories": cols}, clu, refine)
    k = res["index"]
    res["fit"] = {"rmsd": float(rmsd[k]), "rec_rmsd": None if rec_rmsd is None else float(rec_rmsd[k]), "tolerance": float(fit_tolerance),
                  "n_rejected": int(rejected.sum())}
    res["fit_data"], res["key"] = fit_data, run.key      # key: what the clustering ranked by, NaN on the removed poses
    return res


def refine_models(run, models, t_begin, n, num_steps, restraints=False, **sampler_kw):
    """dock_pair's second stage (`refine_t`): the K cluster centres of `models` refined in ONE dfm_refine call - B = K n trajectories,
    start_pos = each centre's backbone n times.  Every model gains `refined_energy` (the minimum over its n trajectories) and
    `refined_index`; <out_pdb stem>_<rank>.pdb becomes that refined pose (the centre's rigid motion, then the refinement's)."""
    model, rec, lig, cols = run.model, run.rec, run.lig, run.cols
    K = len(models)
    cen = [m["index"] for m in models]
    start = rebuild_backbone(run.lig0, cols["rot_update"][cen], cols["tr_update"][cen], model.hp.family)      # [K,L,3,3]
    r = run.gx.refine(B=K * n, t_begin=t_begin, start_pos=np.repeat(start, n, 0), num_steps=num_steps, seed=run.seed, restraints=restraints,
                      **engine.precision_kwargs(run.precision), **sampler_kw)
    center = _center(model)
    kept = [k * n + int(np.argmin(r["energy"][k * n:(k + 1) * n])) for k in range(K)]
    if run.native is not None:      # every centre after its refinement (before: the model's `metrics`, _top_models)
        for m, rm in zip(models, native_metrics(model, run.native, rec["bb_coords"], r["lig_pos"][kept])):
            m["refined_metrics"] = rm
    for k, m in enumerate(models):
        j = kept[k]
        m.update(refined_energy=float(r["energy"][j]), refined_index=j - k * n)
        if run.sym is not None:      # `symmetry` describes the cluster centre; the file written below holds the refined pose: its own record
            from . import symmetry as SY
            m["refined_symmetry"] = SY.record(rec["bb_coords"], r["lig_pos"][j], run.sym["n"], _center(model))
        if run.out_pdb:
            aa = pdbio.apply_pose_all_atom(lig["aa_coords"], lig["bb_coords"], cols["rot_update"][cen[k]], cols["tr_update"][cen[k]], center=center)
            aa = pdbio.apply_pose_all_atom(aa, start[k], r["rot_update"][j], r["tr_update"][j], center=center)
            _write_pose(run, model_path(run.out_pdb, m["rank"]), aa, r["lig_pos"][j])
    return models


def _top_models(run, clu):
    """dock_pair's `models`: the centres of up to top_k clusters in cluster order, each written as <out_pdb stem>_<rank>.pdb with the screen's REMARK line.
    Every model gains the per-pose summary of every analysis that is on (ANALYSES: pose, model_key).  run.bad: poses the clash filter removed - their key is
    NaN, so they come last, and a cluster one of them would lead is left out.  With min_bsa a centre that buries less is left out as well (`bsa_dropped`)."""
    top_k, radius, rule = clu
    model, rec, lig, cols, bad, sd = run.model, run.rec, run.lig, run.cols, run.bad, run.data.get("sterics")
    min_bsa = run.opts["surface"][0] if "surface" in run.opts else None
    min_cc, cc_dropped = (run.opts["density"][4] if "density" in run.opts else None), 0
    cl = cluster_trajectories(model, run.lig0, cols["rot_update"], cols["tr_update"], run.key, radius, rule, top_k)
    models, dropped = [], 0
    for c, n in zip(cl["center"], cl["size"]):
        c = int(c)
        if bad is not None and bad[c]:
            continue
        if min_bsa is not None and run.data["surface"]["bsa"][c] < min_bsa:
            dropped += 1
            continue
        if min_cc is not None and not run.data["density"]["cc"][c] >= min_cc:
            cc_dropped += 1
            continue
        k = len(models)
        models.append({"rank": k + 1, "index": c, "energy": float(cols["energy"][c]), "cluster_size": int(n)})
        for a in ANALYSES:
            if a.pose and a.name in run.opts:
                summary = a.pose(run.data[a.name], c)
                models[-1].update(summary if a.model_key is None else {a.model_key: summary})
        if run.out_pdb:
            aa = pdbio.apply_pose_all_atom(lig["aa_coords"], lig["bb_coords"], cols["rot_update"][c], cols["tr_update"][c], center=_center(model))
            _write_pose(run, model_path(run.out_pdb, k + 1), aa, _pose_bb(run, c), remarks=_remarks(sd, c))
    if run.native is not None and models:
        cen = [m["index"] for m in models]
        poses = rebuild_backbone(run.lig0, cols["rot_update"][cen], cols["tr_update"][cen], model.hp.family)
        for m, pm in zip(models, native_metrics(model, run.native, rec["bb_coords"], poses)):
            m["metrics"] = pm
    return {"models": models, "cluster_of": cl["cluster_of"], **({"bsa_dropped": dropped} if min_bsa is not None else {}),
            **({"density_dropped": cc_dropped} if min_cc is not None else {})}


def model_path(out_pdb, rank):
    """<stem>_<rank>.pdb next to out_pdb."""
    return os.path.splitext(out_pdb)[0] + f"_{rank}.pdb"
