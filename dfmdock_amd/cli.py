"""Checkpoint-driven command line of the sampling engine.

    python -m dfmdock_amd dock REC.pdb LIG.pdb --ckpt model_0.ckpt --features F.npz [--num-samples 120] [--out output.pdb]
    python -m dfmdock_amd sweep --db5 data/db5_test --ckpt model_0.ckpt [--num-samples 40] [--out-csv results.csv]
    python -m dfmdock_amd selfcheck REC.pdb LIG.pdb --ckpt model_0.ckpt --features F.npz
    python -m dfmdock_amd dock ... --restraints FILE [--restraint-rank satisfied|energy]
    python -m dfmdock_amd sweep ... --native-restraints K [--restraint-cutoff 8.0]
    python -m dfmdock_amd dock ... --top-k K [--cluster-radius 4.0] [--cluster-rule energy|size]
    python -m dfmdock_amd sweep ... --cluster-radius R [--top-k 10] [--cluster-rule energy|size]
    python -m dfmdock_amd refine REC.pdb LIG.pdb --ckpt model_0.ckpt --features F.npz --t-begin 0.1 [--num-samples 32] [--no-perturb]
    python -m dfmdock_amd dock ... --top-k K --refine-t T [--refine-samples 8]
    python -m dfmdock_amd dock|refine ... --native NATIVE_REC.pdb NATIVE_LIG.pdb
    python -m dfmdock_amd sweep ... --metrics gpu [--step-metrics steps.csv]
    python -m dfmdock_amd dock|refine ... --consensus [--rank consensus] [--consensus-top 0.5] [--contact-map map.npz]
    python -m dfmdock_amd dock|refine ... --write-restraints consensus.txt --restraint-top 10 [--restraint-upper 8.0]
    python -m dfmdock_amd sweep ... --consensus [--consensus-top 0.5]
    python -m dfmdock_amd dock|refine ... --interface-energy [--rank interface] [--ie-weights 0.18 1.0 0.5] [--ie-cutoff 8.0] [--energy-residues FILE]
    python -m dfmdock_amd dock|refine ... --pair-potential FILE.npz [--rank pairpot] [--pairpot-residues FILE] [--pair-counts FILE.npz]
    python -m dfmdock_amd dock|refine|rescore ... --density MAP.mrc --density-resolution 8 [--rank density] [--density-threshold 1.0] [--min-density-cc X]
                                                  [--density-residues FILE] [--write-simulated-map OUT.mrc]
    python -m dfmdock_amd dock|refine ... --affinity [--affinity-cutoff 5.5] [--contact-residues FILE]
    python -m dfmdock_amd dock|refine ... --hbonds [--bsa] [--hbond-cutoff 3.5] [--hbond-angle 90] [--salt-cutoff 4.0] [--hbond-residues FILE]
    python -m dfmdock_amd dock|refine ... --distogram [--rank distogram] [--distogram-map map.npz] [--distogram-restraints FILE] [--distogram-t 1e-3]
    python -m dfmdock_amd dock|refine ... --clash-screen [--clash-filter] [--clash-cutoff 3.0] [--contact-cutoff 5.0] [--clash-residues FILE]
    python -m dfmdock_amd dock|refine A.pdb A2.pdb ... --symmetry C3 [--symmetry-gain 0.5] [--symmetry-t-start 1] [--symmetry-tolerance 0.1] [--no-symmetry-snap]
    python -m dfmdock_amd rescore REC.pdb LIG.pdb --ckpt model_0.ckpt --features F.npz --decoys D.pdb [D2.pdb ...] | --coords C.npz | --poses P.npz
                                  [--decoy-chains A B] [--fit-tolerance 0.1] [--score-t 1e-3] [--scores scores.csv] [--top-k K [--refine-t T]] [every dock analysis]

  dock       <- src/inference_single.py:1-12 -> inference() (src/inference_base.py:601-670): num_samples (120) trajectories of
                num_steps (40), the minimum-energy one applied to the all-atom ligand, `output.pdb` written, {"energy": E} printed.
                The reference embeds both sequences with ESM-2 650M inside inference() (:606-609, get_esm_rep); that language
                model is outside this engine's scope, so its per-residue representations come in as
                a file: --features F.npz with `rec_esm [R,1280]`, `lig_esm [L,1280]` (the one-hot block is appended here from
                the PDB's own sequence, inference_base.py:192-215) or ready `rec_x [R,1301]`, `lig_x [L,1301]`.
  sweep      <- inference_mlsb.Sampler.run_sampling over PPIDataset('db5_test') (src/inference_mlsb.py:188-262,
                src/datasets/ppi_dataset.py:224-329): every `<id>.pt` of --db5 (ids from `test.txt` when present), the
                reference-schema CSV (src/inference_base.py:495-499) and the DockQ success-rate table.
  restraints no reference counterpart: interface distance restraints applied in the sampler (dfmdock_amd/restraints.py; file
             format there and in INTEGRATION.md).  `dock --restraints` keeps the minimum-energy trajectory among those satisfying the
             most groups (`--restraint-rank energy`: the plain minimum-energy rule); `sweep --native-restraints K` restrains every
             complex with K seeded native CA-CA contacts (< --restraint-cutoff A), the usual evaluation of guided docking.
  symmetry   no reference counterpart: Cn symmetric docking of a homo-oligomer (dfmdock_amd/symmetry.py, dfm_complex_set_symmetry).
             Both inputs are the same single chain (same sequence, rigid images of each other within --symmetry-tolerance A); the
             sampler's symmetry step keeps the monomer-to-monomer transform on a pure rotation by 2 pi m / n, the last step projects
             exactly (--no-symmetry-snap: it does not), the result line gains a `symmetry` object (n, m, theta, screw, sym_rmsd,
             closure, axis, axis_point; n >= 4: ring_clashes) and every written file holds all n chains.
  clustering no reference counterpart: trajectories grouped by ligand RMSD on the GPU (dfmdock_amd/cluster.py, dfm_pose_cluster).
             `dock --top-k K` writes the centres of the first K clusters as <out stem>_1.pdb ... <out stem>_K.pdb (model 1 of rule
             energy is output.pdb) and lists them under `models`; `sweep --cluster-radius R` adds `cluster` / `is_center` to the CSV and
             a top{K} success rate (any of the first K cluster centres reaches the DockQ threshold).
  refine     no reference counterpart as a command; the forward process is the reference's training-step noising (dfmdock_amd/refine.py):
             the pose the two PDB files are in is noised at --t-begin and the sampler runs down from there (dfm_refine); same output
             contract as `dock`.  `dock --top-k K --refine-t T` refines the K cluster centres in one batched call; <out stem>_k.pdb is
             then the minimum-energy refined pose of centre k and `models` carries both energies.
  metrics    c_rmsd, i_rmsd, l_rmsd, fnat and DockQ as the reference's compute_metrics defines them (src/utils/metrics.py:3-121), batched
             on the GPU (dfm_pose_metrics).  `dock / refine --native REC.pdb LIG.pdb` add the metrics of the kept pose (of every --top-k
             model, and of each centre before and after --refine-t) to the result line; the native is matched to the input residue by
             residue and may be in any frame.  `sweep --metrics gpu` evaluates the final poses on the GPU instead of the host (same
             definition; the CSV differs from the host's in the last digits), `sweep --step-metrics FILE.csv` (implies --metrics gpu)
             writes the metrics after EVERY step of every trajectory and adds, per complex, the step at which the minimum-energy
             trajectory first reaches DockQ >= 0.23 and the best DockQ seen along any trajectory to the summary.
  consensus  no reference counterpart: CONSRANK-style consensus contact scoring of the trajectories on the GPU (dfmdock_amd/consensus.py,
             dfm_pose_consensus) - a ranking that needs neither a native nor the energy head.  `dock / refine --consensus` add the
             consensus score, consensus rank and contact count of the kept pose to the result line; `--rank consensus` keeps the pose
             with the highest consensus instead of the minimum energy (and makes that order the clustering key of --top-k);
             `--contact-map FILE.npz` writes the R x L contact counts and frequencies, the per-residue interface counts and the residue
             labels; `--write-restraints FILE --restraint-top N` writes the N most frequent contacts as a restraint file for a second,
             guided run (`dock --restraints FILE`).  `--consensus-top FRAC`: only the best FRAC of the trajectories by energy are members
             of the ensemble (all are scored).  `sweep --consensus` appends `consensus` and `n_contacts` to the CSV and adds the DockQ
             success rates of the consensus-selected trajectory to the table.
  sterics    no reference counterpart: the all-atom clash / contact screen of every trajectory on the GPU (dfmdock_amd/sterics.py,
             dfm_pose_sterics) - the only step that reads the side chains.  CAPRI's rule: a clash is a pair of heavy atoms of the two
             chains closer than --clash-cutoff (3.0 A), the interface size the pairs closer than --contact-cutoff (5.0 A), and a model
             whose clash count exceeds the ensemble's mean by more than two standard deviations is flagged.  `dock / refine
             --clash-screen` add a `sterics` object for the kept pose (and for every --top-k model) to the result line and a REMARK line
             with the counts to every written model; `--clash-filter` removes the flagged trajectories before the selection, the
             consensus ranking and the clustering; `--clash-residues FILE` lists the kept model's counts per ligand residue.
  ifenergy   no reference counterpart: the physics rescoring step of docking pipelines on the GPU (dfmdock_amd/ifenergy.py,
             dfm_pose_iface_energy) - soft Lennard-Jones plus Coulomb with the dielectric 4 r over the heavy-atom pairs of the two chains
             within --ie-cutoff (8.0 A), element-wise AMBER-style LJ parameters and formal charges, no hydrogens.  `dock / refine
             --interface-energy` add an `interface_energy` object (rep, att, elec, total in kcal/mol, pairs, rank) for the kept pose and
             for every --top-k model; `--rank interface` keeps the pose with the lowest total instead of the minimum energy (and makes
             the totals the clustering key of --top-k; with --clash-filter the flagged poses are out, as under --rank consensus);
             total = w_rep rep + w_att att + w_elec elec with --ie-weights (default 0.18 1.0 0.5: ZRANK-like starting values, not
             fitted); `--energy-residues FILE` lists the kept model's unweighted sums per ligand residue.
  affinity   no reference counterpart: which residues touch which over all heavy atoms, on the GPU (dfmdock_amd/affinity.py,
             dfm_pose_rescon) - the residue pairs with two heavy atoms closer than --affinity-cutoff (5.5 A), counted by residue class -
             and the contacts-based affinity estimate IC-NIS over them and the non-interacting surface.  `dock / refine --affinity` add an
             `affinity` object (ic = AA AP AC PP PC CC, n_pairs, n_rec_res, n_lig_res, nis_apolar, nis_charged, dg in kcal/mol, kd in M)
             for the kept pose and for every --top-k model; `--contact-residues FILE` lists the kept model's residue pairs.  The
             coefficients, class tables and reference areas are starting values that are not verified or calibrated, the surface is this
             project's own Shrake-Rupley, and no agreement with the PRODIGY server is claimed.  Nothing is ranked by it.
  hbonds     no reference counterpart: the interface hydrogen bonds and salt bridges of every trajectory on the GPU (dfmdock_amd/hbonds.py,
             dfm_pose_hbonds).  The files carry no hydrogens, so the criteria are on heavy atoms only: a donor and an acceptor closer than
             --hbond-cutoff (3.5 A) with both antecedent angles at least --hbond-angle (90 degrees); a cation and an anion closer than
             --salt-cutoff (4.0 A), counted as residue pairs.  HIS is donor, acceptor and cation.  `dock / refine --hbonds` add n_hbond,
             hb_bb_bb, hb_bb_sc, hb_sc_sc and n_salt for the kept pose and for every --top-k model, and with --bsa in the same run n_unsat:
             the donors and acceptors the pose buries completely and leaves without a bond.  `--hbond-residues FILE` lists the kept
             model's counts per residue of both chains (and <FILE stem>_<rank> those of every --top-k model).  No agreement with the
             counts of PISA or HBPLUS is claimed.  Nothing is ranked or filtered by them.
  pairpot    no reference counterpart: a tabulated, distance-binned, type-pair potential of every trajectory on the GPU
             (dfmdock_amd/pairpot.py, dfm_pose_pairpot) - E = the sum over heavy-atom pairs of table[type_a][type_b][bin(r)], the shape of
             DFIRE, DOPE, ITScore-PP or a table fitted to one's own decoys.  The project ships NO table and claims nothing about any
             potential's ranking quality: `--pair-potential FILE.npz` names the user's file (edges [NB+1] in A, table [T,T,NB] in kcal/mol
             indexed ligand type, receptor type, bin, type_names [T]: RES:ATOM, RES:*, *:ATOM, @ELEMENT or *, the first that fits an atom
             in that order; an atom none fits is left out and counted in n_untyped) and adds a `pair_potential` object (energy, n_pairs,
             n_untyped, T, NB, cutoff) for the kept pose and for every --top-k model; `--rank pairpot` keeps the pose with the lowest
             energy (ties: the lower index); `--pairpot-residues FILE` lists the kept model's energy per ligand residue; `--pair-counts
             FILE.npz` writes the pair counts [T,T,NB] of every written model - what a potential of this shape is fitted from.
  density    no reference counterpart: the fit of every trajectory into a cryo-EM map on the GPU (dfmdock_amd/density.py,
             dfm_pose_density).  `dock / refine / rescore --density MAP.mrc --density-resolution R` read an MRC map the RECEPTOR already
             sits in and add a `density` object - density_cc (the overlap correlation of the simulated complex with the map; atoms are
             Gaussians of sigma = R / (pi sqrt(2)) weighted by atomic number), density_inclusion (the share of the ligand's heavy atoms in
             density at or above `--density-threshold`, default 1.0, in units of the normalised map) and density_n_outside - for the kept
             pose and for every --top-k model; `--rank density` keeps the pose with the highest correlation; `--min-density-cc X` keeps
             cluster centres below X out of the models; `--density-residues FILE` and `--write-simulated-map OUT.mrc` describe the kept
             model.  Rigid ligand, no density-guided sampling, no local resolution, masks or FSC, no claim about real maps.
  distogram  the model's own distogram head (second model family only: EGNN_Net.to_dist, 64 distance bins per residue pair) evaluated at
             every final pose and reduced on the GPU (dfmdock_amd/distogram.py, dfm_score_distogram).  `dock / refine --distogram` add
             dist_nll (the reference's distogram_loss of the pose's own CA-CA distances under the prediction made at that pose: lower =
             the pose agrees better with what the model expects), dist_nll_near (the same over pairs closer than the model's cut-off) and
             exp_contacts (expected number of residue pairs within 7.85 A) for the kept pose and for every --top-k model; `--rank
             distogram` keeps the pose with the lowest dist_nll (and makes it the clustering key of --top-k; with --clash-filter the
             flagged poses are out); `--distogram-map FILE.npz` writes the predicted contact probabilities averaged over all
             trajectories and the expected-distance map of every written model; `--distogram-restraints FILE` writes the --restraint-top
             most probable contacts as a restraint file (upper bound --restraint-upper, weight = probability) for a second, guided run;
             `--distogram-t T` (default 1e-3) is the diffusion time of the evaluation.  A first-family checkpoint is refused before
             sampling.
  rescore    no reference counterpart as a command: decoys made elsewhere (another docking program, an earlier run) ranked with the model's
             energy head and screened, clustered and described with every analysis of `dock`.  The decoys are rigid images of the ligand
             PDB: `--decoys` (PDB files, every MODEL; matched to the input residue by residue, `--decoy-chains` when the chain ids
             differ; a model that carries the receptor may sit in any frame), `--coords` (backbones) or `--poses` (rot_update /
             tr_update as they are).  Coordinates are fitted on the GPU (dfmdock_amd/fit.py, dfm_pose_fit); a decoy whose fit leaves more
             than --fit-tolerance (0.1 A) backbone RMSD is rejected: no energy, never kept, never a model.  The energy is the model's at
             --score-t (default: the end of the sampler's grid).  Same output contract as `dock`, plus `fit` and `num_decoys`;
             `--scores FILE.csv` lists every decoy; `--top-k K --refine-t T` hands the cluster centres to the local refinement.
  selfcheck  no reference counterpart: dfm_complex_selfcheck on the pair (what `dock` and `sweep` run once per complex anyway).

--ckpt takes the Lightning checkpoint the reference loads (src/inference_base.py:611-616; read without Lightning / omegaconf by
weights.load_lightning_checkpoint) or a bare state_dict; the model family (Score_Net / EGNN_Net) is read off the keys.
Everything computes on the MI355X through the C ABI; without a GPU the commands fail (no CPU fallback).
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
from typing import Callable, NamedTuple

import numpy as np

DOCKQ_THRESHOLDS = (("acceptable", 0.23), ("medium", 0.49), ("high", 0.80))      # CAPRI classes by DockQ


def _add_native(p):
    p.add_argument("--native", nargs=2, default=None, metavar=("REC.pdb", "LIG.pdb"),
                   help="native complex (same residues as the input, any frame): add c_rmsd / i_rmsd / l_rmsd / fnat / DockQ to the result")


def _add_consensus(p):
    p.add_argument("--consensus", action="store_true",
                   help="score the trajectories by consensus contacts (adds a `consensus` object to the result line)")
    p.add_argument("--rank", default="energy", choices=["energy", "consensus", "interface", "distogram", "pairpot", "density"],
                   help="which trajectory is kept: the minimum energy (default), the highest consensus score (implies --consensus), the "
                        "lowest interface energy (implies --interface-energy), the lowest distogram nll (implies --distogram), the lowest "
                        "tabulated pair potential (dock / refine only; needs --pair-potential) or the highest map correlation (needs --density)")
    p.add_argument("--consensus-top", type=float, default=None, metavar="FRAC",
                   help="with --consensus: members of the ensemble are the best FRAC of the trajectories by energy (default 1.0: all)")
    p.add_argument("--contact-map", default=None, metavar="FILE.npz",
                   help="write the consensus contact map: count, freq, rec_count, lig_count, M, cutoff, residue labels (implies --consensus)")
    p.add_argument("--write-restraints", default=None, metavar="FILE",
                   help="write the --restraint-top most frequent consensus contacts as a restraint file (implies --consensus)")
    p.add_argument("--restraint-top", type=int, default=None, metavar="N",
                   help="with --write-restraints / --distogram-restraints: number of contacts (default 10)")
    p.add_argument("--restraint-upper", type=float, default=None, metavar="U",
                   help="with --write-restraints / --distogram-restraints: upper bound on the CA-CA distance of every written contact (A, default 8.0)")


def _add_distogram(p):
    p.add_argument("--distogram", action="store_true",
                   help="evaluate the model's distogram head at every final pose (family-1 checkpoints): adds dist_nll, dist_nll_near, "
                        "exp_contacts to the result line and to every model")
    p.add_argument("--distogram-map", default=None, metavar="FILE.npz",
                   help="write pcontact_mean [R,L] over all trajectories and the expected-distance map of every written model (implies --distogram)")
    p.add_argument("--distogram-restraints", default=None, metavar="FILE",
                   help="write the --restraint-top most probable predicted contacts as a restraint file (implies --distogram)")
    p.add_argument("--distogram-t", type=float, default=None, metavar="T", help="with --distogram: diffusion time of the evaluation (default 1e-3)")


def _add_sterics(p):
    p.add_argument("--clash-screen", action="store_true",
                   help="all-atom clash / contact screen of every trajectory (adds a `sterics` object to the result line, a REMARK to the models)")
    p.add_argument("--clash-filter", action="store_true",
                   help="remove the trajectories CAPRI's rule flags (clashes > ensemble mean + 2 std) before any selection (implies --clash-screen)")
    p.add_argument("--clash-cutoff", type=float, default=None, metavar="A", help="with --clash-screen: heavy-atom distance of a clash (default 3.0)")
    p.add_argument("--contact-cutoff", type=float, default=None, metavar="A",
                   help="with --clash-screen: heavy-atom distance of an interface contact (default 5.0, >= --clash-cutoff)")
    p.add_argument("--clash-residues", default=None, metavar="FILE",
                   help="write the kept model's clash / contact counts per ligand residue (implies --clash-screen)")


def _add_interface(p):
    p.add_argument("--interface-energy", action="store_true",
                   help="soft LJ + Coulomb interface energy of every trajectory (adds an `interface_energy` object to the result line and to every model)")
    p.add_argument("--ie-weights", type=float, nargs=3, default=None, metavar=("REP", "ATT", "ELEC"),
                   help="with --interface-energy: weights of the total (default 0.18 1.0 0.5, starting values that are not fitted)")
    p.add_argument("--ie-cutoff", type=float, default=None, metavar="A", help="with --interface-energy: heavy-atom pair cutoff (default 8.0, at most 16)")
    p.add_argument("--energy-residues", default=None, metavar="FILE",
                   help="write the kept model's LJ and Coulomb interface energy per ligand residue (implies --interface-energy)")


def _add_pairpot(p):
    p.add_argument("--pair-potential", default=None, metavar="FILE.npz",
                   help="tabulated pair potential of every trajectory from the user's table (edges, table, type_names; no table is shipped): "
                        "adds a `pair_potential` object to the result line and to every model")
    p.add_argument("--pairpot-residues", default=None, metavar="FILE",
                   help="with --pair-potential: write the kept model's pair potential per ligand residue")
    p.add_argument("--pair-counts", default=None, metavar="FILE.npz",
                   help="with --pair-potential: write the pair counts [T,T,NB] of every written model with type_names and edges")


def _add_affinity(p):
    p.add_argument("--affinity", action="store_true",
                   help="residue contacts by class and the contacts-based affinity estimate of every trajectory (adds an `affinity` object "
                        "to the result line and to every model; IC-NIS with starting values that are not calibrated)")
    p.add_argument("--affinity-cutoff", type=float, default=None, metavar="A",
                   help="with --affinity: heavy-atom distance of a residue contact (default 5.5, at most 16)")
    p.add_argument("--contact-residues", default=None, metavar="FILE",
                   help="write the kept model's residue pairs in contact, one per line (implies --affinity)")


def _add_hbonds(p):
    p.add_argument("--hbonds", action="store_true",
                   help="interface hydrogen bonds and salt bridges of every trajectory, heavy-atom criteria (adds n_hbond, hb_bb_bb, hb_bb_sc, "
                        "hb_sc_sc, n_salt - with --bsa also n_unsat - to the result line and to every model)")
    p.add_argument("--hbond-cutoff", type=float, default=None, metavar="A", help="with --hbonds: donor - acceptor distance (default 3.5, at most 8)")
    p.add_argument("--hbond-angle", type=float, default=None, metavar="DEG",
                   help="with --hbonds: smallest angle at the donor and at the acceptor, taken to their antecedents (default 90, in [90, 180))")
    p.add_argument("--salt-cutoff", type=float, default=None, metavar="A", help="with --hbonds: cation - anion distance (default 4.0, at most 8)")
    p.add_argument("--hbond-residues", default=None, metavar="FILE",
                   help="write the kept model's hydrogen bonds and salt-bridge atom pairs per residue of both chains (implies --hbonds)")


def _add_surface(p):
    p.add_argument("--bsa", action="store_true",
                   help="buried solvent-accessible surface area of every trajectory (adds bsa, bsa_rec, bsa_lig in A^2 to the result line and to every model)")
    p.add_argument("--min-bsa", type=float, default=None, metavar="A",
                   help="with --top-k: cluster centres that bury less than A A^2 do not become a model (implies --bsa)")
    p.add_argument("--interface-residues", default=None, metavar="FILE",
                   help="write the kept model's buried area per residue of both chains (implies --bsa)")
    p.add_argument("--probe", type=float, default=None, metavar="A", help="with --bsa: probe radius (default 1.4)")
    p.add_argument("--sphere-points", type=int, default=None, metavar="K",
                   help="with --bsa: sphere points per atom, a multiple of 64 in 64 .. 256 (default 128)")


def _add_models(p, what):
    """--top-k and what goes with it, for dock and rescore."""
    p.add_argument("--top-k", type=int, default=None, metavar="K",
                   help=f"cluster the {what} and write the first K cluster centres as <out stem>_1.pdb ... _K.pdb")
    p.add_argument("--cluster-radius", type=float, default=4.0, help="with --top-k: ligand RMSD radius of a cluster (A)")
    p.add_argument("--cluster-rule", default="energy", choices=["energy", "size"],
                   help="with --top-k: leader clustering in key order (default) or greedy by cluster size")
    p.add_argument("--refine-t", type=float, default=None, metavar="T",
                   help="with --top-k: refine every cluster centre locally from t_begin = T (one batched call)")
    p.add_argument("--refine-samples", type=int, default=8, metavar="n", help="with --refine-t: trajectories per cluster centre")


def _add_symmetry(p):
    p.add_argument("--symmetry", default=None, metavar="Cn",
                   help="Cn symmetric docking of a homo-oligomer (C3 or 3; n in 2 .. 24): both inputs are the same single chain; the "
                        "sampler keeps every pose on a closed n-mer and the written files hold all n chains")
    p.add_argument("--symmetry-gain", type=float, default=None, metavar="G",
                   help="with --symmetry: fraction of the angle error and of the screw translation one step removes, in (0, 1] (default 0.5)")
    p.add_argument("--symmetry-t-start", type=float, default=None, metavar="T",
                   help="with --symmetry: the symmetry step runs on the steps with t <= T (default 1: every step)")
    p.add_argument("--symmetry-tolerance", type=float, default=None, metavar="A",
                   help="with --symmetry: largest Kabsch rmsd (A) of the two input monomers' backbones (default 0.1)")
    p.add_argument("--no-symmetry-snap", action="store_true",
                   help="with --symmetry: the last step follows the gains like every other one instead of projecting exactly")


def symmetry_parser():
    """The options of --symmetry as a parser of their own: parse_args takes them out of the command line of dock and refine before the
    command's parser reads the rest (the command's own option list stays what it was; its help shows these in the epilog)."""
    p = argparse.ArgumentParser(prog="python -m dfmdock_amd dock|refine", add_help=False, allow_abbrev=False, usage=argparse.SUPPRESS)
    _add_symmetry(p.add_argument_group("Cn symmetric docking (dock and refine)"))
    return p


def _symmetry_epilog():
    return symmetry_parser().format_help().strip()


SYMMETRY_DESTS = ("symmetry", "symmetry_gain", "symmetry_t_start", "symmetry_tolerance", "no_symmetry_snap")


def symmetry_kwargs(args, ap=None):
    """The driver keywords of --symmetry and its options (none without it); the options alone are an error."""
    def bad(msg):
        if ap is not None:
            ap.error(msg)
        raise SystemExit(msg)
    if not hasattr(args, "symmetry"):      # a namespace of the command's parser alone (parse_args adds these): no symmetry
        return {}
    given = [o for o, v in (("--symmetry-gain", args.symmetry_gain), ("--symmetry-t-start", args.symmetry_t_start),
                            ("--symmetry-tolerance", args.symmetry_tolerance), ("--no-symmetry-snap", args.no_symmetry_snap or None))
             if v is not None]
    if args.symmetry is None:
        if given:
            bad(f"{', '.join(given)} need(s) --symmetry")
        return {}
    from .symmetry import SymmetryParams, parse_symmetry
    try:
        n = parse_symmetry(args.symmetry)
        par = SymmetryParams(**({} if args.symmetry_gain is None else {"gain_rot": args.symmetry_gain, "gain_tr": args.symmetry_gain}),
                             **({} if args.symmetry_t_start is None else {"t_start": args.symmetry_t_start}),
                             snap_last=0 if args.no_symmetry_snap else 1)
    except ValueError as e:
        bad(str(e))
    kw = {"symmetry": n, "symmetry_params": par}
    if args.symmetry_tolerance is not None:
        if not (np.isfinite(args.symmetry_tolerance) and args.symmetry_tolerance >= 0):
            bad("--symmetry-tolerance must be finite and >= 0")
        kw["symmetry_tolerance"] = args.symmetry_tolerance
    return kw


def _add_density(p):
    p.add_argument("--density", default=None, metavar="MAP.mrc",
                   help="cryo-EM density fit of every trajectory against an MRC map the receptor already sits in: adds a `density` object "
                        "(density_cc, density_inclusion, density_n_outside) to the result line and its three figures to every model; `--rank "
                        "density` keeps the pose with the highest correlation")
    p.add_argument("--density-resolution", type=float, default=None, metavar="R",
                   help="with --density (required): the map's resolution in A; atoms are simulated as Gaussians of sigma = R / (pi sqrt(2))")
    p.add_argument("--density-threshold", type=float, default=None, metavar="T",
                   help="with --density: an atom counts as included at or above T, in units of the normalised map (default 1.0)")
    p.add_argument("--min-density-cc", type=float, default=None, metavar="X",
                   help="with --density and --top-k: leave a cluster centre whose correlation is below X out of the models")
    p.add_argument("--density-residues", default=None, metavar="FILE",
                   help="with --density: write the mean weighted map value per ligand residue over the kept pose and the models")
    p.add_argument("--write-simulated-map", default=None, metavar="OUT.mrc",
                   help="with --density: write the kept model simulated on the map's grid, for visual checks")


def density_parser():
    """The options of --density as a parser of their own, as symmetry_parser: parse_args takes them out of the command line of dock,
    refine and rescore before the command's parser reads the rest; the command's help shows them in the epilog."""
    p = argparse.ArgumentParser(prog="python -m dfmdock_amd dock|refine|rescore", add_help=False, allow_abbrev=False, usage=argparse.SUPPRESS)
    _add_density(p.add_argument_group("cryo-EM density fit (dock, refine and rescore)"))
    return p


DENSITY_DESTS = ("density", "density_resolution", "density_threshold", "min_density_cc", "density_residues", "write_simulated_map")


def _density_epilog():
    return density_parser().format_help().strip()


def _add_common(p):
    p.add_argument("--ckpt", required=True, help="Lightning checkpoint or bare state_dict (torch.save)")
    p.add_argument("--num-steps", type=int, default=40)
    p.add_argument("--precision", default="mfma16", choices=["mfma16", "f16", "fp32", "bf16"],
                   help="mfma16 (default): 16-bit MFMA engine, self-checked against fp32 once per complex; fp32: exact; bf16: deprecated alias of mfma16")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", type=int, default=None, help="GPU index (default: LOCAL_RANK, else 0)")
    p.add_argument("--max-batch", type=int, default=256, help="trajectories in flight per dfm_sample call")
    p.add_argument("--no-selfcheck", action="store_true", help="skip the per-complex fp32-vs-16-bit check")
    p.add_argument("--on-selfcheck-fail", default="fp32", choices=["fp32", "raise", "warn"],
                   help="a failed check switches the complex to the fp32 engine (default), aborts, or only warns")


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m dfmdock_amd", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dock", help="dock one receptor / ligand PDB pair (inference_single.py)", epilog=_symmetry_epilog() + "\n\n" + _density_epilog(),
                       formatter_class=argparse.RawDescriptionHelpFormatter)
    d.add_argument("pdb_1", help="receptor PDB")
    d.add_argument("pdb_2", help="ligand PDB")
    d.add_argument("--features", required=True, help=".npz with rec_esm / lig_esm [n,1280] (or rec_x / lig_x [n,1301])")
    d.add_argument("--num-samples", type=int, default=120)
    d.add_argument("--out", default="output.pdb")
    d.add_argument("--json", default=None, help="also write the result line to this file")
    d.add_argument("--restraints", default=None, help="interface restraint file: REC_RESIDUES LIG_RESIDUES UPPER [WEIGHT] per line")
    d.add_argument("--restraint-rank", default="satisfied", choices=["satisfied", "energy"],
                   help="with --restraints: keep the minimum energy among the trajectories satisfying the most groups (default) "
                        "or the plain minimum energy")
    _add_models(d, "trajectories")
    _add_native(d)
    for a in ANALYSES:
        a.add(d)
    _add_common(d)
    r = sub.add_parser("refine", help="refine the pose the two PDB files are in (partial diffusion from --t-begin)", epilog=_symmetry_epilog() + "\n\n" + _density_epilog(),
                       formatter_class=argparse.RawDescriptionHelpFormatter)
    r.add_argument("pdb_1", help="receptor PDB")
    r.add_argument("pdb_2", help="ligand PDB, in the pose to refine")
    r.add_argument("--features", required=True, help=".npz with rec_esm / lig_esm [n,1280] (or rec_x / lig_x [n,1301])")
    r.add_argument("--t-begin", type=float, default=0.1, help="time the forward process noises the pose to (eps < t <= 1)")
    r.add_argument("--num-samples", type=int, default=32)
    r.add_argument("--no-perturb", action="store_true", help="start every trajectory at the pose itself")
    r.add_argument("--out", default="output.pdb")
    r.add_argument("--json", default=None, help="also write the result line to this file")
    r.add_argument("--restraints", default=None, help="interface restraint file (as for dock)")
    _add_native(r)
    for a in ANALYSES:
        a.add(r)
    _add_common(r)
    x = sub.add_parser("rescore", help="rank, screen and describe decoys made elsewhere with the model's energy and every analysis of dock",
                       epilog=_density_epilog(), formatter_class=argparse.RawDescriptionHelpFormatter)
    x.add_argument("pdb_1", help="receptor PDB")
    x.add_argument("pdb_2", help="ligand PDB: the conformation the decoys are rigid images of")
    x.add_argument("--features", required=True, help=".npz with rec_esm / lig_esm [n,1280] (or rec_x / lig_x [n,1301])")
    src = x.add_mutually_exclusive_group(required=True)
    src.add_argument("--decoys", nargs="+", default=None, metavar="FILE.pdb", help="decoy files: every MODEL of every file, in order")
    src.add_argument("--coords", default=None, metavar="FILE.npz", help="decoy backbones: lig_pos [P,L,3,3] and optionally rec_pos [P,R,3,3]")
    src.add_argument("--poses", default=None, metavar="FILE.npz", help="decoys as poses: rot_update [P,3] and tr_update [P,3], taken as they are")
    x.add_argument("--decoy-chains", nargs=2, default=None, metavar=("RCHAINS", "LCHAINS"),
                   help="with --decoys: the chain ids of the receptor and of the ligand in the decoy files (default: those of the input files)")
    x.add_argument("--fit-tolerance", type=float, default=0.1, metavar="A",
                   help="a decoy whose rigid fit leaves a larger backbone RMSD is rejected (default 0.1)")
    x.add_argument("--score-t", type=float, default=None, metavar="T", help="time of the energy evaluation (default: the end of the sampler's grid)")
    x.add_argument("--out", default="output.pdb")
    x.add_argument("--json", default=None, help="also write the result line to this file")
    x.add_argument("--scores", default=None, metavar="FILE.csv",
                   help="one row per decoy: source, model, fit_rmsd, rec_rmsd, rejected, energy, rank")
    _add_models(x, "decoys")
    _add_native(x)
    for a in ANALYSES:
        a.add(x)
    _add_common(x)
    s = sub.add_parser("sweep", help="sample every complex of a DB5-style directory (inference_mlsb.py run_sampling)")
    s.add_argument("--db5", required=True, help="directory of <id>.pt files (+ optional test.txt with the ids to run)")
    s.add_argument("--num-samples", type=int, default=40)
    s.add_argument("--out-csv", default="results.csv")
    s.add_argument("--summary", default=None, help="write the success-rate table + self-check records as JSON")
    s.add_argument("--traj-dir", default=None, help="write one multi-MODEL PDB per trajectory (save_trj)")
    s.add_argument("--no-global-rotation", action="store_true", help="skip the loader's random rotation (ppi_dataset.py:309)")
    s.add_argument("--limit", type=int, default=None, help="first N ids only")
    s.add_argument("--native-restraints", type=int, default=None, metavar="K",
                   help="restrain every complex with K seeded native CA-CA contacts (adds restraint columns to the CSV)")
    s.add_argument("--restraint-cutoff", type=float, default=8.0, help="contact cutoff and upper bound of --native-restraints (A)")
    s.add_argument("--cluster-radius", type=float, default=None, metavar="R",
                   help="cluster every complex's trajectories by ligand RMSD (adds cluster / is_center to the CSV and a top-K success rate)")
    s.add_argument("--top-k", type=int, default=10, metavar="K", help="with --cluster-radius: clusters per complex (default 10)")
    s.add_argument("--cluster-rule", default="energy", choices=["energy", "size"], help="with --cluster-radius: clustering rule")
    s.add_argument("--metrics", default="host", choices=["host", "gpu"],
                   help="where the final poses are scored: host (default, numpy) or gpu (dfm_pose_metrics, one call per complex)")
    s.add_argument("--step-metrics", default=None, metavar="FILE.csv",
                   help="also write the metrics after every step of every trajectory (implies --metrics gpu)")
    s.add_argument("--consensus", action="store_true",
                   help="consensus contact score of every trajectory within its complex (adds consensus / n_contacts to the CSV and the "
                        "success rates of the consensus-selected trajectory to the table)")
    s.add_argument("--consensus-top", type=float, default=None, metavar="FRAC",
                   help="with --consensus: members of the ensemble are the best FRAC of a complex's trajectories by energy")
    _add_common(s)
    c = sub.add_parser("selfcheck", help="fp32-vs-16-bit check + fp16 range telemetry of one pair")
    c.add_argument("pdb_1")
    c.add_argument("pdb_2")
    c.add_argument("--features", required=True)
    c.add_argument("--n-eval", type=int, default=4)
    _add_common(c)
    return ap


def parse_args(argv=None):
    ap = build_parser()
    argv = list(sys.argv[1:] if argv is None else argv)
    sym = None
    if argv and argv[0] in ("dock", "refine"):      # the symmetry options: their own parser first, the command's parser reads the rest
        sym, argv = symmetry_parser().parse_known_args(argv)
    den = None
    if argv and argv[0] in ("dock", "refine", "rescore"):      # the density options likewise
        den, argv = density_parser().parse_known_args(argv)
    args = ap.parse_args(argv)
    for dest in DENSITY_DESTS:
        setattr(args, dest, getattr(den, dest) if den is not None else None)
    for dest in SYMMETRY_DESTS:
        setattr(args, dest, getattr(sym, dest) if sym is not None else (False if dest == "no_symmetry_snap" else None))
    symmetry_kwargs(args, ap)      # (checked here, before anything is loaded)
    if args.cmd in ("dock", "rescore") and args.refine_t is not None and args.top_k is None:
        ap.error("--refine-t refines the cluster centres: it needs --top-k")
    if args.cmd == "rescore":
        if args.decoy_chains is not None and args.decoys is None:
            ap.error("--decoy-chains names the chains of --decoys files")
        if not (args.fit_tolerance >= 0.0):
            ap.error("--fit-tolerance must be >= 0")
        for path in (args.decoys or []) + [p for p in (args.coords, args.poses) if p]:
            if not os.path.isfile(path):
                ap.error(f"{path}: no such file")
    if args.cmd == "sweep" and args.step_metrics is not None:
        args.metrics = "gpu"
    if args.cmd in ("dock", "refine", "rescore"):
        for a in ANALYSES:
            a.check(ap, args)
    elif getattr(args, "rank", None) in ("pairpot", "density"):
        ap.error(f"--rank {args.rank} is offered by dock and refine")
    if args.cmd in ("dock", "refine", "rescore", "sweep"):
        if args.consensus_top is not None and not args.consensus:
            ap.error("--consensus-top selects the members of the consensus ensemble: it needs --consensus")
        args.consensus_top = 1.0 if args.consensus_top is None else args.consensus_top
        if not (0.0 < args.consensus_top <= 1.0):
            ap.error("--consensus-top must be in (0, 1]")
    return args


def load_model(args):
    from . import distributed as D
    from . import engine
    from .weights import load_lightning_checkpoint, pack_blob
    dev = args.device if args.device is not None else D.dist_env()[1]
    engine.set_device(dev)
    sd, hp = load_lightning_checkpoint(args.ckpt)
    return engine.Model(pack_blob(sd, hp), hp), hp


def load_pair(pdb_1, pdb_2, features, lm_embed_dim=1301):
    """Two PDB files + the features file -> (rec, lig, rec_x, lig_x); the residue counts of the features must match the residues
    get_info_from_pdb keeps (N, CA and C present, HETATM dropped - pdbio.backbone_from_atoms)."""
    from . import pdbio
    from .synthetic import seq_to_onehot
    rec = pdbio.backbone_from_atoms(pdbio.read_pdb(pdb_1))
    lig = pdbio.backbone_from_atoms(pdbio.read_pdb(pdb_2))
    f = np.load(features, allow_pickle=False)
    xs = []
    for side, chain in (("rec", rec), ("lig", lig)):
        n = len(chain["seq"])
        if side + "_x" in f:
            x = np.asarray(f[side + "_x"], np.float32)
        elif side + "_esm" in f:
            esm = np.asarray(f[side + "_esm"], np.float32)
            if esm.ndim != 2 or esm.shape[0] != n:
                raise ValueError(f"{features}: {side}_esm is {esm.shape}, the PDB has {n} residues with N, CA and C")
            x = np.concatenate([esm, seq_to_onehot(chain["seq"])], axis=1)
        else:
            raise ValueError(f"{features}: need `{side}_esm` [n,1280] or `{side}_x` [n,{lm_embed_dim}]")
        if x.shape != (n, lm_embed_dim):
            raise ValueError(f"{features}: {side} features are {x.shape}, the PDB has {n} residues with N, CA and C "
                             f"(expected ({n}, {lm_embed_dim}))")
        if side + "_seq" in f and str(f[side + "_seq"]) != chain["seq"]:
            raise ValueError(f"{features}: {side}_seq does not match the sequence read from the PDB")
        xs.append(x)
    return rec, lig, xs[0], xs[1]


def load_native(paths):
    """--native REC.pdb LIG.pdb -> (receptor [R,3,3], ligand [L,3,3]) backbones, residues as pdbio.backbone_from_atoms keeps them."""
    from . import pdbio
    return tuple(np.asarray(pdbio.backbone_from_atoms(pdbio.read_pdb(p))["bb_coords"], np.float32) for p in paths)


def step_summary(step_rows, rows, threshold=0.23):
    """Per complex, from the long table of run_set(step_metrics=True): the step at which the minimum-energy trajectory (what inference()
    keeps) first reaches DockQ >= threshold (None: never) and the best DockQ seen after any step of any trajectory."""
    top = {}
    for r in rows:
        if r["id"] not in top or (r["energy"], int(r["index"])) < (top[r["id"]]["energy"], int(top[r["id"]]["index"])):
            top[r["id"]] = r
    out = {}
    for s in sorted(step_rows, key=lambda x: (x["id"], int(x["index"]), int(x["step"]))):
        o = out.setdefault(s["id"], {"top1_first_acceptable_step": None, "best_DockQ_any_step": float("-inf")})
        if float(s["DockQ"]) > o["best_DockQ_any_step"]:
            o["best_DockQ_any_step"] = float(s["DockQ"])
        if s["id"] in top and str(s["index"]) == str(top[s["id"]]["index"]) and o["top1_first_acceptable_step"] is None \
                and float(s["DockQ"]) >= threshold:
            o["top1_first_acceptable_step"] = int(s["step"])
    return out


def residue_labels(chain):
    """`chain:resnum[icode]` of every residue of a pdbio.backbone_from_atoms dict, the names restraint files use."""
    return np.array([f"{k[0]}:{int(k[1])}{k[2] if k[2] != ' ' else ''}" for k in chain["residues"]])


def check_consensus(ap, args):
    if args.rank == "consensus" or args.contact_map or args.write_restraints:
        args.consensus = True


def consensus_kwargs(args, model=None):
    """Driver keyword arguments of the consensus flags of dock / refine: none without them."""
    if not args.consensus:
        return {}
    return dict(consensus=True, rank=args.rank, consensus_top=args.consensus_top)


def consensus_outputs(args, model, res, rec, lig, line, kw):
    """The consensus part of a dock / refine result: the `consensus` object of the line, --contact-map and --write-restraints."""
    if not args.consensus:
        return
    from . import consensus as CS
    cd = res["consensus_data"]
    line.update(consensus=res["consensus"], index=res["index"])
    if args.contact_map:
        np.savez(args.contact_map, count=cd["count"], freq=cd["freq"], rec_count=cd["rec_count"], lig_count=cd["lig_count"],
                 M=np.int64(cd["M"]), cutoff=np.float64(cd["cutoff"]), rec_residues=residue_labels(rec), lig_residues=residue_labels(lig))
        line.update(contact_map=os.path.abspath(args.contact_map))
    if args.write_restraints:
        groups = CS.contact_groups(cd["count"], cd["M"], args.restraint_top, upper=args.restraint_upper)
        CS.write_restraints(args.write_restraints, groups, rec, lig,
                            header=f"top {len(groups)} consensus contacts of {len(cd['consensus'])} trajectories ({cd['M']} members, "
                                   f"contact cutoff {cd['cutoff']:g} A): REC LIG UPPER WEIGHT(= contact frequency)")
        line.update(restraints_written=os.path.abspath(args.write_restraints), restraints_written_n=len(groups))


def check_distogram(ap, args):
    if args.rank == "distogram" or args.distogram_map or args.distogram_restraints:
        args.distogram = True
    if not args.distogram and args.distogram_t is not None:
        ap.error("--distogram-t is the time of the --distogram evaluation: it needs it")
    args.distogram_t = 1e-3 if args.distogram_t is None else args.distogram_t
    if not (0.0 < args.distogram_t <= 1.0):
        ap.error("--distogram-t must be in (0, 1]")
    # the file of --write-restraints / --distogram-restraints: checked here, once both have been implied
    if not (args.write_restraints or args.distogram_restraints) and (args.restraint_top is not None or args.restraint_upper is not None):
        ap.error("--restraint-top / --restraint-upper describe the file of --write-restraints / --distogram-restraints: they need one")
    args.restraint_top = 10 if args.restraint_top is None else args.restraint_top
    args.restraint_upper = 8.0 if args.restraint_upper is None else args.restraint_upper
    if args.restraint_top < 1:
        ap.error("--restraint-top must be >= 1")
    if not (args.restraint_upper > 0 and np.isfinite(args.restraint_upper)):
        ap.error("--restraint-upper must be finite and > 0")


def distogram_kwargs(args, model=None):
    """Driver keyword arguments of the distogram flags of dock / refine: none without them.  The head exists in the second model
    family only: a first-family checkpoint with any of the flags ends the command here, before anything is sampled."""
    if not args.distogram:
        return {}
    if model.hp.family != 1:
        raise SystemExit("--distogram / --rank distogram / --distogram-map / --distogram-restraints need a family-1 checkpoint (EGNN_Net "
                         "has the distogram head to_dist, Score_Net does not); this checkpoint is family 0")
    return dict(distogram=True, rank=args.rank, distogram_t=args.distogram_t,
                distogram_maps=bool(args.distogram_map or args.distogram_restraints))


def distogram_outputs(args, model, res, rec, lig, line, kw):
    """The distogram part of a dock / refine result: dist_nll, dist_nll_near, exp_contacts of the line (the models carry theirs),
    --distogram-map and --distogram-restraints."""
    if not args.distogram:
        return
    from . import consensus as CS
    from . import distogram as DG
    dd, d = res["distogram_data"], res["distogram"]
    line.update(dist_nll=d["dist_nll"], dist_nll_near=d["dist_nll_near"], exp_contacts=d["exp_contacts"], dist_rank=d["rank"],
                distogram_t=d["t"], index=res["index"])
    if args.distogram_map:
        idx = [int(res["index"])] + [int(m["index"]) for m in res.get("models", [])]
        np.savez(args.distogram_map, pcontact_mean=dd["pcontact_mean"], edist=dd["edist"][idx].astype(np.float32), edist_index=np.array(idx, np.int64),
                 nll=dd["nll"], contact_bins=np.int64(dd["contact_bins"]), t=np.float64(dd["t"]), rec_residues=residue_labels(rec),
                 lig_residues=residue_labels(lig))
        line.update(distogram_map=os.path.abspath(args.distogram_map))
    if args.distogram_restraints:
        groups = DG.contact_groups(dd["pcontact_mean"], args.restraint_top, upper=args.restraint_upper)
        CS.write_restraints(args.distogram_restraints, groups, rec, lig,
                            header=f"top {len(groups)} predicted contacts (distogram head, bins below {DG.BOUNDS[dd['contact_bins'] - 1]:.2f} A, "
                                   f"mean over {len(dd['nll'])} trajectories at t = {dd['t']:g}): REC LIG UPPER WEIGHT(= contact probability)")
        line.update(distogram_restraints=os.path.abspath(args.distogram_restraints), distogram_restraints_n=len(groups))


def check_sterics(ap, args):
    if args.clash_filter or args.clash_residues:
        args.clash_screen = True
    if not args.clash_screen and (args.clash_cutoff is not None or args.contact_cutoff is not None):
        ap.error("--clash-cutoff / --contact-cutoff are the cutoffs of --clash-screen: they need it")
    args.clash_cutoff = 3.0 if args.clash_cutoff is None else args.clash_cutoff
    args.contact_cutoff = 5.0 if args.contact_cutoff is None else args.contact_cutoff
    if not (np.isfinite(args.clash_cutoff) and np.isfinite(args.contact_cutoff) and 0 < args.clash_cutoff <= args.contact_cutoff):
        ap.error("need 0 < --clash-cutoff <= --contact-cutoff, both finite")


def sterics_kwargs(args, model=None):
    """Driver keyword arguments of the screen flags of dock / refine: none without them."""
    if not args.clash_screen:
        return {}
    return dict(clash_screen=True, clash_filter=args.clash_filter, clash_cutoff=args.clash_cutoff, contact_cutoff=args.contact_cutoff)


def sterics_outputs(args, model, res, rec, lig, line, kw):
    """The screen's part of a dock / refine result: the `sterics` object of the line and --clash-residues."""
    if not args.clash_screen:
        return
    line.update(sterics=res["sterics"], index=res["index"])
    if args.clash_residues:
        from . import driver
        from .sterics import write_clash_residues
        keys, clash, contact = driver.residue_sterics(model, rec, lig, res["rot_update"], res["tr_update"], args.clash_cutoff, args.contact_cutoff)
        write_clash_residues(args.clash_residues, keys, clash, contact)
        line.update(clash_residues=os.path.abspath(args.clash_residues))


def check_interface(ap, args):
    if args.rank == "interface" or args.energy_residues:
        args.interface_energy = True
    if not args.interface_energy and (args.ie_weights is not None or args.ie_cutoff is not None):
        ap.error("--ie-weights / --ie-cutoff describe --interface-energy: they need it")
    args.ie_cutoff = 8.0 if args.ie_cutoff is None else args.ie_cutoff
    if not (np.isfinite(args.ie_cutoff) and 0 < args.ie_cutoff <= 16):
        ap.error("--ie-cutoff must be in (0, 16]")
    if args.ie_weights is not None and not np.isfinite(args.ie_weights).all():
        ap.error("--ie-weights must be finite")


def interface_kwargs(args, model=None):
    """Driver keyword arguments of the interface-energy flags of dock / refine: none without them."""
    if not args.interface_energy:
        return {}
    return dict(interface_energy=True, ie_weights=args.ie_weights, ie_cutoff=args.ie_cutoff, rank=args.rank)


def check_pairpot(ap, args):
    if args.pair_potential is None and (args.rank == "pairpot" or args.pairpot_residues or args.pair_counts):
        ap.error("--rank pairpot / --pairpot-residues / --pair-counts need --pair-potential FILE.npz: no table is shipped")


def pairpot_kwargs(args, model=None):
    """Driver keyword arguments of the pair-potential flags of dock / refine: none without them.  The file is read here, once."""
    if args.pair_potential is None:
        return {}
    from .pairpot import load
    return dict(pair_potential=load(args.pair_potential), rank=args.rank)


def pairpot_outputs(args, model, res, rec, lig, line, kw):
    """The pair-potential part of a dock / refine result: the `pair_potential` object of the line, --pairpot-residues and --pair-counts
    (the kept pose first, then the models in their order)."""
    if args.pair_potential is None:
        return
    line.update(pair_potential=res["pair_potential"], index=res["index"])
    pot = kw["pair_potential"]      # as pairpot_kwargs read it
    if args.pairpot_residues:
        from . import driver
        from .pairpot import write_pairpot_residues
        keys, q = driver.residue_pairpot(model, rec, lig, res["rot_update"], res["tr_update"], pot)
        write_pairpot_residues(args.pairpot_residues, keys, q)
        line.update(pairpot_residues=os.path.abspath(args.pairpot_residues))
    if args.pair_counts:
        from . import driver
        idx = [int(res["index"])] + [int(m["index"]) for m in res.get("models", [])]
        tj = res["pairpot_data"]      # the pair-potential path's own poses: `trajectories` of a restrained run holds no transforms
        cd = driver.ensemble_pairpot(model, rec, lig, np.asarray(tj["rot_update"])[idx], np.asarray(tj["tr_update"])[idx], pot, counts=True)
        with open(args.pair_counts, "wb") as f:
            np.savez(f, counts=cd["counts"], index=np.asarray(idx, np.int64), n_pairs=cd["n_pairs"], energy_q=cd["energy_q"],
                     type_names=np.asarray([str(n) for n in pot["type_names"]]), edges=np.asarray(pot["edges"], np.float32))
        line.update(pair_counts=os.path.abspath(args.pair_counts))


def _density_flags(p):
    """Nothing: the density flags are density_parser's, which parse_args reads first (the commands' own option lists stay what they were)."""


def check_density(ap, args):
    if getattr(args, "density", None) is None:
        given = [o for o, d in (("--density-resolution", "density_resolution"), ("--density-threshold", "density_threshold"), ("--min-density-cc", "min_density_cc"),
                                ("--density-residues", "density_residues"), ("--write-simulated-map", "write_simulated_map")) if getattr(args, d, None) is not None]
        if given or getattr(args, "rank", None) == "density":
            ap.error(f"{', '.join(given + (['--rank density'] if args.rank == 'density' else []))} need(s) --density MAP.mrc")
        return
    if args.density_resolution is None or not (np.isfinite(args.density_resolution) and args.density_resolution > 0):
        ap.error("--density needs --density-resolution R, finite and > 0 (A)")
    if not os.path.isfile(args.density):
        ap.error(f"{args.density}: no such file")
    args.density_threshold = 1.0 if args.density_threshold is None else args.density_threshold
    if not np.isfinite(args.density_threshold):
        ap.error("--density-threshold must be finite")
    if args.min_density_cc is not None and (not np.isfinite(args.min_density_cc) or getattr(args, "top_k", None) is None):
        ap.error("--min-density-cc must be finite and filters the models of --top-k: it needs it")


def density_kwargs(args, model=None):
    """Driver keyword arguments of the density flags: none without --density.  The map is read here, once."""
    if getattr(args, "density", None) is None:
        return {}
    from .density import read_mrc
    kw = dict(density_map=read_mrc(args.density), density_resolution=args.density_resolution, density_threshold=args.density_threshold, rank=args.rank)
    if args.min_density_cc is not None:
        kw["min_density_cc"] = args.min_density_cc
    return kw


def density_outputs(args, model, res, rec, lig, line, kw):
    """The density part of a result: the `density` object of the line, --density-residues (the kept pose and the models) and
    --write-simulated-map (the kept model on the map's grid)."""
    if getattr(args, "density", None) is None:
        return
    line.update(density=res["density"], index=res["index"])
    if "density_dropped" in res:
        line.update(density_dropped=res["density_dropped"])
    dmap = kw["density_map"]      # as density_kwargs read it
    if args.density_residues:
        from . import driver
        from .density import write_density_residues
        idx = [int(res["index"])] + [int(m["index"]) for m in res.get("models", [])]
        tj = res["density_data"]      # the density path's own poses
        keys, mean = driver.residue_density(model, rec, lig, np.asarray(tj["rot_update"])[idx], np.asarray(tj["tr_update"])[idx], dmap,
                                            args.density_resolution, args.density_threshold)
        write_density_residues(args.density_residues, keys, mean)
        line.update(density_residues=os.path.abspath(args.density_residues))
    if args.write_simulated_map:
        from . import density as DN
        from . import driver
        from . import sterics as ST
        ra, rw, _, lw, _ = driver.density_inputs(rec, lig, model.hp.family)
        posed = np.asarray(res["lig_aa_coords"], np.float64)[ST.heavy_atoms(lig["atoms"])]
        sim = DN.simulate_map(np.concatenate([ra.astype(np.float64), posed]), np.concatenate([rw, lw]), res["density"]["sigma"],
                              np.shape(dmap["grid"]), dmap["origin"], dmap["voxel"])
        DN.write_mrc(args.write_simulated_map, sim.astype(np.float32), dmap["origin"], dmap["voxel"])
        line.update(simulated_map=os.path.abspath(args.write_simulated_map))


def interface_outputs(args, model, res, rec, lig, line, kw):
    """The interface-energy part of a dock / refine result: the `interface_energy` object of the line and --energy-residues."""
    if not args.interface_energy:
        return
    line.update(interface_energy=res["interface_energy"], index=res["index"])
    if args.energy_residues:
        from . import driver
        from .ifenergy import write_energy_residues
        keys, vdw, elec = driver.residue_interface_energy(model, rec, lig, res["rot_update"], res["tr_update"], args.ie_cutoff)
        write_energy_residues(args.energy_residues, keys, vdw, elec)
        line.update(energy_residues=os.path.abspath(args.energy_residues))


def check_affinity(ap, args):
    if args.contact_residues:
        args.affinity = True
    if not args.affinity and args.affinity_cutoff is not None:
        ap.error("--affinity-cutoff is the cutoff of --affinity: it needs it")
    args.affinity_cutoff = 5.5 if args.affinity_cutoff is None else args.affinity_cutoff
    if not (np.isfinite(args.affinity_cutoff) and 0 < args.affinity_cutoff <= 16):
        ap.error("--affinity-cutoff must be in (0, 16]")


def affinity_kwargs(args, model=None):
    """Driver keyword arguments of the affinity flags of dock / refine: none without them."""
    if not args.affinity:
        return {}
    return dict(affinity=True, affinity_cutoff=args.affinity_cutoff)


def affinity_outputs(args, model, res, rec, lig, line, kw):
    """The affinity part of a dock / refine result: the `affinity` object of the line and --contact-residues."""
    if not args.affinity:
        return
    line.update(affinity=res["affinity"], index=res["index"])
    if "affinity_data" in res and sum(res["affinity_data"]["unclassified"]):      # residue names outside the 20: counted as apolar
        line.update(affinity_unclassified=[int(v) for v in res["affinity_data"]["unclassified"]])
    if args.contact_residues:
        from . import driver
        from .affinity import pairs_of, write_contact_residues
        cd = driver.ensemble_contacts(model, rec, lig, res["rot_update"], res["tr_update"], args.affinity_cutoff, bits=True)
        write_contact_residues(args.contact_residues, cd["rec_keys"], cd["lig_keys"], pairs_of(cd["contact_bits"][0]))
        line.update(contact_residues=os.path.abspath(args.contact_residues))


def check_hbonds(ap, args):
    if args.hbond_residues:
        args.hbonds = True
    if not args.hbonds and (args.hbond_cutoff is not None or args.hbond_angle is not None or args.salt_cutoff is not None):
        ap.error("--hbond-cutoff / --hbond-angle / --salt-cutoff describe --hbonds: they need it")
    args.hbond_cutoff = 3.5 if args.hbond_cutoff is None else args.hbond_cutoff
    args.hbond_angle = 90.0 if args.hbond_angle is None else args.hbond_angle
    args.salt_cutoff = 4.0 if args.salt_cutoff is None else args.salt_cutoff
    if not (np.isfinite(args.hbond_cutoff) and 0 < args.hbond_cutoff <= 8 and np.isfinite(args.salt_cutoff) and 0 < args.salt_cutoff <= 8):
        ap.error("--hbond-cutoff and --salt-cutoff must be in (0, 8]")
    if not (90.0 <= args.hbond_angle < 180.0):
        ap.error("--hbond-angle must be in [90, 180)")


def hbonds_kwargs(args, model=None):
    """Driver keyword arguments of the hydrogen-bond flags of dock / refine: none without them."""
    if not args.hbonds:
        return {}
    return dict(hbonds=True, hbond_cutoff=args.hbond_cutoff, hbond_angle=args.hbond_angle, salt_cutoff=args.salt_cutoff)


def hbonds_outputs(args, model, res, rec, lig, line, kw):
    """The hydrogen-bond part of a dock / refine result: the counts of the line (the models carry theirs already), one note on stderr
    when polar atoms could not be typed, and --hbond-residues."""
    if not args.hbonds:
        return
    line.update({k: res[k] for k in ("n_hbond", "hb_bb_bb", "hb_bb_sc", "hb_sc_sc", "n_salt", "n_unsat") if k in res}, index=res["index"])
    untyped = res["hbond_data"]["untyped"] if "hbond_data" in res else (0, 0)
    if sum(untyped):
        line.update(hbond_untyped=[int(v) for v in untyped])
        print(f"hbonds: {untyped[0]} receptor and {untyped[1]} ligand polar atoms have no antecedent in the file and take no part",
              file=sys.stderr, flush=True)
    if args.hbond_residues:
        from . import driver
        from .hbonds import write_hbond_residues

        def write(path, rot, tr):
            keys, hb, sb = driver.residue_hbonds(model, rec, lig, rot, tr, args.hbond_cutoff, args.hbond_angle, args.salt_cutoff)
            write_hbond_residues(path, keys[0], hb[0], sb[0], keys[1], hb[1], sb[1])
        write(args.hbond_residues, res["rot_update"], res["tr_update"])
        line.update(hbond_residues=os.path.abspath(args.hbond_residues))
        stem, ext = os.path.splitext(args.hbond_residues)
        for m in res.get("models", ()):      # every --top-k model: <stem>_<rank><ext>
            t = res["hbond_data"]
            write(f"{stem}_{m['rank']}{ext}", t["rot_update"][m["index"]], t["tr_update"][m["index"]])


def check_surface(ap, args):
    if args.min_bsa is not None or args.interface_residues:
        args.bsa = True
    if not args.bsa and (args.probe is not None or args.sphere_points is not None):
        ap.error("--probe / --sphere-points describe the surface of --bsa: they need it")
    args.probe = 1.4 if args.probe is None else args.probe
    args.sphere_points = 128 if args.sphere_points is None else args.sphere_points
    if not (np.isfinite(args.probe) and args.probe > 0):
        ap.error("--probe must be finite and > 0")
    if args.sphere_points < 64 or args.sphere_points > 256 or args.sphere_points % 64:
        ap.error("--sphere-points must be a multiple of 64 in 64 .. 256")
    if args.min_bsa is not None and not np.isfinite(args.min_bsa):
        ap.error("--min-bsa must be finite")


def surface_kwargs(args, model=None):
    """Driver keyword arguments of the surface flags of dock / refine: none without them."""
    if not args.bsa:
        return {}
    return dict(bsa=True, min_bsa=args.min_bsa, probe=args.probe, sphere_points=args.sphere_points)


def surface_outputs(args, model, res, rec, lig, line, kw):
    """The surface part of a dock / refine result: the areas of the line and --interface-residues."""
    if not args.bsa:
        return
    line.update(bsa=res["bsa"], bsa_rec=res["bsa_rec"], bsa_lig=res["bsa_lig"], probe=res["probe"], sphere_points=res["sphere_points"],
                index=res["index"])
    if args.min_bsa is not None:
        line.update(min_bsa=args.min_bsa)
        if "bsa_dropped" in res:
            line.update(bsa_dropped=res["bsa_dropped"])
    if args.interface_residues:
        from . import driver
        from .surface import write_interface_residues
        keys, area = driver.residue_surface(model, rec, lig, res["rot_update"], res["tr_update"], args.probe, args.sphere_points)
        write_interface_residues(args.interface_residues, keys, area)
        line.update(interface_residues=os.path.abspath(args.interface_residues))


def consensus_table(rows):
    """Per complex the trajectory consensus ranking keeps (highest consensus, ties: lower energy, lower index; no contact anywhere: the
    minimum energy) with its DockQ, and the success rates of that choice at the CAPRI thresholds."""
    from . import consensus as CS
    by = {}
    for r in rows:
        by.setdefault(r["id"], []).append(r)
    per = {}
    for cid, rs in sorted(by.items()):
        rs = sorted(rs, key=lambda r: int(r["index"]))
        k = CS.pick([float(r["consensus"]) for r in rs], [float(r["energy"]) for r in rs])
        top = rs[k] if k is not None else min(rs, key=lambda r: (r["energy"], int(r["index"])))
        per[cid] = {"index": int(top["index"]), "consensus": float(top["consensus"]), "n_contacts": int(top["n_contacts"]),
                    "DockQ": float(top["DockQ"]), "energy": float(top["energy"]), "fallback": k is None}
    n = max(len(per), 1)
    return per, {name: {"threshold": thr, "consensus_top1": sum(p["DockQ"] >= thr for p in per.values()) / n} for name, thr in DOCKQ_THRESHOLDS}


def format_consensus_table(per, table, energy_table):
    lines = [f"consensus-selected trajectory ({sum(p['fallback'] for p in per.values())} of {len(per)} complexes without any contact: energy pick):"]
    for cid, p in per.items():
        lines.append(f"{cid:8s} index {p['index']:4d} consensus {p['consensus']:8.4f} contacts {p['n_contacts']:5d} DockQ {p['DockQ']:8.4f}")
    for name, t in table.items():
        lines.append(f"  {name:10s} DockQ >= {t['threshold']:.2f}: consensus pick {100 * t['consensus_top1']:5.1f} % | energy pick "
                     f"{100 * energy_table[name]['top1']:5.1f} %")
    return "\n".join(lines)


def success_table(rows, top_k=None):
    """Per complex: DockQ of the minimum-energy trajectory (what inference() keeps) and the best DockQ among its trajectories;
    success rates at the CAPRI thresholds.  `top_k` (rows with cluster columns): also the best DockQ among the centres of the first
    top_k clusters and the `top{K}` success rate."""
    by = {}
    for r in rows:
        by.setdefault(r["id"], []).append(r)
    per = {}
    for cid, rs in sorted(by.items()):
        top = min(rs, key=lambda r: (r["energy"], int(r["index"])))
        per[cid] = {"n": len(rs), "top1_DockQ": float(top["DockQ"]), "top1_energy": float(top["energy"]),
                    "best_DockQ": float(max(r["DockQ"] for r in rs)), "mean_DockQ": float(np.mean([r["DockQ"] for r in rs]))}
        if top_k is not None:
            cen = [float(r["DockQ"]) for r in rs if int(r["is_center"]) and 0 <= int(r["cluster"]) < top_k]
            per[cid][f"top{top_k}_DockQ"] = max(cen) if cen else float("nan")
            per[cid]["clusters"] = len(cen)
    n = max(len(per), 1)
    table = {name: {"threshold": thr, "top1": sum(p["top1_DockQ"] >= thr for p in per.values()) / n,
                    "best_of_n": sum(p["best_DockQ"] >= thr for p in per.values()) / n} for name, thr in DOCKQ_THRESHOLDS}
    if top_k is not None:
        for name, thr in DOCKQ_THRESHOLDS:
            table[name][f"top{top_k}"] = sum(p[f"top{top_k}_DockQ"] >= thr for p in per.values()) / n
    return per, table


def restraint_summary(rows, restraints_by_id):
    """Per complex: the number of restraint groups, the trajectories satisfying all of them, and the mean number satisfied."""
    out = {}
    for cid, groups in sorted(restraints_by_id.items()):
        rs = [r for r in rows if r["id"] == cid]
        if not rs:
            continue
        sat = [int(r["restraints_satisfied"]) for r in rs]
        out[cid] = {"groups": len(groups), "all_satisfied": sum(s == len(groups) for s in sat), "n": len(rs),
                    "mean_satisfied": float(np.mean(sat))}
    return out


def format_table(per, table, top_k=None):
    if top_k is not None:
        return _format_table_clustered(per, table, top_k)
    lines = [f"{'id':8s} {'n':>4s} {'top1 DockQ':>11s} {'best DockQ':>11s} {'top1 energy':>12s}"]
    for cid, p in per.items():
        lines.append(f"{cid:8s} {p['n']:4d} {p['top1_DockQ']:11.4f} {p['best_DockQ']:11.4f} {p['top1_energy']:12.4f}")
    lines.append(f"success rate over {len(per)} complexes (DockQ of the minimum-energy trajectory | best of the trajectories):")
    for name, t in table.items():
        lines.append(f"  {name:10s} DockQ >= {t['threshold']:.2f}: {100 * t['top1']:5.1f} % | {100 * t['best_of_n']:5.1f} %")
    return "\n".join(lines)


def _format_table_clustered(per, table, top_k):
    tk = f"top{top_k}"
    lines = [f"{'id':8s} {'n':>4s} {'top1 DockQ':>11s} {tk + ' DockQ':>11s} {'best DockQ':>11s} {'top1 energy':>12s}"]
    for cid, p in per.items():
        lines.append(f"{cid:8s} {p['n']:4d} {p['top1_DockQ']:11.4f} {p[tk + '_DockQ']:11.4f} {p['best_DockQ']:11.4f} {p['top1_energy']:12.4f}")
    lines.append(f"success rate over {len(per)} complexes (DockQ of the minimum-energy trajectory | best of the first {top_k} cluster "
                 "centres | best of the trajectories):")
    for name, t in table.items():
        lines.append(f"  {name:10s} DockQ >= {t['threshold']:.2f}: {100 * t['top1']:5.1f} % | {100 * t[tk]:5.1f} % | "
                     f"{100 * t['best_of_n']:5.1f} %")
    return "\n".join(lines)


class _Flags(NamedTuple):
    """The command-line side of one per-pose analysis of dock / refine."""
    add: Callable          # (subparser): its flags
    check: Callable        # (ap, args): what its flags imply, their defaults and their errors
    kwargs: Callable       # (args, model) -> its driver keyword arguments: none without its flags
    outputs: Callable      # (args, model, res, rec, lig, line, kw): its entries of the result line and its files


# in the order of the flags in --help and of the entries in the result line
ANALYSES = (
    _Flags(_add_consensus, check_consensus, consensus_kwargs, consensus_outputs),
    _Flags(_add_distogram, check_distogram, distogram_kwargs, distogram_outputs),
    _Flags(_add_sterics, check_sterics, sterics_kwargs, sterics_outputs),
    _Flags(_add_surface, check_surface, surface_kwargs, surface_outputs),
    _Flags(_add_interface, check_interface, interface_kwargs, interface_outputs),
    _Flags(_add_pairpot, check_pairpot, pairpot_kwargs, pairpot_outputs),
    _Flags(_density_flags, check_density, density_kwargs, density_outputs),
    _Flags(_add_affinity, check_affinity, affinity_kwargs, affinity_outputs),
    _Flags(_add_hbonds, check_hbonds, hbonds_kwargs, hbonds_outputs),
)


def _pair_kwargs(args, model, kw, models):
    """What dock, refine and rescore give their driver alike, added to kw: the model / refinement options (`models`: the command has
    them), --native and the keywords of every analysis."""
    if models and args.top_k is not None:
        kw.update(top_k=args.top_k, cluster_radius=args.cluster_radius, cluster_rule=args.cluster_rule)
    if models and args.refine_t is not None:
        kw.update(refine_t=args.refine_t, refine_samples=args.refine_samples)
    if args.native:
        kw.update(native=load_native(args.native))
    for a in ANALYSES:
        kw.update(a.kwargs(args, model))
    return kw


def _pose_entries(res):
    """The kept pose's entries of a result line."""
    return dict(rot_update=[float(v) for v in res["rot_update"]], tr_update=[float(v) for v in res["tr_update"]],
                selfcheck_ok=None if res["selfcheck"] is None else bool(res["selfcheck"]["ok"]))


def _finish_line(args, model, res, rec, lig, line, kw, models, native_extra=()):
    """The tail of a result line - models, refinement, --native metrics (and the command's own `native_extra` entries of res), every
    analysis' entries and files - and the line itself on stdout."""
    from . import driver
    if models and args.top_k is not None:
        line.update(models=[dict(m, path=os.path.abspath(driver.model_path(args.out, m["rank"]))) for m in res["models"]],
                    cluster_radius=args.cluster_radius, cluster_rule=args.cluster_rule)
    if models and args.refine_t is not None:
        line.update(refine_t=args.refine_t, refine_samples=args.refine_samples)
    if args.native:
        line.update(metrics=res["metrics"], **{k: res[k] for k in native_extra})
    for a in ANALYSES:
        a.outputs(args, model, res, rec, lig, line, kw)
    print(json.dumps(line), flush=True)


def cmd_pair(args):
    """dock and refine: one body; they differ in their own driver keywords, their own entries of the line and what --json adds."""
    from . import driver
    dock = args.cmd == "dock"
    sym_kw = symmetry_kwargs(args)      # (checked before the checkpoint is read)
    model, _ = load_model(args)
    rec, lig, rec_x, lig_x = load_pair(args.pdb_1, args.pdb_2, args.features, model.hp.lm_embed_dim)
    kw = {} if dock else dict(t_begin=args.t_begin, perturb=not args.no_perturb)
    kw.update(sym_kw)
    if args.restraints:
        from .restraints import read_restraints
        kw.update(restraints=read_restraints(args.restraints, rec, lig), **({"restraint_rank": args.restraint_rank} if dock else {}))
    _pair_kwargs(args, model, kw, models=dock)
    try:
        res = (driver.dock_pair if dock else driver.refine_pair)(
            model, rec, lig, rec_x, lig_x, num_samples=args.num_samples, num_steps=args.num_steps, seed=args.seed, precision=args.precision,
            out_pdb=args.out, max_batch=args.max_batch, selfcheck=not args.no_selfcheck, on_selfcheck_fail=args.on_selfcheck_fail, **kw)
    except ValueError as e:
        if sym_kw and str(e).startswith("symmetry"):      # the inputs are no homo-oligomer: the cause, not a traceback
            raise SystemExit(str(e)) from None
        raise
    line = {"energy": res["energy"], "output": os.path.abspath(args.out), "num_samples": args.num_samples, "precision": res["precision"]}
    if not dock:
        line.update(t_begin=res["t_begin"], perturb=not args.no_perturb, index=res["index"])
    line.update(_pose_entries(res))
    if dock and args.restraints:
        line.update(restraints=res["restraints"], restraints_satisfied=res["restraints_satisfied"],
                    restraint_energy=res["restraint_energy"], restraint_rank=res["restraint_rank"], index=res["index"])
    if sym_kw:
        line.update(symmetry=res["symmetry"], index=res["index"])
    _finish_line(args, model, res, rec, lig, line, kw, models=dock, native_extra=() if dock else ("start_metrics",))
    if args.json:
        if dock:
            extra = {"trajectories": {k: [float(x) for x in v] for k, v in res["trajectories"].items()}} if args.restraints else {}
        else:
            extra = {"energies": [float(e) for e in res["trajectories"]["energy"]]}
        if sym_kw:      # every trajectory's m, theta, screw, sym_rmsd, closure
            extra["symmetry_data"] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in res["symmetry_data"].items()}
        with open(args.json, "w") as f:
            json.dump(dict(line, selfcheck=res["selfcheck"], **extra), f, default=float)
    return 0


def load_decoys(args, rec, lig):
    """The decoys of `rescore` -> (decoys of driver.rescore_pair, [(source, model number)] per decoy)."""
    from . import pdbio
    if args.poses:
        f = np.load(args.poses, allow_pickle=False)
        for k in ("rot_update", "tr_update"):
            if k not in f:
                raise ValueError(f"{args.poses}: need rot_update [P,3] and tr_update [P,3]")
        dec = {"rot_update": np.asarray(f["rot_update"], np.float32), "tr_update": np.asarray(f["tr_update"], np.float32)}
        return dec, [(args.poses, i + 1) for i in range(dec["rot_update"].reshape(-1, 3).shape[0])]
    L, R = len(lig["bb_coords"]), len(rec["bb_coords"])
    if args.coords:
        f = np.load(args.coords, allow_pickle=False)
        if "lig_pos" not in f:
            raise ValueError(f"{args.coords}: need lig_pos [P,{L},3,3] (and optionally rec_pos [P,{R},3,3])")
        lp = np.asarray(f["lig_pos"], np.float32)
        if lp.size == 0 or lp.size % (L * 9):
            raise ValueError(f"{args.coords}: lig_pos is {lp.shape}, the ligand PDB has {L} residues with N, CA and C")
        dec = {"lig_pos": lp.reshape(-1, L, 3, 3)}
        if "rec_pos" in f:
            rp = np.asarray(f["rec_pos"], np.float32)
            if rp.size != dec["lig_pos"].shape[0] * R * 9:
                raise ValueError(f"{args.coords}: rec_pos is {rp.shape}, expected ({dec['lig_pos'].shape[0]}, {R}, 3, 3)")
            dec["rec_pos"] = rp.reshape(-1, R, 3, 3)
        return dec, [(args.coords, i + 1) for i in range(dec["lig_pos"].shape[0])]
    chains = args.decoy_chains or (None, None)
    ligs, recs, names = [], [], []
    for path in args.decoys:
        models = pdbio.read_models(path)
        if not models:
            raise ValueError(f"{path}: no ATOM records")
        for i, atoms in enumerate(models):
            lb, rb = pdbio.match_model(atoms, rec, lig, chains[0], chains[1], source=path, model=i + 1)
            ligs.append(lb)
            recs.append(rb)
            names.append((path, i + 1))
    dec = {"lig_pos": np.asarray(ligs, np.float32)}
    if any(r is not None for r in recs):      # a model without a receptor is in the input's frame: it travels with the input's receptor
        dec["rec_pos"] = np.asarray([rec["bb_coords"] if r is None else r for r in recs], np.float32)
    return dec, names


def write_scores(path, names, res):
    """--scores: one row per decoy, in input order; rank: its place by the key the run clustered by (1 = best), empty when rejected."""
    from .cluster import rank_order
    fd, energy = res["fit_data"], res["trajectories"]["energy"]
    key = np.asarray(res["key"], np.float64)
    rank = np.empty(len(names), np.int64)
    rank[rank_order(key, len(names))] = np.arange(1, len(names) + 1)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["source", "model", "fit_rmsd", "rec_rmsd", "rejected", "energy", "rank"])
        for i, (src, m) in enumerate(names):
            rej = bool(fd["rejected"][i])
            w.writerow([src, m, repr(float(fd["rmsd"][i])), "" if fd["rec_rmsd"] is None else repr(float(fd["rec_rmsd"][i])), int(rej),
                        "" if rej else repr(float(energy[i])), "" if rej or np.isnan(key[i]) else int(rank[i])])


def cmd_rescore(args):
    """rescore: cmd_pair's line for decoys that were made elsewhere, plus `fit` and `num_decoys`.  What is wrong with the decoys - a
    file that does not match the pair, an array of the wrong shape, no rigid image among them - is one line on stderr and status 1."""
    from . import driver
    model, _ = load_model(args)
    rec, lig, rec_x, lig_x = load_pair(args.pdb_1, args.pdb_2, args.features, model.hp.lm_embed_dim)
    try:
        decoys, names = load_decoys(args, rec, lig)
    except ValueError as e:
        print(f"rescore: {e}", file=sys.stderr)
        return 1
    kw = _pair_kwargs(args, model, {} if args.score_t is None else dict(t=args.score_t), models=True)
    try:
        res = driver.rescore_pair(model, rec, lig, rec_x, lig_x, decoys, fit_tolerance=args.fit_tolerance, num_steps=args.num_steps,
                                  seed=args.seed, precision=args.precision, out_pdb=args.out, max_batch=args.max_batch,
                                  selfcheck=not args.no_selfcheck, on_selfcheck_fail=args.on_selfcheck_fail, **kw)
    except driver.AllRejected as e:
        print(f"rescore: {e}", file=sys.stderr)
        return 1
    k = res["index"]
    line = {"energy": res["energy"], "output": os.path.abspath(args.out), "num_decoys": len(names), "precision": res["precision"],
            "t": res["t"], "index": k, "source": names[k][0], "model": names[k][1], "fit": res["fit"]}
    line.update(_pose_entries(res))
    _finish_line(args, model, res, rec, lig, line, kw, models=True)
    if args.scores:
        write_scores(args.scores, names, res)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(line, selfcheck=res["selfcheck"], energies=[float(e) for e in res["trajectories"]["energy"]]), f, default=float)
    return 0


def db5_ids(root, limit=None):
    lst = os.path.join(root, "test.txt")
    if os.path.exists(lst):
        ids = [l.strip() for l in open(lst) if l.strip()]
    else:
        ids = sorted(f[:-3] for f in os.listdir(root) if f.endswith(".pt"))
    present = [i for i in ids if os.path.exists(os.path.join(root, i + ".pt"))]
    for i in ids:
        if i not in present:
            print(f"sweep: {i}.pt is listed but missing - skipped", file=sys.stderr)
    return present[:limit] if limit else present


def cmd_sweep(args):
    from . import distributed as D
    from . import driver
    from .db5 import load_db5_pt
    model, _ = load_model(args)
    rank, local_rank, world = D.dist_env()
    grp = D.init(device_index=args.device if args.device is not None else local_rank) if world > 1 else None
    cxs = []
    for cid in db5_ids(args.db5, args.limit):
        c = load_db5_pt(os.path.join(args.db5, cid + ".pt"))
        c["id"] = c.get("id") or cid
        cxs.append(c)
    if not cxs:
        raise SystemExit(f"sweep: no <id>.pt under {args.db5}")
    checks = []
    rkw = {}
    if args.native_restraints is not None:
        from .restraints import native_contact_groups
        rkw["restraints_by_id"] = {c["id"]: native_contact_groups(c["rec_pos"], c["lig_pos"], args.native_restraints,
                                                                  cutoff=args.restraint_cutoff, seed=args.seed) for c in cxs}
    top_k = None
    if args.cluster_radius is not None:
        top_k = args.top_k
        rkw.update(cluster_radius=args.cluster_radius, cluster_rule=args.cluster_rule, top_k=top_k)
    steps = []
    if args.metrics != "host":
        rkw.update(metrics=args.metrics)
    if args.step_metrics is not None:
        rkw.update(step_csv=args.step_metrics, steps_out=steps)
    if args.consensus:
        rkw.update(consensus=True, consensus_top=args.consensus_top)
    rows, _ = driver.run_set(model, cxs, num_samples=args.num_samples, num_steps=args.num_steps, seed=args.seed,
                             precision=args.precision, global_rotation=not args.no_global_rotation, out_csv=args.out_csv,
                             traj_dir=args.traj_dir, max_batch=args.max_batch, selfcheck=not args.no_selfcheck,
                             on_selfcheck_fail=args.on_selfcheck_fail, checks_out=checks, **rkw)
    all_rows = driver._gather_rows(rows, world)
    all_steps = driver._gather_rows(steps, world) if args.step_metrics is not None else []
    all_checks = [c for part in D.gather_objects(checks) for c in part] if world > 1 else checks
    if rank == 0:
        per, table = success_table(all_rows, top_k)
        print(format_table(per, table, top_k), flush=True)
        extra = {}
        if "restraints_by_id" in rkw:
            extra["restraints"] = restraint_summary(all_rows, rkw["restraints_by_id"])
            print(json.dumps({"restraints": extra["restraints"]}), flush=True)
        if args.step_metrics is not None:
            extra["step_metrics"] = step_summary(all_steps, all_rows)
            extra["step_csv"] = os.path.abspath(args.step_metrics)
        if args.consensus:
            cper, ctable = consensus_table(all_rows)
            print(format_consensus_table(cper, ctable, table), flush=True)
            extra["consensus"] = {"complexes": cper, "success": ctable, "members_fraction": args.consensus_top}
        if args.summary:
            with open(args.summary, "w") as f:
                json.dump({"csv": os.path.abspath(args.out_csv), "complexes": per, "success": table, "selfcheck": all_checks,
                           "world": world, "backend": grp.backend if grp else "single", **extra}, f, default=float, indent=1)
    if world > 1:
        D.shutdown()
    return 0


def cmd_selfcheck(args):
    from . import engine
    model, _ = load_model(args)
    rec, lig, rec_x, lig_x = load_pair(args.pdb_1, args.pdb_2, args.features, model.hp.lm_embed_dim)
    gx = engine.Complex(model, rec_x, lig_x, rec["bb_coords"], lig["bb_coords"])
    prec = args.precision if engine.canonical_precision(args.precision) != "fp32" else "mfma16"
    r = gx.selfcheck(n_eval=args.n_eval, seed=args.seed, precision=prec)
    print(engine.format_selfcheck(r, os.path.basename(args.pdb_1) + "+" + os.path.basename(args.pdb_2)), file=sys.stderr)
    print(json.dumps(r, default=float), flush=True)
    return 0 if r["ok"] else 1


def main(argv=None):
    args = parse_args(argv)
    return {"dock": cmd_pair, "sweep": cmd_sweep, "selfcheck": cmd_selfcheck, "refine": cmd_pair, "rescore": cmd_rescore}[args.cmd](args)
