"""ctypes binding of the C ABI declared in include/dfmdock_amd.h.

The shared library is the product: if it is missing this module raises - there
is no Python / CPU fallback for the hot path.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DFM_LIB") or os.path.join(_HERE, "libdfmdock_amd.so")   # DFM_LIB: A/B builds of the same engine

F32P = C.POINTER(C.c_float)
I32P = C.POINTER(C.c_int32)
U32P = C.POINTER(C.c_uint32)

DFM_F_MFMA16 = 1 << 0
DFM_F_BF16 = DFM_F_MFMA16      # name of rounds 1-2
DFM_F_ENERGY = 1 << 1
DFM_F_NOISE_ANNEALING = 1 << 2
DFM_F_CLASH_FORCE = 1 << 3
DFM_F_ODE = 1 << 4
DFM_F_PROFILE = 1 << 5
DFM_F_STEP_ENERGY = 1 << 6
DFM_F_F16 = 1 << 7
DFM_F_IRES = 1 << 8
DFM_F_BF16_OPS = 1 << 9
DFM_F_DIST = 1 << 10
DFM_F_L0_TABLE = 1 << 11       # dfm_score: layer 0 through the per-complex message table
DFM_F_NO_L0_TABLE = 1 << 12    # dfm_sample: layer 0 evaluated directly
DFM_F_GRAPH = 1 << 13          # dfm_sample: replay one captured step as a hipGraph (opt-in)
DFM_F_RESTRAINTS = 1 << 14     # dfm_sample: the interface restraint step (dfm_complex_set_restraints)
DFM_F_SYMMETRY = 1 << 15       # dfm_sample / dfm_refine: the Cn symmetry step (dfm_complex_set_symmetry)

DFM_CLUSTER_ENERGY = 0         # dfm_pose_cluster rules
DFM_CLUSTER_SIZE = 1

EXPORTS = [
    "dfm_last_error", "dfm_config_string", "dfm_device_count", "dfm_set_device", "dfm_default_hparams", "dfm_param_count",
    "dfm_model_create", "dfm_model_destroy", "dfm_complex_create", "dfm_complex_destroy", "dfm_complex_degree",
    "dfm_complex_set_pose", "dfm_complex_set_homomer",
    "dfm_score", "dfm_sample", "dfm_get_profile", "dfm_diffusion_coef", "dfm_complex_selfcheck", "dfm_trim_cache", "dfm_alloc_diag",
    "dfm_complex_set_restraints", "dfm_restraint_eval", "dfm_complex_set_symmetry", "dfm_symmetry_eval", "dfm_pose_rmsd", "dfm_pose_cluster", "dfm_pose_last_timing",
    "dfm_refine", "dfm_forward_marginal", "dfm_igso3_table",
    "dfm_native_create", "dfm_native_destroy", "dfm_native_info", "dfm_pose_metrics", "dfm_metrics_last_timing",
    "dfm_pose_consensus", "dfm_consensus_chunk_poses", "dfm_consensus_last_timing",
    "dfm_atoms_create", "dfm_atoms_destroy", "dfm_atoms_info", "dfm_pose_sterics", "dfm_pose_sterics_chunked", "dfm_sterics_last_timing",
    "dfm_sterics_exit_counts",
    "dfm_surface_create", "dfm_surface_destroy", "dfm_surface_info", "dfm_pose_bsa", "dfm_pose_bsa_chunked", "dfm_bsa_last_timing",
    "dfm_iface_create", "dfm_iface_destroy", "dfm_iface_info", "dfm_pose_iface_energy", "dfm_pose_iface_energy_chunked",
    "dfm_iface_last_timing",
    "dfm_rescon_create", "dfm_rescon_destroy", "dfm_rescon_info", "dfm_pose_rescon", "dfm_pose_rescon_chunked", "dfm_rescon_last_timing",
    "dfm_rescon_last_phases",
    "dfm_hbond_create", "dfm_hbond_destroy", "dfm_hbond_info", "dfm_pose_hbonds", "dfm_pose_hbonds_chunked", "dfm_hbond_last_timing",
    "dfm_hbond_last_phases",
    "dfm_pairpot_create", "dfm_pairpot_destroy", "dfm_pairpot_info", "dfm_pose_pairpot", "dfm_pose_pairpot_chunked",
    "dfm_pairpot_last_timing", "dfm_pairpot_last_phases",
    "dfm_score_distogram", "dfm_distogram_last_timing",
    "dfm_pose_fit", "dfm_pose_fit_chunked", "dfm_fit_last_timing",
    "dfm_density_create", "dfm_density_destroy", "dfm_density_info", "dfm_pose_density", "dfm_pose_density_chunked", "dfm_density_last_timing",
]


class HParamsC(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("lm_embed_dim", "positional_embed_dim", "spatial_embed_dim", "node_dim",
                                       "edge_dim", "inner_dim", "depth", "knn", "n_sample")] + \
               [("cut_off", C.c_float), ("mask_dist", C.c_float)] + \
               [(n, C.c_double) for n in ("r3_min_sigma", "r3_max_sigma", "so3_min_sigma", "so3_max_sigma")] + \
               [("family", C.c_int), ("agg_mean", C.c_int)]


class ScoreOutC(C.Structure):
    _fields_ = [("tr_score", F32P), ("rot_score", F32P), ("energy", F32P), ("num_clashes", I32P), ("f", F32P),
                ("h_last", F32P), ("h_first", F32P), ("edges", I32P), ("edge_codes", U32P), ("confidence", F32P),
                ("ires", F32P), ("dist_logits", F32P)]


class InjectC(C.Structure):
    _fields_ = [("R0", F32P), ("tr_draw", F32P), ("z_rot", F32P), ("z_tr", F32P), ("edges", I32P)]


class TrajOutC(C.Structure):
    _fields_ = [("lig_pos", F32P), ("rot_update", F32P), ("tr_update", F32P), ("energy", F32P),
                ("num_clashes", I32P), ("final_scores", F32P), ("trace_pose", F32P), ("trace_scores", F32P),
                ("init_pose", F32P)]


class RefineParamsC(C.Structure):
    _fields_ = [("t_begin", C.c_float), ("perturb", C.c_int), ("start_pos", F32P)]


class RefineInjectC(C.Structure):
    _fields_ = [("u_angle", F32P), ("axis_draw", F32P), ("tr_draw", F32P)]


class ProfileC(C.Structure):
    _fields_ = [("edge_kernel_ms", C.c_double), ("edge_kernel_launches", C.c_int64), ("edge_rows", C.c_int64),
                ("total_ms", C.c_double), ("phase_cycles", C.c_double * 4), ("slot_cycles", C.c_double * 16),
                ("l0_evals", C.c_int64), ("l0_edges", C.c_int64), ("l0_miss_rows", C.c_int64),
                ("l0_rows_ms", C.c_double), ("l0_gather_ms", C.c_double), ("l0_build_ms", C.c_double),
                ("edge_lig_launches", C.c_int64), ("edge_lig_ms", C.c_double),
                ("edge_shader_cycles", C.c_double), ("edge_ref_ticks", C.c_double)]


class SelfcheckC(C.Structure):
    _fields_ = [("n_eval", C.c_int), ("depth", C.c_int),
                ("dev_f", C.c_float), ("dev_tr_score", C.c_float), ("dev_rot_score", C.c_float), ("dev_energy", C.c_float),
                ("cancel_ratio", C.c_float * 2), ("score_bound", C.c_float * 2),
                ("gate_f", C.c_float), ("gate_score", C.c_float), ("gate_energy", C.c_float), ("limit", C.c_float),
                ("max_h", C.c_float * 9), ("max_A", C.c_float * 8), ("max_Bm", C.c_float * 8), ("max_tab", C.c_float * 8),
                ("max_sum16", C.c_float * 8), ("max_pre", C.c_float * 8), ("max_acc", C.c_float * 8), ("headroom", C.c_float),
                ("saturated", C.c_int64), ("range_ok", C.c_int), ("dev_ok", C.c_int), ("ok", C.c_int)]


class RestraintParamsC(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("k_tr", "k_rot", "max_tr", "max_rot", "t_start")]


class SymmetryParamsC(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("gain_rot", "gain_tr", "max_rot", "max_tr", "t_start")] + [("snap_last", C.c_int32)]


class SymmetryOutC(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_double)) for n in ("theta", "screw", "axis", "axis_point", "fit_rmsd", "sym_rmsd")] + \
               [("order_m", C.POINTER(C.c_int32)), ("step", C.POINTER(C.c_float))]


class MetricsOutC(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_double)) for n in ("c_rmsd", "i_rmsd", "l_rmsd", "fnat", "dockq")] + [("n_recovered", I32P)]


class ConsensusOutC(C.Structure):
    _fields_ = [("count", I32P), ("rec_count", I32P), ("lig_count", I32P), ("n_contacts", I32P), ("score_sum", C.POINTER(C.c_int64)),
                ("bits", C.POINTER(C.c_uint64))]


class StericsParamsC(C.Structure):
    _fields_ = [("clash_cutoff", C.c_float), ("contact_cutoff", C.c_float), ("chunk_poses", C.c_int)]


class StericsOutC(C.Structure):
    _fields_ = [("n_clash", I32P), ("n_contact", I32P), ("min_dist", C.POINTER(C.c_double)), ("lig_clash", I32P), ("lig_contact", I32P)]


class SurfaceParamsC(C.Structure):
    _fields_ = [("probe", C.c_float), ("K", C.c_int), ("dirs", F32P), ("chunk_poses", C.c_int)]


class BsaOutC(C.Structure):
    _fields_ = [("lig_buried", I32P), ("rec_buried", I32P), ("lig_points", I32P), ("rec_points", I32P), ("class_points", I32P),
                ("bsa", C.POINTER(C.c_double))]


class IfaceOutC(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_int64)) for n in ("rep_q", "att_q", "elec_q", "n_pairs", "lig_vdw_q", "lig_elec_q")]


class ResconOutC(C.Structure):
    _fields_ = [(n, I32P) for n in ("ic", "n_pairs", "n_rec_res", "n_lig_res", "rec_degree", "lig_degree")] + [("contact_bits", U32P)]


class HbondOutC(C.Structure):
    _fields_ = [(n, I32P) for n in ("n_hbond", "hb_kind", "n_salt", "n_salt_atoms", "rec_hb", "lig_hb", "rec_sb", "lig_sb")]


class PairpotOutC(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_int64)) for n in ("energy_q", "n_pairs", "lig_q")] + [("counts", I32P)]


class DensityOutC(C.Structure):
    _fields_ = [("sum_q", C.POINTER(C.c_int64)), ("n_inside", I32P), ("n_above", I32P), ("atom_q", C.POINTER(C.c_int64))]


class FitOutC(C.Structure):
    _fields_ = [("rot", F32P), ("tr", F32P), ("rmsd", C.POINTER(C.c_double)), ("rec_rmsd_or_null", C.POINTER(C.c_double))]


class DistogramParamsC(C.Structure):
    _fields_ = [("contact_bins", C.c_int32), ("near_cutoff", C.c_float)]


class DistogramOutC(C.Structure):
    _fields_ = [("nll", F32P), ("nll_near", F32P), ("n_near", I32P), ("exp_contacts", F32P), ("pair_nll", F32P), ("pcontact", F32P),
                ("edist", F32P), ("pcontact_mean", F32P)]


_lib = None


def lib():
    """Load libdfmdock_amd.so (built by `make -C dfmdock_amd/csrc` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP engine has not been built. Run `python -c 'import "
            "__graft_entry__ as g; g.build()'` (or `make -C dfmdock_amd/csrc`). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    L.dfm_last_error.restype = C.c_char_p
    L.dfm_config_string.restype = C.c_char_p
    L.dfm_device_count.argtypes = [C.POINTER(C.c_int)]
    L.dfm_set_device.argtypes = [C.c_int]
    L.dfm_default_hparams.argtypes = [C.POINTER(HParamsC)]
    L.dfm_default_hparams.restype = None
    L.dfm_param_count.argtypes = [C.POINTER(HParamsC)]
    L.dfm_param_count.restype = C.c_int64
    L.dfm_model_create.argtypes = [F32P, C.c_size_t, C.POINTER(HParamsC)]
    L.dfm_model_create.restype = C.c_void_p
    L.dfm_model_destroy.argtypes = [C.c_void_p]
    L.dfm_model_destroy.restype = None
    L.dfm_complex_create.argtypes = [C.c_void_p, F32P, F32P, F32P, F32P, C.c_int, C.c_int]
    L.dfm_complex_create.restype = C.c_void_p
    L.dfm_complex_destroy.argtypes = [C.c_void_p]
    L.dfm_complex_destroy.restype = None
    L.dfm_complex_degree.argtypes = [C.c_void_p]
    L.dfm_complex_set_pose.argtypes = [C.c_void_p, F32P, F32P]
    L.dfm_complex_set_homomer.argtypes = [C.c_void_p, C.c_int]
    L.dfm_score.argtypes = [C.c_void_p, C.c_int, F32P, F32P, I32P, C.c_uint64, C.c_uint32, C.POINTER(ScoreOutC)]
    L.dfm_sample.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint64,
                             C.POINTER(InjectC), C.POINTER(TrajOutC)]
    L.dfm_refine.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint64,
                             C.POINTER(RefineParamsC), C.POINTER(InjectC), C.POINTER(RefineInjectC), C.POINTER(TrajOutC)]
    L.dfm_forward_marginal.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.POINTER(RefineInjectC), F32P, F32P]
    L.dfm_igso3_table.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dfm_get_profile.argtypes = [C.c_void_p, C.POINTER(ProfileC)]
    L.dfm_complex_selfcheck.argtypes = [C.c_void_p, C.c_int, F32P, C.c_uint64, C.c_uint32, C.POINTER(SelfcheckC)]
    L.dfm_complex_set_restraints.argtypes = [C.c_void_p, C.c_int, I32P, I32P, F32P, F32P, C.POINTER(RestraintParamsC)]
    L.dfm_restraint_eval.argtypes = [C.c_void_p, C.c_int, F32P, F32P, I32P, F32P]
    L.dfm_complex_set_symmetry.argtypes = [C.c_void_p, C.c_int, C.POINTER(SymmetryParamsC)]
    L.dfm_symmetry_eval.argtypes = [C.c_void_p, C.c_int, F32P, C.POINTER(SymmetryOutC)]
    L.dfm_pose_rmsd.argtypes = [C.c_void_p, C.c_int, C.c_int, F32P, I32P, C.c_int, F32P]
    L.dfm_pose_cluster.argtypes = [C.c_void_p, C.c_int, C.c_int, F32P, I32P, C.c_int, F32P, C.c_float, C.c_int, C.c_int, I32P, I32P, I32P,
                                   I32P]
    L.dfm_pose_last_timing.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dfm_native_create.argtypes = [C.c_void_p, F32P, F32P, C.c_int, C.c_int, C.c_float, C.c_float]
    L.dfm_native_create.restype = C.c_void_p
    L.dfm_native_destroy.argtypes = [C.c_void_p]
    L.dfm_native_destroy.restype = None
    L.dfm_native_info.argtypes = [C.c_void_p, I32P, I32P, I32P, I32P, I32P, I32P]
    L.dfm_pose_metrics.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.POINTER(MetricsOutC)]
    L.dfm_metrics_last_timing.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dfm_pose_consensus.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, F32P, F32P, C.POINTER(C.c_uint8), C.c_float,
                                     C.POINTER(ConsensusOutC)]
    L.dfm_consensus_chunk_poses.argtypes = [C.c_int, C.c_int]
    L.dfm_consensus_last_timing.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dfm_atoms_create.argtypes = [C.c_void_p, C.c_int, F32P, C.c_int, F32P, F32P, C.POINTER(StericsParamsC)]
    L.dfm_atoms_create.restype = C.c_void_p
    L.dfm_atoms_destroy.argtypes = [C.c_void_p]
    L.dfm_atoms_destroy.restype = None
    L.dfm_atoms_info.argtypes = [C.c_void_p, I32P, I32P, F32P]
    L.dfm_pose_sterics.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.POINTER(StericsOutC)]
    L.dfm_pose_sterics_chunked.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.c_int, C.POINTER(StericsOutC)]
    L.dfm_sterics_last_timing.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dfm_sterics_exit_counts.argtypes = [C.c_int, C.POINTER(C.c_uint64)]
    L.dfm_surface_create.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.c_int, F32P, F32P, F32P, C.POINTER(SurfaceParamsC)]
    L.dfm_surface_create.restype = C.c_void_p
    L.dfm_surface_destroy.argtypes = [C.c_void_p]
    L.dfm_surface_destroy.restype = None
    L.dfm_surface_info.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), I32P, I32P, I32P, F32P, I32P, I32P, F32P]
    L.dfm_pose_bsa.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.POINTER(BsaOutC)]
    L.dfm_pose_bsa_chunked.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.c_int, C.POINTER(BsaOutC)]
    L.dfm_bsa_last_timing.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dfm_iface_create.argtypes = [C.c_void_p, C.c_int, F32P, F32P, F32P, F32P, C.c_int, F32P, F32P, F32P, F32P, F32P, C.c_float, C.c_float,
                                   C.c_float, C.c_float]
    L.dfm_iface_create.restype = C.c_void_p
    L.dfm_iface_destroy.argtypes = [C.c_void_p]
    L.dfm_iface_destroy.restype = None
    L.dfm_iface_info.argtypes = [C.c_void_p, I32P, I32P, F32P, C.POINTER(C.c_double)]
    L.dfm_pose_iface_energy.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.POINTER(IfaceOutC)]
    L.dfm_pose_iface_energy_chunked.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.c_int, C.POINTER(IfaceOutC)]
    L.dfm_iface_last_timing.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dfm_rescon_create.argtypes = [C.c_void_p, C.c_int, F32P, I32P, C.c_int, C.POINTER(C.c_uint8), C.c_int, F32P, I32P, C.c_int,
                                    C.POINTER(C.c_uint8), F32P, C.c_float]
    L.dfm_rescon_create.restype = C.c_void_p
    L.dfm_rescon_destroy.argtypes = [C.c_void_p]
    L.dfm_rescon_destroy.restype = None
    L.dfm_rescon_info.argtypes = [C.c_void_p, I32P, I32P, F32P, I32P, I32P]
    L.dfm_pose_rescon.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.POINTER(ResconOutC)]
    L.dfm_pose_rescon_chunked.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.c_int, C.POINTER(ResconOutC)]
    L.dfm_rescon_last_timing.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dfm_rescon_last_phases.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    U8P = C.POINTER(C.c_uint8)
    L.dfm_hbond_create.argtypes = [C.c_void_p, C.c_int, F32P, F32P, U8P, I32P, C.c_int, C.c_int, F32P, F32P, U8P, I32P, C.c_int, F32P,
                                   C.c_float, C.c_double, C.c_float, C.POINTER(C.c_int)]
    L.dfm_hbond_create.restype = C.c_void_p
    L.dfm_hbond_destroy.argtypes = [C.c_void_p]
    L.dfm_hbond_destroy.restype = None
    L.dfm_hbond_info.argtypes = [C.c_void_p, I32P, I32P, F32P, I32P, I32P, I32P]
    L.dfm_pose_hbonds.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.POINTER(HbondOutC)]
    L.dfm_pose_hbonds_chunked.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.c_int, C.POINTER(HbondOutC)]
    L.dfm_hbond_last_timing.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dfm_hbond_last_phases.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dfm_pairpot_create.argtypes = [C.c_void_p, C.c_int, F32P, I32P, C.c_int, F32P, I32P, F32P, C.c_int, C.c_int, F32P, F32P, C.c_int]
    L.dfm_pairpot_create.restype = C.c_void_p
    L.dfm_pairpot_destroy.argtypes = [C.c_void_p]
    L.dfm_pairpot_destroy.restype = None
    L.dfm_pairpot_info.argtypes = [C.c_void_p, I32P, I32P, F32P, C.POINTER(C.c_double), I32P, I32P]
    L.dfm_pose_pairpot.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.POINTER(PairpotOutC)]
    L.dfm_pose_pairpot_chunked.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.c_int, C.POINTER(PairpotOutC)]
    L.dfm_pairpot_last_timing.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dfm_pairpot_last_phases.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dfm_score_distogram.argtypes = [C.c_void_p, C.c_int, F32P, F32P, I32P, C.c_uint64, C.c_uint32, C.POINTER(DistogramParamsC),
                                      C.POINTER(DistogramOutC)]
    L.dfm_distogram_last_timing.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dfm_pose_fit.argtypes = [C.c_void_p, C.c_int, C.c_int, F32P, F32P, C.c_int, F32P, F32P, F32P, C.POINTER(FitOutC)]
    L.dfm_pose_fit_chunked.argtypes = [C.c_void_p, C.c_int, C.c_int, F32P, F32P, C.c_int, F32P, F32P, F32P, C.c_int, C.POINTER(FitOutC)]
    L.dfm_fit_last_timing.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dfm_density_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, F32P, F32P, C.c_int, F32P, C.c_int, F32P, F32P, F32P, C.c_float,
                                     C.POINTER(C.c_int)]
    L.dfm_density_create.restype = C.c_void_p
    L.dfm_density_destroy.argtypes = [C.c_void_p]
    L.dfm_density_destroy.restype = None
    L.dfm_density_info.argtypes = [C.c_void_p, I32P, I32P, I32P, I32P, I32P, C.POINTER(C.c_double)]
    L.dfm_pose_density.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.POINTER(DensityOutC)]
    L.dfm_pose_density_chunked.argtypes = [C.c_void_p, C.c_int, F32P, F32P, C.c_int, C.POINTER(DensityOutC)]
    L.dfm_density_last_timing.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dfm_trim_cache.argtypes = [C.c_int]
    L.dfm_trim_cache.restype = C.c_longlong
    L.dfm_alloc_diag.argtypes = [C.POINTER(C.c_int64)]
    L.dfm_diffusion_coef.argtypes = [C.POINTER(HParamsC), C.c_int, C.c_double, C.POINTER(C.c_double),
                                     C.POINTER(C.c_double)]
    _lib = L
    return L


class DfmError(RuntimeError):
    pass


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().dfm_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError(f"{what}: {msg}")   # the reference raises ValueError for these
        raise DfmError(f"{what}: status {rc}: {msg}")
