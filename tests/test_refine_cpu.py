"""Local refinement, host side: the float64 mirror dfmdock_amd/refine.py against the reference's recorded forward process
(tests/golden/igso3_ref.npz, written by tests/golden/make_golden_igso3.py running the unmodified reference), the inverse-cdf rule on a
non-monotone table, the C layout of the two new structs and the command-line parser."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def ref():
    return load_golden("igso3_ref.npz")


def test_mirror_tables_and_angles_vs_reference(ref):
    """sigma_idx equal; cdf within 1e-12 absolute; sample_igso3 angles within 1e-9 rad for the recorded uniforms (drawn in
    0.01 <= u <= 0.99, inside the strictly increasing part of every table - asserted by the generating script, so no case is left out).
    The cdf bound: an independent float64 evaluation with another summation order (ascending over l here, numpy's pairwise sum in the
    reference) differs from the reference's table by at most 6.7e-16 on the eight t (0.001: 6.7e-16, 0.02: 3.3e-16, 0.05: 1.1e-16,
    0.1 / 0.2 / 0.3 / 1.0: 4.4e-16, 0.5: 1.1e-16); angles: at most 8.9e-16 rad."""
    from dfmdock_amd import refine as RF
    np.testing.assert_array_equal(ref["omega"], RF.OMEGA)
    for n, t in enumerate(ref["t"]):
        idx, sg = RF.sigma_index(t)
        assert idx == int(ref[f"t{n}/sigma_idx"]) and sg == float(ref[f"t{n}/sigma"])
        cdf = RF.igso3_cdf(sg)
        dev = np.abs(cdf - ref[f"t{n}/cdf"]).max()
        ang = RF.inverse_cdf(ref[f"t{n}/u"], cdf)
        da = np.abs(ang - ref[f"t{n}/angle"]).max()
        print(f"mirror t={t}: idx {idx} max |cdf - reference| {dev:.2e} max |angle - reference| {da:.2e}")
        assert ref[f"t{n}/u"].min() >= 0.01 and ref[f"t{n}/u"].max() <= 0.99 and ref[f"t{n}/u"].size == 64
        assert dev < 1e-12 and da < 1e-9


def test_mirror_noised_pose_vs_reference(ref):
    """The reference's own noising of syn_24_16 (forward_marginal of both diffusers under a seeded np.random, then modify_coords) from
    its recorded draws: rotation vector / translation in float64, pose within 3e-5 A - the project's gate for randomize_pose
    (test_gpu_parity.py), the same arithmetic class: one float32 rigid transform of coordinates of tens of A."""
    from conftest import complex_for
    from dfmdock_amd import refine as RF
    np.testing.assert_array_equal(complex_for("fwd_syn_24_16")["lig_pos"], ref["lig_pos"])
    for n, t in enumerate(ref["t"]):
        rot, tr = RF.forward_marginal(t, [ref[f"t{n}/fm_u"]], ref[f"t{n}/fm_axis"], ref[f"t{n}/fm_z"])
        np.testing.assert_allclose(rot[0], ref[f"t{n}/fm_rot"], atol=1e-12)
        np.testing.assert_allclose(tr[0], ref[f"t{n}/fm_tr"], atol=1e-12)
        assert RF.r3_sigma(t) == float(ref[f"t{n}/sigma_r3"])
        pose = RF.noise_pose(ref["lig_pos"], rot[0], tr[0])
        print(f"mirror t={t}: |rot| {np.linalg.norm(rot[0]):.4f} rad, pose vs reference {np.abs(pose - ref[f't{n}/fm_pose']).max():.2e} A")
        np.testing.assert_allclose(pose, ref[f"t{n}/fm_pose"], atol=3e-5)


def test_inverse_cdf_first_crossing_rule(ref):
    from dfmdock_amd import refine as RF
    w = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    cdf = np.array([0.1, 0.5, 0.4, 0.9, 0.8])      # not monotone
    np.testing.assert_allclose(RF.inverse_cdf([0.05, 0.1], cdf, w), [1.0, 1.0])                 # at or below cdf[0] -> omega_1
    np.testing.assert_allclose(RF.inverse_cdf([0.95], cdf, w), [5.0])                           # above every entry -> the last omega
    np.testing.assert_allclose(RF.inverse_cdf([0.3, 0.45, 0.5], cdf, w), [1.5, 1.875, 2.0])     # FIRST crossing: k = 1, not k = 3
    np.testing.assert_allclose(RF.inverse_cdf([0.7, 0.85], cdf, w), [3.6, 3.9])                 # k = 3, between (0.4, 3) and (0.9, 4)
    # the reference's table at t = 0.001 stops increasing in its tail; the rule still answers, and equals np.interp below the tail
    c = ref["t0/cdf"]
    assert np.any(np.diff(c) <= 0)
    u = np.linspace(0.001, 0.999, 401)
    np.testing.assert_allclose(RF.inverse_cdf(u, c), np.interp(u, c[:200], RF.OMEGA[:200]), atol=1e-12)
    assert RF.inverse_cdf([1.0 + 1e-9], c)[0] == np.pi


def test_time_grid_is_the_samplers_at_t_begin_one():
    from dfmdock_amd import refine as RF
    k = load_golden("scalar_kats.npz")
    ts, dt = RF.time_grid(1.0, 1e-3, 40)
    np.testing.assert_array_equal(ts, k["time_steps"].astype(np.float32))
    assert dt == np.float32(k["dt"])
    ts, _ = RF.time_grid(0.1, 1e-3, 40)
    assert ts[0] == np.float32(0.1) and ts[-1] == np.float32(1e-3) and np.all(np.diff(ts) < 0)


def test_new_structs_have_the_c_layout(tmp_path):
    from dfmdock_amd import _lib
    names = {"dfm_refine_params": (_lib.RefineParamsC, ["t_begin", "perturb", "start_pos"]),
             "dfm_refine_inject": (_lib.RefineInjectC, ["u_angle", "axis_draw", "tr_draw"])}
    body = "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names)
    body += "".join(f'printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for n, (_, fs) in names.items() for f in fs)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dfmdock_amd.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    for n, (cls, fs) in names.items():
        assert int(got[n]) == C.sizeof(cls), n
        for f in fs:
            assert int(got[f"{n}.{f}"]) == getattr(cls, f).offset, (n, f)
    for s in ("dfm_refine", "dfm_forward_marginal", "dfm_igso3_table"):
        assert s in _lib.EXPORTS


def test_cli_parser_refine_arguments(capsys):
    from dfmdock_amd import cli
    a = cli.parse_args(["refine", "r.pdb", "l.pdb", "--ckpt", "m.ckpt", "--features", "f.npz"])
    assert a.cmd == "refine" and a.t_begin == 0.1 and a.num_samples == 32 and not a.no_perturb and a.out == "output.pdb"
    a = cli.parse_args(["refine", "r.pdb", "l.pdb", "--ckpt", "m.ckpt", "--features", "f.npz", "--t-begin", "0.05", "--num-samples", "4",
                        "--no-perturb", "--restraints", "r.txt"])
    assert a.t_begin == 0.05 and a.num_samples == 4 and a.no_perturb and a.restraints == "r.txt"
    d = cli.parse_args(["dock", "r.pdb", "l.pdb", "--ckpt", "m.ckpt", "--features", "f.npz", "--top-k", "3", "--refine-t", "0.1"])
    assert d.refine_t == 0.1 and d.refine_samples == 8 and d.top_k == 3
    d = cli.parse_args(["dock", "r.pdb", "l.pdb", "--ckpt", "m.ckpt", "--features", "f.npz"])
    assert d.refine_t is None
    with pytest.raises(SystemExit):
        cli.parse_args(["dock", "r.pdb", "l.pdb", "--ckpt", "m.ckpt", "--features", "f.npz", "--refine-t", "0.1"])
    assert "--top-k" in capsys.readouterr().err
