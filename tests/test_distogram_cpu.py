"""The distogram reductions without a GPU: the float64 definition (dfmdock_amd/distogram.py) against numbers recorded from the
reference's own distogram_loss (tests/golden/distogram_ref.npz, make_golden_distogram.py), hand-made logits, the bin edges, the
restraint hand-off, the C layout of the new structs and the command line's flag plumbing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, complex_for, load_golden, pair_hparams
from dfmdock_amd import distogram as DG


def case_distances(case, stride):
    g, cx = load_golden(case + ".npz"), complex_for(case)
    return DG.ca_distances(cx["rec_pos"], g["lig_pos"])[::stride, ::stride]


@pytest.mark.parametrize("case,key,stride", [("fwd2_syn_24_16", "syn_24_16", 1), ("fwd2_7CEI_p1", "cei_p1_stride8", 8)])
def test_definition_against_the_reference_loss(case, key, stride):
    ref, z = load_golden("distogram_ref.npz"), load_golden("fwd2_dist.npz")[key]
    e = DG.pose_scores(z, case_distances(case, stride), int(ref["contact_bins"]))
    assert abs(e["nll"] - float(ref[key + "_nll"])) < 1e-6
    assert abs(e["nll"] - {"syn_24_16": 4.36285, "cei_p1_stride8": 4.21576}[key]) < 1e-5
    np.testing.assert_allclose([e["pcontact"].min(), e["pcontact"].max()], ref[key + "_pcontact_range"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(e["pcontact"][:4, :4], ref[key + "_pcontact_4x4"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(e["pair_nll"][:4, :4], ref[key + "_pair_nll_4x4"], rtol=0, atol=1e-6)
    if key == "syn_24_16":
        assert abs(e["pcontact"].min() - 0.0606) < 1e-4 and abs(e["pcontact"].max() - 0.1884) < 1e-4


def test_hand_made_logits():
    D = np.array([[2.0, 7.0, 30.0, 60.0]])
    for cb in (1, 7, 63):
        e = DG.pose_scores(np.zeros((1, 4, 64)), D, cb, 12.0)
        assert e["nll"] == pytest.approx(np.log(64), abs=1e-14) and np.allclose(e["pcontact"], cb / 64, atol=1e-15)
        assert np.allclose(e["edist"], DG.CENTRES.mean(), atol=1e-12) and e["exp_contacts"] == pytest.approx(4 * cb / 64)
    for big in (50.0, -50.0):      # a one-hot logit: no overflow, the mass is where it should be
        z = np.zeros((1, 4, 64))
        z[..., 5] = big
        e = DG.pose_scores(z, D, 7, 12.0)
        assert all(np.isfinite(e[k]).all() for k in ("pair_nll", "pcontact", "edist"))
        if big > 0:
            assert np.allclose(e["pcontact"], 1.0) and np.allclose(e["edist"], DG.CENTRES[5])
            assert e["pair_nll"][0, 1] == pytest.approx(0.0, abs=1e-12) and e["pair_nll"][0, 0] == pytest.approx(50.0, abs=1e-12)      # 7 A is bin 5
        else:
            assert np.allclose(e["pcontact"], 6 / 63, atol=1e-12) and e["pair_nll"][0, 1] == pytest.approx(50.0 + np.log(63), abs=1e-9)
    for cb in (0, 64):
        with pytest.raises(ValueError):
            DG.pair_maps(np.zeros((1, 1, 64)), np.ones((1, 1)), cb)


def test_bin_edges_and_centres():
    assert DG.BOUNDS.shape == (63,) and DG.BOUNDS[0] == 3.25 and DG.BOUNDS[-1] == 50.75 and DG.STEP == pytest.approx(0.766129, abs=1e-6)
    assert DG.bin_of(3.25) == 0 and DG.bin_of(np.nextafter(3.25, 4)) == 1 and DG.bin_of(0.0) == 0
    assert DG.bin_of(50.75) == 62 and DG.bin_of(np.nextafter(50.75, 60)) == 63 and DG.bin_of(1e4) == 63
    assert DG.BOUNDS[6] == pytest.approx(7.846774, abs=1e-6) and DG.bin_of(DG.BOUNDS[6]) == 6 and DG.bin_of(7.85) == 7
    np.testing.assert_allclose(DG.CENTRES[1:-1], 0.5 * (DG.BOUNDS[:-1] + DG.BOUNDS[1:]), atol=1e-12)      # inner bins: midpoints
    assert DG.CENTRES[0] == pytest.approx(3.25 - DG.STEP / 2) and DG.CENTRES[63] == pytest.approx(50.75 + DG.STEP / 2)
    d = np.linspace(0, 60, 2001)
    np.testing.assert_array_equal(DG.bin_of(d), np.searchsorted(DG.BOUNDS ** 2, d ** 2, side="left"))


def test_empty_near_set_is_nan():
    e = DG.pose_scores(np.zeros((2, 3, 64)), np.full((2, 3), 20.0), 7, 12.0)
    assert e["n_near"] == 0 and np.isnan(e["nll_near"]) and np.isfinite(e["nll"])
    e = DG.pose_scores(np.zeros((2, 3, 64)), np.array([[20.0, 11.0, 12.0], [5.0, 30.0, 40.0]]), 7, 12.0)
    assert e["n_near"] == 2 and e["nll_near"] == pytest.approx(np.log(64))      # D < cutoff: 12.0 itself is out


def test_pcontact_mean_is_the_ordered_double_sum():
    rng = np.random.default_rng(0)
    pc = rng.random((5, 3, 4)).astype(np.float32)
    s = np.zeros((3, 4))
    for b in range(5):
        s = s + pc[b].astype(np.float64)
    np.testing.assert_array_equal(DG.pcontact_mean(pc), s / 5)


def test_top_contacts_order_ties_and_the_restraint_file():
    from dfmdock_amd import consensus as CS
    from dfmdock_amd.restraints import parse_restraints
    pm = np.array([[0.1, 0.9, 0.5], [0.9, 0.5, 0.2]])
    top = DG.top_contacts(pm, 4)
    assert [(r, l) for r, l, _ in top] == [(0, 1), (1, 0), (0, 2), (1, 1)] and [p for _, _, p in top] == [0.9, 0.9, 0.5, 0.5]
    assert DG.top_contacts(pm, 0) == [] and len(DG.top_contacts(pm, 99)) == 6
    with pytest.raises(ValueError):
        DG.top_contacts(pm[0], 1)
    keys = lambda ch, n: {"residues": [(ch, 10 + i, " ", "ALA") for i in range(n)],
                          "atoms": [{"chain": ch, "res_id": 10 + i, "ins": " "} for i in range(n)]}
    rec, lig = keys("A", 2), keys("B", 3)
    groups = DG.contact_groups(pm / 3.0, 4, upper=7.5)      # weights that are not short decimals
    assert [g.pairs for g in groups] == [((0, 1),), ((1, 0),), ((0, 2),), ((1, 1),)]
    text = CS.format_restraints(groups, rec, lig, header="predicted contacts")
    back = parse_restraints(text, rec, lig)
    assert back == groups and all(g.upper == 7.5 for g in back) and [g.weight for g in back] == [0.9 / 3.0, 0.9 / 3.0, 0.5 / 3.0, 0.5 / 3.0]


def test_new_structs_have_the_c_layout(tmp_path):
    from dfmdock_amd import _lib
    names = {"dfm_distogram_params": _lib.DistogramParamsC, "dfm_distogram_out": _lib.DistogramOutC}
    probes = {"dfm_distogram_params": ["contact_bins", "near_cutoff"],
              "dfm_distogram_out": ["nll", "nll_near", "n_near", "exp_contacts", "pair_nll", "pcontact", "edist", "pcontact_mean"]}
    body = "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names)
    body += "".join(f'printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for n, fs in probes.items() for f in fs)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dfmdock_amd.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    for n, cls in names.items():
        assert int(got[n]) == C.sizeof(cls), n
        assert [f for f, _ in cls._fields_] == probes[n]
        for f in probes[n]:
            assert int(got[f"{n}.{f}"]) == getattr(cls, f).offset, (n, f)
    lib = _lib.lib()
    for s in ("dfm_score_distogram", "dfm_distogram_last_timing"):
        assert s in _lib.EXPORTS and hasattr(lib, s) and getattr(lib, s).argtypes
    # nothing is enqueued for bad arguments, so the refusals need no device
    a, b = C.c_double(), C.c_double()
    assert lib.dfm_distogram_last_timing(C.byref(a), C.byref(b)) == 0 and lib.dfm_distogram_last_timing(None, None) != 0
    assert lib.dfm_score_distogram(None, 1, None, None, None, 0, 0, None, None) != 0


def test_cli_flags_and_the_family_0_refusal(tmp_path):
    from cli_fixtures import write_ckpt
    from dfmdock_amd import cli
    from dfmdock_amd.weights import HParams, load_lightning_checkpoint
    base = ["r.pdb", "l.pdb", "--ckpt", "m.ckpt", "--features", "f.npz"]
    for cmd in ("dock", "refine"):
        a = cli.parse_args([cmd] + base)
        assert not a.distogram and a.distogram_t == 1e-3 and cli.distogram_kwargs(a, None) == {}
        for extra in (["--distogram"], ["--rank", "distogram"], ["--distogram-map", "m.npz"], ["--distogram-restraints", "f.txt"]):
            assert cli.parse_args([cmd] + base + extra).distogram, extra
        a = cli.parse_args([cmd] + base + ["--distogram-restraints", "f.txt", "--restraint-top", "4", "--restraint-upper", "7", "--distogram-t", "0.01"])
        assert (a.restraint_top, a.restraint_upper, a.distogram_t, a.consensus) == (4, 7.0, 0.01, False)
        for bad in (["--distogram-t", "0.01"], ["--distogram", "--distogram-t", "0"], ["--distogram", "--distogram-t", "1.5"], ["--restraint-top", "4"]):
            with pytest.raises(SystemExit):
                cli.parse_args([cmd] + base + bad)
    # the seeded checkpoints of the command-line tests: the family is read off the keys, and family 0 ends the command before sampling
    models = {}
    for fam, hp in ((0, HParams()), (1, pair_hparams())):
        path = str(tmp_path / f"m{fam}.ckpt")
        write_ckpt(path, hp)
        models[fam] = type("Model", (), {"hp": load_lightning_checkpoint(path)[1]})()
        assert models[fam].hp.family == fam
    a = cli.parse_args(["dock"] + base + ["--rank", "distogram", "--distogram-map", "m.npz"])
    with pytest.raises(SystemExit, match="family-1"):
        cli.distogram_kwargs(a, models[0])
    assert cli.distogram_kwargs(a, models[1]) == dict(distogram=True, rank="distogram", distogram_t=1e-3, distogram_maps=True)
    assert cli.distogram_kwargs(cli.parse_args(["refine"] + base + ["--distogram"]), models[1])["distogram_maps"] is False


def test_drivers_refuse_family_0_before_sampling(monkeypatch):
    from dfmdock_amd import driver

    def no_handle(*a, **k):
        raise AssertionError("a handle was opened")
    monkeypatch.setattr(driver.engine, "Complex", no_handle)
    m0 = type("Model", (), {"hp": type("Hp", (), {"family": 0})()})()
    for fn in (driver.dock_pair, driver.refine_pair):
        for kw in (dict(distogram=True), dict(rank="distogram"), dict(distogram_maps=True)):
            with pytest.raises(ValueError, match="family-1"):
                fn(m0, None, None, None, None, **kw)
    m1 = type("Model", (), {"hp": type("Hp", (), {"family": 1})()})()
    with pytest.raises(ValueError, match="distogram_t"):
        driver.dock_pair(m1, None, None, None, None, distogram=True, distogram_t=0.0)
    assert driver._check_distogram(m1, False, "energy", 1e-3, False, 256) is None
    assert driver._check_distogram(m1, False, "distogram", 1e-3, False, 64) == (True, 1e-3, False, 64)


def test_distogram_pick_and_result():
    """The selecting half on made-up numbers: the lowest nll among the poses the clash filter left, NaN never wins, the key is the nll."""
    from dfmdock_amd import driver
    dd = dict(nll=np.array([4.2, np.nan, 4.0, 4.1]), nll_near=np.array([4.0, np.nan, 3.9, np.nan]), n_near=np.array([3, 0, 2, 0]),
              exp_contacts=np.array([10.0, np.nan, 12.0, 11.0]), t=1e-3, contact_bins=7)
    orig = driver.ensemble_distogram
    driver.ensemble_distogram = lambda *a, **k: dd
    try:
        cols = dict(rot_update=np.zeros((4, 3)), tr_update=np.zeros((4, 3)))
        def pick(k, key, opts, bad):      # the selecting stages of driver._finish, from the pose and key the driver's own rule gave
            run = driver._Run(None, type("G", (), {"lig_pos0": None}), None, None, cols, "fp32", {"distogram": opts})
            run.k, run.key, run.bad = k, key, bad
            for a in driver.ANALYSES:
                if a.stage in ("handle", "select") and a.name in run.opts:
                    a.run(run)
            return run.k, run.key, run.data.get("distogram")
        assert pick(0, None, None, None) == (0, None, None)
        k, key, d = pick(0, np.arange(4.0), (True, 1e-3, False, 2), None)
        assert k == 2 and np.array_equal(key, dd["nll"], equal_nan=True)
        bad = np.array([False, False, True, False])
        k, key, d = pick(0, np.arange(4.0), (True, 1e-3, False, 2), bad)
        assert k == 3 and np.isnan(key[2])
        k, key, d = pick(1, np.arange(4.0), (False, 1e-3, False, 2), None)
        assert k == 1 and np.array_equal(key, np.arange(4.0))
        r = driver._distogram_result(dd, 3, (True, 1e-3, False, 2), bad)
        assert r["distogram"] == dict(dist_nll=4.1, dist_nll_near=None, exp_contacts=11.0, n_near=0, rank=1, t=1e-3, contact_bins=7,
                                      ranked_by_distogram=True) and r["index"] == 3
    finally:
        driver.ensemble_distogram = orig
