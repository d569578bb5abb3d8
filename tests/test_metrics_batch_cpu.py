"""CPU side of the batched docking metrics: the float64 batch definition, the ABI declarations, the command line and the argument
checks of the drivers (the GPU call itself: tests/test_gpu_metrics.py)."""
import re
import os

import numpy as np
import pytest

from conftest import ROOT, db5_complex, db5_ids, load_golden


def test_batch_equals_a_loop_of_compute_metrics():
    from dfmdock_amd.metrics import NativeContext, compute_metrics, compute_metrics_batch, _min_dist_pairs
    rng = np.random.default_rng(4)
    for cid in db5_ids()[:3]:
        c = db5_complex(cid)
        native = (c["rec_pos"], c["lig_pos"])
        ctx = NativeContext(native)
        poses = (c["lig_pos"][None] + np.linspace(0, 3, 5, dtype=np.float32)[:, None, None, None] * rng.standard_normal(3).astype(np.float32))
        recs = (c["rec_pos"][None] + 0.1 * rng.standard_normal((5,) + c["rec_pos"].shape)).astype(np.float32)
        for rec in (None, recs):
            got = compute_metrics_batch(poses, native, ctx, rec)
            for p in range(5):
                mr = c["rec_pos"] if rec is None else rec[p]
                want = compute_metrics((mr, poses[p]), native, ctx)
                for k, v in want.items():
                    assert got[k][p] == v and got[k].dtype == np.float64, (cid, p, k)
                d = _min_dist_pairs(np.asarray(mr, np.float32).astype(np.float64), poses[p].astype(np.float64), *ctx.act)
                assert got["n_recovered"][p] == int((d < 5.5).sum())
                assert want["fnat"] == round(int(got["n_recovered"][p]) / (len(ctx.act[0]) + 1e-6), 6)
        assert compute_metrics_batch(poses, native)["fnat"][0] == 1.0      # pose 0 is the native


def test_abi_declares_and_binds_the_metrics_calls():
    import ctypes as C
    from dfmdock_amd import _lib
    txt = open(os.path.join(ROOT, "include", "dfmdock_amd.h")).read()
    names = ("dfm_native_create", "dfm_native_destroy", "dfm_native_info", "dfm_pose_metrics", "dfm_metrics_last_timing")
    lib = _lib.lib()
    for n in names:
        assert re.search(r"\b" + n + r"\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)), n
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert "typedef struct dfm_native dfm_native;" in txt
    # dfm_metrics_out: five double pointers and one int32 pointer, in the header's order
    m = re.search(r"typedef struct \{([^}]*)\} dfm_metrics_out;", txt)
    fields = re.findall(r"\*\s*(\w+)", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f for f, _ in _lib.MetricsOutC._fields_] == ["c_rmsd", "i_rmsd", "l_rmsd", "fnat", "dockq", "n_recovered"]
    assert C.sizeof(_lib.MetricsOutC) == 6 * C.sizeof(C.c_void_p)
    # host-only error paths: no device is touched before the arguments are checked
    assert lib.dfm_pose_metrics(None, 1, None, None, None) == -1 and b"NULL" in lib.dfm_last_error()
    assert not lib.dfm_native_create(None, None, None, 1, 1, 10.0, 5.5) and lib.dfm_last_error()
    a, b = C.c_double(-1), C.c_double(-1)
    assert lib.dfm_metrics_last_timing(C.byref(a), C.byref(b)) == 0 and a.value == 0.0 and b.value == 0.0
    assert lib.dfm_metrics_last_timing(None, None) == -1


def test_cli_parses_the_metrics_options():
    from dfmdock_amd import cli
    pair = ["r.pdb", "l.pdb", "--ckpt", "m.ckpt", "--features", "f.npz"]
    assert cli.parse_args(["dock"] + pair).native is None and cli.parse_args(["refine"] + pair).native is None
    assert cli.parse_args(["dock"] + pair + ["--native", "nr.pdb", "nl.pdb"]).native == ["nr.pdb", "nl.pdb"]
    assert cli.parse_args(["refine"] + pair + ["--native", "nr.pdb", "nl.pdb", "--t-begin", "0.2"]).native == ["nr.pdb", "nl.pdb"]
    with pytest.raises(SystemExit):
        cli.parse_args(["dock"] + pair + ["--native", "only_one.pdb"])
    sw = ["sweep", "--db5", "d", "--ckpt", "m.ckpt"]
    a = cli.parse_args(sw)
    assert a.metrics == "host" and a.step_metrics is None
    assert cli.parse_args(sw + ["--metrics", "gpu"]).metrics == "gpu"
    a = cli.parse_args(sw + ["--step-metrics", "steps.csv"])
    assert a.metrics == "gpu" and a.step_metrics == "steps.csv"
    with pytest.raises(SystemExit):
        cli.parse_args(sw + ["--metrics", "cpu"])


def test_step_summary():
    from dfmdock_amd import cli
    rows = [{"id": "A", "index": "0", "energy": -1.0}, {"id": "A", "index": "1", "energy": -2.0}, {"id": "B", "index": "0", "energy": 0.0}]
    steps = [{"id": "A", "index": "0", "step": s, "DockQ": d} for s, d in enumerate((0.1, 0.9, 0.2))] + \
            [{"id": "A", "index": "1", "step": s, "DockQ": d} for s, d in enumerate((0.1, 0.2, 0.25))] + \
            [{"id": "B", "index": "0", "step": s, "DockQ": d} for s, d in enumerate((0.01, 0.02, 0.03))]
    got = cli.step_summary(steps, rows)
    assert got == {"A": {"top1_first_acceptable_step": 2, "best_DockQ_any_step": 0.9},
                   "B": {"top1_first_acceptable_step": None, "best_DockQ_any_step": 0.03}}


def test_drivers_check_their_metrics_arguments():
    """Bad options fail before a handle is created or a kernel launched (model = None would fail otherwise)."""
    from dfmdock_amd import driver
    with pytest.raises(ValueError, match="metrics must be"):
        driver.run_set(None, [], metrics="cuda")
    with pytest.raises(ValueError, match="needs metrics='gpu'"):
        driver.run_set(None, [], step_metrics=True)
    with pytest.raises(ValueError, match="needs metrics='gpu'"):
        driver.run_set(None, [], step_csv="steps.csv")
    rec, lig = {"bb_coords": np.zeros((7, 3, 3), np.float32)}, {"bb_coords": np.zeros((5, 3, 3), np.float32)}
    native = (np.zeros((7, 3, 3), np.float32), np.zeros((6, 3, 3), np.float32))
    for fn in (driver.dock_pair, driver.refine_pair):
        with pytest.raises(ValueError, match="7 receptor / 6 ligand residues, the input pair 7 / 5"):
            fn(None, rec, lig, None, None, native=native)
    assert driver.STEP_FIELDS == ["id", "index", "step", "t", "c_rmsd", "i_rmsd", "l_rmsd", "fnat", "DockQ"]
