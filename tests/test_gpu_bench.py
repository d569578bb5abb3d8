"""bench.py itself on one GPU: a plain run carries the headline and nothing that needs runs of its own (the secondary records are
behind --full), and --dump-outputs writes what the last timed step returned - the same arrays from run to run, the same arrays the
engine returns for that step's call."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SHAPE = dict(R=40, L=30, batch=8, num_steps=4, steps=2, warmup=1)
NAMES = ("lig_pos", "rot_update", "tr_update", "energy", "num_clashes", "final_scores", "records")


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(SHAPE["steps"]), "--warmup", str(SHAPE["warmup"]),
           "--R", str(SHAPE["R"]), "--L", str(SHAPE["L"]), "--batch", str(SHAPE["batch"]), "--num-steps", str(SHAPE["num_steps"]),
           "--dump-outputs", str(out_dir)]
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout.decode()[-2000:]
    return json.loads(lines[0]), {n: np.load(os.path.join(out_dir, n + ".npy")) for n in NAMES}


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out, a = _bench(tmp_path / "a")
    assert out["steps"] == SHAPE["steps"] and out["warmup"] == SHAPE["warmup"] and out["higher_is_better"] is True
    assert out["unit"] == "trajectories/s" and out["dtype"] == "f16" and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(SHAPE["batch"] / (out["ms_per_step"] / 1e3))
    assert not {"fp32_engine", "c4", "c5", "c4_sharded", "cpu_baseline"} & set(out)      # secondary records: --full only
    B, L = SHAPE["batch"], SHAPE["L"]
    assert a["lig_pos"].shape == (B, L, 3, 3) and a["energy"].shape == (B,) and a["records"].shape == (B, 10)
    assert all(v.dtype == np.float32 for v in a.values()) and all(np.isfinite(v).all() for v in a.values())
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in NAMES)

    _, b = _bench(tmp_path / "b")
    for n in NAMES:      # same arguments, same inputs: the same outputs
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)

    # the last timed step is the engine's call with seed 1000 + warmup + steps - 1 on bench's seeded weights and complex
    from dfmdock_amd import engine
    from dfmdock_amd.synthetic import make_complex
    from dfmdock_amd.weights import make_random_weights, pack_blob
    engine.set_device(0)
    cx = make_complex(SHAPE["R"], L, seed=1)
    model = engine.Model(pack_blob(make_random_weights(0)))
    gx = engine.Complex(model, cx["rec_x"], cx["lig_x"], cx["rec_pos"], cx["lig_pos"])
    r = gx.sample(B=B, num_steps=SHAPE["num_steps"], seed=1000 + SHAPE["warmup"] + SHAPE["steps"] - 1, **engine.precision_kwargs("mfma16"))
    gx.close()
    model.close()
    for n in ("lig_pos", "rot_update", "tr_update", "energy", "num_clashes", "final_scores"):
        np.testing.assert_array_equal(a[n], np.asarray(r[n], np.float32), err_msg=n)
