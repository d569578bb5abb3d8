"""The sampler's host arithmetic and the decoding of the engine flags (dfmdock_amd/csrc/dfm_schedule.h) without a GPU:
tests/schedule_main.cpp, built by g++ with the address and undefined-behaviour sanitizers, is run as a child process and its output is
held against restatements in numpy float32 (one rounding per operation) and Python's math (the same libm, float64).

The time grid is pinned AS THE ENGINE COMPUTES IT TODAY: an entry is float32(t_first + float32(step * float32(i))) - the product is
rounded, then the sum - and not the once-rounded entry of torch.linspace / dfmdock_amd.refine.time_grid, from which single entries
differ by one ulp (7 of 40 on the default grid).  Closing that gap changes trajectory bits and is a change of its own: it then is a
one-line change of `grid_restated` below."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
# include/dfmdock_amd.h
DFM_E_INVALID = -1
F_MFMA16, F_NOISE_ANNEALING, F_CLASH_FORCE, F_ODE, F_PROFILE = 1 << 0, 1 << 2, 1 << 3, 1 << 4, 1 << 5
F_F16, F_BF16_OPS, F_NO_L0_TABLE, F_GRAPH, F_RESTRAINTS = 1 << 7, 1 << 9, 1 << 12, 1 << 13, 1 << 14
SIGMAS = dict(r3_min=0.1, r3_max=30.0, so3_min=0.1, so3_max=1.5)      # dfm_default_hparams
TR_NOISE, ROT_NOISE = 0.5, 0.25
CASES = [(1.0, 1e-3, 2),        # the smallest legal schedule
         (1.0, 1e-3, 40),
         (0.1, 1e-3, 40),
         (0.3, 1e-2, 7),        # odd, the split in the middle
         (1.0, 1e-3, 4097)]     # beyond the default time-grid capacity
FLAGS = {"plain": 0, "annealing": F_NOISE_ANNEALING, "ode": F_ODE}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("schedule") / "schedule_main")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1",
                           "-I", os.path.join(ROOT, "dfmdock_amd", "csrc"), os.path.join(ROOT, "tests", "schedule_main.cpp"), "-o", path])

    def run(*args):
        r = subprocess.run([path] + [str(a) for a in args], capture_output=True, text=True)
        assert r.stderr == "", r.stderr      # a sanitizer report
        assert r.returncode == 0, (r.returncode, r.stdout[-500:])
        return r.stdout.splitlines()
    return run


_grids = {}


def grid(exe, case, flags):
    """the child's output for one case, run once: name -> list of tokens"""
    if (case, flags) not in _grids:
        t_first, eps, n = case
        lines = exe("grid", repr(t_first), repr(eps), n, flags, TR_NOISE, ROT_NOISE, *(repr(SIGMAS[k]) for k in ("r3_min", "r3_max", "so3_min", "so3_max")))
        _grids[(case, flags)] = {ln.split()[0]: ln.split()[1:] for ln in lines}
    return _grids[(case, flags)]


def hexes(tokens):
    return np.array([float.fromhex(v) for v in tokens], np.float64)


def grid_restated(t_first, eps, n):
    """today's arithmetic: two roundings per entry (see the module docstring)"""
    tb, e = F32(t_first), F32(eps)
    step = F32(F32(e - tb) / F32(n - 1))
    i = np.arange(n)
    lower = (tb + (step * i.astype(F32)).astype(F32)).astype(F32)
    upper = (e - (step * (n - 1 - i).astype(F32)).astype(F32)).astype(F32)
    return np.where(i < n // 2, lower, upper).astype(F32)


def coef(which, t):
    """g(t), sigma(t) in float64 with Python's math: r3_diffuser.py:20-24, so3_diffuser.py:210-227"""
    if which == 0:
        mn, mx = SIGMAS["r3_min"], SIGMAS["r3_max"]
        sigma = mn * math.pow(mx / mn, t)
        return sigma * math.sqrt(2.0 * (math.log(mx) - math.log(mn))), sigma
    mn, mx = SIGMAS["so3_min"], SIGMAS["so3_max"]
    sigma = math.log(t * math.exp(mx) + (1.0 - t) * math.exp(mn))
    return math.sqrt(2.0 * (math.exp(mx) - math.exp(mn)) * sigma / math.exp(sigma)), sigma


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%g-%g-%d" % c)
def test_time_grid_and_coefficients(exe, case):
    t_first, eps, n = case
    out = grid(exe, case, 0)
    assert out["rc"] == ["0"]
    ts = hexes(out["ts"])
    want = grid_restated(t_first, eps, n)
    assert ts.shape == (n,) and np.array_equal(ts.astype(F32).astype(np.float64), ts)      # float32 values
    assert np.array_equal(ts.astype(F32).view(np.uint32), want.view(np.uint32))
    assert ts[0] == float(F32(t_first)) and ts[-1] == float(F32(eps))
    assert hexes(out["dt"])[0] == float(F32(want[0] - want[1]))
    for which, gk in ((1, "gr"), (0, "gt")):
        ref = np.array([coef(which, float(t)) for t in ts], np.float64)
        g, sigma = hexes(out[gk]), hexes(out["sigma%d" % which])
        assert np.all(np.abs(g - ref[:, 0]) <= 1e-15 * np.abs(ref[:, 0])), gk
        assert np.all(np.abs(sigma - ref[:, 1]) <= 1e-15 * np.abs(ref[:, 1])), which


@pytest.mark.parametrize("mode", list(FLAGS))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%g-%g-%d" % c)
def test_step_params(exe, case, mode):
    n = case[2]
    out = grid(exe, case, FLAGS[mode])
    assert out["rc"] == ["0"] and out["sizeof"] == ["48"]
    ts, dt = hexes(out["ts"]).astype(F32), F32(hexes(out["dt"])[0])
    gr, gt = hexes(out["gr"]), hexes(out["gt"])
    field = lambda k: np.array([int(v) for v in out[k]], np.uint32)
    bits = lambda x: np.asarray(x, F32).view(np.uint32)
    # every float field from the printed doubles: the product and the half in float64, one rounding to float32
    for tag, g in (("r", gr), ("t", gt)):
        assert np.array_equal(field("g2_" + tag), bits((g * g).astype(F32)))
        assert np.array_equal(field("g_" + tag), bits(g.astype(F32)))
        assert np.array_equal(field("hg2_" + tag), bits((0.5 * (g * g)).astype(F32)))
    assert np.array_equal(field("dt_f"), bits(np.full(n, dt))) and np.array_equal(field("sqrt_dt"), bits(np.full(n, np.sqrt(dt))))
    assert np.sqrt(dt).dtype == F32
    assert np.array_equal(field("step"), np.arange(n, dtype=np.uint32)) and not field("pad").any()
    if mode == "annealing":      # inference_base.py:428-430: both scales are the step's time, the last step included
        assert np.array_equal(field("tr_noise"), bits(ts)) and np.array_equal(field("rot_noise"), bits(ts))
    else:                        # the caller's scales, zero on the last step
        last = np.arange(n) == n - 1
        assert np.array_equal(field("tr_noise"), bits(np.where(last, F32(0), F32(TR_NOISE))))
        assert np.array_equal(field("rot_noise"), bits(np.where(last, F32(0), F32(ROT_NOISE))))
        assert field("tr_noise")[-1] == 0 and field("rot_noise")[-1] == 0
    if mode == "ode":            # the ODE switch is an argument of the launch, not a per-step scalar
        plain = grid(exe, case, 0)
        assert all(out[k] == plain[k] for k in out)


@pytest.mark.parametrize("t_first,eps", [(1.5, 1e-3), (1.0, -0.25), (float("nan"), 1e-3)])
def test_time_outside_unit_interval_is_rejected(exe, t_first, eps):
    out = grid(exe, (t_first, eps, 5), 0)
    assert out == {"rc": [str(DFM_E_INVALID)]}


# (MFMA16, F16, BF16_OPS) -> bf16, f16, bf16_ops, has_table: transcribed from the expressions of dfm_score / dfm_sample
#   f16 = F16; bf16 = MFMA16 or F16; bf16_ops = bf16 and not f16 and BF16_OPS; has_table = (bf16 and not f16 and not BF16_OPS) or not bf16
ENGINE_SEL = {(0, 0, 0): (0, 0, 0, 1), (1, 0, 0): (1, 0, 0, 1), (0, 1, 0): (1, 1, 0, 0), (1, 1, 0): (1, 1, 0, 0),
              (0, 0, 1): (0, 0, 0, 1), (1, 0, 1): (1, 0, 1, 0), (0, 1, 1): (1, 1, 0, 0), (1, 1, 1): (1, 1, 0, 0)}


def test_engine_selection(exe):
    rows = [[int(v) for v in ln.split()] for ln in exe("sel")]
    assert len(rows) == 16 and len({r[0] for r in rows}) == 16
    seen = {}
    for flags, bf16, f16, ops, table, default in rows:
        assert flags & ~(F_MFMA16 | F_F16 | F_BF16_OPS | F_NO_L0_TABLE) == 0
        key = (int(bool(flags & F_MFMA16)), int(bool(flags & F_F16)), int(bool(flags & F_BF16_OPS)))
        no_table = bool(flags & F_NO_L0_TABLE)
        assert (bf16, f16, ops, table) == ENGINE_SEL[key], flags
        assert default == int(table and not no_table), flags      # dfm_sample: ... and not DFM_F_NO_L0_TABLE
        seen[key + (int(no_table),)] = default
    # dfm_complex_selfcheck runs its 16-bit pass with DFM_F_MFMA16 forced and tests DFM_F_F16 | DFM_F_BF16_OPS | DFM_F_NO_L0_TABLE
    for f in (0, 1):
        for o in (0, 1):
            for nt in (0, 1):
                assert seen[(1, f, o, nt)] == int(not (f or o or nt))


def test_graph_key(exe):
    base = F_MFMA16
    inputs = [(4, base, 1, 0), (5, base, 1, 0), (4, base, 0, 0), (4, base, 1, 1), (4, 0, 1, 0), (4, F_F16, 1, 0), (4, base | F_BF16_OPS, 1, 0),
              (4, base | F_CLASH_FORCE, 1, 0), (4, base | F_ODE, 1, 0), (4, base | F_NO_L0_TABLE, 0, 0), (1 << 20, base, 1, 0),
              # what the key does not hold: flags that do not change the captured nodes
              (4, base | F_PROFILE, 1, 0), (4, base | F_GRAPH, 1, 0), (4, base | F_NOISE_ANNEALING, 1, 0), (4, base | F_RESTRAINTS, 1, 0)]
    keys = [int(ln) for ln in exe("key", *[v for t in inputs for v in t])]
    mask = F_MFMA16 | F_F16 | F_BF16_OPS | F_CLASH_FORCE | F_ODE | F_NO_L0_TABLE
    ident = [(b, fl & mask, l0, rs) for b, fl, l0, rs in inputs]
    assert len(keys) == len(inputs) and len(set(ident)) == 11
    for i in range(len(inputs)):
        for j in range(len(inputs)):
            assert (keys[i] == keys[j]) == (ident[i] == ident[j]), (inputs[i], inputs[j])


@pytest.mark.parametrize("n", [1, 9, 360, 1926])      # one value, one residue, 24 + 16 residues, 7CEI (214 x 9)
def test_first_nonfinite(exe, n):
    """The scan behind the refusal of a non-finite stored pose (dfm_complex_create / dfm_complex_set_pose): the index of the FIRST NaN or
    infinity - either sign, quiet, signalling, any payload - and n for an array of numbers (the largest finite value and denormals
    included); the block has exactly n floats, so reading past it is a sanitizer report."""
    one = lambda *planted: int(exe("finite", n, *[f"{o}:{w:x}" for o, w in planted])[0])
    assert one() == n
    assert one((n - 1, 0x7F7FFFFF), (0, 0x00000001), (n // 2, 0x80000000), (n // 3, 0xFF7FFFFF)) == n
    for w in (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFBFFFFF, 0x7FFFFFFF, 0x7F800000, 0xFF800000):
        assert one((n - 1, w)) == n - 1 and one((0, w)) == 0 and one((n // 2, w)) == n // 2
        assert one((n - 1, w), (n // 2, 0x7FC00000)) == n // 2
