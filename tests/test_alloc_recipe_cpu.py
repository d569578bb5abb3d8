"""What tests/test_gpu_alloc_diag.py leans on, without a GPU: the comparer of tests/alloc_recipe.py against seeded mutants of a synthetic
result set, and the band scan of the diagnostic allocator (dfmdock_amd/csrc/dfm_guardscan.h) called from tests/guard_scan_main.cpp, built
by g++ with the address and undefined-behaviour sanitizers and run as a child process."""
import os
import subprocess

import numpy as np
import pytest

import alloc_recipe as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def result_set():
    rng = np.random.default_rng(3)
    nan = np.float32([1.0, np.nan, -np.inf, 0.0, -0.0])
    return {"score/f": rng.standard_normal((3, 16, 3)).astype(np.float32), "score/edges": rng.integers(0, 40, (3, 40, 20)).astype(np.int32),
            "score/nan": nan, "metrics/DockQ": rng.random(9), "consensus/bits": rng.integers(0, 1 << 62, (11, 9, 1)).astype(np.uint64),
            "scalar/M": np.asarray(11), "empty/center": np.zeros(0, np.int32), "__seconds": np.float64(1.5)}


def flip(a, index, bit):
    """a copy of `a` with one bit of element `index` (flat) flipped"""
    b = a.copy()
    v = b.reshape(-1).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    v[index] ^= v.dtype.type(1) << v.dtype.type(bit)
    return b


def mutants(base):
    nan2 = base["score/nan"].copy()
    nan2.view(np.uint32)[1] ^= np.uint32(1)      # still a NaN, another payload
    assert np.isnan(nan2[1]) and np.array_equal(nan2, base["score/nan"], equal_nan=True)
    off = base["score/edges"].copy()
    off[-1, -1, -1] += 1
    zero = base["score/nan"].copy()
    zero[3] = -0.0                                  # +0.0 -> -0.0: equal as numbers
    return {"mantissa bit": ("score/f", flip(base["score/f"], 77, 0)),
            "sign bit of the last element": ("score/f", flip(base["score/f"], base["score/f"].size - 1, 31)),
            "float64 mantissa bit": ("metrics/DockQ", flip(base["metrics/DockQ"], 4, 0)),
            "NaN payload": ("score/nan", nan2), "sign of zero": ("score/nan", zero),
            "shape": ("score/f", base["score/f"].reshape(3, 3, 16)), "dtype": ("score/edges", base["score/edges"].view(np.uint32)),
            "int32 off by one in the last element": ("score/edges", off), "uint64 top bit": ("consensus/bits", flip(base["consensus/bits"], 0, 63)),
            "scalar": ("scalar/M", np.asarray(12)), "empty against one element": ("empty/center", np.zeros(1, np.int32)),
            "scalar against [1]": ("scalar/M", np.asarray([11]))}


def test_comparer_accepts_a_copy_and_names_every_mutant():
    base = result_set()
    copy = {k: v.copy() for k, v in base.items()}
    copy["__seconds"] = np.float64(9.0)              # the child's own keys are not the recipe's
    assert ar.compare(base, copy) == [] and ar.compare(copy, base) == []
    fortran = dict(copy, **{"score/f": np.asfortranarray(base["score/f"])})      # the same values in another memory order
    assert ar.compare(base, fortran) == []
    for what, (key, value) in mutants(base).items():
        bad = dict(copy, **{key: value})
        assert ar.compare(base, bad) == [key] and ar.compare(bad, base) == [key], what
    missing = {k: v for k, v in copy.items() if k != "metrics/DockQ"}
    assert ar.compare(base, missing) == ["metrics/DockQ"] and ar.compare(missing, base) == ["metrics/DockQ"]
    extra = dict(copy, **{"zz/new": np.zeros(2)})
    assert ar.compare(base, extra) == ["zz/new"]
    # several differences come back in the recipe's order
    bad = dict(copy, **{"consensus/bits": flip(base["consensus/bits"], 5, 1), "score/f": flip(base["score/f"], 0, 22)})
    assert ar.compare(base, bad) == ["score/f", "consensus/bits"]


def test_results_keep_copies_under_unique_keys():
    r = ar.Results()
    a = np.arange(4, dtype=np.int32)
    r.put("call", {"x": a, "nested": {"y": 2.5}, "flag": True, "list": [1.0, 2.0]})
    a[0] = 9
    assert list(r) == ["call/x", "call/nested/y", "call/flag", "call/list"] and r["call/x"][0] == 0
    assert r["call/nested/y"].dtype == np.float64 and r["call/flag"].dtype == np.bool_
    with pytest.raises(AssertionError):
        r.put("call/x", a)
    with pytest.raises(AssertionError):
        r.put("__diag", a)
    with pytest.raises(AssertionError):
        r.put("obj", [None, 1])


def test_results_survive_the_npz_round_trip_in_order(tmp_path):
    base = result_set()
    np.savez(tmp_path / "r.npz", **base)
    back = dict(np.load(tmp_path / "r.npz", allow_pickle=False))
    assert list(back) == list(base) and ar.compare(base, back) == []


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("guard_scan") / "guard_scan")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1",
                           "-I", os.path.join(ROOT, "dfmdock_amd", "csrc"), os.path.join(ROOT, "tests", "guard_scan_main.cpp"), "-o", exe])

    def run(n, *damage):
        r = subprocess.run([exe, str(n)] + [f"{o}:{b}" for o, b in damage], capture_output=True, text=True)
        assert r.stderr == "" and r.returncode == 0, r.stderr      # a sanitizer report
        return int(r.stdout)
    return run


@pytest.mark.parametrize("n", [1, 7, 64, 65536])
def test_band_scan(scan, n):
    assert scan(n) == n                                           # intact
    assert scan(n, (0, 0)) == 0 and scan(n, (n - 1, 0xA4)) == n - 1 and scan(n, (n // 2, 0x5A)) == n // 2
    assert scan(n, (n - 1, 0), (n // 2, 255)) == n // 2         # the FIRST damaged byte
    assert scan(n, (n // 2, 0xA5)) == n                           # rewriting the guard byte itself is no damage


def test_band_of_no_bytes_is_intact(scan):
    assert scan(0) == 0
