"""The host preparation of the per-pose all-atom calls (dfmdock_amd/csrc/dfm_poseprep.h: the receptor's cell grid, the ligand in blocks of 64
neighbours) without a GPU: tests/pose_prep_main.cpp, built by g++ with the address and undefined-behaviour sanitizers, is run as a child
process on hand-built shapes and its output is held against numpy.  Every condition is an integer equality, an equality of float64 values
that both sides compute with the same IEEE operations, or a containment that must hold outright.  tests/pose_frame_main.cpp does the
same for build_pose_frame, the frame that the four cutoff-based creators share: its fp32 threshold, reject2 and slack are recomputed in
float32, its grid, corners and the ligand's low corner in float64, and all of them are compared for equality."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE = 5.0


@pytest.fixture(scope="module")
def prep(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_prep")
    exe = str(d / "pose_prep")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1",
                           "-I", os.path.join(ROOT, "dfmdock_amd", "csrc"), os.path.join(ROOT, "tests", "pose_prep_main.cpp"), "-o", exe])

    def run(rec, lig, center, edge=EDGE):
        path = str(d / "atoms.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<iid", rec.shape[0], lig.shape[0], edge))
            for a in (center, rec, lig):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.stderr == "", r.stderr      # a sanitizer report
        return r.returncode, {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    return run


@pytest.fixture(scope="module")
def frame(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_frame")
    exe = str(d / "pose_frame")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1",
                           "-I", os.path.join(ROOT, "dfmdock_amd", "csrc"), os.path.join(ROOT, "tests", "pose_frame_main.cpp"), "-o", exe])

    def run(rec, lig, center, reach, name="cutoff"):
        path = str(d / "atoms.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<iif", rec.shape[0], lig.shape[0], reach))
            for a in (center, rec, lig):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
        r = subprocess.run([exe, path, name], capture_output=True, text=True)
        assert r.stderr == "", r.stderr      # a sanitizer report
        return r.returncode, {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    return run


def receptor(kind):
    rng = np.random.default_rng(11)
    if kind == "one":
        return np.float32([[-3.25, 7.5, 120.125]])
    if kind == "cell":       # 150 atoms in one cell: the box is narrower than the edge
        return (np.float32([-40.0, 2.0, 9.0]) + rng.uniform(0.0, 0.9 * EDGE, (150, 3))).astype(np.float32)
    x = -30.0 + 0.37 * np.arange(400)      # 400 atoms on a line along x, in shuffled order: 30 cells, ny = nz = 1
    return np.stack([rng.permutation(x), np.full(400, 4.0), np.full(400, -2.5)], 1).astype(np.float32)


def ligand(n):
    return (np.float32([12.0, -7.0, 3.0]) + 8.0 * np.random.default_rng(n).standard_normal((n, 3))).astype(np.float32)


def cells(x, lo, n, edge=EDGE):
    """cell_of of dfm_walkgrid.h, per axis, in float64"""
    return np.clip(np.floor((x.astype(np.float64) - lo) / edge), 0.0, np.asarray(n, np.float64) - 1.0).astype(np.int64)


def morton(c):
    code = np.zeros(c.shape[0], np.uint64)
    for b in range(21):
        for k in range(3):
            code |= ((c[:, k].astype(np.uint64) >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + k)
    return code


@pytest.mark.parametrize("Al", [1, 64, 65, 130])
@pytest.mark.parametrize("kind", ["one", "cell", "line"])
def test_grid_and_ligand_blocks_against_numpy(prep, kind, Al):
    rec, lig = receptor(kind), ligand(Al)
    center = lig.astype(np.float64).mean(0).astype(np.float32)
    rc, out = prep(rec, lig, center)
    assert rc == 0, out
    f64 = lambda k: np.array([float(v) for v in out[k]], np.float64)
    i64 = lambda k: np.array([int(v) for v in out[k]], np.int64)
    # the receptor's grid: box, dims, the prefix sum of the per-cell counts, the stable sort by cell
    lo, hi = rec.astype(np.float64).min(0), rec.astype(np.float64).max(0)
    dims = (np.floor((hi - lo) / EDGE) + 1.0).astype(np.int64)
    assert np.array_equal(f64("lo"), lo) and np.array_equal(f64("hi"), hi) and np.array_equal(i64("dims")[:3], dims)
    assert {"one": (1, 1, 1), "cell": (1, 1, 1), "line": (30, 1, 1)}[kind] == tuple(dims)
    c = cells(rec, lo, dims)
    cell = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    counts = np.bincount(cell, minlength=int(dims.prod()))
    assert np.array_equal(i64("cell_start"), np.concatenate([[0], np.cumsum(counts)])) and i64("dims")[3] == counts.max()
    assert np.array_equal(i64("order"), np.argsort(cell, kind="stable"))
    # the ligand: a permutation in non-decreasing Morton code of its own cells, ties in the caller's order
    llo = lig.astype(np.float64).min(0)
    assert np.array_equal(f64("lig_lo"), llo)
    index, code = i64("lig_index"), morton(cells(lig, llo, [1 << 21] * 3))
    assert np.array_equal(np.sort(index), np.arange(Al)) and (np.diff(code[index].astype(np.int64)) >= 0).all()
    assert np.array_equal(index, np.argsort(code, kind="stable"))
    # every sphere, about the fp32 centre the kernel reads, holds its block's atoms in float64
    sph = np.array([float(v) for v in out["sphere"]], np.float32).astype(np.float64).reshape(-1, 4)      # (9 digits give the fp32 back)
    assert sph.shape[0] == (Al + 63) // 64 and np.isfinite(sph).all() and out["finite"] == ["1"]
    q = lig.astype(np.float64)[index] - center.astype(np.float64)
    for b in range(sph.shape[0]):
        d = np.sqrt(((q[64 * b:64 * b + 64] - sph[b, :3]) ** 2).sum(1))
        assert (d <= sph[b, 3]).all(), (b, d.max(), sph[b, 3])
    # slack = max(1e-3, 2.5e-7 maxabs) in fp32
    want = [max(np.float32(1e-3), np.float32(2.5e-7 * m)) for m in (hi[0], 1e5)]
    assert np.array_equal(np.array([float(v) for v in out["slack"]], np.float32), np.float32(want)) and want[1] == np.float32(0.025)


def test_argument_checks_name_the_argument(prep):
    rec, lig, cen = receptor("cell"), ligand(65), np.zeros(3, np.float32)
    bad = rec.copy()
    bad[7, 1] = np.nan
    assert prep(bad, lig, cen) == (2, {"error": "rec_atoms: atom 7 is not finite".split()})
    bad = lig.copy()
    bad[64, 2] = np.inf
    assert prep(rec, bad, cen) == (2, {"error": "lig_atoms: atom 64 is not finite".split()})
    assert prep(rec, lig, np.float32([0, np.inf, 0])) == (2, {"error": "center is not finite".split()})
    assert prep(rec[:0], lig, cen) == (2, {"error": "need Ar >= 1 and Al >= 1".split()})
    wide = rec.copy()
    wide[0, 0] = 2000.0      # 400^3 cells of 5 A > 2^24
    wide[1, 1] = 2000.0
    wide[2, 2] = 2000.0
    assert prep(wide, lig, cen) == (3, {"error": ["cells"]})


def frame_numbers(rec, reach):
    """slack, thr and reject2 as build_pose_frame forms them: maxabs in float64, the rest in float32, one rounding per operation"""
    r64 = rec.astype(np.float64)
    maxabs = max(np.abs(r64.min(0)).max(), np.abs(r64.max(0)).max()) + 2.0 * float(np.float32(reach)) + 1.0
    slack = max(np.float32(1e-3), np.float32(2.5e-7 * maxabs))
    thr = np.float32(np.float32(reach) * np.float32(1.0001)) + slack
    return slack, thr, np.float32(thr * thr)


@pytest.mark.parametrize("reach", [3.5, 5.0, 8.0])
@pytest.mark.parametrize("Al", [1, 65])
@pytest.mark.parametrize("kind", ["one", "cell", "line"])
def test_pose_frame_against_numpy(frame, kind, Al, reach):
    rec, lig = receptor(kind), ligand(Al)
    center = lig.astype(np.float64).mean(0).astype(np.float32)
    rc, out = frame(rec, lig, center, reach)
    assert rc == 0, out
    f64 = lambda k: np.array([float(v) for v in out[k]], np.float64)
    f32 = lambda k: np.array([float(v) for v in out[k]], np.float32)      # (9 digits give the fp32 back)
    i64 = lambda k: np.array([int(v) for v in out[k]], np.int64)
    # the receptor's grid of cells of the reach, as the kernels take it
    lo, hi = rec.astype(np.float64).min(0), rec.astype(np.float64).max(0)
    dims = (np.floor((hi - lo) / reach) + 1.0).astype(np.int64)
    assert np.array_equal(f64("lo"), lo) and np.array_equal(f64("hi"), hi) and np.array_equal(i64("dims")[:3], dims)
    assert np.array_equal(f64("center"), center.astype(np.float64))
    c = cells(rec, lo, dims, reach)
    cell = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    counts = np.bincount(cell, minlength=int(dims.prod()))
    assert np.array_equal(i64("cell_start"), np.concatenate([[0], np.cumsum(counts)])) and i64("dims")[3] == counts.max()
    assert np.array_equal(i64("order"), np.argsort(cell, kind="stable"))
    # the fp32 reject threshold: edge = the reach, grow = thr = reach * 1.0001 + slack, reject2 = thr^2
    slack, thr, reject2 = frame_numbers(rec, reach)
    assert np.array_equal(f32("thr_reject2"), np.float32([thr, reject2]))
    assert np.array_equal(f64("edge_grow"), np.float64([np.float32(reach), thr]))
    if kind == "one" and reach == 5.0:      # the floor of the slack applies
        assert slack == np.float32(1e-3) and thr == np.float32(5.00150013) and reject2 == np.float32(25.0150032)
    # the ligand: its low corner, Morton order of its own cells of the reach, every sphere about the fp32 centre holds its block
    llo = lig.astype(np.float64).min(0)
    assert np.array_equal(f64("lig_lo"), llo)
    index, code = i64("lig_index"), morton(cells(lig, llo, [1 << 21] * 3, reach))
    assert np.array_equal(index, np.argsort(code, kind="stable"))
    sph = f32("sphere").astype(np.float64).reshape(-1, 4)
    assert sph.shape[0] == (Al + 63) // 64 and np.isfinite(sph).all() and out["finite"] == ["1"]
    q = lig.astype(np.float64)[index] - center.astype(np.float64)
    for b in range(sph.shape[0]):
        d = np.sqrt(((q[64 * b:64 * b + 64] - sph[b, :3]) ** 2).sum(1))
        assert (d <= sph[b, 3]).all(), (b, d.max(), sph[b, 3])


def test_pose_frame_slack_grows_with_the_coordinates(frame):
    """A receptor atom 20000 A out: maxabs = 20008, so 2.5e-7 maxabs exceeds the floor of 1e-3."""
    rec, lig = np.float32([[20000.0, -3.0, 1.0]]), ligand(65)
    rc, out = frame(rec, lig, np.zeros(3, np.float32), 3.5)
    assert rc == 0, out
    slack, thr, reject2 = frame_numbers(rec, 3.5)
    assert slack == np.float32(0.0050019999) and thr == np.float32(3.50535202)
    assert np.array_equal(np.array([float(v) for v in out["thr_reject2"]], np.float32), np.float32([thr, reject2]))
    assert [float(v) for v in out["edge_grow"]] == [3.5, float(thr)]


def test_pose_frame_refusals(frame):
    rec, lig, cen = receptor("cell"), ligand(65), np.zeros(3, np.float32)
    wide = rec.copy()
    wide[0, 0] = 2000.0      # 400^3 cells of 5 A > 2^24
    wide[1, 1] = 2000.0
    wide[2, 2] = 2000.0
    for name in ("contact cutoff", "cutoff", "larger cutoff"):
        rc, out = frame(wide, lig, cen, 5.0, name)
        assert rc == 3 and " ".join(out["error"]) == "the receptor's bounding box needs more than 2^24 cells of the " + name
    # one ligand atom at 3e38 about a centre at -3e38: every input is finite, the block's centre relative to the rotation centre is not
    rc, out = frame(receptor("one"), np.float32([[3e38, 0.0, 0.0]]), np.float32([-3e38, 0.0, 0.0]), 5.0)
    assert rc == 3 and " ".join(out["error"]) == "lig_atoms / center: the ligand's extent about the centre overflows fp32"
    assert out["finite"] == ["0"]
