"""The float64 definition of the density fit (dfmdock_amd/density.py), its MRC reader and writer, the closed-form correlation against
brute force, the host checks and bounds of dfm_poseprep.h (tests/density_prep_main.cpp under the address and undefined-behaviour
sanitizers) and the plumbing, on the CPU.  The GPU call is held against this definition in tests/test_gpu_density.py."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from cli_fixtures import golden_7cei, write_pair
from conftest import ROOT

Q = 2.0 ** 20
# correlation() against brute_force_correlation() on 7CEI, 33 poses, 8 A, 2 A voxels (test_closed_form_against_brute_force prints the
# figure of every run): the largest gap measured, at the native pose, and the gate at twice that.  The gap is the discretisation error of
# the definition - a trilinear gather from a 2 A grid of Gaussians of sigma 1.8 A flattens their peaks - not an error of any kernel.
MEASURED_MAX_GAP = 0.02784
GATE = 2.0 * MEASURED_MAX_GAP


# ---- MRC files --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2, 6, 12])
@pytest.mark.parametrize("big_endian", [False, True])
def test_mrc_round_trip(tmp_path, mode, big_endian):
    """Every supported mode in both byte orders, with mapc / mapr / maps straight and permuted, an extended header to skip, and the origin
    in words 50-52 or in nxstart / nystart / nzstart: the grid comes back [nz,ny,nx] value for value with its origin and voxel."""
    from dfmdock_amd import density as DN
    rng = np.random.default_rng(mode)
    grid = rng.integers(0, 100, (3, 5, 4)).astype(np.float32)      # exact in every mode, int8 and uint16 included
    voxel = np.float32([1.5, 2.0, 2.5])
    for order in ((1, 2, 3), (3, 1, 2), (2, 3, 1), (3, 2, 1)):
        for in_start, origin in ((False, np.float32([-7.25, 3.5, 11.0])), (True, np.float32([-3.0, 4.0, 10.0]))):
            path = str(tmp_path / f"m{mode}_{int(big_endian)}_{''.join(map(str, order))}_{int(in_start)}.mrc")
            DN.write_mrc(path, grid, origin, voxel, mode=mode, order=order, big_endian=big_endian, nsymbt=80 if order[0] == 3 else 0, origin_in_start=in_start)
            m = DN.read_mrc(path)
            assert m["grid"].dtype == np.float32 and m["grid"].shape == (3, 5, 4) and np.array_equal(m["grid"], grid), (order, in_start)
            assert np.array_equal(m["origin"], origin) and np.allclose(m["voxel"], voxel, rtol=1e-6, atol=0), (order, in_start)
            head = open(path, "rb").read(1024)
            assert head[208:212] == b"MAP " and struct.unpack((">" if big_endian else "<") + "i", head[12:16])[0] == mode


def test_mrc_refusals(tmp_path):
    from dfmdock_amd import density as DN
    grid = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    path = str(tmp_path / "ok.mrc")
    DN.write_mrc(path, grid, [0, 0, 0], [1, 1, 1])
    raw = bytearray(open(path, "rb").read())
    assert np.array_equal(DN.read_mrc(path)["grid"], grid)

    def variant(name, data):
        p = str(tmp_path / name)
        open(p, "wb").write(bytes(data))
        return p
    skew = bytearray(raw)
    skew[56:60] = struct.pack("<f", 100.0)      # beta
    with pytest.raises(ValueError, match="orthogonal"):
        DN.read_mrc(variant("skew.mrc", skew))
    with pytest.raises(ValueError, match="truncated"):
        DN.read_mrc(variant("short.mrc", raw[:-4]))
    with pytest.raises(ValueError, match="no MRC header"):
        DN.read_mrc(variant("tiny.mrc", raw[:500]))
    mode3 = bytearray(raw)
    mode3[12:16] = struct.pack("<i", 3)      # complex int16: not supported
    with pytest.raises(ValueError, match="mode"):
        DN.read_mrc(variant("mode3.mrc", mode3))
    axes = bytearray(raw)
    axes[64:68] = struct.pack("<i", 2)      # mapc = mapr = 2
    with pytest.raises(ValueError, match="permutation"):
        DN.read_mrc(variant("axes.mrc", axes))
    with pytest.raises(ValueError):
        DN.write_mrc(path, grid, [0.5, 0, 0], [1, 1, 1], origin_in_start=True)      # no whole number of voxels


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def test_interpolate_equals_hand_computed_values():
    from dfmdock_amd import density as DN
    g = np.arange(8, dtype=np.float32).reshape(2, 2, 2)      # g[z,y,x] = 4z + 2y + x
    o, v = np.float32([-1.0, 2.0, 0.5]), np.float32([2.0, 0.5, 4.0])
    centre = o.astype(np.float64) + 0.5 * v.astype(np.float64)
    val, inside = DN.interpolate(g, o, v, centre[None])
    assert inside.tolist() == [True] and val.shape == (1, 1) and val[0, 0] == 3.5      # the mean of the eight corners
    val, inside = DN.interpolate(g, o, v, o.astype(np.float64)[None])      # at a node: f = 0, the node's own value
    assert inside.tolist() == [True] and val[0, 0] == 0.0
    g3 = np.arange(27, dtype=np.float32).reshape(3, 3, 3)
    node = o.astype(np.float64) + v.astype(np.float64) * [1, 1, 1]
    val, inside = DN.interpolate(g3, o, v, node[None])
    assert inside.tolist() == [True] and val[0, 0] == 13.0
    quarter = o.astype(np.float64) + v.astype(np.float64) * [0.25, 0.5, 0.75]      # 4z + 2y + x is trilinear: the value is exact
    assert DN.interpolate(g, o, v, quarter[None])[0][0, 0] == 4 * 0.75 + 2 * 0.5 + 0.25
    # the last node of an axis is outside by the strict rule, on every axis; so is anything below the first, and a NaN
    last = o.astype(np.float64) + v.astype(np.float64)
    pts = np.array([[last[0], o[1], o[2]], [o[0], last[1], o[2]], [o[0], o[1], last[2]], [np.nextafter(o[0], -np.inf), o[1], o[2]], [np.nan, o[1], o[2]]])
    val, inside = DN.interpolate(g, o, v, pts)
    assert inside.tolist() == [False] * 5 and not val.any()
    # one ulp below the last node (origin 0 and voxel 1, so that ux is the coordinate itself) is inside, and the value is ux
    below = np.nextafter(1.0, 0.0)
    val, inside = DN.interpolate(g, [0, 0, 0], [1, 1, 1], [[below, 0.0, 0.0], [0.0, below, 0.0], [0.0, 0.0, below]])
    assert inside.all() and val[0].tolist() == [below, 2 * below, 4 * below]
    # two channels: each on its own
    val, _ = DN.interpolate(np.stack([g, -2 * g]), o, v, centre[None])
    assert val[:, 0].tolist() == [3.5, -7.0]


def test_the_definition_on_a_hand_case():
    from dfmdock_amd import density as DN
    g = np.arange(8, dtype=np.float32).reshape(2, 2, 2)
    o, v = np.float32([0, 0, 0]), np.float32([1, 1, 1])
    lig = np.float32([[0.5, 0.5, 0.5], [0.25, 0.0, 0.0], [5.0, 0.5, 0.5]])      # centre, on an edge, outside
    w = np.float32([2.0, -1.0, 3.0])
    rot, tr = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32)
    tr[1] = [0.25, 0.0, 0.0]
    rot[2, 0] = np.nan
    out = DN.density(np.stack([g, g * 0 + 1]), o, v, lig, w, [0, 0, 0], rot, tr, threshold=3.5, per_atom=True)
    assert out["sum_q"].dtype == np.int64 and out["n_inside"].dtype == np.int32 and out["atom_q"].shape == (3, 3)
    assert out["atom_q"][0].tolist() == [int(7 * Q), int(-0.25 * Q), 0] and out["sum_q"][0].tolist() == [int(6.75 * Q), int(1 * Q)]
    assert (out["n_inside"][0], out["n_above"][0]) == (2, 1)      # 3.5 >= 3.5 counts
    assert out["atom_q"][1].tolist() == [int(2 * 3.75 * Q), int(-0.5 * Q), 0] and out["n_above"][1] == 1
    assert not out["sum_q"][2].any() and not out["atom_q"][2].any() and out["n_inside"][2] == 0      # a pose that is not finite
    assert np.array_equal(DN.units(out["sum_q"][0]), [6.75, 1.0]) and DN.inclusion(out["n_above"], 3).tolist() == [1 / 3, 1 / 3, 0.0]
    assert DN.residue_density(out["atom_q"], np.array([0, 0, 1]), 2).tolist() == [[int(6.75 * Q), 0], [int(7.0 * Q), 0], [0, 0]]
    # ties to even at the quantum: w val 2^20 = 0.5 and 1.5
    half = DN.density(np.full((2, 2, 2), 2.0 ** -21, np.float32), o, v, np.float32([[0.5, 0.5, 0.5]] * 2), np.float32([1.0, 3.0]), [0, 0, 0], rot[:1], tr[:1], per_atom=True)
    assert half["atom_q"][0].tolist() == [0, 2]
    for bad in (dict(grids=np.zeros((5, 2, 2, 2))), dict(grids=np.zeros((1, 2, 2))), dict(grids=np.full((2, 2, 2), 1025.0)), dict(grids=np.full((2, 2, 2), np.nan)),
                dict(voxel=[1, 0, 1]), dict(voxel=[1, 17, 1]), dict(origin=[0, np.inf, 0]), dict(lig_w=[1, 2]), dict(lig_w=[1, 2, 129]), dict(threshold=np.nan)):
        kw = dict(dict(grids=g, origin=o, voxel=v, lig_atoms=lig, lig_w=w, center=[0, 0, 0], rot=rot, tr=tr), **bad)
        with pytest.raises(ValueError):
            DN.density(**kw)


# ---- the closed form --------------------------------------------------------------------------------------------------------------------
def native_map_7cei(work_dir, resolution=8.0, voxel=2.0, margin=10.0):
    """7CEI's two chains as cli.load_pair reads them, the driver's density inputs and the map of the native pose (the input pose) simulated
    at `resolution` on a `voxel` grid over the complex's box grown by `margin`; the map is also written to <work_dir>/native.mrc."""
    from dfmdock_amd import cli, driver
    from dfmdock_amd import density as DN
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(work_dir), cx, rs, ls)
    rec, lig, rec_x, lig_x = cli.load_pair(rec_pdb, lig_pdb, feat)
    ra, rw, la, lw, cen = driver.density_inputs(rec, lig, 0)
    both = np.concatenate([ra, la]).astype(np.float64)
    vox = np.float32([voxel] * 3)
    origin = np.floor(both.min(0) - margin).astype(np.float32)
    shape = tuple(int(n) + 1 for n in np.ceil((both.max(0) + margin - origin) / voxel)[::-1])
    sigma = resolution * DN.SIGMA_FACTOR
    grid = DN.simulate_map(both, np.concatenate([rw, lw]), sigma, shape, origin, vox).astype(np.float32)
    path = os.path.join(str(work_dir), "native.mrc")
    DN.write_mrc(path, grid, origin, vox)
    return dict(rec=rec, lig=lig, rec_x=rec_x, lig_x=lig_x, rec_pdb=rec_pdb, lig_pdb=lig_pdb, feat=feat, ra=ra, rw=rw, la=la, lw=lw, cen=cen,
                map={"grid": grid, "origin": origin, "voxel": vox}, path=path, resolution=resolution, sigma=sigma)


def perturbed_poses(P, seed=0):
    """Pose 0 is the identity; the others turn by 0.05 .. 0.5 rad about a seeded axis and move by 3 A per axis."""
    rng = np.random.default_rng(seed)
    rot, tr = np.zeros((P, 3), np.float32), np.zeros((P, 3), np.float32)
    for p in range(1, P):
        ax = rng.standard_normal(3)
        rot[p] = (ax / np.linalg.norm(ax) * rng.uniform(0.05, 0.5)).astype(np.float32)
        tr[p] = (3.0 * rng.standard_normal(3)).astype(np.float32)
    return rot, tr


def test_closed_form_against_brute_force(tmp_path):
    """The map of 7CEI's native pose at 8 A on a 2 A grid; the native and 32 perturbed poses.  correlation() - three gathers per atom and
    four scalars - against the correlation of each posed complex simulated on the grid: within GATE, and the native pose has the highest
    correlation of the 33 by both routes."""
    from dfmdock_amd import density as DN
    from dfmdock_amd import sterics as ST
    f = native_map_7cei(tmp_path)
    assert np.array_equal(DN.read_mrc(f["path"])["grid"], f["map"]["grid"]) and set(f["rw"].tolist()) <= {6.0, 7.0, 8.0, 16.0}
    grids, sc = DN.channels(f["map"], f["ra"], f["rw"], f["sigma"], f["la"], f["lw"])
    assert grids.shape == (3,) + f["map"]["grid"].shape and grids.dtype == np.float32 and abs(grids[0].mean()) < 1e-6 and abs(grids[0].std() - 1) < 1e-5
    assert set(sc) >= {"E2", "S_rr", "S_ll", "C_rE"} and "S_ll" not in DN.channels(f["map"], f["ra"], f["rw"], f["sigma"])[1]
    rot, tr = perturbed_poses(33)
    out = DN.density(grids, f["map"]["origin"], f["map"]["voxel"], f["la"], f["lw"], f["cen"], rot, tr)
    assert (out["n_inside"] == f["la"].shape[0]).all()      # the margin holds every pose: nothing is cut off
    cc = DN.correlation(out["sum_q"], sc)
    brute = np.array([DN.brute_force_correlation(f["map"], f["ra"], f["rw"], ST.pose_atoms(f["la"], f["cen"], rot[p], tr[p]), f["lw"], f["sigma"]) for p in range(33)])
    gap = np.abs(cc - brute)
    print(f"closed form vs brute force: max gap {gap.max():.5f} at pose {int(gap.argmax())}, mean {gap.mean():.5f}; gate {GATE:.5f}; "
          f"cc {cc.min():.4f} .. {cc.max():.4f}, brute {brute.min():.4f} .. {brute.max():.4f}")
    assert gap.max() <= GATE
    assert int(np.argmax(cc)) == 0 == int(np.argmax(brute)) and cc[0] - np.sort(cc)[-2] > GATE
    assert np.isnan(DN.correlation(np.zeros((1, 3), np.int64), dict(sc, S_rr=0.0, S_ll=0.0))).all()


# ---- dfm_poseprep.h under the sanitizers ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prep(tmp_path_factory):
    d = tmp_path_factory.mktemp("density_prep")
    exe = str(d / "density_prep")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1",
                           "-I", os.path.join(ROOT, "dfmdock_amd", "csrc"), os.path.join(ROOT, "tests", "density_prep_main.cpp"), "-o", exe])

    def parse(r):
        assert r.stderr == "", r.stderr      # a sanitizer report
        out = {"rc": r.returncode}
        for line in r.stdout.splitlines():
            k, _, v = line.partition(" ")
            out[k] = v
        return out
    n = [0]

    def run(shape, C, Al, origin, voxel, center, grids, atoms, w):
        n[0] += 1
        path = str(d / f"case{n[0]}.bin")
        arr = [None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1) for a in (grids, atoms, w)]
        with open(path, "wb") as f:
            f.write(np.int32([shape[2], shape[1], shape[0], C, Al] + [0 if a is None else a.size for a in arr]).tobytes())
            f.write(np.float32(list(origin) + list(voxel) + list(center)).tobytes())
            for a in arr:
                if a is not None:
                    f.write(a.tobytes())
        return parse(subprocess.run([exe, path], capture_output=True, text=True))
    run.cmd = lambda *a: parse(subprocess.run([exe] + [str(v) for v in a], capture_output=True, text=True))
    return run


def test_host_checks_and_layouts_under_the_sanitizers(prep):
    rng = np.random.default_rng(1)
    shape, Cn, Al = (3, 5, 4), 3, 7
    grids = rng.uniform(-4, 4, (Cn,) + shape).astype(np.float32)
    atoms, w = rng.uniform(-5, 5, (Al, 3)).astype(np.float32), rng.uniform(-8, 8, Al).astype(np.float32)
    base = dict(shape=shape, C=Cn, Al=Al, origin=[-1, 2, 3], voxel=[1, 2, 0.5], center=[0, 1, 2], grids=grids, atoms=atoms, w=w)
    ok = prep(**base)
    assert ok["rc"] == 0 and ok["bound"] == f"{Al * 2.0 ** 37:.17g} 1"
    g4 = np.array([float.fromhex(x) for x in ok["grid4"].split()], np.float32).reshape(shape + (4,))
    assert np.array_equal(g4[..., :3], grids.transpose(1, 2, 3, 0)) and not g4[..., 3].any()      # a node's channels side by side, zeros behind
    l4 = np.array([float.fromhex(x) for x in ok["lig4"].split()], np.float32).reshape(Al, 4)
    assert np.array_equal(l4[:, :3], atoms) and np.array_equal(l4[:, 3], w)

    def mod(a, k, v):
        b = np.array(a, copy=True)
        b[k] = v
        return b
    cases = [(dict(C=0), "need 1 <= C <= 4"), (dict(C=5), "need 1 <= C <= 4"), (dict(shape=(3, 5, 1)), "need 2 <= nx <= 1024"), (dict(shape=(3, 1025, 4)), "need 2 <= ny <= 1024"),
             (dict(shape=(1, 5, 4)), "need 2 <= nz <= 1024"), (dict(grids=None), "grids is NULL"), (dict(origin=[0, np.nan, 0]), "origin is not finite"),
             (dict(voxel=[1, 0, 1]), "voxel is not in (0, 16]"), (dict(voxel=[1, 1, 16.5]), "voxel is not in (0, 16]"), (dict(voxel=[np.inf, 1, 1]), "voxel is not in (0, 16]"),
             (dict(grids=mod(grids, (1, 0, 0, 2), np.nan)), "grids: value 62 is not in [-1024, 1024]"), (dict(grids=mod(grids, (0, 0, 0, 1), 1024.5)), "grids: value 1 is not"),
             (dict(atoms=None), "lig_atoms is NULL"), (dict(w=None), "lig_w is NULL"), (dict(Al=0), "need Al >= 1"), (dict(Al=(1 << 24) + 1), "Al exceeds 2^24 atoms"),
             (dict(atoms=mod(atoms, (3, 1), np.inf)), "lig_atoms: atom 3 is not finite"), (dict(w=mod(w, 4, 128.5)), "lig_w: weight 4 is not in [-128, 128]"),
             (dict(w=mod(w, 0, np.nan)), "lig_w: weight 0 is not"), (dict(center=[0, 0, np.inf]), "center is not finite")]
    for kw, word in cases:
        r = prep(**dict(base, **kw))
        assert r["rc"] == 2 and word in r["error"], (word, r)
    # the order: the grid before the atoms
    assert "need 1 <= C" in prep(**dict(base, C=9, atoms=None))["error"] and "voxel" in prep(**dict(base, voxel=[0, 1, 1], w=None))["error"]
    assert prep(**dict(base, grids=mod(mod(grids, (0, 0, 0, 0), 1024.0), (2, 2, 4, 3), -1024.0), w=mod(w, 0, -128.0), voxel=[16, 16, 16]))["rc"] == 0      # the limits themselves
    # the bound: Al 2^37 quanta, refused from 2^62 on - 2^25 atoms, above the 2^24 the creator takes
    assert prep.cmd("bound", 1)["bound"] == f"{2.0 ** 37:.17g} 1" and prep.cmd("bound", (1 << 25) - 1)["bound"].endswith(" 1")
    assert prep.cmd("bound", 1 << 25)["bound"] == f"{2.0 ** 62:.17g} 0"
    chunk = lambda *a: int(prep.cmd("chunk", *a)["chunk"])
    assert chunk(2400, 0) == 32768 and chunk(2400, 1) == (64 << 20) // (2400 * 8) and chunk(1 << 24, 1) == 1 and chunk(1, 1) == 32768


def test_struct_layout_and_exports(tmp_path):
    """dfm_density_out as gcc lays it out against the ctypes mirror; the new symbols are exported and listed; argument checks run before
    any device work."""
    from dfmdock_amd import _lib
    c_name, cls = "dfm_density_out", _lib.DensityOutC
    body = f'printf("{c_name} %zu\\n", sizeof({c_name}));' + "".join(f'printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));' for f, _ in cls._fields_)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dfmdock_amd.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(got[c_name]) == C.sizeof(cls) == 32 and [f for f, _ in cls._fields_] == ["sum_q", "n_inside", "n_above", "atom_q"]
    for f, _ in cls._fields_:
        assert int(got[f"{c_name}.{f}"]) == getattr(cls, f).offset, f
    lib = _lib.lib()
    for s in ("dfm_density_create", "dfm_density_destroy", "dfm_density_info", "dfm_pose_density", "dfm_pose_density_chunked", "dfm_density_last_timing"):
        assert s in _lib.EXPORTS and hasattr(lib, s) and (getattr(lib, s).argtypes or s == "dfm_density_destroy")
    from test_abi_cpu import header_symbols
    assert sorted(_lib.EXPORTS) == header_symbols()
    err = C.c_int(7)
    assert lib.dfm_density_create(None, 2, 2, 2, None, None, 1, None, 1, None, None, None, 1.0, C.byref(err)) is None
    assert b"m is NULL" in lib.dfm_last_error() and err.value == -1
    assert lib.dfm_pose_density(None, 1, None, None, None) == -1 and b"h is NULL" in lib.dfm_last_error()
    assert lib.dfm_density_last_timing(None, None) == -1 and lib.dfm_density_info(None, None, None, None, None, None, None) == -1


def test_the_audits_see_both_instantiations():
    """k_density_pose and both instantiations of k_density are in the shipped gfx950 code object (so the scratch / LDS / op_sel audits of
    test_abi_cpu.py run over them), use no scratch, and k_density holds the grid's geometry - 16 doubles - in static LDS."""
    import shutil
    import tempfile
    from dfmdock_amd import _lib
    tools = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(tools, "llvm-readelf")):
        pytest.skip("llvm-readelf not available")
    src = open(os.path.join(ROOT, "dfmdock_amd", "csrc", "kernels_density.hip")).read()
    assert set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)) == {"k_density_pose", "k_density"}
    assert "atomicAdd(o" in src and not re.search(r"atomicAdd\([^;]*\((float|double)\)", src)      # integer atomics only
    mk = open(os.path.join(ROOT, "dfmdock_amd", "csrc", "Makefile")).read()
    assert re.search(r"kernels_density\.o: kernels_density\.hip \$\(HDRS\)\n\t\$\(HIPCC\) \$\(COMMON\) \$\(STRICT\)", mk)      # nothing contracted
    td = tempfile.mkdtemp()
    try:
        lib = os.path.join(td, "lib.so")
        shutil.copy(_lib.LIB_PATH, lib)
        subprocess.run([os.path.join(tools, "llvm-objdump"), "--offloading", lib], cwd=td, check=True, capture_output=True)
        found = {}
        for f in sorted(os.listdir(td)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([os.path.join(tools, "llvm-readelf"), "--notes", os.path.join(td, f)], capture_output=True, text=True).stdout
            for blk in notes.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                for n, pat in (("k_density_pose", r"\d+k_density_poseE"), ("k_density<true>", r"\d+k_densityILb1EE"), ("k_density<false>", r"\d+k_densityILb0EE")):
                    if re.search(pat, name):
                        found[n] = tuple(int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in ("private_segment_fixed_size", "group_segment_fixed_size"))
        assert found == {"k_density_pose": (0, 0), "k_density<true>": (0, 128), "k_density<false>": (0, 128)}, found
    finally:
        shutil.rmtree(td, ignore_errors=True)


# ---- drivers and command line -----------------------------------------------------------------------------------------------------------
def stub_density(cc, Al=626):
    """What driver.ensemble_density returns, made up from a column of correlations."""
    cc = np.asarray(cc, np.float64)
    n = cc.size
    return {"sum_q": np.zeros((n, 3), np.int64), "n_inside": np.full(n, Al, np.int32) - np.arange(n, dtype=np.int32), "n_above": np.arange(100, 100 + n, dtype=np.int32),
            "cc": cc, "neg_cc": -cc, "inclusion": np.arange(100, 100 + n) / Al, "n_outside": np.arange(n, dtype=np.int64), "Al": Al, "scalars": {},
            "resolution": 8.0, "sigma": 1.8, "threshold": 1.0}


def test_driver_inputs_and_selection_helpers(tmp_path):
    from dfmdock_amd import driver
    from dfmdock_amd import density as DN
    from dfmdock_amd import sterics as ST
    f = native_map_7cei(tmp_path)
    sa = driver.sterics_inputs(f["rec"], f["lig"], 0)
    assert np.array_equal(f["ra"], sa[0]) and np.array_equal(f["la"], sa[1]) and np.array_equal(f["cen"], sa[2])
    heavy = ST.heavy_atoms(f["lig"]["atoms"])
    assert f["lw"].dtype == np.float32 and f["lw"].shape == heavy.shape and [f["lw"][i] for i in range(4)] == [7.0, 6.0, 6.0, 8.0]      # N CA C O
    assert DN.atom_weights([{"name": " SG ", "element": "S", "res_name": "CYS"}, {"name": "ZN  ", "element": "ZN", "res_name": "ZN"}], [0, 1]).tolist() == [16.0, 6.0]
    assert driver._check_density(None, None, 1.0, None, "energy") is None
    for kw in (dict(rank="density"), dict(min_density_cc=0.5)):
        with pytest.raises(ValueError):
            driver._check_density(**dict(dict(density_map=None, density_resolution=None, density_threshold=1.0, min_density_cc=None, rank="energy"), **kw))
    by, dmap, res, thr, mcc = driver._check_density(f["path"], 8.0, 1.0, None, "density")
    assert by is True and np.array_equal(dmap["grid"], f["map"]["grid"]) and (res, thr, mcc) == (8.0, 1.0, None)
    assert driver._check_density(f["map"], 8, 0.5, 0.3, "energy")[0] is False and driver._check_density(f["map"], 8, 0.5, 0.3, "energy")[4] == 0.3
    for bad in (dict(density_resolution=None), dict(density_resolution=0.0), dict(density_resolution=np.inf), dict(density_threshold=np.nan), dict(min_density_cc=np.nan),
                dict(density_map=dict(f["map"], voxel=[0, 1, 1])), dict(density_map=dict(f["map"], grid=np.zeros((1, 4, 4)))),
                dict(density_map=dict(f["map"], grid=np.full((2, 2, 2), np.nan)))):
        with pytest.raises(ValueError):
            driver._check_density(**dict(dict(density_map=f["map"], density_resolution=8.0, density_threshold=1.0, min_density_cc=None, rank="energy"), **bad))
    driver._check_rank("density", 1.0)
    with pytest.raises(ValueError, match="'density'"):
        driver._check_rank("map", 1.0)
    dd = stub_density([0.25, np.nan, 0.75])
    assert driver._pose_density(dd, 2) == {"density_cc": 0.75, "density_inclusion": 102 / 626, "density_n_outside": 2}
    assert driver._pose_density(dd, 1)["density_cc"] is None
    json.dumps(driver._pose_density(dd, 0))
    names = [a.name for a in driver.ANALYSES]
    assert "density" in names and names.index("pairpot") < names.index("density") < names.index("consensus")
    off = driver._Run(None, type("G", (), {"lig_pos0": None}), None, None, None, "fp32", {"density": None})      # off: no stage of _finish runs it
    off.k = 3
    [a.run(off) for a in driver.ANALYSES if a.name in off.opts]
    assert (off.k, off.key, off.data) == (3, None, {}) and not off.any()


def test_every_summary_describes_the_kept_pose(tmp_path, monkeypatch):
    """_finish with the engine stubbed: under rank "density" the `density` object, `index` and the returned transform belong to the pose
    of the HIGHEST correlation (ties: the lower index; a NaN never wins); without the rank the energy's pick is described; off: no key."""
    from dfmdock_amd import cli, driver
    cx, rs, ls = golden_7cei()
    rec_pdb, lig_pdb, feat = write_pair(str(tmp_path), cx, rs, ls)
    rec, lig, _, _ = cli.load_pair(rec_pdb, lig_pdb, feat)
    n = 5
    energy = np.float32([-5.0, -1.0, -2.0, -3.0, -4.0])      # energy keeps 0
    cc = np.array([0.2, np.nan, 0.9, 0.1, 0.9])              # density keeps 2 (the tie with 4 goes to the lower index)
    cols = {"energy": energy, "rot_update": 0.01 * np.arange(3 * n, dtype=np.float32).reshape(n, 3), "tr_update": np.arange(3 * n, dtype=np.float32).reshape(n, 3)}
    seen = []
    monkeypatch.setattr(driver, "ensemble_density", lambda model, rec, lig, rot, tr, dmap, res, thr, per_atom=False: seen.append((res, thr)) or stub_density(cc))

    class Gx:
        lig_pos0 = np.asarray(lig["bb_coords"], np.float32)

        def close(self):
            pass

    class Hp:
        family = 0
    model = type("M", (), {"hp": Hp})()
    dmap = {"grid": np.zeros((4, 4, 4), np.float32), "origin": np.zeros(3, np.float32), "voxel": np.ones(3, np.float32)}

    def finish(rank, on, bad=None):
        opts = driver._check_density(dmap if on else None, 8.0 if on else None, 1.5, None, rank)
        if bad is not None:
            monkeypatch.setattr(driver, "_screen", lambda *a: ({"flags": bad, "n_clash": np.zeros(n, int), "n_contact": np.ones(n, int), "min_dist": np.ones(n),
                                                              "threshold": 1.0, "ensemble_mean": 0.0, "ensemble_std": 0.0, "clash_cutoff": 3.0,
                                                              "contact_cutoff": 5.0, "filtered": True, "fallback": False}, bad))
        run = driver._Run(model, Gx(), rec, lig, cols, "fp32", dict(density=opts, sterics=(True, 3.0, 5.0) if bad is not None else None))
        run.key = energy
        return driver._finish(run, (np.argmin, "energy"), lambda k: {}), run
    r, run = finish("density", True)
    assert r["index"] == 2 and np.array_equal(r["rot_update"], cols["rot_update"][2]) and r["energy"] == -2.0 and seen[-1] == (8.0, 1.5)
    assert r["density"] == {"density_cc": 0.9, "density_inclusion": 102 / 626, "density_n_outside": 2, "rank": 1, "resolution": 8.0, "sigma": 1.8, "threshold": 1.0,
                            "ranked_by_density": True}
    assert r["density_data"]["cc"][r["index"]] == r["density"]["density_cc"] and np.array_equal(r["density_data"]["rot_update"], cols["rot_update"])
    assert run.ranked_by == "density" and np.array_equal(run.key, -cc, equal_nan=True) and set(r["trajectories"]) >= {"energy", "rot_update", "tr_update"}
    r, run = finish("energy", True)
    assert r["index"] == 0 and r["density"]["density_cc"] == 0.2 and r["density"]["rank"] == 3 and not r["density"]["ranked_by_density"] and run.ranked_by == "energy"
    r, _ = finish("energy", False)
    assert "density" not in r and "density_data" not in r and "index" not in r
    # the clash filter removes the density pick: the other pose of the tie is kept
    r, _ = finish("density", True, np.array([False, False, True, False, False]))
    assert r["index"] == 4 and r["density"]["density_cc"] == 0.9 and r["density"]["rank"] == 1 and r["density"]["density_n_outside"] == 4


def test_cli_flags_parse_default_off_and_reach_the_driver(tmp_path, monkeypatch, capsys):
    from dfmdock_amd import cli, driver
    from dfmdock_amd import density as DN
    f = native_map_7cei(tmp_path)
    base = ["r.pdb", "l.pdb", "--ckpt", "c.ckpt", "--features", "f.npz"]
    poses = str(tmp_path / "p.npz")
    np.savez(poses, rot_update=np.zeros((2, 3), np.float32), tr_update=np.zeros((2, 3), np.float32))
    for cmd, extra in (("dock", []), ("refine", []), ("rescore", ["--poses", poses])):
        a = cli.parse_args([cmd] + base + extra)
        assert a.density is None and a.rank == "energy" and a.density_residues is None and cli.density_kwargs(a) == {}
        a = cli.parse_args([cmd] + base + extra + ["--density", f["path"], "--density-resolution", "8"])
        kw = cli.density_kwargs(a)
        assert set(kw) == {"density_map", "density_resolution", "density_threshold", "rank"} and kw["rank"] == "energy" and kw["density_threshold"] == 1.0
        assert np.array_equal(kw["density_map"]["grid"], f["map"]["grid"]) and kw["density_resolution"] == 8.0
        a = cli.parse_args([cmd] + base + extra + ["--density", f["path"], "--density-resolution", "8", "--rank", "density", "--density-threshold", "0.5",
                                                   "--density-residues", "r.txt", "--write-simulated-map", "s.mrc"])
        assert cli.density_kwargs(a)["rank"] == "density" and cli.density_kwargs(a)["density_threshold"] == 0.5 and not a.consensus and a.pair_potential is None
        for bad in (["--rank", "density"], ["--density-resolution", "8"], ["--density-residues", "r.txt"], ["--write-simulated-map", "s.mrc"], ["--density-threshold", "1"],
                    ["--density", f["path"]], ["--density", f["path"], "--density-resolution", "0"], ["--density", str(tmp_path / "none.mrc"), "--density-resolution", "8"],
                    ["--density", f["path"], "--density-resolution", "8", "--min-density-cc", "0.5"]):      # the last: no --top-k (refine has none at all)
            with pytest.raises(SystemExit):
                cli.parse_args([cmd] + base + extra + bad)
        if cmd != "refine":
            assert cli.density_kwargs(cli.parse_args([cmd] + base + extra + ["--density", f["path"], "--density-resolution", "8", "--min-density-cc", "0.5", "--top-k", "2"])) \
                ["min_density_cc"] == 0.5
        with pytest.raises(SystemExit) as e:
            cli.parse_args([cmd, "--help"])
        assert e.value.code == 0
        text = capsys.readouterr().out
        assert all(flag in text for flag in ("--density MAP.mrc", "--density-resolution", "--density-threshold", "--min-density-cc", "--density-residues", "--write-simulated-map"))
    with pytest.raises(SystemExit):
        cli.parse_args(["sweep", "--db5", "d", "--ckpt", "c", "--density", f["path"]])      # sweep is left alone: the DB5 files hold backbones only
    seen = {}

    class Hp:
        lm_embed_dim, family = 1301, 0
    fake_model = type("M", (), {"hp": Hp})()
    monkeypatch.setattr(cli, "load_model", lambda args: (fake_model, Hp))
    obj = {"density_cc": 0.875, "density_inclusion": 0.5, "density_n_outside": 3, "rank": 1, "resolution": 8.0, "sigma": f["sigma"], "threshold": 1.0, "ranked_by_density": True}
    figures = {k: obj[k] for k in ("density_cc", "density_inclusion", "density_n_outside")}
    tj = {"energy": np.zeros(6, np.float32), "rot_update": 0.1 * np.arange(18, dtype=np.float32).reshape(6, 3), "tr_update": np.arange(18, dtype=np.float32).reshape(6, 3)}

    def dock_pair(model, rec, lig, rec_x, lig_x, **kw):
        seen.update(kw)
        res = {"energy": -1.5, "precision": "mfma16", "rot_update": tj["rot_update"][4], "tr_update": tj["tr_update"][4], "selfcheck": None,
               "lig_aa_coords": np.asarray(lig["aa_coords"], np.float64)}
        if kw.get("density_map") is not None:
            res.update(density=obj, index=4, trajectories={"energy": tj["energy"]}, density_data=tj)
        if kw.get("top_k"):
            res.update(models=[dict({"rank": 1, "index": 4, "energy": 0.0, "cluster_size": 3}, **figures),
                               dict({"rank": 2, "index": 2, "energy": 0.0, "cluster_size": 2}, **dict(figures, density_cc=0.5))], cluster_of=np.zeros(6, int))
        return res

    def residue_density(model, rec, lig, rot, tr, dmap, resolution, threshold=1.0):
        seen["residue_call"] = (np.asarray(rot).tolist(), resolution, threshold)
        keys = [tuple(k) for k in lig["residues"]]
        return keys, np.arange(len(keys)) * 0.25
    monkeypatch.setattr(driver, "dock_pair", dock_pair)
    monkeypatch.setattr(driver, "residue_density", residue_density)
    args = ["dock", f["rec_pdb"], f["lig_pdb"], "--ckpt", "c.ckpt", "--features", f["feat"], "--out", str(tmp_path / "o.pdb")]
    assert cli.main(args) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "density" not in plain and "index" not in plain and not any(k.startswith(("density", "rank", "min_density")) for k in seen)
    seen.clear()
    assert cli.main(args + ["--density", f["path"], "--density-resolution", "8", "--rank", "density", "--top-k", "2", "--density-residues", str(tmp_path / "res.txt"),
                            "--write-simulated-map", str(tmp_path / "sim.mrc")]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert seen["rank"] == "density" and seen["density_resolution"] == 8.0 and seen["density_threshold"] == 1.0 and "min_density_cc" not in seen and "pair_potential" not in seen
    assert line["density"] == obj and line["index"] == 4 and [m["density_cc"] for m in line["models"]] == [0.875, 0.5]
    assert {k: v for k, v in line.items() if k in plain and k not in ("rot_update", "tr_update")} == {k: v for k, v in plain.items() if k not in ("rot_update", "tr_update")}
    # the kept pose first, then the models in their order
    assert seen["residue_call"] == (tj["rot_update"][[4, 4, 2]].tolist(), 8.0, 1.0)
    assert os.path.samefile(line["density_residues"], tmp_path / "res.txt") and os.path.samefile(line["simulated_map"], tmp_path / "sim.mrc")
    rows = (tmp_path / "res.txt").read_text().splitlines()
    k = f["lig"]["residues"][2]
    assert rows[0].startswith("#") and len(rows) == 1 + len(f["lig"]["residues"]) and rows[3] == f"{k[0]}:{k[1]} {k[3]} 0.500000"
    # the stub leaves the ligand where it is: the written map is the native complex on the map's grid, i.e. the map itself
    sim = DN.read_mrc(str(tmp_path / "sim.mrc"))
    assert np.array_equal(sim["origin"], f["map"]["origin"]) and np.array_equal(sim["voxel"], f["map"]["voxel"])
    np.testing.assert_allclose(sim["grid"], f["map"]["grid"], rtol=1e-5, atol=1e-7)
