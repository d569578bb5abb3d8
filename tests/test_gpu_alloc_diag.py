"""Every public call under the allocator's poison fills and guard bands (DFM_ALLOC_POISON, DFM_ALLOC_GUARD: dfmdock_amd/csrc/dfm_host.h).

By default DevPool::alloc rounds a request up to 64 KiB granules and hands out blocks that destroyed handles parked, with their old
contents: a write a few elements past a buffer, or a read of memory that no launch of the call wrote, changes nothing that a whole-call
test sees.  tests/alloc_recipe.py is a fixed list of calls over the whole public surface in three groups; each group runs in a child
process (the switches are read once per process) under

  default   nothing set                          again   the same: the control of the comparison itself
  nan       DFM_ALLOC_POISON=255                 every byte handed out is a NaN pattern in fp32 / fp16
  junk      DFM_ALLOC_POISON=90                  0x5A5A5A5A = 1.5e16 in fp32, 203.25 in fp16: finite garbage for the paths on which a
                                                 NaN is dropped by a max, a < or a !(x > y) reject
  guard     DFM_ALLOC_GUARD=64 + poison 90       exact-size blocks between 64 KiB bands of 0xA5 that are checked at release

and every one of them must give, key by key and bit by bit (alloc_recipe.compare: dtype, shape, bytes - no tolerance, no key left
out), what `default` gives; inside each child the second pass over the same handles, after a pass that dirties and resizes every
buffer, must equal the first.  The counters of engine.alloc_diag() show that the diagnostics were live: bytes poisoned, two bands
checked per block handed out (every handle is closed and the cache trimmed before they are read) and none damaged.

No setting takes accessible bytes away behind a buffer (DFM_ALLOC_CACHE=0 without guards would, and is not in the matrix), so none can
turn a latent over-read into a fault.  The graph=True entries run under `guard` as well: no DevPool::alloc can run between
hipStreamBeginCapture and hipStreamEndCapture (sample_impl captures enqueue_forward, launch_heads, launch_restraint and
launch_clash_force only; none of them allocates - the workspace, the time grid and the message table are ensured before the capture).

One child at a time, each under its own time limit: three times what the group's `default` child took on an MI355X, interpreter
start included - 1.1 / 0.7 / 1.3 s, so 3.3 / 2.1 / 3.9 s (profiles/alloc_diag.txt holds every child's seconds and counters; `guard`,
with its device-wide wait per block, stayed within 0.1 s of `default` there).  A child that ends by a signal, with status 134 or 139,
or at its time limit stops the module: every later case fails at once without starting a process.  The recipe itself takes under a
second, most of a child is interpreter start, library load and HIP initialisation: a child stopped at limits this short has, far
more likely than hung, started slowly on a busy machine - the message says how long it ran; read it before looking for a hang.

The recipe is sized for the MI355X's 256 compute units: its launch on the dynamic-task form (alloc_recipe.DYN) is asserted in the
trunk child before anything is stored, so on a device with another CU count every trunk case fails at that assert.

Found with it (both in the diagnostic itself, none in a kernel): the poison fill of a block was not waited for.  A bound pool filled on
its own non-blocking stream and upload() then copied synchronously, in no stream's order (refine's start_pos came out as NaN in one
pass of `nan`); an unbound pool filled on the null stream and upload_async() then copied on the call's own stream (the
one-byte-per-residue interface flags of dfm_native_create and the one-atom ligand of dfm_atoms_create were replaced by the fill under
`nan` and `junk`: i_rmsd over every residue, no contact at all).  DevPool::alloc now waits for the fill."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import alloc_recipe as ar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = {"default": {}, "again": {}, "nan": {"DFM_ALLOC_POISON": "255"}, "junk": {"DFM_ALLOC_POISON": "90"},
        "guard": {"DFM_ALLOC_GUARD": "64", "DFM_ALLOC_POISON": "90"}}
DEFAULT_SECONDS = {"trunk": 1.1, "start": 0.7, "analysis": 1.3}      # the whole child, measured on an MI355X: profiles/alloc_diag.txt
_results = {}
_stopped = []      # the message of the child that faulted, hung or aborted


def child(group, tag, tmp):
    """The result set of `group` under `tag`: one child process, run once per session."""
    if (group, tag) in _results:
        return _results[(group, tag)]
    if _stopped:
        pytest.fail("not started: an earlier child faulted or hung\n" + _stopped[0], pytrace=False)
    out = str(tmp / f"{group}_{tag}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DFM_")}      # the switches are read once per process
    env.update(ENVS[tag])
    limit = 3.0 * DEFAULT_SECONDS[group]
    cmd = [sys.executable, os.path.join(ROOT, "tests", "alloc_recipe.py"), group, out]
    t0 = time.perf_counter()
    try:
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=limit)
        rc, text = p.returncode, p.stdout
    except subprocess.TimeoutExpired as e:
        rc, text = "time limit", e.stdout or b""
    tail = f"{group} / {tag}: exit {rc} after {time.perf_counter() - t0:.1f} s (limit {limit:.1f} s)\n" + text.decode(errors="replace")[-2000:]
    if rc == "time limit":
        tail = "stopped at its time limit (sized for a warm start: a slow start on a busy machine looks the same as a hang)\n" + tail
    if rc == "time limit" or rc < 0 or rc in (134, 139):
        _stopped.append(tail)
    assert rc == 0, tail
    print(tail)
    _results[(group, tag)] = dict(np.load(out, allow_pickle=False))
    return _results[(group, tag)]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("alloc_diag")


@pytest.mark.parametrize("tag", list(ENVS))
@pytest.mark.parametrize("group", ar.GROUPS)
def test_results_do_not_depend_on_what_the_allocator_hands_out(group, tag, tmp):
    # tag "default" is compared with itself: those three cases check pass 1 == pass 2 and the zero counters only; the control of the
    # comparison between processes is "again"
    ref = child(group, "default", tmp)
    r = child(group, tag, tmp)
    keys = [k for k in r if not k.startswith("__")]
    assert len(keys) > 50, keys
    assert r["__pass2_differs"].tolist() == [], "the second pass over the same handles differs from the first"
    assert ar.compare(ref, r) == [], f"differs from the default allocator under {ENVS[tag]}"
    d = dict(zip(ar.DIAG, r["__diag"].tolist()))
    cfg = str(r["__config"])
    assert d["blocks"] > 0, d
    for k, v in ENVS[tag].items():
        assert f"{k}={v}" in cfg, cfg
    if not ENVS[tag]:
        assert "env: none" in cfg and [d[k] for k in ar.DIAG[1:]] == [0, 0, 0, -1, -1], (d, cfg)
    if "DFM_ALLOC_POISON" in ENVS[tag]:
        assert d["poisoned_bytes"] > 0, d
    if "DFM_ALLOC_GUARD" in ENVS[tag]:
        # every handle is closed and the cache trimmed: each block handed out has been released, both of its bands checked
        assert d["bands_checked"] == 2 * d["blocks"] > 0 and d["bands_damaged"] == 0, d
        assert d["poisoned_bytes"] > 0 and d["first_damaged_size"] == -1 and d["first_damaged_offset"] == -1, d
    else:
        assert d["bands_checked"] == 0 and d["bands_damaged"] == 0, d


def test_the_dynamic_task_launch_is_in_the_recipe(tmp):
    """The trunk child asserts with edge_harness.task_form / coord_form that its B = 44 launch runs the dynamic-task form of the message
    and coordinate kernels on this device; here: that the launch is there and counts on 256 compute units."""
    import edge_harness as eh
    r = child("trunk", "default", tmp)
    B, N, Lg = ar.DYN["B"], ar.DYN["R"] + ar.DYN["L"], ar.DYN["L"]
    assert r["sample_dynamic/mfma16/lig_pos"].shape == (B, Lg, 3, 3) and np.isfinite(r["sample_dynamic/mfma16/lig_pos"]).all()
    assert B * N >= 2 * 256 * eh.EDGE_WAVES and eh.task_form(B, N, 60, 256) == "dynamic" and eh.coord_form(B, Lg, 256) == "dynamic"
