"""The shared binding of the kernel harnesses without a GPU (tests/kernel_harness.py over tests/kernels/harness_common.h): every shim's
call record has the layout its module declares, fill_call builds the record and the guard-banded host blocks by one rule, collect has
power (a byte outside a block, or a block missing after a success, is refused), stored launches survive a round trip, and a shim is
built once per process."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_harness
import edge_harness
import ensemble_harness
import geom_harness
import heads_harness
import kernel_harness as kh
import metrics_harness
import pose_harness
from kernel_harness import HIP_INVALID_VALUE, HIP_SUCCESS, Out

MODULES = {"dense": dense_harness, "edge": edge_harness, "heads": heads_harness, "geom": geom_harness, "metrics": metrics_harness,
           "pose": pose_harness, "ensemble": ensemble_harness}


@pytest.mark.parametrize("name", sorted(MODULES))
def test_call_record_layout(name, tmp_path_factory):
    """Constructing the Harness asserts kh_call_bytes() == sizeof(Call): a field added on one side only is caught in all seven."""
    m = MODULES[name]
    h = m.Harness(m.compile_shim(tmp_path_factory.mktemp(name + "_layout")))
    assert h.guard >= 1024 and C.sizeof(m.Call) > len(m.SLOTS) * C.sizeof(kh.Buf)
    assert h.check == (name in ("metrics", "pose", "ensemble"))


@pytest.fixture(scope="module")
def h(tmp_path_factory):
    return geom_harness.Harness(geom_harness.compile_shim(tmp_path_factory.mktemp("geom_fill")))


def test_fill_call(h):
    ca4 = np.arange(8, dtype=np.float32)
    bufs = dict(ca4=ca4, ctl=np.zeros(0, np.uint32), edges=Out(np.int32, 3), lig_cur=Out(np.float64, init=[1, 2]), codes=None)
    call, host, keep = h.fill_call(bufs, dict(B=2, mask_dist=np.float32(20.5), seed=2 ** 63 + 5))
    b = {k: call.buf[h.slots.index(k)] for k in bufs}
    assert [b[k].out for k in ("ca4", "ctl", "edges", "lig_cur")] == [0, 0, 1, 2]
    assert [b[k].bytes for k in ("ca4", "ctl", "edges", "lig_cur")] == [ca4.nbytes, 0, 12, 16]
    assert b["ctl"].host and b["ca4"].host and not b["codes"].host
    assert all(not call.buf[i].host for i, s in enumerate(h.slots) if s not in bufs)
    assert set(host) == {"edges", "lig_cur"}
    g = h.guard
    for k, (raw, dt, nbytes) in host.items():
        assert b[k].host == raw.ctypes.data and raw.size == 2 * g + nbytes
        assert not raw[:g].any() and not raw[g + nbytes:].any(), "host guards start as zero"
    assert np.array_equal(host["lig_cur"][0][g:g + 16].view(np.float64), [1.0, 2.0]) and host["lig_cur"][1] == np.float64
    assert not host["edges"][0].any()
    assert (call.B, call.mask_dist, call.seed) == (2, 20.5, 2 ** 63 + 5)


def block(h, dtype, values, guard_fill):
    """A host block as fill_call builds it, its guards then set to guard_fill (0xff: it came back; 0: it never did)."""
    v = np.ascontiguousarray(values, dtype)
    raw = np.zeros(2 * h.guard + v.nbytes, np.uint8)
    raw[h.guard:h.guard + v.nbytes] = v.view(np.uint8)
    raw[:h.guard] = raw[h.guard + v.nbytes:] = guard_fill
    return raw, np.dtype(dtype), v.nbytes


def test_collect_has_power(h):
    r = h.collect(HIP_SUCCESS, {"edges": block(h, np.int32, [7, -8, 9], 0xff)}, check=True)
    assert r["err"] == HIP_SUCCESS and r["edges"].dtype == np.int32 and r["edges"].tolist() == [7, -8, 9] and kh.guards_intact(r, "edges")
    for at in (0, h.guard - 1, h.guard + 12, 2 * h.guard + 11):      # first and last byte of the front guard, then of the back guard
        blk = block(h, np.int32, [7, -8, 9], 0xff)
        blk[0][at] ^= 0x10
        for err in (HIP_SUCCESS, HIP_INVALID_VALUE):
            with pytest.raises(AssertionError, match="outside the edges block"):
                h.collect(err, {"edges": blk})
    never = {"edges": block(h, np.int32, [0, 0, 0], 0)}
    r = h.collect(HIP_INVALID_VALUE, never)      # refused before the upload: nothing comes back, and that is accepted
    assert r["err"] == HIP_INVALID_VALUE and not kh.guards_intact(r, "edges")
    with pytest.raises(AssertionError, match="did not come back"):
        h.collect(HIP_SUCCESS, never, check=True)
    with pytest.raises(AssertionError, match="did not come back"):
        h.collect(HIP_SUCCESS, never)
    with pytest.raises(AssertionError, match="hipError 1"):
        h.collect(HIP_INVALID_VALUE, never, check=True)


class Echo:
    """A stand-in for a Harness: run() records its arguments and returns every Out as its prefill (zeros without one)."""
    def __init__(self):
        self.calls = []

    def run(self, op, bufs, **scalars):
        self.calls.append((op, bufs, scalars))
        res = {"err": HIP_SUCCESS}
        ff = np.full(8, 0xff, np.uint8)
        for k, v in bufs.items():
            if isinstance(v, Out):
                res[k] = np.zeros(v.n, v.dtype) if v.init is None else v.init.reshape(-1).copy()
                res[k + "_guard"] = (ff, ff if k != "mbuf" else ff * 0)      # (mbuf: reported as not intact)
        return res


def test_save_launches_replay_round_trip(tmp_path):
    A = np.arange(12, dtype=np.float32).reshape(3, 4)
    agg = np.array([5, 6, 7], np.uint64)
    launches = [{"op": "edge_bf16", "bufs": {"A": A, "Ah": None, "fout": Out(np.float32, 6), "agg": Out(np.uint64, init=agg)},
                 "scalars": dict(B=3, att_b=0.375, ab_bstride=2 ** 40)},
                {"op": "coord_bf16", "bufs": {"edges": np.array([[1, 2]], np.int32), "mbuf": Out(np.uint16, 5)}, "scalars": dict(K=60)}]
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    kh.save_launches(fin, launches)
    e = Echo()
    kh.replay(e, fin, fout)
    (op0, b0, s0), (op1, b1, s1) = e.calls
    assert (op0, op1) == ("edge_bf16", "coord_bf16")
    assert set(b0) == {"A", "fout", "agg"} and b0["A"].dtype == np.float32 and np.array_equal(b0["A"], A)
    assert (b0["fout"].dtype, b0["fout"].n, b0["fout"].init) == (np.float32, 6, None)
    assert b0["agg"].dtype == np.uint64 and np.array_equal(b0["agg"].init, agg)
    assert s0 == dict(B=3, att_b=0.375, ab_bstride=2 ** 40) and type(s0["B"]) is int and type(s0["att_b"]) is float
    assert np.array_equal(b1["edges"], [[1, 2]]) and b1["edges"].dtype == np.int32 and (b1["mbuf"].dtype, b1["mbuf"].n) == (np.uint16, 5)
    assert s1 == dict(K=60)
    o = np.load(fout)
    assert set(o.files) == {"0/fout", "0/fout_guard_ok", "0/agg", "0/agg_guard_ok", "1/mbuf", "1/mbuf_guard_ok"}
    assert np.array_equal(o["0/agg"], agg) and o["0/fout"].shape == (6,) and o["1/mbuf"].dtype == np.uint16
    assert bool(o["0/agg_guard_ok"]) and bool(o["0/fout_guard_ok"]) and not bool(o["1/mbuf_guard_ok"])

    class Refuses(Echo):
        def run(self, op, bufs, **scalars):
            return {"err": HIP_INVALID_VALUE}

    with pytest.raises(RuntimeError, match=r"launch 0 \(edge_bf16\): hipError 1"):
        kh.replay(Refuses(), fin, fout)


CHILD = """
import os, subprocess, sys
import edge_harness as eh
import kernel_harness as kh
try:
    eh.compile_shim(sys.argv[1])
    sys.exit("no error without a compiler")
except RuntimeError as e:
    assert "hipcc not found (/nonexistent/hipcc)" in str(e), e
os.environ["HIPCC"] = sys.executable      # a file that exists: the compiler check passes, and the compiler itself is the fake below
built = []
def fake(cmd, **kw):
    built.append(cmd[cmd.index("-o") + 1])
    open(built[-1], "w").close()
subprocess.run = fake
a = eh.compile_shim(sys.argv[1])
b = eh.compile_shim(sys.argv[2])
c = kh.compile_shim("dense", sys.argv[2])
assert a == b == os.path.join(sys.argv[1], "libedge_harness.so"), (a, b)
assert c == os.path.join(sys.argv[2], "libdense_harness.so") and built == [a, c], built
print("ok")
"""


def test_compile_shim_is_memoised_and_needs_a_compiler(tmp_path):
    """In a child process, so that this process's environment and memo stay as they are: a missing compiler is a RuntimeError for edge
    too, and two requests for one shim run the compiler once and return the first build's path."""
    d1, d2 = tmp_path / "a", tmp_path / "b"
    d1.mkdir(); d2.mkdir()
    p = subprocess.run([sys.executable, "-c", CHILD, str(d1), str(d2)], env={**os.environ, "HIPCC": "/nonexistent/hipcc"},
                       cwd=os.path.dirname(os.path.abspath(__file__)), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
