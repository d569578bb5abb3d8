"""The binding every kernel harness shares (tests/{dense,edge,heads,geom,metrics,pose,ensemble,aux}_harness.py over tests/kernels/harness_common.h).

The guard-band protocol.  A shim (tests/kernels/<name>_harness.hip) is host code that drives the shipped launchers of
dfmdock_amd/libdfmdock_amd.so on host arrays.  One call is a ctypes record: SLOTS named buffers first, then the shim's scalars.  Every
buffer in use gets a device block of its own with `guard` bytes of 0xff before and after its interior, and an output's interior starts
as 0xff too (Out(dtype, n)) or as what the caller put there (Out(dtype, init=...)).  The shim returns every output block WITH its guard
bands after a success and after a launcher's refusal (hipErrorInvalidValue).  The host copy of an output block starts with ZERO guards:
a block that came back has 0xff there, one that never did has zeros, and `collect` refuses anything else - a byte a kernel wrote
outside its block - in every call of every harness.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dfmdock_amd")
HIP_SUCCESS, HIP_INVALID_VALUE = 0, 1


class Buf(C.Structure):
    """harness_common.h HarnessBuf.  out 0: input; 1: output, sentinel interior; 2: in / out, the host's interior uploaded first."""
    _fields_ = [("host", C.c_void_p), ("bytes", C.c_longlong), ("out", C.c_int)]


class Out:
    """An output buffer: dtype and element count; init = None (sentinel interior) or an array the interior starts as (in / out)."""
    def __init__(self, dtype, n=None, init=None):
        self.dtype = np.dtype(dtype)
        self.init = None if init is None else np.ascontiguousarray(init, self.dtype)
        self.n = int(n if init is None else self.init.size)


def guards_intact(res, slot):
    a, b = res[slot + "_guard"]
    return bool((a == 0xff).all() and (b == 0xff).all())


def is_sentinel(x):
    """Elementwise: does a 4-byte element still hold the 0xff fill?"""
    return np.ascontiguousarray(x).view(np.uint32) == 0xffffffff


def hipcc():
    return os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"


_built = {}


def compile_shim(name, outdir):
    """tests/kernels/<name>_harness.hip -> lib<name>_harness.so in outdir: hipcc --offload-arch=gfx950 -shared -fPIC, linked against the
    built library with an rpath.  Once per process and shim: a second request returns the first build's path.  Raises if the compiler
    is missing."""
    if name not in _built:
        cc = hipcc()
        if not (os.path.isfile(cc) or shutil.which(cc)):
            raise RuntimeError(f"hipcc not found ({cc}): the kernel harness cannot be built")
        out = os.path.join(str(outdir), f"lib{name}_harness.so")
        subprocess.run([cc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC",
                        os.path.join(ROOT, "tests", "kernels", f"{name}_harness.hip"), "-o", out,
                        "-L", LIBDIR, "-ldfmdock_amd", "-Wl,-rpath," + LIBDIR], check=True, capture_output=True, text=True)
        _built[name] = out
    return _built[name]


def exported_symbols(path, defined):
    """`nm -D` of a shared library: its defined (exported) or its undefined (imported) dynamic symbols, as nm prints them."""
    return subprocess.run(["nm", "-D", "--defined-only" if defined else "--undefined-only", path], check=True, capture_output=True,
                          text=True).stdout


def _converter(ctype):
    """How a Python value becomes a field of this ctypes type: double[3] and the like from a sequence, float, else int."""
    if issubclass(ctype, C.Array):
        return lambda v: ctype(*[float(x) for x in v])
    return float if ctype in (C.c_float, C.c_double) else int      # (a c_float field takes a float32 value unchanged)


class KernelHarness:
    """One loaded shim.  call: the module's Call structure; slots / ops: the names of its buffer slots and op codes, in the shim's order.
    check: whether run() asserts success unless told otherwise."""
    check = False

    def __init__(self, path, call, slots, ops):
        self.path, self.Call, self.slots, self.ops = path, call, tuple(slots), tuple(ops)
        self.convert = {n: _converter(t) for n, t in call._fields_[1:]}
        self.lib = L = C.CDLL(path)
        L.kh_run.argtypes = [C.POINTER(call), C.c_int]
        L.kh_run.restype = C.c_int
        L.kh_guard_bytes.restype = L.kh_call_bytes.restype = C.c_longlong
        self.guard = int(L.kh_guard_bytes())
        assert int(L.kh_call_bytes()) == C.sizeof(call), f"{os.path.basename(path)}: the ctypes call record differs from the shim's"

    def fill_call(self, bufs, scalars):
        """The ctypes record of one call.  bufs: slot -> None (unused), array (input, uploaded as is) or Out.  Returns (call, host, keep):
        host[slot] = (guard-banded host block, dtype, interior bytes) of every Out; keep holds the input arrays alive."""
        call, g = self.Call(), self.guard
        keep, host = [], {}
        for k, v in scalars.items():
            setattr(call, k, self.convert[k](v))
        for k, v in bufs.items():
            if v is None:
                continue
            b = call.buf[self.slots.index(k)]
            if isinstance(v, Out):
                nbytes = v.dtype.itemsize * v.n
                raw = np.zeros(g * 2 + nbytes, np.uint8)
                if v.init is not None:
                    raw[g:g + nbytes] = v.init.reshape(-1).view(np.uint8)
                host[k] = (raw, v.dtype, nbytes)
                b.host, b.bytes, b.out = raw.ctypes.data, nbytes, 1 if v.init is None else 2
            else:
                a = np.ascontiguousarray(v)
                nbytes = a.nbytes
                if a.size == 0:      # an empty array still needs an address
                    a = np.zeros(1, a.dtype)
                keep.append(a)
                b.host, b.bytes, b.out = a.ctypes.data, nbytes, 0
        return call, host, keep

    def collect(self, err, host, check=False, op=""):
        """{slot: interior array, slot + '_guard': (before, after) bytes, 'err': err}.  Always: no byte outside a block that came back
        changed, and a successful call returned every block.  check: the call succeeded."""
        g, res = self.guard, {"err": int(err)}
        if check:
            assert err == HIP_SUCCESS, f"{op}: hipError {err}"
        for k, (raw, dt, nbytes) in host.items():
            res[k] = raw[g:g + nbytes].view(dt).copy()
            res[k + "_guard"] = (raw[:g], raw[g + nbytes:])
            back = bool(raw[:g].any())      # (a call that was refused before the upload copies nothing back: the guards are still zero)
            assert back or err != HIP_SUCCESS, f"{op}: the {k} block did not come back from a successful call"
            assert not back or guards_intact(res, k), f"{op}: bytes outside the {k} block changed"
        return res

    def run(self, op, bufs, check=None, **scalars):
        """One launch: fill_call, the shim's kh_run, collect.  check = None: the class's default."""
        call, host, keep = self.fill_call(bufs, scalars)
        err = self.lib.kh_run(C.byref(call), self.ops.index(op))
        return self.collect(err, host, self.check if check is None else check, op)


# ---- replay of stored launches (child processes) ------------------------------------------------------------------------------------
def save_launches(path, launches):
    """launches: list of {op, bufs: {slot: array | Out | None}, scalars: {...}} -> one npz."""
    flat = {"n": np.array(len(launches))}
    for i, L in enumerate(launches):
        flat[f"{i}/op"] = np.array(L["op"])
        for k, v in L["bufs"].items():
            if isinstance(v, Out):
                if v.init is None:
                    flat[f"{i}/out/{k}"] = np.array([v.dtype.str, str(v.n)])
                else:
                    flat[f"{i}/io/{k}"] = v.init
            elif v is not None:
                flat[f"{i}/in/{k}"] = np.asarray(v)
        for k, v in L["scalars"].items():
            flat[f"{i}/int/{k}"] = np.array(v)
    np.savez(path, **flat)


def replay(h, path_in, path_out):
    """Runs every stored launch on harness h; writes each output as <i>/<slot> and whether its guards held as <i>/<slot>_guard_ok."""
    d = np.load(path_in)
    res = {}
    for i in range(int(d["n"])):
        op = str(d[f"{i}/op"])
        part = lambda kind: {k.split("/")[2]: d[k] for k in d.files if k.startswith(f"{i}/{kind}/")}
        bufs = part("in")
        bufs.update({k: Out(np.dtype(str(v[0])), int(v[1])) for k, v in part("out").items()})
        bufs.update({k: Out(v.dtype, init=v) for k, v in part("io").items()})
        r = h.run(op, bufs, **{k: v.item() for k, v in part("int").items()})
        if r["err"] != HIP_SUCCESS:
            raise RuntimeError(f"launch {i} ({op}): hipError {r['err']}")
        for k, v in bufs.items():
            if isinstance(v, Out):
                res[f"{i}/{k}"] = r[k]
                res[f"{i}/{k}_guard_ok"] = np.array(guards_intact(r, k))
    np.savez(path_out, **res)


def child_main(harness, argv):
    """`python <module>_harness.py child SHIM IN.npz OUT.npz`: the body of a harness module's __main__."""
    if len(argv) == 5 and argv[1] == "child":
        replay(harness(argv[2]), argv[3], argv[4])
    else:
        raise SystemExit(f"usage: {os.path.basename(argv[0])} child SHIM IN.npz OUT.npz")
