"""Kernel-level harness of the graph front end and the pose kernels (tests/kernels/geom_harness.hip): everything upstream of the trunk.

The shim drives the shipped launchers of dfmdock_amd/libdfmdock_amd.so (dfm::launch_knn_sample, launch_edge_feat with and without the
table classification, launch_l0_pairs, launch_init_pose, launch_clash_force) under the guard-band protocol of tests/kernel_harness.py;
it exports the host versions of philox4x32 / u01 / pack_code and holds one test-only kernel that evaluates the hardware log2 of the
sampling race on a given array.  This module binds it and holds
  * the references, written from the model definition (score_net_mlsb.py:30-135, coords6d.py, inference_base.py:255-384), not from the
    kernels: kernels_geom.hip is compiled with -ffp-contract=off, so subtraction, product, sum, sqrt and division are correctly rounded
    fp32 in the order written and a numpy float32 restatement gives the same bits - kNN slots and order, distance bin, relpos, radial
    and every index are EXACT; only the angles (float64 from the same fp32 inputs, with a decided / undecided margin), the race keys
    (float64 with the measured envelope of the hardware log2) and the native draws of k_init_pose carry a margin;
  * the comparisons the GPU tests use (check_knn, check_sampled, check_edge_codes, check_pairs, check_classification), which
    tests/test_geom_harness_cpu.py also turns on seeded mutants of the references to show that they have power;
  * the input generators, so that the CPU tests can check the exclusion caps on the inputs the GPU tests use;
  * non-finite poses (include/dfmdock_amd.h, "non-finite poses in the trunk calls"): the geometries NONFINITE with a NaN or infinite
    coordinate in one trajectory, the ordering rule of the graph as order_word / knn_ref / sample_ref(near=) / check_sampled, the
    features and the table-hit predicate with IEEE comparisons, and present_selection - a word-level restatement of the selection
    as it stood before the rule, kept as a named mutant.
Out of scope: k_prep_pose is in the heads harness; k_restraint, k_igso3_cdf and k_start_pose each have a direct comparison with numpy
or the reference (tests/test_gpu_restraints.py, tests/test_gpu_refine.py).

The counter layout of the edge stream (k_knn_sample): candidate j of node i of trajectory b takes word j % 4 of the Philox block with
counter (lo32(b N + i), hi32(b N + i) ^ ((j / 4) << 8), evaluation index, RNG_EDGES) and key (seed lo, seed hi).  The node index is
b N + i: trajectory b of a batch draws the stream a B = 1 launch would draw for node b N + i, NOT the one of node i - two trajectories
holding the same pose get different graphs, and a trajectory's graph depends on its place in the batch.
"""
import ctypes as C
import functools

import numpy as np

import kernel_harness as kh
from kernel_harness import HIP_INVALID_VALUE, HIP_SUCCESS, LIBDIR, ROOT, Out, guards_intact, is_sentinel      # noqa: F401 (re-exported)

LAUNCHERS = ("_ZN3dfm17launch_knn_sampleEPK15HIP_vector_typeIfLj4EEiiiimjPiPKjP12ihipStream_t",
             "_ZN3dfm16launch_edge_featEPK15HIP_vector_typeIfLj4EES3_S3_PKiiiiifPjPfRKNS_10L0ClassifyES6_P12ihipStream_t",
             "_ZN3dfm15launch_l0_pairsEPK15HIP_vector_typeIfLj4EES3_S3_iifPS0_IjLj2EEPS0_IjLj4EEP12ihipStream_t",
             "_ZN3dfm16launch_init_poseEPKfS1_iiiiS1_S1_mPfS2_S2_P12ihipStream_t",
             "_ZN3dfm18launch_clash_forceEPKfiiiPfS2_P12ihipStream_t")
U = 2.0 ** -24                    # unit roundoff of fp32
RNG_EDGES, RNG_INIT = 1, 3
MISS = 0x80000000

SLOTS = ("n4", "ca4", "cb4", "edges", "ctl", "codes", "radial", "code0", "src", "rows", "counter", "eval_ctr",
         "rec_pos", "lig0", "R0", "tr_draw", "lig_cur", "tr_upd", "rot_upd", "log_in", "log_out")
INTS = ("B", "N", "R", "L", "K", "knn", "nsamp", "all_atoms")
OPS = ("knn_sample", "edge_feat", "l0_pairs", "init_pose", "clash_force", "hw_log2")

# the provisional envelope of the hardware log2 (the CPU tests check the exclusion caps with it) and the measured one
# (profiles/geom_kernels.txt: test_hw_log2_envelope on an MI355X; the GPU test asserts that the measurement stays inside it)
LOG2_PROVISIONAL = (2.0 ** -20, 2.0 ** -24)      # |hw - log2 u| <= rel |log2 u| + abs
LOG2_ENVELOPE = (2.0 ** -22, 2.0 ** -26)         # measured: 2^-23.01 relative over all u < 1, no absolute excess near 1; twice that, the term kept


class Call(C.Structure):
    _fields_ = ([("buf", kh.Buf * len(SLOTS)), ("n", C.c_longlong), ("seed", C.c_ulonglong), ("mask_dist", C.c_float),
                 ("stream_id", C.c_uint)] + [(n, C.c_int) for n in INTS])


compile_shim = functools.partial(kh.compile_shim, "geom")
U32P = C.POINTER(C.c_uint)


class Harness(kh.KernelHarness):
    def __init__(self, path):
        super().__init__(path, Call, SLOTS, OPS)
        L = self.lib
        L.gh_philox.argtypes = [C.c_longlong, U32P, C.c_uint, C.c_uint, U32P]
        L.gh_u01.argtypes = [C.c_longlong, U32P, C.POINTER(C.c_float)]
        L.gh_u01_scan.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.gh_pack_code.argtypes = [C.c_int] * 5
        L.gh_pack_code.restype = C.c_uint
        L.gh_rng_edges.restype = L.gh_rng_init.restype = C.c_uint
        L.gh_find_top_uniform.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_uint, C.c_ulonglong, C.c_longlong, U32P]

    # ---- host functions of the library's headers
    def philox(self, ctr, k0, k1):
        ctr = np.ascontiguousarray(ctr, np.uint32).reshape(-1, 4)
        out = np.zeros_like(ctr)
        self.lib.gh_philox(ctr.shape[0], ctr.ctypes.data_as(U32P), int(k0), int(k1), out.ctypes.data_as(U32P))
        return out

    def u01(self, x):
        x = np.ascontiguousarray(x, np.uint32).reshape(-1)
        out = np.zeros(x.size, np.float32)
        self.lib.gh_u01(x.size, x.ctypes.data_as(U32P), out.ctypes.data_as(C.POINTER(C.c_float)))
        return out

    def u01_scan(self):
        lo, hi = C.c_float(), C.c_float()
        mono = self.lib.gh_u01_scan(C.byref(lo), C.byref(hi))
        return int(mono), np.float32(lo.value), np.float32(hi.value)

    def find_top_uniform(self, n0, n1, c1_mul, n2, vary_seed, c3, seed, max_blocks=1 << 26):
        found = np.zeros(4, np.uint32)
        ok = self.lib.gh_find_top_uniform(n0, n1, c1_mul, n2, int(vary_seed), c3, seed, max_blocks, found.ctypes.data_as(U32P))
        return tuple(int(x) for x in found) if ok else None


f32 = np.float32


def f64(x):
    return np.asarray(x, np.float64)


# ---- Philox4x32-10 and u01 in numpy ----------------------------------------------------------------------------------------------
def philox_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011) on arrays of counter words; returns the four output words."""
    M0, M1, W0, W1, M = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85, np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(x, np.uint64) for x in (c0, c1, c2, c3)))
    k0, k1 = int(k0), int(k1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & M, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & M
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def u01_np(x):
    """((float)(x >> 8) + 0.5f) * 2^-24 in fp32: x >> 8 < 2^24 converts exactly, the sum rounds (to even) from 2^23 on."""
    return ((np.asarray(x, np.uint32) >> np.uint32(8)).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0)


def edge_stream_u(nodes, N, stream_id, seed):
    """The uniforms of the edge stream: u [len(nodes)][N] of the candidates j < N of the global node indices `nodes` (= b N + i)."""
    nodes = np.asarray(nodes, np.uint64)[:, None]
    c = np.arange((N + 3) // 4, dtype=np.uint64)[None, :]
    w = philox_np(nodes & np.uint64(0xFFFFFFFF), (nodes >> np.uint64(32)) ^ (c << np.uint64(8)), stream_id, RNG_EDGES,
                  seed & 0xFFFFFFFF, seed >> 32)
    return u01_np(np.stack(w, -1).reshape(nodes.shape[0], -1)[:, :N])


# ---- kNN and the sampling race ---------------------------------------------------------------------------------------------------
def degree_of(N, knn=20, nsamp=40):
    """score_net_mlsb.py:89-94: a complex smaller than the degree keeps every residue."""
    if N < knn:
        knn, nsamp = N, 0
    if N < knn + nsamp:
        nsamp = N - knn
    return knn, nsamp


def dist32(ca):
    """|x_i - x_j| [N][N] in fp32 with the kernel's (and torch's op-by-op) order: sqrt((dx dx + dy dy) + dz dz)."""
    x, y, z = (np.ascontiguousarray(ca[:, k], f32) for k in range(3))
    with np.errstate(invalid="ignore"):      # non-finite coordinates: inf - inf and every operation on a NaN give NaN
        dx = x[:, None] - x[None, :]
        acc = dx * dx
        dx = y[:, None] - y[None, :]
        acc += dx * dx
        dx = z[:, None] - z[None, :]
        acc += dx * dx
        return np.sqrt(acc, out=acc)


NAN_WORD = 0x7F800001      # the one word of every NaN in the graph's order: just above +inf (0x7F800000)


def order_word(d):
    """The ordering rule of the graph (include/dfmdock_amd.h, non-finite poses) as one uint32 per distance: a number (>= +0, +inf
    included) orders like its bit pattern; a NaN - either sign, any payload - orders after every number, and all NaN tie."""
    d = np.ascontiguousarray(d, f32)
    return np.where(np.isnan(d), np.uint32(NAN_WORD), d.view(np.uint32))


def knn_ref(d, knn, mutant=None):
    """The knn smallest (d, j) of every row in ascending order, the lowest j first on equal d: (order_word(d) << 32) | j is one sortable
    word per candidate (a NaN distance after every number, ties by ascending j).  Only residues j < N are candidates: there is no
    padding here, so none can be taken.  mutant 'tie_high': the highest j first."""
    N = d.shape[1]
    j = np.arange(N, dtype=np.uint64)[None, :]
    word = (order_word(d).astype(np.uint64) << np.uint64(32)) | (np.uint64(N - 1) - j if mutant == "tie_high" else j)
    low = np.sort(np.partition(word, knn - 1, axis=1)[:, :knn], axis=1) & np.uint64(0xFFFFFFFF)
    return (N - 1 - low if mutant == "tie_high" else low).astype(np.int32)


def npl_of(N):
    """Candidate slots per lane of the k_knn_sample instantiation that launch_knn_sample picks for N residues (64 NPL slots per node)."""
    return 4 if N <= 256 else 8 if N <= 512 else 12 if N <= 768 else 16 if N <= 1024 else 32 if N <= 2048 else 64


def present_select(keys, k):
    """Word-level restatement of knn_select AS IT STOOD before the ordering rule: keys [slots] uint32, slot index = candidate index.  A
    radix threshold from bit 30 down (bit 31 taken for clear), sel = key < threshold, ties at the k-th word by ascending candidate."""
    keys = np.asarray(keys, np.uint32)
    prefix = 0
    for bit in range(30, -1, -1):
        t = prefix | (1 << bit)
        c = int((keys < t).sum())
        if c == k:
            return keys < t
        if c < k:
            prefix = t
    sel = keys < prefix
    tie = np.flatnonzero(keys == prefix)[:max(k - int(sel.sum()), 0)]
    sel[tie] = True
    return sel


def present_selection(d, knn):
    """The named mutant of knn_ref: the kNN slots [N][knn] of the selection as it stood, on the raw words of the fp32 distances d [N][N]
    with +inf in the padding slots j >= N.  A selected padding slot comes out as its index j >= N; a slot that no winner was written to
    (fewer than knn words below the threshold: the kernel read LDS rows nobody wrote) as -1.  On finite coordinates it IS knn_ref."""
    N = d.shape[0]
    slots = 64 * npl_of(N)
    out = np.full((N, knn), -1, np.int32)
    pad = np.full(slots - N, 0x7F800000, np.uint32)
    for i in range(N):
        keys = np.concatenate([np.ascontiguousarray(d[i], f32).view(np.uint32), pad])
        win = np.flatnonzero(present_select(keys, knn))
        win = win[np.lexsort((win, keys[win]))][:knn]      # ranked by (word, j) through LDS
        out[i, :win.size] = win
    return out


def present_race(d, near, u, nsamp):
    """The sampled slots [N][nsamp] of the race as it stood, through the same word-level present_select: the word of a slot is +inf when
    it is a kNN winner, a padding slot OR at a distance whose word is +inf (`d != inf` was the test for "is a residue"), else the fp32
    word of |log2 u| d^3 (numpy's log2 for the hardware's: the last bits of a key differ, the words that decide here are +inf and NaN).
    Slots come out in candidate order, a missing one as -1."""
    N = d.shape[0]
    slots = 64 * npl_of(N)
    out = np.full((N, nsamp), -1, np.int32)
    with np.errstate(invalid="ignore"):
        dc = np.where(d < f32(1e-10), f32(1e-10), d)
        k2 = (np.abs(np.log2(f64(u))).astype(f32) * ((dc * dc) * dc)).astype(f32)
    k2 = np.where(d == f32(np.inf), f32(np.inf), k2)
    np.put_along_axis(k2, near.astype(np.int64), f32(np.inf), axis=1)
    pad = np.full(slots - N, 0x7F800000, np.uint32)
    for i in range(N):
        win = np.flatnonzero(present_select(np.concatenate([k2[i].view(np.uint32), pad]), nsamp))[:nsamp]
        out[i, :win.size] = win
    return out


def race_keys(d, near, u, envelope, mutant=None):
    """float64 race keys -log2(u_j) d_j^3 [n][N] (inf: not a candidate) and their error bounds.  d^3 as the kernel forms it, (d d) d in
    fp32 of the distance clamped at 1e-10; the kernel's key differs by the hardware log2 (envelope = (rel, abs)) and one fp32 product:
    bound = 2 ((rel |log2 u| + abs) d^3 + 2 u key).  mutant 'all_keys': the kNN winners stay in the race.
    Non-finite distances: a NaN distance has a NaN key (the clamp d < 1e-10 ? 1e-10 : d keeps a NaN); a residue at +inf has the key
    +inf, or NaN = 0 inf when its uniform is exactly 1.  check_sampled tells these from the +inf of a kNN winner by `near`."""
    with np.errstate(invalid="ignore"):
        dc = np.where(d < f32(1e-10), f32(1e-10), d)
        d3 = f64((dc * dc) * dc)
        l2 = np.abs(np.log2(f64(u)))
        key = l2 * d3
        bound = 2.0 * ((envelope[0] * l2 + envelope[1]) * d3 + 2 * U * key)
    if mutant != "all_keys":
        np.put_along_axis(key, near.astype(np.int64), np.inf, axis=1)
    return key, bound


def sample_ref(key, nsamp, mutant=None, near=None):
    """The nsamp smallest keys of every row as index lists [n][nsamp] (ascending key).  mutant 'largest': the 40 largest finite keys.
    With `near` (the kNN slots: no candidates), by the ordering rule on any keys: the candidates with a number key in ascending
    (key, j), +inf included; then the candidates with a NaN key in ascending j.  mutant 'nan_first': the NaN keys before the numbers."""
    if near is not None:
        n, N = key.shape
        cls = np.isnan(key).astype(np.int64)
        if mutant == "nan_first":
            cls = 1 - cls
        if near.shape[1]:
            np.put_along_axis(cls, near.astype(np.int64), 2, axis=1)
        k = np.where(cls == (1 if mutant == "nan_first" else 0), key, 0.0)
        jj = np.broadcast_to(np.arange(N), (n, N))
        return np.lexsort((jj, k, cls), axis=1)[:, :nsamp].astype(np.int32)
    if mutant == "largest":
        k = np.where(np.isfinite(key), -key, np.inf)
        return np.argsort(k, axis=1, kind="stable")[:, :nsamp].astype(np.int32)
    return np.argsort(key, axis=1, kind="stable")[:, :nsamp].astype(np.int32)


def check_knn(got, ref):
    """Exact: slots and order."""
    np.testing.assert_array_equal(np.asarray(got, np.int32), ref)


def check_sampled(got, near, key, bound, nsamp):
    """got [n][nsamp]: the sampled slots of n nodes, every one a residue index.  A node all of whose candidates (the residues outside its
    kNN slots `near`) have finite race keys - every node of a finite trajectory - goes through check_sampled_finite, exactly.  The others:
      * fewer than nsamp candidates at a number distance (key not NaN): every one of them is among the sampled slots (numbers first);
        nothing else is asked of the node but the range - the NaN candidates that fill it up may repeat;
      * at least nsamp of them: the slots are distinct candidates with number keys and, as a set, the nsamp smallest (key, j) - +inf keys
        (residues at infinity) tie and go by ascending j - exactly when the nsamp-th and the next key are decided, else within the band.
    Returns the number of undecided nodes."""
    got = np.asarray(got, np.int64)
    n, N = key.shape
    assert got.shape == (n, nsamp)
    if nsamp == 0:
        return 0
    assert ((got >= 0) & (got < N)).all(), "a sampled slot is no residue index"
    cand = np.ones((n, N), bool)
    if near.shape[1]:
        np.put_along_axis(cand, near.astype(np.int64), False, axis=1)
    plain = (np.isfinite(key) | ~cand).all(1)
    und = check_sampled_finite(got[plain], near[plain], key[plain], bound[plain], nsamp) if plain.any() else 0
    jj = np.arange(N)
    for r in np.flatnonzero(~plain):
        num = cand[r] & ~np.isnan(key[r])
        g = got[r]
        if num.sum() < nsamp:
            assert np.isin(jj[num], g).all(), f"node {r}: a candidate at a number distance was passed over for one at a NaN distance"
            continue
        assert np.unique(g).size == nsamp, f"node {r} has a sampled slot twice"
        assert num[g].all(), f"node {r}: a sampled slot is a kNN slot or has a NaN key although {int(num.sum())} number keys are left"
        idx = jj[num]
        idx = idx[np.lexsort((idx, key[r, idx]))]
        ref, lo = idx[:nsamp], key[r, idx[nsamp - 1]]
        hi = key[r, idx[nsamp]] if idx.size > nsamp else np.inf
        if not np.isfinite(hi) or hi - lo > bound[r, idx[nsamp - 1]] + bound[r, idx[nsamp]]:
            assert set(g.tolist()) == set(ref.tolist()), f"decided node {r} differs from the nsamp smallest race keys"
            continue
        und += 1
        fin = np.isfinite(key[r]) & num
        band = fin & (key[r] + bound[r] >= lo - bound[r, idx[nsamp - 1]]) & (key[r] - bound[r] <= hi + bound[r, idx[nsamp]])
        diff = np.zeros(N, bool)
        diff[np.setxor1d(g, ref)] = True
        assert not (diff & ~band).any(), f"undecided node {r}: a slot outside the ambiguous band differs"
    return und


def check_sampled_finite(got, near, key, bound, nsamp):
    """got [n][nsamp]: the sampled slots.  They are distinct, disjoint from the kNN slots `near`, candidates (finite key), and as a set
    the nsamp smallest keys: exactly at a DECIDED node (its nsamp-th and (nsamp+1)-th keys further apart than the sum of their bounds);
    at an undecided node the symmetric difference lies within the ambiguous band.  Returns the number of undecided nodes."""
    n, N = key.shape
    srt = np.sort(got, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "a node has a sampled slot twice"
    if near.shape[1]:
        assert not (got[:, :, None] == near[:, None, :]).any(), "a sampled slot repeats a kNN slot"
    assert np.isfinite(np.take_along_axis(key, got, axis=1)).all(), "a sampled slot is no candidate"
    if N > nsamp:      # the nsamp + 1 smallest keys are all the comparison needs
        part = np.argpartition(key, nsamp, axis=1)[:, :nsamp + 1]
        order = np.take_along_axis(part, np.argsort(np.take_along_axis(key, part, axis=1), axis=1, kind="stable"), axis=1)
    else:
        order = np.argsort(key, axis=1, kind="stable")
    ks, bs = np.take_along_axis(key, order, axis=1), np.take_along_axis(bound, order, axis=1)
    sel = np.zeros((n, N), bool)
    np.put_along_axis(sel, got, True, axis=1)
    ref = np.zeros((n, N), bool)
    np.put_along_axis(ref, order[:, :nsamp], True, axis=1)
    if N > nsamp:
        nxt = ks[:, nsamp]
        decided = ~np.isfinite(nxt) | (nxt - ks[:, nsamp - 1] > bs[:, nsamp - 1] + np.where(np.isfinite(nxt), bs[:, nsamp], 0.0))
    else:
        decided = np.ones(n, bool)
    bad = decided & (sel != ref).any(1)
    assert not bad.any(), f"decided nodes {np.flatnonzero(bad)[:5].tolist()} differ from the nsamp smallest race keys"
    for r in np.flatnonzero(~decided):
        lo, hi = ks[r, nsamp - 1] - bs[r, nsamp - 1], ks[r, nsamp] + bs[r, nsamp]
        band = (key[r] + bound[r] >= lo) & (key[r] - bound[r] <= hi)
        diff = sel[r] != ref[r]
        assert not (diff & ~band).any(), f"undecided node {r}: a slot outside the ambiguous band differs"
    return int((~decided).sum())


# ---- edge features ---------------------------------------------------------------------------------------------------------------
# torch.linspace(-180, 180, 23) as float32 (the model definition: score_net_mlsb.py:30-70; tests/golden/scalar_kats.npz holds the same)
ANGLE_BOUNDS = np.array([-180.0, -163.63636779785156, -147.27273559570312, -130.90908813476562, -114.54545593261719,
                         -98.18182373046875, -81.81818389892578, -65.45454406738281, -49.090911865234375, -32.72727584838867,
                         -16.36363983154297, 3.814697265625e-06, 16.36363983154297, 32.72727584838867, 49.090911865234375,
                         65.45454406738281, 81.81818389892578, 98.18182373046875, 114.54545593261719, 130.90908813476562,
                         147.27273559570312, 163.63636779785156, 180.0], np.float32)
PHI_BOUNDS = (18.0 * np.arange(11)).astype(np.float32)              # linspace(0, 180, 11)
DIST_BOUNDS = (3.25 + 1.25 * np.arange(39)).astype(np.float32)      # linspace(3.25, 50.75, 39): every value exact in fp32


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _norm(a):
    return np.sqrt(_dot(a, a))


def dihedral_deg(a, b, c, d, dt):
    """coords6d.py:25-43 in dtype dt, op by op."""
    a, b, c, d = (np.asarray(x, dt) for x in (a, b, c, d))
    b1, b2, b3 = a - b, b - c, c - d
    n1 = _cross(b1, b2)
    n1 = n1 / _norm(n1)[..., None]
    n2 = _cross(b2, b3)
    n2 = n2 / _norm(n2)[..., None]
    m1 = _cross(n1, b2 / _norm(b2)[..., None])
    return np.arctan2(_dot(m1, n2), _dot(n1, n2)) * dt(180.0) / dt(3.14159265358979323846)


def planar_deg(a, b, c, dt):
    """coords6d.py:46-58 in dtype dt."""
    a, b, c = (np.asarray(x, dt) for x in (a, b, c))
    v1, v2 = a - b, c - b
    return np.arccos(_dot(v1, v2) / (_norm(v1) * _norm(v2))) * dt(180.0) / dt(3.14159265358979323846)


def pair_index(i, j, R, L, mutant=None):
    """Index of the intra-chain ordered pair (i, j) in the layer-0 table: the receptor block [R][R], then the ligand block [L][L].
    mutant 'blocks_swapped': the ligand block first."""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    if mutant == "blocks_swapped":
        return np.where(i < R, L * L + i * R + j, (i - R) * L + (j - R))
    return np.where(i < R, i * R + j, R * R + (i - R) * L + (j - R))


def edge_ref(n4, ca4, cb4, i, j, R, mask_dist, mutant=None):
    """Features of the ordered pairs (i, j) of ONE trajectory.  Exact (fp32 restatement): r2, the distance bin `bd`, relpos `rp`, the
    gate d < mask_dist and i != j.  Angles omega / theta / phi in float64 from the same fp32 inputs (`a64`) and in numpy fp32 (`a32`).
    mutant 'ge': >= instead of > at the distance-bin boundaries.
    Non-finite coordinates, with IEEE comparisons as the kernel makes them: a NaN distance passes no `>` (distance bin 0) and not the gate
    (angle bins 0); a distance of +inf passes all 39 and not the gate; relpos is index arithmetic and stays exact; r2 is NaN or +inf."""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    n, ca, cb = (np.asarray(x, f32)[:, :3] for x in (n4, ca4, cb4))
    with np.errstate(invalid="ignore"):
        dv = ca[i] - ca[j]
        r2 = (dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2]
        d = np.sqrt(r2)
        cmp = np.greater_equal if mutant == "ge" else np.greater
        bd = cmp(d[:, None], DIST_BOUNDS[None, :]).sum(1)
        gate = (d < f32(mask_dist)) & (i != j)
    same = (i < R) == (j < R)
    rp = np.where(same, np.clip(i - j + 32, 0, 64), 65)
    out = dict(r2=r2, bd=bd, rp=rp, gate=gate)
    with np.errstate(invalid="ignore", divide="ignore"):
        for dt, key in ((np.float64, "a64"), (f32, "a32")):
            out[key] = np.stack([dihedral_deg(ca[i], cb[i], cb[j], ca[j], dt), dihedral_deg(n[i], ca[i], cb[i], cb[j], dt),
                                 planar_deg(ca[i], cb[i], cb[j], dt)], -1)
    return out


def unpack_code(code):
    code = np.asarray(code, np.uint32)
    return dict(bd=code & 63, om=(code >> 6) & 31, th=(code >> 11) & 31, ph=(code >> 16) & 15, rp=code >> 20)


def angle_margin(ref):
    """m = four times the largest difference between the numpy fp32 restatement and float64 over the gated edges."""
    g = ref["gate"]
    with np.errstate(invalid="ignore"):
        dlt = np.abs(f64(ref["a32"][g]) - ref["a64"][g])
    dlt = np.where(dlt > 180.0, 360.0 - dlt, dlt)      # the two sides of the +-180 wrap
    return 4.0 * float(np.nanmax(dlt)) if dlt.size and np.isfinite(dlt).any() else 0.0


def _bins(a, bounds):
    with np.errstate(invalid="ignore"):
        return (a[:, None] > f64(bounds)[None, :]).sum(1)      # NaN compares false: bin 0


def angle_undecided(ref, m):
    """[n][3] bool: gated, and the float64 angle within m of a boundary (the 23 angle bounds / 18 q; +-180 are among the first)."""
    out = np.zeros(ref["a64"].shape, bool)
    for k, bounds in enumerate((ANGLE_BOUNDS, ANGLE_BOUNDS, PHI_BOUNDS)):
        a = ref["a64"][:, k]
        with np.errstate(invalid="ignore"):
            out[:, k] = ref["gate"] & (np.abs(a[:, None] - f64(bounds)[None, :]) <= m).any(1)
    return out


def assert_same_f32(got, want):
    """Bit for bit, +inf / -inf included; where `want` is NaN, `got` is a NaN (sign and payload of a NaN are not part of any contract)."""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def check_edge_codes(codes, radial, ref, m):
    """codes / radial of a launch against edge_ref: radial, distance bin and relpos exact; masked pairs have the three angle bins 0; a
    decided angle has the float64 bin (NaN: 0); an undecided one has one of the bins within m of it (across the +-180 wrap for the
    dihedrals).  Returns the number of undecided edges."""
    f = unpack_code(codes)
    assert_same_f32(radial, ref["r2"])
    np.testing.assert_array_equal(f["bd"], ref["bd"])
    np.testing.assert_array_equal(f["rp"], ref["rp"])
    und = angle_undecided(ref, m)
    for k, (name, bounds) in enumerate((("om", ANGLE_BOUNDS), ("th", ANGLE_BOUNDS), ("ph", PHI_BOUNDS))):
        a = ref["a64"][:, k]
        want = np.where(ref["gate"], _bins(a, bounds), 0)
        dec = ~und[:, k]
        np.testing.assert_array_equal(f[name][dec], want[dec], err_msg=name)
        if (~dec).any():
            x, g = a[~dec], f[name][~dec].astype(np.int64)
            wrap = lambda v: (v + 180.0) % 360.0 - 180.0
            alts = [x, x - m, x + m] + ([wrap(x - m), wrap(x + m)] if k < 2 else [])
            ok = np.zeros(g.shape, bool)
            for v in alts:
                ok |= g == _bins(v, bounds)
            assert ok.all(), f"{name}: an undecided edge has a bin that is not adjacent"
    return int(und.any(1).sum())


def all_pairs(R, L):
    """(i, j) of every intra-chain ordered pair: the receptor block, then the ligand block."""
    ii = np.concatenate([np.repeat(np.arange(R), R), R + np.repeat(np.arange(L), L)])
    jj = np.concatenate([np.tile(np.arange(R), R), R + np.tile(np.arange(L), L)])
    return ii, jj


def check_pairs(code0, rows, R, L, codes, radial, mutant=None):
    """k_l0_pairs: rows[q] = (i, j, code, r2 bits) and code0[q] = (code, r2 bits) at q = pair_index(i, j) for every intra-chain ordered
    pair, with (codes, radial) the features of those pairs in (i, j) order [receptor pairs, then ligand pairs]."""
    ii, jj = all_pairs(R, L)
    q = pair_index(ii, jj, R, L, mutant)
    rows, code0 = np.asarray(rows, np.uint32).reshape(-1, 4), np.asarray(code0, np.uint32).reshape(-1, 2)
    assert rows.shape[0] == R * R + L * L == code0.shape[0]
    r2b = np.asarray(radial, f32).view(np.uint32)
    np.testing.assert_array_equal(rows[q], np.stack([ii, jj, codes, r2b], 1).astype(np.uint32))
    np.testing.assert_array_equal(code0[q], np.stack([codes, r2b], 1).astype(np.uint32))
    return ii, jj


def check_graph(edges, ca4, knn, nsamp, seed, stream, envelope, cap=0.02):
    """edges [B][N][knn + nsamp] of one k_knn_sample launch: kNN slots exact (check_knn), sampled slots against the float64 race with the
    given log2 envelope (check_sampled: decided nodes exactly).  At most cap B N nodes may be undecided; returns their number.
    Whatever the coordinates, every edge is a residue index, and the order is the ordering rule of the graph (order_word)."""
    B, N = ca4.shape[:2]
    edges = np.asarray(edges)
    assert ((edges >= 0) & (edges < N)).all(), "an edge is no residue index"
    und = 0
    for b in range(B):
        d = dist32(ca4[b, :, :3])
        near = knn_ref(d, knn)
        check_knn(edges[b, :, :knn], near)
        if nsamp:
            key, bound = race_keys(d, near, edge_stream_u(b * N + np.arange(N), N, stream, seed), envelope)
            und += check_sampled(edges[b, :, knn:], near, key, bound, nsamp)
    assert und <= cap * B * N, f"{und} undecided nodes of {B * N}"
    return und


def ref_graph(ca4, knn, nsamp, seed, stream):
    """The reference's own edges [B][N][knn + nsamp] by the ordering rule, float64 race keys: in-range index lists for the kernels
    downstream of k_knn_sample that owe nothing to the kernel under test."""
    B, N = ca4.shape[:2]
    out = np.zeros((B, N, knn + nsamp), np.int32)
    for b in range(B):
        d = dist32(ca4[b, :, :3])
        near = knn_ref(d, knn)
        key, _ = race_keys(d, near, edge_stream_u(b * N + np.arange(N), N, stream, seed), LOG2_ENVELOPE)
        out[b] = np.concatenate([near, sample_ref(key, nsamp, near=near)], 1)
    return out


def hit_ref(i, j, codes, radial, code0, R, L, mutant=None):
    """The table-hit predicate of k_edge_feat<1>: both residues of one chain, the entry's code equal, |r2_entry - r2| <= 1e-3 max(sqrt(r2),
    1) in fp32.  mutant 'no_sqrt': tolerance 1e-3.  Returns (hit, pair index)."""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    same = (i < R) == (j < R)
    idx = np.where(same, pair_index(i, j, R, L), 0)
    c0 = np.asarray(code0, np.uint32).reshape(-1, 2)[idx]
    r2 = np.asarray(radial, f32)
    with np.errstate(invalid="ignore"):      # a pair whose r2 is NaN or inf is never a hit (mutant 'inf_hits': inf <= inf passes)
        tol = f32(1e-3) * (f32(1.0) if mutant == "no_sqrt" else np.maximum(np.sqrt(r2), f32(1.0)))
        hit = same & (c0[:, 0] == np.asarray(codes, np.uint32)) & (np.abs(c0[:, 1].copy().view(f32) - r2) <= tol)
    if mutant != "inf_hits":
        hit &= np.isfinite(r2)
    return hit, idx


def check_classification(src, rows, counter, start, i, j, codes, radial, hit, idx):
    """Every edge: src = the pair index (a hit) or 0x80000000 | at with rows[at] = (i, j, code, r2 bits); the positions are exactly
    0 .. misses - 1 past `start`; the counter ends at start + misses.  Returns the number of misses."""
    src, rows = np.asarray(src, np.uint32), np.asarray(rows, np.uint32).reshape(-1, 4)
    np.testing.assert_array_equal(src[hit], idx[hit].astype(np.uint32))
    miss = ~hit
    n = int(miss.sum())
    assert (src[miss] & MISS).all(), "a miss without the row-list flag"
    at = (src[miss] & 0x7FFFFFFF).astype(np.int64)
    np.testing.assert_array_equal(np.sort(at), start + np.arange(n))
    want = np.stack([np.asarray(i)[miss], np.asarray(j)[miss], np.asarray(codes, np.uint32)[miss],
                     np.asarray(radial, f32).view(np.uint32)[miss]], 1).astype(np.uint32)
    np.testing.assert_array_equal(rows[at], want)
    rest = np.ones(rows.shape[0], bool)
    rest[at] = False
    assert is_sentinel(rows[rest]).all(), "a row outside the reserved positions was written"
    assert int(counter) == start + n
    return n


# ---- clash force -----------------------------------------------------------------------------------------------------------------
def clash_ref(rec, lig):
    """get_clash_force (inference_base.py:366-384) in float64: E = -5 sum_{0 < d < 4} (4 - d)^1.5 / (0.75 d) over all backbone-atom
    pairs; the shift is the mean over the 3 L ligand atoms of dE/dx.  rec [R][9], lig [B][L][9] -> (shift [B][3], scale [B][3]) with
    scale = the same mean over |terms|."""
    r = f64(rec).reshape(-1, 3)
    out, sc = [], []
    for lb in f64(lig):
        x = lb.reshape(-1, 3)
        dv = r[:, None, :] - x[None, :, :]
        d = np.sqrt((dv * dv).sum(-1))
        ok = (d < 4.0) & (d > 0.0)
        ds = np.where(ok, d, 1.0)
        u = np.where(ok, 4.0 - ds, 0.0)
        dE = np.where(ok, -5.0 * (-1.5 * np.sqrt(u) * ds - u * np.sqrt(u)) / (0.75 * ds * ds), 0.0)
        t = dE[..., None] * (-dv / ds[..., None])
        out.append(t.sum((0, 1)) / x.shape[0])
        sc.append(np.abs(t).sum((0, 1)) / x.shape[0])
    return np.array(out), np.array(sc)


# ---- initial pose ----------------------------------------------------------------------------------------------------------------
def quat_to_mat64(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def init_draws64(b, seed):
    """The native draws of trajectory b (inference_base.py:318-340; scipy Rotation.random: a normalised Gaussian quaternion (x, y, z, w);
    translation 30 N(0, I)): Philox blocks (b, 0..3, 0, RNG_INIT), Box-Muller sqrt(-2 ln u_a) cos(2 pi u_b) on word pairs, in float64.
    Returns (q [4], draw [3], |dz| bounds of the seven normals, the first uniforms of the pairs)."""
    w = np.stack(philox_np(np.full(4, b), np.arange(4), 0, RNG_INIT, seed & 0xFFFFFFFF, seed >> 32), -1)      # [block][word]
    u = f64(u01_np(w))
    ua = np.array([u[0, 0], u[0, 2], u[1, 0], u[1, 2], u[2, 0], u[2, 2], u[3, 0]])
    ub = np.array([u[0, 1], u[0, 3], u[1, 1], u[1, 3], u[2, 1], u[2, 3], u[3, 1]])
    r = np.sqrt(-2.0 * np.log(ua))
    z = r * np.cos(2 * np.pi * ub)
    # logf 1 ulp (2 u), x 2 exact, sqrtf halves it and rounds: 2 u r; the argument 2 pi u_b carries 2 roundings (<= 2 u 2 pi absolute),
    # cosf 2 ulp of a value <= 1: (4 pi + 4) u; the product rounds once more
    dz = r * (4 * np.pi + 4) * U + 3 * U * np.abs(z) + 2 * U * r
    return z[:4], 30.0 * z[4:], dz, ua


def centroid64(x, all_atoms):
    x = f64(x).reshape(-1, 3, 3)
    return x.reshape(-1, 3).mean(0) if all_atoms else x[:, 1].mean(0)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def chain_coords(B, N, seed=0, step=3.8, confine=None):
    """A random synthetic CA chain per trajectory: a 3.8 A random walk (confined to a ball of radius `confine` by reflection), fp32 [B][N][4]."""
    rng = np.random.default_rng([seed, B, N, 1])
    confine = confine or 4.0 * max(N, 8) ** (1.0 / 3.0)
    ca = np.zeros((B, N, 4), f32)
    for b in range(B):
        v = rng.standard_normal((N, 3))
        v *= step / np.linalg.norm(v, axis=1, keepdims=True)
        p = np.zeros(3)
        for k in range(N):
            q = p + v[k]
            if np.linalg.norm(q) > confine:
                q = p - v[k]
            p = q
            ca[b, k, :3] = p
    return ca


def lattice_coords(B, N, seed=0):
    """CA on an integer lattice with about four sites per residue: every squared distance is a small integer, so many distances are
    exactly equal (shells) and the tie branch of the selection runs on most nodes; some sites are taken twice (coincident residues)."""
    rng = np.random.default_rng([seed, B, N, 2])
    span = max(1, int(round((4.0 * N) ** (1.0 / 3.0) / 2.0)))
    ca = np.zeros((B, N, 4), f32)
    ca[..., :3] = rng.integers(-span, span + 1, (B, N, 3))
    return ca


def coincident_coords(B, N, seed=0):
    """A chain in which a few residues coincide with an earlier one (and one triple)."""
    ca = chain_coords(B, N, seed + 7)
    rng = np.random.default_rng([seed, B, N, 3])
    for b in range(B):
        for _ in range(min(4, N // 3)):
            a, c = rng.integers(0, N, 2)
            ca[b, c] = ca[b, a]
        if N >= 6:
            ca[b, N - 1] = ca[b, N // 2] = ca[b, 0]
    return ca


def _words(*w):
    return np.array(w, np.uint32).view(f32)


def bad_trajectory(B):
    """The one trajectory of a non-finite geometry that holds the non-finite coordinates: 1 (of B = 3), 0 when there is one only."""
    return min(1, B - 1)


def _nonfinite(fill):
    def make(B, N, seed=0):
        ca = chain_coords(B, N, seed)
        fill(ca[bad_trajectory(B)], N // 2, N)
        return ca
    return make


def _nan_residue(ca, R, N):
    ca[R + (N - R) // 3, 1] = np.nan      # one coordinate of one ligand CA


def _inf_residue(ca, R, N):
    ca[R // 2, 0] = np.inf                # one receptor residue at +inf, one ligand residue at -inf
    ca[N - 1, 2] = -np.inf


def _ligand(*words):
    def fill(ca, R, N):
        ca[R:, :3] = _words(*words)[(np.arange(N - R)[:, None] + np.arange(3)[None, :]) % len(words)]      # rotated from residue to residue
    return fill


# Non-finite geometries (trajectory bad_trajectory(B) of the random chain; the others stay finite).  R = N // 2 is the receptor.
NONFINITE = {"nan_residue": _nonfinite(_nan_residue),                             # one CA of the ligand half is NaN
             "nan_ligand": _nonfinite(_ligand(0x7FC00000)),                       # every coordinate behind R is +NaN
             "neg_nan_ligand": _nonfinite(_ligand(0xFFC00000)),                   # ... is the NaN with the sign bit set
             "payload_nan": _nonfinite(_ligand(0x7F800001, 0xFFBFFFFF, 0x7FFFFFFF)),      # signalling, negative, all ones
             "inf_residue": _nonfinite(_inf_residue)}
COORDS = {"chain": chain_coords, "lattice": lattice_coords, "coincident": coincident_coords, **NONFINITE}
NONFINITE_SIZES = (16, 40, 214, 255, 256, 257, 600, 1030)      # 16: the degree clamps; 1030: NPL = 32, the vector-pipe count
NONFINITE_DEGREES = ((20, 40), (60, 0))


def finite_twin(kind, B, N, seed=0):
    """The same launch with the bad trajectory made finite: the chain the non-finite geometry was cut from."""
    return chain_coords(B, N, seed)

KNN_SIZES_SMALL = (1, 19, 20, 21, 59, 60, 61)
KNN_SIZES_LARGE = (256, 257, 512, 513, 768, 769, 1024, 1025, 2048, 2049)
# NPL = 64 holds candidate j in mask bit 4 (j / 256) + j % 4 of lane (j / 4) % 64: N = 2049 reaches bit 35 only, the largest complex
# (MAX_NODES = 4096 = 4 x 64 x 16 candidates) fills all 64 bits.  4093 is odd (the early wave exit); 4133 is past the capacity: refused.
KNN_SIZES_TOP = (4093, 4096)
KNN_N_REFUSED = 4133
DEGREES = ((20, 40), (10, 0), (1, 59), (32, 28), (33, 27), (60, 0))
DEGREE_SIZES = (61, 257, 513, 769, 1025, 2049)     # one N per instantiation (NPL 4, 8, 12, 16 -> 1025: 32, 64) for the other degrees


def batch_of(N):
    """B = 3 at the small sizes, 1 or 2 at the large ones; B N is no multiple of 4 at least once in every NPL class."""
    if N <= 61:
        return 3
    return 1 if N >= 2048 or N % 2 == 0 else 2 if (2 * N) % 4 else 1


def knn_cases():
    """(kind, N, B, knn, nsamp) of every k_knn_sample launch the GPU tests compare with the references."""
    out = []
    for N in KNN_SIZES_SMALL + KNN_SIZES_LARGE:
        for kind in ("chain", "lattice"):
            out.append((kind, N, batch_of(N), 20, 40))
    for N in (21, 61, 513, 769, 1025):
        out.append(("coincident", N, batch_of(N), 20, 40))
    for N in DEGREE_SIZES:
        for knn, ns in DEGREES[1:]:
            out.append(("lattice" if N in (61, 769) else "chain", N, batch_of(N), knn, ns))
    out.append(("chain", KNN_SIZES_TOP[0], 1, 20, 40))
    out.append(("lattice", KNN_SIZES_TOP[1], 1, 20, 40))
    out.append(("chain", KNN_SIZES_TOP[1], 1, 33, 27))
    return out


def knn_case_id(c):
    return f"{c[0]}-N{c[1]}-B{c[2]}-k{c[3]}-s{c[4]}"


def backbone(ca4, seed=0, collinear=()):
    """(n4, ca4, cb4) [B][N][4] from CA coordinates: N and C at random offsets of 1.46 / 1.52 A, the virtual CB of coords6d.py:71-75 in fp32
    with the engine's expression order (dfm_device.h: prep_pose_block).  Residues in `collinear` get N, CA, C on one axis-parallel line:
    b x c = 0 exactly, CB lies on the line and theta is NaN."""
    rng = np.random.default_rng([seed, 4])
    ca = np.asarray(ca4, f32)[..., :3]

    def off(r):
        v = rng.standard_normal(ca.shape)
        return (v * (r / np.linalg.norm(v, axis=-1, keepdims=True))).astype(f32)
    with np.errstate(invalid="ignore"):      # (a signalling NaN among the coordinates)
        n, c = ca + off(1.46), ca + off(1.52)
    for k in collinear:
        n[:, k] = ca[:, k] + np.array([-1.5, 0, 0], f32)
        c[:, k] = ca[:, k] + np.array([1.5, 0, 0], f32)
    return backbone_from_pos(np.stack([n, ca, c], -2))


def backbone_from_pos(pos):
    """(n4, ca4, cb4) of backbone coordinates pos [B][N][3 atoms][3]: Cb = -0.58273431 a + 0.56802827 b - 0.54067466 c + Ca with b = Ca - N,
    c = C - Ca, a = b x c (coords6d.py:71-75), in fp32 in the engine's expression order."""
    pos = np.asarray(pos, f32)
    n, ca, c = pos[..., 0, :], pos[..., 1, :], pos[..., 2, :]
    with np.errstate(invalid="ignore"):
        b, cc = ca - n, c - ca
        a = _cross(b, cc)
        cb = ((f32(-0.58273431) * a + f32(0.56802827) * b) - f32(0.54067466) * cc) + ca
    pad = lambda x: np.concatenate([x, np.zeros(x.shape[:-1] + (1,), f32)], -1).astype(f32)
    return pad(n), pad(ca), pad(cb)


def boundary_pose(N, R):
    """One trajectory on a quarter-Angstrom lattice (squared distances exact in fp32) whose first residues sit at distances that equal
    bin boundaries 3.25 + 1.25 q exactly (3.25, 4.5, 7 twice, 12, 17, 22 = the mask distance of the first family) from residue 0; two
    coincident residues with the same backbone (omega NaN) and one collinear backbone (theta NaN)."""
    rng = np.random.default_rng([N, R, 5])
    ca = np.zeros((1, N, 4), f32)
    ca[0, :, :3] = rng.integers(-40, 41, (N, 3)) * 0.25
    special = [(0, 0, 0), (3.25, 0, 0), (0, 4.5, 0), (7, 0, 0), (2, 3, 6), (0, 0, 12), (8, 15, 0), (22, 0, 0), (0, 20, 0)]
    for k, p in enumerate(special[:N]):
        ca[0, k, :3] = p
    n4, ca4, cb4 = backbone(ca, seed=N, collinear=(2,) if N > 2 else ())
    if N > 12:
        for x in (n4, ca4, cb4):
            x[0, 11] = x[0, 10]
    return n4, ca4, cb4


def random_edges(rng, B, N, K):
    """Random index lists [B][N][K]: i = j in slot 0, any residue of either chain elsewhere."""
    e = rng.integers(0, N, (B, N, K)).astype(np.int32)
    e[:, :, 0] = np.arange(N)[None, :]
    return e


def edge_ij(edges, N, K):
    """(b, i, j) of every edge of edges [B][N][K], flattened."""
    e = np.asarray(edges).reshape(-1)
    node = np.arange(e.size) // K
    return node // N, node % N, e.astype(np.int64)


EDGE_CASES = (("boundary", 51, 20, 5, 22.0), ("boundary", 64, 33, 4, 20.0), ("boundary", 257, 100, 1, 22.0),
              ("chain", 70, 40, 60, 22.0), ("chain", 300, 130, 7, 20.0))      # (pose, N, R, K, mask_dist); N K = 255, 256, 257, ...


def edge_case(pose, N, R, K, mask_dist):
    """Inputs of one k_edge_feat<0> launch with random index lists (B = 1 for the boundary pose, 2 for the chain, whose relpos offsets
    pass -32 and +32 in both chain orders)."""
    rng = np.random.default_rng([N, R, K, 6])
    if pose == "boundary":
        n4, ca4, cb4 = boundary_pose(N, R)
    else:
        n4, ca4, cb4 = backbone(chain_coords(2, N, seed=3), seed=1)
    B = ca4.shape[0]
    edges = random_edges(rng, B, N, K)
    if pose == "boundary":
        edges[0, 0, :min(K, 9)] = np.arange(min(K, 9))      # residue 0 against the residues on the boundaries, and back
        edges[0, 1:9, K - 1] = 0
        if N > 12:
            edges[0, 10, K - 1] = 11
    return dict(n4=n4, ca4=ca4, cb4=cb4, edges=edges, B=B, N=N, R=R, K=K, mask_dist=mask_dist)


def edge_case_ref(c):
    """edge_ref over the trajectories of an edge case, concatenated in edge order."""
    b, i, j = edge_ij(c["edges"], c["N"], c["K"])
    parts = [edge_ref(c["n4"][t], c["ca4"][t], c["cb4"][t], i[b == t], j[b == t], c["R"], c["mask_dist"]) for t in range(c["B"])]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


PAIR_SIZES = ((1, 1), (5, 3), (17, 16), (64, 31))
CLASSIFY_TOTALS = ((1, 1, 1, 1), (1023, 341, 3, 200), (1024, 256, 4, 100), (1025, 205, 5, 105), (5127, 1709, 3, 1000))      # total, N, K, R


def classify_case(N, K, R, mode="mixed"):
    """Inputs of one k_edge_feat<1> launch at B = 1 (total = N K edges): a chain pose, its own kind of edges mixed with random lists.
    mode 'mixed': random pairs; 'first_clean': the first 1024 edges are intra-chain pairs (no miss in the first workgroup unless
    planted); 'all_miss': every edge is an inter-chain pair."""
    rng = np.random.default_rng([N, K, R, 8])
    n4, ca4, cb4 = backbone(chain_coords(1, N, seed=5), seed=2)
    L = N - R
    edges = random_edges(rng, 1, N, K)
    i = np.repeat(np.arange(N), K)
    if mode == "all_miss":
        edges = np.where(i < R, R + edges.reshape(-1) % max(L, 1), edges.reshape(-1) % max(R, 1)).astype(np.int32).reshape(1, N, K)
    elif mode == "first_clean":
        e = edges.reshape(-1)
        same = np.where(i < R, e % max(R, 1), R + e % max(L, 1))
        e[:1024] = same[:1024]
        edges = e.reshape(1, N, K).astype(np.int32)
    return dict(n4=n4, ca4=ca4, cb4=cb4, edges=edges, B=1, N=N, R=R, L=L, K=K, mask_dist=22.0)


def plant(code0, radial_of_pair, rng, skip_below=0):
    """Plants in a copy of code0 [P][2]: every 7th entry gets one code field changed (the five fields in turn), every 11th its r2 moved by
    2 x the tolerance 1e-3 max(sqrt(r2), 1) (a miss), every 13th by 0.5 x (still a hit).  Entries below skip_below stay."""
    c = np.array(code0, np.uint32).reshape(-1, 2).copy()
    r2 = np.asarray(radial_of_pair, f32)
    tol = f32(1e-3) * np.maximum(np.sqrt(r2), f32(1.0))
    q = np.arange(c.shape[0])
    live = q >= skip_below
    shifts = np.array([0, 6, 11, 16, 20], np.uint32)
    m7 = live & (q % 7 == 3)
    c[m7, 0] ^= (np.uint32(1) << shifts[(q[m7] // 7) % 5])
    m11 = live & (q % 11 == 5) & ~m7
    c[m11, 1] = (r2[m11] + f32(2.0) * tol[m11]).astype(f32).view(np.uint32)
    m13 = live & (q % 13 == 6) & ~m7 & ~m11
    c[m13, 1] = (r2[m13] + f32(0.5) * tol[m13]).astype(f32).view(np.uint32)
    return c


CLASH_SIZES = ((5, 3), (300, 40), (1025, 7), (9, 342), (1030, 345))      # (R, L): second receptor chunk from R = 1025, second ligand atom
                                                                          # per thread from L = 342


def clash_case(R, L, B=3, seed=0):
    """Receptor and B ligand poses (different rigid shifts of one ligand) interleaved on a 3 A grid so that a fraction of the atom pairs
    lies inside 4 A; a coincident pair (d = 0, skipped) and pairs just outside 4 A but inside the fp32 prefilter (16 < d^2 < 16.5)."""
    rng = np.random.default_rng([seed, R, L, 9])
    side = int(np.ceil((3 * (R + L)) ** (1.0 / 3.0))) + 1
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pick = rng.permutation(len(grid))[:3 * (R + L)]
    pts = (grid[pick] * 3.0 + rng.uniform(-0.6, 0.6, (3 * (R + L), 3))).astype(f32)
    rec = pts[:3 * R].reshape(R, 9).copy()
    lig0 = pts[3 * R:].reshape(L, 9).copy()
    lig = np.stack([lig0 + np.tile(rng.uniform(-0.5, 0.5, 3), 3).astype(f32) for _ in range(B)]).astype(f32)
    lig[0, 0, :3] = rec[0, :3]                                             # coincident: d = 0
    lig[B - 1, L - 1, 6:9] = rec[R - 1, 6:9] + np.array([4.03, 0, 0], f32)      # d^2 = 16.24: passes the prefilter, no force
    lig[B - 1, L - 1, 3:6] = rec[R - 1, 3:6] + np.array([0, 4.0, 0.1], f32)     # d^2 = 16.01
    tr0 = (rng.standard_normal((B, 3)) * 5).astype(f32)
    return dict(rec=rec, lig=lig, tr0=tr0, R=R, L=L, B=B)


def init_case(L, R=40, B=5, seed=0):
    """Inputs of k_init_pose: a receptor, a ligand, injected rotations of angles in (0.2, 2.4) about random axes and injected draws."""
    rng = np.random.default_rng([seed, L, 10])
    rec = (rng.standard_normal((R, 9)) * 8 + 5).astype(f32)
    lig = (rng.standard_normal((L, 9)) * 6 - 20).astype(f32)
    R0 = np.zeros((B, 9), f32)
    for b in range(B):
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        th = rng.uniform(0.2, 2.4)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R0[b] = (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)).reshape(9)
    draw = (rng.standard_normal((B, 3)) * 30).astype(f32)
    return dict(rec=rec, lig=lig, R0=R0, draw=draw, R=R, L=L, B=B)


# ---- a uniform of exactly 1.0f ------------------------------------------------------------------------------------------------------
# u01's largest value is 1.0f (x >> 8 = 0xFFFFFF: 16777215.5 rounds to 2^24).  Found with Harness.find_top_uniform (a bounded search of
# at most 2^26 Philox blocks; tests/test_geom_harness_cpu.py repeats the search and checks both records):
TOP_UNIFORM_SEED = 1
TOP_UNIFORM_EDGE = (230, 76, 12, 1)      # (evaluation index, node b N + i at N = 61, block j / 4, word j % 4): candidate j = 49 of node 15 of trajectory 1
TOP_UNIFORM_INIT_SEED = 37388            # k_init_pose: block 0, word 0 of trajectory 3 - the first uniform of its first normal
TOP_UNIFORM_INIT_B = 3


def top_uniform_coords():
    """B = 3 chains of 61 residues in which candidate 49 is none of the 20 nearest of node 15 (so it takes part in the race)."""
    return chain_coords(3, 61, seed=61)
