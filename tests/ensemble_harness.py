"""Kernel-level harness of the clustering and consensus kernels (tests/kernels/ensemble_harness.hip): k_pose_dist, k_cluster_leader,
k_cluster_count, k_cluster_pick and k_cluster_dec of kernels_cluster.hip, k_contact_bits, k_contact_count, k_contact_marginals and
k_contact_score of kernels_consensus.hip, launch by launch.

The shim drives the shipped launchers of dfmdock_amd/libdfmdock_amd.so under the guard-band protocol of tests/kernel_harness.py, after
checking every array, permutation and index a launch follows.  This module binds it and holds
  * the definitions the kernels are held to: cluster.pose_rmsd / cluster.cluster_adjacency and consensus.contacts / from_contacts /
    consensus, in float64 on the fp32 inputs, and `device_bits`, the device layout [n][W][R] written from the header's words;
  * numpy restatements of the kernels (restate_pose: the fp32 chain of k_pose_dist bit for bit; restate_leader / restate_count /
    restate_step / restate_size_full: the two rules with their intermediate state; restate_contact_bits / restate_contact_count /
    restate_contact_score), each with seeded mutants that tests/test_ensemble_harness_cpu.py turns the comparisons on;
  * the comparisons the GPU tests use (check_*), and the input generators, so that the CPU tests can check the border caps and the
    restatements on the very inputs the GPU tests use.

Gates.
  k_pose_dist      against float64: |got - ref| <= (D / 2 + 4) 2^-24 ref with D = 9 n_res (one rounding in d, none in the fma's product,
                   D - 1 in the running sum, one each for inv_atoms, the multiply and the root, the sum's error halved by the root:
                   D / 2 + 3, one to spare); diagonal exactly 0, bitwise symmetric.  Against the restatement: every RMSD and every mask
                   bit equal bit for bit.  Mask against float64: equal to r64 <= radius outside a border of that relative width around
                   the radius; border pairs at most 0.5 % of the generic pairs and none of the lattice pairs.
  clustering       everything an integer: n, center, size, cluster_of, counts on U, U, state exact; mlist as a set.
  consensus        every word of k_contact_bits equals the definition, no border; every count and sum array_equal.
"""
import ctypes as C
import fractions
import functools

import numpy as np

import kernel_harness as kh
from kernel_harness import HIP_INVALID_VALUE, HIP_SUCCESS, LIBDIR, ROOT, Out, guards_intact, is_sentinel      # noqa: F401 (re-exported)

LAUNCHERS = ("_ZN3dfm16launch_pose_distEPKfiiPKiifPfPjP12ihipStream_t",
             "_ZN3dfm21launch_cluster_leaderEPKjiPKiiPiS4_S4_S4_P12ihipStream_t",
             "_ZN3dfm20launch_cluster_countEPKjiPiPjS2_S2_P12ihipStream_t",
             "_ZN3dfm19launch_cluster_stepEPKjiPiPKiS4_PjS2_S2_S2_S2_S2_P12ihipStream_t",
             "_ZN3dfm19launch_contact_bitsEPKfS1_iiifPmP12ihipStream_t",
             "_ZN3dfm20launch_contact_countEPKmPKhiiiPiS4_S4_P12ihipStream_t",
             "_ZN3dfm20launch_contact_scoreEPKmPKiiiiPiPlP12ihipStream_t")
SLOTS = ("X", "res", "rmsd", "mask", "order", "pos", "counts", "U", "cluster_of", "center", "size", "n_out", "mlist", "state",
         "rec", "lig", "bits", "member", "count", "rec_count", "lig_count", "n_contacts", "score_sum")
INTS = ("B", "L", "n_res", "max_clusters", "n", "R")
OPS = ("pose_rmsd", "pose_mask", "leader", "count", "step", "size_full", "contact_bits", "contact_count", "contact_score", "consensus_full")
U32 = 2.0 ** -24                  # unit roundoff of fp32
BORDER_CAP = 0.005                # at most this share of a generic generator's pairs may lie in the border around the radius
PT, KC, STRIDE = 64, 32, 1024     # k_pose_dist: poses per tile edge, coordinates per LDS chunk; k_cluster_leader: ranks per scan stride
SENT32 = np.uint32(0xffffffff)

f32, i32, u32, u64 = np.float32, np.int32, np.uint32, np.uint64


class Call(C.Structure):
    _fields_ = [("buf", kh.Buf * len(SLOTS)), ("radius", C.c_float), ("cutoff", C.c_float)] + [(n, C.c_int) for n in INTS]


compile_shim = functools.partial(kh.compile_shim, "ensemble")


def rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ---- binding -------------------------------------------------------------------------------------------------------------------------
STEP_KEYS = ("counts", "U", "cluster_of", "center", "size", "mlist", "state")


class Harness(kh.KernelHarness):
    check = True      # run() asserts success unless told check=False

    def __init__(self, path):
        super().__init__(path, Call, SLOTS, OPS)

    @staticmethod
    def _pose_args(x, res):
        x = np.ascontiguousarray(x, f32)
        B, L = x.shape[0], x.shape[1]
        res = None if res is None else np.ascontiguousarray(res, i32)
        return x, res, dict(B=B, L=L, n_res=L if res is None else res.size)

    def pose_rmsd(self, x, res=None):
        """k_pose_dist in its evaluation mode: x [B, L, 9] -> [B, B] float32."""
        x, res, sc = self._pose_args(x, res)
        B = sc["B"]
        return self.run("pose_rmsd", dict(X=x, res=res, rmsd=Out(f32, B * B)), radius=1.0, **sc)["rmsd"].reshape(B, B)

    def pose_mask(self, x, radius, res=None):
        """k_pose_dist's bitmask: [B, ceil(B / 32)] uint32."""
        x, res, sc = self._pose_args(x, res)
        B = sc["B"]
        return self.run("pose_mask", dict(X=x, res=res, mask=Out(u32, B * words32(B))), radius=f32(radius), **sc)["mask"].reshape(B, -1)

    def leader(self, mask, order, max_clusters):
        B = mask.shape[0]
        cap = min(max_clusters, B)
        r = self.run("leader", dict(mask=mask, order=np.ascontiguousarray(order, i32), cluster_of=Out(i32, B), center=Out(i32, cap),
                                    size=Out(i32, cap), n_out=Out(i32, 1)), B=B, max_clusters=max_clusters)
        return dict(n=int(r["n_out"][0]), center=r["center"], size=r["size"], cluster_of=r["cluster_of"])

    def count(self, mask):
        B = mask.shape[0]
        r = self.run("count", dict(mask=mask, counts=Out(i32, B), U=Out(u32, words32(B)), cluster_of=Out(i32, B), state=Out(i32, 3)), B=B)
        return {k: r[k] for k in ("counts", "U", "cluster_of", "state")}

    def step(self, mask, pos, order, st, max_clusters):
        """One pick + decrement on the state st (STEP_KEYS; center / size hold min(max_clusters, B) entries): the state after it."""
        B = mask.shape[0]
        bufs = dict(mask=mask, pos=np.ascontiguousarray(pos, i32), order=np.ascontiguousarray(order, i32))
        bufs.update({k: Out(u32 if k == "U" else i32, init=st[k]) for k in STEP_KEYS})
        r = self.run("step", bufs, B=B, max_clusters=max_clusters)
        return {k: r[k] for k in STEP_KEYS}

    def size_full(self, mask, pos, order, max_clusters):
        """count, then min(max_clusters, B) steps."""
        B = mask.shape[0]
        cap = min(max_clusters, B)
        bufs = dict(mask=mask, pos=np.ascontiguousarray(pos, i32), order=np.ascontiguousarray(order, i32), counts=Out(i32, B),
                    U=Out(u32, words32(B)), cluster_of=Out(i32, B), center=Out(i32, cap), size=Out(i32, cap), mlist=Out(i32, B), state=Out(i32, 3))
        r = self.run("size_full", bufs, B=B, max_clusters=max_clusters)
        return {k: r[k] for k in STEP_KEYS}

    def contact_bits(self, rec, lig, cutoff):
        """rec [R, 9], lig [n, L, 9] -> bits [n, W, R] uint64."""
        rec, lig = np.ascontiguousarray(rec, f32).reshape(-1, 9), np.ascontiguousarray(lig, f32)
        n, L, R = lig.shape[0], lig.shape[1], rec.shape[0]
        r = self.run("contact_bits", dict(rec=rec, lig=lig, bits=Out(u64, n * words64(L) * R)), n=n, R=R, L=L, cutoff=f32(cutoff))
        return r["bits"].reshape(n, words64(L), R)

    def contact_count(self, bits, member, L, count, rec_count, lig_count):
        n, _, R = bits.shape
        r = self.run("contact_count", dict(bits=np.ascontiguousarray(bits, u64), member=np.ascontiguousarray(member, np.uint8),
                                           count=Out(i32, init=count), rec_count=Out(i32, init=rec_count), lig_count=Out(i32, init=lig_count)),
                     n=n, R=R, L=L)
        return dict(count=r["count"].reshape(R, L), rec_count=r["rec_count"], lig_count=r["lig_count"])

    def contact_score(self, bits, count, L):
        n, _, R = bits.shape
        r = self.run("contact_score", dict(bits=np.ascontiguousarray(bits, u64), count=np.ascontiguousarray(count, i32),
                                           n_contacts=Out(i32, n), score_sum=Out(np.int64, n)), n=n, R=R, L=L)
        return dict(n_contacts=r["n_contacts"], score_sum=r["score_sum"])

    def consensus_full(self, rec, lig, member, cutoff):
        rec, lig = np.ascontiguousarray(rec, f32).reshape(-1, 9), np.ascontiguousarray(lig, f32)
        n, L, R = lig.shape[0], lig.shape[1], rec.shape[0]
        r = self.run("consensus_full", dict(rec=rec, lig=lig, member=np.ascontiguousarray(member, np.uint8), bits=Out(u64, n * words64(L) * R),
                                            count=Out(i32, init=np.zeros(R * L)), rec_count=Out(i32, init=np.zeros(R)),
                                            lig_count=Out(i32, init=np.zeros(L)), n_contacts=Out(i32, n), score_sum=Out(np.int64, n)),
                     n=n, R=R, L=L, cutoff=f32(cutoff))
        return dict(bits=r["bits"].reshape(n, words64(L), R), count=r["count"].reshape(R, L), rec_count=r["rec_count"],
                    lig_count=r["lig_count"], n_contacts=r["n_contacts"], score_sum=r["score_sum"])


def words32(B):
    return (B + 31) // 32


def words64(L):
    return (L + 63) // 64


def pack32(bits):
    """bool [B, n] -> uint32 [B, ceil(n / 32)], bit j % 32 of word j / 32."""
    bits = np.asarray(bits, bool)
    B, n = bits.shape
    W = words32(n)
    pad = np.zeros((B, W * 32), np.uint8)
    pad[:, :n] = bits
    return np.ascontiguousarray(np.packbits(pad.reshape(B, W, 4, 8), axis=-1, bitorder="little").reshape(B, W, 4)).view("<u4").reshape(B, W).astype(u32)


def unpack32(words, n=None):
    """uint32 [B, W] -> bool [B, W * 32] (or its first n columns)."""
    w = np.ascontiguousarray(np.asarray(words, u32).astype("<u4"))
    flat = np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=-1, bitorder="little").astype(bool)
    return flat if n is None else flat[:, :n]


# ======================================================================================================================================
# k_pose_dist
# ======================================================================================================================================
def fma32(d, acc):
    """fl32(d * d + acc) of float32 arrays, one rounding.  d * d is exact in float64 (48 bits).  s = fl64(acc + d*d) with its TwoSum
    error: where s is exact, or is not exactly half way between two float32, fl32(s) is the correctly rounded result (rounding is
    monotone and the half-way points are float64 numbers); where s is inexact AND sits on such a point, the element is resolved exactly
    with fractions."""
    with np.errstate(invalid="ignore", over="ignore"):
        a, p = acc.astype(np.float64), d.astype(np.float64) * d.astype(np.float64)
        s = a + p
        bb = s - a
        err = (a - (s - bb)) + (p - bb)
        out = s.astype(f32)
    half = (np.ascontiguousarray(s).view(np.uint64) & np.uint64(0x1fffffff)) == np.uint64(0x10000000)
    tie = half & (err != 0) & np.isfinite(s)
    for idx in zip(*np.nonzero(tie)):
        out[idx] = round32(fractions.Fraction(float(a[idx])) + fractions.Fraction(float(p[idx])))
    return out


def round32(q):
    """A non-negative Fraction rounded to the nearest float32, ties to even (normal range)."""
    if q == 0:
        return f32(0)
    e = 0
    while q >= 2 ** (e + 24):
        e += 1
    while q < 2 ** (e + 23):
        e -= 1
    scaled = q / fractions.Fraction(2) ** e
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > fractions.Fraction(1, 2) or (rem == fractions.Fraction(1, 2) and n % 2):
        n += 1
    return f32(float(n) * 2.0 ** e)


def subset_coords(x, res):
    """x [B, L, 9] -> [B, D] the compared coordinates in the kernel's order."""
    x = np.asarray(x, f32)
    return (x if res is None else x[:, np.asarray(res)]).reshape(x.shape[0], -1)


def restate_pose(x, res, radius, mutant=None):
    """The chain of k_pose_dist: (rmsd [B, B] float32, mask words [B, W] uint32).  Mutants: see POSE_MUTANTS."""
    x = np.asarray(x, f32)
    B, L = x.shape[0], x.shape[1]
    n_res = L if res is None else len(res)
    c = subset_coords(x, None if mutant == "subset_ignored" else res)[:, :9 * n_res]
    D = c.shape[1]
    if mutant == "last_chunk_dropped" and D % KC:
        c = c[:, :D - D % KC]
    nt = (B + PT - 1) // PT
    cp = np.zeros((nt * PT, c.shape[1]), f32)      # the zero-filled padding lanes of a partial tile
    cp[:B] = c
    with np.errstate(invalid="ignore", over="ignore"):
        if mutant == "gram":
            sq = np.zeros(len(cp), f32)
            for k in range(cp.shape[1]):
                sq = sq + cp[:, k] * cp[:, k]
            dot = np.zeros((len(cp), len(cp)), f32)
            for k in range(cp.shape[1]):
                dot = dot + cp[:, None, k] * cp[None, :, k]
            acc = np.maximum(sq[:, None] + sq[None, :] - f32(2) * dot, f32(0))
        else:
            acc = np.zeros((len(cp), len(cp)), f32)
            for k in range(cp.shape[1]):
                acc = fma32(cp[:, None, k] - cp[None, :, k], acc)
        inv = f32(1) / f32(n_res if mutant == "mean_over_residues" else n_res * 3)
        r = np.sqrt(acc * inv)
        nb = r < f32(radius) if mutant == "lt_radius" else r <= f32(radius)
    rm = r[:B, :B].copy()
    W = words32(B)
    if mutant != "padding_not_skipped":
        nb[B:] = False
        nb[:, B:] = False
    words = pack32(nb[:B])[:, :W]
    if mutant == "transpose_not_written":      # rows of tile tj, columns of tile ti < tj: never written
        for a in range(B):
            lo = (a // PT) * PT
            rm[a, :lo] = np.frombuffer(b"\xff" * 4, f32)[0]
            words[a, :lo // 32] = SENT32
    return rm, words


POSE_MUTANTS = ("gram", "last_chunk_dropped", "subset_ignored", "lt_radius", "mean_over_residues", "transpose_not_written", "padding_not_skipped")


def gate_rel(D):
    return (D / 2 + 4) * U32


def rmsd64(x, res):
    from dfmdock_amd.cluster import pose_rmsd
    x = np.asarray(x, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        return pose_rmsd(x, None if res is None else np.asarray(res))


def check_rmsd(got, case, restatement=True):
    """The [B, B] matrix against float64 (gate_rel) and the restatement (bit for bit): the largest error / gate over finite pairs."""
    B, D = case.B, case.D
    assert got.shape == (B, B) and got.dtype == f32
    fin = case.finite
    ok = np.outer(fin, fin)
    assert not np.isfinite(got[~ok]).any(), "a pair with a non-finite pose is not finite"
    gt = np.ascontiguousarray(got.T)
    assert ((got.view(u32) == gt.view(u32)) | (np.isnan(got) & np.isnan(gt))).all(), "bitwise symmetric (NaN with NaN)"
    assert (np.diag(got)[fin] == 0).all(), "the diagonal is exactly 0"
    ref = case.r64
    with np.errstate(invalid="ignore"):
        err, gate = np.abs(got.astype(np.float64) - ref)[ok], gate_rel(D) * ref[ok]
    assert (err <= gate).all(), float((err / np.maximum(gate, 1e-300)).max())
    assert not is_sentinel(got).any(), "an entry is left at the 0xff fill"
    if restatement:
        want, _ = case.restated
        same = (got.view(u32) == want.view(u32)) | (np.isnan(got) & np.isnan(want))      # (the sign and payload of a NaN are not compared)
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))[~same]
        assert same.all(), f"{int((~same).sum())} entries differ from the restatement, by at most {int(ulps.max())} ulp"
    off = gate > 0
    return float((err[off] / gate[off]).max()) if off.any() else 0.0


def border_pairs(case):
    """(pairs a < b of finite poses, those within the border around the radius)."""
    iu = np.triu_indices(case.B, 1)
    ok = np.outer(case.finite, case.finite)[iu]
    r = case.r64[iu][ok]
    return int(ok.sum()), int((np.abs(r - case.radius) <= gate_rel(case.D) * case.radius).sum())


def check_mask(words, case, restatement=True):
    """The [B, W] bitmask: structure, the restatement bit for bit, float64 outside the border.  Returns (pairs, border pairs)."""
    B, W = case.B, words32(case.B)
    assert words.shape == (B, W) and words.dtype == u32
    bits = unpack32(words)
    assert not bits[:, B:].any(), "a bit at or beyond B is set"
    nb = bits[:, :B]
    assert (nb == nb.T).all(), "bit (a, b) equals bit (b, a)"
    fin = case.finite
    assert np.diag(nb)[fin].all() and not nb[~fin].any() and not nb[:, ~fin].any()
    _, want = case.restated if restatement else (None, words)
    # (also: no word is left at the 0xff fill - 32 neighbours in a row give the same word, so the restatement decides)
    assert np.array_equal(words, want), f"{int((unpack32(words) != unpack32(want)).sum())} bits differ from the restatement"
    inside = np.abs(case.r64 - case.radius) <= gate_rel(case.D) * case.radius
    sure = np.outer(fin, fin) & ~inside
    with np.errstate(invalid="ignore"):
        assert (nb[sure] == (case.r64 <= case.radius)[sure]).all(), "a pair outside the border differs from float64"
    return border_pairs(case)


# ---- pose cases ------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def backbone(n, rng, start=(0.0, 0.0, 0.0)):
    """[n, 3, 3] float64 (N, CA, C): CA a random walk of 3.8 A steps, N and C 1.46 / 1.52 A off their CA."""
    steps, dn, dc = (rng.standard_normal((n, 3)) for _ in range(3))
    ca = np.asarray(start) + np.cumsum(3.8 * _unit(steps), 0)
    return np.stack([ca + 1.46 * _unit(dn), ca, ca + 1.52 * _unit(dc)], 1)


def rotation(rng, angle):
    k = _unit(rng.standard_normal(3))
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


class PoseCase:
    """B poses x [B, L, 9] float32, the compared residues res (None: all), a radius; kind: the generator ('lattice': exact sums)."""

    def __init__(self, name, x, res, radius, kind):
        self.name, self.kind = name, kind
        self.x = np.ascontiguousarray(x, f32).reshape(len(x), -1, 9)
        self.res = None if res is None else np.asarray(res, i32)
        self.radius = float(f32(radius))
        self.B, self.L = self.x.shape[0], self.x.shape[1]
        self.n_res = self.L if res is None else len(self.res)
        self.D = 9 * self.n_res

    @functools.cached_property
    def finite(self):
        return np.isfinite(subset_coords(self.x, self.res)).all(1)

    @functools.cached_property
    def r64(self):
        return rmsd64(self.x, self.res)

    @functools.cached_property
    def restated(self):
        return restate_pose(self.x, self.res, self.radius)

    def __repr__(self):
        return self.name


def _subset(kind, L, n_res, rng):
    if kind == "none":
        return None
    if kind == "perm":
        return rng.permutation(L)
    r = rng.choice(L, size=n_res, replace=False)
    if kind == "sorted":
        return np.sort(r)
    while n_res > 1 and (np.diff(r) > 0).all():
        r = rng.permutation(r)
    return r


def _poses(kind, B, L, rng):
    """B poses of an L-residue ligand, float64 [B, L, 3, 3]."""
    base = backbone(L, rng)
    c = base[:, 1].mean(0)
    if kind in ("rigid", "far"):      # rigid moves about the CA centroid; 'far': 9000 A from the origin
        off = np.array([9000.0, -9000.0, 9000.0]) if kind == "far" else 0.0
        return np.stack([(base - c) @ rotation(rng, rng.uniform(0, 0.4)).T + c + 2.0 * rng.standard_normal(3) + off for _ in range(B)])
    if kind == "noise":               # non-rigid
        return base[None] + rng.normal(0, 1.5, (B, L, 3, 3))
    if kind == "origin":              # every coordinate within the radius of the origin: the zero padding lanes would be neighbours
        return rng.uniform(-1.0, 1.0, (B, L, 3, 3))
    raise ValueError(kind)


def _median_radius(x, res):
    r = rmsd64(np.asarray(x, f32).reshape(len(x), -1, 9), res)
    off = r[np.triu_indices(len(r), 1)]
    return float(np.median(off)) if off.size else 3.0


# (B, n_res, L, subset, generator): every B and n_res of the issue, every subset kind, every generator
POSE_SHAPES = ((1, 1, 1, "none", "rigid"), (31, 3, 5, "sorted", "noise"), (32, 4, 9, "unsorted", "rigid"), (33, 7, 7, "perm", "origin"),
               (63, 8, 8, "none", "far"), (64, 32, 40, "sorted", "rigid"), (65, 3, 6, "unsorted", "origin"), (96, 4, 4, "none", "lattice"),
               (97, 7, 11, "unsorted", "lattice"), (129, 8, 8, "perm", "far"), (200, 32, 32, "none", "noise"), (65, 1, 1, "none", "lattice"),
               (200, 3, 4, "sorted", "origin"), (33, 4, 6, "unsorted", "planted"))


@functools.lru_cache(None)
def pose_cases():
    out = []
    for i, (B, n_res, L, sub, kind) in enumerate(POSE_SHAPES):
        rng = np.random.default_rng(100 + i)
        res = _subset(sub, L, n_res, rng)
        name = f"B{B} n_res{n_res} L{L} {sub} {kind}"
        if kind in ("lattice", "planted"):
            # multiples of 0.25 A; two poses differ by at most 4 A per coordinate, so every partial sum is a multiple of 1/16 below
            # 2^24 / 16: exact in fp32.  The radius lies between two attainable sums S0 and S0 + 1/16.
            base = np.round(backbone(L, rng) * 4) / 4
            x = base[None] + rng.integers(-8, 9, (B, L, 3, 3)) * 0.25
            xs = subset_coords(x.reshape(B, L, 9).astype(f32), res).astype(np.float64)
            S = ((xs[:, None] - xs[None]) ** 2).sum(-1)[np.triu_indices(B, 1)]
            S0 = np.sort(S)[len(S) // 3]
            radius = np.sqrt((S0 + 1.0 / 32) / (3 * n_res))
            if kind == "planted":      # the radius IS the restated value of pair (0, B - 1): a neighbour under <=
                rm, _ = restate_pose(x.reshape(B, L, 9), res, 1.0)
                radius = rm[0, B - 1]
        else:
            x = _poses(kind, B, L, rng)
            radius = 0.9 * np.sqrt(3.0) if kind == "origin" else _median_radius(x.reshape(B, L, 9), res)
        out.append(PoseCase(name, x.reshape(B, L, 9), res, radius, kind))
    return tuple(out)


def poisoned(case, how, compared):
    """case with a NaN ('nan') at pose B // 2 and +inf ('inf') at pose B - 1, in a compared residue or (compared = False) in one outside the
    subset; how: 'nan', 'inf' or 'both'.  Returns None when the case has no such residue or pose."""
    all_res = np.arange(case.L) if case.res is None else case.res
    outside = np.setdiff1d(np.arange(case.L), all_res)
    pick = all_res if compared else outside
    if pick.size == 0 or case.B < 3:
        return None
    x = case.x.copy()
    r = int(pick[len(pick) // 2])
    if how in ("nan", "both"):
        x[case.B // 2, r, 4] = np.nan
    if how in ("inf", "both"):
        x[case.B - 1, r, 7] = np.inf
    return PoseCase(f"{case.name} {how} {'in' if compared else 'outside'}", x, case.res, case.radius, case.kind)


# ======================================================================================================================================
# clustering on crafted masks
# ======================================================================================================================================
class GraphCase:
    """A symmetric neighbour matrix adj [B, B] bool (diagonal True but for the 'non-finite' poses, whose row and column are clear),
    a key [B] or None."""

    def __init__(self, name, adj, key):
        from dfmdock_amd.cluster import rank_order
        self.name, self.adj, self.key = name, np.asarray(adj, bool), key
        self.B = self.adj.shape[0]
        assert (self.adj == self.adj.T).all()
        self.order = rank_order(key, self.B).astype(i32)
        self.pos = np.empty(self.B, i32)
        self.pos[self.order] = np.arange(self.B, dtype=i32)
        self.mask = pack32(self.adj)

    @functools.cached_property
    def natural(self):
        """clusters each rule forms without a limit"""
        from dfmdock_amd.cluster import cluster_adjacency
        return {r: cluster_adjacency(self.adj, self.key, r)["n_clusters"] for r in ("energy", "size")}

    def limits(self):
        """max_clusters: 1, a value below the natural count, B"""
        below = max(1, min(self.natural.values()) // 2)
        return sorted({1, below, self.B})

    def __repr__(self):
        return self.name


def _cliques(B, sizes, members):
    """disjoint cliques: members = pose indices, cut into consecutive groups of `sizes`"""
    adj = np.zeros((B, B), bool)
    at = 0
    for s in sizes:
        g = members[at:at + s]
        adj[np.ix_(g, g)] = True
        at += s
    return adj


def graph(kind, B, rng):
    eye = np.eye(B, dtype=bool)
    if kind == "empty":
        return eye
    if kind == "complete":
        return np.ones((B, B), bool)
    if kind == "cliques":
        sizes, left = [], B
        while left:
            s = min(left, int(rng.integers(1, max(2, B // 3 + 1))))
            sizes.append(s)
            left -= s
        return _cliques(B, sizes, rng.permutation(B))
    if kind == "path":
        adj = eye.copy()
        p = rng.permutation(B)
        adj[p[:-1], p[1:]] = adj[p[1:], p[:-1]] = True
        return adj
    if kind == "star":
        adj = eye.copy()
        hub = int(rng.integers(B))
        adj[hub, :] = adj[:, hub] = True
        return adj
    if kind == "gnp":      # expected degree 3: many equal counts
        up = np.triu(rng.random((B, B)) < min(1.0, 3.0 / max(B - 1, 1)), 1)
        return up | up.T | eye
    raise ValueError(kind)


def keys(kind, B, rng):
    if kind == "none":
        return None
    if kind == "distinct":
        return rng.permutation(B).astype(f32)
    k = rng.integers(0, max(2, B // 4), B).astype(f32)      # ties
    if kind == "nan":
        k[rng.random(B) < 0.2] = np.nan
    return k


GRAPH_KINDS = ("empty", "complete", "cliques", "path", "star", "gnp")
KEY_KINDS = ("none", "distinct", "ties", "nan")
GRAPH_B = (1, 31, 32, 33, 64, 65, 1023, 1024, 1025, 2500)


def planted_scan_case():
    """B = 2500: the 2100 best-keyed poses form one clique (the leader's scan then crosses two whole 1024-strides with nothing found),
    then cliques of 150 and 249, and the worst-keyed pose alone at rank B - 1."""
    B = 2500
    rng = np.random.default_rng(77)
    by_rank = rng.permutation(B)      # pose at each rank
    adj = _cliques(B, [2100, 150, 249, 1], by_rank)
    key = np.empty(B, f32)
    key[by_rank] = np.arange(B, dtype=f32)
    return GraphCase("B2500 planted scan", adj, key)


@functools.lru_cache(None)
def graph_cases():
    out, i = [], 0
    for bi, B in enumerate(GRAPH_B):
        kinds = GRAPH_KINDS if B <= 65 else (GRAPH_KINDS[(bi + j) % 6] for j in (0, 2, 3))      # every kind at the small sizes
        for kind in kinds:
            rng = np.random.default_rng(500 + i)
            adj = graph(kind, B, rng)
            kk = KEY_KINDS[i % 4]
            out.append(GraphCase(f"B{B} {kind} key {kk}", adj, keys(kk, B, rng)))
            if B >= 3 and (B <= 65 or i % 2 == 0):      # the same with a few non-finite poses: row, column and diagonal clear
                bad = rng.choice(B, size=min(3, B - 1), replace=False)
                a2 = adj.copy()
                a2[bad, :] = False
                a2[:, bad] = False
                kk2 = KEY_KINDS[(i + 1) % 4]
                out.append(GraphCase(f"B{B} {kind} key {kk2} nonfinite", a2, keys(kk2, B, rng)))
            i += 1
    out.append(planted_scan_case())
    return tuple(out)


def fresh_state(B, cap):
    """What k_cluster_count leaves plus sentinel-filled center / size / mlist, before the count itself."""
    return dict(counts=np.zeros(B, i32), U=np.zeros(words32(B), u32), cluster_of=np.full(B, -1, i32), center=np.full(cap, -1, i32),
                size=np.full(cap, -1, i32), mlist=np.full(B, -1, i32), state=np.zeros(3, i32))


CLUSTER_MUTANTS = ("tie_lower_index", "no_decrement", "decrement_assigned_too", "leader_one_stride", "max_clusters_off_by_one", "nonfinite_opens")


def restate_count(adj, mutant=None):
    B = adj.shape[0]
    free = np.ones(B, bool) if mutant == "nonfinite_opens" else adj.diagonal().copy()
    return dict(counts=adj.sum(1).astype(i32), U=pack32(free[None])[0], cluster_of=np.full(B, -1, i32), state=np.zeros(3, i32))


def restate_step(adj, pos, order, st, mutant=None):
    """One pick + decrement of the definition on the state st; returns the new state (st is not changed)."""
    st = {k: v.copy() for k, v in st.items()}
    B = adj.shape[0]
    if st["state"][1]:
        return st
    free = unpack32(st["U"][None], B)[0]
    cand = np.nonzero(free)[0]
    cnt = st["counts"].astype(np.int64)
    if cand.size == 0:      # no pose that is its own neighbour is left (k_cluster_pick: best == 0)
        st["state"][1] = 1
        return st
    tie = cand if mutant == "tie_lower_index" else pos[cand]
    best = cand[np.lexsort((tie, -cnt[cand]))[0]]
    m = adj[best] & free
    k = int(st["state"][0])
    st["cluster_of"][m] = k
    free = free & ~m
    st["U"] = pack32(free[None])[0]
    if mutant != "no_decrement":
        gone = ~free & adj.diagonal() if mutant == "decrement_assigned_too" else m
        st["counts"] = (cnt - adj[:, gone].sum(1)).astype(i32)
    st["center"][k], st["size"][k] = best, int(m.sum())
    members = np.nonzero(m)[0]
    st["mlist"][:members.size] = members
    st["state"][0], st["state"][2] = k + 1, members.size
    return st


def restate_size_full(adj, pos, order, max_clusters, mutant=None):
    B = adj.shape[0]
    cap = min(max_clusters, B)
    steps = cap + 1 if mutant == "max_clusters_off_by_one" else cap
    st = fresh_state(B, max(cap, steps))
    st.update(restate_count(adj, mutant))
    for _ in range(steps):
        st = restate_step(adj, pos, order, st, mutant)
    st["center"], st["size"] = st["center"][:cap], st["size"][:cap]
    return st


def restate_leader(adj, order, max_clusters, mutant=None):
    B = adj.shape[0]
    cap = min(max_clusters, B) + (1 if mutant == "max_clusters_off_by_one" else 0)
    free = np.ones(B, bool) if mutant == "nonfinite_opens" else adj.diagonal().copy()
    of, center, size = np.full(B, -1, i32), np.full(cap, -1, i32), np.full(cap, -1, i32)
    at = k = 0
    while k < cap and at < B:
        ranks = np.nonzero(free[order[at:]])[0]
        if ranks.size == 0 or (mutant == "leader_one_stride" and ranks[0] >= STRIDE):
            break
        at += int(ranks[0])
        p = order[at]
        at += 1
        m = adj[p] & free
        of[m] = k
        free &= ~m
        center[k], size[k] = p, int(m.sum())
        k += 1
    cap = min(max_clusters, B)
    return dict(n=k, center=center[:cap], size=size[:cap], cluster_of=of)


def check_against_definition(n, center, size, cluster_of, case, rule, max_clusters):
    """n, center, size and cluster_of equal cluster.cluster_adjacency exactly; entries beyond n still hold the sentinel."""
    from dfmdock_amd.cluster import cluster_adjacency
    want = cluster_adjacency(case.adj, case.key, rule, max_clusters)
    cap = min(max_clusters, case.B)
    assert n == want["n_clusters"], (n, want["n_clusters"])
    assert len(center) == cap and len(size) == cap
    assert np.array_equal(center[:n], want["center"]) and np.array_equal(size[:n], want["size"])
    assert (center[n:] == -1).all() and (size[n:] == -1).all(), "entries beyond n hold the sentinel"
    assert np.array_equal(cluster_of, want["cluster_of"])
    assert (np.asarray(size[:n]) >= 1).all() and (cluster_of[~case.adj.diagonal()] == -1).all()


def check_leader(got, case, max_clusters):
    check_against_definition(got["n"], got["center"], got["size"], got["cluster_of"], case, "energy", max_clusters)


def check_size_full(got, case, max_clusters):
    st = got["state"]
    check_against_definition(int(st[0]), got["center"], got["size"], got["cluster_of"], case, "size", max_clusters)
    assert int(st[1]) == (1 if min(max_clusters, case.B) > int(st[0]) else 0), "done exactly when a step found no pose left"
    free = unpack32(got["U"][None], case.B)[0]
    assert np.array_equal(free, (got["cluster_of"] == -1) & case.adj.diagonal()), "U = the poses still to be assigned"
    assert not unpack32(got["U"][None])[0][case.B:].any()
    assert np.array_equal(got["counts"][free], (case.adj[free][:, free]).sum(1)), "counts on U = unassigned neighbours"


def check_count(got, case):
    want = restate_count(case.adj)
    assert np.array_equal(got["counts"], case.adj.sum(1)), "counts = the row popcounts"
    assert np.array_equal(got["U"], want["U"]), "U = the valid bits AND each pose's own diagonal bit"
    assert (got["cluster_of"] == -1).all() and (got["state"] == 0).all()


def check_step(got, before, case, max_clusters):
    """One step against the step of the definition on the same state."""
    want = restate_step(case.adj, case.pos, case.order, before)
    if before["state"][1]:
        for k in STEP_KEYS:
            assert got[k].tobytes() == before[k].tobytes(), f"a step after the done flag changed {k}"
        return
    assert np.array_equal(got["state"], want["state"]), (got["state"], want["state"])
    assert np.array_equal(got["U"], want["U"]) and np.array_equal(got["cluster_of"], want["cluster_of"])
    if not want["state"][1]:
        k = int(before["state"][0])
        assert got["center"][k] == want["center"][k] and got["size"][k] == want["size"][k], (k, got["center"][k], want["center"][k])
        others = np.arange(len(got["center"])) != k
        assert np.array_equal(got["center"][others], before["center"][others]) and np.array_equal(got["size"][others], before["size"][others])
        nm = int(want["state"][2])
        assert set(got["mlist"][:nm].tolist()) == set(want["mlist"][:nm].tolist()) and len(set(got["mlist"][:nm].tolist())) == nm
    free = unpack32(want["U"][None], case.B)[0]
    assert np.array_equal(got["counts"][free], want["counts"][free]), "counts on the poses still in U"


# ======================================================================================================================================
# consensus
# ======================================================================================================================================
def device_bits(c):
    """bool [n, R, L] -> the device layout [n][W][R] uint64, W = ceil(L / 64): word (p, w, i) holds ligand residues 64 w .. 64 w + 63 of
    receptor residue i, bit j % 64 = contact (i, j), unused high bits 0."""
    c = np.asarray(c, bool)
    n, R, L = c.shape
    W = words64(L)
    out = np.zeros((n, W, R), u64)
    for j in range(L):
        out[:, j // 64, :] |= c[:, :, j].astype(u64) << u64(j % 64)
    return out


def host_bits(bits, L):
    """the device layout back to bool [n, R, L] and the number of set bits at or beyond L"""
    bits = np.asarray(bits, u64)
    n, W, R = bits.shape
    full = np.zeros((n, R, W * 64), bool)
    for j in range(W * 64):
        full[:, :, j] = ((bits[:, j // 64, :] >> u64(j % 64)) & u64(1)).astype(bool)
    return full[:, :, :L], int(full[:, :, L:].sum())


CONSENSUS_MUTANTS = ("le_at_cutoff", "reject_without_reach", "reach_from_n_only", "fp32_distance", "non_members_counted",
                     "score_over_members_only", "score_sum_32bit", "high_bits_leak", "row_tail_lost", "rec_count_counts_contacts")


def _reach32(x, mutant):
    """k_contact_bits' reach of residues x [n, 9] in fp32"""
    with np.errstate(invalid="ignore", over="ignore"):
        a = x[:, 0:3] - x[:, 3:6]
        c = x[:, 6:9] - x[:, 3:6]
        a2 = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
        c2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        if mutant == "reach_from_n_only":
            return np.sqrt(a2)
        return np.sqrt(np.where((a2 > c2) | np.isnan(a2), a2, c2))


def restate_contact_bits(rec, lig, cutoff, mutant=None):
    """k_contact_bits: the fp32 reject, then the fp64 distance, packed as the wave's ballot packs it."""
    from dfmdock_amd.consensus import min_dist
    rec, lig = np.asarray(rec, f32).reshape(-1, 9), np.asarray(lig, f32)
    n, L, R = lig.shape[0], lig.shape[1], rec.shape[0]
    W = words64(L)
    cf = f32(cutoff)
    ligp = np.zeros((n, W * 64, 9), f32)      # padding lanes hold zeros
    ligp[:, :L] = lig
    valid = np.arange(W * 64) < L
    c = np.zeros((n, R, W * 64), bool)
    rr = _reach32(rec, mutant)
    for p in range(n):
        with np.errstate(invalid="ignore", over="ignore"):
            far = cf + _reach32(ligp[p], mutant)
            d = rec[:, None, 3:6] - ligp[p][None, :, 3:6]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            thr = (far[None, :] + rr[:, None]) * f32(1.0001) + f32(1e-3)
            if mutant == "reject_without_reach":
                thr = np.broadcast_to(cf * f32(1.0001) + f32(1e-3), d2.shape)
            passed = ~(d2 > thr * thr)
            if mutant == "fp32_distance":
                a, b = rec.reshape(-1, 3, 3), ligp[p].reshape(-1, 3, 3)
                best = None
                for s in range(3):
                    for t in range(3):
                        e = a[:, None, s] - b[None, :, t]
                        dd = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
                        best = dd if best is None else np.minimum(best, dd)
                near = best < cf
            else:
                md = min_dist(rec, ligp[p])
                near = md <= float(cf) if mutant == "le_at_cutoff" else md < float(cf)
        c[p] = passed & near
        if mutant != "high_bits_leak":
            c[p][:, ~valid] = False
    bits = np.zeros((n, W, R), u64)
    for j in range(W * 64):
        bits[:, j // 64, :] |= c[:, :, j].astype(u64) << u64(j % 64)
    if mutant == "row_tail_lost" and R % 64:
        bits[:, :, R - R % 64:] = u64(0xffffffffffffffff)
    return bits


def restate_contact_count(bits, member, L, count, rec_count, lig_count, mutant=None):
    c, _ = host_bits(bits, L)
    m = np.asarray(member).astype(bool)
    if mutant == "non_members_counted":
        m = np.ones_like(m)
    cm = c[m]
    rc = cm.sum(2).sum(0) if mutant == "rec_count_counts_contacts" else cm.any(2).sum(0)
    return dict(count=(np.asarray(count, np.int64).reshape(c.shape[1], L) + cm.sum(0)).astype(i32),
                rec_count=(np.asarray(rec_count, np.int64) + rc).astype(i32), lig_count=(np.asarray(lig_count, np.int64) + cm.any(1).sum(0)).astype(i32))


def restate_contact_score(bits, count, L, member=None, mutant=None):
    c, _ = host_bits(bits, L)
    count = np.asarray(count, np.int64).reshape(c.shape[1], L)
    s = np.array([int(count[c[p]].sum()) for p in range(len(c))], np.int64)
    nc = c.reshape(len(c), -1).sum(1).astype(i32)
    if mutant == "score_over_members_only" and member is not None:
        s[~np.asarray(member).astype(bool)] = 0
    if mutant == "score_sum_32bit":
        s = s.astype(np.int32).astype(np.int64)
    return dict(n_contacts=nc, score_sum=s)


def check_contact_bits(bits, rec, lig, cutoff):
    """Every word equals the definition, no border; unused high bits 0; no word left at the sentinel."""
    from dfmdock_amd.consensus import contacts
    lig = np.asarray(lig, f32)
    n, L = lig.shape[0], lig.shape[1]
    R = np.asarray(rec).reshape(-1, 9).shape[0]
    assert bits.shape == (n, words64(L), R) and bits.dtype == u64
    want = device_bits(contacts(np.asarray(rec, f32).reshape(-1, 9), lig, cutoff))
    if L % 64:
        assert not (bits[:, -1, :] >> u64(L % 64)).any(), "unused high bits are 0"
    # (a word left at the 0xff fill differs from the definition, or - 64 contacts in a row, L % 64 == 0 - is what the kernel wrote)
    assert np.array_equal(bits, want), f"{int((host_bits(bits, L)[0] != host_bits(want, L)[0]).sum())} contacts differ from the definition"


def check_contact_count(got, bits, member, L, prefill):
    """count, rec_count, lig_count = the prefill plus consensus.from_contacts on the member poses (none: the prefill)."""
    from dfmdock_amd.consensus import from_contacts
    c, high = host_bits(bits, L)
    assert high == 0
    m = np.asarray(member).astype(bool)
    if m.any():
        ref = from_contacts(c, m)
        add = {k: ref[k].astype(np.int64) for k in ("count", "rec_count", "lig_count")}
    else:
        add = dict(count=0, rec_count=0, lig_count=0)
    for k in ("count", "rec_count", "lig_count"):
        want = (np.asarray(prefill[k], np.int64).reshape(got[k].shape) + add[k]).astype(i32)
        assert got[k].dtype == i32 and np.array_equal(got[k], want), k


def check_contact_score(got, bits, count, L):
    """n_contacts and score_sum of every pose on the given count: the formulas of consensus.from_contacts."""
    c, high = host_bits(bits, L)
    assert high == 0
    count = np.asarray(count, np.int64).reshape(c.shape[1], L)
    want_n = c.reshape(len(c), -1).sum(1, dtype=np.int64).astype(i32)
    want_s = np.array([int(count[c[p]].sum(dtype=np.int64)) for p in range(len(c))], np.int64)
    assert got["n_contacts"].dtype == i32 and np.array_equal(got["n_contacts"], want_n)
    assert got["score_sum"].dtype == np.int64 and np.array_equal(got["score_sum"], want_s)


def check_consensus_full(got, rec, lig, member, cutoff):
    from dfmdock_amd.consensus import consensus
    ref = consensus(np.asarray(rec, f32).reshape(-1, 9), lig, cutoff, member)
    check_contact_bits(got["bits"], rec, lig, cutoff)
    for k in ("count", "rec_count", "lig_count", "n_contacts", "score_sum"):
        assert np.array_equal(got[k], ref[k]) and got[k].dtype == ref[k].dtype, k


# ---- consensus cases ------------------------------------------------------------------------------------------------------------------
class ContactCase:
    def __init__(self, name, rec, lig, cutoff, kind, planted=()):
        self.name, self.kind, self.cutoff, self.planted = name, kind, float(f32(cutoff)), tuple(planted)
        self.rec = np.ascontiguousarray(rec, f32).reshape(-1, 9)
        self.lig = np.ascontiguousarray(lig, f32).reshape(len(lig), -1, 9)
        self.n, self.L, self.R = self.lig.shape[0], self.lig.shape[1], self.rec.shape[0]

    def __repr__(self):
        return self.name


CONTACT_SHAPES = ((1, 1, 1), (63, 65, 3), (64, 64, 1), (65, 63, 3), (130, 129, 3), (1, 129, 1), (130, 1, 3))      # (R, L, n)


def _generic_contact(R, L, n, rng):
    rec = backbone(R, rng)
    ligs = []
    for _ in range(n):      # each pose starts next to a receptor residue
        at = rec[int(rng.integers(R)), 1] + 5.0 * _unit(rng.standard_normal(3))
        ligs.append(backbone(L, rng, at))
    return rec, np.stack(ligs)


def _lattice_contact(R, L, n, rng):
    """Residues on a coarse lattice, compact (N, CA, C 1 A apart along z).  Planted: receptor residue R - 1 with its C at the origin side
    of a 3-4-5 triangle to the N of ligand residue L - 1 of pose 0 (exactly 5.0: no contact under cutoff 5.0) and, one fp32 ulp inside,
    to ligand residue 0 of pose n - 1 when that is another pair."""
    def res_at(p):
        p = np.asarray(p, np.float64)
        return np.stack([p + [0, 0, -1.0], p, p + [0, 0, 1.0]])
    rec = np.stack([res_at([20.0 * i, 100.0, 0.0]) for i in range(R)])      # far from everything planted
    lig = np.stack([[res_at([20.0 * j, -100.0 - 50.0 * p, 0.0]) for j in range(L)] for p in range(n)])
    rec[R - 1] = res_at([0.0, 0.0, -1.0])            # its C at (0, 0, 0)
    planted = []
    lig[0, L - 1] = res_at([3.0, 4.0, 1.0])          # its N at (3, 4, 0): exactly 5.0 from that C
    planted.append((0, R - 1, L - 1, False))
    if (n - 1, 0) != (0, L - 1):
        inside = res_at([3.0, -4.0, 1.0])
        inside[0, 0] = np.nextafter(f32(3.0), f32(0.0))      # one fp32 ulp inside: 9 - 2^-20 + 16 rounds to 25 in fp32
        lig[n - 1, 0] = inside
        planted.append((n - 1, R - 1, 0, True))
    return rec, lig, planted


def _stretched_contact(R, L, n, rng):
    """N or C up to 40 A from their CA: contacts between residues whose CAs are 60 A and more apart."""
    rec, lig = _generic_contact(R, L, n, rng)
    rec = rec + np.array([0.0, 0.0, 0.0])
    lig = lig + np.array([70.0, 0.0, 0.0])      # CAs far apart
    for i in range(0, R, 2):      # the C of every other receptor residue reaches towards the ligand
        rec[i, 2] = rec[i, 1] + np.array([rng.uniform(30, 40), 0.0, 0.0])
    for p in range(n):
        for j in range(0, L, 2):      # the N (even poses) or the C (odd poses) of every other ligand residue reaches back
            lig[p, j, 0 if p % 2 == 0 else 2] = lig[p, j, 1] - np.array([rng.uniform(30, 40), 0.0, 0.0])
    return rec, lig


def _origin_contact(R, L, n, rng):
    """Receptor residues at the origin: the zero-filled padding lanes of the last ligand word would be in contact."""
    rec, lig = _generic_contact(R, L, n, rng)
    rec[:: 2] = rng.uniform(-1.0, 1.0, rec[:: 2].shape)
    return rec, lig


@functools.lru_cache(None)
def contact_cases():
    out = []
    for i, (R, L, n) in enumerate(CONTACT_SHAPES):
        for kind in ("generic", "lattice", "stretched", "origin"):
            rng = np.random.default_rng(900 + 10 * i + len(kind))
            planted = ()
            if kind == "generic":
                rec, lig = _generic_contact(R, L, n, rng)
            elif kind == "lattice":
                rec, lig, planted = _lattice_contact(R, L, n, rng)
            elif kind == "stretched":
                rec, lig = _stretched_contact(R, L, n, rng)
            else:
                rec, lig = _origin_contact(R, L, n, rng)
            out.append(ContactCase(f"R{R} L{L} n{n} {kind}", rec, lig, 5.0 if kind == "lattice" else 5.5, kind, planted))
    return tuple(out)


def contact_poisoned(case, how, where):
    """A NaN coordinate, or +inf in every atom, in ligand residue L // 2 of pose n - 1 (where = 'lig') or in receptor residue R // 2
    (where = 'rec')."""
    rec, lig = case.rec.copy(), case.lig.copy()
    at = [4] if how == "nan" else [0, 3, 6]      # one NaN coordinate; +inf in the x of every atom (one infinite atom leaves the others' contacts)
    v = np.nan if how == "nan" else np.inf
    if where == "lig":
        lig[case.n - 1, case.L // 2, at] = v
    else:
        rec[case.R // 2, at] = v
    return ContactCase(f"{case.name} {how} {where}", rec, lig, case.cutoff, case.kind)


def crafted_bits(n, R, L, rng):
    """bool [n, R, L]: random contacts, with rows that are all ones, all zero and single-bit."""
    c = rng.random((n, R, L)) < 0.3
    for p in range(n):
        c[p, (3 * p) % R] = True
        c[p, (3 * p + 1) % R] = False
        if R > 2:
            c[p, (3 * p + 2) % R] = False
            c[p, (3 * p + 2) % R, (7 * p) % L] = True
    return c


COUNT_N = (1, 7, 8, 9, 67)
MEMBER_KINDS = ("all", "one", "alternating", "none")


def members(kind, n):
    m = np.zeros(n, np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "one":
        m[n // 2] = 1
    elif kind == "alternating":
        m[::2] = 1
    return m


@functools.lru_cache(None)
def count_cases():
    """(name, contacts bool [n, R, L], member, prefill dict) over every n and member kind; R, L cycle through the word edges."""
    shapes = ((65, 63), (64, 130), (130, 64), (1, 65), (63, 1))
    out = []
    for a, n in enumerate(COUNT_N):
        for b, mk in enumerate(MEMBER_KINDS):
            R, L = shapes[(a + b) % len(shapes)]
            rng = np.random.default_rng(1300 + 10 * a + b)
            pre = dict(count=rng.integers(1, 1000, (R, L)).astype(i32), rec_count=rng.integers(1, 1000, R).astype(i32),
                       lig_count=rng.integers(1, 1000, L).astype(i32))
            out.append((f"n{n} R{R} L{L} members {mk}", crafted_bits(n, R, L, rng), members(mk, n), pre))
    return tuple(out)


def big_score_case():
    """R = L = 192, every bit set, count = 65536 everywhere: score_sum = 36864 * 65536 = 2 415 919 104 > 2^31."""
    return np.ones((2, 192, 192), bool), np.full((192, 192), 65536, i32)
