"""Cryo-EM density fit of an ensemble of rigid ligand poses - which of these thousand models does the map support? - as HADDOCK-EM,
PowerFit, Situs or ChimeraX's "fit in map" ask it: the float64 numpy definition of dfm_pose_density (include/dfmdock_amd.h,
kernels_density.hip) and its host finishes.  No reference counterpart: the reference reads no map.

  frame                  the receptor's coordinates are taken to be in the map's frame (fitting the receptor into the map is not done
                         here); pose p of the ligand is sterics.pose_atoms
  grid                   C channels (1 to 4) of float32 on ONE orthogonal grid [nz, ny, nx]; origin [3] and voxel [3] float32 in A, (x, y,
                         z), the voxel may be anisotropic; node (iz, iy, ix) sits at origin + (ix, iy, iz) * voxel
  one atom, one channel  everything widened to float64, in this order, nothing contracted:
                           ux = (x - ox) / vx ; ix = floor(ux) ; fx = ux - ix        (same for y, z)
                           inside  iff 0 <= ux < nx-1 and 0 <= uy < ny-1 and 0 <= uz < nz-1      (a NaN is outside)
                           c00 = c000 + fx*(c100 - c000) ; c10 = c010 + fx*(c110 - c010)         (cXYZ: the node at ix+X, iy+Y, iz+Z)
                           c01 = c001 + fx*(c101 - c001) ; c11 = c011 + fx*(c111 - c011)
                           c0  = c00  + fy*(c10 - c00)   ; c1  = c01  + fy*(c11 - c01)
                           val = c0   + fz*(c1 - c0)
                           term_q = int64(rint((w_a * val) * 2^20)), ties to even; 0 for an outside atom
                         no square root and no transcendental anywhere
  sum_q [P,C] int64      the sum of term_q over the ligand's atoms, per channel
  n_inside [P] int32     the atoms inside the grid
  n_above [P] int32      the inside atoms whose channel-0 val >= threshold (a float32, widened)
  atom_q [P,Al] int64    term_q of channel 0 per atom, in the caller's atom order (optional)

Integer sums do not depend on their order, so the device's results equal these integer for integer, whatever the blocks and chunks.  A
pose with a non-finite transform gets zeros.  The limits (dfm_poseprep.h: check_density_grid, check_density_atoms, density_sum_bound):
every grid value finite and |value| <= 2^10, |w| <= 2^7, 2 <= n <= 1024 per axis, voxel finite and in (0, 16]; |term_q| <= 2^37, and a
ligand of Al atoms is refused if Al * 2^37 could reach 2^62.

The host finishes: read_mrc / write_mrc (MRC2014, numpy only), simulate_map (a sum of Gaussians; sigma = resolution * SIGMA_FACTOR is a
named convention, and no agreement with any other program's map simulator is claimed or tested), channels (the three grids the drivers
gather from and the pose-independent scalars) and correlation, the overlap correlation of the simulated complex with the map in closed
form: every pose-dependent term of it is a gather.  Nothing is claimed about the ranking quality on real maps; there is no local
resolution, no mask, no FSC, the ligand is rigid and no density guides the sampler.
"""
from __future__ import annotations

import numpy as np

from . import sterics as ST

QUANTA = 1048576.0            # 2^20 per unit of w * val
MAX_CHANNELS = 4
MAX_VALUE = 1024.0            # |grid value|
MAX_WEIGHT = 128.0            # |w|
MIN_AXIS, MAX_AXIS = 2, 1024  # nodes per axis
MAX_VOXEL = 16.0              # A
SIGMA_FACTOR = 1.0 / (np.pi * np.sqrt(2.0))      # sigma = resolution * SIGMA_FACTOR: the Gaussian whose Fourier transform falls to 1/e at 1 / resolution

_MRC_MODES = {0: "i1", 1: "i2", 2: "f4", 6: "u2", 12: "f2"}


def check_grid(grids, origin, voxel):
    """(grids [C,nz,ny,nx] float32, origin [3] float32, voxel [3] float32) as the device takes them.  ValueError outside the limits of
    dfm_density_create; a single [nz,ny,nx] grid is one channel."""
    g = np.asarray(grids, np.float32)
    if g.ndim == 3:
        g = g[None]
    if g.ndim != 4 or not 1 <= g.shape[0] <= MAX_CHANNELS:
        raise ValueError(f"grids must be [C,nz,ny,nx] with 1 <= C <= {MAX_CHANNELS}, got shape {g.shape}")
    if not all(MIN_AXIS <= n <= MAX_AXIS for n in g.shape[1:]):
        raise ValueError(f"need {MIN_AXIS} <= n <= {MAX_AXIS} nodes per axis, got {g.shape[1:]}")
    if not np.isfinite(g).all() or not (np.abs(g) <= MAX_VALUE).all():
        raise ValueError(f"grid values must be finite and at most {MAX_VALUE:g} in magnitude")
    o, v = np.asarray(origin, np.float32).reshape(-1), np.asarray(voxel, np.float32).reshape(-1)
    if o.size != 3 or v.size != 3:
        raise ValueError("origin and voxel must have 3 entries (x, y, z)")
    if not np.isfinite(o).all():
        raise ValueError("origin must be finite")
    if not (np.isfinite(v).all() and (v > 0).all() and (v <= MAX_VOXEL).all()):
        raise ValueError(f"voxel must be finite and in (0, {MAX_VOXEL:g}], got {v.tolist()}")
    return np.ascontiguousarray(g), o, v


def check_weights(w, n):
    """Atom weights [n] as the device takes them: float32, finite, |w| <= 128."""
    w = np.asarray(w, np.float32).reshape(-1)
    if w.shape != (n,):
        raise ValueError(f"weights must be [{n}], got {w.shape}")
    if not np.isfinite(w).all() or not (np.abs(w) <= MAX_WEIGHT).all():
        raise ValueError(f"weights must be finite and at most {MAX_WEIGHT:g} in magnitude")
    return w


def interpolate(grids, origin, voxel, X):
    """(val [C,n] float64, inside [n] bool) of the points X [n,3] float64: the trilinear value of every channel in the module docstring's
    operation order; val of an outside point is 0."""
    return _interpolate(*check_grid(grids, origin, voxel), X)


def _interpolate(g, o, v, X):
    """interpolate on a grid that check_grid has returned."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    C, nz, ny, nx = g.shape
    o, v = o.astype(np.float64), v.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (X - o) / v
        inside = (u[:, 0] >= 0) & (u[:, 0] < nx - 1) & (u[:, 1] >= 0) & (u[:, 1] < ny - 1) & (u[:, 2] >= 0) & (u[:, 2] < nz - 1)
    u = np.where(inside[:, None], u, 0.0)
    fl = np.floor(u)
    f = u - fl
    ix, iy, iz = (fl[:, k].astype(np.int64) for k in range(3))
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    c = lambda dz, dy, dx: g[:, iz + dz, iy + dy, ix + dx].astype(np.float64)
    c000, c100, c010, c110 = c(0, 0, 0), c(0, 0, 1), c(0, 1, 0), c(0, 1, 1)
    c001, c101, c011, c111 = c(1, 0, 0), c(1, 0, 1), c(1, 1, 0), c(1, 1, 1)
    c00, c10 = c000 + fx * (c100 - c000), c010 + fx * (c110 - c010)
    c01, c11 = c001 + fx * (c101 - c001), c011 + fx * (c111 - c011)
    c0, c1 = c00 + fy * (c10 - c00), c01 + fy * (c11 - c01)
    val = c0 + fz * (c1 - c0)
    return np.where(inside[None], val, 0.0), inside


def density(grids, origin, voxel, lig_atoms, lig_w, center, rot, tr, threshold=1.0, per_atom=False):
    """The definition.  grids [C,nz,ny,nx], origin / voxel [3], lig_atoms [Al,3], lig_w [Al], center [3], rot [P,3] axis-angle, tr [P,3],
    threshold: of channel 0.  Returns {sum_q [P,C] int64, n_inside, n_above [P] int32} and, with `per_atom`, atom_q [P,Al] int64."""
    g, o, v = check_grid(grids, origin, voxel)
    lig = np.asarray(lig_atoms, np.float32).reshape(-1, 3)
    w = check_weights(lig_w, lig.shape[0]).astype(np.float64)
    thr = float(np.float32(threshold))
    if not np.isfinite(thr):
        raise ValueError("threshold must be finite")
    rot, tr = np.asarray(rot, np.float32).reshape(-1, 3), np.asarray(tr, np.float32).reshape(-1, 3)
    if rot.shape != tr.shape:
        raise ValueError(f"rot and tr must both be [P,3], got {rot.shape} and {tr.shape}")
    P, Al, C = rot.shape[0], lig.shape[0], g.shape[0]
    out = {"sum_q": np.zeros((P, C), np.int64), "n_inside": np.zeros(P, np.int32), "n_above": np.zeros(P, np.int32)}
    if per_atom:
        out["atom_q"] = np.zeros((P, Al), np.int64)
    cen = np.asarray(center, np.float32).reshape(3)
    for p in range(P):
        if not (np.isfinite(rot[p]).all() and np.isfinite(tr[p]).all()):
            continue
        val, inside = _interpolate(g, o, v, ST.pose_atoms(lig, cen, rot[p], tr[p]))
        q = np.where(inside[None], np.rint((w[None] * val) * QUANTA), 0.0).astype(np.int64)
        out["sum_q"][p], out["n_inside"][p] = q.sum(1), inside.sum()
        out["n_above"][p] = (inside & (val[0] >= thr)).sum()
        if per_atom:
            out["atom_q"][p] = q[0]
    return out


def units(q):
    """Quanta -> units of w * val (float64; exact for |q| < 2^53)."""
    return np.asarray(q, np.int64).astype(np.float64) / QUANTA


# ---- MRC2014 ---------------------------------------------------------------------------------------------------------------------------
def read_mrc(path):
    """An MRC2014 / CCP4 map as {grid [nz,ny,nx] float32, origin [3] float32, voxel [3] float32 (x, y, z; A)}.  Modes 0 (int8), 1 (int16),
    2 (float32), 6 (uint16) and 12 (float16), either byte order, mapc / mapr / maps in any order, nsymbt bytes of extended header skipped.
    The origin is words 50-52 when one of them is non-zero, otherwise nxstart / nystart / nzstart times the voxel.  ValueError for a cell
    angle other than 90 degrees, an unsupported mode, a header that makes no sense or a file shorter than its header says."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 1024:
        raise ValueError(f"{path}: {len(raw)} bytes are no MRC header (1024)")
    for bo in ("<", ">"):
        iw = np.frombuffer(raw[:1024], bo + "i4")
        if int(iw[3]) in _MRC_MODES and all(1 <= int(n) <= 1 << 16 for n in iw[:3]):
            break
    else:
        raise ValueError(f"{path}: mode {int(np.frombuffer(raw[12:16], '<i4')[0])} is not one of {sorted(_MRC_MODES)} in either byte order")
    fw = np.frombuffer(raw[:1024], bo + "f4")
    nc, nr, ns, mode = (int(x) for x in iw[:4])
    start, m = [int(x) for x in iw[4:7]], [int(x) for x in iw[7:10]]
    cell, angles = fw[10:13].astype(np.float64), fw[13:16].astype(np.float64)
    order = [int(x) for x in iw[16:19]]      # mapc, mapr, maps: the spatial axis (1 = x, 2 = y, 3 = z) of columns, rows, sections
    nsymbt = int(iw[23])
    if sorted(order) != [1, 2, 3]:
        raise ValueError(f"{path}: mapc / mapr / maps = {order} is no permutation of 1, 2, 3")
    if not np.all(np.abs(angles - 90.0) <= 1e-3):
        raise ValueError(f"{path}: cell angles {angles.tolist()} - only orthogonal cells (90 degrees) are supported")
    if nsymbt < 0 or min(m) < 1 or not (np.isfinite(cell).all() and (cell > 0).all()):
        raise ValueError(f"{path}: header with nsymbt {nsymbt}, sampling {m}, cell {cell.tolist()}")
    dt = np.dtype(bo + _MRC_MODES[mode])
    n = nc * nr * ns
    body = raw[1024 + nsymbt:1024 + nsymbt + n * dt.itemsize]
    if len(body) < n * dt.itemsize:
        raise ValueError(f"{path}: truncated - {len(raw)} bytes, the header asks for {1024 + nsymbt + n * dt.itemsize}")
    data = np.frombuffer(body, dt).reshape(ns, nr, nc).astype(np.float32)
    axis_of = {order[0]: 2, order[1]: 1, order[2]: 0}      # spatial axis -> axis of data
    grid = np.ascontiguousarray(data.transpose(axis_of[3], axis_of[2], axis_of[1]))
    voxel = cell / np.asarray(m, np.float64)      # x, y, z
    origin = fw[49:52].astype(np.float64)
    if not origin.any():
        origin = np.array([start[order.index(k)] for k in (1, 2, 3)], np.float64) * voxel
    return {"grid": grid, "origin": origin.astype(np.float32), "voxel": voxel.astype(np.float32)}


def write_mrc(path, grid, origin, voxel, mode=2, order=(1, 2, 3), big_endian=False, nsymbt=0, origin_in_start=False):
    """Write grid [nz,ny,nx] as an MRC2014 map: `mode` 0, 1, 2, 6 or 12 (the values are cast), columns / rows / sections along the spatial
    axes `order` = (mapc, mapr, maps), `nsymbt` zero bytes of extended header; the origin goes to words 50-52, or with `origin_in_start`
    (it must then be a whole number of voxels) to nxstart / nystart / nzstart."""
    g = np.asarray(grid)
    if g.ndim != 3 or mode not in _MRC_MODES or sorted(order) != [1, 2, 3]:
        raise ValueError(f"write_mrc: grid {g.shape}, mode {mode}, order {order}")
    bo = ">" if big_endian else "<"
    o, v = np.asarray(origin, np.float64).reshape(3), np.asarray(voxel, np.float64).reshape(3)
    data = g.transpose(*(3 - order[k] for k in (2, 1, 0)))      # [sections, rows, columns]; spatial axis k is grid axis 3 - k
    ns, nr, nc = data.shape
    m = [g.shape[2], g.shape[1], g.shape[0]]
    iw = np.zeros(256, bo + "i4")
    fw = iw.view(bo + "f4")
    iw[0:4] = [nc, nr, ns, mode]
    iw[7:10] = m
    fw[10:13] = v * m
    fw[13:16] = 90.0
    iw[16:19] = order
    fw[19:22] = [float(g.min()), float(g.max()), float(g.mean())]
    iw[22], iw[23] = 1, int(nsymbt)
    if origin_in_start:
        st = np.rint(o / v).astype(np.int64)
        if not np.allclose(st * v, o, rtol=0, atol=1e-4):
            raise ValueError("write_mrc: origin_in_start needs an origin of whole voxels")
        iw[4:7] = [int(st[order[k] - 1]) for k in range(3)]
    else:
        fw[49:52] = o
    head = bytearray(iw.tobytes())
    head[208:212] = b"MAP "
    head[212:216] = bytes([0x11, 0x11, 0, 0]) if big_endian else bytes([0x44, 0x44, 0, 0])
    head[216:220] = np.array([float(g.std())], bo + "f4").tobytes()
    with open(path, "wb") as f:
        f.write(bytes(head))
        f.write(b"\0" * int(nsymbt))
        f.write(np.ascontiguousarray(data).astype(np.dtype(bo + _MRC_MODES[mode])).tobytes())


# ---- simulated maps and the closed form --------------------------------------------------------------------------------------------------
def _axis_gauss(x, n, o, v, sigma):
    """[len(x), n] = the normalised 1-D Gaussian of width sigma about each x at the nodes o + i v."""
    d = (o + v * np.arange(n))[None] - np.asarray(x, np.float64)[:, None]
    return np.exp(-0.5 * (d / sigma) ** 2) / (np.sqrt(2.0 * np.pi) * sigma)


def simulate_map(atoms, w, sigma, shape, origin, voxel):
    """rho [nz,ny,nx] float64 = sum_a w_a g(x - y_a) at every node x, g the normalised 3-D Gaussian of width sigma (A): the whole sum,
    no cutoff.  sigma = resolution * SIGMA_FACTOR is the module's convention for a map `at a resolution`."""
    y = np.asarray(atoms, np.float64).reshape(-1, 3)
    w = np.asarray(w, np.float64).reshape(-1)
    nz, ny, nx = (int(n) for n in shape)
    o, v = np.asarray(origin, np.float64).reshape(3), np.asarray(voxel, np.float64).reshape(3)
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError("sigma must be finite and > 0")
    ex, ey, ez = _axis_gauss(y[:, 0], nx, o[0], v[0], sigma), _axis_gauss(y[:, 1], ny, o[1], v[1], sigma), _axis_gauss(y[:, 2], nz, o[2], v[2], sigma)
    zy = ((w[:, None] * ez)[:, :, None] * ey[:, None, :]).reshape(y.shape[0], nz * ny)
    return (zy.T @ ex).reshape(nz, ny, nx)


def _blur(grid, voxel, sigma):
    """M [nz,ny,nx] = sum over nodes x' of g(x - x') grid(x'): the discrete, separable convolution with the normalised Gaussian."""
    out = np.asarray(grid, np.float64)
    for axis, v in zip((2, 1, 0), np.asarray(voxel, np.float64)):
        n = out.shape[axis]
        k = _axis_gauss(v * np.arange(n), n, 0.0, v, sigma)      # [n, n], symmetric
        out = np.moveaxis(np.tensordot(k, np.moveaxis(out, axis, 0), axes=(1, 0)), 0, axis)
    return out


def self_overlap(atoms, w, sigma, voxel):
    """sum_a sum_b w_a w_b g2(y_a - y_b) / dV: the sum over nodes of a simulated chain's square, taken analytically (g2 = g * g, the
    Gaussian of width sigma sqrt(2); dV the voxel's volume)."""
    y, w = np.asarray(atoms, np.float64).reshape(-1, 3), np.asarray(w, np.float64).reshape(-1)
    s2 = 2.0 * sigma * sigma
    tot = 0.0
    for lo in range(0, y.shape[0], 512):
        d2 = ((y[lo:lo + 512, None, :] - y[None, :, :]) ** 2).sum(-1)
        tot += float((w[lo:lo + 512, None] * w[None, :] * np.exp(-0.5 * d2 / s2)).sum())
    return tot / ((2.0 * np.pi * s2) ** 1.5 * float(np.prod(np.asarray(voxel, np.float64))))


def channels(map, rec_atoms, rec_w, sigma, lig_atoms=None, lig_w=None):
    """(grids [3,nz,ny,nx] float32, scalars) of a map (read_mrc's dict) and the receptor in the map's frame, for a ligand simulated at
    `sigma`.  Every sum <.,.> is over the nodes of the map's grid.
      channel 0   E: the map scaled to zero mean and unit variance, clipped to the value limit - what n_above / inclusion look at
      channel 1   M1 = g * E, the map blurred with the atom Gaussian (separable, discrete): sum_a w_a M1(y_a) ~ <S_lig, E>
      channel 2   M2 = sum_b w_b g2(x - y_b) / dV over the receptor's atoms, g2 = g * g analytic at sigma sqrt(2): sum_a w_a M2(y_a) ~
                  <S_lig, S_rec>
    scalars: E2 = |E|^2, C_rE = <S_rec, E>, S_rr = <S_rec, S_rec> (S_rec = simulate_map of the receptor on the grid) and, when the ligand is
    given, S_ll = self_overlap of the ligand (a rigid ligand's does not depend on the pose)."""
    grid = np.asarray(map["grid"], np.float64)
    o, v = np.asarray(map["origin"], np.float64), np.asarray(map["voxel"], np.float64)
    sd = grid.std()
    if not (np.isfinite(sd) and sd > 0):
        raise ValueError("the map is constant or not finite")
    E = np.clip((grid - grid.mean()) / sd, -MAX_VALUE, MAX_VALUE).astype(np.float32).astype(np.float64)
    ra, rw = np.asarray(rec_atoms, np.float64).reshape(-1, 3), np.asarray(rec_w, np.float64).reshape(-1)
    S_rec = simulate_map(ra, rw, sigma, grid.shape, o, v)
    M1 = _blur(E, v, sigma)
    M2 = simulate_map(ra, rw, sigma * np.sqrt(2.0), grid.shape, o, v) / float(np.prod(v))
    grids = np.clip(np.stack([E, M1, M2]), -MAX_VALUE, MAX_VALUE).astype(np.float32)
    scalars = {"E2": float((E * E).sum()), "C_rE": float((S_rec * E).sum()), "S_rr": float((S_rec * S_rec).sum()), "sigma": float(sigma)}
    if lig_atoms is not None:
        scalars["S_ll"] = self_overlap(lig_atoms, lig_w, sigma, v)
    return grids, scalars


def correlation(sum_q, scalars):
    """CC [P] = (C_rE + N) / sqrt(|E|^2 (S_rr + 2 X + S_ll)), N = sum_q[:, 1] 2^-20, X = sum_q[:, 2] 2^-20: the overlap correlation of the
    simulated complex with the map, every pose-dependent term a gather (channels explains the grids).  NaN where the root is not > 0."""
    q = np.asarray(sum_q, np.int64)
    N, X = units(q[:, 1]), units(q[:, 2])
    den = scalars["E2"] * (scalars["S_rr"] + 2.0 * X + scalars["S_ll"])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, (scalars["C_rE"] + N) / np.sqrt(np.where(den > 0, den, 1.0)), np.nan)


def brute_force_correlation(map, rec_atoms, rec_w, posed_lig_atoms, lig_w, sigma):
    """The same correlation without the closed form: the posed complex simulated on the map's grid and correlated with E node by node.
    What correlation() differs from this by is the discretisation error of the definition (tests/test_density_cpu.py measures it)."""
    grid = np.asarray(map["grid"], np.float64)
    E = np.clip((grid - grid.mean()) / grid.std(), -MAX_VALUE, MAX_VALUE).astype(np.float32).astype(np.float64)
    atoms = np.concatenate([np.asarray(rec_atoms, np.float64).reshape(-1, 3), np.asarray(posed_lig_atoms, np.float64).reshape(-1, 3)])
    w = np.concatenate([np.asarray(rec_w, np.float64).reshape(-1), np.asarray(lig_w, np.float64).reshape(-1)])
    S = simulate_map(atoms, w, sigma, grid.shape, map["origin"], map["voxel"])
    return float((S * E).sum() / np.sqrt((S * S).sum() * (E * E).sum()))


def inclusion(n_above, Al):
    """n_above / Al: the share of the ligand's atoms that sit in density above the threshold."""
    return np.asarray(n_above, np.float64) / float(Al)


def residue_density(atom_q, res, n_res):
    """Per-atom quanta [.., n] summed per residue -> [.., n_res] int64 (sterics.residue_counts)."""
    return ST.residue_counts(atom_q, res, n_res)


ATOMIC_NUMBER = {"C": 6.0, "N": 7.0, "O": 8.0, "S": 16.0, "P": 15.0, "SE": 34.0}


def atom_weights(atoms, index):
    """The weight of the atoms `index` of pdbio.read_pdb records: the element's atomic number (ifenergy.element_of; 6 for an element
    this table does not hold)."""
    from . import ifenergy as IE
    return np.asarray([ATOMIC_NUMBER.get(IE.element_of(atoms[int(i)]).upper(), 6.0) for i in index], np.float32)


def write_density_residues(path, keys, mean_val):
    """--density-residues: one line `chain:resnum[icode] res_name mean` per ligand residue - the mean of w * val of channel 0 over the
    residue's heavy atoms, in units of the normalised map times the atomic number."""
    with open(path, "w") as f:
        f.write("# ligand residue, name, mean weighted value of the normalised map over the residue's heavy atoms\n")
        for k, v in zip(keys, mean_val):
            f.write(f"{k[0]}:{int(k[1])}{k[2] if k[2] != ' ' else ''} {k[3]} {float(v):.6f}\n")
