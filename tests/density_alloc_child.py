"""The child process of tests/test_gpu_density.py: test_under_the_allocator_diagnostics.  One handle on a seeded three-channel grid and a
seeded lump of weighted atoms, one dfm_pose_density call with every output in two chunks and one lean call; every output is stored under a
stable key next to the keys that differ from the float64 definition, `alloc_diag()` and `config_string()` after the handle is closed and
the block cache trimmed.

    python tests/density_alloc_child.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    if len(argv) != 2:
        print(f"usage: {argv[0]} OUT.npz", file=sys.stderr)
        return 2
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import alloc_recipe as ar
    from dfmdock_amd import engine, density as DN
    from dfmdock_amd.weights import make_random_weights, pack_blob
    rng = np.random.default_rng(29)
    grids = rng.uniform(-3.0, 3.0, (3, 9, 11, 10)).astype(np.float32)
    origin, voxel = np.float32([-2.0, 1.0, 0.5]), np.float32([1.5, 1.0, 2.0])
    lig = (rng.random((100, 3)) * [12.0, 9.0, 14.0] + [-1.0, 1.5, 1.0]).astype(np.float32)
    w = rng.uniform(-8.0, 8.0, 100).astype(np.float32)
    cen = lig.mean(0)
    rot, tr = (0.3 * rng.standard_normal((6, 3))).astype(np.float32), (1.5 * rng.standard_normal((6, 3))).astype(np.float32)
    want = DN.density(grids, origin, voxel, lig, w, cen, rot, tr, 0.5, per_atom=True)
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0)))
    with model.density(grids, origin, voxel, lig, w, cen, 0.5) as h:
        full = h.fit(rot, tr, per_atom=True, chunk_poses=4)
        lean = h.fit(rot, tr)
    model.close()
    engine.trim_cache()
    out = {f"full/{k}": v for k, v in full.items()}
    out.update({f"lean/{k}": v for k, v in lean.items()})
    differs = [k for k in full if not np.array_equal(full[k], want[k])] + [k for k in lean if not np.array_equal(lean[k], want[k])]
    d = engine.alloc_diag()
    out["__differs_from_definition"] = np.array(differs, dtype="U40")
    out["__diag"] = np.array([d[k] for k in ar.DIAG], np.int64)
    out["__config"] = np.array(engine.config_string())
    np.savez(argv[1], **out)
    print(f"{len(out) - 3} keys, differs from the definition at {differs}, diag {out['__diag'].tolist()}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
