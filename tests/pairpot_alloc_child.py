"""The child process of tests/test_gpu_pairpot.py: test_under_the_allocator_diagnostics.  One handle on a seeded pair of typed lumps, one
dfm_pose_pairpot call with every output in two chunks and one lean call; every output is stored under a stable key next to the keys that
differ from the float64 definition, `alloc_diag()` and `config_string()` after the handle is closed and the block cache trimmed.

    python tests/pairpot_alloc_child.py OUT.npz
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
    from dfmdock_amd import engine, pairpot as PP
    from dfmdock_amd.weights import make_random_weights, pack_blob
    rng = np.random.default_rng(23)
    T, NB = 5, 12
    rec, lig = (9.0 * rng.random((180, 3))).astype(np.float32), (6.0 * rng.random((100, 3)) + 2.0).astype(np.float32)
    rt, lt = rng.integers(0, T, 180).astype(np.int32), rng.integers(0, T, 100).astype(np.int32)
    edges = np.linspace(1.0, 9.0, NB + 1).astype(np.float32)
    table = rng.uniform(-4.0, 4.0, (T, T, NB)).astype(np.float32)
    cen = lig.mean(0)
    rot, tr = (0.3 * rng.standard_normal((6, 3))).astype(np.float32), (1.5 * rng.standard_normal((6, 3))).astype(np.float32)
    want = PP.pair_potential(rec, rt, lig, lt, cen, rot, tr, edges, table, per_atom=True, counts=True)
    engine.set_device(0)
    model = engine.Model(pack_blob(make_random_weights(0)))
    with model.pairpot(rec, rt, lig, lt, cen, edges, table) as h:
        full = h.energy(rot, tr, per_atom=True, counts=True, chunk_poses=4)
        lean = h.energy(rot, tr)
    model.close()
    engine.trim_cache()
    out = {f"full/{k}": v for k, v in full.items()}
    out.update({f"lean/{k}": v for k, v in lean.items()})
    differs = [k for k in full if k in want and not np.array_equal(full[k], want[k])] + [k for k in lean if k in want and not np.array_equal(lean[k], want[k])]
    d = engine.alloc_diag()
    out["__differs_from_definition"] = np.array(differs, dtype="U40")
    out["__diag"] = np.array([d[k] for k in ar.DIAG], np.int64)
    out["__config"] = np.array(engine.config_string())
    np.savez(argv[1], **out)
    print(f"{len(out) - 3} keys, differs from the definition at {differs}, diag {out['__diag'].tolist()}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
