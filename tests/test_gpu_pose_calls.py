"""What the six rigid-pose calls share on the host (dfmdock_amd/csrc/api_pose.hip: one frame builder, one handle base, one chunk driver): on
the same coordinates and the same reach the five cutoff-based handles (the pair potential's reach is its last edge) report the same grid, and every call's results do not depend on
how its poses are cut into chunks.  130 receptor and 65 ligand atoms: the ligand has two blocks of 64, the second holding one atom."""
import numpy as np
import pytest

from test_hbonds_cpu import lump, poses

pytestmark = pytest.mark.gpu

REACH = 5.5


@pytest.fixture(scope="module")
def handles(blob):
    from dfmdock_amd import engine
    engine.set_device(0)
    model = engine.Model(blob)
    rng = np.random.default_rng(3)
    rec, lig = lump(rng, 130, 12, (0, 0, 0), 6.0), lump(rng, 65, 7, (5, 0, 0), 4.0)      # every atom has a role
    cen = lig["xyz"].astype(np.float64).mean(0).astype(np.float32)
    params = lambda n: np.stack([rng.uniform(1.0, 2.2, n), rng.uniform(0.05, 0.5, n), rng.uniform(-1.0, 1.0, n)], 1).astype(np.float32)
    h = {"sterics": model.atoms(rec["xyz"], lig["xyz"], cen, 3.0, REACH),
         "iface": model.interface(rec["xyz"], params(130), lig["xyz"], params(65), cen, cutoff=REACH),
         "rescon": model.contacts(rec["xyz"], rec["res"], rng.integers(0, 3, 12), lig["xyz"], lig["res"], rng.integers(0, 3, 7), cen, REACH),
         "hbond": model.hbonds(rec, lig, cen, 3.5, 90.0, REACH),
         "pairpot": model.pairpot(rec["xyz"], rng.integers(0, 3, 130), lig["xyz"], rng.integers(0, 3, 65), cen,
                                  np.linspace(1.0, REACH, 7).astype(np.float32), rng.uniform(-3.0, 3.0, (3, 3, 6)).astype(np.float32)),
         "surface": model.surface(rec["xyz"], rng.choice(np.float32([1.5, 1.7, 1.9]), 130), lig["xyz"], rng.choice(np.float32([1.5, 1.7, 1.9]), 65),
                                  cen)}
    yield h
    for v in h.values():
        v.close()
    model.close()


def test_same_coordinates_same_grid(handles):
    grids = {k: {f: v.info()[f] for f in ("n_cells", "max_cell_atoms", "cell_edge")} for k, v in handles.items() if k != "surface"}
    assert len(grids) == 5 and all(g == grids["sterics"] for g in grids.values()), grids
    assert grids["sterics"]["cell_edge"] == REACH and grids["sterics"]["n_cells"] > 1


def test_results_do_not_depend_on_the_chunks(handles):
    rot, tr = poses(np.random.default_rng(4), 5)
    calls = {"sterics": lambda c: handles["sterics"].sterics(rot, tr, per_atom=True, chunk_poses=c),
             "surface": lambda c: handles["surface"].bsa(rot, tr, per_atom=True, chunk_poses=c),
             "iface": lambda c: handles["iface"].energy(rot, tr, per_atom=True, chunk_poses=c),
             "rescon": lambda c: handles["rescon"].count(rot, tr, per_residue=True, bits=True, chunk_poses=c),
             "hbond": lambda c: handles["hbond"].count(rot, tr, per_atom=True, chunk_poses=c),
             "pairpot": lambda c: handles["pairpot"].energy(rot, tr, per_atom=True, counts=True, chunk_poses=c)}
    live = {"sterics": "n_contact", "surface": "lig_points", "iface": "n_pairs", "rescon": "n_pairs", "hbond": "n_hbond", "pairpot": "n_pairs"}
    assert calls.keys() == handles.keys() and len(calls) == 6
    for name, call in calls.items():
        whole, cut = call(0), call(2)      # one chunk of 5 | two full chunks and a ragged one
        assert whole.keys() == cut.keys(), name
        for k, v in whole.items():
            a, b = np.asarray(v), np.asarray(cut[k])
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, k)
        assert np.asarray(whole[live[name]]).sum() > 0, name      # the poses touch: the comparison is not of zeros
