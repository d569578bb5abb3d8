"""Host replay of one dfm_refine trajectory through the CPU oracle (tests/test_gpu_refine.py): start draws -> the mirror's forward
marginal (dfmdock_amd/refine.py) -> oracle.modify_coords, then per step Oracle.score -> oracle.torch_reverse -> oracle.modify_coords /
rot_compose over the refine grid, with the edge lists drawn by oracle.knn_sample on the ORACLE's own poses.  Everything the engine needs
injected comes back in the dict."""
import numpy as np

CONTACT_CUTOFF = 8.0      # the restraint module's contact cutoff (restraints.native_contact_groups)


def contacts(rec_pos, lig_pos, cutoff=CONTACT_CUTOFF):
    """Receptor-ligand CA pairs within `cutoff` A."""
    d = np.linalg.norm(np.asarray(rec_pos, np.float64)[:, None, 1, :] - np.asarray(lig_pos, np.float64)[None, :, 1, :], axis=-1)
    return int((d < cutoff).sum())


def oracle_refine_replay(blob, cx, t_begin, steps=40, eps=1e-3, seed=0, noise_scale=0.5):
    from dfmdock_amd import refine as RF
    from oracle import oracle as ora
    rng = np.random.Generator(np.random.PCG64(seed))
    u = rng.uniform(0.01, 0.99, size=1).astype(np.float32)
    axis = rng.standard_normal(3).astype(np.float32)
    z0 = rng.standard_normal(3).astype(np.float32)
    z_rot = rng.standard_normal((steps, 3)).astype(np.float32)
    z_tr = rng.standard_normal((steps, 3)).astype(np.float32)
    rot0, tr0 = RF.forward_marginal(np.float32(t_begin), u, axis, z0)
    rot0, tr0 = rot0[0].astype(np.float32), tr0[0].astype(np.float32)
    o = ora.Oracle(blob, cx)
    rec = np.asarray(cx["rec_pos"], np.float32)
    pose = ora.modify_coords(cx["lig_pos"], rot0, tr0)
    ts, dt = RF.time_grid(t_begin, eps, steps)
    g3, gso, _, _ = ora.diffusion_coefs(ts)
    out = dict(u_angle=u, axis_draw=axis, tr_draw=z0, z_rot=z_rot, z_tr=z_tr, init_pose=pose.copy(), rot0=rot0, tr0=tr0, ts=ts,
               poses=np.zeros((steps,) + pose.shape, np.float32), edges=np.zeros((steps + 1, o.N, o.K), np.int32),
               contacts=np.zeros(steps, np.int64), scores=np.zeros((steps + 1, 6), np.float32))
    rot_u, tr_u = rot0.copy(), tr0.copy()
    for i in range(steps + 1):
        ca = np.concatenate([rec[:, 1, :], pose[:, 1, :]], 0)
        e = ora.knn_sample(ca, seed=seed * 1000 + i)
        out["edges"][i] = e
        r = o.score(pose, ts[min(i, steps - 1)], edges=e, debug=False)
        out["scores"][i, :3], out["scores"][i, 3:] = r["tr_score"][0], r["rot_score"][0]
        if i == steps:
            out["energy"] = float(r["energy"])
            break
        ns = 0.0 if i == steps - 1 else noise_scale
        rot = ora.torch_reverse(gso[i], r["rot_score"][0], dt, ns, z_rot[i])
        tr = ora.torch_reverse(g3[i], r["tr_score"][0], dt, ns, z_tr[i])
        pose = ora.modify_coords(pose, rot, tr)
        rot_u = ora.rot_compose(rot_u, rot)[0]
        tr_u = tr_u + tr
        out["poses"][i] = pose
        out["contacts"][i] = contacts(rec, pose)
    out["rot_update"], out["tr_update"] = rot_u, tr_u
    return out
