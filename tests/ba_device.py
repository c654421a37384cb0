"""What the GPU tests of the dense BA share (tests/test_gpu_ba_edges.py, tests/test_gpu_ba_solvers.py): a case of
oracle/ba_cases.py or oracle/solver_cases.py through `slam_ext.dense_ba` in buffers with frames beyond the graph, and the
comparison of what comes back with the float64 oracle at per-output bounds."""

import numpy as np
import torch

from oracle import se3 as ose3
from vipe_amd.synth import expand_edges

GUARD = 2  # frames beyond the graph in the pose and disparity buffers


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def _padded(a, rows, fill):
    """[rows + extra, ...] float32: `a` and then sentinel rows cycling through `fill`"""
    a = np.asarray(a, np.float32)
    tail = np.resize(np.asarray(fill, np.float32), (rows,) + a.shape[1:])
    return np.concatenate([a, tail])


def case_tensors(c):
    """the device arguments of `slam_ext.dense_ba` that a call only reads (everything but poses, disps, intrinsics, rig)
    -> dict; the index tensors keep their addresses, so calls that share it can share a plan"""
    g = c.g
    V = g.V if c.rig else 1
    n, ht, wd = g.n, g.ht, g.wd
    pi, qi, di, pj, qj = expand_edges(g.ii, g.jj, V)
    M = len(pi)
    flat = lambda a: np.asarray(a).reshape(n * V, ht, wd)
    return dict(sens=T(_padded(flat(g.disps_sens), GUARD * V, [0.0])), eta=T(_padded(flat(g.eta), GUARD * V, [0.01])),
                target=T(g.target.reshape(M, -1, 2)), weight=T(g.weight.reshape(M, -1, 2)),
                index=[T(x) for x in (pi, qi, pj, qj, di)])


def run_case(c, opts=0, tensors=None, **call_kw):
    """`slam_ext.dense_ba` on a case, in buffers of n + GUARD poses / (n + GUARD) V frames.  The sentinel poses must keep
    their bits; the sentinel disparities (0.5 and 1e-5 in turn) change only by the clamp at 1e-3 of the whole buffer
    (buffer.py:525).  `call_kw`: further keyword arguments of the call (`state=`, `plan_key=`).
    -> poses [n,7], disps like g.disps, intrinsics, rig, info"""
    from vipe_amd.ext import slam_ext
    g = c.g
    V = g.V if c.rig else 1
    n, ht, wd = g.n, g.ht, g.wd
    flat = lambda a: np.asarray(a).reshape(n * V, ht, wd)
    sentinel_pose = np.array([[0.3, -0.2, 0.1, 0.5, -0.5, 0.5, 0.5], [7.0, 8.0, 9.0, 0.0, 0.6, 0.0, 0.8]], np.float32)
    poses = T(_padded(g.poses, GUARD, sentinel_pose))
    disps = T(_padded(flat(g.disps), GUARD * V, [0.5, 1e-5]))
    t = case_tensors(c) if tensors is None else tensors
    intr = T(c.intr).clone()
    rig = T(g.rig if c.rig else ose3.se3_identity(1)).clone()
    tail_p, tail_d = poses[n:].clone(), disps[n * V:].clone()
    pi, qi, pj, qj, di = t["index"]
    info = slam_ext.dense_ba(poses, disps, t["sens"], intr, rig, t["target"], t["weight"], t["eta"], pi, qi, pj, qj, di,
                             camera=c.cam, want_info=True, solver_options=opts, **c.bk, **call_kw)
    torch.cuda.synchronize()
    assert torch.equal(poses[n:].view(torch.int32), tail_p.view(torch.int32)), "a pose beyond the graph was written"
    assert torch.equal(disps[n * V:], tail_d.clamp(min=1e-3)), "disparities beyond the graph: only the 1e-3 clamp may act"
    return (poses[:n].cpu().numpy(), disps[:n * V].cpu().numpy().reshape(g.disps.shape), intr.cpu().numpy(),
            rig.cpu().numpy(), info.cpu().numpy())


def option_sets():
    from vipe_amd.ext import slam_ext
    return {"default": 0, "general": slam_ext.BA_OPT_ONE_CHAIN | slam_ext.BA_OPT_GENERAL_ACCUMULATE}


def check_outputs(name, tag, got, o64, bounds):
    """poses, disps, intrinsics, rig of `got` against the float64 oracle's `o64`, each within its bound of `bounds`
    (output -> (delta32, bound)); every figure is printed before the first assertion.  -> output -> kernel error"""
    p, d, k, r = got[:4]
    outs = {"poses": p, "disps": d.reshape(o64[1].shape), "intr": k, "rig": r}
    errs = {}
    for (key, (d32, bound)), ref in zip(bounds.items(), o64):
        errs[key] = float(np.nan_to_num(np.abs(outs[key].astype(np.float64) - ref), nan=np.inf).max())
        ratio = errs[key] / d32 if d32 > 0 else (0.0 if errs[key] == 0 else np.inf)
        print(f"{name} [{tag}] {key}: kernel error {errs[key]:.3g}, delta32 {d32:.3g}, ratio {ratio:.3g}, bound {bound:.3g}")
    for key, (d32, bound) in bounds.items():
        assert errs[key] <= bound, (name, tag, key, errs[key], d32, bound)
    return errs
