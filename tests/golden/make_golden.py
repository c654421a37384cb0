"""Generate golden fixtures from the reference's own Python files (build container only).

Run:  python tests/golden/make_golden.py  [/root/reference]

The reference package cannot be imported as a whole (omegaconf/hydra/cv2 absent, and
`vipe.ext` would JIT-compile CUDA sources), so the individual hot-path files are
loaded by path under their dotted names with `vipe.ext`'s NATIVE modules stubbed:
  * vipe.ext.lietorch_ext  -> oracle.se3 closed forms (SE3 only).  The reference's
    pure-Python lietorch wrapper (vipe/ext/lietorch/*.py) is the real one.
  * vipe.ext.{scatter_ext,droid_net_ext,slam_ext} -> empty namespaces (never called:
    scatter_add/scatter_mean go through torch.scatter_add_, vipe/ext/scatter.py:24-53).
Only DATA (inputs + outputs) is written, as .npz next to this script.
"""

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import se3 as ose3  # noqa: E402
from vipe_amd.synth import make_graph, make_tracks  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"


def _np(t):
    return t.detach().cpu().numpy()


def _wrap(fn):
    def f(gid, *args):
        assert gid == 3, "only SE3 is stubbed"
        out = fn(*[_np(a) for a in args])
        return torch.from_numpy(np.ascontiguousarray(out)).to(args[0].dtype)
    return f


def _load(name, relpath):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    parent, _, child = name.rpartition(".")
    if parent in sys.modules:
        setattr(sys.modules[parent], child, mod)
    return mod


def load_reference():
    for pkg in ["vipe", "vipe.ext", "vipe.ext.lietorch", "vipe.utils", "vipe.slam", "vipe.slam.maths",
                "vipe.slam.ba", "vipe.slam.networks"]:
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
        parent, _, child = pkg.rpartition(".")
        if parent:
            setattr(sys.modules[parent], child, m)
    ext = sys.modules["vipe.ext"]
    for n in ["scatter_ext", "droid_net_ext", "slam_ext"]:
        setattr(ext, n, types.SimpleNamespace())
    lie = types.SimpleNamespace(
        expm=_wrap(ose3.se3_exp), logm=_wrap(ose3.se3_log), inv=_wrap(ose3.se3_inv), mul=_wrap(ose3.se3_mul),
        adj=_wrap(ose3.se3_adj), adjT=_wrap(ose3.se3_adjT), act=_wrap(ose3.se3_act3), act4=_wrap(ose3.se3_act4),
    )
    def _absent(*a, **k):
        raise NotImplementedError("backward / auxiliary lietorch ops are not needed under torch.no_grad")

    for n in ["expm", "logm", "inv", "mul", "adj", "adjT", "act", "act4"]:
        setattr(lie, n + "_backward", _absent)
    lie.Jinv = lie.projector = _absent
    lie.as_matrix = _wrap(ose3.se3_matrix)
    ext.lietorch_ext = lie
    sys.modules["vipe.ext.lietorch_ext"] = lie
    _load("vipe.ext.lietorch.broadcasting", "vipe/ext/lietorch/broadcasting.py")
    _load("vipe.ext.lietorch.group_ops", "vipe/ext/lietorch/group_ops.py")
    g = _load("vipe.ext.lietorch.groups", "vipe/ext/lietorch/groups.py")
    lt = sys.modules["vipe.ext.lietorch"]
    for n in ["SE3", "SO3", "Sim3", "RxSO3", "cat", "stack"]:
        setattr(lt, n, getattr(g, n))
    R = types.SimpleNamespace()
    R.scatter = _load("vipe.ext.scatter", "vipe/ext/scatter.py")
    R.cameras = _load("vipe.utils.cameras", "vipe/utils/cameras.py")
    R.vector = _load("vipe.slam.maths.vector", "vipe/slam/maths/vector.py")
    R.matrix = _load("vipe.slam.maths.matrix", "vipe/slam/maths/matrix.py")
    R.geom = _load("vipe.slam.maths.geom", "vipe/slam/maths/geom.py")
    R.retractor = _load("vipe.slam.maths.retractor", "vipe/slam/maths/retractor.py")
    R.kernel = _load("vipe.slam.ba.kernel", "vipe/slam/ba/kernel.py")
    R.terms = _load("vipe.slam.ba.terms", "vipe/slam/ba/terms.py")
    R.solver = _load("vipe.slam.ba.solver", "vipe/slam/ba/solver.py")
    R.droid_net = _load("vipe.slam.networks.droid_net", "vipe/slam/networks/droid_net.py")
    R.SE3 = g.SE3
    return R


def reference_ba(R, poses, disps, disps_sens, intrinsics, target, weight, eta, ii, jj, t0, t1, n_iters,
                 pose_damping, pose_ep, motion_only, limited_disp, optimize_intrinsics, camera="pinhole",
                 alpha=0.001, tracks=None):
    """Drive the reference Solver exactly as GraphBuffer.bundle_adjustment does (buffer.py:396-525), mono rig.
    `tracks` = (target, weight) of the second flow term the reference adds when sparse tracks are enabled
    (buffer.py:422-447, weight_tracks = 0.001)."""
    Solver, SparseBlockVector = R.solver.Solver, R.vector.SparseBlockVector
    T, RT = R.terms, R.retractor
    cam = R.cameras.CameraType.PINHOLE if camera == "pinhole" else R.cameras.CameraType.MEI
    poses = torch.tensor(poses).float().clone()
    N, ht, wd = disps.shape
    dis = torch.tensor(disps).float().clone().view(N, 1, ht, wd)
    sens = torch.tensor(disps_sens).float().view(N, ht * wd)
    intr = torch.tensor(intrinsics).float().clone()
    rig = torch.tensor([[0, 0, 0, 0, 0, 0, 1.0]])
    ii_t, jj_t = torch.tensor(ii), torch.tensor(jj)
    pi, pj = ii_t, jj_t
    qi = qj = torch.zeros_like(ii_t)
    di = pi
    di_unique, pi_unique = torch.unique(di), torch.unique(ii_t)
    E = len(ii)
    solver = Solver(compute_energy=True)
    solver.add_term(T.DenseDepthFlowTerm(
        pose_i_inds=pi, pose_j_inds=pj, rig_i_inds=qi, rig_j_inds=qj, dense_disp_i_inds=di,
        target=torch.tensor(target).float().reshape(E, ht * wd, 2),
        weight=0.001 * torch.tensor(weight).float().reshape(E, ht * wd, 2),
        intrinsics=None, intrinsics_factor=8.0, rig=None, image_size=(ht, wd), camera_type=cam))
    if tracks is not None:
        solver.add_term(T.DenseDepthFlowTerm(
            pose_i_inds=pi, pose_j_inds=pj, rig_i_inds=qi, rig_j_inds=qj, dense_disp_i_inds=di,
            target=torch.tensor(tracks[0]).float().reshape(E, ht * wd, 2),
            weight=0.001 * torch.tensor(tracks[1]).float().reshape(E, ht * wd, 2),
            intrinsics=None, intrinsics_factor=8.0, rig=None, image_size=(ht, wd), camera_type=cam))
    solver.set_fixed("pose", torch.cat([pi_unique[pi_unique < t0], pi_unique[pi_unique >= t1]]) if t0 < t1 else None)
    solver.set_retractor("pose", RT.PoseRetractor())
    solver.set_damping("pose", damping=pose_damping, ep=pose_ep)
    if not motion_only:
        sens_i = di_unique[sens[di_unique].sum(1) > 0.0]
        if len(sens_i) > 0:
            solver.add_term(T.DispSensRegularizationTerm(i_inds=sens_i, alpha=alpha, disps_sens=sens))
        solver.set_retractor("dense_disp", RT.DenseDispRetractor())
        damp = torch.tensor(eta).float().view(N, ht * wd)
        solver.set_damping("dense_disp", damping=SparseBlockVector(inds=di_unique, data=0.2 * damp[di_unique] + 1e-7),
                           ep=1e-7)
        if limited_disp:
            solver.set_fixed("dense_disp", torch.cat([di[pi < t0], di[pi >= t1]]))
    else:
        solver.set_fixed("dense_disp")
    solver.set_marginilized("dense_disp")
    solver.set_retractor("intrinsics", RT.IntrinsicsRetractor(cam))
    solver.set_damping("intrinsics", damping=1e-6, ep=1e-6)
    if not optimize_intrinsics:
        solver.set_fixed("intrinsics")
    solver.set_retractor("rig", RT.RigRotationOnlyRetractor())
    solver.set_damping("rig", damping=1e-4, ep=1e-4)
    solver.set_fixed("rig")
    flat = dis.view(N, ht * wd)
    energies = []
    for _ in range(n_iters):
        energies.append(solver.run_inplace({"pose": R.SE3(poses), "dense_disp": flat, "intrinsics": intr,
                                            "rig": R.SE3(rig)}))
    dis.clamp_(min=0.001)
    return _np(poses), _np(dis.view(N, ht, wd)), _np(intr), np.asarray(energies, dtype=np.float64)


BA_CASES = {
    # name: (graph kwargs, BA kwargs)
    "cfg1_pose_only": (dict(n=2, height=96, width=128, radius=1, seed=7),
                       dict(t0=1, t1=2, n_iters=3, pose_damping=1e-3, pose_ep=0.1, motion_only=True,
                            limited_disp=False, optimize_intrinsics=False)),
    "n5_frontend": (dict(n=5, height=96, width=128, radius=3, seed=11),
                    dict(t0=1, t1=5, n_iters=3, pose_damping=1e-3, pose_ep=0.1, motion_only=False,
                         limited_disp=False, optimize_intrinsics=False)),
    "n6_window_prior": (dict(n=6, height=96, width=128, radius=2, seed=13, depth_prior=True),
                        dict(t0=3, t1=6, n_iters=2, pose_damping=1e-3, pose_ep=0.1, motion_only=False,
                             limited_disp=False, optimize_intrinsics=False)),
    "n5_backend_intr": (dict(n=5, height=96, width=128, radius=3, seed=17),
                        dict(t0=1, t1=5, n_iters=2, pose_damping=1e-5, pose_ep=1e-2, motion_only=False,
                             limited_disp=False, optimize_intrinsics=True)),
    "n5_fixed_motion": (dict(n=5, height=96, width=128, radius=2, seed=19),
                        dict(t0=2, t1=2, n_iters=2, pose_damping=1e-3, pose_ep=0.1, motion_only=False,
                             limited_disp=False, optimize_intrinsics=False)),
    "n6_infill_motion_limited": (dict(n=6, height=96, width=128, radius=2, seed=23),
                                 dict(t0=4, t1=6, n_iters=2, pose_damping=1e-3, pose_ep=0.1, motion_only=True,
                                      limited_disp=True, optimize_intrinsics=False)),
    "n5_mei": (dict(n=5, height=96, width=128, radius=3, seed=29),
               dict(t0=1, t1=5, n_iters=2, pose_damping=1e-3, pose_ep=0.1, motion_only=False,
                    limited_disp=False, optimize_intrinsics=False, camera="mei", k1=0.35)),
    "n5_mei_intr": (dict(n=5, height=96, width=128, radius=3, seed=37),
                    dict(t0=1, t1=5, n_iters=2, pose_damping=1e-5, pose_ep=1e-2, motion_only=False,
                         limited_disp=False, optimize_intrinsics=True, camera="mei", k1=0.05)),
}


def gen_ba(R):
    out = {}
    for name, (gk, bk) in BA_CASES.items():
        g = make_graph(**gk)
        intr = g.intrinsics
        bk = dict(bk)
        k1 = bk.pop("k1", None)
        if bk.get("camera") == "mei":
            intr = np.concatenate([intr, np.array([[k1]], dtype=np.float32)], axis=1)
        p, d, k, en = reference_ba(R, g.poses, g.disps, g.disps_sens, intr, g.target, g.weight, g.eta, g.ii,
                                   g.jj, **bk)
        out[name + "/poses"] = p
        out[name + "/disps"] = d
        out[name + "/intrinsics"] = k
        out[name + "/energy"] = en
        print(name, "energy", en)
    np.savez_compressed(os.path.join(HERE, "ba_reference.npz"), **out)


BA_TRACKS_CASES = ["n5_frontend", "n6_window_prior", "n6_infill_motion_limited"]


def gen_ba_tracks(R):
    """Two flow terms on the same edges - the dense one and the sparse-track one - through the reference Solver."""
    out = {}
    for k, name in enumerate(BA_TRACKS_CASES):
        gk, bk = BA_CASES[name]
        g = make_graph(**gk)
        tt, tw = make_tracks(g, 100 + k)
        p, d, kk, en = reference_ba(R, g.poses, g.disps, g.disps_sens, g.intrinsics, g.target, g.weight, g.eta, g.ii,
                                    g.jj, tracks=(tt, tw), **bk)
        out[name + "/poses"], out[name + "/disps"], out[name + "/intrinsics"], out[name + "/energy"] = p, d, kk, en
        print(name, "+ tracks: energy", en)
    np.savez_compressed(os.path.join(HERE, "ba_tracks_reference.npz"), **out)


def reference_ba_rig(R, g, t0, t1, n_iters, pose_damping, pose_ep, motion_only=False, limited_disp=False,
                     optimize_intrinsics=False, optimize_rig_rotation=False, alpha=0.001):
    """The reference Solver on a multi-view rig exactly as GraphBuffer.bundle_adjustment sets it up (buffer.py:396-525):
    V views, per-view intrinsics, `expand_edge_multiview` terms incl. cross-view self edges, rig group with view 0
    fixed and the rotation-only retractor (buffer.py:497-506, retractor.py:32-37)."""
    from vipe_amd.synth import expand_edges
    Solver, SparseBlockVector = R.solver.Solver, R.vector.SparseBlockVector
    T, RT = R.terms, R.retractor
    cam = R.cameras.CameraType.PINHOLE
    V, N, ht, wd = g.V, g.n, g.ht, g.wd
    poses = torch.tensor(g.poses).float().clone()
    dis = torch.tensor(g.disps).float().clone().view(N * V, ht * wd)
    sens = torch.tensor(g.disps_sens).float().view(N * V, ht * wd)
    intr = torch.tensor(g.intrinsics).float().clone()
    rig = torch.tensor(g.rig).float().clone()
    pi, qi, di, pj, qj = (torch.tensor(x) for x in expand_edges(g.ii, g.jj, V))
    di_unique, pi_unique = torch.unique(di), torch.unique(torch.tensor(g.ii))
    M = len(pi)
    solver = Solver(compute_energy=True)
    solver.add_term(T.DenseDepthFlowTerm(
        pose_i_inds=pi, pose_j_inds=pj, rig_i_inds=qi, rig_j_inds=qj, dense_disp_i_inds=di,
        target=torch.tensor(g.target).float().reshape(M, ht * wd, 2),
        weight=0.001 * torch.tensor(g.weight).float().reshape(M, ht * wd, 2),
        intrinsics=None, intrinsics_factor=8.0, rig=None, image_size=(ht, wd), camera_type=cam))
    solver.set_fixed("pose", torch.cat([pi_unique[pi_unique < t0], pi_unique[pi_unique >= t1]]) if t0 < t1 else None)
    solver.set_retractor("pose", RT.PoseRetractor())
    solver.set_damping("pose", damping=pose_damping, ep=pose_ep)
    if not motion_only:
        sens_i = di_unique[sens[di_unique].sum(1) > 0.0]
        if len(sens_i) > 0:
            solver.add_term(T.DispSensRegularizationTerm(i_inds=sens_i, alpha=alpha, disps_sens=sens))
        solver.set_retractor("dense_disp", RT.DenseDispRetractor())
        damp = torch.tensor(g.eta).float().view(N * V, ht * wd)
        solver.set_damping("dense_disp", damping=SparseBlockVector(inds=di_unique, data=0.2 * damp[di_unique] + 1e-7),
                           ep=1e-7)
        if limited_disp:
            solver.set_fixed("dense_disp", torch.cat([di[pi < t0], di[pi >= t1]]))
    else:
        solver.set_fixed("dense_disp")
    solver.set_marginilized("dense_disp")
    solver.set_retractor("intrinsics", RT.IntrinsicsRetractor(cam))
    solver.set_damping("intrinsics", damping=1e-6, ep=1e-6)
    if not optimize_intrinsics:
        solver.set_fixed("intrinsics")
    solver.set_retractor("rig", RT.RigRotationOnlyRetractor())
    solver.set_damping("rig", damping=1e-4, ep=1e-4)
    if not optimize_rig_rotation:
        solver.set_fixed("rig")
    else:
        solver.set_fixed("rig", torch.zeros(1).long())
    energies = []
    for _ in range(n_iters):
        energies.append(solver.run_inplace({"pose": R.SE3(poses), "dense_disp": dis, "intrinsics": intr, "rig": R.SE3(rig)}))
    dis.clamp_(min=0.001)
    return _np(poses), _np(dis.view(N, V, ht, wd)), _np(intr), _np(rig), np.asarray(energies, dtype=np.float64)


BA_RIG_CASES = {
    # name: (make_rig_graph kwargs, BA kwargs) - V = 2 unless stated
    "v2_fixed_rig": (dict(n=4, V=2, radius=2, seed=3),
                     dict(t0=1, t1=4, n_iters=3, pose_damping=1e-3, pose_ep=0.1)),
    "v2_rig_rotation": (dict(n=4, V=2, radius=2, seed=5),
                        dict(t0=1, t1=4, n_iters=3, pose_damping=1e-5, pose_ep=1e-2, optimize_rig_rotation=True)),
    "v2_intrinsics": (dict(n=4, V=2, radius=2, seed=7),
                      dict(t0=1, t1=4, n_iters=2, pose_damping=1e-5, pose_ep=1e-2, optimize_intrinsics=True)),
    "v2_rig_and_intrinsics_prior": (dict(n=5, V=2, radius=2, seed=9, depth_prior=True),
                                    dict(t0=1, t1=5, n_iters=2, pose_damping=1e-5, pose_ep=1e-2, optimize_intrinsics=True,
                                         optimize_rig_rotation=True)),
    "v3_rig_rotation_window": (dict(n=5, V=3, radius=1, seed=11),
                               dict(t0=2, t1=5, n_iters=2, pose_damping=1e-3, pose_ep=0.1, optimize_rig_rotation=True)),
    "v2_no_self_edges_motion_only": (dict(n=4, V=2, radius=2, seed=13, self_edges=False),
                                     dict(t0=1, t1=4, n_iters=2, pose_damping=1e-3, pose_ep=0.1, motion_only=True)),
    # round 3: rigs of more than four cameras (the reference's Solver is generic in V, buffer.py:404-506)
    "v5_rig_and_intrinsics": (dict(n=3, V=5, radius=1, seed=15),
                              dict(t0=1, t1=3, n_iters=2, pose_damping=1e-5, pose_ep=1e-2, optimize_intrinsics=True,
                                   optimize_rig_rotation=True)),
    "v6_rig_rotation_prior": (dict(n=3, V=6, radius=2, seed=17, depth_prior=True),
                              dict(t0=1, t1=3, n_iters=2, pose_damping=1e-4, pose_ep=1e-2, optimize_rig_rotation=True)),
}


def gen_ba_rig(R):
    """Multi-view rigs through the reference Solver: fixed rig, rig-rotation group, per-view intrinsics, both + depth
    prior, three views with a pose window, and a motion-only case without cross-view terms."""
    from vipe_amd.synth import make_rig_graph
    out = {}
    for name, (gk, bk) in BA_RIG_CASES.items():
        g = make_rig_graph(**gk)
        p, d, k, r, en = reference_ba_rig(R, g, **bk)
        out[name + "/poses"], out[name + "/disps"], out[name + "/intrinsics"], out[name + "/rig"] = p, d, k, r
        out[name + "/energy"] = en
        print(name, "energy", en)
    # the reference's fp32 solve is not bit-reproducible from run to run (1e-6 relative: thread order of its reductions): cases
    # already frozen keep their first values, new cases are appended
    path = os.path.join(HERE, "ba_rig_reference.npz")
    if os.path.exists(path):
        old = np.load(path)
        out.update({k: old[k] for k in old.files})
    np.savez_compressed(path, **out)


def gen_ba_edges(R):
    """The cases of oracle/ba_cases.py (validity, zero support, step rejection, ragged and large plans) through the
    reference Solver: mono through `reference_ba`, the 8-view rig through `reference_ba_rig`.  OUTPUTS only - the inputs
    are re-created from the seeds by the tests."""
    from oracle import ba_cases as bc
    out = {}
    for name in bc.ALL:
        c = bc.case(name)
        g = c.g
        if c.rig:
            p, d, k, r, en = reference_ba_rig(R, g, **c.bk)
        else:
            p, d, k, en = reference_ba(R, g.poses, g.disps, g.disps_sens, c.intr, g.target, g.weight, g.eta, g.ii, g.jj,
                                       camera=c.cam, **c.bk)
            r = ose3.se3_identity(1).astype(np.float32)
        out[name + "/poses"], out[name + "/disps"], out[name + "/intrinsics"], out[name + "/rig"] = p, d, k, r
        print(name, "energy", en)
    np.savez_compressed(os.path.join(HERE, "ba_edges_reference.npz"), **out)


def gen_reproject(R):
    """geom.iproj_i_proj_j_disp values + Jacobians, pinhole and MEI (geom.py:187-298)."""
    out = {}
    for cam_name in ["pinhole", "mei"]:
        g = make_graph(n=4, height=64, width=96, radius=2, seed=31)
        cam = R.cameras.CameraType.PINHOLE if cam_name == "pinhole" else R.cameras.CameraType.MEI
        intr = torch.tensor(g.intrinsics).float()
        if cam_name == "mei":
            intr = torch.cat([intr, torch.tensor([[0.35]])], 1)
        intr8 = cam.build_camera_model(intr).scaled(1 / 8.0).intrinsics
        ii, jj = torch.tensor(g.ii), torch.tensor(g.jj)
        z = torch.zeros_like(ii)
        x1, valid, (Ji, Jj, Jz), (Jfi, Jfj), _ = R.geom.iproj_i_proj_j_disp(
            R.SE3(torch.tensor(g.poses)), torch.tensor(g.disps), None, intr8, cam,
            R.SE3(torch.tensor([[0, 0, 0, 0, 0, 0, 1.0]])), ii, jj, z, z, ii,
            jacobian_p_d=True, jacobian_f=True, jacobian_r=False)
        for k, v in dict(coords=x1, valid=valid, Ji=Ji, Jj=Jj, Jz=Jz, Jfi=Jfi, Jfj=Jfj).items():
            out[f"{cam_name}/{k}"] = _np(v)
        out[f"{cam_name}/intr"] = _np(intr)
    np.savez_compressed(os.path.join(HERE, "reproject_reference.npz"), **out)


def gen_update_module(R):
    """UpdateModule forward with seeded default-init weights (droid_net.py:432-499), fp32 CPU."""
    torch.manual_seed(0)
    um = R.droid_net.UpdateModule().eval()
    E, ht, wd = 5, 12, 16
    gen = torch.Generator().manual_seed(1)
    net = torch.randn(1, E, 128, ht, wd, generator=gen).tanh()
    inp = torch.randn(1, E, 128, ht, wd, generator=gen).relu()
    corr = torch.randn(1, E, 196, ht, wd, generator=gen)
    flow = torch.randn(1, E, 4, ht, wd, generator=gen) * 4
    ix = torch.tensor([0, 0, 1, 2, 2])
    with torch.no_grad():
        net2, delta, weight, eta, upmask = um(net, inp, corr, flow, ix)
    # weights and inputs are re-created from the seeds by the tests (same torch build); the fixture
    # keeps per-tensor checksums of them plus the outputs (hidden state subsampled 1:4 in channels)
    sd = {"sdsum/" + k: np.array([float(v.double().sum()), float(v.double().abs().sum())])
          for k, v in um.state_dict().items()}
    insum = np.array([float(t.double().sum()) for t in (net, inp, corr, flow)])
    np.savez_compressed(os.path.join(HERE, "update_module_reference.npz"), input_sums=insum, ix=_np(ix),
                        out_net_sub=_np(net2[:, :, ::4]), out_delta=_np(delta), out_weight=_np(weight),
                        out_eta=_np(eta), out_upmask_sub=_np(upmask[:, :, ::16]), **sd)


def gen_corr(R):
    """CorrBlock volume + pyramid (droid_net.py:56-69,94-102) and AltCorrBlock pyramid (:130-142), fp32 CPU."""
    gen = torch.Generator().manual_seed(2)
    fmap1 = torch.randn(1, 1, 128, 16, 16, generator=gen)
    fmap2 = torch.randn(1, 1, 128, 16, 16, generator=gen)
    cb = R.droid_net.CorrBlock(fmap1, fmap2)  # 4 levels need H2, W2 >= 16 (the loop pools once more after the last level)
    out = {"fmap1": _np(fmap1), "fmap2": _np(fmap2)}
    for i, lvl in enumerate(cb.corr_pyramid):
        out[f"level{i}"] = _np(lvl)
    fm = torch.randn(1, 2, 128, 16, 16, generator=gen)
    ab = R.droid_net.AltCorrBlock(fm)
    out["alt_fmaps"] = _np(fm)
    for i, lvl in enumerate(ab.pyramid):
        out[f"alt_level{i}"] = _np(lvl)
    np.savez_compressed(os.path.join(HERE, "corr_reference.npz"), **out)


def gen_lie_wrapper(R):
    """The reference's Python LieGroup wrapper over the (stubbed) backend: retr/adjT broadcasting semantics."""
    rng = np.random.default_rng(5)
    xi = torch.tensor(rng.normal(0, 0.3, (6, 6))).float()
    X = R.SE3.exp(xi)
    a = torch.tensor(rng.normal(0, 1, (6, 3, 2, 6))).float()
    out = {"xi": _np(xi), "X": _np(X.data), "a": _np(a),
           "adjT": _np(X[:, None, None].adjT(a)), "retr": _np(X.retr(xi * 0.1).data),
           "inv": _np(X.inv().data), "mul": _np((X * X.inv()).data), "log": _np(X.log()),
           "matrix": _np(X.matrix())}
    np.savez_compressed(os.path.join(HERE, "lie_wrapper_reference.npz"), **out)


def gen_edge_selection(R):
    """Golden vector #8 of SURVEY 8(c): the exact (ii, jj) lists `FactorGraph.add_proximity_factors`
    (factor_graph.py:411-488) hands to add_factors, from the reference file itself driven by a fake buffer whose
    frame distances come from a fixed matrix.  Pure integer / ordering logic -> pins "bit-exact edge indexing"."""
    for name in ["rerun"]:
        sys.modules.setdefault(name, types.ModuleType(name))
    comp = types.ModuleType("vipe.slam.components")
    comp.__path__ = []
    sys.modules["vipe.slam.components"] = comp
    sys.modules["vipe.slam"].components = comp
    bufmod = types.ModuleType("vipe.slam.components.buffer")
    bufmod.GraphBuffer = type("GraphBuffer", (), {})
    sys.modules["vipe.slam.components.buffer"] = bufmod
    comp.buffer = bufmod
    fg = _load("vipe.slam.components.factor_graph", "vipe/slam/components/factor_graph.py")
    out = {}
    cases = {
        # name: (n_frames, existing edge radius, n inactive, t0, t1, rad, nms, beta, thresh, max_factors, seed)
        "frontend": (12, 2, 3, 7, 2, 2, 2, 0.25, 16.0, 48, 1),
        "backend": (16, 0, 0, 0, 0, 2, 2, 0.25, 20.0, 16 * 16, 2),
        "backend_dense": (14, 1, 4, 0, 0, 3, 1, 0.25, 30.0, 60, 3),
    }
    for cname, (t, er, ninac, t0, t1, rad, nms, beta, thresh, maxf, seed) in cases.items():
        rng = np.random.default_rng(seed)
        D = rng.uniform(0.0, 40.0, size=(t, t)).astype(np.float32)
        ii0, jj0 = np.meshgrid(np.arange(t), np.arange(t), indexing="ij")
        keep = (np.abs(ii0 - jj0) > 0) & (np.abs(ii0 - jj0) <= er)
        ii_act, jj_act = ii0[keep].astype(np.int64), jj0[keep].astype(np.int64)
        inac = rng.integers(0, t, size=(ninac, 2)).astype(np.int64)

        class FakeBuffer:
            n_frames = t
            n_views = 1

            def frame_distance_dense_disp(self, ii, jj, beta):
                return torch.from_numpy(D)[ii, jj][:, None]

        g = object.__new__(fg.FactorGraph)
        g.buffer, g.device, g.cross_view, g.max_factors = FakeBuffer(), torch.device("cpu"), False, maxf
        g.ii, g.jj = torch.from_numpy(ii_act), torch.from_numpy(jj_act)
        g.ii_inac, g.jj_inac = torch.from_numpy(inac[:, 0].copy()), torch.from_numpy(inac[:, 1].copy())
        got = {}

        def record(ii, jj, remove=False, got=got):
            got["ii"], got["jj"], got["remove"] = ii.numpy().copy(), jj.numpy().copy(), remove

        g.add_factors = record
        g.add_proximity_factors(t0, t1, rad, nms, beta, thresh, True)
        out[cname + "_D"] = D
        out[cname + "_params"] = np.array([t, t0, t1, rad, nms, maxf], dtype=np.int64)
        out[cname + "_beta_thresh"] = np.array([beta, thresh], dtype=np.float64)
        out[cname + "_act"] = np.stack([ii_act, jj_act], 1)
        out[cname + "_inac"] = inac
        out[cname + "_es"] = np.stack([got["ii"], got["jj"]], 1).astype(np.int64)
    np.savez_compressed(os.path.join(HERE, "edge_selection_reference.npz"), **out)
    print("edge selection:", {k: v.shape for k, v in out.items() if k.endswith("_es")})


def gen_encoder(R):
    """BasicEncoder fnet (instance norm) / cnet (no norm) with seeded default-init weights (droid_net.py:290-370) and the
    DroidNet.encode_features / encode_context arithmetic around them (:510-527, restated inline because DroidNet()
    itself downloads weights), fp32 CPU.  Weights and images are re-created from the seeds by the tests; the fixture
    keeps their checksums and the outputs."""
    torch.manual_seed(0)
    fnet = R.droid_net.BasicEncoder(output_dim=128, norm_fn="instance").eval()
    cnet = R.droid_net.BasicEncoder(output_dim=256, norm_fn="none").eval()
    gen = torch.Generator().manual_seed(5)
    out = {}
    for tag, (V, H, W) in {"small": (2, 96, 128), "odd": (1, 72, 104)}.items():
        images = torch.rand(V, 3, H, W, generator=gen)
        mean = torch.as_tensor([0.485, 0.456, 0.406])
        std = torch.as_tensor([0.229, 0.224, 0.225])
        x = (images[None] - mean[:, None, None]) / std[:, None, None]
        with torch.no_grad():
            fmap = fnet(x).squeeze(0)
            net, inp = cnet(x).split([128, 128], dim=2)
            net, inp = net.tanh().squeeze(0), inp.relu().squeeze(0)
        out[tag + "/shape"] = np.array([V, H, W])
        out[tag + "/image_sum"] = np.array([float(images.double().sum())])
        out[tag + "/fmap"], out[tag + "/net"], out[tag + "/inp"] = _np(fmap), _np(net), _np(inp)
    for name, m in (("fnet", fnet), ("cnet", cnet)):
        for k, v in m.state_dict().items():
            out[f"sdsum/{name}.{k}"] = np.array([float(v.double().sum()), float(v.double().abs().sum())])
    np.savez_compressed(os.path.join(HERE, "encoder_reference.npz"), **out)
    print("encoder:", {k: v.shape for k, v in out.items() if not k.startswith("sdsum")})


def gen_splat(R):
    """`bilinear_splatting_inplace` (vipe/utils/depth.py:123-155), the reference function itself: points inside, on the
    borders, outside, on cell centres and exactly half-way between cells."""
    depth = _load("vipe.utils.depth", "vipe/utils/depth.py")
    rng = np.random.default_rng(5)
    H, W = 12, 16
    uv = np.concatenate([rng.uniform(-1.5, [W + 0.5, H + 0.5], (300, 2)),
                         np.array([[3.0, 4.0], [3.5, 4.5], [0.0, 0.0], [-0.5, -0.5], [W - 1.0, H - 1.0], [W - 1.5, H - 1.5],
                                   [W - 2.0, H - 2.0], [7.49999, 2.50001]])]).astype(np.float32)
    data = rng.normal(0, 2, (uv.shape[0], 2)).astype(np.float32)
    out, wgt = torch.zeros(H, W, 2), torch.zeros(H, W)
    depth.bilinear_splatting_inplace(torch.tensor(data), torch.tensor(uv), out, wgt)
    np.savez_compressed(os.path.join(HERE, "splat_reference.npz"), uv=uv, data=data, out=_np(out), weight=_np(wgt))
    print("splat: weight sum", float(wgt.sum()))


CORR_SAMPLER_CASES = {
    # name: (B, C, H, W), (kH, kW, patchH, patchW, padH, padW, dilH, dilW, dil_patchH, dil_patchW, dH, dW)
    "k1_patch5": ((2, 5, 9, 11), (1, 1, 5, 5, 0, 0, 1, 1, 2, 1, 1, 1)),
    "k3_pad_stride": ((2, 4, 10, 12), (3, 3, 3, 5, 1, 1, 1, 1, 1, 2, 2, 1)),
    "k2_dilated": ((1, 3, 8, 9), (2, 3, 7, 1, 2, 1, 2, 1, 1, 1, 1, 2)),
    "even_patch": ((1, 6, 7, 7), (1, 1, 4, 2, 0, 0, 1, 1, 1, 3, 1, 1)),
}


def gen_corr_sampler(R):
    """`corr_ext` against the reference's OWN CPU implementation, compiled here from
    /root/reference/csrc/corr_ext/correlation.cpp by oracle/build_ref.py (oracle/_ref/ref_corr.so): forward and backward
    on four geometries (kernel, patch, padding, both dilations, strides, an even patch size), float32."""
    from oracle.build_ref import build_ref_corr
    ref = build_ref_corr(REF)
    out = {}
    gen = torch.Generator().manual_seed(17)
    for name, (shape, geom) in CORR_SAMPLER_CASES.items():
        a = torch.randn(*shape, generator=gen)
        b = torch.randn(*shape, generator=gen)
        y = ref.forward(a, b, *geom)
        go = torch.randn(y.shape, generator=gen)
        g1, g2 = ref.backward(a, b, go, *geom)
        for k, v in dict(a=a, b=b, out=y, grad_out=go, grad1=g1, grad2=g2).items():
            out[f"{name}/{k}"] = _np(v)
        print("corr sampler", name, tuple(y.shape))
    np.savez_compressed(os.path.join(HERE, "corr_sampler_reference.npz"), **out)


def gen_schedules(R):
    """The control flow AROUND the update iteration, from the reference's own files driven by recording fakes
    (tests/golden/fakes.py): `SLAMFrontend` (frontend.py:32-167: initialisation, per-keyframe update with the keyframe
    test, pose extrapolation, next-frame disparity), `SLAMBackend` (backend.py:31-122: graph construction, the depth-prior
    branch, the empty-graph branch) and `InnerFiller.compute` (inner_filler.py:64-131: neighbour keyframes, interpolated
    poses, the edges it adds, ten motion-only iterations).  Frozen: the exact call traces and the poses / disparities they
    leave.  `omegaconf`, `vipe.priors.depth` and `rerun` are imported by those files for type annotations / logging only
    and are absent here: empty stand-in modules."""
    import json
    sys.path.insert(0, HERE)
    import fakes
    for name, attrs in (("omegaconf", {"DictConfig": dict}), ("rerun", {}), ("vipe.priors", {}),
                        ("vipe.priors.depth", {"DepthEstimationModel": object})):
        m = sys.modules.get(name) or types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
    comp = sys.modules.get("vipe.slam.components") or types.ModuleType("vipe.slam.components")
    comp.__path__ = []
    sys.modules["vipe.slam.components"] = comp
    sys.modules["vipe.slam"].components = comp
    for sub, attrs in (("buffer", {"GraphBuffer": object}), ("factor_graph", {"FactorGraph": fakes.FakeGraph})):
        m = types.ModuleType("vipe.slam.components." + sub)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules["vipe.slam.components." + sub] = m
        setattr(comp, sub, m)
    fe = _load("vipe.slam.components.frontend", "vipe/slam/components/frontend.py")
    be = _load("vipe.slam.components.backend", "vipe/slam/components/backend.py")
    inf = _load("vipe.slam.components.inner_filler", "vipe/slam/components/inner_filler.py")
    out = {}
    NS = types.SimpleNamespace
    # ---- frontend
    for tag, has_pose, seq_init in (("frontend", False, True), ("frontend_init_pose_no_seq", True, False)):
        args = NS(warmup=8, beta=0.3, frontend_nms=1, keyframe_thresh=4.0, frontend_window=25, frontend_thresh=16.0,
                  frontend_radius=2, has_init_pose=has_pose, cross_view=True, seq_init=seq_init)
        trace, poses, disps, t1, n = fakes.run_frontend(fe.SLAMFrontend, args, has_pose)
        out[tag + "/trace"] = np.array(json.dumps(trace))
        out[tag + "/poses"], out[tag + "/disps"] = _np(poses), _np(disps)
        out[tag + "/t1_n"] = np.array([t1, n])
        print(tag, len(trace), "calls; t1, n_frames =", t1, n)
    # ---- backend: plain, with a depth model + intrinsics, a single keyframe (empty graph)
    for tag, n_frames, depth, opt_intr, adaptive, edges in (("backend", 12, False, False, False, 3), ("backend_depth_intr", 12, True, True, True, 3),
                                                            ("backend_single", 1, False, False, False, 0)):
        video = fakes.FakeBuffer(n_frames)
        video.disps_sens[0, 0, 0] = 0.7
        fakes.FakeGraph.edges_per_add = edges
        args = NS(beta=0.3, backend_thresh=22.0, backend_radius=2, backend_nms=3, optimize_intrinsics=opt_intr,
                  optimize_rig_rotation=False, cross_view=True, adaptive_cross_view=adaptive, map_filter_thresh=0.05)
        b = be.SLAMBackend(None, video, args, torch.device("cpu"))
        b.depth_model = object() if depth else None
        b.run(7)
        b.run_if_necessary(5)
        fakes.FakeGraph.edges_per_add = 3
        out[tag + "/trace"] = np.array(json.dumps(video.trace))
        out[tag + "/disps0"] = _np(video.disps[0])
        print(tag, len(video.trace), "calls")
    # ---- inner filler: keyframes at frames 0, 3, 6, 9; the 12 frames 0..11 appended behind them in two chunks of 6
    for tag, dense in (("infill", False), ("infill_dense_disp", True)):
        video = fakes.FakeBuffer(4, seed=3)
        video.tstamp[:4] = torch.tensor([0, 3, 6, 9])
        video.disps_sens[4:10, 0, 0] = 0.9
        args = NS(infill_chunk_size=6, infill_dense_disp=dense)
        f = inf.InnerFiller(None, video, args, torch.device("cpu"))
        f.set_start_idx(4)
        for frame in range(12):
            video.tstamp[video.n_frames] = frame
            video.n_frames += 1
            if f.check() or frame == 11:
                f.compute()
        res = f.get_result()
        out[tag + "/trace"] = np.array(json.dumps(video.trace))
        out[tag + "/filled_poses"] = _np(res.poses.data)
        if dense:
            out[tag + "/filled_disps"] = _np(res.dense_disps)
        print(tag, len(video.trace), "calls;", tuple(res.poses.data.shape))
    np.savez_compressed(os.path.join(HERE, "schedule_reference.npz"), **out)


def gen_headline(R):
    """Headline-size fixtures from the reference itself (BASELINE configs[2]: 512 x 384, 48 keyframes, E = 276, depth
    prior on - the graph `bench.py` times):
      (a) the reference `Solver` on `make_graph(n=48, 384 x 512, radius 3, seed 1234, depth_prior=True)` with the
          frontend's BA parameters, 3 Gauss-Newton iterations -> poses [48,7], disps [48,48,64] (inputs are re-created from
          the seed by the tests);
      (b) the reference `UpdateModule` (seed-0 default-init weights) on [1,4,.,48,64] inputs with `ix` - SURVEY 8(c)
          golden #1 at the full grid; hidden state kept 1:8 in channels."""
    g = make_graph(n=48, height=384, width=512, radius=3, seed=1234, depth_prior=True)
    p, d, k, en = reference_ba(R, g.poses, g.disps, g.disps_sens, g.intrinsics, g.target, g.weight, g.eta, g.ii, g.jj,
                               t0=1, t1=48, n_iters=3, pose_damping=1e-3, pose_ep=0.1, motion_only=False,
                               limited_disp=False, optimize_intrinsics=False)
    print("headline BA: E =", len(g.ii), "energy", en)
    np.savez_compressed(os.path.join(HERE, "ba_headline_reference.npz"), poses=p, disps=d, intrinsics=k, energy=en,
                        n_edges=np.array([len(g.ii)]))
    torch.manual_seed(0)
    um = R.droid_net.UpdateModule().eval()
    E, ht, wd = 4, 48, 64
    gen = torch.Generator().manual_seed(21)
    net = torch.randn(1, E, 128, ht, wd, generator=gen).tanh()
    inp = torch.randn(1, E, 128, ht, wd, generator=gen).relu()
    corr = torch.randn(1, E, 196, ht, wd, generator=gen)
    flow = torch.randn(1, E, 4, ht, wd, generator=gen) * 4
    ix = torch.tensor([0, 0, 1, 2])
    with torch.no_grad():
        net2, delta, weight, eta, upmask = um(net, inp, corr, flow, ix)
    insum = np.array([float(t.double().sum()) for t in (net, inp, corr, flow)])
    sd = {"sdsum/" + kk: np.array([float(v.double().sum()), float(v.double().abs().sum())]) for kk, v in um.state_dict().items()}
    np.savez_compressed(os.path.join(HERE, "update_module_headline_reference.npz"), input_sums=insum, ix=_np(ix),
                        out_net_sub=_np(net2[:, :, ::8]).astype(np.float16), out_delta=_np(delta), out_weight=_np(weight),
                        out_eta=_np(eta), **sd)
    print("headline UpdateModule:", tuple(net2.shape), "delta range", float(delta.min()), float(delta.max()))


if __name__ == "__main__":
    torch.set_num_threads(8)
    R = load_reference()
    if os.environ.get("GOLDEN_ONLY") == "schedules":
        gen_schedules(R)
        sys.exit(0)
    if os.environ.get("GOLDEN_ONLY") == "corr_sampler":
        gen_corr_sampler(R)
        sys.exit(0)
    if os.environ.get("GOLDEN_ONLY") == "headline":
        gen_headline(R)
        sys.exit(0)
    if os.environ.get("GOLDEN_ONLY") == "edges":
        gen_edge_selection(R)
        sys.exit(0)
    if os.environ.get("GOLDEN_ONLY") == "ba_rig":
        gen_ba_rig(R)
        sys.exit(0)
    if os.environ.get("GOLDEN_ONLY") == "splat":
        gen_splat(R)
        sys.exit(0)
    if os.environ.get("GOLDEN_ONLY") == "ba_tracks":
        gen_ba_tracks(R)
        sys.exit(0)
    if os.environ.get("GOLDEN_ONLY") == "ba_edges":
        gen_ba_edges(R)
        sys.exit(0)
    if os.environ.get("GOLDEN_ONLY") == "encoder":
        gen_encoder(R)
        sys.exit(0)
    gen_edge_selection(R)
    gen_lie_wrapper(R)
    gen_reproject(R)
    gen_ba(R)
    gen_ba_rig(R)
    gen_ba_tracks(R)
    gen_ba_edges(R)
    gen_splat(R)
    gen_update_module(R)
    gen_corr(R)
    gen_encoder(R)
    gen_headline(R)
    gen_corr_sampler(R)
    gen_schedules(R)
    print("golden fixtures written to", HERE)
