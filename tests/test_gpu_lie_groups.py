"""`lie.hip` on the device against the float64 references of oracle/lie_groups.py: all four groups, float32 and float64.

Inputs: oracle/pose_cases.py - 1000 rows per group with angles from 1e-9 to pi - 1e-3, dense on both sides of the Taylor
threshold, throughout the float32 cancellation zone of (1 - cos t) / t^2, every branch of `log` and of calcW, quaternions
that are not normalised; and one set of 2048 x 256 + 257 rows for the second trip of the grid-stride loops.  Bounds:
oracle/lie_groups.bound, derived there, per row.  tests/test_oracle_pose.py holds the host path to half of them.
Output buffers have a guard row on each side, prefilled with NaN, and are compared whole."""

import numpy as np
import pytest
import torch

from oracle import lie_groups as lg
from oracle import pose_cases as pc

pytestmark = pytest.mark.gpu

GROUPS = list(lg.GROUPS)
DTYPES = [np.float32, np.float64]
DT_IDS = ["float32", "float64"]


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def _guarded_call(fn, gid, ins, n, width, dtype, extra=()):
    """fn(gid, *ins, out, *extra-or-n ...) into a NaN-filled [n + 2, width] buffer -> the body as numpy; guards must hold"""
    from vipe_amd._lib import DTYPE_CODE, ptr, stream_ptr
    buf = torch.full((n + 2, width), float("nan"), dtype=dtype, device=dev())
    body = buf[1:-1]
    if extra:
        rc = fn(gid, *[ptr(t) for t in ins], ptr(body), *extra, DTYPE_CODE[dtype], stream_ptr(buf))
    else:
        rc = fn(gid, *[ptr(t) for t in ins], ptr(body), n, DTYPE_CODE[dtype], 1, stream_ptr(buf))
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()), "guard rows written"
    return body.cpu().numpy()


def _fractions(got, ref, bd):
    err = np.abs(got.astype(np.float64) - ref)
    bd = np.broadcast_to(bd if bd.ndim == 2 else bd[:, None], err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / bd)


def _ops(group, dt):
    """op -> (entry point, device inputs, output width, float64 reference, bound inputs)"""
    from vipe_amd._lib import lib
    L = lib()
    o = pc.operands(group)
    a, X, Y, av, p3, p4 = (z.astype(dt) for z in (pc.tangents(group), pc.elements(group), o.Y, o.a, o.p3, o.p4))
    d = lambda z: z.astype(np.float64)
    K, N = lg.K[group], lg.N[group]
    return {
        "exp": (L.vipe_lie_expm, [a], N, lambda: lg.exp(group, d(a)), (d(a), None)),
        "log": (L.vipe_lie_logm, [X], K, lambda: lg.log(group, d(X)), (d(X), None)),
        "inv": (L.vipe_lie_inv, [X], N, lambda: lg.inv(group, d(X)), (d(X), None)),
        "mul": (L.vipe_lie_mul, [X, Y], N, lambda: lg.mul(group, d(X), d(Y)), (d(X), d(Y))),
        "adj": (L.vipe_lie_adj, [X, av], K, lambda: lg.adj(group, d(X), d(av)), (d(X), d(av))),
        "adjT": (L.vipe_lie_adjT, [X, av], K, lambda: lg.adjT(group, d(X), d(av)), (d(X), d(av))),
        "act": (L.vipe_lie_act, [X, p3], 3, lambda: lg.act(group, d(X), d(p3)), (d(X), d(p3))),
        "act4": (L.vipe_lie_act4, [X, p4], 4, lambda: lg.act4(group, d(X), d(p4)), (d(X), d(p4))),
        "matrix": (L.vipe_lie_as_matrix, [X], 16, lambda: lg.matrix(group, d(X)).reshape(len(X), -1), (d(X), None)),
        "vec": (L.vipe_lie_projector, [X], N * N, lambda: lg.projector(group, d(X)).reshape(len(X), -1), (d(X), None)),
        "Jinv": (L.vipe_lie_jinv, [X, av], K, lambda: lg.jinv(group, d(X), d(av)), (d(X), d(av))),
    }


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("group", GROUPS)
def test_forward_ops_on_the_device_against_the_float64_reference(group, dt):
    """exp, log, inv, mul, adj, adjT, act, act4, matrix, the projector (`vec`) and Jinv, 1000 rows each: every element within the
    row's bound; prints the worst fraction per op, and for exp per angle decade (DESIGN.md records them)."""
    tdt = torch.float32 if dt == np.float32 else torch.float64
    worst = {}
    for op, (fn, ins, width, ref, args) in _ops(group, dt).items():
        got = _guarded_call(fn, lg.GROUPS[group], [T(x) for x in ins], len(ins[0]), width, tdt)
        assert np.isfinite(got).all(), op
        fr = _fractions(got, ref(), lg.bound(group, op, dt, *args))
        worst[op] = float(fr.max())
        if op == "exp" and lg.HAS_T[group]:
            theta = np.linalg.norm(lg.split_tangent(group, args[0])[1], axis=-1)
            for lo in (1e-6, 1e-5, 1e-4, 1e-3, 1e-2):
                m = (theta >= lo) & (theta < 10 * lo)
                print(group, DT_IDS[DTYPES.index(dt)], "exp, device, angle decade %.0e: worst error / bound %.3f" % (lo, fr[m].max()))
    print(group, DT_IDS[DTYPES.index(dt)], "device worst error / bound", {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("group", GROUPS)
def test_broadcast_entries_equal_the_expanded_call(group, dt):
    """`vipe_lie_adjT_bcast` / `vipe_lie_act4_bcast` with 37 elements x 23 rows each (every group: the wrapper routes
    adjT and homogeneous act of all four to them): equal to the call on the replicated elements, bit for bit, and within
    the bound of the float64 reference"""
    from vipe_amd._lib import lib
    L, gid = lib(), lg.GROUPS[group]
    tdt = torch.float32 if dt == np.float32 else torch.float64
    E, R = 37, 23
    rng = np.random.default_rng(500 + gid)
    X = pc.elements(group)[64:64 + E].astype(dt)  # includes rows that are not normalised
    Xe = np.repeat(X, R, axis=0)
    for name, bfn, fn, y, ref in (("adjT", L.vipe_lie_adjT_bcast, L.vipe_lie_adjT, rng.standard_normal((E * R, lg.K[group])).astype(dt), lg.adjT),
                                  ("act4", L.vipe_lie_act4_bcast, L.vipe_lie_act4, rng.standard_normal((E * R, 4)).astype(dt), lg.act4)):
        got = _guarded_call(bfn, gid, [T(X), T(y)], E * R, y.shape[1], tdt, extra=(E, R))
        full = _guarded_call(fn, gid, [T(Xe), T(y)], E * R, y.shape[1], tdt)
        assert np.array_equal(got, full), name
        fr = _fractions(got, ref(group, Xe.astype(np.float64), y.astype(np.float64)),
                        lg.bound(group, name, dt, Xe.astype(np.float64), y.astype(np.float64)))
        assert fr.max() <= 1.0, (name, fr.max())
    # and through the wrapper's broadcasting
    from vipe_amd.ext import lietorch as lt
    G = getattr(lt, group)
    p = T(rng.standard_normal((E, R, 4)).astype(dt))
    fast = G(T(X))[:, None].act(p)
    slow = G(T(Xe)).act(p.view(E * R, 4)).view(E, R, 4)
    assert torch.equal(fast, slow)


def test_second_grid_stride_trip_forward_and_backward():
    """524 545 SE3 rows (the launch is capped at 2048 x 256 lanes) through a unary op (inv), a binary op (act) and the
    backward pass of act through autograd: rows 524 288 + i are bit-equal to rows i, a 4096-row sample of the forward
    results is within the bound of the float64 reference, and the backward results of the first 4096 rows equal the same
    pass run on those rows alone."""
    from vipe_amd._lib import lib
    from vipe_amd.ext.lietorch import SE3
    L = lib()
    b = pc.big_set()
    n, H, Tl = pc.BIG_ROWS, pc.BIG_HEAD, pc.BIG_TAIL
    X, p = T(b.X), T(b.p)
    inv = _guarded_call(L.vipe_lie_inv, 3, [X], n, 7, torch.float32)
    act = _guarded_call(L.vipe_lie_act, 3, [X, p], n, 3, torch.float32)
    s = b.sample
    X64, p64 = b.X[s].astype(np.float64), b.p[s].astype(np.float64)
    for name, got, ref, bd in (("inv", inv, lg.inv("SE3", X64), lg.bound("SE3", "inv", np.float32, X64)),
                               ("act", act, lg.act("SE3", X64, p64), lg.bound("SE3", "act", np.float32, X64, p64))):
        assert np.isfinite(got).all(), name
        assert np.array_equal(got[H:].view(np.uint32), got[:Tl].view(np.uint32)), name
        assert _fractions(got[s], ref, bd).max() <= 1.0, name
    Xg, pg = X.clone().requires_grad_(True), p.clone().requires_grad_(True)
    SE3(Xg).act(pg).backward(T(b.grad))
    dX, dp = Xg.grad.cpu().numpy(), pg.grad.cpu().numpy()
    Xs, ps = X[:4096].clone().requires_grad_(True), p[:4096].clone().requires_grad_(True)
    SE3(Xs).act(ps).backward(T(b.grad[:4096]))
    for name, big, small in (("dX", dX, Xs.grad.cpu().numpy()), ("dp", dp, ps.grad.cpu().numpy())):
        assert np.isfinite(big).all() and np.abs(big[H:]).max() > 0, name
        assert np.array_equal(big[H:].view(np.uint32), big[:Tl].view(np.uint32)), name
        assert np.array_equal(big[:4096].view(np.uint32), small.view(np.uint32)), name


def test_argument_checks():
    """n = 0 is VIPE_OK with null pointers; group id 5 and an unknown dtype code are VIPE_EINVAL and write nothing"""
    from vipe_amd._lib import F32, lib, ptr, stream_ptr
    L = lib()
    X = T(pc.elements("SE3").astype(np.float32))
    out = torch.full((1000, 7), float("nan"), device=dev())
    st = stream_ptr(X)
    assert L.vipe_lie_inv(3, None, None, 0, F32, 1, st) == 0
    assert L.vipe_lie_mul(3, None, None, None, 0, F32, 1, st) == 0
    assert L.vipe_lie_inv(5, ptr(X), ptr(out), 1000, F32, 1, st) == -1
    assert L.vipe_lie_inv(3, ptr(X), ptr(out), 1000, 7, 1, st) == -1
    assert L.vipe_lie_act4_bcast(5, ptr(X), ptr(X), ptr(out), 10, 10, F32, st) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("n_mean", [1, 4])
def test_frontend_next_frame_against_the_float64_oracle(n_mean):
    """`vipe_frontend_next_frame` at P = 2993, V = 2, t1 = 6: poses[6] against Exp(1/2 Log(G_5 G_4^-1)) G_5 from the
    oracle's own operators.  Pose tolerance 5 x 32 u x (1 + |t|): five float32 group ops (inv, mul, log, exp, mul; the
    halving is exact), each within 2 BASE u of an output of size 1 + |t| (oracle/lie_groups.bound for inv / mul / act; log
    and exp need no cancellation or branch term here: the rotation of G_5 G_4^-1 is 0.2 .. 1 rad, far from the c1 zone
    and from pi, and the half-angle step maps errors through Jl^-1 / Jl, whose norms are below 1.2 at these angles).
    The means against the float64 mean within (ceil(P n_mean / 256) + 6 + 4 + 2) u x mean: a lane's serial sum, six
    shuffle steps, four adds - all of non-negative terms - and two roundings for the count's conversion and the division; every frame below t1 and frame 7 keep their bits; with init_pose = 0 so do the poses."""
    from vipe_amd._lib import lib, ptr, stream_ptr
    c = pc.next_frame_case()
    u = 2.0 ** -24
    for init_pose in (1, 0):
        poses, disps = T(c.poses), T(c.disps)
        rc = lib().vipe_frontend_next_frame(ptr(poses), ptr(disps), c.t1, c.V, c.P, n_mean, init_pose, stream_ptr(poses))
        torch.cuda.synchronize()
        assert rc == 0
        gp, gd = poses.cpu().numpy(), disps.cpu().numpy()
        keep = [i for i in range(8) if i != c.t1]
        assert np.array_equal(gp[keep].view(np.uint32), c.poses[keep].view(np.uint32))
        assert np.array_equal(gd[keep].view(np.uint32), c.disps[keep].view(np.uint32))
        if init_pose:
            tol = 5 * 32 * u * (1 + np.abs(c.pose_ref[:3]).max())
            err = np.abs(gp[c.t1].astype(np.float64) - c.pose_ref).max()
            print("next_frame pose err", err, "tol", tol)
            assert err <= tol
        else:
            assert np.array_equal(gp[c.t1].view(np.uint32), c.poses[c.t1].view(np.uint32))
        src = c.disps[c.t1 - n_mean:c.t1].astype(np.float64)
        want = src.mean(axis=(0, 2))
        bound = (np.ceil(c.P * n_mean / 256) + 6 + 4 + 2) * u * want
        for v in range(c.V):
            row = gd[c.t1, v]
            assert (row == row[0]).all()
            assert abs(float(row[0]) - want[v]) <= bound[v], (v, float(row[0]), want[v], bound[v])
