"""Dense-BA problems at the route and tile boundaries of the reduced-system solvers.

ORACLE (test infrastructure).  Pure numpy, seeded, cached, CPU-only; nothing is modified after it is built.  The device
solves the reduced system with the LDS band solver (narrow, wide, two-chain), the LDS dense solver, the single-workgroup
global-memory Cholesky (12-column blocks) or the 64 x 64 tiled one; `vipe_amd/csrc/ba_route.cuh` picks, `oracle/ba_route.py`
restates the pick.  Every case here is `make_graph` / `make_rig_graph` as it comes, names the route it is meant for and the
boundary it sits on, and is a namespace like the ones of `oracle/ba_cases.py` (`g`, `cam`, `intr`, `bk`, `rig`) plus
`route`, `tile` (the owning solver's tile: 64 tiled, 16 single workgroup and dense, 6 band) and `boundary`.

tests/test_oracle_solver_cases.py proves on the CPU that each case sits where it says and that the tolerance tells a
subtly wrong solver (`defects`) from a right one; tests/test_gpu_ba_solvers.py feeds the cases to the kernels.

Tolerance (`step_bounds`): per output min(8 x delta32, the suite's 1e-4 form), not below 8 float32 units in the last place
of the output's largest value; delta32 = |oracle(float32) - oracle(float64)| on the case.  Nothing of the kernels enters.
"""

import functools
from types import SimpleNamespace

import numpy as np

from vipe_amd.synth import make_graph, make_rig_graph

from . import ba, ba_route
from . import ba_cases as bc

F8 = np.float64
FACTOR, ULPS = 8, 8
TILE = {"tiled": 64, "one_workgroup": 16, "dense": 16, "narrow": 6, "wide": 6, "two_chain": 6}
# the one case whose 8 x delta32 on the poses is not below the suite's 1e-4 form (0.75 of it: there the old form binds)
OLD_FORM_BINDS = ("wg175",)


def _case(name, g, route, boundary, cam="pinhole", intr=None, rig=False, **bk):
    t1 = bk.pop("t1", g.n)
    if rig:
        kw = dict(t0=1, t1=t1, n_iters=2, pose_damping=1e-3, pose_ep=0.1)
        kw.update(bk)
    else:
        kw = bc._bk(bk.pop("t0", 1), t1, **bk)
    return SimpleNamespace(name=name, g=g, cam=cam, intr=g.intrinsics if intr is None else intr, bk=kw, rig=rig, route=route,
                           tile=TILE[route], boundary=boundary)


def _mei(g):
    return np.concatenate([g.intrinsics, np.array([[0.4]], np.float32)], 1)


_BUILD = {}


def _add(name, build):
    assert name not in _BUILD, name
    _BUILD[name] = build


# ------------------------------------------------------------------------------------------------ single workgroup (n <= 256)

_add("wg168", lambda: _case("wg168", make_graph(n=29, height=32, width=48, radius=28, seed=301), "one_workgroup",
                            "n = 168 = 14 x 12: the last 12-column block is full"))
_add("wg252", lambda: _case("wg252", make_graph(n=43, height=32, width=48, radius=42, seed=302), "one_workgroup",
                            "n = 252 = 21 x 12: the largest pose-only size of the kernel"))
_add("wg253", lambda: _case("wg253", make_graph(n=43, height=32, width=48, radius=42, seed=302), "one_workgroup",
                            "n = 253: a last block of one column, the largest size with the focal length",
                            optimize_intrinsics=True))
_add("wg234_band", lambda: _case("wg234_band", make_graph(n=40, height=96, width=128, radius=8, seed=305), "one_workgroup",
                                 "n = 234, band 16 of 39 blocks, no tail: panels of band rows only (the band solver declines "
                                 "by pair count and LDS, the dense solver by size)"))
_add("wg254_rig", lambda: _case("wg254_rig", make_rig_graph(n=42, V=2, height=96, width=128, radius=2, seed=402),
                                "one_workgroup", "n = 254 = 6 x 41 + 2 + 6, band 4: a narrow band + 8 dense tail rows, close to "
                                "the largest size of the kernel", rig=True, optimize_intrinsics=True, optimize_rig_rotation=True))
_add("wg256_rig4", lambda: _case("wg256_rig4", make_rig_graph(n=43, V=4, height=96, width=128, radius=1, seed=403),
                                 "one_workgroup", "n = 256 = 6 x 42 + 4 = CT_MIN_N, band 2 + 4 tail rows (four views' focal "
                                 "lengths): the largest system of the kernel, a last block of four columns", rig=True,
                                 optimize_intrinsics=True))
_add("wg240_in_big_ws",lambda: _case("wg240_in_big_ws", make_graph(n=50, height=96, width=128, radius=3, extra_edges=150,
                                                                    seed=306), "one_workgroup",
                                      "n = 240 in a workspace for more than 256 unknowns: the tiled launches run beside it and "
                                      "must all exit", t0=10))

# ------------------------------------------------------------------------------------------------ tiled (n > 256)

_add("ct258", lambda: _case("ct258", make_graph(n=44, height=32, width=48, radius=43, seed=303), "tiled",
                            "n = 258 = 4 x 64 + 2: the first size of the route"))
_add("ct319", lambda: _case("ct319", make_graph(n=54, height=32, width=48, radius=53, seed=304), "tiled",
                            "n = 319 = 5 x 64 - 1: the rhs is row 63 of the last tile", optimize_intrinsics=True))
_add("ct320_rig", lambda: _case("ct320_rig", make_rig_graph(n=54, V=2, height=32, width=48, radius=1, seed=401), "tiled",
                                "n = 320 = 5 x 64: tail rows close the last full tile, the rhs has a tile row of its own; banded",
                                rig=True, optimize_intrinsics=True))
_add("ct385", lambda: _case("ct385", make_graph(n=65, height=32, width=48, radius=64, seed=4600), "tiled",
                            "n = 385 = 6 x 64 + 1: the last tile column is one column + the rhs", optimize_intrinsics=True))
_add("ct360_in_big_ws", lambda: _case("ct360_in_big_ws", make_graph(n=70, height=96, width=128, radius=3, extra_edges=260,
                                                                    seed=101), "tiled",
                                      "n = 360 in a workspace sized for seven tile columns: six used", t0=10))


# ------------------------------------------------------------------------------------------------ band solver boundaries


def band_boundaries(radius, limit=400):
    """free-pose counts of the pose-only radius-`radius` chain (bandblk = 2 radius, n = 6 n_free) at which
    `ba_route.band_form` changes -> dict: two_min (smallest two_chain), two_max (largest), one_max (largest one-chain)"""
    b = 2 * radius
    form = {nf: ba_route.band_form(6 * nf, nf, b, 0, 0) for nf in range(b + 1, limit)}
    one = {nf: ba_route.band_form(6 * nf, nf, b, 0, 0, band2=False) for nf in range(b + 1, limit)}
    two = [nf for nf, f in form.items() if f == "two_chain"]
    return dict(two_min=min(two), two_max=max(two), one_max=max(nf for nf, f in one.items() if f != "declines"))


def _band_case(name, seed, radius, n_free, route, boundary):
    return lambda: _case(name, make_graph(n=n_free + 1, height=96, width=128, radius=radius, seed=seed), route, boundary)


BAND_PAIRS = []  # (case, its neighbour across the boundary)
for _r in (1, 3):
    _b, _p, _s = band_boundaries(_r), f"band_r{_r}_", 500 + 10 * _r
    _add(_p + "below_two", _band_case(_p + "below_two", _s, _r, _b["two_min"] - 1, "narrow",
                                      f"{_b['two_min'] - 1} free poses: one fewer than 4 bandblk + 4, one chain"))
    _add(_p + "two_min", _band_case(_p + "two_min", _s + 1, _r, _b["two_min"], "two_chain",
                                    f"{_b['two_min']} = 4 bandblk + 4 free poses: the smallest two-chain system"))
    _add(_p + "two_max", _band_case(_p + "two_max", _s + 2, _r, _b["two_max"], "two_chain",
                                    f"{_b['two_max']} free poses: the longest chain whose two images fit the LDS"))
    _add(_p + "above_two", _band_case(_p + "above_two", _s + 3, _r, _b["two_max"] + 1, "narrow",
                                      f"{_b['two_max'] + 1} free poses: the first chain that falls back to one image"))
    _add(_p + "one_max", _band_case(_p + "one_max", _s + 4, _r, _b["one_max"], "narrow",
                                    f"{_b['one_max']} free poses: the longest one-chain system (band_need <= LDS)"))
    BAND_PAIRS += [(_p + "below_two", _p + "two_min"), (_p + "two_max", _p + "above_two")]
_add("ct_band", _band_case("ct_band", 307, 3, band_boundaries(3)["one_max"] + 1, "tiled",
                           "the first radius-3 chain the one-chain form cannot hold: a banded matrix in the tiled solver"))
BAND_PAIRS.append(("band_r3_one_max", "ct_band"))

# ------------------------------------------------------------------------------------------------ the existing solver graphs
# (tests/test_gpu_parity.py, same arguments: there they are held to the 1e-4 form)

for _n, _rad, _cam, _f, _form in ((8, 2, "pinhole", False, "narrow"), (14, 2, "pinhole", True, "narrow"), (14, 2, "mei", True, "narrow"),
                                  (13, 12, "mei", True, "wide"), (9, 8, "pinhole", True, "wide")):
    def _b(n=_n, rad=_rad, cam=_cam, f=_f, form=_form, name=f"form_n{_n}_r{_rad}_{_cam}{'_f' if _f else ''}"):
        g = make_graph(n=n, height=96, width=128, radius=rad, seed=200 + n + rad)
        return _case(name, g, form, "test_band_solver_forms_against_fp64_oracle", cam=cam, intr=_mei(g) if cam == "mei" else None,
                     optimize_intrinsics=f)
    _add(f"form_n{_n}_r{_rad}_{_cam}{'_f' if _f else ''}", _b)

for _n, _f, _route in ((4, False, "narrow"),(9, True, "wide"), (17, False, "dense"), (17, True, "dense"), (24, False, "dense"),
                       (27, False, "dense"), (27, True, "dense"), (28, False, "one_workgroup")):
    def _b(n=_n, f=_f, route=_route, name=f"window{_n}{'_f' if _f else ''}"):
        return _case(name, make_graph(n=n, height=96, width=128, radius=n - 1, seed=17 + n), route,
                     "test_dense_window_solver_sizes", optimize_intrinsics=f)
    _add(f"window{_n}{'_f' if _f else ''}", _b)


def _window17_mei():
    g = make_graph(n=17, height=96, width=128, radius=16, seed=53)
    return _case("window17_mei", g, "dense", "test_dense_window_solver_with_two_intrinsics_columns", cam="mei", intr=_mei(g),
                 optimize_intrinsics=True)


_add("window17_mei", _window17_mei)
for _f in (False, True):
    _add("twelve" + ("_f" if _f else ""), lambda f=_f: _case(
        "twelve" + ("_f" if f else ""), make_graph(n=13, height=96, width=128, radius=12, seed=31), "wide",
        "test_dense_ba_dense_window_of_twelve_poses", pose_damping=1e-4, pose_ep=1e-2, optimize_intrinsics=f))
    _add("dense114" + ("_f" if _f else ""), lambda f=_f: _case(
        "dense114" + ("_f" if f else ""), make_graph(n=20, height=96, width=128, radius=19, seed=91), "dense",
        "test_dense_ba_dense_window_takes_lds_dense_solver", optimize_intrinsics=f))
    _add("ct414" + ("_f" if _f else ""), lambda f=_f: _case(
        "ct414" + ("_f" if f else ""), make_graph(n=70, height=96, width=128, radius=3, extra_edges=260, seed=101), "tiled",
        "test_dense_ba_large_dense_system_takes_tiled_cholesky", pose_damping=1e-5, pose_ep=1e-2, optimize_intrinsics=f))
_add("wg175", lambda: _case("wg175", make_graph(n=30, height=96, width=128, radius=2, extra_edges=60, seed=77), "one_workgroup",
                            "test_dense_ba_non_banded_graph_takes_global_memory_solver", pose_damping=1e-5, pose_ep=1e-2,
                            optimize_intrinsics=True))
for _n, _rad in ((48, 3), (33, 2), (34, 1), (40, 3)):
    _add(f"chain{_n}_r{_rad}", lambda n=_n, rad=_rad: _case(
        f"chain{n}_r{rad}", make_graph(n=n, height=96, width=128, radius=rad, seed=100 + n), "two_chain",
        "test_two_chain_band_solve_equals_one_chain"))

ALL = tuple(_BUILD)
BOUNDARY = tuple(n for n in ALL if n.startswith(("wg", "ct", "band_")) and n != "wg175")  # the new ones
# one case per route for the plan-reuse pass
REUSE = ("band_r3_two_min", "form_n14_r2_pinhole_f", "twelve_f", "dense114", "wg254_rig", "ct319")


@functools.lru_cache(maxsize=None)
def case(name):
    c = _BUILD[name]()
    assert c.name == name, (c.name, name)
    return c


# ------------------------------------------------------------------------------------------------ route


def facts(name):
    """(n_free, n, bandblk, ntail, max_degree) of the case's plan, `ba_route.plan_facts`"""
    c = case(name)
    return ba_route.plan_facts(c.g.ii, c.g.jj, c.bk["t0"], c.bk["t1"], c.g.V if c.rig else 1, c.bk.get("optimize_intrinsics", False),
                               c.intr.shape[1] - 4, c.bk.get("optimize_rig_rotation", False))


def route_args(name, band2=True):
    """the arguments of the `ba_route` functions for the case"""
    n_free, n, bandblk, ntail, _ = facts(name)
    return n, n_free, bandblk, ntail, int(case(name).rig), band2


def route(name, band2=True):
    return ba_route.route_name(*route_args(name, band2))


# ------------------------------------------------------------------------------------------------ oracle runs


class _Watch:
    """numpy.linalg.solve, and a record of what it was given: the first system's block band and every step"""

    def __init__(self, n_free):
        self.n_free, self.band, self.dx = n_free, None, []

    def __call__(self, S, g):
        if self.band is None:
            self.band = ba_route.block_band(S, self.n_free)
            self.symmetric = bool(np.abs(S - S.T).max() <= 1e-9 * np.abs(S).max())
        dx = np.linalg.solve(S, g)
        self.dx.append(dx)
        return dx


@functools.lru_cache(maxsize=None)
def _run(name, dtype):
    c = case(name)
    args, kw = bc.oracle_inputs(c)
    watch = _Watch(facts(name)[0]) if dtype == "float64" else None
    out = ba.bundle_adjustment(*args, dtype=np.dtype(dtype), solve=watch, **kw)
    return out, watch


def oracle_run(name, dtype="float64"):
    """(poses, disps [n,V,ht,wd], intrinsics, rig) of the oracle on the case, computed once"""
    return _run(name, dtype)[0]


def oracle_system(name):
    """the float64 run's record: .band (block band of the first reduced system's pose part), .dx (the steps), .symmetric"""
    return _run(name, "float64")[1]


def step_bounds(name):
    """dict output -> (delta32, bound): min(8 delta32, the 1e-4 form), at least 8 ulp of the output's largest value"""
    return bc.output_bounds(oracle_run(name, "float64"), oracle_run(name, "float32"), factor=FACTOR, ulps=ULPS)


def old_pose_bound(name):
    return 1e-4 * max(1.0, float(np.abs(oracle_run(name)[0]).max()))


def pose_step(name):
    """largest change of a pose component over the call, float64 oracle"""
    return float(np.abs(oracle_run(name)[0] - case(name).g.poses.astype(F8)).max())


# ------------------------------------------------------------------------------------------------ wrong solvers


def _chol_solve(S, g, tile, edit_factor=None, skip_rhs=None, skip_back=None):
    """x = S^-1 g through the lower Cholesky factor in float64, tile by tile as the device does it: the rhs rides along as
    row n of the factorisation (y = L^-1 g), then L^T x = y from the last tile column to the first.  The three hooks leave
    one piece of that out; None of them set, this is a plain solve.  -> (x, largest magnitude that was left out)"""
    n = len(g)
    S, g = np.asarray(S, F8), np.asarray(g, F8)
    cols = [(c, min(c + tile, n)) for c in range(0, n, tile)]
    A = np.concatenate([np.tril(S), g[None]])  # rows 0..n-1 lower triangle, row n = rhs
    left = 0.0
    for k, (c0, c1) in enumerate(cols):
        if edit_factor is not None:
            left = max(left, edit_factor(A, k, cols))
        Lkk = np.linalg.cholesky(A[c0:c1, c0:c1] + np.tril(A[c0:c1, c0:c1], -1).T)
        A[c0:c1, c0:c1] = Lkk
        A[c1:, c0:c1] = np.linalg.solve(Lkk, A[c1:, c0:c1].T).T
        P = A[c1:, c0:c1]
        upd = P @ P[:n - c1].T  # rows c1..n, columns c1..n-1
        if skip_rhs is not None and k == skip_rhs(cols):
            left = max(left, float(np.abs(upd[-1]).max()) if upd.size else 0.0)
            upd[-1] = 0
        A[c1:, c1:n] -= np.concatenate([np.tril(upd[:n - c1]), upd[n - c1:]])
    y = A[n].copy()
    x = np.zeros(n)
    for k in range(len(cols) - 1, -1, -1):
        c0, c1 = cols[k]
        x[c0:c1] = np.linalg.solve(A[c0:c1, c0:c1].T, y[c0:c1])
        tileblk = A[c0:c1, :c0].copy()
        if skip_back is not None and k == len(cols) - 1 and c0 > 0:
            lo, hi = cols[0]
            left = max(left, float(np.abs(tileblk[:, lo:hi]).max()))
            tileblk[:, lo:hi] = 0
        y[:c0] -= tileblk.T @ x[c0:c1]
    return x, left


class _Defect:
    """a wrong solver (S, g) -> dx; .left = the largest magnitude of what it left out or changed so far (0: the defect never
    touched a nonzero, so on this case it is no defect)"""
    with_diag = False

    def __init__(self, fn):
        self.fn, self.left = fn, 0.0

    def __call__(self, S, g, *diag):
        try:
            x, left = self.fn(S, g, *diag)
        except np.linalg.LinAlgError:  # the damaged matrix is no longer positive definite: a failed factorisation, zero step
            x, left = np.zeros(len(g)), np.inf
        self.left = max(self.left, left)
        return x


def defects(tile, n_free=None, bandblk=None, tail=None):
    """Solvers with one thing wrong each, built on the float64 Cholesky factor in tiles of `tile` -> dict name -> _Defect.
      update_entry  the entry (row n - 1, first column of the last tile column) misses the preceding panel's trailing update
      backsub_tile  the back substitution ignores the off-diagonal tile (last tile row, first tile column)
      rhs_panel     the rhs row misses the update of the panel before the last tile column
      band_short    the 6 x 6 blocks at distance `bandblk` from the diagonal are dropped (given n_free and bandblk < n_free - 1)
      tail_as_pose  the last unknown, a tail one, is damped with the poses' (lambda, ep); `tail` = (pose lambda, pose ep, the
                    tail unknown's lambda, ep)"""
    def update_entry(S, g):
        def edit(A, k, cols):
            if k != len(cols) - 1 or k == 0:
                return 0.0
            n, c0, (p0, p1) = len(g), cols[k][0], cols[k - 1]
            miss = float(A[n - 1, p0:p1] @ A[c0, p0:p1])  # what panel k - 1 subtracted from A[n - 1, c0]
            A[n - 1, c0] += miss
            return abs(miss)
        return _chol_solve(S, g, tile, edit_factor=edit)

    out = {"update_entry": _Defect(update_entry),
           "backsub_tile": _Defect(lambda S, g: _chol_solve(S, g, tile, skip_back=True)),
           "rhs_panel": _Defect(lambda S, g: _chol_solve(S, g, tile, skip_rhs=lambda cols: len(cols) - 2))}
    if n_free is not None and bandblk is not None and 0 < bandblk < n_free - 1:
        def band_short(S, g):
            S = np.array(S, F8)
            blk = np.arange(6 * n_free) // 6
            far = np.zeros(S.shape, bool)
            far[:6 * n_free, :6 * n_free] = np.abs(blk[:, None] - blk[None]) == bandblk
            left = float(np.abs(S[far]).max())
            S[far] = 0
            return np.linalg.solve(S, g), left
        out["band_short"] = _Defect(band_short)
    if tail is not None:
        lam_p, ep_p, lam_t, ep_t = tail

        def tail_as_pose(S, g, diag):
            S = np.array(S, F8)
            add = (ep_p - ep_t) + (lam_p - lam_t) * diag[-1]
            S[-1, -1] += add
            return np.linalg.solve(S, g), abs(float(add))
        out["tail_as_pose"] = _Defect(tail_as_pose)
        out["tail_as_pose"].with_diag = True
    return out


def case_defects(name):
    """`defects` for the case: its solver's tile, its band, and its last tail unknown (a rig rotation: 1e-4, 1e-4; an
    intrinsic: 1e-6, 1e-6 - oracle/ba.py) if it has a tail"""
    c = case(name)
    n_free, n, bandblk, ntail, _ = facts(name)
    tail = None
    if ntail:
        lt = 1e-4 if c.bk.get("optimize_rig_rotation") else 1e-6
        tail = (c.bk["pose_damping"], c.bk["pose_ep"], lt, lt)
    return defects(c.tile, n_free, bandblk, tail)


def run_with(name, solve):
    args, kw = bc.oracle_inputs(case(name))
    return ba.bundle_adjustment(*args, solve=solve, **kw)


def off_by(name, out, bounds=None):
    """largest distance of `out` from the float64 oracle over the outputs, in bounds of the GPU test"""
    bounds = step_bounds(name) if bounds is None else bounds
    return max(float(np.nan_to_num(np.abs(a - b), nan=np.inf).max()) / bound
               for (_, (_, bound)), a, b in zip(bounds.items(), out, oracle_run(name)))


def old_asserts_catch(name, out):
    """would the 1e-4 asserts of tests/test_gpu_parity.py (poses, disparities, intrinsics) have failed on `out`"""
    p, d, k, _ = oracle_run(name)
    return bool(np.abs(out[0] - p).max() > 1e-4 * max(1.0, np.abs(p).max()) or np.abs(out[1] - d).max() > 1e-4 * np.abs(d).max()
                or np.abs(out[2] - k).max() > 1e-4 * np.abs(k).max())
