"""Which solver takes the reduced system of a dense-BA plan: `vipe_amd/csrc/ba_route.cuh` restated on the CPU.

ORACLE (test infrastructure).  Pure integer Python, no numpy in the route itself.  The device decides from
(n, n_free, bandblk, ntail, mv, band2, lds_doubles): info[3], info[0], info[4] of the plan, BAArgs::ntail / mv / band2 and
the LDS the band and dense solvers are launched with.  Every function below carries the name of the one it restates;
`plan_facts` restates the part of the plan kernel (`ba_plan.inc`) that produces those integers from the edge list, with
the fixed-pose rule of `oracle/ba.py` (buffer.py:462-465).  A solver case (oracle/solver_cases.py) is shown to sit on its
boundary with these functions, without a GPU; the GPU test then asserts that the device reports the same.
"""

import numpy as np

from vipe_amd.synth import expand_edges

SOLVER_LDS_DOUBLES = 158 * 1024 // 8
BAND_T = 512
BAND_UPT = 6
DN_PP = 20
DN_SLOTS = 10
LDS_TAIL_MAX = 2
CT_MIN_N = 256
NB, CT = 12, 64  # block / tile width of the single-workgroup and the tiled global-memory Cholesky (ba_solve_global.inc)
SOLVER_GLOBAL, SOLVER_BAND, SOLVER_DENSE = 0, 1, 2  # enum Solver (ba_common.cuh): what info[5] reports


# ------------------------------------------------------------------------------------------------ band solver


def band_npair(PB, rows):
    F = rows - 1
    return PB * (PB + 1) // 2 + rows * PB + (0 if F == 0 else (2 if F == 1 else 5))


def band_pair_cap(UPT):
    return 21 + UPT * (BAND_T - 64)


def band_need(n, npr, rows, WBP):
    return npr * WBP + rows * (n + 1) + npr + 64


def band2_rows_max(nb, bandblk):
    return 6 * (nb - (nb - bandblk) // 2)


def band2_image(nprmax, WBP):
    return nprmax * WBP + (nprmax + 1) + nprmax + 48


def band_form(n, n_free, bandblk, ntail, mv, band2=True, lds_doubles=SOLVER_LDS_DOUBLES):
    """-> "declines", "narrow", "wide" or "two_chain" (enum BandForm)"""
    if mv or n == 0:
        return "declines"
    npr, rows, PB = 6 * n_free, ntail + 1, 6 * bandblk
    WBP = PB + 7
    wide = WBP > 64 or band_npair(PB, rows) > band_pair_cap(2)
    if (not wide and ntail == 0 and band2 and bandblk >= 1 and n_free >= 4 * bandblk + 4
            and 2 * band2_image(band2_rows_max(n_free, bandblk), WBP) + 8 <= lds_doubles):
        return "two_chain"
    if (band_need(n, npr, rows, WBP) > lds_doubles or band_npair(PB, rows) > band_pair_cap(BAND_UPT if wide else 2)
            or PB + rows > BAND_T or WBP > (128 if wide else 64) or ntail > LDS_TAIL_MAX):
        return "declines"
    return "wide" if wide else "narrow"


# ------------------------------------------------------------------------------------------------ dense solver


def dense_packed(n):
    return ((n + 1) * (n + 2) // 2 + 1) & ~1


def dense_tile_rows(n):
    return (n + 16) >> 4


def dense_tiles(n):
    return dense_tile_rows(n) * (dense_tile_rows(n) + 1) // 2


def dense_need(n):
    return dense_packed(n) + 64 + 2 * 36 + 36 + (n + 8) + 6 * (n + 6) + DN_PP * 16 * dense_tile_rows(n)


def dense_takes(n, n_free, bandblk, ntail, mv, band2=True, lds_doubles=SOLVER_LDS_DOUBLES):
    return (n != 0 and not mv and band_form(n, n_free, bandblk, ntail, mv, band2, lds_doubles) == "declines"
            and dense_need(n) <= lds_doubles and ntail <= LDS_TAIL_MAX and dense_tiles(n) <= 6 * DN_SLOTS)


# ------------------------------------------------------------------------------------------------ global-memory solvers


def global_form(n, n_free, bandblk, ntail, mv, band2=True, lds_doubles=SOLVER_LDS_DOUBLES):
    """-> "declines", "one_workgroup" (`ba_solve_kernel`) or "tiled" (`chol_*_kernel`)"""
    r = (n, n_free, bandblk, ntail, mv, band2, lds_doubles)
    if n == 0 or band_form(*r) != "declines" or dense_takes(*r):
        return "declines"
    return "one_workgroup" if n <= CT_MIN_N else "tiled"


def solver(n, n_free, bandblk, ntail, mv, band2=True, lds_doubles=SOLVER_LDS_DOUBLES):
    """the Solver id the kernel that solves writes to info[5]; None for a system without unknowns (nobody reports)"""
    r = (n, n_free, bandblk, ntail, mv, band2, lds_doubles)
    if n == 0:
        return None
    if band_form(*r) != "declines":
        return SOLVER_BAND
    return SOLVER_DENSE if dense_takes(*r) else SOLVER_GLOBAL


def route_name(n, n_free, bandblk, ntail, mv, band2=True, lds_doubles=SOLVER_LDS_DOUBLES):
    """one word for tables and case expectations: a band form, or dense / one_workgroup / tiled"""
    r = (n, n_free, bandblk, ntail, mv, band2, lds_doubles)
    if n == 0:
        return "none"
    form = band_form(*r)
    if form != "declines":
        return form
    return "dense" if dense_takes(*r) else global_form(*r)


# ------------------------------------------------------------------------------------------------ the plan's facts


def plan_facts(ii, jj, t0, t1, V=1, optimize_intrinsics=False, D=0, optimize_rig_rotation=False):
    """-> (n_free, n, bandblk, ntail, max_degree): info[0], info[3], info[4], BAArgs::ntail and info[6] of the live BA's plan
    for the keyframe edges ii -> jj (expanded to V terms each, `expand_edges`).

    A pose is fixed iff it is the SOURCE of a term and lies outside [t0, t1) (t0 >= t1 fixes all); free poses that occur
    in a term get slots in ascending id (ba_plan.inc:91-104).  Tail (live_args, ba.hip): mono 1 + D shared intrinsics,
    a rig V (1 + D) intrinsics and 6 (V - 1) rig rotations.  Band (ba_plan.inc:137-150): over the disparity frames with
    terms, hi - lo over the free slots among {pose of the frame} + {targets of its terms}; degree: terms per frame."""
    pi, qi, di, pj, qj = expand_edges(ii, jj, V)
    all_fixed = not (t0 < t1)
    src = set(pi.tolist())
    used = sorted(src | set(pj.tolist()))
    free = [p for p in used if not (all_fixed or (p in src and (p < t0 or p >= t1)))]
    slot = {p: s for s, p in enumerate(free)}
    mv = V > 1
    F = 1 + D
    ntail = ((V * F if mv else F) if optimize_intrinsics else 0) + (6 * (V - 1) if optimize_rig_rotation else 0)
    bandblk, degree = 0, 0
    for k in np.unique(di).tolist():
        sel = di == k
        members = [slot[p] for p in [k // V] + pj[sel].tolist() if p in slot]
        if members:
            bandblk = max(bandblk, max(members) - min(members))
        degree = max(degree, int(sel.sum()))
    return len(free), 6 * len(free) + ntail, bandblk, ntail, degree


def block_band(S, n_free):
    """largest |a - b| over the nonzero 6 x 6 blocks (a, b) of the pose part of a reduced system"""
    B = np.abs(np.asarray(S)[:6 * n_free, :6 * n_free]).reshape(n_free, 6, n_free, 6).max(axis=(1, 3)) > 0
    a, b = np.nonzero(B)
    return int(np.abs(a - b).max()) if len(a) else 0
