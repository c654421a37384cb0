"""Inputs for the glue kernels of the update step (edge-store gathers, segment mean, pooled-context product, the tail of
FactorGraph.update, the motion filter's score).

ORACLE (test infrastructure).  One place builds them, seeded, so that the CPU test that checks the inputs themselves
(which copy unit a job selects, which segment sizes occur, how much the fp16 rounding of the deltas matters:
tests/test_oracle_glue.py) and the GPU test that feeds them to the kernels (tests/test_gpu_glue_kernels.py) look at the
same numbers.  Everything returned is shared between tests: do not write into it.
"""

import functools
from types import SimpleNamespace

import numpy as np

from .glue import rows_job

SENTINEL_BYTE = 0xA5
SENTINEL_F16 = np.float16(-7.0)
SENTINEL_F32 = np.float32(-12345.5)

# ------------------------------------------------------------------------------------------------ vipe_rows_gather
# launch -> [(job or None for an empty job with null pointers, rows of src, rows of dst)]
_P = 45  # a 5 x 9 grid
_BIG_ROWS = 1100
ROWS_LAUNCHES = {
    # one launch with all three copy units: 4608 B rows (unit 16), 360 B = [5,9,2] f32 (8), 36 B (4 from the size), 4608 B
    # with both views 4 bytes into their allocations (4 from the address), and 8 bytes in (8)
    "units": [(rows_job(5, 4608, [6, 0, 3, 3, 1], dst_row0=2), 7, 8),
              (rows_job(6, 360, [4, 1, 0, 8, 2, 7], dst_row0=1), 9, 8),
              (rows_job(4, 36, [2, 5, 0, 1], dst_row0=3), 6, 8),
              (rows_job(3, 4608, [1, 4, 2], dst_row0=1, src_off=4, dst_off=4), 5, 5),
              (rows_job(3, 4608, [0, 3, 2], dst_row0=2, src_off=8, dst_off=8), 4, 6)],
    # per-pixel segments: xbuf[..., :128] of a 320-channel fp16 store (256 B every 640 B, 45 pixels), and 8 B every 24 B
    "segments": [(rows_job(4, _P * 640, [5, 1, 2, 0], dst_row0=1, seg=(256, 640, _P)), 6, 6),
                 (rows_job(5, 7 * 24, [3, 3, 0, 6, 1], dst_row0=2, seg=(8, 24, 7)), 7, 8)],
    # no index (row r -> dst_row0 + r), and an index that is no ascending keep-list: descending with repeats
    "indices": [(rows_job(4, 360, None, dst_row0=3), 4, 8),
                (rows_job(6, 360, [8, 8, 5, 3, 3, 0], dst_row0=1), 9, 8)],
    # eight jobs, job 0 and job 3 empty; job 2 has 1100 x 1001 four-byte units > 4096 blocks x 256 lanes: a second trip
    "big": [(None, 0, 0),
            (rows_job(3, 4608, [4, 0, 2], dst_row0=1), 5, 5),
            (rows_job(_BIG_ROWS, 4004, np.random.default_rng(5).permutation(_BIG_ROWS), dst_row0=2), _BIG_ROWS, _BIG_ROWS + 3),
            (None, 0, 0),
            (rows_job(1, 4, [2], dst_row0=1), 3, 3),
            (rows_job(2, 360, [1, 0], dst_row0=0), 2, 3),
            (rows_job(3, 36, [0, 2, 2], dst_row0=2), 3, 6),
            (rows_job(2, 7 * 24, [1, 0], dst_row0=1, seg=(8, 24, 7)), 2, 4)],
}


@functools.lru_cache(maxsize=None)
def rows_launch(name):
    """-> [SimpleNamespace(job, src [bytes] uint8, dst [bytes] uint8 = the sentinel)] (job None: an empty job)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    out = []
    for job, n_src, n_dst in ROWS_LAUNCHES[name]:
        if job is None:
            out.append(SimpleNamespace(job=None, src=None, dst=None))
            continue
        src = rng.integers(0, 256, job["src_off"] + n_src * job["src_row_pitch"], dtype=np.uint8)
        dst = np.full(job["dst_off"] + n_dst * job["dst_row_pitch"], SENTINEL_BYTE, dtype=np.uint8)
        out.append(SimpleNamespace(job=job, src=src, dst=dst))
    return out


# ---------------------------------------------------------------------------------- vipe_gather_nchw_to_nhwc_f16
# (C, P, dst_ctot, dst_coff): one, exactly one, one and a bit, two and a bit, three and a bit 64-pixel tiles; channel counts
# that divide 256 lanes and that do not; a slice in the middle of a wider store
NHWC_SINGLE = [(128, 45, 128, 0), (128, 64, 128, 0), (128, 65, 128, 0), (96, 130, 104, 8), (64, 200, 320, 128), (8, 1, 8, 0),
               (3, 200, 5, 1)]
NHWC_FRAMES = np.array([3, 0, 3, 1], dtype=np.int64)  # unsorted, with a repeat
NHWC_N = 5
NHWC_ROW0 = 2
# one launch, eight jobs: (dst_ctot, dst_coff, dst_row0, frames)
NHWC_MULTI_CP = (32, 70)
NHWC_MULTI = [(32, 0, 0, [3, 0, 3]), (40, 8, 1, [1, 1, 4]), (64, 32, 2, [4, 2, 0]), (320, 128, 0, [0, 3, 1]),
              (33, 1, 1, [2, 4, 4]), (128, 96, 2, [3, 1, 0]), (48, 0, 1, [0, 0, 2]), (36, 3, 0, [4, 3, 2])]
NHWC_NULL_FRAME = (16, 70, 24, 4, 1, 3)  # C, P, dst_ctot, dst_coff, dst_row0, n_rows: row r reads frame r


@functools.lru_cache(maxsize=None)
def nhwc_src(C, P, seed=0):
    """[NHWC_N, C, P] fp16"""
    return np.random.default_rng(1000 * C + P + seed).normal(0, 1, (NHWC_N, C, P)).astype(np.float16)


def nhwc_dst(rows, P, ctot):
    return np.full((rows, P, ctot), SENTINEL_F16, dtype=np.float16)


# ---------------------------------------------------------------------------------- vipe_segment_mean_nhwc_f16
SEG_SIZES = [2, 0, 37, 1, 3]  # edges per segment; the last one holds inputs in fp16's subnormal range
# name -> (rows per item, src_ctot, src_coff, C)
SEG_LAYOUTS = {"operator": (45, 384, 256, 128), "narrow": (7, 8, 0, 8), "middle": (11, 40, 8, 24)}
SEG_STRIDE = (16400, 128, 0, 128)  # 16400 x 16 eight-channel units > 1024 blocks x 256 lanes: a second trip


@functools.lru_cache(maxsize=None)
def segment_case(name):
    """-> SimpleNamespace(src [E, rows, ctot] fp16, ctot, coff, C, order [E] int32, rowptr [n_out + 1] int32)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "stride":
        rows, ctot, coff, C = SEG_STRIDE
        order, rowptr = np.array([2, 0, 1], dtype=np.int32), np.array([0, 2, 3], dtype=np.int32)
    else:
        rows, ctot, coff, C = SEG_LAYOUTS[name]
        rowptr = np.concatenate([[0], np.cumsum(SEG_SIZES)]).astype(np.int32)
        order = rng.permutation(int(rowptr[-1])).astype(np.int32)  # edges interleaved over the segments
    E = int(rowptr[-1])
    x = rng.normal(0, 1, (E, rows, ctot))
    if name != "stride":
        x[order[rowptr[-2]:rowptr[-1]]] *= 3e-5
        outside = np.ones(ctot, dtype=bool)
        outside[coff:coff + C] = False
        x[..., outside] = np.where(np.arange(int(outside.sum())) % 2 == 0, 1000.0, -1000.0)  # an offset error is obvious
    return SimpleNamespace(src=x.astype(np.float16), ctot=ctot, coff=coff, C=C, order=order, rowptr=rowptr, rows=rows)


# ------------------------------------------------------------------------------------------------ vipe_glo_context
GLO_E = [1, 5, 300]
GLO_HW = [1, 3, 45, 3072]


@functools.lru_cache(maxsize=None)
def glo_case(E, hw):
    """the sum over hw pixels of sigmoid(.) * net per channel (values of the order hw), weights, bias: float32"""
    rng = np.random.default_rng(10 * E + hw)
    return SimpleNamespace(glo_sum=(rng.normal(0, 0.5, (E, 128)) * hw).astype(np.float32),
                           wT=(rng.normal(0, 1, (128, 384)) / np.sqrt(128)).astype(np.float32),
                           bias=rng.normal(0, 0.1, 384).astype(np.float32))


# ------------------------------------------------------------------------------------------------ vipe_update_finish
UF_GRIDS = [(5, 5, 9), (3, 7, 37)]  # (E, h, w): 225 pixels, under one workgroup / 777, a partial last one
UF_DAMPING_ROWS = 9
# per E: source frames of the eta maps.  none: n_src = 0; fewer: n_src < E; equal: n_src == E, a permutation
UF_DU = {5: {"none": None, "fewer": [7, 2, 4], "equal": [3, 0, 4, 1, 2]}, 3: {"none": None, "fewer": [7, 2], "equal": [2, 0, 1]}}
UF_MORE = ((1, 5, 9), [5, 0, 7])  # n_src > E, through the ABI only: the launch is sized by the eta maps


@functools.lru_cache(maxsize=None)
def finish_case(E, h, w, du, masked):
    """du: tuple or None.  mask (when `masked`): ~30 % of the pixels of every edge but the first (of the only one when E == 1)"""
    rng = np.random.default_rng(100 * E + w + (7 if masked else 0) + (0 if du is None else 13 * len(du)))
    c = SimpleNamespace(E=E, h=h, w=w)
    c.coords1 = rng.uniform(-2, 40, (E, h, w, 2)).astype(np.float32)
    c.dw = np.concatenate([rng.normal(0, 1.5, (E, h, w, 2)), rng.uniform(0.01, 1, (E, h, w, 2))], -1).astype(np.float32)
    c.mask = None
    if masked:
        c.mask = rng.uniform(0, 1, (E, h, w)) < 0.3
        if E > 1:
            c.mask[0] = False
    c.du = None if du is None else np.array(du, dtype=np.int64)
    c.eta = None if du is None else rng.uniform(0.001, 0.1, (len(du), h, w)).astype(np.float32)
    c.damping = rng.uniform(1, 2, (UF_DAMPING_ROWS, h, w)).astype(np.float32)
    return c


# ------------------------------------------------------------------------------------------------ vipe_flow_score
FLOW_SIZES = [(1, 45), (2, 192), (3, 256), (2, 257), (2, 3072)]  # (views, P)
FLOW_MAGNITUDES = ["unit", "large"]
FLOW_MASKS = ["none", "random", "first_invalid", "last_valid"]


@functools.lru_cache(maxsize=None)
def flow_case(V, P, magnitude, mask, nan_weights=False):
    """dw [V,P,4] float32, invalid [V,P] bool or None.
    unit: deltas ~ N(0, 1).  large: |components| in [2048, 2900) (|delta| about 3500), where fp16 steps are 2, each 0.9 -
    0.999 above a multiple of 2: the fp16 rounding lowers EVERY component by that much - it does not average out.
    random: each pixel invalid with probability 0.4; first_invalid: view 0 wholly invalid on top of that; last_valid:
    the last view wholly valid on top of that (a mask is passed, the divisor is 1 + 1e-6)"""
    rng = np.random.default_rng(V * 10000 + P + (1 if magnitude == "large" else 0))
    if magnitude == "unit":
        d = rng.normal(0, 1, (V, P, 2))
    else:
        grid = 2.0 * np.floor(rng.uniform(2048, 2900, (V, P, 2)) / 2.0)
        d = (grid + rng.uniform(0.9, 0.999, (V, P, 2))) * rng.choice([-1.0, 1.0], (V, P, 2))
    wts = rng.uniform(0, 1, (V, P, 2))
    if nan_weights:
        wts[:] = np.nan
    dw = np.concatenate([d, wts], -1).astype(np.float32)
    invalid = None
    if mask != "none":
        invalid = rng.uniform(0, 1, (V, P)) < 0.4
        if mask == "first_invalid":
            invalid[0] = True
        if mask == "last_valid":
            invalid[-1] = False
    return SimpleNamespace(dw=dw, invalid=invalid, V=V, P=P)
