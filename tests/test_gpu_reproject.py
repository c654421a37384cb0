"""`reproject.hip` against the float64 oracle, beyond one workgroup, with index arrays that do not alias.

Inputs, reference and bound: oracle/pose_cases.py (grids of 2993 / 261 / 256 / 35 pixels, 8 terms over 8 frames x 2 views,
a rig without an identity row, two intrinsics rows, intr_factor 8 and 5, both depth branches, motion targets that reach
both clamps); tests/test_oracle_pose.py proves those inputs and that the usual wrong formulas leave the bound.  Every
output buffer has a guard row before and after, prefilled with a NaN bit pattern, and is compared whole."""

import numpy as np
import pytest
import torch

from oracle import geom
from oracle import pose_cases as pc

pytestmark = pytest.mark.gpu

CASES = [(g, cam) for g in pc.GRIDS for cam in ("pinhole", "mei")]
IDS = ["%dx%d-%s" % (g[0], g[1], cam) for g, cam in CASES]
NAN32, NAN16 = 0x7FC00ABC, 0x7E01  # quiet NaNs with a payload: no kernel output looks like them


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


class Guarded:
    """[rows + 2, width] buffer of NaN bit patterns; `.body` is what the kernel writes, `.intact()` says that nothing else moved"""

    def __init__(self, rows, width, dtype):
        self.pattern = NAN32 if dtype == torch.float32 else NAN16
        self.itype = torch.int32 if dtype == torch.float32 else torch.int16
        self.pat = self.pattern
        self.raw = torch.full((rows + 2, width), self.pat, dtype=self.itype, device=dev())
        self.body = self.raw[1:-1].view(dtype)

    def intact(self):
        return bool((self.raw[0] == self.pat).all()) and bool((self.raw[-1] == self.pat).all())

    def untouched(self):
        return bool((self.raw == self.pat).all())


def _inputs(c):
    return [T(a) for a in (c.poses, c.disps, c.intr, c.rig, c.pi, c.qi, c.pj, c.qj, c.di)]


def _call(fn, c, ins, outs, extra):
    from vipe_amd._lib import CAMERA_CODE, ptr, stream_ptr
    return fn(*[ptr(t) for t in ins], *outs, c.M, c.ht, c.wd, pc.V, CAMERA_CODE[c.cam], float(c.factor), *extra, stream_ptr(ins[0]))


def _reproject(c, ins, want_valid=True):
    from vipe_amd._lib import lib, ptr
    P = c.ht * c.wd
    coords, valid = Guarded(c.M, P * 2, torch.float32), Guarded(c.M, P, torch.float32)
    rc = _call(lib().vipe_reproject, c, ins, [ptr(coords.body), ptr(valid.body) if want_valid else None], [])
    torch.cuda.synchronize()
    assert rc == 0
    return coords, valid


def _motion(c, ins, target, kind):
    """kind: 'f32' / 'f16' -> vipe_reproject_motion [M,4,P]; 'nhwc' -> vipe_reproject_motion_nhwc [M,P,4] fp16"""
    from vipe_amd._lib import F16, F32, lib, ptr
    P = c.ht * c.wd
    coords = Guarded(c.M, P * 2, torch.float32)
    motn = Guarded(c.M, P * 4, torch.float32 if kind == "f32" else torch.float16)
    if kind == "nhwc":
        rc = _call(lib().vipe_reproject_motion_nhwc, c, ins, [ptr(target), ptr(coords.body), ptr(motn.body)], [])
    else:
        rc = _call(lib().vipe_reproject_motion, c, ins, [ptr(target), ptr(coords.body), ptr(motn.body)], [F32 if kind == "f32" else F16])
    torch.cuda.synchronize()
    assert rc == 0
    return coords, motn


@pytest.mark.parametrize("grid,cam", CASES, ids=IDS)
def test_reproject_coords_and_valid_against_the_float64_oracle(grid, cam):
    """coords within the per-pixel bound of oracle/pose_cases.reproject_reference at every kept pixel (all but those whose
    float64 depth is within 2e-5 of MIN_DEPTH, at most 0.5 %), finite everywhere; `valid` equal to the oracle's on the kept
    pixels; guard rows intact; without `valid` the coordinates are the same bits and the valid buffer is not touched."""
    c, r = pc.reproject_case(*grid, cam), pc.reproject_reference(*grid, cam)
    ins = _inputs(c)
    coords, valid = _reproject(c, ins)
    assert coords.intact() and valid.intact()
    got = coords.body.view(c.M, c.ht, c.wd, 2).cpu().numpy()
    assert np.isfinite(got).all()
    frac = np.abs(got.astype(np.float64) - r.coords) / r.bound
    print("reproject", grid, cam, "worst error / bound per term", frac.reshape(c.M, -1).max(1).round(3), "kept", r.keep.mean())
    assert (~r.keep).mean() <= pc.CAP
    assert np.all(frac[r.keep] <= 1.0)
    v = valid.body.view(c.M, c.ht, c.wd).cpu().numpy()
    assert np.isin(v, (0.0, 1.0)).all() and np.array_equal(v[r.keep], r.valid[r.keep].astype(np.float32))
    coords2, valid2 = _reproject(c, ins, want_valid=False)
    assert torch.equal(coords2.raw, coords.raw) and valid2.untouched()


@pytest.mark.parametrize("grid,cam", CASES, ids=IDS)
def test_motion_features_in_all_three_forms(grid, cam):
    """`vipe_reproject_motion` (fp32, fp16) and `vipe_reproject_motion_nhwc`: coords bit-equal to `vipe_reproject`'s; the
    fp32 features EQUAL the clamp of cat(coords - grid, target - coords) computed from the kernel's own coordinates
    (oracle/geom.motion_features: one float32 subtraction and the clamp), the fp16 form is that rounded to nearest even, the
    channels-last form is the fp16 form permuted; guards intact.  The target is built from the kernel's own coordinates
    (oracle/pose_cases.target_from), so that the expected features hold +64 and -64 in every channel the case can reach
    (`clamp_channels`) and at least 8 exact fp16 ties in channels 2 and 3 - asserted here, on what the kernel is fed."""
    c = pc.reproject_case(*grid, cam)
    ins = _inputs(c)
    coords, _ = _reproject(c, ins)
    own = coords.body.view(c.M, c.ht, c.wd, 2).cpu().numpy()
    tgt = pc.target_from(own)
    target = T(tgt)
    want32, want16 = geom.motion_features(own, tgt, c.ht, c.wd)
    for ch in pc.clamp_channels(grid, cam):
        assert (want32[:, ch] == 64).sum() >= 4 and (want32[:, ch] == -64).sum() >= 4, ch
    ties = pc.count_fp16_ties(want32)
    print("motion", grid, cam, "fp16 ties per channel", ties)
    assert ties[2] >= 8 and ties[3] >= 8, ties
    bits = lambda a: a.view(np.uint32 if a.dtype == np.float32 else np.uint16)
    for kind, want in (("f32", want32), ("f16", want16), ("nhwc", np.ascontiguousarray(np.moveaxis(want16, 1, -1)))):
        cm, motn = _motion(c, ins, target, kind)
        assert cm.intact() and motn.intact(), kind
        assert torch.equal(cm.raw, coords.raw), kind
        got = motn.body.cpu().numpy().reshape(want.shape)
        assert np.array_equal(bits(got), bits(want)), (kind, int((bits(got) != bits(want)).sum()))


def test_nhwc_out_buffers_are_written_and_nothing_else():
    """the wrapper's `out=`: the caller's buffers (views into larger NaN-filled ones) come back, hold what a fresh call
    returns, and their surroundings keep their bits"""
    from vipe_amd.ext import slam_ext
    grid, cam = (9, 29), "mei"
    c = pc.reproject_case(*grid, cam)
    ins = _inputs(c)
    target = T(pc.motion_target(*grid, cam))
    P = c.ht * c.wd
    cb, mb = Guarded(c.M, P * 2, torch.float32), Guarded(c.M, P * 4, torch.float16)
    oc, om = cb.body.view(c.M, c.ht, c.wd, 2), mb.body.view(c.M, c.ht, c.wd, 4)
    kw = dict(camera=cam, intr_factor=c.factor)
    rc, rm = slam_ext.reproject_motion_nhwc(*ins, target, out=(oc, om), **kw)
    fc_, fm = slam_ext.reproject_motion_nhwc(*ins, target, **kw)
    torch.cuda.synchronize()
    assert rc.data_ptr() == oc.data_ptr() and rm.data_ptr() == om.data_ptr()
    assert torch.equal(rc.view(torch.int32), fc_.view(torch.int32)) and torch.equal(rm.view(torch.int16), fm.view(torch.int16))
    assert cb.intact() and mb.intact()


def test_argument_checks_launch_nothing():
    """M = 0 with null pointers is VIPE_OK; M = 65536, camera code 7 and an unknown motn_dtype are VIPE_EINVAL - and the
    output buffers keep every bit"""
    from vipe_amd._lib import F32, lib, ptr, stream_ptr
    L = lib()
    c = pc.reproject_case(5, 7, "pinhole")
    ins = _inputs(c)
    st = stream_ptr(ins[0])
    nul = [None] * 9
    assert L.vipe_reproject(*nul, None, None, 0, 5, 7, 2, 0, 8.0, st) == 0
    assert L.vipe_reproject_motion(*nul, None, None, None, 0, 5, 7, 2, 0, 8.0, F32, st) == 0
    assert L.vipe_reproject_motion_nhwc(*nul, None, None, None, 0, 5, 7, 2, 0, 8.0, st) == 0
    P = 35
    coords, valid = Guarded(c.M, P * 2, torch.float32), Guarded(c.M, P, torch.float32)
    motn = Guarded(c.M, P * 4, torch.float32)
    target = T(pc.motion_target(5, 7, "pinhole"))
    p = [ptr(t) for t in ins]
    assert L.vipe_reproject(*p, ptr(coords.body), ptr(valid.body), 65536, 5, 7, 2, 0, 8.0, st) == -1
    assert L.vipe_reproject(*p, ptr(coords.body), ptr(valid.body), c.M, 5, 7, 2, 7, 8.0, st) == -1
    assert L.vipe_reproject_motion(*p, ptr(target), ptr(coords.body), ptr(motn.body), c.M, 5, 7, 2, 7, 8.0, F32, st) == -1
    assert L.vipe_reproject_motion(*p, ptr(target), ptr(coords.body), ptr(motn.body), c.M, 5, 7, 2, 0, 8.0, 5, st) == -1
    assert L.vipe_reproject_motion_nhwc(*p, ptr(target), ptr(coords.body), ptr(motn.body), 65536, 5, 7, 2, 0, 8.0, st) == -1
    assert L.vipe_reproject_motion_nhwc(*p, ptr(target), ptr(coords.body), ptr(motn.body), c.M, 5, 7, 2, 7, 8.0, st) == -1
    torch.cuda.synchronize()
    assert coords.untouched() and valid.untouched() and motn.untouched()
