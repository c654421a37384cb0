"""The float64 reference of the sparse tracker (tests/klt_reference.py) against ground truth - an analytic texture seen
through a known warp - and `KLTSparseTracks` driven by that reference through `_kernels=` (no GPU: the device tests pin
the kernels to the same reference)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_reference as K  # noqa: E402

_SEQ = {}


def _sequence():
    """the reference-driven run over the 6-frame sequence, once"""
    if not _SEQ:
        kern = K.NumpyKernels()
        tr, statuses = K.run_sequence(kern)
        _SEQ.update(tr=tr, statuses=statuses, kern=kern)
    return _SEQ["tr"], _SEQ["statuses"], _SEQ["kern"]


def test_reference_recovers_the_known_warp():
    """96 x 128, 3 levels, r = 4, 10 iterations, the 117 lattice points: every point within 0.1 px of the truth, the
    forward-backward distance below 0.01 px"""
    _, _, warp, pa, pb = K.pair_pyramids()
    pts = K.lattice(96, 128)
    assert len(pts) == 117
    r = K.track_fb_ref(pa, pb, pts, K.track_params(4))
    err = np.linalg.norm(r["out"] - warp.forward(pts), axis=1)
    fb = np.linalg.norm(r["back"] - pts, axis=1)
    print(f"error median {np.median(err):.4f} max {err.max():.4f} px, forward-backward max {fb.max():.5f} px")
    assert err.max() < 0.1 and fb.max() < 0.01
    assert not (r["status"].astype(int) & ~K.OOB).any()  # nothing but the coarse-level border rule flags a lattice point


def test_track_bound_is_what_the_reference_measures():
    measured = K.measure_track_bound()
    print(f"16 x float32-vs-float64 = {measured:.3e} px, TRACK_BOUND = {K.TRACK_BOUND:.3e} px")
    assert measured <= K.TRACK_BOUND <= 2 * measured
    assert K.TRACK_BOUND <= K.TRACK_BOUND_LIMIT


def test_reference_leaves_out_no_decision_on_the_named_inputs():
    _, _, _, pa, pb = K.pair_pyramids()
    r = K.track_fb_ref(pa, pb, K.lattice(96, 128), K.track_params(4), cell=16)
    assert r["clear"].all()
    for name, pts, prm in K.track_cases():
        r = K.track_fb_ref(pa, pb, pts, prm, cell=16)
        assert (~r["clear"]).sum() <= 0.02 * len(pts), name
    for H, W, cell in K.DETECT_CASES:
        img = K.pyramid_ref(K.make_pair(H, W)[0], 1)[0]
        out, clear = K.detect_ref(img, cell, 8, K.track_params()["min_eig"])
        assert clear.all() and (out[:, 0] >= 0).sum() > len(out) // 2, (H, W, cell)


def test_float32_restatement_stays_inside_the_counted_bounds():
    """the bounds of the pyramid and of the corner response hold for the reference's own float32 run"""
    for dtype in (np.float32, np.uint8):
        rgb = K.make_pair(70, 200, dtype=dtype)[0]
        p64, p32 = K.pyramid_ref(rgb, 4), K.pyramid_ref(rgb, 4, np.float32)
        for l, (a, b) in enumerate(zip(p64, p32)):
            assert np.abs(a - b).max() <= K.pyramid_c(l) * K.EPS32 * 255
    img = K.pyramid_ref(K.make_pair(90, 130)[0], 1)[0]
    r64, apc = K.response_ref(img)
    r32, _ = K.response_ref(img, np.float32)
    assert (np.abs(r32 - r64) <= K.RESPONSE_C * K.EPS32 * apc).all()


def test_detect_reference_ties_mask_and_busy():
    img = K.pyramid_ref(K.make_pair(90, 130)[0], 1)[0]
    mask = np.ones(img.shape, np.uint8)
    mask[20:50, 30:80] = 0
    busy = (np.arange(6 * 9) % 3 == 0).astype(np.uint8)
    out, _ = K.detect_ref(img, 16, 8, 4.0, mask, busy)
    assert (out[busy != 0, 0] == -1).all()
    found = out[out[:, 0] >= 0]
    assert len(found) and (mask[found[:, 1].astype(int), found[:, 0].astype(int)] != 0).all()
    assert found[:, 0].min() >= 8 and found[:, 0].max() <= 130 - 9 and found[:, 1].min() >= 8 and found[:, 1].max() <= 90 - 9
    flat, _ = K.detect_ref(np.full((40, 40), 7.0), 16, 8, 4.0)
    assert (flat[:, 0] == -1).all()
    tie, _ = K.detect_ref(np.tile(np.arange(48.0) % 2 * 50, (48, 1)), 16, 0, 0.0)  # a constant response of 0: lowest row, column
    assert (tie[:, 0] % 16 == 0).all() and (tie[:, 1] % 16 == 0).all()


def test_tracker_class_over_the_sequence():
    tr, statuses, kern = _sequence()
    frames, mask, warps = K.sequence_inputs()
    obs = tr.observations[0]
    assert len(obs) == 6 and all(len(o) > 20 for o in obs)
    assert kern.excluded <= 0.02 * kern.decisions
    # ids persist, and a persisting point follows the warp
    first = obs[0]
    kept = sorted(first.keys() & obs[5].keys())
    assert len(kept) >= 10
    p0 = np.stack([first[i] for i in kept])
    truth = warps[5].forward(p0)
    err = np.linalg.norm(np.stack([obs[5][i] for i in kept]) - truth, axis=1)
    print(f"{len(kept)} of {len(first)} points live through 6 frames, error max {err.max():.3f} px")
    assert np.mean(err < 0.15) >= 0.9
    # points leave (the image moves by (3.3, -2.6) px a frame) and free cells are refilled with new, larger ids in
    # ascending cell order
    gone = set(first) - set(obs[5])
    assert gone
    top = -1
    n_new = 0
    for k, o in enumerate(obs):
        new = sorted(i for i in o if i > top)
        if k:
            assert set(o) - set(new) <= set(obs[k - 1])
            n_new += len(new)
            cells = [int(np.floor(o[i][1] + 0.5)) // 16 * 8 + int(np.floor(o[i][0] + 0.5)) // 16 for i in new]
            assert cells == sorted(cells) and len(set(cells)) == len(cells)  # one new corner per free cell
            old_cells = {int(np.floor(o[i][1] + 0.5)) // 16 * 8 + int(np.floor(o[i][0] + 0.5)) // 16 for i in o if i not in new}
            assert not (old_cells & set(cells))  # only free cells are filled
        top = max(top, max(o))
    assert n_new > 0
    # a point that leaves through the border is flagged OOB, and no observation is reported inside the border
    assert any(s is not None and (s & K.OOB).any() for s in statuses)
    # the mask: no corner on it, and points that move onto it are dropped
    for o in obs:
        for uv in o.values():
            assert mask[int(np.floor(uv[1] + 0.5)), int(np.floor(uv[0] + 0.5))] != 0
            assert 8 <= uv[0] <= 128 - 9 and 8 <= uv[1] <= 96 - 9
    assert any(s is not None and (s & K.MASKED).any() for s in statuses)


def test_base_class_methods_read_the_dictionaries():
    tr, _, _ = _sequence()
    obs = tr.observations[0]
    ids = tr.get_correspondences(0, 1, 4)
    assert ids.tolist() == sorted(obs[1].keys() & obs[4].keys()) and len(ids) > 0
    uv = tr.get_observations(0, 4, ids)
    assert uv.shape == (len(ids), 2)
    assert np.allclose(uv.numpy(), np.stack([obs[4][int(i)] for i in ids]), atol=1e-5)
    assert tr.get_observations(0, 4, ids[:0]).shape == (0, 2)


def test_observations_through_a_standard_resize():
    """270 x 480 frames tracked at that size; with `resize` the observations are the native ones through the resize's
    scale and crop (what `forward_intrinsics` does to a principal point), and all lie inside `out_size`"""
    from vipe_amd.slam.ingest import StandardResize
    frames, _ = K.make_sequence(3, 270, 480)
    r = StandardResize(270, 480)
    native, _ = K.run_sequence(K.NumpyKernels(), frames=frames, mask=None, border=1)
    mapped, _ = K.run_sequence(K.NumpyKernels(), frames=frames, mask=None, resize=r, border=1)
    Kmat = r.forward_intrinsics(torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float64)).numpy()
    H, W = r.out_size
    n_out = 0
    for a, b in zip(native.observations[0], mapped.observations[0]):
        assert set(b) <= set(a) and len(b) > 100
        for i, uv in a.items():
            want = uv * Kmat[:2] + Kmat[2:]
            inside = 0 <= want[0] <= W - 1 and 0 <= want[1] <= H - 1
            assert (i in b) == inside
            if inside:
                assert np.abs(b[i] - want).max() < 1e-9
            n_out += not inside
    assert n_out > 0  # 270 x 480 -> 332 x 590, cropped to 328 x 584: some points fall into the cut margin
