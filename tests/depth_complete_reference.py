"""Float64 restatement of `vipe_depth_complete` (include/vipe_amd.h, csrc/depth_complete.hip) by brute force, with the
float32 bounds of everything the kernel thresholds and of what it writes.  Not a test module; the tests import it.

The neighbours are integers: every anchor of the image is tried for every target, the K smallest by (d2, dy, dx) are kept.
No tolerance applies to them.

The fit is evaluated in float64 on the values the kernel loads (the stored f32 / f16 numbers; in the depth domain their
float64 reciprocals).  Bounds, first order in u = 2^-24 with a guard factor G = 1.02 for the higher orders, n = k'
neighbours, c = 1 in the depth domain (each loaded disparity is one rounded division) and 0 otherwise:

    w = 1 / d2                      one division: relative u
    S = sum w                       n - 1 additions of positive terms: relative n u
    sum w p                         per term (2 + c) u (w, p, the product), n - 1 additions: relative (n + 1 + c) u
    pm, dm                          one more division: relative em = (2 n + 2 + c) u
    e = p - pm                      absolute Ae = c u |p| + em pm + u |e|;   f = d - dm likewise, Af
    var = sum (w e) e               A_var = sum w (2 |e| Ae + Ae^2) + (n + 2) u sum w e^2     (w, two products, n - 1 additions)
    cov = sum (w e) f               A_cov = sum w (|e| Af + |f| Ae + Ae Af) + (n + 2) u sum w |e f|
    thr = ((2^-10 pm)(2^-10 pm)) S  relative 2 em + (n + 2) u  (the scalings are exact)
    s = cov / var                   A_s = (A_cov + |s| A_var) / (var - A_var) + u |s|
    t = dm - s pm                   A_t = em dm + |s| em pm + pm A_s + u |s pm| + u |t|
    s = dm / pm (scale only)        A_s = |s| (2 em + u),  A_t = 0
    r = s p + t                     A_r = A_s p + |s| c u p + u |s p| + A_t + u |r|
    out = r (disparity domain)      A_out = A_r
    out = 1 / r (depth domain)      A_out = A_r / (r (r - A_r)) + u / r
    f16 output                      + 2^-11 (|out| + A_out) + 2^-25

Three quantities are thresholded: var against thr, the sign of cov (that of s, var being positive), the sign of r.  A
target is DECIDED when each is cleared by more than its bound; an undecided target may come out by either branch
(`alts`).  Values are assumed to stay in the normal range of the formats (no overflow, no underflow)."""
import numpy as np

U = 2.0 ** -24
G = 1.02
STATS = ("affine", "scale_only", "unreached", "rejected")
BIG = np.int64(1) << 62


def pos_finite(v):
    with np.errstate(invalid="ignore"):
        return np.isfinite(v) & (v > 0)


def classify(sparse, pred, mask=None):
    """-> (anchor, target) bool [H,W] of one image"""
    s, p = sparse.astype(np.float64), pred.astype(np.float64)
    anchor = pos_finite(s) & pos_finite(p)
    target = ~anchor & pos_finite(p)
    if mask is not None:
        target &= np.asarray(mask) != 0
    return anchor, target


def neighbours(anchor, ty, tx, K, R, wrap=False):
    """anchors [H,W] bool, targets (ty, tx) -> (d2 [T,K] int64 with -1 padding, index [T,K] int64 row-major, -1 padded), the
    K smallest by (d2, dy, dx) among the anchors with d2 <= R^2; with `wrap` dx is the column offset of smallest magnitude"""
    H, W = anchor.shape
    ay, ax = np.nonzero(anchor)
    T = len(ty)
    d2_out = np.full((T, K), -1, dtype=np.int64)
    idx_out = np.full((T, K), -1, dtype=np.int64)
    if len(ay) == 0 or T == 0:
        return d2_out, idx_out
    for c0 in range(0, T, 512):
        y, x = ty[c0:c0 + 512, None].astype(np.int64), tx[c0:c0 + 512, None].astype(np.int64)
        dy, dx = ay[None, :] - y, ax[None, :] - x
        if wrap:
            dx = dx - W * np.round(dx / W).astype(np.int64)
        d2 = dy * dy + dx * dx
        # the rule's lexicographic key as one integer: offsets are within [-R, R] wherever the key counts
        key = np.where(d2 <= R * R, (d2 << 40) | ((dy + (1 << 19)) << 20) | (dx + (1 << 19)), BIG)
        order = np.argsort(key, axis=1, kind="stable")[:, :K]
        kk = np.take_along_axis(key, order, 1)
        ok = kk < BIG
        n = order.shape[1]
        d2_out[c0:c0 + 512, :n] = np.where(ok, np.take_along_axis(d2, order, 1), -1)
        idx_out[c0:c0 + 512, :n] = np.where(ok, ay[order] * W + ax[order], -1)
    return d2_out, idx_out


def neighbours_scan(anchor, ty, tx, K, R, wrap=False):
    """`neighbours` for images too large to try every anchor for every target (the end-to-end runs): the offsets of the
    disc are walked in key order and every target takes the first K that land on an anchor.  Same result
    (tests/test_depth_complete_reference.py compares the two on the seeded cases)."""
    H, W = anchor.shape
    T = len(ty)
    d2_out = np.full((T, K), -1, dtype=np.int64)
    idx_out = np.full((T, K), -1, dtype=np.int64)
    cnt = np.zeros(T, dtype=np.int64)
    offs = sorted((dy * dy + dx * dx, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if dy * dy + dx * dx <= R * R)
    live = np.arange(T)
    for d2, dy, dx in offs[1:]:  # the first offset is the target itself
        yy, xx = ty[live] + dy, tx[live] + dx
        inside = (yy >= 0) & (yy < H)
        if wrap:
            xx = xx % W
        else:
            inside &= (xx >= 0) & (xx < W)
        hit = np.zeros(len(live), bool)
        hit[inside] = anchor[yy[inside], xx[inside]]
        rows = live[hit]
        if len(rows):
            d2_out[rows, cnt[rows]] = d2
            idx_out[rows, cnt[rows]] = yy[hit] * W + xx[hit]
            cnt[rows] += 1
            live = live[cnt[live] < K]
            if len(live) == 0:
                break
    return d2_out, idx_out


def fit(d2, p, d, pt, depth_domain, f16_out):
    """d2 [T,K] (-1 = none), p, d [T,K] and pt [T] float64 disparities -> dict of per-target arrays (see `complete_ref`)"""
    valid = d2 > 0
    n = valid.sum(1)
    c = 1.0 if depth_domain else 0.0
    with np.errstate(all="ignore"):
        w = np.where(valid, 1.0 / np.where(valid, d2, 1), 0.0)
        p, d = np.where(valid, p, 0.0), np.where(valid, d, 0.0)
        S = w.sum(1)
        pm, dm = (w * p).sum(1) / S, (w * d).sum(1) / S
        em = (2 * n + 2 + c) * U * G
        e, f = np.where(valid, p - pm[:, None], 0.0), np.where(valid, d - dm[:, None], 0.0)
        Ae = np.where(valid, (c * U * np.abs(p) + (em * pm)[:, None] + U * np.abs(e)) * G, 0.0)
        Af = np.where(valid, (c * U * np.abs(d) + (em * dm)[:, None] + U * np.abs(f)) * G, 0.0)
        var, cov = (w * e * e).sum(1), (w * e * f).sum(1)
        A_var = ((w * (2 * np.abs(e) * Ae + Ae * Ae)).sum(1) + (n + 2) * U * var) * G
        A_cov = ((w * (np.abs(e) * Af + np.abs(f) * Ae + Ae * Af)).sum(1) + (n + 2) * U * (w * np.abs(e * f)).sum(1)) * G
        thr = (2.0 ** -10 * pm) ** 2 * S
        A_thr = thr * (2 * em + (n + 2) * U) * G
        var_hi, var_lo = var - thr > A_var + A_thr, var - thr < -(A_var + A_thr)
        cov_pos, cov_neg = cov > A_cov, cov < -A_cov
        many = n >= 2
        is_affine = many & (var > thr) & (cov / var > 0)  # float64's own decision
        can_aff = many & ~var_lo & ~cov_neg
        can_sc = ~(many & var_hi & cov_pos)
        # the two branches
        s_a = cov / var
        As_a = np.where(var > A_var, (A_cov + np.abs(s_a) * A_var) / (var - A_var) + U * np.abs(s_a), np.inf) * G
        t_a = dm - s_a * pm
        At_a = (em * dm + np.abs(s_a) * em * pm + pm * As_a + U * np.abs(s_a * pm) + U * np.abs(t_a)) * G
        s_s = dm / pm
        As_s = np.abs(s_s) * (2 * em + U) * G
        branches = {}
        for name, s, t, As, At in (("affine", s_a, t_a, As_a, At_a), ("scale", s_s, np.zeros_like(s_s), As_s, np.zeros_like(s_s))):
            r = s * pt + t
            Ar = (As * pt + np.abs(s) * c * U * pt + U * np.abs(s * pt) + At + U * np.abs(r)) * G
            Ar = np.where(np.isfinite(Ar), Ar, np.inf)
            if depth_domain:
                out = 1.0 / r
                A_out = np.where(r > Ar, Ar / (r * (r - Ar)) + U / r, np.inf) * G
            else:
                out, A_out = r, Ar
            if f16_out:
                A_out = A_out + 2.0 ** -11 * (np.abs(out) + A_out) + 2.0 ** -25
            # `value`: the branch may write a number (r is not below zero by more than its bound); `zero`: it may reject
            branches[name] = dict(s=s, t=t, A_s=As, A_t=At, r=r, A_r=Ar, out=out, A_out=A_out, value=~(r < -Ar),
                                  zero=~(r > Ar), ok=np.isfinite(r) & (r > 0))
    reached = n > 0
    # all neighbours hold one and the same sparse value (one point's footprint, drawn over several pixels): cov is zero in
    # exact arithmetic and its sign is rounding's in any finite one - no bound can decide such a target
    flat = many & (np.where(valid, d, -np.inf).max(1) == np.where(valid, d, np.inf).min(1))
    can_aff, can_sc = can_aff & reached, can_sc & reached
    a, s = branches["affine"], branches["scale"]
    n_alts = (can_aff & a["value"]).astype(int) + (can_aff & a["zero"]) + (can_sc & s["value"]) + (can_sc & s["zero"])
    decided = ~reached | (n_alts == 1)
    chosen_ok = np.where(is_affine, a["ok"], s["ok"])
    kind = np.where(~reached, 2, np.where(~chosen_ok, 3, np.where(is_affine, 0, 1)))
    pick = lambda key: np.where(is_affine, a[key], s[key])
    result = np.where(reached & chosen_ok, pick("out"), 0.0)
    return dict(n=n, var=var, thr=thr, A_var=A_var + A_thr, cov=cov, A_cov=A_cov, is_affine=is_affine, can_affine=can_aff,
                can_scale=can_sc, affine=a, scale=s, decided=decided, flat=flat, kind=kind, result=result,
                s=np.where(reached & chosen_ok, pick("s"), 0.0), t=np.where(reached & chosen_ok, pick("t"), 0.0),
                A_out=np.where(reached & chosen_ok, pick("A_out"), 0.0), reached=reached)


def complete_ref(sparse, pred, K, R, domain="depth", mask=None, wrap=False, scan=False):
    """One image: sparse, pred [H,W] float32 / float16 arrays as the kernel loads them -> dict:
    anchor, target [H,W]; ty, tx [T]; nbr [T,K] row-major indices in key order (-1 padded); d2 [T,K]; the per-target
    arrays of `fit`: s, t, result (0 where unreached or rejected), A_out, kind (index into STATS), decided, the thresholded
    quantities with their bounds (var / thr / A_var, cov / A_cov, per branch r / A_r) and both branches' outputs with their
    bounds for the undecided; stats [4], float64's own counts.  `scan`: find the neighbours with `neighbours_scan`."""
    assert sparse.shape == pred.shape and sparse.dtype == pred.dtype and sparse.dtype in (np.float32, np.float16)
    assert 1 <= K <= 8 and 1 <= R <= 64 and domain in ("depth", "disp")
    H, W = sparse.shape
    assert not wrap or W >= 2 * R + 1
    anchor, target = classify(sparse, pred, mask)
    ty, tx = np.nonzero(target)
    d2, idx = (neighbours_scan if scan else neighbours)(anchor, ty, tx, K, R, wrap)
    sv, pv = sparse.astype(np.float64).ravel(), pred.astype(np.float64).ravel()
    safe = np.where(idx >= 0, idx, 0)
    depth = domain == "depth"
    with np.errstate(all="ignore"):
        conv = (lambda v: 1.0 / v) if depth else (lambda v: v)
        res = fit(d2, conv(pv[safe]), conv(sv[safe]), conv(pv[ty * W + tx]), depth, sparse.dtype == np.float16)
    res.update(anchor=anchor, target=target, ty=ty, tx=tx, nbr=idx, d2=d2,
               stats=np.array([int((res["kind"] == k).sum()) for k in range(4)], dtype=np.int64))
    return res


def check_image(ref, sparse, out, nbr=None, scale=None, shift=None):
    """One image of the kernel's outputs against `complete_ref`'s dict -> (targets, undecided): asserts anchors copied
    bit for bit, zeros at pixels that are neither, the neighbour lists exactly, every target inside the bound of a branch
    it may take."""
    H, W = sparse.shape
    anchor, target, ty, tx = ref["anchor"], ref["target"], ref["ty"], ref["tx"]
    bits = np.uint32 if sparse.dtype == np.float32 else np.uint16
    assert out.dtype == sparse.dtype and out.shape == sparse.shape
    assert np.array_equal(out.view(bits)[anchor], sparse.view(bits)[anchor]), "anchors are copied bit for bit"
    assert np.all(out.view(bits)[~anchor & ~target] == 0), "+0 where the pixel is neither anchor nor target"
    K = ref["nbr"].shape[1]
    if nbr is not None:
        assert nbr.shape == (H, W, K) and nbr.dtype == np.int32
        assert np.all(nbr[~target] == -1), "no neighbours at non-targets"
        bad = np.nonzero((nbr[ty, tx].astype(np.int64) != ref["nbr"]).any(1))[0]
        assert len(bad) == 0, (f"{len(bad)} neighbour lists differ, first at ({ty[bad[0]]}, {tx[bad[0]]}): "
                               f"{nbr[ty[bad[0]], tx[bad[0]]].tolist()} against {ref['nbr'][bad[0]].tolist()}")
    got = out[ty, tx].astype(np.float64)
    ok = ~ref["reached"] & (got == 0)
    with np.errstate(invalid="ignore"):
        for name, can in (("affine", ref["can_affine"]), ("scale", ref["can_scale"])):
            br = ref[name]
            ok |= can & br["value"] & (np.abs(got - br["out"]) <= br["A_out"])
            ok |= can & br["zero"] & (got == 0)
    bad = np.nonzero(~ok)[0]
    assert len(bad) == 0, (f"{len(bad)} of {len(ty)} targets outside every admissible bound, first at ({ty[bad[0]]}, {tx[bad[0]]}): "
                           f"got {got[bad[0]]!r}, reference {ref['result'][bad[0]]!r} +- {ref['A_out'][bad[0]]:.3e}, "
                           f"decided {bool(ref['decided'][bad[0]])}")
    if scale is not None:
        assert np.all(scale[anchor] == 1) and np.all(shift[anchor] == 0) and np.all(scale[~anchor & ~target] == 0) \
            and np.all(shift[~anchor & ~target] == 0)
        zero = got == 0
        assert np.all(scale[ty, tx][zero] == 0) and np.all(shift[ty, tx][zero] == 0), "(0, 0) where nothing was fitted"
        d = ref["decided"] & ~zero  # there the branch is known: the stored pair lies within A_s, A_t of float64's
        A_s = np.where(ref["is_affine"], ref["affine"]["A_s"], ref["scale"]["A_s"])
        A_t = np.where(ref["is_affine"], ref["affine"]["A_t"], ref["scale"]["A_t"])
        assert np.all(np.abs(scale[ty, tx] - ref["s"])[d] <= A_s[d]), "scale within its bound at decided targets"
        assert np.all(np.abs(shift[ty, tx] - ref["t"])[d] <= A_t[d]), "shift within its bound at decided targets"
    return len(ty), int((~ref["decided"]).sum())


def emulate_f32(ref, sparse, pred, domain="depth"):
    """The kernel's arithmetic step by step in numpy float32 (every operation rounded on its own, neighbours in key
    order) on the reference's neighbour lists -> (out [H,W] of the maps' dtype, scale, shift [H,W] f32, stats [4]): what a
    correct build writes, up to the last bit of the divisions.  It lets the bounds be checked without a device."""
    f = np.float32
    H, W = sparse.shape
    idx, d2, ty, tx = ref["nbr"], ref["d2"], ref["ty"], ref["tx"]
    valid, safe = idx >= 0, np.where(idx >= 0, idx, 0)
    depth = domain == "depth"
    one = f(1.0)
    with np.errstate(all="ignore"):
        conv = (lambda v: one / v) if depth else (lambda v: v)
        p, d = conv(pred.astype(f).ravel()[safe]), conv(sparse.astype(f).ravel()[safe])
        pt = conv(pred.astype(f)[ty, tx])
        w = one / np.where(valid, d2, 1).astype(f)
        T, K = idx.shape
        S, Sp, Sd = np.zeros(T, f), np.zeros(T, f), np.zeros(T, f)
        for i in range(K):
            m = valid[:, i]
            S, Sp, Sd = np.where(m, S + w[:, i], S), np.where(m, Sp + w[:, i] * p[:, i], Sp), np.where(m, Sd + w[:, i] * d[:, i], Sd)
        pm, dm = Sp / S, Sd / S
        var, cov = np.zeros(T, f), np.zeros(T, f)
        for i in range(K):
            m = valid[:, i]
            e, g = p[:, i] - pm, d[:, i] - dm
            we = w[:, i] * e
            var, cov = np.where(m, var + we * e, var), np.where(m, cov + we * g, cov)
        e0 = f(2.0 ** -10) * pm
        thr = (e0 * e0) * S
        n = valid.sum(1)
        s_a = cov / var
        affine = (n >= 2) & (var > thr) & (s_a > 0)
        s = np.where(affine, s_a, dm / pm).astype(f)
        t = np.where(affine, dm - s * pm, f(0)).astype(f)
        r = s * pt + t
        ok = (n > 0) & np.isfinite(r) & (r > 0)
        res = np.where(ok, one / r if depth else r, f(0)).astype(f)
    out = np.zeros((H, W), sparse.dtype)
    out[ref["anchor"]] = sparse[ref["anchor"]]
    out[ty, tx] = res.astype(sparse.dtype)
    scale, shift = np.zeros((H, W), f), np.zeros((H, W), f)
    scale[ref["anchor"]] = 1
    scale[ty, tx], shift[ty, tx] = np.where(ok, s, f(0)), np.where(ok, t, f(0))
    kind = np.where(n == 0, 2, np.where(~ok, 3, np.where(affine, 0, 1)))
    return out, scale, shift, np.array([int((kind == k).sum()) for k in range(4)], dtype=np.int64)


def make_case(seed, H, W, density=0.2, dtype=np.float32, domain="depth", hole=None, strip=None):
    """A seeded scene -> (sparse, pred): a smooth positive field as the truth, the prediction a smoothly varying affine
    distortion of it (in the disparity domain) with 2 % multiplicative noise, sparse samples of the truth at `density`;
    `hole` (y0, y1, x0, x1) and `strip` (x0, x1) remove the samples of a rectangle / of whole columns."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    truth = 1.0 + 0.6 * np.sin(3.1 * xx + 0.5) * np.cos(2.3 * yy) + 0.8 * yy  # disparities, 0.4 .. 2.4
    a, b = 1.3 + 0.3 * np.sin(2.0 * xx + yy), 0.1 + 0.05 * np.cos(3.0 * yy)
    pred = np.maximum((truth - b) / a, 0.05) * (1.0 + 0.02 * rng.standard_normal((H, W)))
    keep = rng.random((H, W)) < density
    if hole is not None:
        keep[hole[0]:hole[1], hole[2]:hole[3]] = False
    if strip is not None:
        keep[:, strip[0]:strip[1]] = False
    sparse = np.where(keep, truth * (1.0 + 0.005 * rng.standard_normal((H, W))), 0.0)
    if domain == "depth":
        pred, sparse = 1.0 / pred, np.where(keep, 1.0 / np.where(keep, sparse, 1.0), 0.0)
    return sparse.astype(dtype), pred.astype(dtype)


# The seeded cases of tests/test_gpu_depth_complete.py (their undecided shares are checked on the CPU in
# tests/test_depth_complete_reference.py and listed in DESIGN.md section 20).  Sizes are no multiples of the 64 x 4
# tile; widths 63, 64, 65, 129 and 130 sit around the bit-word boundaries; K covers 1, 2, 5, 8 and R 1, 3, 12, 64.
CASES = [
    dict(name="23x41_k5_r12", seed=1, B=1, H=23, W=41, K=5, R=12, dtype="f32", domain="depth", density=0.2),
    dict(name="37x63_k1_r3_disp", seed=2, B=2, H=37, W=63, K=1, R=3, dtype="f32", domain="disp", density=0.2),
    dict(name="29x64_k2_r12_f16", seed=3, B=1, H=29, W=64, K=2, R=12, dtype="f16", domain="depth", density=0.2),
    dict(name="31x65_k8_r64", seed=4, B=1, H=31, W=65, K=8, R=64, dtype="f32", domain="depth", density=0.05),
    dict(name="61x130_k5_r12_hole", seed=5, B=1, H=61, W=130, K=5, R=12, dtype="f32", domain="depth", density=0.2,
         hole=(8, 52, 30, 90)),
    dict(name="45x129_k5_r64_f16_disp", seed=6, B=3, H=45, W=129, K=5, R=64, dtype="f16", domain="disp", density=0.02),
    dict(name="33x77_k8_r1_disp", seed=7, B=1, H=33, W=77, K=8, R=1, dtype="f32", domain="disp", density=0.4),
    dict(name="27x70_k5_r12_wrap", seed=8, B=1, H=27, W=70, K=5, R=12, dtype="f32", domain="depth", density=0.2, wrap=True,
         strip=(24, 46)),
    dict(name="25x25_k5_r12_wrap_min", seed=9, B=2, H=25, W=25, K=5, R=12, dtype="f32", domain="disp", density=0.1, wrap=True),
    dict(name="41x129_k2_r64_wrap_f16", seed=10, B=1, H=41, W=129, K=2, R=64, dtype="f16", domain="depth", density=0.03,
         wrap=True),
    dict(name="35x65_k5_r3_mask_poison", seed=11, B=2, H=35, W=65, K=5, R=3, dtype="f32", domain="depth", density=0.3,
         mask=True, poison=True),
    dict(name="30x63_k2_r12_f16_poison", seed=12, B=1, H=30, W=63, K=2, R=12, dtype="f16", domain="disp", density=0.2,
         poison=True),
]
UNDECIDED_CAP = 0.02


def build_case(case):
    """-> (sparse [B,H,W], pred [B,H,W], mask [B,H,W] uint8 or None) of one entry of CASES"""
    dtype = np.float32 if case["dtype"] == "f32" else np.float16
    maps = [make_case(case["seed"] * 100 + b, case["H"], case["W"], case["density"], dtype, case["domain"], case.get("hole"),
                      case.get("strip")) for b in range(case["B"])]
    sparse, pred = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    rng = np.random.default_rng(case["seed"] + 7000)
    if case.get("poison"):  # NaN, +-inf, 0 and negative values in either map
        for arr in (sparse, pred):
            for v in (np.nan, np.inf, -np.inf, 0.0, -1.5):
                arr[rng.random(arr.shape) < 0.01] = v
    mask = (rng.random(sparse.shape) < 0.7).astype(np.uint8) if case.get("mask") else None
    return sparse, pred, mask


def case_refs(case):
    """-> (sparse, pred, mask, [reference dict per image])"""
    sparse, pred, mask = build_case(case)
    refs = [complete_ref(sparse[b], pred[b], case["K"], case["R"], case["domain"], None if mask is None else mask[b],
                         bool(case.get("wrap"))) for b in range(case["B"])]
    return sparse, pred, mask, refs
