"""Float64 references and error bounds for the four groups of lietorch_ext: SO3, RxSO3, SE3, Sim3.

ORACLE (test infrastructure).  Rows as in the library: SO3 [q], RxSO3 [q, s], SE3 [t, q], Sim3 [t, q, s] with q = (x, y, z, w);
tangents [phi], [phi, sigma], [tau, phi], [tau, phi, sigma].  Quaternions are normalised on load, as the kernels do.

What is a convention follows the reference as `lie_math.h` restates it:
  * `log` of a quaternion with w < 0 is f * v with f = 2 atan(n / w) / n < 0, i.e. the rotation vector of -q: the short way
    round, |phi| < pi (so3.h:96-131).  `log` of an exactly zero vector part is zero.
  * Sim3 `Jinv` uses the TRUNCATED series I - Xi/2 + Xi^2/12 - Xi^4/720 in Xi = adj(log X) (sim3.h:176-184), not the inverse
    of the true left Jacobian.  RxSO3 pads the SO3 inverse Jacobian with a 1 (rxso3.h:286-292).

What is arithmetic does NOT follow the closed forms, whose float64 run loses digits where they cancel (1 - cos t below
t ~ 1e-4, exp(s) - 1 below s ~ 1e-3): the translation part W(phi, sigma) = int_0^1 exp(u (Phi + sigma I)) du = C I + A Phi
+ B Phi^2 is integrated by a 32-point Gauss-Legendre rule on integrands without a subtraction (`calc_w_coeffs`).
scipy's 4 x 4 matrix exponential of `hat(a)` is the independent formulation it is pinned to (tests/test_oracle_pose.py,
all 1000 rows of every set, 4e-14 of the matrix's size) and can be asked for (`matrix_exponential=True`); it is not
the row-wise reference because its own error - 1.6e-14 at |a| ~ 3, scaling and squaring - is above what the float64
kernels are held to.

ERROR BOUNDS (`bound`).  u = 2^-24 (float32) or 2^-53 (float64).  Every op gets BASE = 16 u x (the magnitude of the
row's output, stated per op below): a dozen roundings of products of O(1) quaternion entries, an ulp for sin / cos / atan
/ exp / log, and the renormalisation.  On top of it, three kinds of explicit terms:

 (a) cancellation in W (`w_coeff_errors`), where the closed forms subtract nearly equal numbers; the error of a
     numerator is the rounding of its largest operand, divided by the small denominator:
       |sigma| < EPS (and all of SO3 / SE3, `left_jacobian_mul`):
           A = (1 - cos t) / t^2: below 1 the cosine is a multiple of 2 u, so 1 - cos t is off by up to 2 u (a cosine that
           is an ulp off) and A by 2 u / t^2 - or by A itself (<= 1/2) when cos t rounds to 1: eA = min(1/2, 2u / t^2).
           It multiplies Phi tau, |Phi tau| <= t |tau|:  the c1 term  min(1/2, 2^-23 / t^2) t |tau|  in float32, largest
           where the cosine starts to round to 1, t = 2^-12: 1.2e-4 |tau|.
           B = (t - sin t) / t^3: t - sin t is off by an ulp of t, 2 u t: eB = min(1/6, 2u / t^2), times t^2 |tau|:
           below 2^-23 |tau|, negligible by the t^2 in front.
       |sigma| >= EPS, with E = exp(sigma) known to uE = 2 u max(E, 1):
           C = (E - 1) / sigma: eC = uE / |sigma|                      (6 % at sigma = 1e-6 in float32)
           t < EPS:   A = ((sigma - 1) E + 1) / sigma^2: eA = 3 uE (1 + |sigma|) / sigma^2
                      B = (E sigma^2 / 2 + E - 1 - sigma E) / sigma^3: eB = 4 uE (1 + |sigma| + sigma^2) / |sigma|^3
           t >= EPS:  A = (a sigma + (1 - b) t) / (t c), a = E sin t, b = E cos t, c = t^2 + sigma^2: eA = 2 uE (1 + |sigma|) / c
                      B = (C - ((b - 1) sigma + a t) / c) / t^2: eB = (eC + 3 uE / sqrt(c) + 2 u max(C, 1)) / t^2
       translation error = (eC + eA t + eB t^2) |tau|.  The reference has the same formulas and thresholds (so3.h:161,
       rxso3.h:183-224, common.h:13): this zone is inherited, not a defect of the port.
 (b) the approximations the branches themselves make: C = 1 and A, B without sigma for |sigma| < EPS (dC/dsigma = 1/2,
     dA/dsigma <= 1/3, dB/dsigma <= 1/8: |sigma| (1/2 + t/3 + t^2/8) |tau|); `log` with |w| < EPS returns +-pi / n for
     (+-pi - 2 atan(w / n)) / n: 2.1 |w|.  The Taylor branches (t < EPS in exp, n^2 < EPS^2 in log) are exact to t^6.
 (c) for `log` of SE3 / Sim3 the error of phi and sigma carried into tau.

MATRIX.  An entry of R = 1 - 2 (y^2 + z^2) carries up to 15 u: 2.5 u per component of the normalised quaternion, squared
(5 u), doubled and summed (+ 2 u at magnitude 2), subtracted from 1.  So whatever goes through R or through the
equivalent sandwich product (matrix, act, act4, adj, adjT; the translations of inv and mul have |t| in front and stay
below) gets 2 BASE.

The library's host path (libm) must stay within HALF of the rounding and cancellation terms (`share` = 0.5;
tests/test_oracle_pose.py); the device gets the whole, for its own sin / cos / exp / log.  Two things are not halved,
because they are not roundings: the branch approximations (b), which host and device make alike, and the cap of the
c1 term: below t = 2^-12 the float32 cosine IS 1, the whole c1 term is lost, and the error equals min(1/2, .) t |tau|,
the issue's 1.2e-4 |tau|, on any machine.  There the host is held to the correctly rounded cosine's
min(1/2, 2^-25 / t^2) t |tau| - a quarter of the device's 2^-23 / t^2 wherever the cap is not active.
"""

import numpy as np

from . import se3

EPS = se3.EPS
GROUPS = {"SO3": 1, "RxSO3": 2, "SE3": 3, "Sim3": 4}
K = {"SO3": 3, "RxSO3": 4, "SE3": 6, "Sim3": 7}
N = {"SO3": 4, "RxSO3": 5, "SE3": 7, "Sim3": 8}
HAS_T = {"SO3": False, "RxSO3": False, "SE3": True, "Sim3": True}
HAS_S = {"SO3": False, "RxSO3": True, "SE3": False, "Sim3": True}
UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
BASE = 16.0
DEVICE, HOST = 1.0, 0.5  # `share` of the rounding and cancellation terms a path is held to (module docstring, last paragraph)


# ----------------------------------------------------------------------------- generators (moved from the Sim3 test)


def hat(group, a):
    """4 x 4 generator: Sim3 [tau, phi, sigma] -> [[Phi + sigma I, tau], [0, 0]]; SE3 without sigma, RxSO3 / SO3 without tau."""
    a = np.asarray(a, dtype=np.float64)
    tau, phi, sigma = split_tangent(group, a)
    M = np.zeros(a.shape[:-1] + (4, 4))
    M[..., :3, :3] = se3.hat(phi) + sigma[..., None, None] * np.eye(3)
    M[..., :3, 3] = tau
    return M


def vee(group, M):
    S = M[..., :3, :3]
    sigma = np.trace(S, axis1=-2, axis2=-1) / 3.0
    A = 0.5 * (S - np.swapaxes(S, -1, -2))
    phi = np.stack([A[..., 2, 1], A[..., 0, 2], A[..., 1, 0]], axis=-1)
    parts = ([M[..., :3, 3]] if HAS_T[group] else []) + [phi] + ([sigma[..., None]] if HAS_S[group] else [])
    return np.concatenate(parts, axis=-1)


def split_tangent(group, a):
    """-> tau [.., 3], phi [.., 3], sigma [..] (zeros where the group has none)"""
    o = 3 if HAS_T[group] else 0
    tau = a[..., :3] if HAS_T[group] else np.zeros(a.shape[:-1] + (3,), a.dtype)
    sigma = a[..., o + 3] if HAS_S[group] else np.zeros(a.shape[:-1], a.dtype)
    return tau, a[..., o:o + 3], sigma


def split(group, X):
    """-> t [.., 3], q [.., 4] normalised, s [..] (zeros / ones where the group has none)"""
    o = 3 if HAS_T[group] else 0
    t = X[..., :3] if HAS_T[group] else np.zeros(X.shape[:-1] + (3,), X.dtype)
    s = X[..., o + 4] if HAS_S[group] else np.ones(X.shape[:-1], X.dtype)
    return t, se3.quat_normalize(X[..., o:o + 4]), s


def join(group, t, q, s):
    parts = ([t] if HAS_T[group] else []) + [q] + ([s[..., None]] if HAS_S[group] else [])
    return np.concatenate(parts, axis=-1)


def join_tangent(group, tau, phi, sigma):
    parts = ([tau] if HAS_T[group] else []) + [phi] + ([sigma[..., None]] if HAS_S[group] else [])
    return np.concatenate(parts, axis=-1)


# ----------------------------------------------------------------------------- accurate pieces

_GL_X, _GL_W = np.polynomial.legendre.leggauss(32)
_GL_X, _GL_W = 0.5 * (_GL_X + 1.0), 0.5 * _GL_W  # on [0, 1]


def calc_w_coeffs(theta, sigma):
    """A, B, C of W = A Phi + B Phi^2 + C I = int_0^1 exp(u sigma) exp(u Phi) du, with exp(u Phi) = I + sin(u t)/t Phi +
    (1 - cos(u t))/t^2 Phi^2:  A = int e^{u s} u sinc(u t),  B = int e^{u s} u^2/2 sinc^2(u t / 2),  C = int e^{u s}.
    Entire integrands, |sigma + i t| < 6 here: the 32-point rule is exact to the last bit or two."""
    theta, sigma = np.asarray(theta, np.float64)[..., None], np.asarray(sigma, np.float64)[..., None]
    e = np.exp(_GL_X * sigma)
    A = (_GL_W * e * _GL_X * np.sinc(_GL_X * theta / np.pi)).sum(-1)
    B = (_GL_W * e * 0.5 * _GL_X ** 2 * np.sinc(0.5 * _GL_X * theta / np.pi) ** 2).sum(-1)
    C = (_GL_W * e).sum(-1)
    return A, B, C


def calc_w(phi, sigma):
    A, B, C = calc_w_coeffs(np.linalg.norm(phi, axis=-1), sigma)
    P = se3.hat(phi)
    return A[..., None, None] * P + B[..., None, None] * (P @ P) + C[..., None, None] * np.eye(3)


def so3_exp(phi):
    """[sin(t/2)/t phi, cos(t/2)] through sinc: no branch, no division by a small number."""
    t = np.linalg.norm(phi, axis=-1, keepdims=True)
    return np.concatenate([0.5 * np.sinc(0.5 * t / np.pi) * phi, np.cos(0.5 * t)], axis=-1)


def so3_log(q):
    """f v with f = 2 atan(n / w) / n of the normalised quaternion: negative for w < 0 (module docstring)."""
    q = se3.quat_normalize(q)
    v, w = q[..., :3], q[..., 3]
    n = np.linalg.norm(v, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(n > 0, 2.0 * np.arctan(n / w) / np.where(n > 0, n, 1.0), 2.0 / w)
    return f[..., None] * v


def _mv(M, v):
    return np.einsum("...ij,...j->...i", M, v)


# ----------------------------------------------------------------------------- the ops, float64


def exp(group, a, matrix_exponential=False):
    """Rotation and scale in closed form (sinc / exp), translation W tau from the quadrature, or, on request, from scipy's
    matrix exponential of hat(a)."""
    a = np.asarray(a, dtype=np.float64)
    tau, phi, sigma = split_tangent(group, a)
    t = None
    if HAS_T[group]:
        if matrix_exponential:
            import scipy.linalg
            t = scipy.linalg.expm(hat(group, a))[..., :3, 3]
        else:
            t = _mv(calc_w(phi, sigma), tau)
    return join(group, t, so3_exp(phi), np.exp(sigma))


def log(group, X):
    X = np.asarray(X, dtype=np.float64)
    t, q, s = split(group, X)
    phi, sigma = so3_log(q), np.log(s)
    tau = np.linalg.solve(calc_w(phi, sigma), t[..., None])[..., 0] if HAS_T[group] else None
    return join_tangent(group, tau, phi, sigma)


def inv(group, X):
    t, q, s = split(group, np.asarray(X, np.float64))
    qi = se3.quat_conj(q)
    return join(group, -se3.so3_act(qi, t) / s[..., None], qi, 1.0 / s)


def mul(group, X, Y):
    tx, qx, sx = split(group, np.asarray(X, np.float64))
    ty, qy, sy = split(group, np.asarray(Y, np.float64))
    return join(group, tx + sx[..., None] * se3.so3_act(qx, ty), se3.quat_normalize(se3.quat_mul(qx, qy)), sx * sy)


def matrix(group, X):
    t, q, s = split(group, np.asarray(X, np.float64))
    T = np.zeros(t.shape[:-1] + (4, 4))
    T[..., :3, :3] = s[..., None, None] * se3.so3_matrix(q)
    T[..., :3, 3] = t
    T[..., 3, 3] = 1
    return T


def act(group, X, p):
    t, q, s = split(group, np.asarray(X, np.float64))
    return s[..., None] * se3.so3_act(q, np.asarray(p, np.float64)) + t


def act4(group, X, p):
    t, q, s = split(group, np.asarray(X, np.float64))
    p = np.asarray(p, np.float64)
    return np.concatenate([s[..., None] * se3.so3_act(q, p[..., :3]) + t * p[..., 3:4], p[..., 3:4]], axis=-1)


def adj_matrix(group, X):
    """K x K adjoint: R | blockdiag(R, 1) | [[R, t^R], [0, R]] | [[sR, t^R, -t], [0, R, 0], [0, 0, 1]] (sim3.h:86-99)"""
    t, q, s = split(group, np.asarray(X, np.float64))
    R = se3.so3_matrix(q)
    k = K[group]
    A = np.zeros(t.shape[:-1] + (k, k))
    if HAS_T[group]:
        A[..., :3, :3] = s[..., None, None] * R
        A[..., :3, 3:6] = se3.hat(t) @ R
        A[..., 3:6, 3:6] = R
        if HAS_S[group]:
            A[..., :3, 6] = -t
            A[..., 6, 6] = 1
    else:
        A[..., :3, :3] = R
        if HAS_S[group]:
            A[..., 3, 3] = 1
    return A


def adj(group, X, a):
    return _mv(adj_matrix(group, X), np.asarray(a, np.float64))


def adjT(group, X, a):
    return _mv(np.swapaxes(adj_matrix(group, X), -1, -2), np.asarray(a, np.float64))


def projector(group, X):
    """d(embedding) / d(tangent), N x N with the last column zero (so3.h:72, rxso3.h:92, se3.h:107, sim3.h:77)"""
    t, q, s = split(group, np.asarray(X, np.float64))
    n, o = N[group], 3 if HAS_T[group] else 0
    P = np.zeros(t.shape[:-1] + (n, n))
    P[..., o:o + 4, o:o + 4] = se3.so3_projector(q)
    if HAS_S[group]:
        P[..., o + 4, o + 3] = s
    if HAS_T[group]:
        P[..., :3, :3] = np.eye(3)
        P[..., :3, 3:6] = se3.hat(-t)
        if HAS_S[group]:
            P[..., :3, 6] = t
    return P


def adj_generator(group, b):
    """ad(b), K x K, as `Jac<G>::adj` writes it: Phi | blockdiag(Phi, 0) | [[Phi, Tau], [0, Phi]] |
    [[Phi + sigma I, Tau, -tau], [0, Phi, 0], [0, 0, 0]] (sim3.h:122-141)"""
    b = np.asarray(b, np.float64)
    tau, phi, sigma = split_tangent(group, b)
    k = K[group]
    A = np.zeros(b.shape[:-1] + (k, k))
    P = se3.hat(phi)
    if HAS_T[group]:
        A[..., :3, :3] = P + sigma[..., None, None] * np.eye(3)
        A[..., :3, 3:6] = se3.hat(tau)
        A[..., 3:6, 3:6] = P
        if HAS_S[group]:
            A[..., :3, 6] = -tau
    else:
        A[..., :3, :3] = P
    return A


def left_jacobian(group, l):
    """SO3 / RxSO3 / SE3: the true left Jacobian int_0^1 Ad(exp(u l)) du by the 32-point rule (for SO3 this is W(phi, 0),
    for SE3 [[J, Q], [0, J]]; RxSO3 pads SO3's with a 1, rxso3.h:278-284)"""
    l = np.asarray(l, np.float64)
    if group in ("SO3", "RxSO3"):
        J = np.zeros(l.shape[:-1] + (K[group], K[group]))
        J[..., :3, :3] = calc_w(l[..., :3], np.zeros(l.shape[:-1]))
        if group == "RxSO3":
            J[..., 3, 3] = 1
        return J
    assert group == "SE3"
    return sum(w * adj_matrix(group, exp(group, x * l)) for x, w in zip(_GL_X, _GL_W))


def jinv(group, X, a):
    """b = Jl^-1(log X) a.  SO3 / RxSO3 / SE3: the inverse of the true left Jacobian (the kernels' closed forms
    I - Phi/2 + c2 Phi^2 and [[Ji, -Ji Q Ji], [0, Ji]] are exact expressions of it).  Sim3: the reference's TRUNCATED series
    I - Xi/2 + Xi^2/12 - Xi^4/720 in Xi = ad(log X), restated as written (sim3.h:176-184)."""
    l = log(group, X)
    a = np.asarray(a, np.float64)
    if group == "Sim3":
        Xi = adj_generator(group, l)
        Xi2 = Xi @ Xi
        J = np.eye(7) - Xi / 2 + Xi2 / 12 - (Xi2 @ Xi2) / 720
        return _mv(J, a)
    return np.linalg.solve(left_jacobian(group, l), a[..., None])[..., 0]


# ----------------------------------------------------------------------------- bounds


def w_coeff_errors(theta, sigma, u, share=1.0):
    """(eA, eB, eC): what the closed forms of W may lose to cancellation at unit roundoff u - module docstring, (a).
    `share` = 0.5 gives the host's part: half of every term, and for c1 the correctly rounded cosine's min(1/2, u/2 / t^2)"""
    theta, sigma = np.asarray(theta, np.float64), np.asarray(sigma, np.float64)
    tt = np.maximum(theta, 1e-30)   # the unused side of each np.where stays finite
    ss = np.maximum(np.abs(sigma), 1e-30)
    E = np.exp(sigma)
    uE = share * 2 * u * np.maximum(E, 1.0)
    # |sigma| < EPS: left_jacobian_mul
    eA0 = np.where(theta < EPS, u, np.minimum(0.5, (0.5 * u if share <= HOST else 2 * u) / tt ** 2))
    eB0 = np.where(theta < EPS, u, share * np.minimum(1.0 / 6.0, 2 * u / tt ** 2))
    eC0 = np.zeros_like(theta)
    # |sigma| >= EPS
    eC1 = uE / ss
    c = tt ** 2 + ss ** 2
    C = np.expm1(sigma) / np.where(sigma == 0, 1.0, sigma)
    eA1 = np.where(theta < EPS, 3 * uE * (1 + ss) / ss ** 2, 2 * uE * (1 + ss) / c)
    eB1 = np.where(theta < EPS, 4 * uE * (1 + ss + ss ** 2) / ss ** 3,
                   (eC1 + 3 * uE / np.sqrt(c) + share * 2 * u * np.maximum(C, 1.0)) / tt ** 2)
    small = np.abs(sigma) < EPS
    return np.where(small, eA0, eA1), np.where(small, eB0, eB1), np.where(small, eC0, eC1)


def w_error(theta, sigma, u, share=1.0, either_side=1.01):
    """||dW|| a row's translation may see: cancellation (a) + branch approximation (b).  A row within 1 % of a threshold
    is given the larger of the two sides, since float32 and float64 may evaluate the predicate differently."""
    theta, sigma = np.asarray(theta, np.float64), np.asarray(sigma, np.float64)

    def one(th, sg):
        eA, eB, eC = w_coeff_errors(th, sg, u, share)
        canc = eC + eA * theta + eB * theta ** 2
        branch = np.where(np.abs(sg) < EPS, np.abs(sigma) * (0.5 + theta / 3 + theta ** 2 / 8), 0.0)
        branch = branch + np.where(th < EPS, theta ** 3 * np.exp(np.abs(sigma)), 0.0)
        return canc + branch
    out = one(theta, sigma)
    for th in (theta / either_side, theta * either_side):
        for sg in (sigma / either_side, sigma * either_side):
            out = np.maximum(out, one(th, sg))
    return out


def _norm(x):
    return np.linalg.norm(x, axis=-1)


def log_phi_error(q, u, rot=BASE):
    """|d phi| of `log`: BASE u |phi| (relative accuracy of f and of the normalised vector part; near pi the angle moves
    by 2 |dw|) + the |w| < EPS branch's 2.1 |w|, granted up to |w| < 1.01 EPS"""
    q = se3.quat_normalize(np.asarray(q, np.float64))
    w = np.abs(q[..., 3])
    return rot * u * _norm(so3_log(q)) + np.where(w < 1.01 * EPS, 2.1 * w, 0.0)


def bound(group, op, dtype, x, y=None, share=1.0):
    """Per-row absolute bound [n] (or [n, C] where the columns differ) on |library - reference| for op(x[, y]) in `dtype`;
    x, y are the float64 casts of the inputs the library sees.  Derivation: module docstring."""
    u = UNIT[np.dtype(dtype)]
    b = share * BASE * u    # outputs that are quaternion entries, scales, or one product with them
    b2 = 2 * b              # outputs through the rotation matrix / the sandwich product: see MATRIX below
    x = np.asarray(x, np.float64)
    if op == "exp":
        tau, phi, sigma = split_tangent(group, x)
        theta = _norm(phi)
        cols = []
        if HAS_T[group]:
            A, B, C = calc_w_coeffs(theta, sigma)
            mag = (np.abs(C) + np.abs(A) * theta + np.abs(B) * theta ** 2) * _norm(tau)
            cols += [np.repeat((b * mag + w_error(theta, sigma, u, share) * _norm(tau))[:, None], 3, 1)]
        cols += [np.full(x.shape[:-1] + (4,), b)]
        if HAS_S[group]:
            cols += [(b * np.exp(sigma))[:, None]]
        return np.concatenate(cols, -1)
    t, q, s = split(group, x)
    if op == "log":
        dphi = log_phi_error(q, u, share * BASE)
        sigma = np.log(s)
        dsig = b * np.abs(sigma)
        cols = []
        if HAS_T[group]:
            phi = so3_log(q)
            theta = _norm(phi)
            W = calc_w(phi, sigma)
            winv = np.linalg.norm(np.linalg.inv(W), ord=2, axis=(-2, -1))
            wnorm = np.linalg.norm(W, ord=2, axis=(-2, -1))
            tau = _norm(np.linalg.solve(W, t[..., None])[..., 0])
            # W^-1 (dW tau): cancellation and branches (a, b), the carried error of phi and sigma (c: |dW/dphi| <= max(E, 1),
            # |dW/dsigma| <= max(E, 1)), and BASE x cond(W) for forming W, inverting it by cofactors and the product
            carried = np.maximum(s, 1.0) * (dphi + dsig)
            dt = winv * (w_error(theta, sigma, u, share) + carried) * tau + b * winv * wnorm * np.maximum(tau, winv * _norm(t))
            cols += [np.repeat(dt[:, None], 3, 1)]
        cols += [np.repeat(dphi[:, None], 3, 1)]
        if HAS_S[group]:
            cols += [dsig[:, None]]
        return np.concatenate(cols, -1)
    if op == "inv":
        cols = ([np.repeat((b * _norm(t) / s)[:, None], 3, 1)] if HAS_T[group] else []) + [np.full(x.shape[:-1] + (4,), b)]
        return np.concatenate(cols + ([(b / s)[:, None]] if HAS_S[group] else []), -1)
    if op == "mul":
        ty, _, sy = split(group, np.asarray(y, np.float64))
        cols = ([np.repeat((b * (_norm(t) + s * _norm(ty)))[:, None], 3, 1)] if HAS_T[group] else [])
        cols += [np.full(x.shape[:-1] + (4,), b)]
        return np.concatenate(cols + ([(b * s * sy)[:, None]] if HAS_S[group] else []), -1)
    y = None if y is None else np.asarray(y, np.float64)
    if op == "act":
        return b2 * (s * _norm(y) + _norm(t))
    if op == "act4":
        return b2 * (s * _norm(y[..., :3]) + np.abs(y[..., 3]) * _norm(t))
    if op in ("adj", "adjT"):
        return b2 * (np.maximum(s, 1.0) + 2 * _norm(t)) * _norm(y)
    if op == "matrix":
        return b2 * np.maximum(np.maximum(s, 1.0), _norm(t))
    if op == "vec":
        return b * np.maximum(np.maximum(s, 1.0), _norm(t))
    if op == "Jinv":
        return _jinv_bound(group, dtype, x, y, share)
    raise KeyError(op)


def _jinv_bound(group, dtype, x, a, share):
    """b = Jl^-1(l) a with l = log X.  Every group: 2 BASE u ||Jl^-1|| |a| for the products, plus what the error dl of the
    library's own `log` (its bound, column by column) does to the result.
      SO3 / RxSO3: Ji = I - Phi/2 + c2 Phi^2, c2 = (1 - t cos(t/2) / (2 sin(t/2))) / t^2.  The numerator cancels to t^2/12 and
        is off by ~3 u, c2 by 3 u / t^2 - but it multiplies Phi^2 a <= t^2 |a|: 3 u |a|, inside the base term.  ||Ji|| <= nJ =
        1 + t/2 + 0.11 t^2 (c2 <= 1/pi^2 up to pi); |dJi/dphi| <= 1/2 + t/4.  RxSO3's last component is a[3] itself: bound 0.
      SE3: top = Ji a1 - Ji Q Ji a2, bottom = Ji a2.  Q (se3_calcQ) has three coefficients that cancel, WITHOUT a small
        factor in front to save them:
          c1 = (t - sin t) / t^3            numerator off by 2 u t          times |PT + TP + PTP| <= (2 t + t^2) |tau|
          c2 = (t^2 + 2 cos t - 2) / (2 t^4)  numerator off by 6 u + u t^2 (the cosine's ulp doubled, the sum rounded at
                                              magnitude 2)                  times |PPT + TPP - 3 PTP| <= 5 t^2 |tau|
          c3 = (2t - 3 sin t + t cos t) / (2 t^5)  numerator off by 16 u t  times |PTPP + PPTP| <= 2 t^3 |tau|
        eQ = |tau| (2 u (2 + t) / t + 5 (6 u + u t^2) / (2 t^2) + 16 u / t): in float32 this is O(1) |tau| near t = 5e-4
        and grows as 1 / t^2 below, down to the Taylor threshold.  The computed numerators are quantised, so the error
        is usually far smaller, but an O(1) |tau| error does occur (t^2 + 2 rounds up by 2.4e-7 against 2 t^4 = 5e-14):
        inherited from the reference (se3.h:138-163), like the c1 zone of exp.  |Q| <= (1/2 + t/5) |tau|.
      Sim3: the truncated polynomial P(Xi) of the 7 x 7 Xi, ||Xi|| <= x = t + |sigma| + 1.5 |tau|: no cancellation;
        2 BASE u P(x) |a| with P(x) = 1 + x/2 + x^2/12 + x^4/720, and P'(x) = 1/2 + x/6 + x^3/180 times |dl|."""
    u = UNIT[np.dtype(dtype)]
    b2 = 2 * share * BASE * u
    a = np.asarray(a, np.float64)
    l = log(group, x)
    tau, phi, sigma = split_tangent(group, l)
    th = _norm(phi)
    dl = bound(group, "log", dtype, x, share=share)
    o = 3 if HAS_T[group] else 0
    dphi = dl[:, o]
    dtau = dl[:, 0] if HAS_T[group] else np.zeros_like(dphi)
    dsig = dl[:, o + 3] if HAS_S[group] else np.zeros_like(dphi)
    nJ = 1 + th / 2 + 0.11 * th ** 2
    dJ = 0.5 + th / 4
    if group in ("SO3", "RxSO3"):
        rot = (b2 * nJ + dJ * dphi) * _norm(a[:, :3])
        cols = [np.repeat(rot[:, None], 3, 1)] + ([np.zeros((len(a), 1))] if group == "RxSO3" else [])
        return np.concatenate(cols, -1)
    if group == "SE3":
        a1, a2, nt = _norm(a[:, :3]), _norm(a[:, 3:]), _norm(tau)
        tt = np.maximum(th, 1e-30)
        eQ = np.where(th < EPS, u, share * nt * (2 * u * (2 + tt) / tt + 5 * (6 * u + u * tt ** 2) / (2 * tt ** 2) + 16 * u / tt))
        nQ = (0.5 + th / 5) * nt
        top = (b2 * nJ + dJ * dphi) * a1 + nJ ** 2 * (b2 * nQ + eQ + (0.5 + th / 5) * dtau + (1 + th) * nt * dphi) * a2 \
            + 2 * nJ * dJ * dphi * nQ * a2
        bot = (b2 * nJ + dJ * dphi) * a2
        return np.concatenate([np.repeat(top[:, None], 3, 1), np.repeat(bot[:, None], 3, 1)], -1)
    xx = th + np.abs(sigma) + 1.5 * _norm(tau)
    P = 1 + xx / 2 + xx ** 2 / 12 + xx ** 4 / 720
    dP = 0.5 + xx / 6 + xx ** 3 / 180
    return (b2 * P + dP * (dtau + dphi + dsig)) * _norm(a)
