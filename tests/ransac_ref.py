"""Float64 reference for the RANSAC affine refit, and the scenes the refit tests share (tests/test_oracle_ransac.py, tests/test_gpu_ransac.py).

The product and the oracle refit the best hypothesis' inliers with fixed-point sums; this module fits the same inliers with np.linalg.lstsq in float64
and bounds how far the two may be apart from the float64 problem alone (refit_tol)."""
import numpy as np

EPS = np.finfo(np.float64).eps
QUANT = 2.0 ** -21  # each second-moment term is rounded to a multiple of 2^-20: at most 2^-21 off


def lstsq_ref(src, dst, inl):
    """(M_ref 2x3, det / tr^2 of the centred 2x2 moment matrix) of the float64 least-squares affine on the inliers, fitted to centred data on both
    sides: with |dst| ~ 1e5 an uncentred right-hand side alone costs lstsq ~3e-7 px."""
    P = src[inl].astype(np.float64)
    Q = dst[inl].astype(np.float64)
    c, d = P.mean(0), Q.mean(0)
    X = P - c
    Z = np.linalg.lstsq(X, Q - d, rcond=None)[0]  # (the least-squares plane passes through the centroids)
    M = np.empty((2, 3))
    M[:, :2] = Z.T
    M[:, 2] = d - M[:, :2] @ c
    S = X.T @ X
    return M, np.linalg.det(S) / np.trace(S) ** 2


def pred_err(M, M_ref, src, inl):
    """max over the inliers of |M p - M_ref p| (px), evaluated in the centred form so the evaluation itself adds no rounding of size |p|."""
    P = src[inl].astype(np.float64)
    c = P.mean(0)
    X = P - c
    D = M - M_ref
    return float(np.abs(X @ D[:, :2].T + (D[:, :2] @ c + D[:, 2])).max())


def refit_tol(src, dst, inl, M_ref):
    """Bound on pred_err between the fixed-point refit and the float64 fit, from the float64 problem.

    The refit solves the 2x2 normal equations S z = s of the centred inliers.  Each of the n terms of every moment is rounded to within 2^-21, so
    every entry of S and s is off by at most eta = n 2^-21, and |dz| <= |S^-1| (|ds| + |dS| |z|) <= 2 eta (1 + |z|) / lambda_min(S).  A prediction
    on the inliers moves by at most R |dz| (R: largest centred radius).  Rounding of the means, the solve and the intercept adds a few ulps of the
    largest term |M| |p|, and the float64 fit itself is good to kappa(S) eps.  Twice the sum of these is the tolerance."""
    P = src[inl].astype(np.float64)
    n = len(P)
    X = P - P.mean(0)
    S = X.T @ X
    lam = np.linalg.eigvalsh(S)
    R = float(np.sqrt((X ** 2).sum(1)).max())
    eta = n * QUANT + 8 * EPS * lam[1]
    tol = 0.0
    for r in range(2):
        z = float(np.linalg.norm(M_ref[r, :2]))
        big = float(np.abs(M_ref[r, :2]) @ np.abs(P).max(0) + abs(M_ref[r, 2]))
        tol = max(tol, R * 2 * eta * (1 + z) / lam[0] + 16 * EPS * big + 8 * R * (1 + z) * EPS * lam[1] / lam[0])
    return 2 * tol


def affine_scene(rng, m, ratio, box, noise=0.2, A=None):
    """m pairs in box = (x0, x1, y0, y1): a fraction `ratio` follows the affine A (+ Gaussian noise), the rest are moved 20-80 px away."""
    x0, x1, y0, y1 = box
    src = np.c_[rng.uniform(x0, x1, m), rng.uniform(y0, y1, m)]
    A = np.array([[0.999, -0.012, 3.5], [0.011, 1.002, -2.25]]) if A is None else A
    dst = src @ A[:, :2].T + A[:, 2] + rng.normal(0, noise, (m, 2))
    bad = rng.permutation(m)[: int(round(m * (1 - ratio)))]
    dst[bad] += rng.uniform(20, 80, (len(bad), 2)) * rng.choice([-1, 1], (len(bad), 2))
    return src.astype(np.float32), dst.astype(np.float32)


def refit_scenes():
    """(name, src, dst, float64 checks must hold) -- pixel-scale frames up to 8K, tight clusters, 20 000 pairs, a 1000-px box far from the origin."""
    rng = np.random.default_rng(2026)
    out = []
    for W, H in ((1920, 1080), (3840, 2160), (7680, 4320)):
        out.append((f"frame {W}x{H}", *affine_scene(rng, 1500, 0.7, (0, W, 0, H), noise=0.3)))
    for spread in (1.0, 2.0, 4.0):
        for m in (3, 10, 64):
            c = rng.uniform(100, 1800, 2)
            out.append((f"cluster {spread} px m={m}", *affine_scene(rng, m, 1.0, (c[0], c[0] + spread, c[1], c[1] + spread), noise=0.01)))
    out.append(("frame 1920x1080 m=20000", *affine_scene(rng, 20000, 0.8, (0, 1920, 0, 1080), noise=0.3)))
    for off in (1e5, 1e6):
        for m in (3072, 20000):
            out.append((f"1000-px box at {off:g} m={m}", *affine_scene(rng, m, 0.8, (off, off + 1000, off, off + 1000), noise=0.3)))
    return out


def check_refit(name, src, dst, M, inl):
    """The refit on the returned inliers against the float64 fit: within refit_tol, or -- where the centred moments are degenerate (det <= 1e-9
    tr^2) -- the hypothesis model kept: three of the inliers mapped exactly.  Returns (error, tolerance) for the report."""
    assert M is not None, name
    M_ref, ratio = lstsq_ref(src, dst, inl)
    if ratio <= 0.5e-9:
        P, Q = src[inl].astype(np.float64), dst[inl].astype(np.float64)
        exact = np.abs(P @ M[:, :2].T + M[:, 2] - Q).max(1) <= 64 * EPS * (1 + np.abs(Q).max())
        assert exact.sum() >= 3, (name, "degenerate moments: the hypothesis model must be kept")
        return 0.0, 0.0
    assert ratio >= 2e-9, (name, "scene too close to the degeneracy threshold to judge", ratio)
    err, tol = pred_err(M, M_ref, src, inl), refit_tol(src, dst, inl, M_ref)
    assert err <= tol, f"{name}: refit differs from the float64 fit by {err:.3g} px on its inliers (bound {tol:.3g} px)"
    return err, tol


def threshold_scene():
    """Integer pairs under identity + (5, -3) (every 3-point hypothesis of them is exact), and pairs near the origin whose residual is exactly 3 px or
    lands next to 9 after the float32 rounding of the squared residual.  Returns (src, dst, expected inlier mask)."""
    rng = np.random.default_rng(17)
    t = np.array([5.0, -3.0])
    g = np.stack(np.meshgrid(np.arange(10, 1000, 60), np.arange(10, 700, 50)), -1).reshape(-1, 2).astype(np.float64)
    src = [g]
    dst = [g + t]
    nine = np.float32(9.0)
    lo, hi = np.nextafter(nine, np.float32(0)), np.nextafter(nine, np.float32(20))
    cases = []
    for p in ((0.5, 0.25), (1.0, 1.5), (0.25, 2.0), (1.75, 0.5), (2.5, 2.5), (0.75, 3.0)):
        q = np.array(p) + t
        ux = np.float32(q[0] + 3.0)
        cases += [(p, (q[0] + 3.0, q[1])), (p, (q[0], q[1] + 3.0)), (p, (q[0] + 3.0, q[1] + 2.0 ** -12))]  # 9; 9; above 9, float32 9
        for j in (-1, 0):  # x residual 3 px or one float32 step below it, then a y residual that lands on each neighbour of 9
            xj = float(np.nextafter(ux, np.float32(0))) if j else float(ux)
            ex = xj - q[0]
            for want in (np.nextafter(lo, np.float32(0)), lo, nine, hi, np.nextafter(hi, np.float32(20))):
                y = _dst_y(q[1], ex, want)
                if y is not None:
                    cases.append((p, (xj, y)))
    P = np.array([c[0] for c in cases], np.float64)
    Q = np.array([c[1] for c in cases], np.float64)
    src.append(P)
    dst.append(Q)
    src = np.concatenate(src).astype(np.float32)
    dst = np.concatenate(dst).astype(np.float32)
    e = dst.astype(np.float64) - (src.astype(np.float64) + t)
    e2 = np.float32(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
    exp = e2 <= nine
    # the scene reaches every side of the threshold: exactly 9, above 9 in float64 yet 9 in float32, and both float32 neighbours of 9
    d2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
    assert (d2 == 9.0).any() and ((d2 > 9.0) & (e2 == nine)).any() and (e2 == lo).any() and (e2 == hi).any()
    perm = rng.permutation(len(src))
    return src[perm], dst[perm], exp[perm]


def _dst_y(qy, ex, want):
    """A float32 y above qy whose residual ey puts float32(ex^2 + ey^2) exactly on `want` (None if no float32 y near the target does)."""
    y0 = np.float32(qy + np.sqrt(max(float(want) - ex * ex, 0.0)))
    for k in range(-64, 65):
        y = float(np.float32(y0 + np.float32(k) * np.spacing(y0)))
        ey = y - qy
        if ey >= 0 and np.float32(ex * ex + ey * ey) == want:
            return y
    return None
