"""NumPy model of the refinement of a frame window with tracks that live through PART of it (vh_session_refine_windows_partial,
TrackerSession.refine_windows(min_obs=...)): THE definition the device is held to.  Built on oracle.nls_oracle.ba_schur_solve(bad=), pixel_to_uvec,
two_view_intercept, project_cam and tests/refine_window_ref.py::window_inputs (anchors: tests/anchor_ref.py).  Checker only: the product never imports it.

Window (slot, first) of nf frames, i = the slot's frame counter, msv = the session's MSV frame.  obs(g) = the frames of the window in which row 4 of g's
history is finite.  A track g takes part iff it is
  A  observed in all nf frames (and, in a replenished session, tri[g]): today's rule (tests/refine_window_ref.py::window_ids); or
  B  obs(g) >= min_obs and the session has established p3[g]: row 2 of the history finite in some frame 0..i (the pose solve's projection: written only
     while g is a pose track), or 0 <= msv <= i and g alive at frame msv (fcnMSV1_t re-triangulated it), or g anchored; or
  C  (start_reproj > 0) neither, obs(g) >= min_obs, and the point triangulated from its first and last observed frame of the window -- the arithmetic of
     tests/replenish_ref.py::ReplenishOracle.triangulate on that one pair -- is finite, in front of both cameras and reprojects within start_reproj
     pixels in both; a C candidate that fails counts as rejected."""
import numpy as np

import anchor_ref as AR
import refine_ref as RR
import refine_window_ref as RW
from oracle import nls_oracle as O


def two_view_start(K, P, B, g, fa, fb):
    """The session-frame point of track g from its observations in frames fa < fb, and the larger of its two reprojection errors (inf where the point
    is not finite or lies behind a camera).  K as the session holds it (float32: the rays are formed in float32, as numpy would); B float32."""
    fr = [int(fa), int(fb)]
    U = np.zeros((3, 2, 1))
    for j, f in enumerate(fr):
        U[:, j] = O.pixel_to_uvec(K, P[0:2, [g], f].T).T  # as fcnMSV1_t builds them (MSV.py:15-17)
    A = (B[0, 0:3] - B[fr, 0:3]).astype(np.float64)  # float32 difference, then widened (MSV.py:18)
    with np.errstate(all="ignore"):
        c = O.two_view_intercept(A, U)[0]
        ok = bool(np.isfinite(c).all())
        err = 0.0
        K64 = np.asarray(K, np.float64)
        for f in fr:
            cam = c + B[f, 3:6].astype(np.float64)
            ok = ok and cam[2] > 0
            d = O.project_cam(cam[None], K64)[0] - P[0:2, g, f].astype(np.float64)
            err = max(err, float(np.sqrt((d * d).sum())))
    return c, (err if ok and np.isfinite(err) else np.inf)


def select_partial(K, P, B, first, nf, i, msv, min_obs, start_reproj=0.0, anchored=None, tri=None):
    """The tracks of the window and why.  anchored: bool mask over the N0 ids or None; tri: the replenishment's flags or None (no replenishment).
    -> dict(ids ascending, kind [N0] of "A" / "B" / "C" / "r" (rejected C candidate) / "" (not in the window), obs [N0], start [N0, 3] (rows of kind
    C: the triangulated point, session coordinates), err [N0] (C candidates: the gate's error), nobs, npart, ntri, nrej)."""
    P, B = np.asarray(P), np.asarray(B, np.float32)
    N0, nh = P.shape[1], P.shape[2]
    assert 2 <= min_obs <= nf and first >= 0 and first + nf <= nh and start_reproj >= 0
    seen = np.isfinite(P[4, :, first:first + nf])
    obs = seen.sum(1)
    a = obs == nf
    if tri is not None:
        a &= np.asarray(tri).astype(bool)
    i = min(int(i), nh - 1)
    trusted = np.isfinite(P[2, :, :i + 1]).any(1)
    if 0 <= msv <= i:
        trusted |= np.isfinite(P[4, :, msv])
    if anchored is not None:
        trusted |= np.asarray(anchored, bool)
    enough = obs >= min_obs
    b = ~a & enough & trusted
    kind = np.full(N0, "", dtype="<U1")
    kind[a], kind[b] = "A", "B"
    start, err = np.zeros((N0, 3)), np.full(N0, np.nan)
    if start_reproj > 0:
        for g in np.flatnonzero(~a & ~b & enough):
            at = np.flatnonzero(seen[g])
            start[g], err[g] = two_view_start(K, P, B, g, first + at[0], first + at[-1])
            kind[g] = "C" if err[g] < start_reproj else "r"
    took = np.isin(kind, ("A", "B", "C"))
    return dict(ids=np.flatnonzero(took).astype(np.int32), kind=kind, obs=obs, start=start, err=err, nobs=int(obs[took].sum()),
                npart=int((took & (obs < nf)).sum()), ntri=int((kind == "C").sum()), nrej=int((kind == "r").sum()))


def pack_partial(Pw, pw0, Bw, ids):
    """z, bad and x0 of the window's tracks `ids` (oracle.ba_pack's layout and zeroing): history rows 0/1, no observation wherever row 4 is NaN."""
    nf = Pw.shape[2]
    uv = np.where(np.isfinite(Pw[4, ids])[None], Pw[0:2][:, ids], np.nan)
    z = np.concatenate([uv[0].T.reshape(-1), uv[1].T.reshape(-1)]).astype(float)
    bad = np.isnan(z)
    z[bad] = 0
    cw0 = Bw[:nf, 3:6].astype(np.float64)
    x = np.concatenate((pw0[ids], cw0[1:], np.zeros((nf - 1, 3)))).reshape(-1).astype(float)
    return z, bad, x, cw0


def refine_partial_ref(K, P, p3, B, first, nf, i, msv, min_obs, start_reproj=0.0, anchors=None, tri=None, max_iter=10):
    """The window's record: refine_window_ref's keys (cw and pw in the window's coordinates), nfix, nobs, npart, ntri, nrej, and `sel`
    (select_partial's dict), `z` / `bad` as solved.  anchors: (ids, xyz) of the slot or None."""
    p3a, amask = AR.anchored_inputs(p3, anchors)
    sel = select_partial(K, P, B, first, nf, i, msv, min_obs, start_reproj, amask if amask.any() else None, tri)
    c = sel["kind"] == "C"
    p3a[c] = sel["start"][c]
    Pw, pw0, Bw = RW.window_inputs(P, p3a, B, first, nf)
    ids = sel["ids"]
    nt, nc = len(ids), nf - 1
    z, bad, x0, cw0 = pack_partial(Pw, pw0, Bw, ids)
    fixed = amask[ids]
    out = {"nt": nt, "ids": ids, "first": first, "nfix": int(fixed.sum()), "sel": sel, "z": z, "bad": bad}
    out.update({k: sel[k] for k in ("nobs", "npart", "ntri", "nrej")})
    if nt == 0:  # not solved
        out.update(cw=cw0, pw=np.zeros((0, 3)), iterations=0, converged=0, trace=np.zeros((0, 2)))
    else:
        K64 = np.asarray(K).astype(float)
        if fixed.any():
            x, trace = AR.solve_anchored(K64, z, bad, x0, nt, nt, nc, fixed=fixed, max_iter=max_iter)
        else:
            x, trace = O.ba_schur_solve(K64, z, x0, nt, nc, max_iter, bad=bad)
        j = 3 * nt
        out.update(cw=np.concatenate((np.zeros((1, 3)), x[j:j + 3 * nc].reshape(nc, 3)), 0), pw=x[:j].reshape(nt, 3), iterations=len(trace),
                   converged=int(trace[-1, 1] < 1e-7), trace=np.asarray(trace))
    out.update(RR.speed_of(out["cw"], Bw[:nf, 12]))
    tr = out["trace"]
    out.update(f_first=tr[0, 0] if len(tr) else np.nan, f_last=tr[-1, 0] if len(tr) else np.nan)
    return out


# ---- analytic windows with tracks that live through part of them: the truth experiment -----------------------------------------------------------------
def analytic_window(seed, nf=8, n_full=6, n_part=34, noise=0.1):
    """A window of nf frames of a camera moving along +z with a little drift: n_full tracks seen in every frame, n_part seen in a random run of 2..nf-1
    consecutive frames, pixels with `noise` px of Gaussian noise; starts: the true points and cameras, perturbed (1 % / 2 %).
    -> (K, P [5, n, nf] float64 with NaN where unobserved, pw0 [n, 3], cw0 [nf, 3], cw_true [nf, 3])."""
    rng = np.random.default_rng(seed)
    K = np.array([[900.0, 0, 0], [0, 900.0, 0], [640.0, 360.0, 1]])
    n = n_full + n_part
    pw = np.column_stack([rng.uniform(-4, 4, n), rng.uniform(-2.5, 2.5, n), rng.uniform(10, 25, n)])
    step = np.column_stack([rng.normal(0, 0.02, nf - 1), rng.normal(0, 0.02, nf - 1), rng.uniform(0.35, 0.55, nf - 1)])
    cw = np.concatenate((np.zeros((1, 3)), np.cumsum(-step, 0)))  # camera-frame point = pw + cw[f]: the camera advances, the points come closer
    P = np.full((5, n, nf), np.nan)
    for g in range(n):
        if g < n_full:
            lo, hi = 0, nf
        else:
            life = int(rng.integers(2, nf))
            lo = int(rng.integers(0, nf - life + 1))
            hi = lo + life
        for f in range(lo, hi):
            uv = O.project_cam((pw[g] + cw[f])[None], K)[0] + rng.normal(0, noise, 2)
            P[0, g, f], P[1, g, f], P[4, g, f] = uv[0], uv[1], f
    pw0 = pw * (1 + rng.normal(0, 0.01, (n, 1)))
    cw0 = cw * (1 + rng.normal(0, 0.02, (nf, 1)))
    return K, P, pw0, cw0, cw


def step_error(cw, cw_true):
    """The worst relative error of the per-step displacements, scale-free: both step-length profiles are normalised by their own mean first."""
    d = np.sqrt((np.diff(cw, axis=0) ** 2).sum(1))
    t = np.sqrt((np.diff(cw_true, axis=0) ** 2).sum(1))
    return float(np.abs(d / d.mean() - t / t.mean()).max())


def solve_analytic(K, P, pw0, cw0, min_obs, max_iter=10):
    """ba_schur_solve(bad=) on the tracks observed in at least min_obs frames -> cw [nf, 3]."""
    nf = P.shape[2]
    ids = np.flatnonzero(np.isfinite(P[4]).sum(1) >= min_obs)
    B = np.zeros((nf, 14))
    B[:, 3:6] = cw0
    z, bad, x0, _ = pack_partial(P, pw0, B, ids)
    x, _ = O.ba_schur_solve(K, z, x0, len(ids), nf - 1, max_iter, bad=bad)
    return np.concatenate((np.zeros((1, 3)), x[3 * len(ids):3 * len(ids) + 3 * (nf - 1)].reshape(nf - 1, 3)), 0), len(ids)
