"""NumPy model of bundle adjustment with Huber weights (vh_nls_batch_windows_robust, vh_session_set_refine_robust): the step of
tests/anchor_ref.py::anchored_step with every measurement pair whose reprojection error exceeds `delta` pixels scaled by sqrt(delta / |r|), the LM loop
around it, the dense form it is pinned to, and the outlier experiment behind profiles/ba_robust/truth.json.  Checker only: the product never imports it."""
import math

import numpy as np

from oracle import nls_oracle as O


def huber_sqrt_weights(r, delta):
    """r [nf, nt, 2] residual pairs -> (sqrt(w) [nf, nt], down [nf, nt] bool): s2 = ru^2 + rv^2; s2 > delta^2: w = delta / sqrt(s2), else 1."""
    s2 = r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]
    down = s2 > delta * delta
    sw = np.ones_like(s2)
    sw[down] = np.sqrt(delta / np.sqrt(s2[down]))
    return sw, down


def robust_step(x, z, K, nc, nt, fixed=None, gain=0.9, bad=None, delta=None, margin=None):
    """anchor_ref.anchored_step, operation for operation (delta None: its bits), with the Huber scaling applied to r, Jp and Jc after the NaN and the
    anchor rules and before anything else reads them.  The returned rms residual is the UNWEIGHTED one.  -> (step, rms residual, down-weighted count).
    margin: a list that receives min |s2 / delta^2 - 1| over the observed measurements (how near the state came to the threshold), or None."""
    nf, nq = nc + 1, 6 * nc
    uv, Jp, Jc = O.ba_compact_jacobian(x, K, nc, nt)
    zu = z[: nf * nt].reshape(nf, nt)
    zv = z[nf * nt:].reshape(nf, nt)
    r = np.stack([zu - uv[..., 0], zv - uv[..., 1]], -1)
    if bad is not None and bad.any():
        mb = (bad[: nf * nt] | bad[nf * nt:]).reshape(nf, nt)
        r[mb] = 0.0
        Jp = Jp.copy(); Jc = Jc.copy()
        Jp[mb] = 0.0
        Jc[mb] = 0.0
    if fixed is not None and np.any(fixed):
        Jp = Jp.copy()
        Jp[:, np.asarray(fixed, bool)] = 0.0
    f = math.sqrt((r * r).sum() / z.size)
    nout = 0
    if delta is not None and delta > 0:
        sw, down = huber_sqrt_weights(r, float(delta))
        nout = int(down.sum())
        if margin is not None:
            s2 = (r * r).sum(-1)
            margin.append(float(np.abs(s2[s2 > 0] / (delta * delta) - 1.0).min()) if (s2 > 0).any() else np.inf)
        r = r * sw[..., None]
        Jp = Jp * sw[..., None, None]
        Jc = Jc * sw[..., None, None]
    U = np.einsum("cima,cimb->iab", Jp, Jp) + np.eye(3)
    gp = np.einsum("cima,cim->ia", Jp, r)
    Ui = np.linalg.inv(U)
    W = np.einsum("cima,cimk->iack", Jp[1:], Jc[1:]).reshape(nt, 3, nq)
    V = np.einsum("cimk,ciml->ckl", Jc[1:], Jc[1:])
    gc = np.einsum("cimk,cim->ck", Jc[1:], r[1:]).reshape(nq)
    Y = Ui @ W
    tp = np.einsum("iab,ib->ia", Ui, gp)
    S = np.eye(nq) - np.einsum("iak,ial->kl", W, Y)
    for c in range(nc):
        S[6 * c: 6 * c + 6, 6 * c: 6 * c + 6] += V[c]
    rhs = gc - np.einsum("iak,ia->k", W, tp)
    dc = np.linalg.solve(S, rhs)
    dp = tp - Y @ dc
    dcm = dc.reshape(nc, 6)
    step = np.concatenate([dp.reshape(-1), dcm[:, :3].reshape(-1), dcm[:, 3:].reshape(-1)]) * gain
    return step, f, nout


def dense_robust_step(x, z, K, nc, nt, fixed, delta, gain=0.9):
    """inv(J^T W J + I) J^T W r * gain with the dense forward-difference J of O.ba_jacobian_fd, the anchors' columns zeroed and W the Huber weights of
    the measurement pairs (both rows of a pair share one weight)."""
    nf = nc + 1
    zhat = O.ba_predict(x, K, nc, nt)
    JT = O.ba_jacobian_fd(x, K, nc, nt, zhat)
    rows = np.flatnonzero(np.repeat(np.asarray(fixed, bool), 3))
    JT[rows] = 0.0
    r = z - zhat
    s2 = r[: nf * nt] ** 2 + r[nf * nt:] ** 2
    w = np.ones(nf * nt)
    down = s2 > delta * delta
    w[down] = delta / np.sqrt(s2[down])
    w2 = np.concatenate((w, w))
    return np.linalg.solve((JT * w2) @ JT.T + np.eye(x.size), (JT * w2) @ r) * gain


def solve_robust(K, z, bad, x, nt_true, nt_pad, nc, fixed=None, max_iter=10, delta=None, margin=None):
    """anchor_ref.solve_anchored with the weights (delta None: its bits) -> (x, trace, nout [iterations])."""
    x = x.copy()
    nx, nz = 3 * nt_true + 6 * nc, 2 * nt_true * (nc + 1)
    trace, nout = [], []
    for _ in range(max_iter):
        step, f, n = robust_step(x, z, K, nc, nt_pad, fixed=fixed, bad=bad, delta=delta, margin=margin)
        x = x + step
        xr = np.sqrt((step * step).sum() / nx)
        trace.append((f * np.sqrt(z.size / nz), xr))
        nout.append(n)
        if xr < 1e-7:
            break
    return x, np.array(trace), np.array(nout, np.int32)


# ---- the outlier experiment ---------------------------------------------------------------------------------------------------------------------------------
def move_measurements(P, fraction=None, count=None, seed=0, lo=5.0, hi=40.0):
    """A copy of the history P [5, nt, nf] with some of its (track, frame > 0) measurements moved by +-U(lo, hi) pixels in each coordinate, drawn with
    default_rng(seed): each of the nt (nf - 1) with probability `fraction` (at least one), or exactly `count` of them chosen without replacement.
    -> (P, moved [n, 2] = (track, frame))."""
    P = np.array(P, copy=True)
    _, nt, nf = P.shape
    rng = np.random.default_rng(seed)
    m = nt * (nf - 1)
    if count is not None:
        pick = np.sort(rng.choice(m, int(count), replace=False))
    else:
        pick = np.flatnonzero(rng.random(m) < fraction)
        if not len(pick):
            pick = rng.choice(m, 1)
    n = len(pick)
    tr, fr = pick // (nf - 1), 1 + pick % (nf - 1)
    shift = rng.uniform(lo, hi, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    P[0, tr, fr] += shift[:, 0].astype(P.dtype)
    P[1, tr, fr] += shift[:, 1].astype(P.dtype)
    return P, np.stack([tr, fr], 1)


def step_error(x, nt, nc, step_true=(0.05, 0.0, 0.37)):
    """Worst relative error of the length of a camera step of the state x -- a speed, once divided by the frame time -- against the truth's
    (synth.ba_scene moves its camera by step_true per frame)."""
    cams = np.concatenate((np.zeros((1, 3)), x[3 * nt: 3 * nt + 3 * nc].reshape(nc, 3)))
    d = np.linalg.norm(np.diff(cams, axis=0), axis=1) / np.linalg.norm(step_true)
    return float(np.abs(d - 1.0).max())


def outlier_problem(nt, nf, seed, fraction):
    """synth.ba_scene(nt, nf, seed) from its own start with `fraction` of its measurements moved (rng 100 + seed) -> (K, z, x0, nt, nc, number moved)."""
    from velocity_amd import synth

    K = np.asarray(synth.K_1080P, np.float64)
    P, pw, cw = synth.ba_scene(nt, nf, seed=seed)
    moved = np.zeros((0, 2), int)
    if fraction > 0:
        P, moved = move_measurements(P, fraction, seed=100 + seed)
    z, x0, nt, nc = synth.ba_pack(P, pw, cw)
    return K, z, x0, nt, nc, len(moved)


def truth_table(cases=((40, 6, 0.0), (40, 6, 0.03), (40, 6, 0.10), (64, 8, 0.03), (64, 8, 0.10)), seeds=range(8), deltas=(None, 1.0, 0.5), max_iter=10):
    """The experiment of the README's claim: per case and loss the worst camera-step error of every seed, and the last count against the number moved."""
    rows = []
    for nt, nf, frac in cases:
        row = {"nt": nt, "nf": nf, "fraction": frac, "moved": [], "loss": {}}
        for d in deltas:
            errs, last = [], []
            for s in seeds:
                K, z, x0, n, nc, nm = outlier_problem(nt, nf, s, frac)
                x, _, nout = solve_robust(K, z, np.zeros(z.size, bool), x0, n, n, nc, max_iter=max_iter, delta=d)
                errs.append(step_error(x, n, nc))
                last.append(int(nout[-1]))
                if d is None:
                    row["moved"].append(nm)
            row["loss"]["plain" if d is None else f"huber {d:g} px"] = {"step_error": errs, "median": float(np.median(errs)), "max": float(np.max(errs)),
                                                                       "nout_last": last}
        rows.append(row)
    return rows


# ---- the session's refinements with the setting on (vh_session_set_refine_robust) ---------------------------------------------------------------------------
def _refine(K, P, p3, B, n, anchors, delta, max_iter, margin=None):
    """anchor_ref._refine with the weights: its packing on the anchors' points, the solve solve_robust; adds nout_first, nout_last, robust."""
    import anchor_ref as AR
    import refine_ref as RR

    p3a, mask = AR.anchored_inputs(p3, anchors)
    seen = {}

    def solver(K_, P_, pw_, cw_, max_iter=10, return_info=True):
        z, bad, x, nt, nc = O.ba_pack(K_, P_, pw_, cw_)
        keep = np.isfinite(P_[4]).sum(1) == P_.shape[2]
        fixed = mask[keep]
        x, trace, nout = solve_robust(np.asarray(K_, np.float64), z, bad, x, nt, nt, nc, fixed=fixed, max_iter=max_iter, delta=delta, margin=margin)
        seen.update(nfix=int(fixed.sum()), nout=nout)
        j = 3 * nt
        return np.concatenate((np.zeros((1, 3)), x[j: j + 3 * nc].reshape(nc, 3)), 0), x[:j].reshape(nt, 3), x, trace

    out = RR.refine_ref(K, P, p3a, B, n, max_iter=max_iter, solver=solver)
    nout = seen.get("nout", np.zeros(0, np.int32))
    out.update(nfix=seen.get("nfix", 0), robust=float(delta), nout_first=int(nout[0]) if len(nout) else 0, nout_last=int(nout[-1]) if len(nout) else 0)
    return out


def refine_robust_ref(K, P, p3, B, n, delta, anchors=None, max_iter=10, margin=None):
    """The whole clip (vh_session_refine) of a session that refines with Huber weights, with the slot's anchors (ids, xyz) or None."""
    out = _refine(K, P, p3, B, n, anchors, delta, max_iter, margin)
    tr = out["trace"]
    out.update(f_first=tr[0, 0] if len(tr) else np.nan, f_last=tr[-1, 0] if len(tr) else np.nan)
    return out


def refine_window_robust_ref(K, P, p3, B, first, nf, delta, anchors=None, max_iter=10, margin=None):
    """Window [first, first + nf) (vh_session_refine_windows): anchor_ref.refine_window_anchored_ref with the weights."""
    import anchor_ref as AR
    import refine_window_ref as RW

    p3a, _ = AR.anchored_inputs(p3, anchors)
    Pw, pw0, Bw = RW.window_inputs(P, p3a, B, first, nf)
    shifted = None if anchors is None or not len(anchors[0]) else (anchors[0], pw0[np.asarray(anchors[0], np.int64)])
    out = _refine(K, Pw, pw0, Bw, nf, shifted, delta, max_iter, margin)
    tr = out["trace"]
    out.update(first=first, f_first=tr[0, 0] if len(tr) else np.nan, f_last=tr[-1, 0] if len(tr) else np.nan)
    return out


def refine_partial_robust_ref(K, P, p3, B, first, nf, i, msv, min_obs, delta, start_reproj=0.0, anchors=None, max_iter=10, margin=None):
    """Window [first, first + nf) with tracks that live through part of it (vh_session_refine_windows_partial): refine_partial_ref.refine_partial_ref's
    selection, packing and record, the solve solve_robust."""
    import anchor_ref as AR
    import refine_partial_ref as RP
    import refine_ref as RR
    import refine_window_ref as RW

    p3a, amask = AR.anchored_inputs(p3, anchors)
    sel = RP.select_partial(K, P, B, first, nf, i, msv, min_obs, start_reproj, amask if amask.any() else None, None)
    c = sel["kind"] == "C"
    p3a[c] = sel["start"][c]
    Pw, pw0, Bw = RW.window_inputs(P, p3a, B, first, nf)
    ids = sel["ids"]
    nt, nc = len(ids), nf - 1
    z, bad, x0, cw0 = RP.pack_partial(Pw, pw0, Bw, ids)
    fixed = amask[ids]
    out = {"nt": nt, "ids": ids, "first": first, "nfix": int(fixed.sum()), "robust": float(delta), "nout_first": 0, "nout_last": 0}
    out.update({k: sel[k] for k in ("nobs", "npart", "ntri", "nrej")})
    if nt == 0:  # not solved
        out.update(cw=cw0, pw=np.zeros((0, 3)), iterations=0, converged=0, trace=np.zeros((0, 2)))
    else:
        x, trace, nout = solve_robust(np.asarray(K).astype(float), z, bad, x0, nt, nt, nc, fixed=fixed, max_iter=max_iter, delta=delta, margin=margin)
        j = 3 * nt
        out.update(cw=np.concatenate((np.zeros((1, 3)), x[j:j + 3 * nc].reshape(nc, 3)), 0), pw=x[:j].reshape(nt, 3), iterations=len(trace),
                   converged=int(trace[-1, 1] < 1e-7), trace=np.asarray(trace), nout_first=int(nout[0]), nout_last=int(nout[-1]))
    out.update(RR.speed_of(out["cw"], Bw[:nf, 12]))
    tr = out["trace"]
    out.update(f_first=tr[0, 0] if len(tr) else np.nan, f_last=tr[-1, 0] if len(tr) else np.nan)
    return out
