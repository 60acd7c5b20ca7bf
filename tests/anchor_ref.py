"""NumPy model of bundle adjustment with anchored (fixed) points (vh_nls_batch_windows_fixed, vh_session_set_anchors): the step of
oracle.nls_oracle.ba_schur_step with the three Jacobian columns of every anchored point zeroed, the LM loop on a padded window, the dense solve it is
pinned to, the scale experiment, and the session's packing with anchors on top of tests/refine_ref.py / tests/refine_window_ref.py.  Checker only:
the product never imports it."""
import math

import numpy as np

import refine_ref as RR
import refine_window_ref as RW
from oracle import nls_oracle as O


def anchored_step(x, z, K, nc, nt, fixed=None, gain=0.9, bad=None):
    """O.ba_schur_step -- its arithmetic restated operation for operation, so an empty mask gives its bits -- with Jp of the rows `fixed` (bool [nt])
    zeroed: U_i + I = I, tp_i = 0, W_i = 0, so delta of those rows is exactly 0 and they subtract nothing from the reduced system, while their Jc^T Jc
    and Jc^T r stay in the camera blocks.  Returns (delta, rms residual)."""
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
    delta = np.concatenate([dp.reshape(-1), dcm[:, :3].reshape(-1), dcm[:, 3:].reshape(-1)]) * gain
    return delta, math.sqrt((r * r).sum() / z.size)


def dense_step(x, z, K, nc, nt, fixed, gain=0.9):
    """inv(J^T J + I) J^T r * gain with the dense forward-difference J of O.ba_jacobian_fd and the anchors' columns zeroed."""
    zhat = O.ba_predict(x, K, nc, nt)
    JT = O.ba_jacobian_fd(x, K, nc, nt, zhat)
    rows = np.flatnonzero(np.repeat(np.asarray(fixed, bool), 3))
    JT[rows] = 0.0
    return np.linalg.solve(JT @ JT.T + np.eye(x.size), JT @ (z - zhat)) * gain


def solve_anchored(K, z, bad, x, nt_true, nt_pad, nc, fixed=None, max_iter=10):
    """RR.solve_padded with anchors: the LM loop of fcnNLS_batch on a window laid out for nt_pad rows, `fixed` bool [nt_pad]; the divisors
    nx = 3 nt + 6 nc and nz = 2 nt (nc + 1) are the true count's, anchors included (an anchored point still counts as rows of x).  -> (x, trace)."""
    x = x.copy()
    nx, nz = 3 * nt_true + 6 * nc, 2 * nt_true * (nc + 1)
    trace = []
    for _ in range(max_iter):
        delta, f = anchored_step(x, z, K, nc, nt_pad, fixed=fixed, bad=bad)
        x = x + delta
        xr = np.sqrt((delta * delta).sum() / nx)
        trace.append((f * np.sqrt(z.size / nz), xr))
        if xr < 1e-7:
            break
    return x, np.array(trace)


def scale_problem(nt, nf, seed, factor=1.08, n_anchor=4):
    """The scale experiment: a noise-free start (synth.ba_scene with sigma_pts = sigma_cams = 0: the start IS the truth, only the pixels are noisy) with
    every point and every camera position scaled by `factor`, except the first n_anchor points.  -> (K, z, x0, nt, nc, fixed, |last camera| of the truth)."""
    from velocity_amd import synth

    K = np.asarray(synth.K_1080P, np.float64)
    P, pw, cw = synth.ba_scene(nt, nf, seed=seed, sigma_pts=0.0, sigma_cams=0.0)
    z, x_true, nt, nc = synth.ba_pack(P, pw, cw)
    x0 = x_true.copy()
    x0[3 * n_anchor: 3 * nt + 3 * nc] *= factor  # points behind the anchors, then the camera positions (the rpy block is 0)
    fixed = np.zeros(nt, bool)
    fixed[:n_anchor] = True
    return K, z, x0, nt, nc, fixed, float(np.linalg.norm(cw[-1]))


def scale_ratio(x, nt, nc, truth):
    """|last camera| of a state x over the truth's."""
    return float(np.linalg.norm(x[3 * nt + 3 * (nc - 1): 3 * nt + 3 * nc])) / truth


def anchored_inputs(p3, anchors):
    """The points a refinement starts from: p3 [N0, 3] with the rows of `anchors` = (ids, xyz [n, 3]) replaced by the anchors' coordinates; and the mask
    over the N0 ids."""
    p3 = np.asarray(p3, np.float64).copy()
    mask = np.zeros(len(p3), bool)
    if anchors is not None and len(anchors[0]):
        ids = np.asarray(anchors[0], np.int64)
        p3[ids] = np.asarray(anchors[1], np.float64).reshape(-1, 3)
        mask[ids] = True
    return p3, mask


def _refine(K, P, p3, B, n, anchors, max_iter):
    """RR.refine_ref with anchors: the packing is its own on the replaced points (O.ba_pack), the solve is solve_anchored on the kept tracks' flags."""
    p3a, mask = anchored_inputs(p3, anchors)
    nfix = []

    def solver(K_, P_, pw_, cw_, max_iter=10, return_info=True):
        z, bad, x, nt, nc = O.ba_pack(K_, P_, pw_, cw_)
        keep = np.isfinite(P_[4]).sum(1) == P_.shape[2]
        fixed = mask[keep]
        nfix.append(int(fixed.sum()))
        x, trace = solve_anchored(np.asarray(K_, np.float64), z, bad, x, nt, nt, nc, fixed=fixed, max_iter=max_iter)
        j = 3 * nt
        return np.concatenate((np.zeros((1, 3)), x[j: j + 3 * nc].reshape(nc, 3)), 0), x[:j].reshape(nt, 3), x, trace

    out = RR.refine_ref(K, P, p3a, B, n, max_iter=max_iter, solver=solver)
    out["nfix"] = nfix[0] if nfix else 0
    return out


def refine_anchored_ref(K, P, p3, B, n, anchors=None, max_iter=10):
    """The whole clip (vh_session_refine) with the slot's anchors (ids, xyz) or None."""
    return _refine(K, P, p3, B, n, anchors, max_iter)


def refine_window_anchored_ref(K, P, p3, B, first, nf, anchors=None, max_iter=10):
    """Window [first, first + nf) (vh_session_refine_windows) with the slot's anchors: anchor coordinates replace p3, THEN + B[first, 3:6]
    (RW.window_inputs); an anchored track that is not alive through the window is simply not among its tracks."""
    p3a, _ = anchored_inputs(p3, anchors)
    Pw, pw0, Bw = RW.window_inputs(P, p3a, B, first, nf)
    # the replaced rows of pw0 are anchors + shift already: hand _refine the shifted anchors so its own replacement is the identity
    shifted = None if anchors is None or not len(anchors[0]) else (anchors[0], pw0[np.asarray(anchors[0], np.int64)])
    out = _refine(K, Pw, pw0, Bw, nf, shifted, max_iter)
    tr = out["trace"]
    out.update(first=first, f_first=tr[0, 0] if len(tr) else np.nan, f_last=tr[-1, 0] if len(tr) else np.nan)
    return out
