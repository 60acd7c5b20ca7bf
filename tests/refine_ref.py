"""NumPy model of the refinement of a finished clip (the reference's author sketched it at vidExample.py:157:
fcnNLS_batch(K, P[:, :, 0:i], p3, B[0:i, 3:6])) and of the padded window layout of vh_nls_batch_windows.  Checker only: the product never
imports it."""
import numpy as np

from oracle import nls_oracle as O


def refine_ref(K, P, p3, B, n, max_iter=10, solver=O.nls_batch_schur):
    """Bundle adjustment of a clip that has had all its n frames (history P [5, N0, >= n], world points p3 [N0, 3], per-frame records B [>= n, 14])
    and the speed derived from the refined camera positions.  Tracks: isfinite(P[4]).sum(1) == n (NLS.py:190), ascending id."""
    P = np.asarray(P)[:, :, :n]
    B = np.asarray(B)
    ids = np.flatnonzero(np.isfinite(P[4]).sum(1) == n).astype(np.int32)
    cw0 = B[:n, 3:6].astype(np.float64)
    out = {"nt": len(ids), "ids": ids}
    if len(ids) == 0:  # not solved
        out.update(cw=cw0, pw=np.zeros((0, 3)), iterations=0, converged=0, trace=np.zeros((0, 2)))
    else:
        cw, pw, x, trace = solver(np.asarray(K), P.copy(), np.asarray(p3, np.float64), cw0, max_iter=max_iter, return_info=True)
        out.update(cw=cw, pw=pw, iterations=len(trace), converged=int(trace[-1, 1] < 1e-7), trace=np.asarray(trace))
    out.update(speed_of(out["cw"], B[:n, 12]))
    return out


def speed_of(cw, t):
    """dr_i = |cw[i] - cw[i-1]| (float64), dt_i = t[i] - t[i-1] in float32 (vidExample.py:142), speed_i = dr_i / dt_i * 3.6; entry 0 is NaN;
    mean and std over i >= 1 (vidExample.py:177)."""
    cw = np.asarray(cw, np.float64)
    t = np.asarray(t, np.float32)
    dr = np.full(len(cw), np.nan)
    dr[1:] = np.sqrt(((cw[1:] - cw[:-1]) ** 2).sum(1))
    speed = np.full(len(cw), np.nan)
    speed[1:] = dr[1:] / (t[1:] - t[:-1]).astype(np.float64) * 3.6
    return {"dr": dr, "speed": speed, "speed_mean": speed[1:].mean(), "speed_std": speed[1:].std()}


def pad_window(z, bad, x, nt, nc, nt_pad):
    """A packed window (oracle.ba_pack) laid out for nt_pad >= nt tracks: padding rows are unobserved (`bad`) and sit at the point (0, 0, 1)."""
    nf = nc + 1
    zp = np.zeros((2, nf, nt_pad))
    bp = np.ones((2, nf, nt_pad), bool)
    zp[:, :, :nt] = z.reshape(2, nf, nt)
    bp[:, :, :nt] = bad.reshape(2, nf, nt)
    xp = np.concatenate((x[: 3 * nt], np.tile([0.0, 0.0, 1.0], nt_pad - nt), x[3 * nt:]))
    return zp.reshape(-1), bp.reshape(-1), xp


def solve_padded(K, z, bad, x, nt_true, nt_pad, nc, max_iter=10):
    """The LM loop of fcnNLS_batch on a padded window: oracle.ba_schur_step on all nt_pad rows, the two rms divisors taken from the true count
    (nx = 3 nt + 6 nc, nz = 2 nt (nc + 1)).  Returns (x, trace)."""
    x = x.copy()
    nx, nz = 3 * nt_true + 6 * nc, 2 * nt_true * (nc + 1)
    trace = []
    for _ in range(max_iter):
        delta, f = O.ba_schur_step(x, z, K, nc, nt_pad, bad=bad)
        x = x + delta
        xr = np.sqrt((delta * delta).sum() / nx)
        trace.append((f * np.sqrt(z.size / nz), xr))
        if xr < 1e-7:
            break
    return x, np.array(trace)
