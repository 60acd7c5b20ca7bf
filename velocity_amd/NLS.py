"""Drop-in counterparts of utils/NLS.py (estimateWorldCameraPose :9-33, fzK :71-78, fcnNLS_t :102-129,
fcnNLS_Rt :133-183) running on libvelocity_hip.  Same signatures, return dtypes and printed warnings."""
import numpy as np

from . import _lib as L
from .transforms import dcm2rpy


def _scratch(torch, shape):
    """BA workspace.  VH_POISON_WORKSPACE=1 (set by the test-suite) fills it with NaN bit patterns first, so a kernel that reads workspace
    memory it never wrote fails loudly instead of passing on whatever the caching allocator handed out."""
    import os

    t = torch.empty(shape, dtype=torch.uint8, device="cuda")
    if os.environ.get("VH_POISON_WORKSPACE"):
        t.fill_(0xFF)
    return t


def _ba_solve(fn, K_host, z, x0, nt, nc, max_iter, nw=None, extra=(), robust=None):
    """The device part of every fcnNLS_batch* shim: upload z and x0, allocate trace / info / workspace (one of each per window when nw is given), call
    the entry point `fn` (its arguments between nc and max_iter: `extra`), read back -> info, x, trace as numpy arrays.  robust = delta (pixels): `fn` is
    vh_nls_batch_windows_robust, `extra` gains delta and the count table, and the counts [nw, max_iter] come back as a fourth array."""
    torch = L.torch_cuda()
    lead = () if nw is None else (nw,)
    zd = L.to_dev(z, torch.float64)
    xd = L.to_dev(x0, torch.float64).clone()
    trace = torch.zeros(lead + (max_iter, 2), dtype=torch.float64, device="cuda")
    info = torch.zeros(lead + (2,), dtype=torch.int32, device="cuda")
    ws = L.workspace()
    nbytes = int(ws.lib.vh_nls_batch_workspace(nt, nc))
    scratch = _scratch(torch, lead + (nbytes,))
    nout = None
    if robust is not None:
        nout = torch.zeros(lead + (max_iter,), dtype=torch.int32, device="cuda")
        extra = tuple(extra) + (float(robust), L.dptr(nout))
    L.check(getattr(ws.lib, fn)(ws.handle, K_host.ctypes.data_as(L.f64p), L.dptr(zd), L.dptr(xd), nt, nc, *extra, int(max_iter), L.dptr(trace), L.dptr(info),
                                L.dptr(scratch), nbytes, L.stream_ptr()), fn)
    if nout is not None:
        return info.cpu().numpy(), xd.cpu().numpy(), trace.cpu().numpy(), nout.cpu().numpy()
    return info.cpu().numpy(), xd.cpu().numpy(), trace.cpu().numpy()


def _robust_delta(robust, who):
    """The Huber threshold of a shim: None (off) or a finite number of pixels >= 0 (0: off as well, through the robust entry point)."""
    if robust is None:
        return None
    d = float(robust)
    if not (np.isfinite(d) and d >= 0.0):
        raise ValueError(f"{who}: robust = {robust} must be a finite number of pixels >= 0")
    return d


def _pose(K, p, pw, x0, R, findR, want_proj=True):
    """vh_pose with ONE upload (p and pw packed into one host buffer when both are host arrays) and ONE download (R | res | proj | t | info packed into one
    device record): the drop-in call costs two PCIe transfers and one host synchronisation, not seven."""
    torch = L.torch_cuda()
    K64 = L.host_K(K)
    if hasattr(p, "is_cuda") or hasattr(pw, "is_cuda"):
        pd = L.to_dev(np.asarray(p, np.float32) if not hasattr(p, "is_cuda") else p, torch.float32).reshape(-1, 2)
        pwd = L.to_dev(np.asarray(pw, np.float64) if not hasattr(pw, "is_cuda") else pw, torch.float64).reshape(-1, 3)
    else:
        ph = np.ascontiguousarray(np.asarray(p, np.float32).reshape(-1, 2))
        pwh = np.ascontiguousarray(np.asarray(pw, np.float64).reshape(-1, 3))
        both = torch.from_numpy(np.concatenate((pwh.reshape(-1).view(np.uint8), ph.reshape(-1).view(np.uint8)))).cuda()
        pwd = both[: pwh.nbytes].view(torch.float64).view(-1, 3)
        pd = both[pwh.nbytes:].view(torch.float32).view(-1, 2)
    n = pd.shape[0]
    if pwd.shape[0] != n:
        raise ValueError("p and pw must have the same number of rows")
    x0 = np.ascontiguousarray(np.asarray(x0, np.float64).reshape(6))
    R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(9))
    npj = 2 * n if want_proj else 0
    rec = torch.zeros(10 + npj + 3, dtype=torch.float64, device="cuda")  # R 9 | res 1 | proj 2n | t (3 x f32 in 2 doubles) | info (2 x i32 in 1 double)
    Rout, res, proj = rec[0:9], rec[9:10], (rec[10: 10 + npj].view(n, 2) if want_proj else None)
    t, info = rec[10 + npj: 12 + npj].view(torch.float32)[:3], rec[12 + npj:].view(torch.int32)
    ws = L.workspace()
    L.check(ws.lib.vh_pose(ws.handle, K64.ctypes.data_as(L.f64p), L.dptr(pd), L.dptr(pwd), n, x0.ctypes.data_as(L.f64p),
                           R.ctypes.data_as(L.f64p), int(bool(findR)), L.dptr(t), L.dptr(Rout), L.dptr(res), L.dptr(proj), L.dptr(info),
                           L.stream_ptr()), "vh_pose")
    h = rec.cpu().numpy()  # the one host synchronisation of the call
    return (h[10 + npj: 12 + npj].view(np.float32)[:3].copy(), h[0:9].reshape(3, 3).copy(), float(h[9]), (h[10: 10 + npj].reshape(n, 2).copy() if want_proj else None),
            h[12 + npj:].view(np.int32).copy())


def estimateWorldCameraPose(K, p, p3, t=np.array([0, 0, 1]), R=np.eye(3), findR=False):
    """Camera pose from 2D-3D correspondences (utils/NLS.py:9-33) -> (t f32[3], R, residuals, p_proj)."""
    x0 = np.concatenate((dcm2rpy(np.asarray(R, float)), np.asarray(t, float)))
    tt, Rr, res, proj, info = _pose(K, p, p3, x0, R, findR is True)
    if not info[1]:
        print("WARNING: fcnNLS_Rt() reaching max iterations!" if findR is True else "WARNING: fcnNLS_t() reaching max iterations!")
    Rout = Rr.astype(np.float32) if findR is True else R
    return tt, Rout, res, proj


def fcnNLS_t(K, p, pw, x):
    """3-DoF translation fit (utils/NLS.py:102-129) -> x float32[3]."""
    x0 = np.concatenate((np.zeros(3), np.asarray(x, float)[:3]))
    t, _, _, _, info = _pose(K, p, pw, x0, np.eye(3), False, want_proj=False)
    if not info[1]:
        print("WARNING: fcnNLS_t() reaching max iterations!")
    return t


def fcnNLS_Rt(K, p, pw, x):
    """6-DoF pose fit, x = [roll,pitch,yaw,tx,ty,tz] (utils/NLS.py:133-183) -> (R float32[3,3], t float32[3])."""
    t, R, _, _, info = _pose(K, p, pw, x, np.eye(3), True, want_proj=False)
    if not info[1]:
        print("WARNING: fcnNLS_Rt() reaching max iterations!")
    return R.astype(np.float32), t


def fzK(a, K):
    """pscale(a @ K) (utils/NLS.py:71-78)."""
    from .common import world2image

    return world2image(K, np.eye(3), np.zeros(3), a)


def _track_filter(P, min_obs, who):
    """The tracks a window of history P [5, n, nf] takes, and its measurements [2, n, nf].  min_obs None: the reference's filter, alive in every frame
    (NLS.py:190), rows 0/1 as they are.  min_obs = M: observed -- row 4 finite -- in at least M of the nf frames, and NaN (no observation: zero
    residual, zero Jacobian rows in the solve) wherever row 4 is NaN."""
    seen = np.isfinite(P[4])
    if min_obs is None:
        return seen.sum(1) == P.shape[2], P[0:2].astype(np.float64)
    if not 2 <= int(min_obs) <= P.shape[2]:
        raise ValueError(f"{who}: min_obs = {min_obs} is outside 2 .. nf = {P.shape[2]}")
    return seen.sum(1) >= int(min_obs), np.where(seen[None], P[0:2].astype(np.float64), np.nan)


def fcnNLS_batch(K, P, pw, cw, max_iter=10, return_info=False, fixed=None, min_obs=None, robust=None):
    """Dense full bundle adjustment over tie points and cameras 1..nc (utils/NLS.py:186-250) -> (cw [nc+1,3], pw [nt,3]).

    The track filter, the measurement ordering and the state layout are the reference's (NLS.py:190-203); the
    iterations (forward-difference Jacobian, damped normal equations, x += 0.9 delta) run on the device.

    fixed: None (the reference's solve: its scale is whatever the start had), or a bool mask over the rows of pw: those points are ANCHORED -- they take
    no step (their rows come back as given) while their measurements still constrain the cameras, which pins the scale to them
    (vh_nls_batch_windows_fixed).  The mask is filtered like the tracks.

    min_obs: None (the reference's filter: alive in every frame), or M with 2 <= M <= nf: the tracks observed in at least M frames take part, a missing
    measurement being no observation (the windows entry takes it; the rms residual still runs over all 2 nt nf entries, as the reference forms it).

    robust: None (plain least squares, the reference's), or the Huber threshold delta in pixels: per iteration a measurement pair whose reprojection error
    |r| exceeds delta is weighted by delta / |r| (vh_nls_batch_windows_robust; f stays the unweighted rms residual).  With return_info the counts of
    down-weighted measurements per iteration run follow the trace.
    """
    P = np.asarray(P)
    pw = np.asarray(pw, np.float64)
    cw = np.asarray(cw, np.float64)
    keep, uv = _track_filter(P, min_obs, "fcnNLS_batch")  # NLS.py:190
    if fixed is not None:
        fixed = _fixed_mask(fixed, len(pw), "fcnNLS_batch")[keep]
    uv, pw = uv[:, keep], pw[keep]
    _, nt, nf = uv.shape
    nc = nf - 1
    z = np.concatenate([uv[0].T.reshape(-1), uv[1].T.reshape(-1)])  # NLS.py:198-199
    x0 = np.concatenate((pw, cw[1:], np.zeros((nc, 3)))).reshape(-1)  # NLS.py:202-203
    robust = _robust_delta(robust, "fcnNLS_batch")
    nout = None
    if robust is not None:  # one window of the robust entry: the launches of the windows entry with the weighted k_ba_jac
        fd = None if fixed is None else L.to_dev(fixed.astype(np.uint8), L.torch_cuda().uint8)
        info, x, tr, nout = (a[0] for a in _ba_solve("vh_nls_batch_windows_robust", L.host_K(K), z[None], x0[None], nt, nc, max_iter, 1,
                                                     (1, L.dptr(None), L.dptr(None), L.dptr(fd)), robust=robust))
    elif fixed is None and min_obs is None:
        info, x, tr = _ba_solve("vh_nls_batch", L.host_K(K), z, x0, nt, nc, max_iter)
    elif fixed is None:  # one window of the windows entry, which takes missing measurements
        info, x, tr = (a[0] for a in _ba_solve("vh_nls_batch_windows", L.host_K(K), z[None], x0[None], nt, nc, max_iter, 1, (1, L.dptr(None), L.dptr(None))))
    else:  # one window of the windows entry: the same launches, the same record
        fd = L.to_dev(fixed.astype(np.uint8), L.torch_cuda().uint8)
        info, x, tr = (a[0] for a in _ba_solve("vh_nls_batch_windows_fixed", L.host_K(K), z[None], x0[None], nt, nc, max_iter, 1, (1, L.dptr(None), L.dptr(None), L.dptr(fd))))
    tr = tr[: info[0]]
    for i, (f, xr) in enumerate(tr):
        print(f"{i:g}: f={f:g}, x={xr}")  # NLS.py:238 (without the wall-time column)
    if not info[1]:
        print("WARNING: fcnNLS_batch() reaching max iterations!")  # NLS.py:242
    j = nt * 3
    pw_out = x[:j].reshape(nt, 3)
    cw_out = np.concatenate((np.zeros((1, 3)), x[j : j + nc * 3].reshape(nc, 3)), 0)
    if return_info:
        return (cw_out, pw_out, x, tr) if nout is None else (cw_out, pw_out, x, tr, nout[: info[0]])
    return cw_out, pw_out


def _fixed_mask(fixed, n, who):
    m = np.asarray(fixed)
    if m.dtype != np.bool_ or m.shape != (n,):
        raise ValueError(f"{who}: fixed must be a bool mask over the {n} rows of pw, got {m.dtype} {m.shape}")
    return m


def pack_windows(Ps, pws, cws, fixed=None, min_obs=None):
    """Track filter and packing of fcnNLS_batch (utils/NLS.py:190-203) for several windows of one number of frames, laid out for the largest track
    count nt: z [nw, 2 nt nf] and x0 [nw, 3 nt + 6 nc] in the layout of vh_nls_batch_multi, counts int32[nw].  Rows behind a window's own count
    are padding: NaN measurements (no observation, see k_ba_jac) and the point (0, 0, 1).  Host only.  fixed: None, or one bool mask per window over
    the rows of its pw (None inside the list: no anchors in that window); the result then gains a sixth item, the flags uint8 [nw, nt] of the kept
    tracks (padding rows 0).  min_obs: None, or the least number of observed frames of a kept track (see fcnNLS_batch); z is then NaN wherever row 4 is."""
    zs, pts, cams, flags, nf0 = [], [], [], [], None
    if fixed is not None and len(fixed) != len(Ps):
        raise ValueError(f"fcnNLS_batch_windows: {len(fixed)} masks for {len(Ps)} windows")
    for w, (P, pw, cw) in enumerate(zip(Ps, pws, cws)):
        P, pw, cw = np.asarray(P), np.asarray(pw, np.float64), np.asarray(cw, np.float64)
        keep, uv = _track_filter(P, min_obs, "fcnNLS_batch_windows")  # NLS.py:190
        if fixed is not None:
            flags.append(np.zeros(int(keep.sum()), bool) if fixed[w] is None else _fixed_mask(fixed[w], len(pw), "fcnNLS_batch_windows")[keep])
        uv, pw = uv[:, keep], pw[keep]
        nf = P.shape[2]
        if nf0 is None:
            nf0 = nf
        elif nf0 != nf:
            raise ValueError(f"fcnNLS_batch_windows: window shapes differ ({nf0} vs {nf} frames)")
        zs.append(uv)  # [2, nt_w, nf] (NaN = no observation: kept)
        pts.append(pw)
        cams.append(np.concatenate((cw[1:], np.zeros((nf - 1, 3)))).reshape(-1))  # NLS.py:202-203
    nf, nw = nf0, len(zs)
    nc = nf - 1
    counts = np.array([len(p) for p in pts], np.int32)
    nt = max(1, int(counts.max()))
    z = np.full((nw, 2, nf, nt), np.nan)  # NLS.py:198-199: [all u | all v], camera-major / track-minor
    x0 = np.empty((nw, 3 * nt + 6 * nc))
    for w in range(nw):
        z[w, :, :, : counts[w]] = zs[w].transpose(0, 2, 1)
        x0[w] = np.concatenate((pts[w].reshape(-1), np.tile([0.0, 0.0, 1.0], nt - counts[w]), cams[w]))
    if fixed is None:
        return z.reshape(nw, -1), x0, counts, nt, nc
    fx = np.zeros((nw, nt), np.uint8)
    for w in range(nw):
        fx[w, : counts[w]] = flags[w]
    return z.reshape(nw, -1), x0, counts, nt, nc, fx


def fcnNLS_batch_windows(K, Ps, pws, cws, max_iter=10, return_info=False, fixed=None, min_obs=None, robust=None):
    """fcnNLS_batch (utils/NLS.py:186-250) for several independent windows of the same number of frames (one finished clip or sliding window per
    video stream) in one launch sequence (grid.y = window).  Ps / pws / cws: sequences of the reference's P, pw, cw arguments.  K: one 3x3 matrix
    for all windows, or one per window ([nw, 3, 3]).  The windows may keep different numbers of full-length tracks: pack_windows lays them out for
    the largest count and pads with unobserved points, which take no part in the solve (vh_nls_batch_windows); windows of equal counts and one K
    go through vh_nls_batch_multi unchanged.  A window without a full-length track is not solved (cw comes back as given).  Returns
    [(cw, pw), ...], pw cut to the window's own tracks (with return_info: also the padded x and the trace).  fixed: None, or a list of bool masks, one per
    window over the rows of its pw (see fcnNLS_batch; None inside the list: that window is solved free).  min_obs: None, or the least number of
    observed frames of a kept track (see fcnNLS_batch); such windows go through vh_nls_batch_windows(_fixed).  robust: None, or the Huber threshold in
    pixels for every window (see fcnNLS_batch; vh_nls_batch_windows_robust); with return_info each window's tuple then ends with its counts."""
    torch = L.torch_cuda()
    fx = None
    if fixed is None:
        z, x0, counts, nt, nc = pack_windows(Ps, pws, cws, min_obs=min_obs)
    else:
        z, x0, counts, nt, nc, fx = pack_windows(Ps, pws, cws, fixed, min_obs=min_obs)
    nw = len(counts)
    K64 = np.asarray(K, np.float64)
    per_window_K = K64.ndim == 3
    if per_window_K and len(K64) != nw:
        raise ValueError(f"fcnNLS_batch_windows: {len(K64)} intrinsics for {nw} windows")
    K_host = L.host_K(K64[0] if per_window_K else K64)
    robust = _robust_delta(robust, "fcnNLS_batch_windows")
    nout = None
    if robust is not None:
        ntd, fd = L.to_dev(counts, torch.int32), (None if fx is None else L.to_dev(fx, torch.uint8))
        Kd = L.to_dev(K64.reshape(nw, 9), torch.float64) if per_window_K else None
        info, x, tr, nout = _ba_solve("vh_nls_batch_windows_robust", K_host, z, x0, nt, nc, max_iter, nw, (nw, L.dptr(ntd), L.dptr(Kd), L.dptr(fd)), robust=robust)
    elif fx is not None:
        ntd, fd = L.to_dev(counts, torch.int32), L.to_dev(fx, torch.uint8)
        Kd = L.to_dev(K64.reshape(nw, 9), torch.float64) if per_window_K else None
        info, x, tr = _ba_solve("vh_nls_batch_windows_fixed", K_host, z, x0, nt, nc, max_iter, nw, (nw, L.dptr(ntd), L.dptr(Kd), L.dptr(fd)))
    elif per_window_K or (counts != nt).any() or min_obs is not None:
        ntd = L.to_dev(counts, torch.int32)
        Kd = L.to_dev(K64.reshape(nw, 9), torch.float64) if per_window_K else None
        info, x, tr = _ba_solve("vh_nls_batch_windows", K_host, z, x0, nt, nc, max_iter, nw, (nw, L.dptr(ntd), L.dptr(Kd)))
    else:
        info, x, tr = _ba_solve("vh_nls_batch_multi", K_host, z, x0, nt, nc, max_iter, nw, (nw,))
    out = []
    for w in range(nw):
        if not info[w, 1] and counts[w]:
            print("WARNING: fcnNLS_batch() reaching max iterations!")  # NLS.py:242
        j = nt * 3
        pw_out = x[w, : 3 * counts[w]].reshape(-1, 3)
        cw_out = np.concatenate((np.zeros((1, 3)), x[w, j : j + nc * 3].reshape(nc, 3)), 0)
        rec = (cw_out, pw_out, x[w], tr[w, : info[w, 0]]) + (() if nout is None else (nout[w, : info[w, 0]],))
        out.append(rec if return_info else (cw_out, pw_out))
    return out


def _cam2ned():  # common.py:159-164
    return np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float64)


def fcnNLS_batch2(K, P, pw, cw, max_iter=20, return_info=False):
    """Constrained bundle adjustment (utils/NLS.py:253-328): tie points, one joint rotation and a straight-line camera
    trajectory [el, az, ranges] -> (cw [nc+1,3], pw [nt,3]).

    Host side = the reference's filtering, packing and initial state (NLS.py:257-274); the LM iterations run on the
    device (vh_nls_batch2).  Reference defect resolved by intent: `sc2cc` switches to its column branch when exactly 3
    cameras are fitted (shape ambiguity, common.py:100); here the ranges / el / az are always read row-wise.
    """
    P = np.asarray(P)
    pw = np.asarray(pw, np.float64)
    cw = np.asarray(cw, np.float64)
    keep = np.isfinite(P[4]).sum(1) == P.shape[2]  # NLS.py:257
    P, pw = P[:, keep], pw[keep]
    _, nt, nf = P.shape
    nc = nf - 1
    z = np.concatenate([P[0].T.reshape(-1), P[1].T.reshape(-1)]).astype(np.float64)  # NLS.py:266-267
    C = _cam2ned()
    d = C @ (cw[1] - cw[0])  # cam -> ned (NLS.py:272), then cc2sc (common.py:81-94)
    r = np.linalg.norm(d)
    el, az = np.arcsin(-d[2] / r), np.arctan2(d[1], d[0])
    ranges = np.arange(1, nc + 1) * r
    x0 = np.concatenate((pw.ravel(), np.zeros(3), [el, az], ranges))  # NLS.py:274
    info, x, tr = _ba_solve("vh_nls_batch2", L.host_K(K), z, x0, nt, nc, max_iter)
    tr = tr[: info[0]]
    if not info[1]:
        print("WARNING: fcnNLS_batch() reaching max iterations!")  # NLS.py:314 (sic)
    print(f"fcnNLS_batch2 done in {info[0] - 1:g} steps, f={tr[-1, 0]:g}")  # NLS.py:315 (without the wall-time column)
    j = nt * 3
    rg, el, az = x[j + 5 : j + 5 + nc], x[j + 3], x[j + 4]
    a = rg * np.cos(el)
    ned = np.stack([a * np.cos(az), a * np.sin(az), -rg * np.sin(el)], 1)  # sc2cc, row-wise (common.py:106-111)
    cw_out = np.concatenate((np.zeros((1, 3)), ned @ C), 0)
    pw_out = x[:j].reshape(nt, 3)
    if return_info:
        return cw_out, pw_out, x, tr
    return cw_out, pw_out
