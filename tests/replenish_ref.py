"""NumPy model of track replenishment (TrackerSession(replenish=...), vh_session_set_replenish): THE semantics the device is held to.
TEST INFRASTRUCTURE ONLY.  Shared by tests/test_replenish_cpu.py and tests/test_gpu_replenish.py.

ReplenishOracle is oracle.session_oracle.SessionOracle with `spare` tail rows and two extra stages behind every step:
  promotion  at frame born + baseline a newborn row is triangulated from its own baseline + 1 observations (fcn2vintercept on the rays fcnMSV1_t would
             build, origins from the tracker's own B) and, if the point passes the gate, joins the pose tracks (vp = 1, tri = 1);
  birth      on the schedule, new corners are detected in the bounding rectangle of the live tracks, away from them, refined by cornerSubPix and appended
             as fresh tail rows with vg = 1, vp = 0 -- "tracked, not yet used for the pose", the state of every non-plate track before the MSV frame
             (vidExample.py:126,160).
It is composed of tests/gftt_ref.good_features, oracle.klt_oracle.corner_subpix / bounding_rect and oracle.nls_oracle.pixel_to_uvec /
two_view_intercept / project_cam."""
import numpy as np

from oracle import klt_oracle as KO
from oracle import nls_oracle as NO
from oracle.session_oracle import SessionOracle

import gftt_ref as G


def birth_due(f, msv_frame, every, baseline, nhist):
    """A birth runs at a stream's own frame f (after that frame's bookkeeping and MSV)."""
    m0 = max(int(msv_frame), 0)
    return f > m0 and (f - m0) % every == 0 and f + baseline < nhist


def exclusion_mask(p, roi, min_distance):
    """ROI-relative uint8 mask: 255, and 0 where abs(x - rint(px)) < min_distance and abs(y - rint(py)) < min_distance for a live track (px, py)."""
    x0, x1, y0, y1 = roi
    rw, rh = x1 - x0, y1 - y0
    mask = np.full((rh, rw), 255, np.uint8)
    r = int(np.ceil(float(min_distance))) - 1  # the integer offsets d with abs(d) < min_distance
    if r < 0:
        return mask
    for px, py in np.asarray(p, np.float32):
        cx, cy = int(np.rint(px)) - x0, int(np.rint(py)) - y0
        xa, xb, ya, yb = max(cx - r, 0), min(cx + r + 1, rw), max(cy - r, 0), min(cy + r + 1, rh)
        if xa < xb and ya < yb:
            mask[ya:yb, xa:xb] = 0
    return mask


class ReplenishOracle(SessionOracle):
    """rep: an object with every, baseline, target, max_new, min_distance, border, max_reproj (velocity_amd.driver.Replenish); det: an object with quality,
    block, use_harris, harris_k, subpix (velocity_amd.driver.Frame0Settings).  p, p3, vp: the frame-0 tracks; the session gets `spare` rows behind them."""

    def __init__(self, K32, frame0, p, p3, vp, t0, rep, det, spare=0, **kw):
        super().__init__(K32, frame0, p, p3, vp, t0, **kw)
        n = self.p.shape[0]
        N0 = n + int(spare)
        nh = self.B.shape[0]
        self.rep, self.det, self.N0, self.nhist = rep, det, N0, nh
        self.vg = np.concatenate([self.vg, np.zeros(spare, bool)])
        self.vp = np.concatenate([self.vp, np.zeros(spare, bool)])
        self.p3 = np.concatenate([self.p3, np.zeros((spare, 3))])
        self.P = np.concatenate([self.P, np.full([5, spare, nh], np.nan, np.float32)], 1)
        self.born = np.full(N0, -1, np.int32)
        self.born[:n] = 0
        self.tri = np.zeros(N0, np.uint8)
        self.tri[:n] = 1
        self.n_rows = n
        self.target = n if rep.target is None else int(rep.target)
        self.counts = dict(born=np.zeros(nh, np.int64), promoted=np.zeros(nh, np.int64), rejected=np.zeros(nh, np.int64))
        self.reproj = {}  # row -> largest reprojection error at its promotion frame (pixels; inf: the point failed before the error was formed)
        self.births = []  # one entry per birth that got as far as the detector: frame, n_cur and rows_left before it, corners found / entered, strengths

    def step(self, im, time_s, frame_no):
        out = super().step(im, time_s, frame_no)
        self._promote(self.i)
        self._birth(self.i, np.asarray(im))
        return out

    # ---- promotion --------------------------------------------------------------------------------------------------------------------------
    def triangulate(self, rows, born):
        """C0 [len(rows), 3] of rows born at frame `born`, and the largest reprojection error of each over its baseline + 1 frames (inf where C0 is not
        finite or lies behind a camera)."""
        nb = self.rep.baseline + 1
        U = np.zeros((3, nb, len(rows)))
        for j in range(nb):
            U[:, j] = NO.pixel_to_uvec(self.K, self.P[0:2, rows, born + j].T).T  # as fcnMSV1_t builds them (MSV.py:15-17)
        A = (self.B[0, 0:3] - self.B[born:born + nb, 0:3]).astype(np.float64)  # float32 difference, then widened (MSV.py:18)
        with np.errstate(all="ignore"):
            C0 = NO.two_view_intercept(A, U)
            K = self.K.astype(np.float64)
            err = np.zeros(len(rows))
            ok = np.isfinite(C0).all(1)
            for j in range(nb):
                cam = C0 + self.B[born + j, 3:6].astype(np.float64)
                ok &= cam[:, 2] > 0
                d = NO.project_cam(cam, K) - self.P[0:2, rows, born + j].T.astype(np.float64)
                err = np.maximum(err, np.sqrt((d * d).sum(1)))
        err[~ok] = np.inf
        err[~np.isfinite(err)] = np.inf
        return C0, err

    def _promote(self, f):
        born = f - self.rep.baseline
        rows = np.nonzero(self.vg & (self.tri == 0) & (self.born == born))[0]
        if born <= 0 or len(rows) == 0:
            return
        C0, err = self.triangulate(rows, born)
        good = err < self.rep.max_reproj
        for g, e in zip(rows, err):
            self.reproj[int(g)] = float(e)
        self.p3[rows[good]] = C0[good]
        self.tri[rows[good]] = 1
        self.vp[rows[good]] = True
        self.counts["promoted"][f] += int(good.sum())
        self.counts["rejected"][f] += int((~good).sum())

    # ---- birth ------------------------------------------------------------------------------------------------------------------------------
    def _birth(self, f, im):
        rep, det = self.rep, self.det
        if not birth_due(f, self.msv_frame, rep.every, rep.baseline, self.nhist):
            return
        n_cur = self.p.shape[0]
        if n_cur == 0 or n_cur >= self.target or self.n_rows == self.N0:
            return
        roi = KO.bounding_rect(self.p, im.shape, rep.border)
        x0, x1, y0, y1 = roi
        rw, rh = x1 - x0, y1 - y0
        if rw < 3 or rh < 3 or rw < det.block or rh < det.block:
            return
        mask = exclusion_mask(self.p, roi, rep.min_distance)
        crop = np.ascontiguousarray(im[y0:y1, x0:x1])
        c = G.good_features(crop, int(rep.max_new), det.quality, rep.min_distance, mask, det.block, det.use_harris, det.harris_k)
        resp = G.response(crop, det.block, det.use_harris, det.harris_k)
        strength = resp[c[:, 1].astype(int), c[:, 0].astype(int)]  # descending: the list is response-ordered, so a prefix equals a smaller budget
        c = c + np.float32([x0, y0])
        win, iters, eps = det.subpix
        if len(c):
            c = KO.corner_subpix(im, c, win, iters, eps)
        m = min(len(c), self.target - n_cur, self.N0 - self.n_rows)
        self.births.append(dict(frame=f, n_cur=n_cur, entered=m, found=len(c), rows_left=self.N0 - self.n_rows, strength=strength))
        if m <= 0:
            return
        rows = np.arange(self.n_rows, self.n_rows + m)
        new = c[:m].astype(np.float32)
        self.p = np.concatenate([self.p, new])
        self.vg[rows] = True
        self.born[rows] = f
        self.P[0:2, rows, f] = new.T
        self.P[4, rows, f] = f
        self.n_rows += m
        self.counts["born"][f] += m

