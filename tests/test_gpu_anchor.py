"""Bundle adjustment with anchored points on the device against the NumPy model tests/anchor_ref.py: the entry point vh_nls_batch_windows_fixed on
every route of the BA plan, the scale it recovers, the session's anchor table (vh_session_set_anchors) through refine() / refine_windows(), and the
drivers' refine_anchor="plate".

Tolerances are the project's own for "GPU against the NumPy model, another partition of the partial sums" (tests/test_gpu_refine.py): x rtol 1e-6 /
atol 1e-8, trace[:, 0] rtol 1e-8, info equal.  What anchoring promises beyond them is exact: an anchored row comes back np.array_equal to its start,
padding rows byte for byte, an empty window untouched, and a NULL or all-zero table gives the bytes of vh_nls_batch_windows."""
import ctypes as C

import numpy as np
import pytest

import anchor_ref as AR
import scenes as S
from scenes import T0
from session_support import raw_export, session_at, step_to
from velocity_amd import synth

pytestmark = pytest.mark.gpu

MAX_ITER = 10


def _solve(K, z, x0, nt, nc, counts=None, Ks=None, fixed="absent"):
    """vh_nls_batch_windows (fixed="absent") or vh_nls_batch_windows_fixed (fixed: None = NULL table, or uint8 [nw, nt]) on packed windows
    -> (x [nw, nx], trace [nw, MAX_ITER, 2], info [nw, 2]).  The workspace is poisoned first."""
    import torch

    from velocity_amd import _lib as L

    ws = L.workspace()
    nw = len(z)
    zd, xd = L.to_dev(z, torch.float64), L.to_dev(x0, torch.float64).clone()
    trace = torch.zeros((nw, MAX_ITER, 2), dtype=torch.float64, device="cuda")
    info = torch.full((nw, 2), -7, dtype=torch.int32, device="cuda")
    nbytes = int(ws.lib.vh_nls_batch_workspace(nt, nc))
    scratch = torch.full((nw, nbytes), 0xFF, dtype=torch.uint8, device="cuda")
    Kp = L.host_K(K).ctypes.data_as(L.f64p)
    ntd = None if counts is None else L.to_dev(np.asarray(counts, np.int32), torch.int32)
    Kd = None if Ks is None else L.to_dev(np.asarray(Ks, np.float64).reshape(nw, 9), torch.float64)
    if isinstance(fixed, str):
        L.check(ws.lib.vh_nls_batch_windows(ws.handle, Kp, L.dptr(zd), L.dptr(xd), nt, nc, nw, L.dptr(ntd), L.dptr(Kd), MAX_ITER, L.dptr(trace),
                                            L.dptr(info), L.dptr(scratch), nbytes, L.stream_ptr()), "vh_nls_batch_windows")
    else:
        fd = None if fixed is None else L.to_dev(np.ascontiguousarray(fixed, np.uint8), torch.uint8)
        assert fd is None or tuple(fd.shape) == (nw, nt)
        L.check(ws.lib.vh_nls_batch_windows_fixed(ws.handle, Kp, L.dptr(zd), L.dptr(xd), nt, nc, nw, L.dptr(ntd), L.dptr(Kd), L.dptr(fd), MAX_ITER,
                                                  L.dptr(trace), L.dptr(info), L.dptr(scratch), nbytes, L.stream_ptr()), "vh_nls_batch_windows_fixed")
    return xd.cpu().numpy(), trace.cpu().numpy(), info.cpu().numpy()


def test_a_null_or_empty_table_is_the_windows_call():
    """The five 50 x 6 windows of test_gpu_refine.py::test_windows_with_null_tables_...: x byte for byte, info equal, the trace to the order of its
    atomics.  (On the parent commit the symbol does not exist.)"""
    from velocity_amd.NLS import pack_windows

    scenes = [synth.ba_scene(50, 6, seed=400 + w) for w in range(5)]
    z, x0, cnt, nt, nc = pack_windows(*zip(*scenes))
    assert list(cnt) == [50] * 5
    a = _solve(synth.K_1080P, z, x0, nt, nc)
    for fixed in (None, np.zeros((5, nt), np.uint8)):
        b = _solve(synth.K_1080P, z, x0, nt, nc, fixed=fixed)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[2], b[2])
        np.testing.assert_allclose(a[1], b[1], rtol=1e-12)
    # ... with the other two tables in use as well
    counts = [50, 37, 1, 0, 50]
    scenes2 = []
    for (P, pw0, cw0), n in zip(scenes, counts):
        P = P.copy()
        P[:, n:, 4:] = np.nan
        scenes2.append((P, pw0, cw0))
    z, x0, cnt, nt, nc = pack_windows(*zip(*scenes2))
    Ks = np.stack([synth.K_1080P * (1.0 + 0.01 * np.array([[w, 0, 0], [0, w, 0], [0, 0, 0]])) for w in range(5)])
    a = _solve(Ks[0], z, x0, nt, nc, counts, Ks)
    b = _solve(Ks[0], z, x0, nt, nc, counts, Ks, fixed=np.zeros((5, nt), np.uint8))
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[2], b[2])
    np.testing.assert_allclose(a[1], b[1], rtol=1e-12)


COUNTS = [24, 17, 4, 0]


ROUTES = pytest.mark.parametrize("nf,force_valu", [(4, 0), (22, 0), (24, 0), (22, 1), (44, 0)],
                                 ids=["gj-mfma", "gj-valu-solve", "cholesky", "valu-schur", "zbuild-syrk"])
_ROUTE = {}
# The scene of the window WITHOUT anchors, per number of frames: the first seed from 900 + nf on which the NumPy model reproduces its own trace to 2e-9, a
# fifth of the bound -- solved with the tracks in reverse order (another order of the sums) and in the reference's dense form inv(J^T J + I) J^T r
# (NLS.py:235) instead of the Schur complement.  A free solve drifts along its scale gauge, and over 700 scene sets tried on the CPU the model's two forms
# agree on a free window's trace to 1e-9 .. 1e-8 only (seeds 922 and 924: 2.2e-9 and 7.7e-9), against 3e-9 at worst with four anchors and 1e-11 with all
# points anchored: on an arbitrary scene the bound of 1e-8 would measure the reference, not the device.
FREE_SEED = {4: 904, 22: 923, 24: 925, 44: 944}


def _route(nf, force_valu):
    """One solve per route, shared by the two tests below: windows laid out for 24 tracks with 24, 17, 4 and 0 of them: none anchored / the first four
    rows / every row of the window / empty.  -> (x0, fx, x, trace, info, the model's (x, trace) per solved window)

    Which window is the free one is not arbitrary.  A free window of 4 tracks and 21 cameras (176 measurements for 138 unknowns and a scale gauge held
    by the damping alone) is so weakly determined that the NumPy model does not reproduce ITSELF to the 1e-8 asked of the trace: solving it with the
    tracks in reverse order -- another order of the sums, nothing else -- moves trace[:, 0] by 1.6e-8 (7.7e-9 at 4 frames).  With the masks placed as
    here the same experiment moves the model by at most 2.2e-9 (the free window of 24 tracks), 8.8e-10 (four anchors among 17) and 8e-12 (all four
    anchored) over the four numbers of frames."""
    from velocity_amd import _lib as L
    from velocity_amd.NLS import pack_windows

    if (nf, force_valu) not in _ROUTE:
        nt, nc = 24, nf - 1
        Ks, scenes = [], []
        for w, cnt in enumerate(COUNTS):
            K = synth.K_1080P.astype(np.float64).copy()
            K[0, 0] *= 1.0 + 0.01 * w
            K[1, 1] *= 1.0 + 0.01 * w
            P, pw0, cw0 = synth.ba_scene(nt, nf, seed=FREE_SEED[nf] if w == 0 else 900 + nf + w, K=K)
            P[:, cnt:, nf - 2:] = np.nan
            Ks.append(K)
            scenes.append((P, pw0, cw0))
        masks = [np.zeros(nt, bool), np.arange(nt) < 4, np.ones(nt, bool), np.ones(nt, bool)]
        z, x0, cnt, nt_common, _, fx = pack_windows(*zip(*scenes), fixed=masks)
        assert list(cnt) == COUNTS and nt_common == nt and fx.sum(1).tolist() == [0, 4, 4, 0]
        L.load().vh_debug_ba_force_valu(force_valu)
        try:
            x, tr, info = _solve(Ks[0], z, x0, nt, nc, COUNTS, Ks, fixed=fx)
        finally:
            L.load().vh_debug_ba_force_valu(0)
        model = []
        for w, n in enumerate(COUNTS[:3]):
            zw = z[w].reshape(2, nf, nt)[:, :, :n].reshape(-1)
            xw = np.concatenate((x0[w, : 3 * n], x0[w, 3 * nt:]))
            model.append(AR.solve_anchored(Ks[w], zw, np.zeros(zw.size, bool), xw, n, n, nc, fixed=fx[w, :n].astype(bool), max_iter=MAX_ITER))
        _ROUTE[nf, force_valu] = (x0, fx, x, tr, info, model)
    return _ROUTE[nf, force_valu]


@ROUTES
def test_anchored_windows_equal_the_model_on_every_route(nf, force_valu):
    """x, info and -- of the windows that have anchors -- the trace against the model; anchored rows equal to the start, padding rows byte for byte,
    the empty window untouched.  (The trace of the free window: the next test.)"""
    nt = 24
    x0, fx, x, tr, info, model = _route(nf, force_valu)
    for w, n in enumerate(COUNTS):
        pad = slice(3 * n, 3 * nt)
        assert x[w, pad].tobytes() == x0[w, pad].tobytes(), f"window {w}: padding rows moved"
        if n == 0:
            assert list(info[w]) == [0, 0] and x[w].tobytes() == x0[w].tobytes(), f"window {w}: an empty window was touched"
            continue
        fixed = fx[w, :n].astype(bool)
        mx, mtr = model[w]
        gx = np.concatenate((x[w, : 3 * n], x[w, 3 * nt:]))
        print(f"nf={nf} valu={force_valu} window {w} (nt_w={n}, {fixed.sum()} anchored): info {info[w]} vs {[len(mtr), int(mtr[-1, 1] < 1e-7)]}, "
              f"max |dx| = {np.abs(gx - mx).max():.3g}, max rel df = {np.abs(tr[w, :len(mtr), 0] / mtr[:, 0] - 1).max():.3g}")
        assert list(info[w]) == [len(mtr), int(mtr[-1, 1] < 1e-7)], f"window {w}"
        np.testing.assert_allclose(gx, mx, rtol=1e-6, atol=1e-8, err_msg=f"window {w}")
        if fixed.any():
            np.testing.assert_allclose(tr[w, :len(mtr), 0], mtr[:, 0], rtol=1e-8, err_msg=f"window {w}")
        rows = np.repeat(fixed, 3)
        assert np.array_equal(x[w, : 3 * n][rows], x0[w, : 3 * n][rows]), f"window {w}: an anchored row moved"
        if not fixed.all():
            assert not np.array_equal(x[w, : 3 * n][~rows], x0[w, : 3 * n][~rows])


@ROUTES
def test_the_free_window_among_anchored_ones_keeps_its_trace(nf, force_valu):
    """trace[:, 0] of the window WITHOUT anchors against the model at rtol 1e-8, on the scenes of FREE_SEED (see there why they are chosen)."""
    _, _, _, tr, _, model = _route(nf, force_valu)
    mtr = model[0][1]
    print(f"nf={nf} valu={force_valu} free window: max rel df = {np.abs(tr[0, :len(mtr), 0] / mtr[:, 0] - 1).max():.3g}")
    np.testing.assert_allclose(tr[0, :len(mtr), 0], mtr[:, 0], rtol=1e-8)


@pytest.mark.parametrize("nt,nf,seed", [(50, 6, 400), (24, 22, 701)])
def test_anchors_recover_the_scale_on_the_device(nt, nf, seed):
    """tests/test_anchor_cpu.py's scale experiment on the device, the same two thresholds (the model meets them alone: free 1.0722 / 1.0675,
    anchored 0.9985 / 1.0006)."""
    K, z, x0, nt, nc, fixed, truth = AR.scale_problem(nt, nf, seed)
    xf, _, _ = _solve(K, z[None], x0[None], nt, nc, fixed=None)
    xa, _, _ = _solve(K, z[None], x0[None], nt, nc, fixed=fixed[None].astype(np.uint8))
    free, anch = AR.scale_ratio(xf[0], nt, nc, truth), AR.scale_ratio(xa[0], nt, nc, truth)
    print(f"({nt}, {nf}, {seed}): free {free:.4f}, anchored {anch:.4f}")
    assert abs(anch - 1.0) <= 0.01
    assert free >= 1.05
    assert np.array_equal(xa[0, :12], x0[:12])


def test_python_shims_and_torch_op_take_the_mask(capsys):
    import torch

    import velocity_amd.torch_ops as tops
    from velocity_amd.NLS import fcnNLS_batch, fcnNLS_batch_windows, pack_windows

    K = synth.K_1080P
    scenes = [synth.ba_scene(24, 4, seed=950 + w) for w in range(2)]
    scenes[1][0][:, 17:, 2:] = np.nan
    masks = [np.arange(24) < 4, np.arange(24) % 5 == 0]
    out = fcnNLS_batch_windows(K, *zip(*scenes), return_info=True, fixed=masks)
    z, x0, cnt, nt, nc, fx = pack_windows(*zip(*scenes), fixed=masks)
    x, tr, info = _solve(K, z, x0, nt, nc, cnt, fixed=fx)
    for w in range(2):
        assert np.array_equal(out[w][2], x[w]) and len(out[w][3]) == info[w, 0]
    cw, pw, xs, trs = fcnNLS_batch(K, scenes[0][0].copy(), scenes[0][1], scenes[0][2], return_info=True, fixed=masks[0])
    assert np.array_equal(pw[:4], scenes[0][1][:4]) and "0: f=" in capsys.readouterr().out
    np.testing.assert_allclose(xs, x[0], rtol=1e-6, atol=1e-8)  # (one window alone: another partition of the partial sums)
    Kt = torch.from_numpy(np.asarray(K, np.float64))
    xt, trt, it = tops.ops.ba_solve_fixed(Kt, torch.from_numpy(z).cuda(), torch.from_numpy(x0).cuda(), nt, nc, torch.from_numpy(cnt).cuda(),
                                          torch.from_numpy(fx).cuda(), MAX_ITER)
    assert np.array_equal(xt.cpu().numpy(), x) and np.array_equal(it.cpu().numpy(), info)
    xn, _, _ = tops.ops.ba_solve_fixed(Kt, torch.from_numpy(z).cuda(), torch.from_numpy(x0).cuda(), nt, nc, torch.from_numpy(cnt).cuda())
    assert np.array_equal(xn.cpu().numpy(), _solve(K, z, x0, nt, nc, cnt)[0])


# ---- the session's anchor table ---------------------------------------------------------------------------------------------------------------------------
N0, NF, NHIST = 150, 8, 10
# The world points of scenes.scenes3 carry N(0, P3_SIGMA^2) of error here, as points measured from a plate do.  With exact points these rendered clips are
# tracked to f = 0.002 - 0.003 pixels, and rtol 1e-8 of that is 2e-11 pixels, which the forward-difference Jacobian (1e-6 steps on coordinates of hundreds
# of pixels: 7e-8 of absolute error per entry) does not give the NumPy model itself; with 2 cm of error f is of the size it has on real footage (0.195
# pixels on the stills), where the bound means what it says.  Every `hopeless`-th track of a stream -- track 0 among them -- dies at once.
P3_SIGMA = 0.02  # metres

# The scene of the slot WITHOUT anchors and the start of its free window.  A free solve drifts along its scale gauge, and on the states this tracker reaches the
# NumPy model reproduces its own free traces (tracks in reverse order; the reference's dense form, NLS.py:235) only to 1e-9 .. 4e-8 for the whole clip and
# 2e-9 .. 2e-8 for a window of four frames: 16 seeds (433 .. 448) x 5 window starts were studied on the CPU from dumped session states.  None reaches the
# 2e-9 of FREE_SEED for both; 439 with the window at frame 3 is the best of them (8.5e-10 for the clip, 2.4e-9 for the window, a quarter of the bound) and is
# what the bound of 1e-8 is asserted on.  The recipe's own 433 gives 5.2e-9 and 9.3e-9: the reference at the bound itself.
SLOT2_SEED, SLOT2_FIRST = 439, 3


def _noisy3(n0=N0):
    return S.scenes3(n0, NHIST, SLOT2_SEED, P3_SIGMA)


# slot 0: a snapshot of ids 0..3 (track 0 dies at once: every window has lost it); slot 1: explicit coordinates of three tracks that all die at once
# (hopeless = 11) and one that lives; slot 2: none
ANCHOR_IDS = ([0, 1, 2, 3], [0, 11, 22, 5], [])


def _explicit_xyz(b, n0=N0):
    return _noisy3(n0)[b][2][ANCHOR_IDS[b]] + np.array([[0.004, -0.003, 0.01]])


def _session_with_anchors(frame, anchors=True, n0=N0):
    """Three streams of two cameras in one session, anchors set right after frame 0 (before the re-triangulation frame 5), stepped to `frame`."""
    scenes = _noisy3(n0)
    ses = session_at(scenes, 0)
    if anchors:
        ses.set_anchors(0, ANCHOR_IDS[0])
        ses.set_anchors(1, ANCHOR_IDS[1], _explicit_xyz(1, n0))
    step_to(ses, scenes, 1, frame)
    return ses


def _equals_model(ba, ref, where, window=False, trace=True):
    print(f"{where}: nt {ba['nt']} / {ref['nt']}, nfix {ba['nfix']} / {ref['nfix']}, iterations {ba['iterations']} / {ref['iterations']}, "
          f"speed {ba['speed_mean']:.4f} (model {ref['speed_mean']:.4f}), max |dcw| {np.abs(ba['cw'] - ref['cw']).max():.3g}")
    assert ba["nt"] == ref["nt"] and ba["nfix"] == ref["nfix"] and np.array_equal(ba["ids"], ref["ids"]), where
    assert ba["iterations"] == ref["iterations"] and ba["converged"] == ref["converged"], where
    for key in ("cw", "pw", "dr", "speed", "speed_mean", "speed_std"):
        np.testing.assert_allclose(ba[key], ref[key], rtol=1e-6, atol=1e-8, equal_nan=True, err_msg=f"{where}: {key}")
    if trace:
        np.testing.assert_allclose(ba["trace"][:, 0], ref["trace"][:, 0], rtol=1e-8, err_msg=where)
    if window:
        assert ba["first"] == ref["first"], where


def _raw_records(handle):
    """The records of a refine() / refine_windows() request as they arrived, one uint8 array per record."""
    handle.result()
    nb = handle.layout.bytes
    if hasattr(handle, "bufs"):
        return [b.numpy()[:nb].copy() for b in handle.bufs]
    return [b.numpy()[k * nb:(k + 1) * nb].copy() for b, cnt in handle.parts for k in range(cnt)]


def _fields_that_differ(a, b, lay):
    """Names of the record fields (offsets `lay`) that hold a differing byte of two records."""
    offs = sorted((getattr(lay, k), k) for k, t in lay._fields_ if t is C.c_size_t and k != "bytes" and (getattr(lay, k) or k in ("nt", "slot")))
    names = set()
    for at in np.flatnonzero(a != b):
        names.add([k for o, k in offs if o <= at][-1])
    return names


_SESSION = {}


def _session_case():
    """The anchored session after its last frame, refined whole and in windows, with the models of every record: built once, shared by the tests below."""
    if _SESSION:
        return _SESSION
    scenes = _noisy3()
    ses = _session_with_anchors(NF - 1)
    anchors = [ses.anchors(0), ses.anchors(1), None]
    before = [raw_export(ses, b) for b in range(3)]
    st = [ses.state(b) for b in range(3)]
    whole = ses.refine([0, 1, 2]).result()
    wins = [(0, 0), (0, 2), (1, 1), (2, SLOT2_FIRST), (1, 3)]
    got = ses.refine_windows(wins, 4, with_points=True).result()
    after = [raw_export(ses, b) for b in range(3)]
    whole_ref = [AR.refine_anchored_ref(scenes[b][4], st[b]["P"], st[b]["p3"], st[b]["B"], NF, anchors[b]) for b in range(3)]
    win_ref = [AR.refine_window_anchored_ref(scenes[b][4], st[b]["P"], st[b]["p3"], st[b]["B"], first, 4, anchors[b]) for b, first in wins]
    _SESSION.update(ses=ses, st=st, before=before, after=after, whole=whole, wins=wins, got=got, whole_ref=whole_ref, win_ref=win_ref)
    return _SESSION


def test_session_anchors_refine_and_refine_windows_equal_the_model():
    """Every record of the request -- anchored or not -- against the model: x, info, speeds and trace."""
    scenes = _noisy3()
    c = _session_case()
    ses = c["ses"]
    # the table holds the frame-0 values although the clip has passed the re-triangulation frame, which rewrote p3 of the surviving tracks
    ids0, xyz0 = ses.anchors(0)
    assert ids0.tolist() == [0, 1, 2, 3] and np.array_equal(xyz0, scenes[0][2][:4])
    assert not np.array_equal(ses.state(0)["p3"][1:4], scenes[0][2][1:4])
    ids1, xyz1 = ses.anchors(1)
    assert ids1.tolist() == sorted(ANCHOR_IDS[1]) and np.array_equal(xyz1, _explicit_xyz(1)[np.argsort(ANCHOR_IDS[1])])
    assert ses.anchors(2)[0].size == 0
    st, whole, wins, got = c["st"], c["whole"], c["wins"], c["got"]
    assert c["after"] == c["before"]  # the session is only read
    for b in range(3):
        _equals_model(whole[b], c["whole_ref"][b], f"stream {b}")
    assert [w["nfix"] for w in whole] == [3, 1, 0]  # track 0 of slot 0 and three of slot 1's four are dead; slot 2 has none
    for (b, first), w, ref in zip(wins, got, c["win_ref"]):
        _equals_model(w, ref, f"window ({b}, {first})", window=True)
        assert (w["slot"], w["first"]) == (b, first)
    assert [w["nfix"] for w in got] == [3, 3, 1, 0, 1]
    # an anchored row of a window with first > 0 sits at the anchor + B[first, 3:6], and stays there
    w = got[1]
    at = [list(w["ids"]).index(i) for i in (1, 2, 3)]
    assert np.array_equal(w["pw"][at], xyz0[1:4] + st[0]["B"][2, 3:6].astype(np.float64))
    # the free twin: a window without an anchor equals its record apart from nothing at all; the anchored ones differ
    twin = _session_with_anchors(NF - 1, anchors=False)
    free = twin.refine_windows(wins, 4, with_points=True).result()
    for key in ("nt", "nfix", "iterations", "converged", "ids", "cw", "pw", "dr", "speed"):
        assert np.array_equal(np.asarray(got[3][key]), np.asarray(free[3][key]), equal_nan=True), key
    assert not np.array_equal(got[0]["cw"], free[0]["cw"]) and free[0]["nfix"] == 0


def test_session_records_keep_their_trace():
    """trace[:, 0] of all eight session records against the model at rtol 1e-8, and of the two without an anchor also against the free session's at
    rtol 1e-12 (two runs of one solve: its sums are atomics).  See SLOT2_SEED for the scene of the slot that has no anchors."""
    c = _session_case()
    pairs = [(w, r, f"stream {b}") for b, (w, r) in enumerate(zip(c["whole"], c["whole_ref"]))] + \
            [(w, r, f"window {win}") for win, w, r in zip(c["wins"], c["got"], c["win_ref"])]
    for ba, ref, where in pairs:
        print(f"{where} ({ref['nfix']} anchors): max rel df = {np.abs(ba['trace'][:, 0] / ref['trace'][:, 0] - 1).max():.3g}, "
              f"max abs df = {np.abs(ba['trace'][:, 0] - ref['trace'][:, 0]).max():.3g}")
    assert len(pairs) == 8 and sum(ref["nfix"] > 0 for _, ref, _ in pairs) == 6
    for ba, ref, where in pairs:
        np.testing.assert_allclose(ba["trace"][:, 0], ref["trace"][:, 0], rtol=1e-8, err_msg=where)
    twin = _session_with_anchors(NF - 1, anchors=False)
    free_whole, free_win = twin.refine([0, 1, 2]).result()[2], twin.refine_windows(c["wins"], 4, with_points=True).result()[3]
    for ba, free, where in ((c["whole"][2], free_whole, "stream 2"), (c["got"][3], free_win, f"window (2, {SLOT2_FIRST})")):
        assert ba["nfix"] == free["nfix"] == 0 and np.array_equal(ba["cw"], free["cw"]) and np.array_equal(ba["pw"], free["pw"]), where
        np.testing.assert_allclose(ba["trace"], free["trace"], rtol=1e-12, err_msg=where)


_CLEARED = {}
N0_SMALL = 32


def _cleared_case(n0):
    """Records of a session whose anchors were set and then cleared beside those of one that never had any: [(records a, records b, layout)] for
    refine() and refine_windows(); built once per track capacity."""
    if n0 not in _CLEARED:
        ses, twin = _session_with_anchors(NF - 1, n0=n0), _session_with_anchors(NF - 1, anchors=False, n0=n0)
        ses.set_anchors(0, [])
        ses.set_anchors(1, [])
        assert all(ses.anchors(b)[0].size == 0 for b in range(3))
        wins = [(0, 0), (1, 2), (2, 4)]
        pairs = []
        for a, b in ((ses.refine([0, 1, 2]), twin.refine([0, 1, 2])), (ses.refine_windows(wins, 4, with_points=True), twin.refine_windows(wins, 4, with_points=True))):
            pairs.append((_raw_records(a), _raw_records(b), a.layout))
        _CLEARED[n0] = pairs
    return _CLEARED[n0]


def test_setting_then_clearing_anchors_gives_byte_identical_records():
    """The whole record, byte for byte, of sessions of 32 tracks.  The size is chosen for what "byte-identical" can mean: the two sums of squares behind
    an iteration record are accumulated with floating-point atomics, one per workgroup -- k_ba_jac's r^2 into 16 slots by block number, the update
    kernel's delta^2 into one word -- so their value has a defined order only while at most two workgroups add to a word (a + b = b + a; three terms
    already round differently by order).  The update kernel takes 32 points per workgroup plus one workgroup for the cameras: 32 tracks is the
    largest session whose iteration record is reproducible at all, between two sessions or between two calls of one (tests/test_gpu_refine.py
    compares the latter at rtol 1e-12 for this reason).  Everything else in a record has no such limit: the next test, at 150 tracks."""
    for ra, rb, lay in _cleared_case(N0_SMALL):
        differ = [_fields_that_differ(x, y, lay) for x, y in zip(ra, rb)]
        assert len(ra) == len(rb) == 3 and not any(differ), differ
        assert all(np.frombuffer(x, np.int32, 1, lay.nt)[0] > 8 for x in ra)  # (solved windows, not empty ones)


def test_setting_then_clearing_anchors_is_never_setting_them_at_150_tracks():
    """Every field the solve's result decides -- header, ids, points, cameras, speeds -- byte for byte; the iteration record (trace, f_first, f_last)
    is summed by six workgroups here, in an order that varies from run to run (see the test above), and is held to rtol 1e-12, the project's bound for
    two runs of one solve."""
    from velocity_amd.driver import unpack_refine, unpack_refine_window

    for ra, rb, lay in _cleared_case(N0):
        differ = [_fields_that_differ(x, y, lay) for x, y in zip(ra, rb)]
        print("fields that differ:", differ)
        assert len(ra) == len(rb) == 3 and not any(d - {"trace", "f_first", "f_last"} for d in differ), differ
        for x, y in zip(ra, rb):
            a, b = (unpack_refine_window(r, lay) if hasattr(lay, "with_points") else unpack_refine(r, lay, NF) for r in (x, y))
            assert a["trace"].shape == b["trace"].shape and len(a["trace"]) > 0
            for key in ("trace", "f_first", "f_last"):
                np.testing.assert_allclose(a[key], b[key], rtol=1e-12, err_msg=key)


def test_reinitialising_a_slot_clears_its_anchors():
    ses = _session_with_anchors(2)
    ses.set_anchors(2, [4, 5, 6])
    assert ses.anchors(2)[0].tolist() == [4, 5, 6] and ses.anchors(0)[0].tolist() == [0, 1, 2, 3]
    frames, p, p3, vp, Kb = _noisy3()[2]
    ses.init_stream(2, frames[0], p, p3, vp, T0, time0=20.0, K=Kb)  # a new clip is a new plate
    assert ses.anchors(2)[0].size == 0 and ses.anchors(0)[0].tolist() == [0, 1, 2, 3]


def test_set_anchors_refusals_name_their_cause_and_queue_nothing():
    from velocity_amd import _lib as L
    from velocity_amd.driver import TrackerSession

    ses = _session_with_anchors(2)
    before = [raw_export(ses, b) for b in range(3)]
    table = [ses.anchors(b) for b in range(3)]
    lib = ses.lib

    def call(slot, ids, handle=ses.handle):
        arr = (C.c_int * max(len(ids), 1))(*ids)
        rc = lib.vh_session_set_anchors(handle, slot, arr, len(ids), None, L.stream_ptr())
        return rc, lib.vh_last_error().decode()

    for (slot, ids), words in (((3, [1]), ("slot 3", "3 slots")), ((-1, [1]), ("slot -1", "3 slots")), ((0, [1, N0]), (f"id {N0}", f"[0, {N0})")),
                               ((0, [-2]), ("id -2", f"[0, {N0})")), ((1, [7, 8, 7]), ("id 7", "twice")),
                               ((2, list(range(N0)) + [0]), (f"n = {N0 + 1}", f"{N0} tracks"))):
        rc, msg = call(slot, ids)
        assert rc == -1 and "vh_session_set_anchors" in msg and all(w in msg for w in words), (slot, ids[:4], msg)
    fresh = TrackerSession(_noisy3()[0][4], 320, 240, N0, nhist=NHIST, batch=2, msv_frame=5)
    rc, msg = call(1, [1, 2], fresh.handle)
    assert rc == -1 and "slot 1" in msg and "not initialised" in msg
    with pytest.raises(RuntimeError, match="twice"):
        ses.set_anchors(0, [5, 5])
    with pytest.raises(ValueError, match="xyz"):
        ses.set_anchors(0, [5, 6], np.zeros((3, 3)))
    assert [raw_export(ses, b) for b in range(3)] == before
    for b in range(3):
        assert all(np.array_equal(a, c) for a, c in zip(ses.anchors(b), table[b]))
    ses.set_anchors(2, [9, 8])  # the next valid call works
    assert ses.anchors(2)[0].tolist() == [8, 9] and np.array_equal(ses.anchors(2)[1], ses.state(2)["p3"][[8, 9]])


# ---- the drivers' refine_anchor="plate" -------------------------------------------------------------------------------------------------------------------
KW = dict(roi_border=(60, 40), max_corners=150)


def _plate_anchors(c):
    """What refine_anchor="plate" anchors: the frame-0 world points of tracks 0..3 (frame0_batch: the 4 plate corners come first)."""
    from velocity_amd.driver import frame0_batch

    return np.arange(4), frame0_batch(c["frames"][:1], [c["q"]], c["K"], **KW)[0]["p3"][:4]


def _ba_close(g, one, where):
    assert g["nt"] == one["nt"] > 0 and g["nfix"] == one["nfix"] and np.array_equal(g["ids"], one["ids"]), where
    assert g["iterations"] == one["iterations"] and g["converged"] == one["converged"], where
    for key in ("cw", "pw", "dr", "speed", "speed_mean", "speed_std"):
        np.testing.assert_allclose(g[key], one[key], rtol=1e-6, atol=1e-8, equal_nan=True, err_msg=f"{where}: {key}")


def test_run_sequence_refine_anchor_plate():
    from velocity_amd import driver as D

    c = S.plate_clip(320, 240, 700.0, 8, 501, "synthetic 320 x 240")
    args = dict(times=c["times"], clock=lambda: 0.0, name=c["name"], **KW)
    free, printed = D.run_sequence(c["frames"], c["q"], c["K"], out=None, refine="ba", **args), []
    got = D.run_sequence(c["frames"], c["q"], c["K"], out=printed.append, refine="ba", refine_anchor="plate", **args)
    anchors = _plate_anchors(c)
    ref = AR.refine_anchored_ref(c["K"], got["P"], got["p3"], got["B"], 8, anchors)
    _equals_model(got["ba"], ref, c["name"])
    alive = len(set(got["ba"]["ids"]) & {0, 1, 2, 3})
    assert got["ba"]["nfix"] == alive >= 1 and got["ba"]["anchor"] == "plate" and "anchor" not in free["ba"] and free["ba"]["nfix"] == 0
    for key in ("S", "B", "P", "vg", "p3", "ids", "vp", "p"):  # the tracker's results do not know about the anchors
        assert np.array_equal(np.asarray(got[key]), np.asarray(free[key]), equal_nan=True), key
    line = D.ba_line(got["ba"])
    assert f"({got['ba']['nt']} tracks, {alive} anchors, f = " in line and got["lines"][:-1] == free["lines"][:-1] and got["lines"][-1] == line
    assert printed == got["lines"] and " anchors" not in free["lines"][-1] and free["lines"][-1] == D.ba_line(free["ba"])
    assert not np.array_equal(got["ba"]["cw"], free["ba"]["cw"])
    # in windows: every window on the tracks alive through it, anchors placed by the tracker's B[first, 3:6]
    W, starts = 4, D.refine_window_starts(8, 4)
    win = D.run_sequence(c["frames"], c["q"], c["K"], out=None, refine="ba", refine_window=W, refine_anchor="plate", **args)
    model = D.merge_window_speeds(8, [AR.refine_window_anchored_ref(c["K"], win["P"], win["p3"], win["B"], f, W, anchors) for f in starts])
    for key in ("first", "nt", "nfix", "iterations", "converged", "cover"):
        assert np.array_equal(win["ba"][key], model[key]), (key, win["ba"][key], model[key])
    for key in ("speed", "speed_mean", "speed_std", "f_last"):
        np.testing.assert_allclose(win["ba"][key], model[key], rtol=1e-6, atol=1e-8, equal_nan=True, err_msg=key)
    assert win["ba"]["nfix"].min() >= 1 and f"tracks, {win['ba']['nfix'].min()}-{win['ba']['nfix'].max()} anchors, f = " in win["lines"][-1]
    with pytest.raises(ValueError, match="refine_anchor needs refine='ba'"):
        D.run_sequence(c["frames"], c["q"], c["K"], out=None, refine_anchor="plate", **args)


def test_run_queue_and_run_sequences_refine_anchor_plate():
    """The clips of test_gpu_refine.py's queue test: each clip's anchored refinement from run_queue and run_sequences equals run_sequence's alone, at
    that test's tolerances; a slot's anchors are its current clip's."""
    from velocity_amd import driver as D

    cams = ((320, 240, 700.0), (256, 192, 560.0))
    clips = [S.plate_clip(*cams[k % 2], n, 600 + k, f"clip {k}") for k, n in enumerate((6, 8, 8, 6, 7))]
    K0 = S.camera(320, 240, 650.0)
    alone = [D.run_sequence(c["frames"], c["q"], c["K"], times=c["times"], out=None, live=False, name=c["name"], refine="ba", refine_anchor="plate", **KW)
             for c in clips]
    got = D.run_queue(clips, K0, streams=2, sessions=1, max_size=(240, 320), refine="ba", refine_anchor="plate", **KW)
    for c, g, one in zip(clips, got, alone):
        _ba_close(g["ba"], one["ba"], c["name"])
        assert g["lines"][-1] == one["lines"][-1] and " anchors, f = " in g["lines"][-1] and g["ba"]["nfix"] >= 1
    both = D.run_sequences([clips[1], clips[2]], K0, sessions=1, refine="ba", refine_anchor="plate", **KW)
    for c, g, one in zip((clips[1], clips[2]), both, (alone[1], alone[2])):
        _ba_close(g["ba"], one["ba"], c["name"])
        assert g["lines"][-1] == one["lines"][-1]
    winq = D.run_queue(clips[:3], K0, streams=2, sessions=1, max_size=(240, 320), refine="ba", refine_window=4, refine_anchor="plate", **KW)
    for c, g in zip(clips[:3], winq):
        one = D.run_sequence(c["frames"], c["q"], c["K"], times=c["times"], out=None, live=False, name=c["name"], refine="ba", refine_window=4,
                             refine_anchor="plate", **KW)
        for key in ("first", "nt", "nfix", "iterations", "converged", "cover"):
            assert np.array_equal(g["ba"][key], one["ba"][key]), (c["name"], key)
        np.testing.assert_allclose(g["ba"]["speed"], one["ba"]["speed"], rtol=1e-6, atol=1e-8, equal_nan=True, err_msg=c["name"])
