"""Bundle adjustment of frame windows with tracks that live through PART of a window (vh_session_refine_windows_partial,
TrackerSession.refine_windows(min_obs=...), NLS.fcnNLS_batch(min_obs=...), the drivers' refine_min_obs) against the NumPy model
tests/refine_partial_ref.py.  Without the feature the whole file fails: the symbol is missing.

Tolerances: those of tests/test_gpu_refine_windows.py and tests/test_gpu_anchor.py -- ids and every count exact, iterations and converged equal, the
rest within rtol 1e-6 / atol 1e-8, the first column of the trace within rtol 1e-6.  Gates: every scene asserts ON THE MODEL that no candidate's
reprojection error lies within 1e-3 pixels of start_reproj, so a device rounding cannot flip a decision."""
import ctypes as C

import numpy as np
import pytest

import anchor_ref as AR
import refine_partial_ref as RP
import replenish_scenes as RS
import scenes as S
from scenes import T0
from session_support import raw_export, same_dict, session_at, step_to
from velocity_amd import synth

pytestmark = pytest.mark.gpu

N0, NHIST, AT, W4 = 150, 12, 8, 4
PATCH = (0, 0, 120, 240)  # of stream 2, from frame 4 on: the tracks inside die there (tests/test_gpu_refine_windows.py: 128 -> 95)
NEVER = 20                # an MSV frame the 12-frame clips never reach: "a clip cut before the MSV frame"
_SES = {}
INTS = ("nt", "nfix", "nobs", "npart", "ntri", "nrej", "iterations", "converged")


def _patched3():
    return S.scenes3(N0, NHIST, patch=PATCH)


def _ses8(msv=5):
    """THE session (per MSV frame) of the tests that only read it: the three patched scenes at frame AT = 8, with the host states."""
    if msv not in _SES:
        ses = session_at(_patched3(), AT, msv_frame=msv)
        _SES[msv] = (ses, [ses.state(b) for b in range(3)])
    return _SES[msv]


def _model(K, st, first, nf, msv, min_obs, start_reproj=0.0, anchors=None, replenished=False):
    ref = RP.refine_partial_ref(K, st["P"], st["p3"], st["B"], first, nf, st["frame_i"], msv, min_obs, start_reproj, anchors=anchors,
                                tri=st["tri"] if replenished else None)
    err = ref["sel"]["err"]
    assert not (np.abs(err[np.isfinite(err)] - start_reproj) < 1e-3).any(), "a gate decision of this scene is a near-tie"
    return ref


def _equals(got, ref, nf, where):
    print(f"{where}: " + ", ".join(f"{k} {got[k]} / {ref[k]}" for k in INTS) + f", speed {got['speed_mean']:.4f} (model {ref['speed_mean']:.4f}), "
          f"max |dcw| {np.abs(got['cw'] - ref['cw']).max():.3g}" + (f", max |dpw| {np.abs(got['pw'] - ref['pw']).max():.3g}" if ref["nt"] else ""))
    assert np.array_equal(got["ids"], ref["ids"]), where
    for k in INTS:
        assert got[k] == ref[k], (where, k, got[k], ref[k])
    for key in ("cw", "pw", "dr", "speed", "speed_mean", "speed_std"):
        np.testing.assert_allclose(got[key], ref[key], rtol=1e-6, atol=1e-8, equal_nan=True, err_msg=f"{where}: {key}")
    np.testing.assert_allclose(got["trace"][:, 0], ref["trace"][:, 0], rtol=1e-6, err_msg=where)
    if ref["nt"]:
        assert got["f_first"] == got["trace"][0, 0] and got["f_last"] == got["trace"][-1, 0], where
    else:
        assert np.isnan(got["f_first"]) and np.isnan(got["f_last"]) and got["trace"].shape == (0, 2), where
    assert got["cw"].shape == (nf, 3) and np.all(got["cw"][0] == 0) and np.isnan(got["speed"][0]), where


def test_partial_windows_of_three_slots_equal_the_model():
    """Two cameras, different `first`, one call; stream 2 loses its patch at frame 4, so its windows around that frame hold partial tracks.  Those die
    before the MSV frame 5 and are no pose tracks: they enter only with a triangulated start."""
    ses, st = _ses8()
    scenes = _patched3()
    wins = [(0, 0), (0, 3), (1, 1), (2, 0), (2, 2), (2, 5), (1, 4)]
    got = ses.refine_windows(wins, W4, with_points=True, min_obs=2, start_reproj=0.1).result()
    bare = ses.refine_windows(wins, W4, with_points=True, min_obs=2).result()
    full = ses.refine_windows(wins, W4).result()
    for (b, f), g, n, o in zip(wins, got, bare, full):
        assert (g["slot"], g["first"]) == (b, f)
        _equals(g, _model(scenes[b][4], st[b], f, W4, 5, 2, 0.1), W4, f"window ({b}, {f})")
        _equals(n, _model(scenes[b][4], st[b], f, W4, 5, 2), W4, f"window ({b}, {f}) without starts")
        assert g["nt"] >= n["nt"] >= o["nt"] and g["nt"] - g["npart"] == o["nt"] and n["ntri"] == n["nrej"] == 0 and n["nt"] == g["nt"] - g["ntri"]
    assert got[4]["npart"] >= 10 and got[4]["ntri"] >= 10 and got[4]["nobs"] < got[4]["nt"] * W4  # (2, 2): the dying tracks are seen in frames 2 and 3 only
    lean = ses.refine_windows(wins, W4, min_obs=2, start_reproj=0.1).result()
    for g, l in zip(got, lean):
        assert "ids" not in l and all(l[k] == g[k] for k in INTS) and np.array_equal(l["cw"], g["cw"])


def test_min_obs_nf_without_starts_is_the_windows_entry_byte_for_byte():
    ses, _ = _ses8()
    wins = [(0, 1), (1, 0), (2, 2), (2, 5)]
    new, old = ses.refine_windows(wins, W4, with_points=True, min_obs=W4), ses.refine_windows(wins, W4, with_points=True)
    rn, ro = new.result(), old.result()
    ln, lo = new.layout, old.layout
    assert ln.bytes == lo.bytes + 16 and (ln.nobs, ln.npart, ln.ntri, ln.nrej) == tuple(lo.bytes + 4 * k for k in range(4))
    assert all(getattr(ln.win, k) == getattr(lo, k) for k, _ in type(lo)._fields_ if k != "bytes")
    loose = np.zeros(lo.bytes, bool)  # the trace and the two residuals copied from it: sums of squares accumulated with atomics
    loose[lo.trace:lo.trace + 16 * lo.max_iter] = True
    loose[lo.f_first:lo.f_first + 8] = loose[lo.f_last:lo.f_last + 8] = True
    for k, (a, b) in enumerate(zip(rn, ro)):
        ra, rb = new.bufs[k].numpy()[: lo.bytes], old.bufs[k].numpy()[: lo.bytes]
        assert np.array_equal(ra[~loose], rb[~loose]), wins[k]
        np.testing.assert_allclose(a["trace"], b["trace"], rtol=1e-12)
        assert (a["nobs"], a["npart"], a["ntri"], a["nrej"]) == (a["nt"] * W4, 0, 0, 0) and a["nt"] > 0


def test_triangulated_starts_on_a_clip_cut_before_the_msv_frame_and_anchors():
    """No track of these clips is trusted beyond the pose tracks: the partial ones are candidates; the gate of 0.1 pixels admits most and rejects some."""
    ses, st = _ses8(NEVER)
    scenes = _patched3()
    wins = [(2, 2), (2, 1), (0, 2), (2, 5)]
    got = ses.refine_windows(wins, W4, with_points=True, min_obs=2, start_reproj=0.1).result()
    for (b, f), g in zip(wins, got):
        _equals(g, _model(scenes[b][4], st[b], f, W4, NEVER, 2, 0.1), W4, f"window ({b}, {f}) with starts")
    assert got[0]["ntri"] >= 10 and got[0]["nrej"] >= 1 and got[0]["npart"] >= got[0]["ntri"]
    none = ses.refine_windows(wins[:1], W4, with_points=True, min_obs=2).result()[0]  # start_reproj = 0: the candidates stay out
    _equals(none, _model(scenes[2][4], st[2], 2, W4, NEVER, 2), W4, "window (2, 2) without starts")
    assert none["nt"] == got[0]["nt"] - got[0]["ntri"] and none["ntri"] == none["nrej"] == 0
    # anchors: an anchored track is trusted (B) and held fixed; two candidates of above and two full-length tracks
    sel = RP.select_partial(scenes[2][4], st[2]["P"], st[2]["B"], 2, W4, AT, NEVER, 2, 0.1)
    ids = np.concatenate((np.flatnonzero(sel["kind"] == "C")[:2], np.flatnonzero(sel["kind"] == "A")[:2])).astype(np.int32)
    ses.set_anchors(2, ids)  # (their p3 rows: what frame 0 gave them)
    try:
        anchors = (ids, st[2]["p3"][ids])
        g = ses.refine_windows([(2, 2)], W4, with_points=True, min_obs=2, start_reproj=0.1).result()[0]
        ref = _model(scenes[2][4], st[2], 2, W4, NEVER, 2, 0.1, anchors=anchors)
        _equals(g, ref, W4, "window (2, 2) with anchors")
        assert g["nfix"] == 4 and g["ntri"] == got[0]["ntri"] - 2 and g["nt"] == got[0]["nt"]
        rows = np.isin(g["ids"], ids)
        assert np.array_equal(g["pw"][rows], st[2]["p3"][ids[np.argsort(ids)]] + st[2]["B"][2, 3:6].astype(np.float64))  # anchored rows come back as given
    finally:
        ses.set_anchors(2, [])


def test_a_replenished_session_spare_rows_included():
    """Rows born mid-clip: promoted ones are trusted once they have been pose tracks, rejected and not-yet-judged ones are candidates."""
    from test_gpu_replenish import _session, _step

    sc = RS.scene()
    ses = _session([sc], replenish=RS.REP_STRICT)
    for k in range(1, 11):
        _step(ses, [sc], [k])
    st = ses.state(0)
    assert ses.n0 == len(sc["p"]) + RS.SPARE and st["n_rows"] > len(sc["p"])
    for (first, nf), gate in (((3, 8), 0.0175), ((7, 4), 0.008), ((3, 8), 0.0), ((0, 8), 0.0057)):
        g = ses.refine_windows([(0, first)], nf, with_points=True, min_obs=2, start_reproj=gate).result()[0]
        ref = _model(sc["K"], st, first, nf, RS.MSV_FRAME, 2, gate, replenished=True)
        _equals(g, ref, nf, f"replenished, window ({first}, {nf}), gate {gate}")
        newborn = st["born"][g["ids"]] > 0
        assert newborn.any() and g["npart"] > 0
        assert (gate == 0.0) == (g["ntri"] == 0) and (gate == 0.0) == (g["nrej"] == 0)


def _big_scene():
    """590 rows (more than two 256-id blocks, not a multiple of 64) of which ids 256..511 -- a whole block -- never live; and a stream of none at all."""
    frames, p, p3, vp, K = S.plane_scene(320, 240, 590, NHIST, 433, 700.0, hopeless=7, patch=PATCH)
    p = np.array(p)
    p[256:512] = np.float32([-40.0, -40.0])
    return [(frames, p, p3, vp, K), (frames, np.full_like(p, -40.0), p3, vp, K)]


def test_more_than_256_rows_an_empty_block_and_an_empty_window():
    scenes = _big_scene()
    ses = session_at(scenes, 6, msv_frame=NEVER)
    st = [ses.state(b) for b in range(2)]
    assert st[1]["n_cur"] == 0 and st[0]["n_cur"] > 128
    wins = [(0, 1), (1, 1), (0, 3), (1, 0)]
    got = ses.refine_windows(wins, W4, with_points=True, min_obs=2, start_reproj=0.1).result()
    for (b, f), g in zip(wins, got):
        _equals(g, _model(scenes[b][4], st[b], f, W4, NEVER, 2, 0.1), W4, f"590 rows, window ({b}, {f})")
    ids = got[0]["ids"]
    assert (ids < 256).any() and (ids >= 512).any() and not ((ids >= 256) & (ids < 512)).any() and np.all(np.diff(ids) > 0)
    assert got[0]["npart"] > 0 and got[1]["nt"] == got[3]["nt"] == 0 and got[1]["iterations"] == 0
    np.testing.assert_allclose(got[1]["cw"], st[1]["B"][1:5, 3:6].astype(np.float64) - st[1]["B"][1, 3:6].astype(np.float64), rtol=0, atol=0)


def test_the_session_is_only_read():
    ses, twin = session_at(_patched3(), 6), session_at(_patched3(), 6)
    before = [raw_export(ses, b) for b in range(3)]
    got = ses.refine_windows([(0, 1), (1, 2), (2, 3), (2, 1), (2, 2)], W4, with_points=True, min_obs=2, start_reproj=0.1).result()
    assert sum(g["npart"] for g in got) > 0
    assert [raw_export(ses, b) for b in range(3)] == before
    step_to(ses, _patched3(), 7, 9)
    step_to(twin, _patched3(), 7, 9)
    for b in range(3):
        same_dict(ses.state(b), twin.state(b), f"stream {b} three frames later")


def test_refusals_queue_nothing_and_name_the_limit():
    import torch

    from velocity_amd import _lib as L

    ses, _ = _ses8()
    lib = ses.lib
    lay = ses.refine_window_layout(W4, 10, True, partial=True)
    need = int(lib.vh_session_refine_windows_partial_workspace(ses.handle, 3, W4))
    assert need > int(lib.vh_session_refine_windows_workspace(ses.handle, 3, W4)) > 0 and lay.bytes % 8 == 0
    recs = torch.zeros(3 * lay.bytes + 8, dtype=torch.uint8, device="cuda")
    work = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")

    def call(wins, nf=W4, max_iter=10, nwin=None, nbytes=need, rec_off=0, work_off=0, min_obs=2, gate=0.0, params=True):
        tab = (L.RefineWindow * max(len(wins), 1))(*[L.RefineWindow(b, f) for b, f in wins])
        prm = L.RefinePartialParams(min_obs, gate)
        rc = lib.vh_session_refine_windows_partial(ses.handle, tab, len(wins) if nwin is None else nwin, nf, max_iter, 1, C.byref(prm) if params else None,
                                                   C.c_void_p(recs.data_ptr() + rec_off), C.c_void_p(work.data_ptr() + work_off), nbytes, L.stream_ptr())
        return rc, lib.vh_last_error().decode()

    ok = [(0, 1), (1, 1), (2, 1)]
    for kw, words in ((dict(wins=ok, min_obs=1), ("min_obs = 1", "at least 2")),
                      (dict(wins=ok, min_obs=W4 + 1), (f"min_obs = {W4 + 1}", f"nf = {W4}")),
                      (dict(wins=ok, gate=-0.5), ("start_reproj = -0.5", ">= 0")),
                      (dict(wins=ok, gate=float("nan")), ("start_reproj = nan", "finite")),
                      (dict(wins=ok, gate=float("inf")), ("start_reproj = inf", "finite")),
                      (dict(wins=ok, params=False), ("bad arguments", "parameters")),
                      (dict(wins=[(0, 1), (3, 0)]), ("slot 3", "3 slots")),
                      (dict(wins=[(0, 1), (1, 6)]), ("slot 1, first 6", "frame 9", "frame 8")),
                      (dict(wins=[(0, 1), (1, 1), (0, 1)]), ("slot 0, first 1", "twice")),
                      (dict(wins=ok, nf=1, min_obs=1), ("nf = 1", "two frames")),
                      (dict(wins=ok, nf=NHIST + 1), (f"nf = {NHIST + 1}", f"{NHIST} frames")),
                      (dict(wins=ok, max_iter=0), ("max_iter = 0",)),
                      (dict(wins=ok, nwin=0), ("nwin = 0",)),
                      (dict(wins=ok, rec_off=4), ("misaligned", "8-byte")),
                      (dict(wins=ok, work_off=8), ("misaligned", "256-byte")),
                      (dict(wins=ok, nbytes=need - 1), ("workspace", str(need)))):
        rc, msg = call(**kw)
        assert rc == -1 and "vh_session_refine_windows_partial" in msg and all(w in msg for w in words), (kw, msg)
    with pytest.raises(RuntimeError, match="min_obs = 9"):
        ses.refine_windows(ok, W4, min_obs=9)
    with pytest.raises(ValueError, match="start_reproj needs min_obs"):
        ses.refine_windows(ok, W4, start_reproj=1.0)
    torch.cuda.synchronize()
    assert not recs.any().item() and not work.any().item()  # nothing was queued: neither buffer was written
    rc, msg = call(ok)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert recs[: 3 * lay.bytes].any().item()


# ---- the drop-in route -----------------------------------------------------------------------------------------------------------------------------
ROUTES = pytest.mark.parametrize("nf,force_valu", [(4, 0), (22, 0), (24, 0), (22, 1), (44, 0)],
                                 ids=["gj-mfma", "gj-valu-solve", "cholesky", "valu-schur", "zbuild-syrk"])


def _holey(nt, nf, seed, missing):
    """synth.ba_scene with runs of frames cut out of every track but the first four (which are anchored in the tests: a free window with this many holes
    does not hold the tolerances model against model, see tests/test_gpu_anchor.py::_route), camera 2 seen by nobody and track 5 seen exactly twice.
    The start is a fifth of ba_scene's default distance from the truth: from the default one the NumPy model does not reproduce ITS OWN trace to the
    1e-8 asked below when only the order of the tracks changes (up to 1.4e-7 over these twelve scenes; from this start 1.4e-9 at worst)."""
    K = synth.K_1080P.astype(np.float64)
    P, pw0, cw0 = synth.ba_scene(nt, nf, seed=seed, K=K, sigma_pts=0.01, sigma_cams=0.004)
    full = P.copy()
    rng = np.random.default_rng(seed)
    for g in range(4, nt):
        n = int(round(missing * nf * rng.uniform(0.8, 1.2)))
        lo = int(rng.integers(0, nf - n + 1))
        P[:, g, lo:lo + n] = np.nan
    P[:, :, 2] = np.nan
    P[:, 5] = np.nan
    P[:, 5, 0] = full[:, 5, 0]
    P[:, 5, nf - 1] = full[:, 5, nf - 1]
    return K, P, pw0, cw0


def _dropin_model(K, P, pw0, cw0, min_obs, fixed):
    nf = P.shape[2]
    ids = np.flatnonzero(np.isfinite(P[4]).sum(1) >= min_obs)
    B = np.zeros((nf, 14))
    B[:, 3:6] = cw0
    z, bad, x0, _ = RP.pack_partial(P, pw0, B, ids)
    x, tr = AR.solve_anchored(K, z, bad, x0, len(ids), len(ids), nf - 1, fixed=fixed[ids], max_iter=10)
    return ids, x, tr


@ROUTES
def test_the_drop_in_calls_take_min_obs_on_every_route(nf, force_valu, capsys):
    from velocity_amd import NLS
    from velocity_amd import _lib as L

    nt = 24
    cases = [_holey(nt, nf, 700 + nf + w, m) for w, m in enumerate((0.33, 0.45, 0.55))]
    fixed = np.arange(nt) < 4
    for K, P, _, _ in cases:
        miss = 1.0 - np.isfinite(P[4]).mean()
        assert 0.3 <= miss <= 0.6 and not np.isfinite(P[4, :, 2]).any() and np.isfinite(P[4, 5]).sum() == 2
    L.load().vh_debug_ba_force_valu(force_valu)
    try:
        one = NLS.fcnNLS_batch(cases[0][0], *cases[0][1:], return_info=True, fixed=fixed, min_obs=2)
        many = NLS.fcnNLS_batch_windows(cases[0][0], [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], return_info=True,
                                        fixed=[fixed] * 3, min_obs=2)
    finally:
        L.load().vh_debug_ba_force_valu(0)
    capsys.readouterr()
    for w, (K, P, pw0, cw0) in enumerate(cases):
        ids, mx, mtr = _dropin_model(K, P, pw0, cw0, 2, fixed)
        n = len(ids)
        assert 5 in ids
        for name, (cw, pw, x, tr) in (("windows", many[w]),) + ((("single", one),) if w == 0 else ()):
            gx = np.concatenate((x[: 3 * n], x[len(x) - 6 * (nf - 1):]))
            print(f"nf={nf} valu={force_valu} {name} {w}: {n} tracks, iterations {len(tr)} / {len(mtr)}, max |dx| {np.abs(gx - mx).max():.3g}")
            assert len(pw) == n and len(tr) == len(mtr), (name, w)
            np.testing.assert_allclose(gx, mx, rtol=1e-6, atol=1e-8, err_msg=f"{name} {w}")
            np.testing.assert_allclose(tr[:, 0], mtr[:, 0], rtol=1e-8, err_msg=f"{name} {w}")
            np.testing.assert_allclose(cw[1:], mx[3 * n:3 * n + 3 * (nf - 1)].reshape(-1, 3), rtol=1e-6, atol=1e-8)


# ---- the drivers -----------------------------------------------------------------------------------------------------------------------------------
KW = dict(roi_border=(60, 40), max_corners=150)


def _clip_model(c, res, nf, starts, min_obs, gate, msv=5, anchors=None):
    n = len(c["frames"])
    st = dict(P=res["P"], p3=res["p3"], B=res["B"], frame_i=n - 1)
    return [_model(c["K"], st, f, nf, msv, min(min_obs, nf), gate, anchors=anchors) for f in starts]


def test_the_drivers_take_refine_min_obs():
    from velocity_amd import driver as D

    cams = ((320, 240, 700.0), (256, 192, 560.0))
    clips = [S.plate_clip(*cams[k % 2], n, 700 + k, f"clip {k}") for k, n in enumerate((9, 12, 9))]
    K0 = S.camera(320, 240, 650.0)
    for win in (None, W4):
        alone = [D.run_sequence(c["frames"], c["q"], c["K"], times=c["times"], out=None, live=False, name=c["name"], refine="ba", refine_window=win,
                                refine_min_obs=3, refine_start_reproj=0.1, **KW) for c in clips]
        for c, one in zip(clips, alone):
            n = len(c["frames"])
            nf = n if win is None else win
            starts = [0] if win is None else D.refine_window_starts(n, win)
            ba, model = one["ba"], _clip_model(c, one, nf, starts, 3, 0.1)
            assert ba["window"] == nf and list(ba["first"]) == starts
            for key in ("nt", "nobs", "npart", "ntri", "nrej", "iterations", "converged"):
                assert list(ba[key]) == [m[key] for m in model], (c["name"], win, key)
            want = D.merge_window_speeds(n, model)
            for key in ("speed", "speed_mean", "speed_std", "f_last"):
                np.testing.assert_allclose(ba[key], want[key], rtol=1e-6, atol=1e-8, equal_nan=True, err_msg=f"{c['name']}: {key}")
            assert one["lines"][-1] == D.ba_line(ba) and f"{int(ba['npart'].sum())} partial" in one["lines"][-1] and "starts triangulated" in one["lines"][-1]
        many = D.run_sequences([clips[0], clips[2]], K0, sessions=1, refine="ba", refine_window=win, refine_min_obs=3, refine_start_reproj=0.1, **KW)
        queue = D.run_queue(clips, K0, streams=2, sessions=1, max_size=(240, 320), refine="ba", refine_window=win, refine_min_obs=3, refine_start_reproj=0.1, **KW)
        for got, ones in ((many, [alone[0], alone[2]]), (queue, alone)):
            assert len(got) == len(ones)
            for g, one in zip(got, ones):
                for key in ("first", "nt", "nobs", "npart", "ntri", "nrej", "iterations", "converged"):
                    assert np.array_equal(g["ba"][key], one["ba"][key]), key
                np.testing.assert_allclose(g["ba"]["speed"], one["ba"]["speed"], rtol=1e-6, atol=1e-8, equal_nan=True)
                assert g["lines"][-1].startswith("BA speed = ") and " partial" in g["lines"][-1]
    # anchored: the plate corners are held fixed as today
    c = clips[0]
    one = D.run_sequence(c["frames"], c["q"], c["K"], times=c["times"], out=None, live=False, name=c["name"], refine="ba", refine_window=W4, refine_min_obs=3,
                         refine_anchor="plate", **KW)
    old = D.run_sequence(c["frames"], c["q"], c["K"], times=c["times"], out=None, live=False, name=c["name"], refine="ba", refine_window=W4,
                         refine_anchor="plate", **KW)
    assert np.array_equal(one["ba"]["nfix"], old["ba"]["nfix"]) and one["ba"]["nfix"].min() == 4 and "4-4 anchors" in one["lines"][-1]
    # without the option: the dicts and the lines are what they were
    plain = D.run_sequence(c["frames"], c["q"], c["K"], times=c["times"], out=None, live=False, name=c["name"], refine="ba", refine_window=W4, **KW)
    assert "nobs" not in plain["ba"] and "partial" not in plain["lines"][-1] and plain["lines"][-1] == D.ba_line(plain["ba"])
    assert sorted(plain["ba"]) == ["converged", "cover", "f_last", "first", "iterations", "nfix", "nt", "speed", "speed_mean", "speed_std", "stride", "window"]
