"""Refinement of windows with tracks that live through part of them, the parts that need no GPU: the NumPy model (tests/refine_partial_ref.py) against
the full-length model, its selection rule case by case, the host packers (NLS.pack_windows(min_obs=)), the gates of the GPU scenes, the truth
experiment, the binding and the drivers' refusals."""
import numpy as np
import pytest

import refine_partial_ref as RP
import refine_window_ref as RW
from test_refine_windows_cpu import _clip
from velocity_amd import synth


def _dying_clip():
    K, P, p3, B = _clip()
    P[:, 5, 7:] = np.nan    # the window tests' deaths: track 5 dies at frame 7, track 9 at frame 4, track 11 never lived
    P[:, 9, 4:] = np.nan
    P[:, 11, :] = np.nan
    return K, P, p3, B


@pytest.mark.parametrize("clip", [_clip, _dying_clip])
@pytest.mark.parametrize("first,nf", [(0, 9), (2, 4), (0, 4), (5, 4), (3, 2)])
def test_min_obs_nf_without_starts_is_the_window_model_bit_for_bit(clip, first, nf):
    K, P, p3, B = clip()
    a, b = RP.refine_partial_ref(K, P, p3, B, first, nf, 8, 5, nf), RW.refine_window_ref(K, P, p3, B, first, nf)
    assert a["nt"] == b["nt"] > 0 and a["iterations"] == b["iterations"] > 0 and a["converged"] == b["converged"] and a["first"] == b["first"]
    for key in ("ids", "cw", "pw", "trace", "dr", "speed"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    for key in ("speed_mean", "speed_std", "f_first", "f_last"):
        assert a[key] == b[key], key
    assert (a["nobs"], a["npart"], a["ntri"], a["nrej"], a["nfix"]) == (a["nt"] * nf, 0, 0, 0, 0)


def _history(n=12, nh=10):
    """A history of n tracks alive in all nh frames (rows 0, 1, 4; row 2 NaN: nobody is a pose track yet), its B, and the camera."""
    K = synth.K_1080P.astype(np.float64)
    P, p3, cw0 = synth.ba_scene(n, nh, seed=5, K=K)
    P = P.astype(np.float32)
    P[2:4] = np.nan
    B = np.zeros((nh, 14), np.float32)
    B[1:, 3:6] = cw0[1:]
    B[:, 0:3] = np.float32([1.0, 0.5, 4.0]) + B[:, 3:6]  # B[i, 0:3] = B[0, 0:3] + t_i (vidExample.py:145)
    B[:, 12] = np.arange(nh, dtype=np.float32) / np.float32(25.0)
    return K, P, p3, B


def test_the_selection_rule_case_by_case():
    K, P, p3, B = _history()
    FIRST, NF, I, MSV, M = 2, 6, 9, 5, 3  # the window: frames 2..7
    P[:, 0, 5:] = np.nan                      # 0: obs == min_obs, died before the MSV frame, was a pose track
    P[2:4, 0, 1:3] = P[0:2, 0, 1:3]
    P[:, 1, 4:] = np.nan                      # 1: obs == min_obs - 1, pose track: too few observations
    P[2:4, 1, 1:3] = P[0:2, 1, 1:3]
    P[:, 2, 5:] = np.nan                      # 2: died before the MSV frame, never a pose track: untrusted
    P[:, 3, 6:] = np.nan                      # 3: alive at the MSV frame and dead the next: re-triangulated
    P[:, 4, :4] = np.nan                      # 4: born at frame 4 (a replenished row), promoted: a pose track from frame 8 on
    P[2:4, 4, 8:] = P[0:2, 4, 8:]
    P[:, 5, :6] = np.nan                      # 5: born at frame 6, rejected or not yet judged: no pose frame, not alive at the MSV frame
    P[:, 6, 5:] = np.nan                      # 6: like 2, but anchored
    P[:, 7, :] = np.nan                       # 7: never lived
    anchored = np.zeros(12, bool)
    anchored[6] = True
    tri = np.ones(12, np.uint8)
    tri[5] = 0
    tri[8] = 0                                # 8: full length but not triangulated (a replenished session): not A; trusted only through the MSV frame
    sel = RP.select_partial(K, P, B, FIRST, NF, I, MSV, M, 0.0, anchored, tri)
    assert "".join(k or "-" for k in sel["kind"]) == "B--BB-B-BAAA"
    assert list(sel["ids"]) == [0, 3, 4, 6, 8, 9, 10, 11] and list(sel["obs"][:9]) == [3, 2, 3, 4, 4, 2, 3, 0, 6]
    assert (sel["nobs"], sel["npart"], sel["ntri"], sel["nrej"]) == (3 + 4 + 4 + 3 + 6 + 18, 4, 0, 0)
    # before the MSV frame has run (i = 4 < msv is impossible for this window; msv = -1 or msv > i: no re-triangulation) track 3 is untrusted
    for msv in (-1, 20):
        assert list(RP.select_partial(K, P, B, FIRST, NF, I, msv, M, 0.0, anchored, tri)["kind"][[3, 8]]) == ["", ""]
    # a pose frame after the slot's counter does not count
    assert [RP.select_partial(K, P, B, FIRST, NF, i, -1, M, 0.0, anchored, tri)["kind"][4] for i in (7, 8, 9)] == ["", "B", "B"]
    # with starts the untrusted ones are candidates (the scene's pixels carry noise: a generous gate admits them, a tight one rejects them)
    wide = RP.select_partial(K, P, B, FIRST, NF, I, MSV, 2, 50.0, anchored, tri)
    assert "".join(k or "-" for k in wide["kind"]) == "BBCBBCB-BAAA" and wide["ntri"] == 2 and wide["nrej"] == 0
    tight = RP.select_partial(K, P, B, FIRST, NF, I, MSV, 2, 1e-9, anchored, tri)
    assert "".join(k or "-" for k in tight["kind"]) == "BBrBBrB-BAAA" and tight["ntri"] == 0 and tight["nrej"] == 2 and list(tight["ids"]) == [0, 1, 3, 4, 6, 8, 9, 10, 11]
    assert "".join(k or "-" for k in RP.select_partial(K, P, B, FIRST, NF, I, -1, 2, 50.0, anchored, tri)["kind"]) == "BBCCBCB-CAAA"
    # the start of a candidate: from its first and last observed frame of the window, whatever lies between
    c, err = RP.two_view_start(K, P, B, 2, 2, 4)
    assert np.array_equal(wide["start"][2], c) and wide["err"][2] == err and np.isfinite(c).all()
    # an empty window: not solved, the tracker's positions
    P[4] = np.nan
    out = RP.refine_partial_ref(K, P, p3, B, FIRST, NF, I, MSV, 2, 1.0)
    assert out["nt"] == 0 and out["iterations"] == 0 and out["trace"].shape == (0, 2) and np.isnan(out["f_last"])
    assert np.array_equal(out["cw"], B[2:8, 3:6].astype(np.float64) - B[2, 3:6].astype(np.float64))
    with pytest.raises(AssertionError):
        RP.select_partial(K, P, B, FIRST, NF, I, MSV, 1)
    with pytest.raises(AssertionError):
        RP.select_partial(K, P, B, FIRST, NF, I, MSV, NF + 1)


def test_pack_windows_min_obs_equals_the_models_z():
    from velocity_amd.NLS import pack_windows

    K, P, p3, B = _history(n=10, nh=6)
    P = P.astype(np.float64)
    P[4, 1, 2] = np.nan          # a gap in a track: rows 0/1 still hold pixels there, row 4 says "not observed"
    P[:, 2, 3:] = np.nan
    P[:, 3, :5] = np.nan         # observed once
    P[4, :, 4] = np.nan          # a frame nobody observes
    cw = B[:, 3:6].astype(np.float64)
    fixed = np.arange(10) % 3 == 0
    for m in (2, 3, 5):
        z, x0, counts, nt, nc, fx = pack_windows([P, P[:, :7]], [p3, p3[:7]], [cw, cw], fixed=[fixed, None], min_obs=m)
        for w, n in enumerate((10, 7)):
            ids = np.flatnonzero(np.isfinite(P[4, :n]).sum(1) >= m)
            mz, bad, mx, _ = RP.pack_partial(P[:, :n], p3[:n], B.astype(np.float64), ids)
            assert counts[w] == len(ids) and nt == counts.max() and nc == 5
            zw = z[w].reshape(2, 6, nt)[:, :, :len(ids)].reshape(-1)
            assert np.array_equal(np.isnan(zw), bad) and np.array_equal(np.where(bad, 0.0, zw), mz)
            assert np.isnan(z[w].reshape(2, 6, nt)[:, :, len(ids):]).all() and np.isnan(z[w].reshape(2, 6, nt)[:, 4]).all()
            assert np.array_equal(np.concatenate((x0[w, :3 * len(ids)], x0[w, 3 * nt:])), mx)
            assert np.array_equal(fx[w, :len(ids)], fixed[ids] if w == 0 else np.zeros(len(ids), bool)) and not fx[w, len(ids):].any()
        assert 3 not in np.flatnonzero(np.isfinite(P[4]).sum(1) >= m) and (1 in np.flatnonzero(np.isfinite(P[4]).sum(1) >= m)) == (m <= 4)
    assert np.array_equal(pack_windows([P], [p3], [cw], min_obs=None)[2], [0])  # the reference's filter: nobody is alive in every frame
    for bad_m in (1, 7):
        with pytest.raises(ValueError, match=f"min_obs = {bad_m}"):
            pack_windows([P], [p3], [cw], min_obs=bad_m)


def _gate_cases():
    """(name, K, P, B, i, msv, tri, [(first, nf, gate)]) of the GPU scenes whose triangulated starts are gated (tests/test_gpu_refine_partial.py), from
    the CPU oracles of the same sessions."""
    import replenish_scenes as RS
    import scenes as S
    from oracle.session_oracle import SessionOracle
    from replenish_ref import ReplenishOracle

    frames, p, p3, vp, K = S.scenes3(150, 12, patch=(0, 0, 120, 240))[2]
    for msv in (5, 20):
        orc = SessionOracle(K, frames[0], p, p3, vp, S.T0, time0=20.0, nhist=12, msv_frame=msv)
        for k in range(1, 9):
            orc.step(frames[k], np.float32(20.0 + k / 27.0), k)
        yield f"patched stream, MSV frame {msv}", K, orc.P, orc.B, 8, msv, None, [(2, 4, 0.1), (1, 4, 0.1), (5, 4, 0.1)]
    sc = RS.scene()
    orc = ReplenishOracle(sc["K"], sc["frames"][0], sc["p"], sc["p3"], sc["vp"], RS.T0, RS.REP_STRICT, RS.DET, spare=RS.SPARE, nhist=RS.NHIST,
                          msv_frame=RS.MSV_FRAME)
    for k in range(1, 11):
        orc.step(sc["frames"][k], np.float32(k / 25.0), k)
    yield "replenished", sc["K"], orc.P, orc.B, 10, RS.MSV_FRAME, orc.tri, [(3, 8, 0.0175), (7, 4, 0.008), (0, 8, 0.0057)]


def test_no_gate_of_the_gpu_scenes_is_a_near_tie():
    seen = dict(C=0, r=0)
    for name, K, P, B, i, msv, tri, wins in _gate_cases():
        for first, nf, gate in wins:
            sel = RP.select_partial(K, P, B, first, nf, i, msv, 2, gate, tri=tri)
            err = sel["err"][np.isfinite(sel["err"])]
            print(f"{name}, window ({first}, {nf}), gate {gate}: {sel['ntri']} admitted, {sel['nrej']} rejected, nearest {np.abs(err - gate).min() if len(err) else np.inf:.4f}")
            assert not (np.abs(err - gate) < 1e-3).any(), (name, first, nf)
            seen["C"] += sel["ntri"]
            seen["r"] += sel["nrej"]
        assert seen["C"] > 0 and seen["r"] > 0, name  # both branches run on every scene set


def test_truth_partial_tracks_improve_the_median_step_error():
    """Measured on the model, not fixed in advance: 8 seeds of analytic windows (8 frames, 6 full-length and 34 partial tracks of 2..7 frames, 0.1 px
    noise).  Recorded in profiles/refine_partial/truth.json by tools/exp/refine_partial_truth.py; single seeds may go the other way."""
    full, part = [], []
    for seed in range(8):
        K, P, pw0, cw0, cw = RP.analytic_window(seed)
        a, na = RP.solve_analytic(K, P, pw0, cw0, 8)
        b, nb = RP.solve_analytic(K, P, pw0, cw0, 2)
        assert na == 6 and nb == 40 and np.isfinite(a).all() and np.isfinite(b).all()
        full.append(RP.step_error(a, cw))
        part.append(RP.step_error(b, cw))
    print(f"median worst relative step error: full-length only {np.median(full):.4f}, min_obs = 2 {np.median(part):.4f}; per seed {np.round(full, 4)} / {np.round(part, 4)}")
    assert np.median(part) < np.median(full)


def test_the_entry_points_are_declared_and_bound():
    import ctypes as C

    from velocity_amd import _lib as L

    lib, declared = L.load(), L.declared_symbols()
    for s in ("vh_session_refine_windows_partial_size", "vh_session_refine_windows_partial_workspace", "vh_session_refine_windows_partial"):
        assert s in declared and s in L._SIGS and hasattr(lib, s), s
    assert C.sizeof(L.RefinePartialParams) == 8 and C.sizeof(L.RefinePartialRecord) == C.sizeof(L.RefineWindowRecord) + 32
    assert [k for k, _ in L.RefinePartialRecord._fields_] == ["win", "nobs", "npart", "ntri", "nrej"]
    assert lib.vh_session_refine_windows_partial_size(None, 4, 10, 0, None) == 0 and b"vh_session_refine_windows_partial_size" in lib.vh_last_error()
    assert lib.vh_session_refine_windows_partial_workspace(None, 1, 4) == 0 and b"vh_session_refine_windows_partial_workspace" in lib.vh_last_error()
    prm = L.RefinePartialParams(2, 0.0)
    assert lib.vh_session_refine_windows_partial(None, None, 1, 4, 10, 0, C.byref(prm), None, None, 0, None) == -1 and b"bad arguments" in lib.vh_last_error()


@pytest.mark.parametrize("kw,words", [(dict(refine_min_obs=3), "refine_min_obs needs refine"),
                                      (dict(refine="ba", refine_min_obs=1), "refine_min_obs = 1"),
                                      (dict(refine="ba", refine_start_reproj=1.0), "refine_start_reproj needs refine_min_obs"),
                                      (dict(refine="ba", refine_min_obs=3, refine_start_reproj=-1.0), "refine_start_reproj = -1.0"),
                                      (dict(refine="ba", refine_min_obs=3, refine_start_reproj=float("nan")), "refine_start_reproj = nan")])
def test_the_drivers_refuse_bad_arguments_before_anything_is_queued(kw, words):
    from velocity_amd.driver import run_queue, run_sequence, run_sequences

    K = synth.K_1080P
    with pytest.raises(ValueError, match=words):
        run_sequence([None, None], None, K, fps=25.0, out=None, **kw)
    with pytest.raises(ValueError, match=words):
        run_sequences([dict(frames=[None, None], q=None, times=[0, 1])], K, **kw)
    with pytest.raises(ValueError, match=words):
        run_queue([dict(frames=[None, None], q=None, times=[0, 1])], K, streams=1, **kw)


def test_the_ba_line_and_dict_carry_the_counts_only_with_the_option():
    from velocity_amd.driver import _check_partial, _merged_ba, ba_line

    nan = np.nan
    wins = [dict(first=0, speed=np.array([nan, 10.0, 12.0]), nt=30, iterations=4, converged=1, f_last=0.5),
            dict(first=2, speed=np.array([nan, 20.0, 22.0]), nt=25, iterations=5, converged=1, f_last=0.75)]
    plain = _merged_ba(5, wins, 3, 2)
    assert "npart" not in plain and ba_line(plain) == "BA speed = 16.00 +/- 5.10 km/h (2 windows of 3 frames, 25-30 tracks, f = 0.750 pixels)"
    part = _merged_ba(5, [dict(w, nobs=70 + k, npart=6 + k, ntri=2 * k, nrej=k) for k, w in enumerate(wins)], 3, 2)
    assert list(part["npart"]) == [6, 7] and list(part["nobs"]) == [70, 71] and list(part["ntri"]) == [0, 2] and list(part["nrej"]) == [0, 1]
    assert ba_line(part) == ("BA speed = 16.00 +/- 5.10 km/h (2 windows of 3 frames, 25-30 tracks, 13 partial of 55, 2 starts triangulated (1 rejected), "
                             "f = 0.750 pixels)")
    assert _check_partial(None) is None and _check_partial("ba") is None and _check_partial("ba", 3) == (3, 0.0) and _check_partial("ba", 2, 1.5) == (2, 1.5)
