"""The model of the clip refinement (tests/refine_ref.py) against the oracle, the padded window packing of velocity_amd.NLS.pack_windows against
oracle.ba_pack, and the reason padding is allowed at all: an unobserved point adds exact zeros to a window's normal equations."""
import numpy as np
import pytest

import refine_ref as RR
from oracle import nls_oracle as O
from velocity_amd import synth


def _clip(nt=50, nf=6, dead=13, seed=5):
    """A finished clip's state built from synth.ba_scene: the last `dead` tracks died before the last frame (rows 0-4 NaN from there on)."""
    P, pw0, cw0 = synth.ba_scene(nt, nf, seed=seed)
    P[:, nt - dead:, nf - 2:] = np.nan
    B = np.zeros((nf, 14), np.float32)
    B[:, 3:6] = cw0
    B[:, 12] = np.arange(nf, dtype=np.float32) / np.float32(30.0)
    return synth.K_1080P, P, pw0, B


def test_refine_ref_is_the_oracle_on_the_surviving_tracks():
    K, P, p3, B = _clip()
    keep = np.arange(37)
    cw0 = B[:, 3:6].astype(np.float64)
    dcw, dpw, dx, dtr = O.nls_batch(K, P[:, keep].copy(), p3[keep], cw0, return_info=True)
    r = RR.refine_ref(K, P, p3, B, 6, solver=O.nls_batch)
    assert r["nt"] == 37 and np.array_equal(r["ids"], keep) and r["ids"].dtype == np.int32
    assert r["iterations"] == len(dtr) and r["converged"] == int(dtr[-1, 1] < 1e-7)
    np.testing.assert_allclose(r["cw"], dcw, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r["pw"], dpw, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r["trace"], dtr, rtol=1e-12, atol=1e-12)
    s = RR.refine_ref(K, P, p3, B, 6)  # the structured solve: the tolerances tests/test_oracle_nls.py pins nls_batch_schur at
    assert s["iterations"] == len(dtr)
    np.testing.assert_allclose(s["trace"][:, 0], dtr[:, 0], rtol=1e-7)
    np.testing.assert_allclose(s["cw"], dcw, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(s["pw"], dpw, rtol=1e-6, atol=1e-6)
    assert np.all(r["cw"][0] == 0) and np.isnan(r["speed"][0]) and np.isnan(r["dr"][0]) and np.all(np.isfinite(r["speed"][1:]))


def test_padded_packing_against_the_oracles():
    """pack_windows lays windows of 50, 37, 1 and 0 full-length tracks out for 50: a window's own rows are oracle.ba_pack's, the rest is NaN
    measurements and the point (0, 0, 1)."""
    from velocity_amd.NLS import pack_windows

    counts, nf = [50, 37, 1, 0], 6
    scenes = []
    for w, n in enumerate(counts):
        P, pw0, cw0 = synth.ba_scene(50, nf, seed=20 + w)
        P[:, n:, nf - 2:] = np.nan
        if n > 3:
            P[0:2, 3, 2] = np.nan  # a hole in a full-length track stays a NaN measurement
        scenes.append((P, pw0, cw0))
    z, x0, cnt, nt, nc = pack_windows(*zip(*scenes))
    assert (nt, nc) == (50, 5) and cnt.dtype == np.int32 and list(cnt) == counts
    assert z.shape == (4, 2 * 50 * 6) and x0.shape == (4, 3 * 50 + 6 * 5) and z.dtype == x0.dtype == np.float64
    for w, n in enumerate(counts):
        ez, ebad, ex, ent, enc = O.ba_pack(synth.K_1080P, *scenes[w])
        assert (ent, enc) == (n, nc)
        zw = z[w].reshape(2, nf, nt)
        own = zw[:, :, :n].reshape(-1)
        assert np.array_equal(np.isnan(own), ebad) and np.array_equal(np.where(ebad, 0.0, own), ez)
        assert np.isnan(zw[:, :, n:]).all()
        assert np.array_equal(x0[w, : 3 * n], ex[: 3 * n]) and np.array_equal(x0[w, 3 * nt:], ex[3 * n:])
        assert np.array_equal(x0[w, 3 * n: 3 * nt].reshape(-1, 3), np.tile([0.0, 0.0, 1.0], (nt - n, 1)))
    with pytest.raises(ValueError, match="frames"):
        pack_windows([scenes[0][0], synth.ba_scene(50, 8)[0]], [scenes[0][1]] * 2, [scenes[0][2], synth.ba_scene(50, 8)[2]])


@pytest.mark.parametrize("nt,nf,pad", [(50, 6, 14), (37, 6, 27), (1, 6, 63), (120, 24, 30)])
def test_padding_is_neutral(nt, nf, pad):
    """A point without an observation has zero residual and zero Jacobian rows: its block is U_i + I = I, W_i = 0, tp_i = 0, so it adds exact zeros
    to S and to the reduced right-hand side and its own step is 0.  With the two rms divisors taken from the true count the padded window takes
    the steps of the unpadded one."""
    K = synth.K_1080P.astype(float)
    nc = nf - 1
    z, bad, x0, _, _ = O.ba_pack(K, *synth.ba_scene(nt, nf, seed=60 + nt))
    ex, etr = O.ba_schur_solve(K, z, x0, nt, nc, 10, bad=bad)
    zp, bp, xp0 = RR.pad_window(z, bad, x0, nt, nc, nt + pad)
    xp, tr = RR.solve_padded(K, zp, bp, xp0, nt, nt + pad, nc)
    assert len(tr) == len(etr)
    assert np.array_equal(np.concatenate((xp[: 3 * nt], xp[3 * (nt + pad):])), ex)
    assert xp[3 * nt: 3 * (nt + pad)].tobytes() == xp0[3 * nt: 3 * (nt + pad)].tobytes()
    np.testing.assert_allclose(tr, etr, rtol=1e-14)


def test_speed_from_hand_made_positions():
    cw = np.array([[0, 0, 0], [0, 0, 0.5], [0.3, 0, 0.9], [0.3, 0.2, 0.9]], float)
    t = np.array([0.0, 0.04, 0.08, 0.16], np.float32)
    s = RR.speed_of(cw, t)
    dt = np.array([np.float32(0.04) - np.float32(0.0), np.float32(0.08) - np.float32(0.04), np.float32(0.16) - np.float32(0.08)], np.float64)
    dr = np.array([0.5, 0.5, 0.2])
    np.testing.assert_allclose(s["dr"][1:], dr, rtol=1e-15)
    np.testing.assert_allclose(s["speed"][1:], dr / dt * 3.6, rtol=1e-15)
    assert np.isnan(s["dr"][0]) and np.isnan(s["speed"][0])
    np.testing.assert_allclose(s["speed_mean"], (dr / dt * 3.6).mean(), rtol=1e-15)
    np.testing.assert_allclose(s["speed_std"], (dr / dt * 3.6).std(), rtol=1e-15)
    assert abs(s["speed"][1] - 45.0) < 1e-5  # 0.5 m in 0.04 s


def test_a_clip_without_a_full_length_track_is_not_solved():
    K, P, p3, B = _clip(dead=50)
    r = RR.refine_ref(K, P, p3, B, 6)
    assert r["nt"] == 0 and len(r["ids"]) == 0 and r["iterations"] == 0 and r["converged"] == 0 and r["trace"].shape == (0, 2)
    assert np.array_equal(r["cw"], B[:, 3:6].astype(np.float64)) and r["pw"].shape == (0, 3)
    np.testing.assert_allclose(r["speed"][1:], RR.speed_of(B[:, 3:6], B[:, 12])["speed"][1:], rtol=0)


def _canned_state(n=3, k=2):
    S = np.zeros((n, 9), np.float32)
    S[:, 0] = np.arange(n)
    S[0, 2] = k
    S[1:, 3], S[1:, 8] = 0.25, [39.5, 41.5]
    B = np.zeros((n, 14), np.float32)
    B[:, 12] = np.arange(n, dtype=np.float32) / np.float32(25.0)
    return dict(S=S, B=B, P=np.zeros((5, k, n), np.float32), vg=np.ones(k, bool), vp=np.ones(k, bool), p=np.zeros((k, 2), np.float32),
                p3=np.zeros((k, 3)), ids=np.arange(k, dtype=np.int32), klt_flags=0)


def test_clip_result_carries_the_refinement_and_its_line():
    from velocity_amd.driver import Admitted, ba_line, clip_result

    st, clip = _canned_state(), dict(n=3, name="canned", frame_numbers=[0, 1, 2])
    f0 = Admitted((0, 0, 1, 1), (0, 0, 1, 1), np.eye(3).reshape(9), 0.5)
    plain = clip_result(st, clip, f0, 1.0, 0.5, 1, np.zeros(2, np.int32))
    assert "ba" not in plain  # refine=None: the keys and the lines are what they always were
    ba = dict(nt=2, speed_mean=40.456, speed_std=1.0049, f_last=0.08449, iterations=10, converged=0)
    got = clip_result(st, clip, f0, 1.0, 0.5, 1, np.zeros(2, np.int32), ba=ba)
    assert set(got) == set(plain) | {"ba"} and got["ba"] is ba
    assert got["lines"] == plain["lines"] + ["BA speed = 40.46 +/- 1.00 km/h (2 tracks, f = 0.084 pixels)"] and got["lines"][-1] == ba_line(ba)
    assert plain["lines"][-2].startswith("\nSpeed = 40.50 +/- 1.00 km/h")


def test_refine_keyword_is_checked_before_anything_runs():
    from velocity_amd.driver import run_queue, run_sequence, run_sequences

    for call in (lambda: run_sequence([None, None], None, None, fps=25.0, refine="lm"), lambda: run_sequences([], None, refine=True),
                 lambda: run_queue([], None, 2, refine="BA")):
        with pytest.raises(ValueError, match="refine must be None or 'ba'"):
            call()


def test_the_refine_entry_points_are_declared_and_bound():
    from velocity_amd import _lib as L

    declared = L.declared_symbols()
    for s in ("vh_nls_batch_windows", "vh_session_refine_size", "vh_session_refine_workspace", "vh_session_refine"):
        assert s in declared and s in L._SIGS and hasattr(L.load(), s), s
    assert len(L._SIGS["vh_nls_batch_windows"][1]) == len(L._SIGS["vh_nls_batch_multi"][1]) + 2
