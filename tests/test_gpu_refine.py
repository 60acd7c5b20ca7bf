"""Refinement of finished clips on the device, in two layers.

Below: finished clips refined straight from the session (vh_session_refine, TrackerSession.refine, the drivers' refine="ba") against the NumPy model
tests/refine_ref.py.  First: bundle-adjustment windows of different track counts and cameras in one launch sequence (vh_nls_batch_windows): every window equals the
single-window call on its own tracks with its own K, on the three solve routes (matrix-core Gauss-Jordan up to 20 free cameras, the
register-resident Gauss-Jordan at 21, the blocked Cholesky from 22) and on the VALU Schur kernel.

Tolerances: a window is laid out for the common track count, so its partial systems are cut elsewhere than the single call's -- "another
partition of the partial sums", for which test_gpu_nls.py::test_nls_batch_windows_equal_single_calls allows x rtol 1e-6 / atol 1e-8 and
trace[:, 0] 1e-8.  The padding itself adds exact zeros (tests/test_refine_cpu.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_ITER = 10


def _scenes(nt, nf, counts, seed):
    """One synth.ba_scene per count, each with a slightly different focal length; tracks behind a window's count lose their last frames (rows 0-4
    NaN there), so the track filter of NLS.py:190 drops them."""
    from velocity_amd import synth

    Ks, scenes = [], []
    for w, cnt in enumerate(counts):
        K = synth.K_1080P.astype(np.float64).copy()
        K[0, 0] *= 1.0 + 0.01 * w
        K[1, 1] *= 1.0 + 0.01 * w
        P, pw0, cw0 = synth.ba_scene(nt, nf, seed=seed + w, K=K)
        P[:, cnt:, nf - 2:] = np.nan
        Ks.append(K)
        scenes.append((P, pw0, cw0))
    return np.stack(Ks), scenes


def _single(K, z, x0, nt, nc):
    """vh_nls_batch on one unpadded window -> (x, trace, info)."""
    import torch

    from velocity_amd import _lib as L

    ws = L.workspace()
    zd, xd = L.to_dev(z, torch.float64), L.to_dev(x0, torch.float64).clone()
    trace = torch.zeros((MAX_ITER, 2), dtype=torch.float64, device="cuda")
    info = torch.zeros(2, dtype=torch.int32, device="cuda")
    nbytes = int(ws.lib.vh_nls_batch_workspace(nt, nc))
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    L.check(ws.lib.vh_nls_batch(ws.handle, L.host_K(K).ctypes.data_as(L.f64p), L.dptr(zd), L.dptr(xd), nt, nc, MAX_ITER, L.dptr(trace), L.dptr(info),
                                L.dptr(scratch), nbytes, L.stream_ptr()), "vh_nls_batch")
    return xd.cpu().numpy(), trace.cpu().numpy(), info.cpu().numpy()


def _batched(entry, K, z, x0, nt, nc, counts=None, Ks=None):
    """vh_nls_batch_multi / vh_nls_batch_windows on packed windows -> (x [nw, nx], trace [nw, MAX_ITER, 2], info [nw, 2])."""
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
    if entry == "multi":
        L.check(ws.lib.vh_nls_batch_multi(ws.handle, Kp, L.dptr(zd), L.dptr(xd), nt, nc, nw, MAX_ITER, L.dptr(trace), L.dptr(info), L.dptr(scratch),
                                          nbytes, L.stream_ptr()), "vh_nls_batch_multi")
    else:
        ntd = None if counts is None else L.to_dev(np.asarray(counts, np.int32), torch.int32)
        Kd = None if Ks is None else L.to_dev(np.asarray(Ks, np.float64).reshape(nw, 9), torch.float64)
        L.check(ws.lib.vh_nls_batch_windows(ws.handle, Kp, L.dptr(zd), L.dptr(xd), nt, nc, nw, L.dptr(ntd), L.dptr(Kd), MAX_ITER, L.dptr(trace),
                                            L.dptr(info), L.dptr(scratch), nbytes, L.stream_ptr()), "vh_nls_batch_windows")
    return xd.cpu().numpy(), trace.cpu().numpy(), info.cpu().numpy()


def _check_windows_equal_single_calls(nt, nf, counts, seed):
    from velocity_amd.NLS import pack_windows

    nc = nf - 1
    Ks, scenes = _scenes(nt, nf, counts, seed)
    z, x0, cnt, nt_common, _ = pack_windows(*zip(*scenes))
    assert list(cnt) == list(counts) and nt_common == nt
    x, tr, info = _batched("windows", Ks[0], z, x0, nt, nc, counts, Ks)
    for w, n in enumerate(counts):
        pad = slice(3 * n, 3 * nt)
        assert x[w, pad].tobytes() == x0[w, pad].tobytes(), f"window {w}: padding rows moved"
        if n == 0:
            assert list(info[w]) == [0, 0] and x[w].tobytes() == x0[w].tobytes(), f"window {w}: an empty window was touched"
            continue
        zw = z[w].reshape(2, nf, nt)[:, :, :n].reshape(-1)
        xw = np.concatenate((x0[w, : 3 * n], x0[w, 3 * nt:]))
        sx, strace, sinfo = _single(Ks[w], zw, xw, n, nc)
        print(f"nf={nf} window {w} (nt_w={n}): info {info[w]} vs {sinfo}, max |dx| = {np.abs(np.concatenate((x[w, :3 * n], x[w, 3 * nt:])) - sx).max():.3g}, "
              f"max |df| = {np.abs(tr[w, :, 0] - strace[:, 0]).max():.3g}")
        assert np.array_equal(info[w], sinfo), f"window {w}"
        np.testing.assert_allclose(np.concatenate((x[w, : 3 * n], x[w, 3 * nt:])), sx, rtol=1e-6, atol=1e-8, err_msg=f"window {w}")
        np.testing.assert_allclose(tr[w, :, 0], strace[:, 0], rtol=1e-8, err_msg=f"window {w}")
    return Ks, scenes, (z, x0)


def test_windows_of_different_counts_and_cameras_small_route():
    """Five windows of 6 frames laid out for 50 tracks, with 50, 37, 1, 0 and 50 full-length tracks and five focal lengths."""
    Ks, scenes, _ = _check_windows_equal_single_calls(50, 6, [50, 37, 1, 0, 50], seed=400)
    # the Python shim: the same windows through fcnNLS_batch_windows against fcnNLS_batch
    from velocity_amd.NLS import fcnNLS_batch, fcnNLS_batch_windows

    out = fcnNLS_batch_windows(Ks, *zip(*scenes), return_info=True)
    for w in (1, 2):
        P, pw0, cw0 = scenes[w]
        scw, spw, sx, strace = fcnNLS_batch(Ks[w], P.copy(), pw0, cw0, return_info=True)
        cw, pw, x, tr = out[w]
        assert pw.shape == spw.shape and len(tr) == len(strace)
        np.testing.assert_allclose(cw, scw, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(pw, spw, rtol=1e-6, atol=1e-8)
    cw, pw, x, tr = out[3]
    assert pw.shape == (0, 3) and len(tr) == 0 and np.array_equal(cw, np.concatenate((np.zeros((1, 3)), scenes[3][2][1:])))


def test_windows_with_null_tables_are_the_multi_call_bit_for_bit():
    from velocity_amd import synth
    from velocity_amd.NLS import pack_windows

    scenes = [synth.ba_scene(50, 6, seed=400 + w) for w in range(5)]
    z, x0, cnt, nt, nc = pack_windows(*zip(*scenes))
    assert list(cnt) == [50] * 5
    a = _batched("multi", synth.K_1080P, z, x0, nt, nc)
    b = _batched("windows", synth.K_1080P, z, x0, nt, nc)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[2], b[2])
    np.testing.assert_allclose(a[1], b[1], rtol=1e-12)  # the two sums of squares behind the trace are accumulated with atomics (order varies run to run)
    # ... and a table that says "every window is full" with the one K changes nothing either
    c = _batched("windows", synth.K_1080P, z, x0, nt, nc, [50] * 5, np.stack([synth.K_1080P] * 5))
    assert a[0].tobytes() == c[0].tobytes() and np.array_equal(a[2], c[2])


@pytest.mark.parametrize("nf,force_valu", [(22, 1), (24, 0), (22, 0)])
def test_windows_of_different_counts_other_routes(nf, force_valu):
    """21 free cameras (register-resident Gauss-Jordan) and 23 (two-pass Schur kernel + blocked Cholesky); the 21-camera case also on the VALU Schur kernel."""
    from velocity_amd import _lib as L

    L.load().vh_debug_ba_force_valu(force_valu)
    try:
        _check_windows_equal_single_calls(120, nf, [120, 77, 9], seed=500 + nf)
    finally:
        L.load().vh_debug_ba_force_valu(0)


# ---- finished clips refined straight from the session (vh_session_refine, TrackerSession.refine, the drivers' refine="ba") --------------------------------
import refine_ref as RR  # noqa: E402
import scenes as S  # noqa: E402
from session_support import raw_export, same_dict, session_at, step_to  # noqa: E402

N0, NF, NHIST = 150, 8, 10  # the three streams of two cameras of scenes.scenes3 (three strides of hopeless tracks: three track counts)


def _ba_equals_model(ba, K, P, p3, B, n, where):
    """A refined clip (unpack_refine's dict) against refine_ref on the same state: nt and ids exact, iterations and converged equal, the rest within
    rtol 1e-6 / atol 1e-8."""
    ref = RR.refine_ref(K, P, p3, B, n)
    print(f"{where}: nt {ba['nt']} / {ref['nt']}, iterations {ba['iterations']} / {ref['iterations']}, converged {ba['converged']} / {ref['converged']}, "
          f"speed {ba['speed_mean']:.4f} +/- {ba['speed_std']:.4f} (model {ref['speed_mean']:.4f} +/- {ref['speed_std']:.4f}), f_last {ba['f_last']:.4f}, "
          f"max |dcw| {np.abs(ba['cw'] - ref['cw']).max():.3g}" + (f", max |dpw| {np.abs(ba['pw'] - ref['pw']).max():.3g}" if ref["nt"] else ""))
    assert ba["nt"] == ref["nt"] and np.array_equal(ba["ids"], ref["ids"]), where
    assert ba["iterations"] == ref["iterations"] and ba["converged"] == ref["converged"], where
    for key in ("cw", "pw", "dr", "speed", "speed_mean", "speed_std"):
        np.testing.assert_allclose(ba[key], ref[key], rtol=1e-6, atol=1e-8, equal_nan=True, err_msg=f"{where}: {key}")
    np.testing.assert_allclose(ba["trace"][:, 0], ref["trace"][:, 0], rtol=1e-6, err_msg=where)
    if ref["nt"]:
        assert ba["f_first"] == ba["trace"][0, 0] and ba["f_last"] == ba["trace"][-1, 0], where
    assert np.all(ba["cw"][0] == 0) and np.isnan(ba["dr"][0]) and np.isnan(ba["speed"][0]) and len(ba["cw"]) == n, where
    return ref


def test_session_refine_equals_the_model_and_leaves_the_session_alone():
    scenes = S.scenes3(N0, NHIST)
    ses, twin = session_at(scenes, NF - 1), session_at(scenes, NF - 1)
    before = [raw_export(ses, b) for b in range(3)]
    h = ses.refine([0, 1, 2])
    got = h.result()
    assert h.done() and len(got) == 3
    assert [raw_export(ses, b) for b in range(3)] == before
    counts = []
    for b in range(3):
        st = ses.state(b)
        assert st["frame_i"] == NF - 1
        _ba_equals_model(got[b], scenes[b][4], st["P"], st["p3"], st["B"], NF, f"stream {b}")
        assert got[b]["nt"] == st["n_cur"] and np.array_equal(got[b]["ids"], np.flatnonzero(st["vg"]))
        counts.append(got[b]["nt"])
    assert len(set(counts)) == 3 and min(counts) > 0, counts  # one launch sequence, three track counts, two cameras
    # the refined session steps on as the one that never refined
    step_to(ses, scenes, NF, NF + 1)
    step_to(twin, scenes, NF, NF + 1)
    for b in range(3):
        same_dict(ses.state(b), twin.state(b), f"stream {b} two frames later")


def test_session_refine_refusals_queue_nothing():
    import ctypes as C

    import torch

    from velocity_amd import _lib as L

    ses = session_at(S.scenes3(N0, NHIST), NF - 1)
    first = ses.refine([0, 1, 2]).result()
    lay = ses.refine_layout(10)
    lib = ses.lib
    need = int(lib.vh_session_refine_workspace(ses.handle, 3, NF))
    assert need > 0 and lay.bytes % 8 == 0
    recs = torch.zeros(3 * lay.bytes, dtype=torch.uint8, device="cuda")
    work = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def call(slots, nf, nbytes=need):
        rc = lib.vh_session_refine(ses.handle, (C.c_int * len(slots))(*slots), len(slots), nf, 10, L.dptr(recs), L.dptr(work), nbytes, L.stream_ptr())
        return rc, lib.vh_last_error().decode()

    for (slots, nf, nbytes), words in ((([0, 1, 2], NF - 1, need), ("slot 0", f"frame {NF - 1}")),   # the slots' counters are NF - 1, not NF - 2
                                       (([0, 1, 0], NF, need), ("slot 0", "twice")),
                                       (([0, 1, 2], 1, need), ("nf = 1", "two frames")),
                                       (([0, 1, 2], NF, need - 1), ("workspace", str(need))),
                                       (([0, 3], NF, need), ("slot 3", "3 slots")),
                                       (([0], NHIST + 1, need), (f"nf = {NHIST + 1}", f"{NHIST} frames"))):
        rc, msg = call(slots, nf, nbytes)
        assert rc == -1 and all(w in msg for w in words), (slots, nf, msg)
    with pytest.raises(RuntimeError, match="twice"):
        ses.refine([1, 1])
    torch.cuda.synchronize()
    assert not recs.any().item() and not work.any().item()  # nothing was queued: neither buffer was written
    again = ses.refine([0, 1, 2]).result()
    for a, b in zip(first, again):
        assert a["nt"] == b["nt"] and a["iterations"] == b["iterations"] and a["converged"] == b["converged"]
        for key in ("ids", "cw", "pw", "dr", "speed"):
            assert np.array_equal(a[key], b[key], equal_nan=True), key
        np.testing.assert_allclose(a["trace"], b["trace"], rtol=1e-12)  # (sums of squares accumulated with atomics)
    # slots in another order, and one of them alone: each record is its slot's
    swapped = ses.refine([2, 0]).result()
    assert np.array_equal(swapped[0]["cw"], first[2]["cw"]) and np.array_equal(swapped[1]["pw"], first[0]["pw"])


KW = dict(roi_border=(60, 40), max_corners=150)
_ALONE = {}


def _alone(c):
    """run_sequence(refine="ba") on the clip alone, once per clip."""
    from velocity_amd.driver import run_sequence

    if c["name"] not in _ALONE:
        _ALONE[c["name"]] = run_sequence(c["frames"], c["q"], c["K"], times=c["times"], out=None, live=False, name=c["name"], refine="ba", **KW)
    return _ALONE[c["name"]]


def _result_equals_model(res, K, where):
    n = res["P"].shape[2]
    return _ba_equals_model(res["ba"], K, res["P"], res["p3"], res["B"], n, where)


def test_run_sequence_refine_ba():
    from velocity_amd.driver import ba_line, run_sequence

    c = S.plate_clip(320, 240, 700.0, 8, 501, "synthetic 320 x 240")
    args = dict(times=c["times"], clock=lambda: 0.0, name=c["name"], **KW)
    plain, printed = run_sequence(c["frames"], c["q"], c["K"], out=None, **args), []
    got = run_sequence(c["frames"], c["q"], c["K"], out=printed.append, refine="ba", **args)
    assert "ba" not in plain and set(got) == set(plain) | {"ba"}
    _result_equals_model(got, c["K"], c["name"])
    assert got["ba"]["nt"] == len(got["ids"]) > 20
    line = ba_line(got["ba"])
    assert line.startswith("BA speed = ") and f"({got['ba']['nt']} tracks, f = " in line and line.endswith(" pixels)")
    assert got["lines"] == plain["lines"] + [line] and printed == got["lines"]
    for key in set(plain) - {"lines", "seconds", "ms_per_frame"}:
        assert np.array_equal(np.asarray(got[key]), np.asarray(plain[key]), equal_nan=True), key
    with pytest.raises(ValueError, match="refine"):
        run_sequence(c["frames"], c["q"], c["K"], out=None, refine="lm", **args)


def test_run_queue_and_run_sequences_refine_ba():
    """Five clips of lengths 6, 8, 8, 6, 7 and two cameras over two streams.  Clips 2 (8 frames) and 3 (6 frames) end at the same step of the plan: clips of
    one step are grouped by length, so that step issues two refine calls; run_sequences then refines two clips of one length in one call."""
    from velocity_amd.driver import run_queue, run_sequences

    cams = ((320, 240, 700.0), (256, 192, 560.0))
    clips = [S.plate_clip(*cams[k % 2], n, 600 + k, f"clip {k}") for k, n in enumerate((6, 8, 8, 6, 7))]
    K0 = S.camera(320, 240, 650.0)
    plain = run_queue(clips, K0, streams=2, sessions=1, max_size=(240, 320), **KW)
    got = run_queue(clips, K0, streams=2, sessions=1, max_size=(240, 320), refine="ba", **KW)
    assert len(got) == len(plain) == 5
    for c, g, p in zip(clips, got, plain):
        one = _alone(c)
        assert "ba" not in p and set(g) == set(p) | {"ba"}
        assert g["ba"]["nt"] == one["ba"]["nt"] > 0 and np.array_equal(g["ba"]["ids"], one["ba"]["ids"]), c["name"]
        assert g["ba"]["iterations"] == one["ba"]["iterations"] and g["ba"]["converged"] == one["ba"]["converged"], c["name"]
        for key in ("cw", "pw", "dr", "speed", "speed_mean", "speed_std"):
            np.testing.assert_allclose(g["ba"][key], one["ba"][key], rtol=1e-6, atol=1e-8, equal_nan=True, err_msg=f"{c['name']}: {key}")
        for key in set(p) - {"lines", "seconds", "ms_per_frame", "S"}:
            assert np.array_equal(np.asarray(g[key]), np.asarray(p[key]), equal_nan=True), (c["name"], key)
        assert np.array_equal(np.delete(g["S"], 1, 1), np.delete(p["S"], 1, 1), equal_nan=True)  # (column 1 is procTime)
        assert len(g["lines"]) == len(p["lines"]) + 1 and g["lines"][-3] == p["lines"][-2] and g["lines"][-1].startswith("BA speed = ")
    # run_sequences: the two 8-frame clips (two cameras) of one session in ONE refine call
    both = run_sequences([clips[1], clips[2]], K0, sessions=1, refine="ba", **KW)
    for c, g in zip((clips[1], clips[2]), both):
        one = _alone(c)
        assert g["ba"]["nt"] == one["ba"]["nt"] and np.array_equal(g["ba"]["ids"], one["ba"]["ids"]) and g["ba"]["iterations"] == one["ba"]["iterations"]
        for key in ("cw", "pw", "speed"):
            np.testing.assert_allclose(g["ba"][key], one["ba"][key], rtol=1e-6, atol=1e-8, equal_nan=True, err_msg=f"{c['name']}: {key}")
        assert g["lines"][-1] == one["lines"][-1]
    assert "ba" not in run_sequences([clips[1], clips[2]], K0, sessions=1, **KW)[0]


def test_real_stills_refine_ba():
    """Sequence B of the reference's stills (label: 40 km/h).  The refined speed is an observation, not a requirement (the scale gauge is held only by the
    +I damping): what is asserted is parity with the model."""
    from velocity_amd.driver import run_sequence

    d = S.load_stills()
    res = run_sequence(d["b_frames"], d["b_q"], d["b_K"], times=d["b_times"], roi_border=(180, 140), out=None, live=False, refine="ba")
    ba = res["ba"]
    _result_equals_model(res, d["b_K"], "stills b")
    assert ba["nt"] == len(res["ids"]) == int(res["vg"].sum()) > 0  # (observed: 87 of the 278 frame-0 tracks live through all seven stills)
    assert all(np.all(np.isfinite(ba[k])) for k in ("cw", "pw", "trace", "speed_mean", "speed_std", "f_first", "f_last"))
    assert np.all(np.isfinite(ba["speed"][1:])) and np.all(np.isfinite(ba["dr"][1:]))
    print(res["lines"][-3].strip().splitlines()[0], "|", res["lines"][-1])
