"""What the GPU tests of TrackerSession share: sessions over the scenes of tests/scenes.py and the comparisons of a stream's state."""
import numpy as np

from scenes import T0, to_cuda


def same_dict(a, b, where):
    """Two state() / export() dicts: the same keys, every value equal (NaN equal to NaN in the float ones)."""
    assert a.keys() == b.keys(), where
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=np.asarray(a[key]).dtype.kind == "f"), (where, key)


def equals_oracle(st, orc, where, records=True):
    """A stream's state() against its SessionOracle: masks, ids and points bit for bit, p3 and the float records to 1e-4."""
    assert st["frame_i"] == orc.i, where
    assert np.array_equal(st["vg"], orc.vg) and np.array_equal(st["vp"], orc.vp), where
    assert np.array_equal(st["ids"], np.nonzero(orc.vg)[0]) and np.array_equal(st["p"], orc.p), where
    np.testing.assert_allclose(st["p3"], orc.p3, rtol=1e-4, atol=1e-5)
    if records:
        n = orc.i + 1
        np.testing.assert_allclose(st["B"][:n, 12:14], orc.B[:n, 12:14], rtol=0, atol=0)
        np.testing.assert_allclose(st["S"][1:n, [0, 2, 4, 5]], orc.S[1:n, [0, 2, 4, 5]], rtol=0, atol=0)
        np.testing.assert_allclose(st["S"][1:n, [3, 6, 7, 8]], orc.S[1:n, [3, 6, 7, 8]], rtol=1e-4)


def raw_export(ses, b):
    """The bytes of slot b's export record."""
    h = ses.export(b)
    h.result()
    return h.buf.numpy()[: h.layout.bytes].tobytes()


def step_to(ses, scenes, first, last):
    """Frames first..last of every scene, stream b on its own clock."""
    nb = len(scenes)
    for k in range(first, last + 1):
        ses.step([to_cuda(sc[0][k]) for sc in scenes], time_s=[np.float32(10.0 * b + k / (25.0 + b)) for b in range(nb)], frame_no=[k] * nb)


def session_at(scenes, frame, **session_kw):
    """One stream per scene (each with its own K) in one session as large as the largest frame, with a history as long as the clips, stepped to `frame`."""
    from velocity_amd.driver import TrackerSession

    H, W = (max(sc[0][0].shape[d] for sc in scenes) for d in (0, 1))
    kw = dict(nhist=len(scenes[0][0]), batch=len(scenes), msv_frame=5)
    kw.update(session_kw)
    ses = TrackerSession(scenes[0][4], W, H, len(scenes[0][1]), **kw)
    for b, (frames, p, p3, vp, Kb) in enumerate(scenes):
        ses.init_stream(b, frames[0], p, p3, vp, T0, time0=10.0 * b, K=Kb)
    step_to(ses, scenes, 1, frame)
    return ses
