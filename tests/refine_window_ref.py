"""NumPy model of the refinement of ONE frame window of a clip (vh_session_refine_windows): the reference's
fcnNLS_batch(K, P[:, :, first:first+nf], pw, cw) in the coordinates of the window's first camera, built on tests/refine_ref.py::refine_ref.
Checker only: the product never imports it."""
import numpy as np

from refine_ref import refine_ref


def window_inputs(P, p3, B, first, nf):
    """The shifted inputs of window [first, first + nf): the history slice, the points p3 + B[first, 3:6] and the records of the window's frames with
    columns 3:6 relative to the window's first camera.  The shift is formed in float64 from the float32 B; the time column stays float32 (float32 ->
    float64 -> float32 is exact, and refine_ref's speed_of takes the float32 difference)."""
    B64 = np.asarray(B, np.float32)[first:first + nf].astype(np.float64)
    shift = B64[0, 3:6].copy()
    B64[:, 3:6] -= shift
    return np.asarray(P)[:, :, first:first + nf], np.asarray(p3, np.float64) + shift, B64


def window_ids(P, first, nf):
    """The tracks of the window: finite in row 4 of every frame of it (NLS.py:190 on the slice), ascending."""
    return np.flatnonzero(np.isfinite(np.asarray(P)[4, :, first:first + nf]).all(1)).astype(np.int32)


def refine_window_ref(K, P, p3, B, first, nf, max_iter=10):
    """refine_ref on window [first, first + nf) of a clip (history P [5, N0, >= first + nf], points p3 [N0, 3], records B [>= first + nf, 14]); adds
    `first`, `f_first` and `f_last` (the rms residual of the first and of the last iteration).  cw and pw come out in the window's coordinates."""
    assert first >= 0 and nf >= 2 and first + nf <= np.asarray(P).shape[2]
    Pw, pw0, Bw = window_inputs(P, p3, B, first, nf)
    out = refine_ref(K, Pw, pw0, Bw, nf, max_iter=max_iter)
    tr = out["trace"]
    out.update(first=first, f_first=tr[0, 0] if len(tr) else np.nan, f_last=tr[-1, 0] if len(tr) else np.nan)  # (the record's fields merge_window_speeds reads)
    return out
