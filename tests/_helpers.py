"""Small helpers shared by the tests."""
import numpy as np


def frozen(*arrays):
    """The arrays, made read-only: what a cached builder hands out, so that a caller who writes into a shared array fails at once."""
    for a in arrays:
        a.setflags(write=False)
    return arrays


def frame0_host(outs, rois, nb):
    """The device outputs (p, p3, vp, t, R, res, n) and the ROI table of a frame-0 call of nb clips as one dict of host arrays."""
    p, p3, vp, t, R, res, n = (x.cpu().numpy() for x in outs)
    return dict(p=p[:nb], p3=p3[:nb], vp=vp[:nb], t=t[:nb], R=R[:nb], res=res[:nb], n=n[:nb], rois=np.array(list(rois)[:8 * nb]).reshape(nb, 8))


def same_table(lines, elines):
    """The printed table, line for line: text equal, or -- where a float computed in float64 on both sides lands on a rounding boundary of its
    printed digits -- every field within one unit of its last printed place."""
    assert len(lines) == len(elines), (len(lines), len(elines))
    for a, b in zip(lines, elines):
        if a == b:
            continue
        fa, fb = a.split(), b.split()
        assert len(fa) == len(fb), (a, b)
        for x, y in zip(fa, fb):
            if x == y:
                continue
            digits = len(x.split(".")[1]) if "." in x else 0
            assert abs(float(x) - float(y)) <= 1.01 * 10.0 ** -digits, (a, b)
