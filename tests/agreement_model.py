"""The numpy restatement of fp_depth_agreement's per-pixel classification (include/fp_amd.h) that the depth-agreement tests compare
the kernel with: every difference in float32, the tolerance rounded to float32 as the C ABI receives it."""
import numpy as np

REFINE_THR = np.float32(0.001)      # the REFINE warp's validity threshold


def classify(zr, zo, tol):
    """-> (model, valid, agree, behind) boolean arrays for render depths zr and observed depths zo"""
    zr, zo, t = np.asarray(zr, np.float32), np.asarray(zo, np.float32), np.float32(tol)
    d = zo - zr                                 # float32 - float32: a float32 difference
    assert d.dtype == np.float32
    model = zr > 0
    valid = model & (zo >= REFINE_THR)
    agree = valid & (np.abs(d) <= t)
    behind = valid & (d > t)
    return model, valid, agree, behind


def counts(zr, zo, tol):
    """(N, ...) render / observed depths -> (N, 4) int64 counts [model, valid, agree, behind] per leading index"""
    zr = np.asarray(zr, np.float32)
    N = zr.shape[0]
    return np.stack([m.reshape(N, -1).sum(1) for m in classify(zr, zo, tol)], 1).astype(np.int64)
