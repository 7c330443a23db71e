"""numpy restatement of fp_mesh_transform_residuals (include/fp_amd.h): the float32 transformed points p' = ((r0*x + r1*y) + r2*z) + t
per row, in that order, one rounding per operation; their squared distances to the mesh by the restatement of fp_mesh_point_distance
(tests/mesh_distance_model.py); per transform the maximum over the points and the number of points strictly above each squared
threshold.  Also the callables that drive foundationpose_amd.symmetry.find_symmetries on the host (host_symmetries).

`wrong=` names a deliberately wrong variant (the host tests show that the bit-equality gate tells each from the definition):
  "translate_first"  the translation added to the point before the rotation: R (x + t)
  "transposed"       the rotation's columns read where the definition reads its rows
  "ge"               a point counts as over a threshold with d2 >= thr2
  "min"              the minimum over the points where the definition takes the maximum
  "nonfinite_zero"   a transformed point that is not finite counted as lying on the surface (d2 = 0)"""
import numpy as np

import mesh_distance_model as mm

f32 = np.float32


def square_thresholds(thresholds):
    """lengths -> their float32 squares as ops.mesh_transform_residuals forms them: rounded to float32, then one float32 product"""
    t = np.asarray([] if thresholds is None else thresholds, np.float64).reshape(-1).astype(f32)
    return t * t


def transform_points(points, tfs, wrong=None):
    """points (Q,3), tfs (T,4,4) -> (T,Q,3) float32"""
    p = np.asarray(points, f32).reshape(-1, 3)
    m = np.asarray(tfs, f32).reshape(-1, 4, 4)
    if wrong == "transposed":
        m = np.concatenate([np.concatenate([m[:, :3, :3].transpose(0, 2, 1), m[:, :3, 3:]], axis=2), m[:, 3:]], axis=1)
    x, y, z = (p[None, :, k] for k in range(3))
    with np.errstate(all="ignore"):
        if wrong == "translate_first":
            x, y, z = x + m[:, 0, 3, None], y + m[:, 1, 3, None], z + m[:, 2, 3, None]
            rows = [(m[:, k, 0, None] * x + m[:, k, 1, None] * y) + m[:, k, 2, None] * z for k in range(3)]
        else:
            rows = [((m[:, k, 0, None] * x + m[:, k, 1, None] * y) + m[:, k, 2, None] * z) + m[:, k, 3, None] for k in range(3)]
    return np.stack(rows, axis=-1).astype(f32)


def mesh_transform_residuals(pos, faces, points, tfs, thr2=None, wrong=None):
    """-> max_d2 (T,) float32, over (T,L) int32, dist2 (T,Q) float32; thr2: the squared thresholds (L,) float32 themselves"""
    pt = transform_points(points, tfs, wrong)
    T, Q = pt.shape[:2]
    thr2 = np.zeros(0, f32) if thr2 is None else np.asarray(thr2, f32).reshape(-1)
    d2 = mm.mesh_point_distance(pos, faces, pt.reshape(-1, 3))[0].reshape(T, Q)
    if wrong == "nonfinite_zero":
        d2 = np.where(np.isfinite(pt).all(axis=2), d2, f32(0))
    if Q == 0:
        max_d2 = np.zeros(T, f32)
    else:
        max_d2 = (d2.min(axis=1) if wrong == "min" else d2.max(axis=1)).astype(f32)
    with np.errstate(invalid="ignore"):
        cmp = (d2[:, :, None] >= thr2[None, None, :]) if wrong == "ge" else (d2[:, :, None] > thr2[None, None, :])
    return max_d2, cmp.sum(axis=1).astype(np.int32).reshape(T, len(thr2)), d2.astype(f32)


# ------------------------------------------------------------------ the detector on the host
def area_centroid(pos, faces):
    """the area-weighted centroid of the surface and the largest vertex distance from it, float64"""
    from foundationpose_amd.symmetry import surface_centre
    return surface_centre(pos, faces)


def host_symmetries(pos, faces, tol=None, samples=(64, 512), **kw):
    """find_symmetries driven by the restatement: what reconstruct.detect_symmetries does on the device, on the host"""
    from foundationpose_amd.symmetry import find_symmetries
    pos, faces = np.asarray(pos, f32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    centre, radius = area_centroid(pos, faces)
    if tol is None:
        tol = 0.01 * 2 * radius
    pts = {"coarse": mm.sample_surface(pos, faces, samples[0], seed=1)[0], "fine": mm.sample_surface(pos, faces, samples[1], seed=0)[0]}

    def residuals(tfs, which):
        return np.sqrt(mesh_transform_residuals(pos, faces, pts[which], np.asarray(tfs, f32))[0].astype(np.float64))

    def closest(tf):
        p = transform_points(pts["fine"], np.asarray(tf, f32)[None])[0]
        return pts["fine"].astype(np.float64), mm.mesh_point_distance(pos, faces, p)[2].astype(np.float64)

    return find_symmetries(residuals, closest, centre, radius, tol, **kw)
