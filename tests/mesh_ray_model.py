"""numpy restatement of fp_mesh_ray_cast (include/fp_amd.h): what a ray hits first on a triangle mesh, operation for operation in
float32 -- Moeller-Trumbore on whole arrays, every difference, product, sum and the one quotient one float32 operation,
dot(x, y) = (x0*y0 + x1*y1) + x2*y2, each cross component one difference of two products, the answer the smallest (t, face).  Also the
same algorithm in float64 with its margins for the host tests, and the numpy stand-ins of ops.mesh_visibility,
reconstruct.view_coverage and compare_meshes(seen_from=).

`wrong=` names a deliberately wrong variant (the host tests show that the bit-equality gate tells each from the definition):
  "larger_index" equal t go to the larger face index
  "contracted"   dot products evaluated with one rounding (what a fused multiply-add chain approaches)
  "exclusive"    t_min < t < t_max where the definition has <=
  "signed_zero"  the t of a hit at -0 kept as -0"""
import numpy as np

from mesh_distance_model import face_vertices

f32 = np.float32


def _dot(x, y, wrong=None):
    if wrong == "contracted":
        return (x[0].astype(np.float64) * y[0] + x[1].astype(np.float64) * y[1] + x[2].astype(np.float64) * y[2]).astype(x[0].dtype)
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _cross(x, y):
    return (x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0])


def ray_triangles(o, d, a, b, c, t_min, t_max, cull=0, wrong=None):
    """o, d, a, b, c: tuples of three arrays (x, y, z) of one float type that broadcast against each other; t_min, t_max scalars of
    that type -> (hit bool, t, U, V, D, det).  In float32 this is the definition; in float64 the same algorithm for the host tests."""
    with np.errstate(all="ignore"):
        sub = lambda x, y: tuple(x[k] - y[k] for k in range(3))     # noqa: E731
        ab, ac = sub(b, a), sub(c, a)
        pvec = _cross(d, ac)
        det = _dot(ab, pvec, wrong)
        tvec = sub(o, a)
        un = _dot(tvec, pvec, wrong)
        qvec = _cross(tvec, ab)
        vn = _dot(d, qvec, wrong)
        tn = _dot(ac, qvec, wrong)
        neg = det < 0
        D = np.abs(det)
        U, V, T = np.where(neg, -un, un), np.where(neg, -vn, vn), np.where(neg, -tn, tn)
        q = T / D
        t = q if wrong == "signed_zero" else np.where(q == 0, np.zeros_like(q), q)
        side = np.ones_like(neg) if cull == 0 else (det > 0) if cull == 1 else neg
        in_range = ((t > t_min) & (t < t_max)) if wrong == "exclusive" else ((t >= t_min) & (t <= t_max))
        hit = (D > 0) & (U >= 0) & (V >= 0) & ((U + V) <= D) & in_range & (t <= np.finfo(t.dtype).max) & side
        return hit, t, U, V, D, det


def _xyz(m):
    return tuple(m[..., k] for k in range(3))


def mesh_ray_cast(pos, faces, origins, dirs, t_min=0.0, t_max=np.inf, cull=0, wrong=None, dtype=f32, block=1 << 21):
    """-> t (R,), face (R,) int32, bary (R,2), hit (R,3) of `dtype` (float32: the definition's bits)"""
    o_, d_ = np.asarray(origins, dtype).reshape(-1, 3), np.asarray(dirs, dtype).reshape(-1, 3)
    tri = face_vertices(pos, faces).astype(dtype)
    R, F = len(o_), len(tri)
    t_min, t_max = dtype(t_min), dtype(t_max)
    best = np.full(R, np.inf, dtype)
    face = np.full(R, -1, np.int32)
    bary = np.full((R, 2), np.nan, dtype)
    hitp = np.full((R, 3), np.nan, dtype)
    if R == 0 or F == 0:
        return best, face, bary, hitp
    o, d = _xyz(o_[:, None, :]), _xyz(d_[:, None, :])
    rows = np.arange(R)
    step = max(1, block // R)
    for f0 in range(0, F, step):
        tt = tri[f0:f0 + step]
        a, b, c = (_xyz(tt[None, :, j, :]) for j in range(3))
        hit, t, U, V, D, _ = ray_triangles(o, d, a, b, c, t_min, t_max, cull, wrong)
        key = np.where(hit, t, dtype(np.inf))
        if wrong == "larger_index":
            j = key.shape[1] - 1 - np.argmin(key[:, ::-1], axis=1)
            better = hit[rows, j] & (key[rows, j] <= best)
        else:
            j = np.argmin(key, axis=1)                             # the first of equal minima: the smaller face
            better = hit[rows, j] & (key[rows, j] < best)
        best = np.where(better, t[rows, j], best)
        face = np.where(better, (f0 + j).astype(np.int32), face)
        with np.errstate(all="ignore"):
            bary[:, 0] = np.where(better, U[rows, j] / D[rows, j], bary[:, 0])
            bary[:, 1] = np.where(better, V[rows, j] / D[rows, j], bary[:, 1])
    with np.errstate(all="ignore"):
        won = face >= 0
        for k in range(3):
            hitp[:, k] = np.where(won, o_[:, k] + best * d_[:, k], dtype(np.nan))
    return best, face, bary, hitp


def margins_float64(pos, faces, origins, dirs, t_min=0.0, t_max=np.inf, eps=1e-4, block=1 << 21):
    """the rays for which, in float64, some triangle in range has a barycentric (u, v or 1 - u - v) within eps of 0 -> (R,) bool"""
    o_, d_ = np.asarray(origins, np.float64).reshape(-1, 3), np.asarray(dirs, np.float64).reshape(-1, 3)
    tri = face_vertices(pos, faces).astype(np.float64)
    out = np.zeros(len(o_), bool)
    o, d = _xyz(o_[:, None, :]), _xyz(d_[:, None, :])
    step = max(1, block // max(1, len(o_)))
    for f0 in range(0, len(tri), step):
        tt = tri[f0:f0 + step]
        a, b, c = (_xyz(tt[None, :, j, :]) for j in range(3))
        _, t, U, V, D, _ = ray_triangles(o, d, a, b, c, np.float64(t_min), np.float64(t_max))
        with np.errstate(all="ignore"):
            u, v = U / D, V / D
            near = (np.abs(u) <= eps) | (np.abs(v) <= eps) | (np.abs(1.0 - u - v) <= eps)
            out |= (near & (D > 0) & (t >= t_min) & (t <= t_max)).any(axis=1)
    return out


# ------------------------------------------------------------------ stand-ins of ops.mesh_visibility / reconstruct.view_coverage
def mesh_visibility(points, eyes, pos, faces, rel_tol=1e-4, cull=0):
    """numpy stand-in of ops.mesh_visibility -> (E,Q) bool, True where nothing of the mesh lies between eye and point"""
    p, e = np.asarray(points, f32).reshape(-1, 3), np.asarray(eyes, f32).reshape(-1, 3)
    E, Q = len(e), len(p)
    origins = np.broadcast_to(e[:, None, :], (E, Q, 3)).reshape(-1, 3)
    dirs = (p[None, :, :] - e[:, None, :]).reshape(-1, 3)
    face = mesh_ray_cast(pos, faces, origins, dirs, 0.0, f32(1.0 - rel_tol), cull)[1]
    return (face < 0).reshape(E, Q)


def view_coverage(pos, faces, ob_in_cams, Ks, hw, samples, seed=0, rel_tol=1e-4, min_cos=0.0):
    """numpy stand-in of reconstruct.view_coverage on (pos, faces) -> ops.ViewCoverage with numpy arrays"""
    from foundationpose_amd import ops
    from foundationpose_amd.reconstruct import _coverage_views, _in_frame_and_facing, _surface_strata
    from mesh_distance_model import sample_surface
    pos, faces = np.asarray(pos, f32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    P, K, eyes, hw, rel_tol, min_cos = _coverage_views(ob_in_cams, Ks, hw, rel_tol, min_cos, "view_coverage")
    pts, f = sample_surface(pos, faces, samples, seed)
    a, b, c = (pos[faces[f, k]].astype(np.float64) for k in range(3))
    n = np.stack(_cross(_xyz(b - a), _xyz(c - a)), axis=1)
    table = _in_frame_and_facing(np, pts.astype(np.float64), n, P, K, eyes.astype(np.float64), hw, min_cos)
    table &= mesh_visibility(pts, eyes, pos, faces, rel_tol)
    return ops.ViewCoverage.from_seen(table, pts, f, float(_surface_strata(pos, faces, 1, 0)[0][-1]))


# ------------------------------------------------------------------ meshes and views the host and the GPU tests share
def cylinder(n_ang=24, radius=0.05, height=0.12, bottom=True):
    """a closed faceted cylinder about z, centred at the origin, outward faces: 2 n_ang side triangles, then n_ang top triangles,
    then (bottom) n_ang bottom triangles -> (pos float32, faces int32)"""
    ang = 2 * np.pi * np.arange(n_ang) / n_ang
    ring = np.stack([radius * np.cos(ang), radius * np.sin(ang)], axis=1)
    pos = np.concatenate([np.c_[ring, np.full(n_ang, -height / 2)], np.c_[ring, np.full(n_ang, height / 2)],
                          [[0, 0, height / 2], [0, 0, -height / 2]]])
    i = np.arange(n_ang)
    j = (i + 1) % n_ang
    side = np.concatenate([np.stack([i, j, j + n_ang], axis=1), np.stack([i, j + n_ang, i + n_ang], axis=1)])
    top = np.stack([i + n_ang, j + n_ang, np.full(n_ang, 2 * n_ang)], axis=1)
    bot = np.stack([j, i, np.full(n_ang, 2 * n_ang + 1)], axis=1)
    return pos.astype(f32), np.concatenate([side, top] + ([bot] if bottom else [])).astype(np.int32)


def ring_of_views(n_views=8, distance=0.5, elevation_deg=35.0, f=600.0, hw=(480, 640)):
    """cameras on a ring above the equator looking at the origin (OpenCV frames: z forward, y down) -> (ob_in_cams (V,4,4) float64,
    K (3,3) float64, hw)"""
    out = []
    el = np.deg2rad(elevation_deg)
    for k in range(n_views):
        az = 2 * np.pi * (k + 0.37) / n_views                       # off the facets' own angles: no face is seen edge-on
        eye = distance * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
        z = -eye / np.linalg.norm(eye)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])                                     # rows: the camera's axes in the object's frame
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, -R @ eye
        out.append(T)
    H, W = hw
    K = np.array([[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1]], np.float64)
    return np.stack(out), K, hw
