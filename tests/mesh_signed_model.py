"""numpy restatement of fp_mesh_pseudonormals, fp_mesh_signed_distance and fp_mesh_penetration (include/fp_amd.h).  The tables are
float64 rounded once; the per-query walk (tests/mesh_distance_model.py: the one restatement of the region walk), the feature, the
choice of the normal and the sign are float32, operation for operation.  Also an independent float64 inside test by the summed solid
angle (Van Oosterom and Strackee 1983), which needs neither tables nor closest points, and the numpy stand-in of
reconstruct.signed_bias.

`wrong=` names a deliberately wrong variant (the host tests show that the gates tell each from the definition):
  "uniform"      vertex normals summed with weight 1 per incident face instead of the interior angle       (tables)
  "unwelded"     adjacency by index instead of by position                                                  (tables)
  "face_normal"  the winning face's own normal for every feature                                            (sign)
  "q_minus_p"    s = dot(q - p, n)                                                                          (sign)
  "le"           inside when s <= 0                                                                         (sign)
  "en_order"     en indexed ab, ca, bc                                                                      (sign)"""
import numpy as np

from mesh_distance_model import f32, face_vertices, mesh_point_distance

FEATURES = ("vertex a", "vertex b", "vertex c", "edge ab", "edge bc", "edge ca", "interior")
# region 1..7 of the walk (vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, interior) -> feature code; 0 (no answer) -> -1
_FEATURE_OF_REGION = np.array([-1, 0, 1, 3, 2, 5, 4, 6], np.int32)
REPORT = ("edges", "boundary", "nonmanifold", "inconsistent", "degenerate", "welded", "closed", "zero")


def weld(pos):
    """w (Nv,) int64: the smallest index with the same three float32 coordinates (-0 == +0; a NaN equals nothing)"""
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    Nv = len(pos)
    if Nv == 0:
        return np.zeros(0, np.int64)
    bits = pos.view(np.uint32).astype(np.int64)
    bits[(bits & 0x7fffffff) == 0] = 0
    tag = np.where(np.isnan(pos).any(axis=1), np.arange(Nv) + 1, 0)
    _, inv = np.unique(np.column_stack([bits, tag]), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    first = np.full(inv.max() + 1, Nv, np.int64)
    np.minimum.at(first, inv, np.arange(Nv))
    return first[inv]


def pseudonormals(pos, faces, wrong=None):
    """-> vn (Nv,3) f32, en (F,3,3) f32, report (8,) int32: include/fp_amd.h, in float64"""
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    Nv, F = len(pos), len(faces)
    w = np.arange(Nv) if wrong == "unwelded" else weld(pos)
    valid = ((faces >= 0) & (faces < Nv)).all(axis=1) if F else np.zeros(0, bool)
    idx = np.where(valid[:, None], faces, 0) if Nv else np.zeros((F, 3), np.int64)
    p64 = pos.astype(np.float64)
    with np.errstate(all="ignore"):
        v = p64[idx] if Nv else np.zeros((F, 3, 3))
        n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        good = valid & (ln > 0) & np.isfinite(ln)
        unit = np.where(good[:, None], n / np.where(good, ln, 1.0)[:, None], 0.0)
        acc = np.zeros((Nv, 3))
        for j in range(3):
            e0, e1 = v[:, (j + 1) % 3] - v[:, j], v[:, (j + 2) % 3] - v[:, j]
            d = (e0[:, 0] * e1[:, 0] + e0[:, 1] * e1[:, 1]) + e0[:, 2] * e1[:, 2]
            l0 = np.sqrt((e0[:, 0] * e0[:, 0] + e0[:, 1] * e0[:, 1]) + e0[:, 2] * e0[:, 2])
            l1 = np.sqrt((e1[:, 0] * e1[:, 0] + e1[:, 1] * e1[:, 1]) + e1[:, 2] * e1[:, 2])
            ang = np.arccos(np.clip(d / (l0 * l1), -1.0, 1.0))
            if wrong == "uniform":
                ang = np.ones_like(ang)
            g = np.nonzero(good)[0]
            if Nv:
                np.add.at(acc, w[idx[g, j]], ang[g, None] * unit[g])
    vn = acc[w].astype(f32) if Nv else np.zeros((0, 3), f32)
    # the edges of every face with valid indices, as (smaller welded index << 32) | larger; edge k runs from corner k to corner k + 1
    w0 = w[idx] if Nv else idx
    w1 = np.roll(w0, -1, axis=1)
    key = (np.minimum(w0, w1) << 32) | np.maximum(w0, w1)                 # (F,3)
    fwd = w0 < w1
    gk = key[good].reshape(-1)
    uniq, inv, cnt = np.unique(gk, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    sums = np.zeros((len(uniq), 3))
    np.add.at(sums, inv, np.repeat(unit[good], 3, axis=0))
    nfwd = np.bincount(inv, weights=fwd[good].reshape(-1).astype(np.float64), minlength=len(uniq))
    en = np.zeros((F, 3, 3), f32)
    if len(uniq):
        at = np.minimum(np.searchsorted(uniq, key), len(uniq) - 1)
        hit = (uniq[at] == key) & valid[:, None]
        en = np.where(hit[:, :, None], sums[at], 0.0).astype(f32)
    boundary, nonmanifold = int((cnt == 1).sum()), int((cnt > 2).sum())
    inconsistent = int(((cnt == 2) & ((nfwd == 0) | (nfwd == 2))).sum())
    closed = int(len(uniq) > 0 and boundary == 0 and nonmanifold == 0 and inconsistent == 0)
    report = np.array([len(uniq), boundary, nonmanifold, inconsistent, int(F - good.sum()), int((w != np.arange(Nv)).sum()), closed, 0],
                      np.int32)
    return vn, en, report


def signed_distance(pos, faces, vn, en, points, wrong=None):
    """-> dict(dist2 (Q,) f32, face (Q,) i32, closest (Q,3) f32, feature (Q,) i32, sign (Q,) i32, s (Q,) f32 the dot product)"""
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    points = np.ascontiguousarray(points, f32).reshape(-1, 3)
    dist2, face, closest, region = mesh_point_distance(pos, faces, points, regions=True)
    feature = _FEATURE_OF_REGION[region]
    Q = len(points)
    sign = np.zeros(Q, np.int32)
    s = np.zeros(Q, f32)
    got = face >= 0
    if got.any():
        f = face[got].astype(np.int64)
        ft = feature[got]
        tri = face_vertices(pos, faces)[f]                                 # (n,3,3) f32
        ab, ac = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        with np.errstate(all="ignore"):
            cr = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                           ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], axis=1).astype(f32)
            k = np.clip(ft - 3, 0, 2)
            if wrong == "en_order":
                k = np.array([0, 2, 1])[k]
            n_edge = np.asarray(en, f32).reshape(-1, 3, 3)[f, k]
            n_vert = np.asarray(vn, f32).reshape(-1, 3)[faces[f, np.clip(ft, 0, 2)]]
            n = np.where((ft < 3)[:, None], n_vert, np.where((ft < 6)[:, None], n_edge, cr)).astype(f32)
            if wrong == "face_normal":
                n = cr
            d = points[got] - closest[got]
            if wrong == "q_minus_p":
                d = closest[got] - points[got]
            sg = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
        inside = (sg <= 0) if wrong == "le" else (sg < 0)
        sign[got] = np.where(inside, -1, 1)
        s[got] = sg
    return dict(dist2=dist2, face=face, closest=closest, feature=feature.astype(np.int32), sign=sign, s=s)


def transformed(points, tfs):
    """(T,Q,3) float32: p'[k] = ((rk[0]*x + rk[1]*y) + rk[2]*z) + rk[3], one float32 operation each"""
    x = np.ascontiguousarray(points, f32).reshape(-1, 3)
    m = np.ascontiguousarray(tfs, f32).reshape(-1, 4, 4)
    with np.errstate(all="ignore"):
        return np.stack([((m[:, k, 0, None] * x[None, :, 0] + m[:, k, 1, None] * x[None, :, 1]) + m[:, k, 2, None] * x[None, :, 2])
                         + m[:, k, 3, None] for k in range(3)], axis=2).astype(f32)


def penetration(pos, faces, vn, en, points, tfs, wrong=None):
    """-> dict(inside (T,) i32, depth2 (T,) f32, deepest (T,) i32, sign (T,Q) i32, dist2 (T,Q) f32)"""
    p = transformed(points, tfs)
    T, Q = p.shape[:2]
    r = signed_distance(pos, faces, vn, en, p.reshape(-1, 3), wrong)
    sign, dist2 = r["sign"].reshape(T, Q), r["dist2"].reshape(T, Q)
    inside = (sign < 0).sum(axis=1).astype(np.int32)
    depth2 = np.zeros(T, f32)
    deepest = np.full(T, -1, np.int32)
    for t in range(T):
        i = np.nonzero(sign[t] < 0)[0]
        if len(i):
            j = i[np.argmax(dist2[t, i])]                                  # the first of equal maxima: the smaller index
            depth2[t], deepest[t] = dist2[t, j], j
    return dict(inside=inside, depth2=depth2, deepest=deepest, sign=sign, dist2=dist2)


# ------------------------------------------------------------------ independent float64 references
def winding_number(pos, faces, points, block=1 << 21):
    """the summed solid angle of the faces seen from each point over 4 pi, float64 (Van Oosterom and Strackee): 1 inside a closed,
    outward-oriented shell, 0 outside.  Faces with an index outside the table are left out."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    faces = faces[((faces >= 0) & (faces < len(pos))).all(axis=1)]
    points = np.asarray(points, np.float64).reshape(-1, 3)
    out = np.zeros(len(points))
    if len(faces) == 0:
        return out
    tri = pos[faces]
    step = max(1, block // len(faces))
    for q0 in range(0, len(points), step):
        p = points[q0:q0 + step, None, :]
        A, B, C = tri[None, :, 0] - p, tri[None, :, 1] - p, tri[None, :, 2] - p
        la, lb, lc = (np.linalg.norm(X, axis=2) for X in (A, B, C))
        num = np.einsum("qfk,qfk->qf", A, np.cross(B, C))
        den = la * lb * lc + np.einsum("qfk,qfk->qf", A, B) * lc + np.einsum("qfk,qfk->qf", A, C) * lb + np.einsum("qfk,qfk->qf", B, C) * la
        out[q0:q0 + step] = (2.0 * np.arctan2(num, den)).sum(axis=1) / (4.0 * np.pi)
    return out


def inside_solid_angle(pos, faces, points):
    """bool (Q,): winding number above one half"""
    return winding_number(pos, faces, points) > 0.5


def distance_float64(pos, faces, points, block=1 << 21):
    """the distance of the points to the surface in float64 (mesh_distance_model.distance2_float64: not the region walk)"""
    from mesh_distance_model import distance2_float64
    tri = face_vertices(pos, faces).astype(np.float64)
    tri = tri[np.isfinite(tri).all(axis=(1, 2))]
    points = np.asarray(points, np.float64).reshape(-1, 3)
    out = np.full(len(points), np.inf)
    step = max(1, block // max(1, len(tri)))
    for q0 in range(0, len(points), step):
        out[q0:q0 + step] = np.sqrt(distance2_float64(points[q0:q0 + step], tri).min(axis=1))
    return out


def signed_bias(a, b, samples, seed=0, wrong=None):
    """numpy stand-in of reconstruct.signed_bias on (pos, faces) pairs -> (mean, inside share, p5, p50, p95) of the signed distances of
    a's stratified surface samples to b"""
    from mesh_distance_model import sample_surface
    pa, _ = sample_surface(a[0], a[1], samples, seed)
    vn, en, _ = pseudonormals(b[0], b[1])
    r = signed_distance(b[0], b[1], vn, en, pa, wrong)
    d = r["sign"].astype(np.float64) * np.sqrt(r["dist2"].astype(np.float64))
    return (float(d.mean()), float((r["sign"] < 0).mean()), *(float(x) for x in np.percentile(d, [5, 50, 95])))
