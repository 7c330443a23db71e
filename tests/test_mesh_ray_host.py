"""CPU: the definition of fp_mesh_ray_cast (tests/mesh_ray_model.py, the numpy restatement of include/fp_amd.h) against the same
algorithm in float64 outside its margins, analytic cases (the sphere, two parallel squares), the cases whose answer is known
beforehand, the wrong variants the bit-equality gate can see, the argument errors of the C entry point and the wrappers' refusals
that need no device, and the logic of ops.mesh_visibility and reconstruct.view_coverage on their numpy stand-ins."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_ray_cases as rc
import mesh_ray_model as rm
from mesh_signed_cases import icosphere

f32 = np.float32
MARGIN = 1e-4             # a barycentric this close to 0 in float64 puts a ray into the margin set
MARGIN_SHARE = 0.10       # at most this share of a case's rays may be in it (the issue measured 8 %)
# the relative error of the restatement's t against float64, over the rays outside the margin set of the three 3000-face soups:
# measured 7.9e-7 (scale 1e-3), 1.1e-6 (scale 1) and 5.9e-6 (scale 50) at most; the gate is four times the largest
T_REL_MEASURED = 5.9e-6
T_REL_GATE = 4 * T_REL_MEASURED


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype.kind == "i" else a.view(np.uint32)


def _same(got, ref):
    return all(np.array_equal(_bits(g), _bits(r)) for g, r in zip(got, ref))


# ------------------------------------------------------------------ 1. the restatement against float64
@pytest.mark.parametrize("c", rc.margin_soups(), ids=lambda c: c["name"].replace(" ", "_"))
def test_restatement_against_float64_outside_the_margins(c):
    t32, f32_, _, _ = rc.references()[c["name"]]
    t64, f64_, _, _ = rc.cast(c, dtype=np.float64)
    margin = rm.margins_float64(c["pos"], c["faces"], c["origins"], c["dirs"], c["t_min"], c["t_max"], MARGIN)
    share = float(margin.mean())
    differ = f32_ != f64_
    hit = (f64_ >= 0) & ~margin
    rel = np.abs(t32[hit].astype(np.float64) - t64[hit]) / t64[hit]
    print(f"{c['name']}: margin set {100 * share:.1f} %, faces differing inside it {int((differ & margin).sum())}, outside "
          f"{int((differ & ~margin).sum())}, max relative error of t {rel.max():.3g}")
    assert share <= MARGIN_SHARE
    assert not (differ & ~margin).any()
    assert hit.sum() > 800 and rel.max() <= T_REL_GATE


def test_answers_known_beforehand():
    refs = rc.references()
    for c in rc.all_cases():
        t, face, bary, hit = refs[c["name"]]
        for k, v in c.get("expect_face", {}).items():
            assert face[k] == v, (c["name"], k, face[k], v)
        for k, v in c.get("expect_t", {}).items():
            assert t[k] == v and not np.signbit(t[k]), (c["name"], k, t[k], v)
        miss = face < 0
        assert np.isposinf(t[miss]).all() and np.isnan(bary[miss]).all() and np.isnan(hit[miss]).all(), c["name"]
        assert np.isfinite(t[~miss]).all() and (t[~miss] >= 0).all() and not np.signbit(t[~miss]).any(), c["name"]
        # the hit is the barycentric combination up to rounding
        if (~miss).any() and np.isfinite(c["pos"]).all():
            tri = c["pos"][c["faces"][face[~miss]]].astype(np.float64)
            u, v = bary[~miss, 0:1].astype(np.float64), bary[~miss, 1:2].astype(np.float64)
            comb = tri[:, 0] + u * (tri[:, 1] - tri[:, 0]) + v * (tri[:, 2] - tri[:, 0])
            size = np.abs(tri).max() + np.abs(c["origins"][~miss]).max()
            assert np.abs(comb - hit[~miss]).max() <= 1e-4 * size, c["name"]


@pytest.mark.parametrize("wrong, case", [("larger_index", "ties on a shared edge and a shared vertex"), ("contracted", "soup F=3000 R=1000 x1 (margins)"),
                                         ("exclusive", "hit exactly at t_min"), ("exclusive", "hit exactly at t_max"),
                                         ("signed_zero", "origin on the triangle")])
def test_wrong_variants_are_told_apart(wrong, case):
    c = next(c for c in rc.all_cases() if c["name"] == case)
    assert not _same(rc.cast(c, wrong=wrong), rc.references()[case])


# ------------------------------------------------------------------ 2. analytic cases
def test_rays_into_the_unit_sphere_hit_within_the_facet_sag():
    pos, faces = icosphere(1.0)
    tri = pos[faces]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    r_in = float(np.min(np.einsum("fk,fk->f", tri[:, 0], n) / np.linalg.norm(n, axis=1)))     # the facets' planes: 0.93 of the radius
    assert 0.9 < r_in < 1.0
    rng = np.random.default_rng(3)
    R = 2000
    u = rng.normal(size=(R, 3))
    o = rng.uniform(1.5, 4.0, (R, 1)) * u / np.linalg.norm(u, axis=1, keepdims=True)
    w = rng.normal(size=(R, 3))
    target = rng.uniform(0, 0.5 * r_in, (R, 1)) * w / np.linalg.norm(w, axis=1, keepdims=True)
    d = (target - o) * rng.uniform(0.5, 2.0, (R, 1))
    o32, d32 = o.astype(f32), d.astype(f32)
    t, face, bary, hit = rm.mesh_ray_cast(pos, faces, o32, d32)
    assert (face >= 0).all()
    # the exact sphere: |o + t d| = 1, the nearer root, from the float32 rays in float64
    o64, d64 = o32.astype(np.float64), d32.astype(np.float64)
    A, B, Cc = (d64 * d64).sum(1), (o64 * d64).sum(1), (o64 * o64).sum(1) - 1.0
    t_s = (-B - np.sqrt(B * B - A * Cc)) / A
    # the hit lies between the radii r_in and 1 on a ray that passes within r_in / 2 of the centre: the path between the two radii is
    # at most (1 - r_in) / (r_in * sqrt(3) / 2)
    gap = (t.astype(np.float64) - t_s) * np.sqrt(A)
    assert gap.min() >= -1e-5 and gap.max() <= (1.0 - r_in) / (r_in * np.sqrt(0.75)) + 1e-5, (gap.min(), gap.max())
    radius = np.linalg.norm(hit.astype(np.float64), axis=1)
    assert radius.min() >= r_in - 1e-5 and radius.max() <= 1.0 + 1e-5


def test_the_nearer_of_two_parallel_squares_answers_whatever_the_face_order():
    pos, faces, _, _ = rc.two_squares()
    rng = np.random.default_rng(4)
    xy = rng.uniform(0.05, 0.95, (300, 2))
    xy = xy[np.abs(xy[:, 0] - xy[:, 1]) > 1e-3]                                   # off the shared diagonal: not watertight there
    o = np.c_[xy, np.full(len(xy), 3.0)].astype(f32)
    d = np.tile(np.array([[0, 0, -1]], f32), (len(xy), 1))
    for order in ([0, 1, 2, 3], [2, 3, 0, 1], [3, 0, 2, 1]):
        t, face, _, hit = rm.mesh_ray_cast(pos, faces[order], o, d)
        assert np.isin(np.asarray(order)[face], (0, 1)).all() and (t == 2.0).all() and (hit[:, 2] == 1.0).all()
        t, face, _, _ = rm.mesh_ray_cast(pos, faces[order], o - np.array([0, 0, 4], f32), -d)   # from below: the receiver is nearer
        assert np.isin(np.asarray(order)[face], (2, 3)).all() and (t == 1.0).all()


# ------------------------------------------------------------------ 3. refusals that need no device
def test_c_entry_point_reports_argument_errors_without_a_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(4096)
    wsb = lib.fp_mesh_ray_cast_workspace_bytes
    assert wsb(0) == 0 == wsb(-3) and wsb(1000) == 8000
    inf, nan = float("inf"), float("nan")

    def call(pos=p, Nv=3, faces=p, F=1, origins=p, dirs=p, R=4, t_min=0.0, t_max=inf, cull=0, t=p, ws=p, ws_bytes=32):
        return lib.fp_mesh_ray_cast(pos, Nv, faces, F, origins, dirs, R, t_min, t_max, cull, t, None, None, None, ws, ws_bytes, None)

    for kw, word in ((dict(R=-1), b"R=-1"), (dict(R=(1 << 30) + 1), b"R="), (dict(F=-1), b"F=-1"), (dict(F=(1 << 30) + 1), b"F="),
                     (dict(Nv=-1), b"Nv=-1"), (dict(t_min=-1.0), b"t_min=-1"), (dict(t_min=2.0, t_max=1.0), b"0 <= t_min <= t_max"),
                     (dict(t_min=nan), b"t_min=nan"), (dict(t_max=nan), b"t_max=nan"),
                     (dict(cull=-1), b"cull=-1"), (dict(cull=3), b"cull=3"), (dict(origins=None), b"NULL origins, dirs or t"),
                     (dict(dirs=None), b"NULL origins, dirs or t"), (dict(t=None), b"NULL origins, dirs or t"),
                     (dict(faces=None), b"faces is NULL"), (dict(pos=None), b"pos is NULL"), (dict(ws=None), b"workspace"),
                     (dict(ws_bytes=31), b"fp_mesh_ray_cast_workspace_bytes"), (dict(ws=C.c_void_p(4100)), b"8-byte aligned"),
                     # two adjacent faults: the earlier one is named
                     (dict(R=-1, F=-1), b"R=-1"), (dict(F=-1, Nv=-1), b"F=-1"), (dict(Nv=-1, t_min=-1.0), b"Nv=-1"),
                     (dict(t_min=-1.0, cull=7), b"t_min=-1"), (dict(cull=7, origins=None), b"cull=7"),
                     (dict(origins=None, faces=None), b"NULL origins"), (dict(faces=None, pos=None), b"faces is NULL"),
                     (dict(pos=None, ws=None), b"pos is NULL")):
        assert call(**kw) == -1, kw
        msg = lib.fp_last_error()
        assert msg.startswith(b"fp_mesh_ray_cast") and word in msg, (kw, msg)
    # nothing to do: R = 0 passes whatever the pointers are, but not a bad range or cull
    assert call(R=0, origins=None, dirs=None, t=None, ws=None, ws_bytes=0) == 0
    assert call(R=0, cull=5) == -1 and call(R=0, t_min=nan) == -1


def test_wrappers_refuse_before_devices():
    from foundationpose_amd import _lib, ops
    from foundationpose_amd.reconstruct import compare_meshes, view_coverage
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    pos, faces = torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32)
    mesh = dict(pos=pos, faces=faces)
    for kw, exc, msg in ((dict(want=("dist2",)), ValueError, "unknown name 'dist2'"),
                         (dict(want=()), ValueError, "want is empty"),
                         (dict(cull="both"), ValueError, "cull must be one of"),
                         (dict(t_min=-0.5), ValueError, "0 <= t_min <= t_max"),
                         (dict(t_min=2.0, t_max=1.0), ValueError, "0 <= t_min <= t_max"),
                         (dict(t_max=float("nan")), ValueError, "0 <= t_min <= t_max"),
                         (dict(origins=o.numpy()), _lib.FpAmdError, "origins must be a tensor"),
                         (dict(dirs=torch.zeros(4)), _lib.FpAmdError, r"dirs must be \(n,3\)"),
                         (dict(dirs=torch.zeros(5, 3)), _lib.FpAmdError, "dirs must be .* like origins"),
                         (dict(mesh_tensors=None), _lib.FpAmdError, "no mesh"),
                         (dict(mesh_tensors=mesh, pos=pos), _lib.FpAmdError, "not both"),
                         (dict(mesh_tensors=dict(pos=torch.zeros(3, 4), faces=faces)), _lib.FpAmdError, r"pos must be \(n,3\)"),
                         (dict(out=dict(dist2=o)), _lib.FpAmdError, "not among the wanted"),
                         (dict(out=dict(bary=torch.zeros(4, 3))), _lib.FpAmdError, r"out\['bary'\] must be a tensor of shape"),
                         (dict(), _lib.FpAmdError, "origins: expected a CUDA")):
        args = dict(origins=o, dirs=d, mesh_tensors=mesh)
        args.update(kw)
        with pytest.raises(exc, match=msg):
            ops.mesh_ray_cast(**args)
    for kw, exc, msg in ((dict(rel_tol=1.0), ValueError, r"rel_tol must be in \[0, 1\)"), (dict(rel_tol=-1e-4), ValueError, "rel_tol must be in"),
                         (dict(cull="both"), ValueError, "cull must be one of"), (dict(eyes=torch.zeros(3)), _lib.FpAmdError, r"eyes must be \(n,3\)"),
                         (dict(), _lib.FpAmdError, "points: expected a CUDA")):
        args = dict(points=o, eyes=d, mesh_tensors=mesh)
        args.update(kw)
        with pytest.raises(exc, match=msg):
            ops.mesh_visibility(**args)
    P, K = np.tile(np.eye(4), (2, 1, 1)), np.eye(3)
    for kw, exc, msg in ((dict(accel="grid"), NotImplementedError, "follow-up"), (dict(accel="bvh"), ValueError, "accel must be None"),
                         (dict(samples=0), ValueError, "samples must be an int >= 1"), (dict(hw=(0, 4)), ValueError, "hw must be"),
                         (dict(hw=7), ValueError, "hw must be"), (dict(ob_in_cams=np.eye(4)), ValueError, r"ob_in_cams must be finite \(V,4,4\)"),
                         (dict(Ks=np.zeros((3, 3, 3))), ValueError, "Ks must be finite"), (dict(rel_tol=2.0), ValueError, "rel_tol must be in"),
                         (dict(min_cos=1.0), ValueError, "min_cos must be in")):
        args = dict(mesh=mesh, ob_in_cams=P, Ks=K, hw=(8, 8))
        args.update(kw)
        with pytest.raises(exc, match=msg):
            view_coverage(**args)
    for bad in (7, dict(ob_in_cams=P, Ks=K), dict(ob_in_cams=P, Ks=K, hw=(8, 8), samples=5)):
        with pytest.raises(ValueError, match="seen_from must be a dict"):
            compare_meshes(mesh, mesh, unit=1.0, seen_from=bad)
    for bad, msg in ((dict(ob_in_cams=np.eye(4), Ks=K, hw=(8, 8)), "compare_meshes: seen_from: ob_in_cams must be finite"),
                     (dict(ob_in_cams=P, Ks=K, hw=(8, 8), rel_tol=1.5), "compare_meshes: seen_from: rel_tol must be in")):
        with pytest.raises(ValueError, match=msg):
            compare_meshes(mesh, mesh, unit=1.0, seen_from=bad)


# ------------------------------------------------------------------ 4. visibility and coverage on the stand-ins
SHADOW_BAND = 1e-4        # = rel_tol: samples this close to an edge of a blocker triangle's shadow are left out, the rest is exact


def squares_visibility():
    """the two-squares case of the host and the GPU tests: (pos, faces, eye, samples of the receiver, in the shadow, near an edge)"""
    from mesh_distance_model import sample_surface
    pos, faces, (rpos, rfaces), eye = rc.two_squares()
    pts, _ = sample_surface(rpos, rfaces, 4096, 0)
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    shadow = (x > -0.5) & (x < 1.5) & (y > -0.5) & (y < 1.5)
    # the shadow's four sides, and the image of the blocker's diagonal, where a ray may slip between its two faces (not watertight)
    edge = ((np.minimum(np.abs(x + 0.5), np.abs(x - 1.5)) < SHADOW_BAND) & (y > -0.6) & (y < 1.6)) \
        | ((np.minimum(np.abs(y + 0.5), np.abs(y - 1.5)) < SHADOW_BAND) & (x > -0.6) & (x < 1.6)) \
        | ((np.abs(x - y) < SHADOW_BAND) & shadow)
    return pos, faces, eye, pts, shadow, edge


def test_the_blocked_set_of_two_squares_is_the_analytic_shadow():
    pos, faces, eye, pts, shadow, edge = squares_visibility()
    assert edge.mean() < 0.01 and 0.2 < shadow.mean() < 0.3                      # the shadow is a quarter of the receiver
    seen = rm.mesh_visibility(pts, eye, pos, faces)
    assert seen.shape == (1, len(pts))
    assert np.array_equal(seen[0][~edge], ~shadow[~edge])
    # from below the receiver itself is in the way of nothing: its own faces lie at t = 1, outside the range
    assert rm.mesh_visibility(pts, np.array([[0.5, 0.5, -2.0]], f32), pos, faces).all()
    # back-face culling from the eye above: the blocker (normal +z) faces the eye and still blocks; with "front" culled it does not
    assert np.array_equal(rm.mesh_visibility(pts, eye, pos, faces, cull=1)[0][~edge], ~shadow[~edge])
    assert rm.mesh_visibility(pts, eye, pos, faces, cull=2).all()


CYL_SAMPLES = 3000


def cylinder_coverage():
    """the cylinder case of the host and the GPU tests -> (pos, faces, ob_in_cams, K, hw, the area share of the side and top faces)"""
    pos, faces = rm.cylinder()
    P, K, hw = rm.ring_of_views()
    tri = pos[faces].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    n_ang = len(faces) // 4
    return pos, faces, P, K, hw, float(area[:3 * n_ang].sum() / area.sum()), area


def test_view_coverage_of_a_cylinder_from_a_ring_above_its_equator():
    pos, faces, P, K, hw, share, area = cylinder_coverage()
    F, n = len(faces), CYL_SAMPLES
    cov = rm.view_coverage(pos, faces, P, K, hw, n)
    assert abs(cov.fraction - share) <= F / n, (cov.fraction, share)
    counts = np.bincount(cov.face, minlength=F)
    assert np.abs(counts - n * area / area.sum()).max() <= 1.0
    bottom = cov.face >= 3 * (F // 4)
    assert (cov.seen[bottom] == 0).all() and (cov.seen[~bottom] >= 1).all() and cov.seen.dtype == np.int32
    assert len(cov.per_view) == len(P) and all(0.2 < v < 0.6 for v in cov.per_view)      # a view sees the top and under half the side
    assert abs(cov.unseen_area - (1 - cov.fraction) * area.sum()) <= 1e-9 * area.sum() and abs(cov.area - area.sum()) <= 1e-9 * area.sum()
    assert "8 views see" in cov.describe() and cov.as_dict()["samples"] == n
    # a view from below sees the bottom and not the top; outside the frame nothing is seen
    flip = np.diag([1.0, -1.0, -1.0, 1.0])
    below = rm.view_coverage(pos, faces, P[:1] @ flip, K, hw, n)
    top = (below.face >= 2 * (F // 4)) & ~bottom
    assert (below.seen[bottom] == 1).all() and (below.seen[top] == 0).all()
    K_off = K.copy()
    K_off[0, 2] += 5000.0
    assert rm.view_coverage(pos, faces, P, K_off, hw, n).fraction == 0.0
    # min_cos = 0.5 drops the faces seen at more than 60 degrees
    assert rm.view_coverage(pos, faces, P[:1], K, hw, n, min_cos=0.5).fraction < rm.view_coverage(pos, faces, P[:1], K, hw, n).fraction
