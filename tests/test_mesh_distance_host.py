"""CPU: the definition of fp_mesh_point_distance (tests/mesh_distance_model.py, the numpy restatement of include/fp_amd.h) against an
independent float64 formulation and closed forms, the wrong variants its bit-equality gate can see, reconstruct.sample_surface and
compare_meshes through their numpy stand-ins, the refusals that need no device, and two reconstructions through the host TSDF path
(tests/tsdf_model.py): the can, whose accuracy against its true mesh must agree with the distance to the analytic cylinder within the
sag of the true mesh's facets, and the L-prism, the first such figures for a concave object (a measurement, not a gate).

FP_MESH_DISTANCE_PROFILE_OUT=<file> merges the figures of a run into that JSON file (profiles/mesh_distance.json)."""
import ctypes as C
import json
import math
import os
import time

import numpy as np
import pytest
import torch

import mesh_distance_cases as mc
import mesh_distance_model as mm
import tsdf_model as tm
from test_tsdf_host import can_model_volume, can_views  # noqa: F401

f32 = np.float32
U = 2.0 ** -24


def record(key, value):
    path = os.environ.get("FP_MESH_DISTANCE_PROFILE_OUT")
    if not path:
        return
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype.kind == "i" else a.view(np.uint32)


def _same(got, ref):
    return all(np.array_equal(_bits(g), _bits(r)) for g, r in zip(got[:3], ref[:3]))


# ------------------------------------------------------------------ 1. the restatement against float64
def pair_bound(points, tri):
    """A first-order bound on |sqrt(dd32) - d64| per (query, triangle) pair, u = 2^-24.  With l the longest of |ab|, |ac|, |bc|, R the
    largest of |p - a|, |p - b|, |p - c|, M the largest coordinate magnitude of the four points and k = l^2 / (2 area) >= 1:
      * a difference of two float32 inputs has one rounding: |delta| <= u R (u l for an edge vector);
      * a dot product of an edge vector and a query vector is <= l R, its two factors carry u each, every product and both additions
        round once: |delta d_i| <= 6 u l R;
      * an edge quotient t = d / (d - d') has the denominator |edge|^2 >= exactly, so |delta t| <= 2 * 6 u l R / |edge|^2 and the point
        moves by |edge| |delta t| <= 12 u R l / |edge| <= 12 u k R  (an edge is at least 2 area / l = l / k long);
      * va, vb, vc are differences of products of two d_i: |delta| <= 2 (2 * 6 + 1) u (l R)^2 + u (l R)^2 <= 32 u l^2 R^2; the interior
        weights v = vb / D, w = vc / D with D = va + vb + vc = 4 area^2 move by <= (32 + 3 * 32 + 2) u l^2 R^2 / (4 area^2), and the point
        by at most l (|delta v| + |delta w|) <= 65 u l^3 R^2 / area^2 = 260 u k^2 R^2 / l;
      * forming q (two products, two sums, of magnitude <= M) and p - q and its dot product add <= 8 u M + 4 u R.
    A point that moves by e changes the distance by at most e, so
      |sqrt(dd32) - d64| <= u (8 M + 4 R + max(12 k R, 260 k^2 R^2 / l)).
    The interior term is loose by design (in the interior the distance changes only in second order with the point)."""
    p = np.asarray(points, np.float64)[:, None, :]
    t = np.asarray(tri, np.float64)[None]
    a, b, c = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    n = lambda x: np.sqrt((x * x).sum(-1))     # noqa: E731
    l = np.maximum(np.maximum(n(b - a), n(c - a)), n(c - b))
    R = np.maximum(np.maximum(n(p - a), n(p - b)), n(p - c))
    M = np.maximum(np.abs(p).max(-1), np.abs(t).max((-1, -2)))
    area = 0.5 * n(np.cross(b - a, c - a))
    with np.errstate(all="ignore"):
        k = l * l / (2 * area)
        return U * (8 * M + 4 * R + np.maximum(12 * k * R, 260 * k * k * R * R / l))


def test_restatement_against_the_float64_formulation():
    """Every (query, triangle) pair of the smaller generated cases within pair_bound of the float64 formulation.  The bound is a
    worst case over the triangle's shape, about a hundred times the largest error seen: this test tells a wrong region or a wrong
    formula from rounding; a deviation of a few ulps is for the bit-equality against the wrong variants to see, not for it."""
    worst, pairs = 0.0, 0
    for c in mc.all_cases():
        if len(c["faces"]) * len(c["points"]) > 300_000:
            continue
        tri = mm.face_vertices(c["pos"], c["faces"])
        p = tuple(c["points"][:, k][:, None] for k in range(3))
        a, b, cc = (tuple(tri[:, j, k][None, :] for k in range(3)) for j in range(3))
        _, dd, _ = mm.closest_points(p, a, b, cc)
        with np.errstate(all="ignore"):
            ref = np.sqrt(mm.distance2_float64(c["points"], tri))
            bound = pair_bound(c["points"], tri)
            ok = np.isfinite(bound) & np.isfinite(ref) & (dd <= mm.FLT_MAX)
            err = np.abs(np.sqrt(dd.astype(np.float64)) - ref)
        assert (err[ok] <= bound[ok]).all(), (c["name"], float((err[ok] / bound[ok]).max()))
        if ok.any():
            worst = max(worst, float((err[ok] / bound[ok]).max()))
        pairs += int(ok.sum())
    print(f"restatement against float64 over {pairs} pairs: largest |error| / bound = {worst:.3e}")
    assert pairs > 500_000
    record("restatement_vs_float64", dict(pairs=pairs, largest_error_over_bound=worst))


def test_a_cubes_distances_in_closed_form():
    """the distance to the surface of an axis-aligned box: outside |max(|p| - h, 0)|, inside min(h - |p|)"""
    c = next(c for c in mc.all_cases() if c["name"] == "box")
    half = np.abs(c["pos"].astype(np.float64)).max(0)
    p = c["points"].astype(np.float64)
    e = np.abs(p) - half
    exact = np.where((e <= 0).all(1), -e.max(1), np.sqrt((np.maximum(e, 0) ** 2).sum(1)))
    d2, face, closest, _ = mc.references()["box"]
    bound = pair_bound(c["points"], mm.face_vertices(c["pos"], c["faces"])).max(1)
    err = np.abs(np.sqrt(d2.astype(np.float64)) - exact)
    print(f"box: largest |distance - closed form| = {err.max():.3e} m, largest ratio to the bound {float((err / bound).max()):.3e}")
    assert (err <= bound).all()
    assert (d2[:len(c["pos"])] == 0).all()                       # its own vertices lie on it
    assert np.array_equal(closest[:len(c["pos"])], c["pos"])


def test_every_region_is_reached_and_the_smaller_face_wins():
    refs = mc.references()
    for c in mc.all_cases():
        d2, face, closest, region = refs[c["name"]]
        for q, f in c.get("expect_face", {}).items():
            assert face[q] == f, (c["name"], q, face[q], f)
        if "expect_region" in c:
            n = len(c["expect_region"])
            assert tuple(region[:n]) == c["expect_region"], (c["name"], region)
            assert (d2[n:] == 0).all() and np.array_equal(_bits(closest[n:]), _bits(c["points"][n:]))   # queries on the triangle
        none = face < 0
        assert np.isinf(d2[none]).all() and (closest[none] == 0).all() and np.isfinite(d2[~none]).all()
    r = refs["skipped and degenerate"]
    assert set(r[1].tolist()) <= {-1, 0, 1, 2}          # the repeat (3), the mirrored collinear ones (9, 11) and every skipped face lose


@pytest.mark.parametrize("wrong,case", [("strict", "skipped and degenerate"), ("no_edge_bc", "regions x1"), ("larger_index", "ties x1"),
                                        ("contracted", "box"), ("degenerate_a", "skipped and degenerate")])
def test_wrong_variants_are_told_apart(wrong, case):
    c = next(c for c in mc.all_cases() if c["name"] == case)
    got = mm.mesh_point_distance(c["pos"], c["faces"], c["points"], wrong=wrong)
    assert not _same(got, mc.references()[case]), (wrong, case)


# ------------------------------------------------------------------ 2. sample_surface and compare_meshes
def _box(size, t=(0, 0, 0)):
    import geometry_cases as gc
    m = gc.box(size, n=2, t=t)
    return np.asarray(m.vertices, f32), np.asarray(m.faces, np.int32)


def test_sample_surface_is_stratified_inside_its_faces_and_reproducible():
    from foundationpose_amd.reconstruct import _surface_strata, sample_surface
    import geometry_cases as gc
    prism = gc.l_prism()
    bad = np.concatenate([np.asarray(prism.faces), [[0, 1, 99], [-1, 2, 3], [4, 4, 5]]])      # two faces with an index outside the table, one of no area
    for name, verts, faces in (("l_prism", prism.vertices, prism.faces), ("l_prism with bad faces", prism.vertices, bad),
                               ("sliver_soup",) + (lambda m: (m.vertices, m.faces))(gc.sliver_soup(n=300, n_twins=10))):
        pos, faces = np.asarray(verts, f32), np.asarray(faces, np.int32)
        # the faces' areas, computed here: half the norm of the float64 cross product, 0 for a face with an index outside the table
        ok = ((faces >= 0) & (faces < len(pos))).all(1)
        tri64 = pos.astype(np.float64)[np.where(ok[:, None], faces, 0)]
        own_area = np.where(ok, 0.5 * np.linalg.norm(np.cross(tri64[:, 1] - tri64[:, 0], tri64[:, 2] - tri64[:, 0]), axis=1), 0.0)
        for n in (1, 7, 1000):
            pts, f = mm.sample_surface(pos, faces, n, seed=3)
            cum, target, w = _surface_strata(pos, faces, n, 3)
            assert pts.shape == (n, 3) and pts.dtype == f32 and f.shape == (n,)
            assert (w >= 0).all() and (w <= 1).all() and np.abs(w.astype(np.float64).sum(1) - 1).max() <= 4 * U
            # inside its face: the point is the weights' combination of the face's vertices, and the exact distance to that face is rounding
            tri = pos[faces[f]].astype(np.float64)
            comb = (tri * w.astype(np.float64)[:, :, None]).sum(1)
            assert np.abs(pts - comb).max() <= 4 * U * np.abs(pos).max()
            assert np.abs(np.diff(np.concatenate([[0.0], cum])) - own_area).max() <= 1e-12 * own_area.sum(), name     # the table is these areas, summed
            counts = np.bincount(f, minlength=len(faces))
            assert np.abs(counts - n * own_area / own_area.sum()).max() <= 1.0 + 1e-9, name
            assert (counts[own_area == 0] == 0).all()
            again, f2 = mm.sample_surface(pos, faces, n, seed=3)
            assert np.array_equal(_bits(again), _bits(pts)) and np.array_equal(f, f2)
            other, _ = mm.sample_surface(pos, faces, n, seed=4)
            assert n == 1 or not np.array_equal(other, pts)
            # the product's function on host tensors is the stand-in
            tp, tf = sample_surface(dict(pos=torch.as_tensor(pos), faces=torch.as_tensor(faces)), n, seed=3)
            assert np.array_equal(tf.numpy(), f) and np.abs(tp.numpy() - pts).max() <= 4 * U * np.abs(pos).max()
    with pytest.raises(ValueError, match="no area"):
        mm.sample_surface(np.zeros((3, 3), f32), np.array([[0, 1, 2]]), 5)


def test_compare_meshes_on_the_restatement():
    from foundationpose_amd import ops
    size, s = (0.5, 0.25, 1.0), 2.0 ** -6                   # dyadic: the shifted vertices are exact in float32
    a, b = _box(size), _box(size)
    # With samples that are exact -- dyadic weights (1/2, 1/4, 1/4) on the dyadic box: every product and sum is exact in float32 -- a
    # mesh against itself is 0 everywhere, and the samples of the face x = +h are exactly s from the copy shifted by s along x.
    tri = a[0][a[1]]
    exact = (tri[:, 0] * f32(0.5) + tri[:, 1] * f32(0.25)) + tri[:, 2] * f32(0.25)
    d2, face, closest = mm.mesh_point_distance(a[0], a[1], exact)
    assert (d2 == 0).all() and np.array_equal(_bits(closest), _bits(exact))
    plus_x = (tri[:, :, 0] == f32(size[0] / 2)).all(1)
    d2s, _, _ = mm.mesh_point_distance(*_box(size, t=(-s, 0, 0)), exact[plus_x])
    assert plus_x.sum() == 8 and (np.sqrt(d2s) == f32(s)).all()
    # compare_meshes' own samples are float32 combinations (x0*w0 + x1*w1) + x2*w2 with rounded weights, so they lie within rounding
    # of their faces, not on them.  Per coordinate, to first order in u = 2^-24, with M a bound on |coordinate| (1 here: the box
    # reaches 0.5 + s): the three float32 weights are roundings of values that sum to 1, so their sum is 1 within u and a coordinate
    # X shared by the face's vertices comes out as X (1 + delta), |delta| <= u; the three products round once each, together
    # <= u M (the weights sum to 1); the two sums round once each, <= 2 u M: at most 4 u M a coordinate and sqrt(3) * 4 u M < 7 u M
    # for the point; the distance's own arithmetic (p - q, the dot product, the root) adds less than u M.  Hence 8 u M.
    slack = 8 * U * 1.0
    same = mm.compare_meshes(a, b, 600, (slack, 0.01))
    assert isinstance(same, ops.MeshComparison)
    print(f"a box against itself: largest distance {same.hausdorff:.3e} m (8 * 2^-24 = {slack:.3e})")
    assert 0.0 <= same.accuracy.max <= slack and 0.0 <= same.completeness.max <= slack and same.chamfer <= slack
    assert np.array_equal(same.dist_a_to_b, same.dist_b_to_a) and same.accuracy == same.completeness
    assert same.precision == (1.0, 1.0) == same.recall and same.fscore == (1.0, 1.0)
    shifted = _box(size, t=(s, 0, 0))
    thr = tuple(s * k / 8 for k in range(0, 11))
    r = mm.compare_meshes(shifted, b, 600, thr)
    assert r.accuracy.max <= s + slack and r.hausdorff >= s - slack
    pts, f = mm.sample_surface(shifted[0], shifted[1], 600)
    on_face = np.abs(shifted[0][shifted[1][f]][:, :, 0] - (size[0] / 2 + s)).max(1) == 0          # the samples of the face x = +h + s
    assert on_face.sum() > 30 and np.abs(r.dist_a_to_b[on_face] - s).max() <= slack
    assert all(p1 <= p2 for p1, p2 in zip(r.precision, r.precision[1:])) and all(r1 <= r2 for r1, r2 in zip(r.recall, r.recall[1:]))
    assert r.precision[0] < 1.0 and r.precision[-1] == 1.0 and r.recall[-1] == 1.0
    assert r.chamfer == 0.5 * (r.accuracy.mean + r.completeness.mean) and r.hausdorff == max(r.accuracy.max, r.completeness.max)
    for p_, r_, f_ in zip(r.precision, r.recall, r.fscore):
        assert f_ == (2 * p_ * r_ / (p_ + r_) if p_ + r_ > 0 else 0.0)
    d = r.as_dict()
    assert json.loads(json.dumps(d))["samples"] == [600, 600] and "dist_a_to_b" not in d
    # a sample that no triangle answered (+inf) shows in the mean and the maximum and leaves the median alone
    st = ops.DistanceStats.of(np.array([1.0, 2.0, 3.0, np.inf]))
    assert st.mean == np.inf and st.max == np.inf and st.median == 2.5 and st.p99 == np.inf
    gaps = ops.MeshComparison.from_distances(np.array([1.0, np.inf], f32), np.array([1.0, 1.0], f32), (2.0,))
    assert gaps.precision == (0.5,) and gaps.recall == (1.0,) and gaps.chamfer == np.inf and gaps.hausdorff == np.inf


# ------------------------------------------------------------------ 3. refusals that need no device
def test_wrappers_refuse_before_devices():
    from foundationpose_amd import _lib, ops
    from foundationpose_amd.reconstruct import compare_meshes, sample_surface
    pts, pos, faces = torch.zeros(4, 3), torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32)
    for kw, exc, msg in ((dict(want=("dist",)), ValueError, "unknown name 'dist'"),
                         (dict(want=()), ValueError, "want is empty"),
                         (dict(mesh_tensors=dict(pos=pos, faces=faces), pos=pos), _lib.FpAmdError, "not both"),
                         (dict(mesh_tensors=dict(pos=pos)), _lib.FpAmdError, "has no 'faces'"),
                         (dict(), _lib.FpAmdError, "no mesh"),
                         (dict(pos=pos), _lib.FpAmdError, "no mesh"),
                         (dict(pos=pos.numpy(), faces=faces), _lib.FpAmdError, "pos must be a tensor"),
                         (dict(pos=torch.zeros(3, 4), faces=faces), _lib.FpAmdError, r"pos must be \(n,3\)"),
                         (dict(pos=pos, faces=torch.zeros(3, dtype=torch.int32)), _lib.FpAmdError, r"faces must be \(n,3\)"),
                         (dict(points=torch.zeros(3), pos=pos, faces=faces), _lib.FpAmdError, r"points must be \(n,3\)"),
                         (dict(pos=pos, faces=faces, out=dict(normal=pts)), _lib.FpAmdError, "not among the wanted"),
                         (dict(pos=pos, faces=faces, want=("dist2",), out=dict(face=torch.zeros(4, dtype=torch.int32))), _lib.FpAmdError,
                          "not among the wanted"),
                         (dict(pos=pos, faces=faces, out=dict(dist2=torch.zeros(5))), _lib.FpAmdError, r"out\['dist2'\] must be a tensor of shape"),
                         (dict(pos=pos, faces=faces), _lib.FpAmdError, "points: expected a CUDA")):
        args = dict(points=pts)
        args.update(kw)
        with pytest.raises(exc, match=msg):
            ops.mesh_point_distance(**args)
    mesh = dict(pos=pos, faces=faces)
    for fn, kw, msg in ((sample_surface, dict(mesh_tensors=mesh, n=0), "n must be an int >= 1"),
                        (sample_surface, dict(mesh_tensors=mesh, n=True), "n must be an int >= 1"),
                        (sample_surface, dict(mesh_tensors=mesh, n=5, seed=-1), "seed must be an int >= 0"),
                        (sample_surface, dict(mesh_tensors=dict(pos=pos), n=5), "has no 'faces'"),
                        (sample_surface, dict(mesh_tensors=mesh, n=5), "no area"),
                        (sample_surface, dict(mesh_tensors=7, n=5), "must be a mesh-tensor dict or a mesh"),
                        (compare_meshes, dict(a=mesh, b=mesh, samples=0, unit=1.0), "samples must be an int >= 1"),
                        (compare_meshes, dict(a=mesh, b=mesh), "pass unit="),
                        (compare_meshes, dict(a=mesh, b=mesh, unit=0.0), "unit must be a positive length"),
                        (compare_meshes, dict(a=mesh, b=mesh, thresholds=(0.1, float("nan"))), "thresholds must be finite"),
                        (compare_meshes, dict(a=mesh, b=mesh, thresholds=()), "thresholds must be finite"),
                        (compare_meshes, dict(a=dict(pos=torch.zeros(3, 2), faces=faces), b=mesh, unit=1.0), r"a needs pos \(Nv,3\)"),
                        (compare_meshes, dict(a=mesh, b=None, unit=1.0), "b must be a mesh-tensor dict or a mesh")):
        with pytest.raises(ValueError, match=msg):
            fn(**kw)


def test_c_entry_point_reports_argument_errors_without_a_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(16)
    assert lib.fp_mesh_point_distance_workspace_bytes(0) == 0 == lib.fp_mesh_point_distance_workspace_bytes(-3)
    assert lib.fp_mesh_point_distance_workspace_bytes(1000) == 8000

    def call(pos=p, Nv=3, faces=p, F=1, points=p, Q=4, dist2=p, ws=p, ws_bytes=32):
        return lib.fp_mesh_point_distance(pos, Nv, faces, F, points, Q, dist2, None, None, ws, ws_bytes, None)

    for kw, word in ((dict(Q=-1), b"Q=-1"), (dict(Q=(1 << 30) + 1), b"Q="), (dict(F=-1), b"F=-1"), (dict(F=(1 << 30) + 1), b"F="),
                     (dict(Nv=-1), b"Nv=-1"), (dict(points=None), b"NULL points"), (dict(dist2=None), b"NULL points or dist2"),
                     (dict(faces=None), b"faces is NULL"), (dict(pos=None), b"pos is NULL"), (dict(ws=None), b"workspace"),
                     (dict(ws_bytes=31), b"workspace"), (dict(ws=C.c_void_p(20)), b"8-byte aligned")):
        assert call(**kw) == -1, kw
        msg = lib.fp_last_error()
        assert msg.startswith(b"fp_mesh_point_distance") and word in msg, (kw, msg)
    assert call(Q=0, points=None, dist2=None, ws=None, ws_bytes=0) == 0        # nothing to do


# ------------------------------------------------------------------ 4. reconstructions through the host path
def facet_sag(radius, n_ang):
    """how far the chords of a regular n-gon inscribed in a circle lie inside it: the Hausdorff distance between the true can mesh
    (vertices on the cylinder, n_ang facets around) and the analytic cylinder, on the side wall and on the rims of the caps alike"""
    return radius * (1.0 - math.cos(math.pi / n_ang))


CAN_N_ANG = 50          # make_can_mesh's default


def test_the_cans_accuracy_agrees_with_the_analytic_cylinder(scene, can_model_volume):
    """The distance of a point to the true can mesh and its distance to the analytic cylinder differ by at most the Hausdorff distance
    of the two surfaces, the facet sag r (1 - cos(pi / n_ang)) = 0.1006 mm: per sample, and so for the mean, the median, the p99 and
    the maximum.  (+ 1e-7 m for the float32 rounding of the samples and of the distances, coordinates below 0.1 m: 8 * 2^-24 * 0.1.)"""
    pos, col, nrm, faces = tm.extract(can_model_volume)
    true = (np.asarray(scene["mesh"].vertices, f32), np.asarray(scene["mesh"].faces, np.int32))
    n = 2000
    t0 = time.perf_counter()
    pts, _ = mm.sample_surface(pos, faces, n)
    d_mesh = np.sqrt(mm.mesh_point_distance(true[0], true[1], pts)[0].astype(np.float64))
    dt = time.perf_counter() - t0
    d_cyl = tm.cylinder_distance(pts, tm.CAN_RADIUS, tm.CAN_HEIGHT)
    sag = facet_sag(tm.CAN_RADIUS, CAN_N_ANG)
    acc, cyl = (dict(mean=float(d.mean()), median=float(np.median(d)), p99=float(np.percentile(d, 99)), max=float(d.max())) for d in (d_mesh, d_cyl))
    print(f"can at 2.5 mm, {len(faces)} faces, {n} samples: accuracy against the true mesh median {acc['median'] * 1e3:.3f} p99 {acc['p99'] * 1e3:.3f} "
          f"max {acc['max'] * 1e3:.3f} mm; against the cylinder median {cyl['median'] * 1e3:.3f} p99 {cyl['p99'] * 1e3:.3f} max {cyl['max'] * 1e3:.3f} mm; "
          f"largest per-sample difference {np.abs(d_mesh - d_cyl).max() * 1e3:.4f} mm (sag {sag * 1e3:.4f} mm); restatement "
          f"{n} x {len(true[1])} pairs in {dt:.2f} s")
    assert np.abs(d_mesh - d_cyl).max() <= sag + 1e-7
    for k in acc:
        assert abs(acc[k] - cyl[k]) <= sag + 1e-7, (k, acc[k], cyl[k])
    assert acc["max"] <= tm.CAN_VOXEL + sag                                   # the existing gate, seen through the mesh
    record("can_host", dict(faces=len(faces), samples=n, accuracy_vs_true_mesh_m=acc, distance_to_cylinder_m=cyl, facet_sag_m=sag,
                            restatement_seconds=dt, restatement_pairs=n * len(true[1])))


def test_the_l_prism_through_the_host_path():
    """the first reconstruction figures for a concave object: 16 oracle renders of the L-prism fused at 2.5 mm by the host path, then
    accuracy and completeness against the true mesh in voxel edges.  A measurement: nothing but finiteness is asserted."""
    import geometry_cases as gc
    from foundationpose_amd import synthetic as syn
    from oracle import ops as oo
    from oracle import pipeline as op
    from foundationpose_amd.reconstruct import PAD_VOXELS
    mesh = gc.l_prism()
    poses = tm.can_view_poses(16, 0.5).astype(f32)
    out = oo.render_crops(op.mesh_tensors_np(mesh), poses, None, syn.YCBV_K, syn.H, syn.W, (syn.H, syn.W), normalize_xyz=False,
                          want=("color", "depth"))
    depth = np.ascontiguousarray(out["depth"], f32)
    rgb = np.ascontiguousarray(np.clip(out["color"], 0, 1) * 255, f32)
    s = tm.CAN_VOXEL
    v = np.asarray(mesh.vertices)
    lo = v.min(0) - PAD_VOXELS * s
    nx, ny, nz = (int(np.ceil(e / s - 1e-9)) + 1 for e in (v.max(0) + PAD_VOXELS * s - lo))
    vol = tm.Volume((nz, ny, nx), lo.astype(f32), f32(s), f32(4 * s))
    tm.integrate(vol, depth, rgb, (depth > 0).astype(np.uint8), poses, np.tile(syn.YCBV_K[None], (16, 1, 1)))
    pos, col, nrm, faces = tm.extract(vol)
    true = (np.asarray(mesh.vertices, f32), np.asarray(mesh.faces, np.int32))
    r = mm.compare_meshes((pos, faces), true, 1000, tuple(k * s for k in (0.5, 1.0, 2.0, 4.0)))
    vox = lambda st: {k: x / s for k, x in st._asdict().items()}     # noqa: E731
    print(f"l_prism at 2.5 mm: volume {vol.dims}, {len(faces)} faces; in voxel edges: accuracy {vox(r.accuracy)}, completeness "
          f"{vox(r.completeness)}, F-score at 0.5 / 1 / 2 / 4 voxels {r.fscore}")
    assert len(faces) > 1000 and np.isfinite(r.dist_a_to_b).all() and np.isfinite(r.dist_b_to_a).all()
    record("l_prism_host", dict(voxel_m=s, volume=list(vol.dims), faces=len(faces), samples=1000, accuracy_voxels=vox(r.accuracy),
                                completeness_voxels=vox(r.completeness), fscore=dict(zip(("0.5", "1", "2", "4"), r.fscore))))
