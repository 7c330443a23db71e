"""CPU: the definition of the TSDF reconstruction (include/fp_amd.h: fp_tsdf_integrate / fp_tsdf_count_triangles /
fp_tsdf_emit_triangles) through its numpy restatement (tests/tsdf_model.py), which the GPU tests then hold the kernels to bit by bit:
what the definition gives on an analytic sphere and on the can from 16 oracle renders, that each deliberately wrong variant of it is
told apart, streaming, empty input, and every refusal that needs no device.  Each test prints its figures before it asserts.

Measured (profiles/tsdf_reconstruct.json): the can at 2.5 mm from 16 views: 41 514 vertices / 83 024 faces, closed, Euler
characteristic 2, distance to the analytic cylinder median 0.240 / p99 1.143 / max 1.928 mm (the bound is one voxel edge, 2.5 mm; the
worst vertices sit on the caps next to the rims); the sphere of 10 voxels radius: at most 0.0334 voxel edges from the sphere where
the bound allows 0.0375."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import tsdf_model as tm
from conftest import ROOT

f32 = np.float32


# ------------------------------------------------------------------ the table
def test_committed_table_is_the_generated_one_and_the_models():
    import importlib.util
    csrc = os.path.join(ROOT, "foundationpose_amd", "csrc")
    spec = importlib.util.spec_from_file_location("gen_tsdf_tables", os.path.join(csrc, "gen_tsdf_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    text = open(os.path.join(csrc, "tsdf_tables.h")).read()
    assert text == gen.header_text(), "tsdf_tables.h is stale: run gen_tsdf_tables.py"
    rows = re.findall(r"^\s*\{(\d), \{([^}]*)\}\},\s*// case", text, flags=re.M)
    assert len(rows) == 16
    for case, (n, codes) in enumerate(rows):
        codes = [int(c) for c in codes.split(",")]
        tris = [tuple((c >> 2, c & 3) for c in codes[3 * t:3 * t + 3]) for t in range(int(n))]
        assert tris == tm.CASES[case], (case, tris, tm.CASES[case])
    tets = re.findall(r"^\s*\{\{(.*)\}, (\d)\},\s*// axes", text, flags=re.M)
    assert len(tets) == 6
    for (corners, odd), perm in zip(tets, tm.PERMS):
        got = np.asarray([int(x) for x in re.findall(r"\d", corners)]).reshape(4, 3)
        assert np.array_equal(got, tm.tet_corners(perm)) and int(odd) == tm.perm_odd(perm)


# ------------------------------------------------------------------ the analytic sphere
R_VOX, N_SPHERE, S_SPHERE = 10, 29, f32(2.0 ** -8)


def sphere_volume(radius_voxels=R_VOX, n=N_SPHERE, s=S_SPHERE):
    """tsdf = the exact signed distance to a sphere about the volume's middle voxel (in float64, rounded once; not clipped: only its
    sign and its values next to the surface are read), every weight 1.  The radius is a whole number of voxels, so lattice points such as
    (6, 8, 0) lie exactly on the sphere: tsdf is exactly 0 there."""
    h = n // 2
    vol = tm.Volume((n, n, n), np.full(3, -h * float(s)), s, 4 * s)
    ix, iy, iz = vol.coords()
    dist = np.sqrt(((ix - h) ** 2 + (iy - h) ** 2 + (iz - h) ** 2).astype(np.float64)) - radius_voxels
    vol.tsdf[:] = (dist * float(s) / float(vol.trunc)).astype(f32)
    vol.weight[:] = 1
    return vol


def test_sphere_is_a_closed_surface_within_the_interpolation_bound():
    """The bound.  Along a tetrahedron edge of length l <= L = sqrt(3) s the distance function g(t) to a sphere has
    |g''| = (1 - (e.n)^2) / r <= 1 / r, with r the distance to the centre, which is R at the crossing.  The vertex is the zero of the
    chord through g's end values, and a chord of a function with |g''| <= k lies within k l^2 / 8 of it, so the vertex's distance to
    the sphere is at most L^2 / (8 R) = 3 s^2 / (8 R): 0.0375 s for R = 10 s.  (The curvature 1 / R is the surface's; elsewhere on the
    edge r is within L of R, which an edge that crosses the surface more than pays for through its factor 1 - (e.n)^2: measured
    0.0334 s.)  float32: the stored end values, t, the product and the sum round once each relative to a coordinate of at most 16 s, so
    16 ulps of that are allowed on top."""
    vol = sphere_volume()
    assert (vol.tsdf == 0).sum() >= 6 + 24, "no lattice point exactly on the sphere"
    pos, col, nrm, faces = tm.extract(vol)
    bad, edges, euler = tm.edge_report(faces)
    s, R = float(vol.voxel), R_VOX * float(vol.voxel)
    d = np.abs(np.linalg.norm(pos.astype(np.float64), axis=1) - R)
    bound = 3 * s * s / (8 * R) + 16 * 2.0 ** -24 * 16 * s
    print(f"sphere: {len(pos)} vertices, {len(faces)} faces, {bad} bad of {edges} edges, Euler {euler}, max distance {d.max() / s:.4f} "
          f"voxel edges (bound {bound / s:.4f}), volume {tm.signed_volume(pos, faces):.3e}")
    assert len(faces) > 1000 and bad == 0 and euler == 2
    assert tm.repeated_vertex_faces(faces) == 0
    assert tm.signed_volume(pos, faces) > 0.9 * 4 / 3 * np.pi * R ** 3
    assert d.max() <= bound
    # normals point outwards, colours are the grey of a volume without any
    radial = pos.astype(np.float64) / np.linalg.norm(pos.astype(np.float64), axis=1, keepdims=True)
    assert (np.einsum("ij,ij->i", radial, nrm.astype(np.float64)) > 0.99).all() and (col == 128).all()
    counts = tm.count_triangles(vol)
    assert counts.sum() == len(faces) and counts.max() <= 12 and counts.dtype == np.int32


# ------------------------------------------------------------------ wrong variants are told apart
def test_wrong_extraction_variants_change_the_sphere():
    vol = sphere_volume()
    ref = tm.extract(vol)
    # a split that differs between neighbouring cubes: the surface tears
    _, _, _, faces = tm.extract(vol, wrong="split")
    bad, _, _ = tm.edge_report(faces)
    print("split differing between neighbours:", bad, "edges are not shared by exactly two faces")
    assert bad > 0
    # <= for inside: the lattice points on the sphere change sides
    _, _, _, faces = tm.extract(vol, wrong="le")
    print("<= for inside:", len(faces), "faces against", len(ref[3]))
    assert len(faces) != len(ref[3]) or not np.array_equal(faces, ref[3])
    # interpolating from the larger index: still closed, other bits
    pos, _, _, faces = tm.extract(vol, wrong="from_b")
    differ = int((pos.view(np.uint32) != ref[0].view(np.uint32)).any(1).sum())
    print("interpolated from the larger index:", differ, "of", len(pos), "vertices differ in bits")
    assert np.array_equal(faces, ref[3]) and tm.edge_report(faces)[0] == 0 and differ > 0


CASE_DIMS = [(5, 6, 7), (17, 9, 33), (64, 3, 2), (2, 2, 2)]
CASE_VIEWS = [(1, 24, 32, 0), (3, 61, 47, 1), (16, 24, 32, 1), (16, 61, 47, 0)]


def all_generated_cases():
    for dims in CASE_DIMS:
        for V, H, W, kv in CASE_VIEWS:
            yield tm.generated_case(dims, V, H, W, kv, seed=V + H + dims[2], with_masks=(V + dims[0]) % 2 == 1)


def test_generated_views_reach_every_way_through_the_definition():
    total = {}
    for case in all_generated_cases():
        st = {}
        vol = tm.fuse_case(case, stats=st)
        for arr in vol.arrays().values():
            assert np.isfinite(arr).all()
        for k, v in st.items():
            total[k] = total.get(k, 0) + v
    print(total)
    assert all(v > 0 for v in total.values()), total


def test_wrong_integration_variants_change_the_volume():
    case = tm.generated_case((17, 9, 33), 3, 61, 47, 1, seed=1)
    st = {}
    ref = tm.fuse_case(case, stats=st)
    assert st["half"] > 0 and st["hidden"] > 0
    for wrong in ("round", "no_trunc_skip"):
        got = tm.fuse_case(case, wrong=wrong)
        differ = int((got.tsdf.view(np.uint32) != ref.tsdf.view(np.uint32)).sum())
        print(f"{wrong}: {differ} of {ref.tsdf.size} tsdf values differ")
        assert differ > 0


# ------------------------------------------------------------------ streaming, empty input
def test_fusing_in_two_calls_is_fusing_in_one():
    case = tm.generated_case((17, 9, 33), 16, 24, 32, 0, seed=3)
    one = tm.fuse_case(case)
    two = tm.Volume(case["dims"], case["origin"], case["voxel"], case["trunc"])
    for sl in (slice(0, 5), slice(5, 16)):
        tm.integrate(two, case["depth"][sl], case["rgb"][sl], case["masks"][sl], case["ob_in_cams"][sl], case["Ks"][sl], case["min_depth"])
    for k, a in one.arrays().items():
        assert np.array_equal(a.view(np.uint32), two.arrays()[k].view(np.uint32)), k


def test_a_volume_no_view_sees_gives_no_triangle():
    case = tm.generated_case((5, 6, 7), 3, 24, 32, 0, seed=2)
    case["ob_in_cams"][:, 2, 3] = -5.0                     # the volume is behind every camera
    vol = tm.fuse_case(case)
    assert (vol.weight == 0).all() and (vol.tsdf == 1).all()
    assert tm.count_triangles(vol).sum() == 0 and len(tm.emit_triangles(vol)[0]) == 0
    from foundationpose_amd.reconstruct import reconstruct_object
    with pytest.raises(ValueError, match="no views"):
        reconstruct_object([], [], [], [], np.eye(3))
    with pytest.raises(ValueError, match="no views"):
        reconstruct_object(np.zeros((0, 4, 4, 3)), np.zeros((0, 4, 4)), np.zeros((0, 4, 4)), np.zeros((0, 4, 4)), np.eye(3))


# ------------------------------------------------------------------ the can from 16 oracle renders
@pytest.fixture(scope="session")
def can_views(scene):
    return can_reference_views(scene)


def can_reference_views(scene):
    """16 full-frame renders of the can by the CPU oracle from the icosphere at 0.5 m: rgb (V,H,W,3) float32 0..255, depth, masks uint8,
    poses float32, Ks"""
    from oracle import ops as oo
    poses = tm.can_view_poses(16, 0.5).astype(f32)
    out = oo.render_crops(scene["mesh_np"], poses, None, scene["K"], scene["H"], scene["W"], (scene["H"], scene["W"]), normalize_xyz=False,
                          want=("color", "depth"))
    depth = np.ascontiguousarray(out["depth"], f32)
    rgb = np.ascontiguousarray(np.clip(out["color"], 0, 1) * 255, f32)
    return dict(rgb=rgb, depth=depth, masks=(depth > 0).astype(np.uint8), ob_in_cams=poses, Ks=np.tile(scene["K"][None], (16, 1, 1)))


@pytest.fixture(scope="session")
def can_model_volume(can_views):
    origin, dims, s, trunc = tm.can_volume_spec()
    vol = tm.Volume(dims, origin, s, trunc)
    return tm.integrate(vol, can_views["depth"], can_views["rgb"], can_views["masks"], can_views["ob_in_cams"], can_views["Ks"])


def test_the_can_from_16_views(can_model_volume):
    vol = can_model_volume
    pos, col, nrm, faces = tm.extract(vol)
    bad, edges, euler = tm.edge_report(faces)
    d = tm.cylinder_distance(pos, tm.CAN_RADIUS, tm.CAN_HEIGHT) * 1e3
    print(f"can at 2.5 mm: volume {vol.dims}, {len(pos)} vertices / {len(faces)} faces, {bad} bad of {edges} edges, Euler {euler}, "
          f"distance to the cylinder median {np.median(d):.3f} p99 {np.percentile(d, 99):.3f} max {d.max():.3f} mm")
    assert vol.dims == (64, 48, 48)
    assert bad == 0 and euler == 2 and tm.repeated_vertex_faces(faces) == 0 and tm.signed_volume(pos, faces) > 0
    assert d.max() <= 2.5
    assert (col >= 0).all() and (col <= 255).all() and (vol.color_weight > 0).sum() > 1000


# ------------------------------------------------------------------ refusals that need no device
def _cpu_volume(dims=(4, 5, 6)):
    return [torch.ones(dims), torch.zeros(dims), torch.zeros(dims + (3,)), torch.zeros(dims)]


def _cpu_views(V=2, H=8, W=9):
    return dict(depth=torch.ones(V, H, W), rgb=torch.zeros(V, H, W, 3), masks=torch.ones(V, H, W, dtype=torch.uint8),
                ob_in_cams=torch.eye(4).repeat(V, 1, 1), Ks=[np.array([[50.0, 0, 4], [0, 50, 4], [0, 0, 1]])] * V)


def test_wrappers_refuse_shapes_and_values_before_devices():
    from foundationpose_amd import _lib, ops
    E = _lib.FpAmdError
    vol, v = _cpu_volume(), _cpu_views()

    def call(vol=vol, origin=(0, 0, 0), voxel=0.01, trunc=0.04, min_depth=0.001, **kw):
        a = dict(v, **kw)
        return ops.tsdf_integrate(*vol, a["depth"], a["rgb"], a["masks"], a["ob_in_cams"], a["Ks"], origin, voxel, trunc, min_depth)

    with pytest.raises(E, match="rgb must be"):
        call(rgb=torch.zeros(2, 8, 9, 4))
    with pytest.raises(E, match="depth must"):
        call(depth=torch.ones(8, 9))
    with pytest.raises(E, match="masks must be"):
        call(masks=torch.ones(2, 8, 8, dtype=torch.uint8))
    with pytest.raises(E, match="ob_in_cams must be"):
        call(ob_in_cams=torch.eye(4).repeat(3, 1, 1))
    with pytest.raises(E, match="weight must be"):
        call(vol=[vol[0], torch.zeros(4, 5, 5), vol[2], vol[3]])
    with pytest.raises(E, match="color must be"):
        call(vol=[vol[0], vol[1], torch.zeros(4, 5, 6), vol[3]])
    with pytest.raises(E, match="tsdf must be"):
        call(vol=[torch.ones(4, 30)] + vol[1:])
    with pytest.raises(E, match="intrinsic matrices"):
        call(Ks=v["Ks"][:1])
    with pytest.raises(ValueError, match="skew"):
        call(Ks=[np.array([[50.0, 0.1, 4], [0, 50, 4], [0, 0, 1]])] * 2)
    for bad in (dict(voxel=0.0), dict(voxel=float("nan")), dict(trunc=-1.0), dict(trunc=float("inf")), dict(min_depth=-0.1),
                dict(origin=(0, float("nan"), 0)), dict(origin=(0, 0))):
        with pytest.raises(ValueError):
            call(**bad)
    # values are refused before the device is looked at, and CPU tensors last of all
    with pytest.raises(ValueError, match="trunc"):
        call(trunc=0.0)
    with pytest.raises(E, match="CUDA"):
        call()
    with pytest.raises(E, match="CUDA"):
        ops.tsdf_extract(*vol, (0, 0, 0), 0.01)
    with pytest.raises(ValueError, match="min_weight"):
        ops.tsdf_extract(*vol, (0, 0, 0), 0.01, min_weight=float("nan"))
    with pytest.raises(ValueError, match="voxel"):
        ops.tsdf_extract(*vol, (0, 0, 0), -1.0)
    from foundationpose_amd.reconstruct import TsdfVolume, bounds_from_views
    with pytest.raises(ValueError, match="masks are required"):
        bounds_from_views(np.ones((1, 4, 4)), None, np.eye(4)[None], np.eye(3))
    with pytest.raises(ValueError, match="dims"):
        TsdfVolume((0, 0, 0), (4, 4), 0.01, device="cpu")


def test_c_entry_points_report_argument_errors_without_a_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    p, o = C.c_void_p(16), (C.c_float * 3)(0, 0, 0)
    bad_o = (C.c_float * 3)(0, float("inf"), 0)

    def integ(V=1, H=8, W=8, nz=4, ny=4, nx=4, origin=o, voxel=0.01, trunc=0.04, min_depth=0.001, depth=p, tsdf=p):
        return lib.fp_tsdf_integrate(depth, p, None, p, p, V, H, W, nz, ny, nx, origin, voxel, trunc, min_depth, tsdf, p, p, p, None)

    for kw, word in ((dict(V=-1), b"V=-1"), (dict(V=5000), b"V=5000"), (dict(H=0), b"H=0"), (dict(H=1 << 15, W=1 << 15), b"2^28"),
                     (dict(nx=0), b"dimension"), (dict(nz=5000), b"dimension"), (dict(nz=2048, ny=2048, nx=2048), b"2^30"),
                     (dict(origin=None), b"NULL origin"), (dict(origin=bad_o), b"not finite"), (dict(voxel=0.0), b"voxel"),
                     (dict(voxel=float("nan")), b"voxel"), (dict(trunc=0.0), b"trunc"), (dict(min_depth=-1.0), b"min_depth"),
                     (dict(tsdf=None), b"NULL volume"), (dict(depth=None), b"NULL depth")):
        assert integ(**kw) == -1, kw
        msg = lib.fp_last_error()
        assert msg.startswith(b"fp_tsdf_integrate") and word in msg, (kw, msg)
    assert integ(V=0, depth=None) == 0                                        # nothing to do
    assert lib.fp_tsdf_count_triangles(p, p, 4, 0, 4, 1.0, p, None) == -1 and b"fp_tsdf_count_triangles" in lib.fp_last_error()
    assert lib.fp_tsdf_count_triangles(p, p, 4, 4, 4, float("nan"), p, None) == -1 and b"min_weight" in lib.fp_last_error()
    assert lib.fp_tsdf_count_triangles(None, p, 4, 4, 4, 1.0, p, None) == -1 and b"NULL" in lib.fp_last_error()
    assert lib.fp_tsdf_count_triangles(None, None, 4, 1, 4, 1.0, None, None) == 0   # no cubes

    def emit(nz=4, total=10, origin=o, voxel=0.01, mw=1.0, keys=p):
        return lib.fp_tsdf_emit_triangles(p, p, p, p, nz, 4, 4, origin, voxel, mw, p, total, keys, p, p, p, None)

    for kw, word in ((dict(nz=0), b"dimension"), (dict(total=-1), b"total"), (dict(total=(1 << 29) + 1), b"total"), (dict(origin=None), b"origin"),
                     (dict(voxel=-1.0), b"voxel"), (dict(mw=float("inf")), b"min_weight"), (dict(keys=None), b"NULL")):
        assert emit(**kw) == -1, kw
        msg = lib.fp_last_error()
        assert msg.startswith(b"fp_tsdf_emit_triangles") and word in msg, (kw, msg)
    assert emit(total=0, keys=None) == 0 and emit(nz=1, keys=None) == 0       # nothing to do
