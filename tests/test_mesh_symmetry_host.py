"""CPU: the definition of fp_mesh_transform_residuals (tests/mesh_symmetry_model.py, the numpy restatement of include/fp_amd.h): the
identity gives fp_mesh_point_distance's restatement, the wrong variants its bit-equality gate can see; the symmetry detector
(foundationpose_amd/symmetry.py) driven through the restatement on shapes whose rotation groups are known in closed form, each in a
random rigid pose; the bound of its coarse scan on random axis pairs; the project's can, true and fused through the host TSDF path
(tests/tsdf_model.py); and the refusals that need no device.

FP_MESH_DISTANCE_PROFILE_OUT=<file> merges the figures of a run into that JSON file (test_mesh_distance_host.record)."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

import mesh_distance_cases as mc
import mesh_distance_model as mm
import mesh_symmetry_cases as sc
import mesh_symmetry_model as sm
import tsdf_model as tm
from test_mesh_distance_host import _bits, facet_sag, record
from test_tsdf_host import can_model_volume, can_views  # noqa: F401

f32 = np.float32


# ------------------------------------------------------------------ 1. the restatement
def test_identity_gives_the_point_distance_restatement():
    for name in ("box", "skipped and degenerate", "soup F=257 Q=64"):
        c = next(c for c in mc.all_cases() if c["name"] == name)
        eye = np.eye(4, dtype=f32)[None].copy()
        eye[0, 3] = [np.nan, 5.0, -np.inf, 0.0]                   # the fourth row is never read
        max_d2, over, dist2 = sm.mesh_transform_residuals(c["pos"], c["faces"], c["points"], eye, sm.square_thresholds([0.0]))
        ref = mc.references()[name][0]
        assert dist2.shape == (1, len(c["points"])) and np.array_equal(_bits(dist2[0]), _bits(ref))
        assert _bits(max_d2)[0] == _bits(ref.max()[None])[0] and over[0, 0] == int((ref > 0).sum())


def test_empty_inputs_and_unanswered_points():
    box = next(c for c in mc.all_cases() if c["name"] == "box")
    tfs = sc.rigid_transforms(3, 1, 0.1)
    thr2 = sm.square_thresholds([0.01, np.inf])
    max_d2, over, dist2 = sm.mesh_transform_residuals(box["pos"], box["faces"], box["points"][:0], tfs, thr2)
    assert max_d2.tolist() == [0, 0, 0] and over.tolist() == [[0, 0]] * 3 and dist2.shape == (3, 0)
    max_d2, over, dist2 = sm.mesh_transform_residuals(box["pos"], box["faces"][:0], box["points"][:5], tfs, thr2)
    assert np.isposinf(max_d2).all() and over.tolist() == [[5, 0]] * 3 and np.isposinf(dist2).all()      # +inf > +inf does not hold
    none = sm.mesh_transform_residuals(box["pos"], box["faces"], box["points"], tfs[:0], thr2)
    assert none[0].shape == (0,) and none[1].shape == (0, 2) and none[2].shape == (0, len(box["points"]))
    c = next(c for c in sc.kernel_cases() if c["name"] == "box special transforms")
    ref = sm.mesh_transform_residuals(c["pos"], c["faces"], c["points"], c["tfs"], c["thr2"])
    assert np.isfinite(ref[0][:3]).all() and np.isposinf(ref[0][3:]).all()      # NaN entry, infinite translation, overflow: unanswered
    assert (ref[1][3:] == 300).all()


@pytest.mark.parametrize("wrong,case", [("translate_first", "box three transforms"), ("transposed", "box three transforms"), ("ge", "thresholds on values"),
                                        ("min", "box three transforms"), ("nonfinite_zero", "box special transforms")])
def test_wrong_variants_are_told_apart(wrong, case):
    if case == "thresholds on values":
        c = threshold_case()
    else:
        c = next(c for c in sc.kernel_cases() if c["name"] == case)
    ref = sm.mesh_transform_residuals(c["pos"], c["faces"], c["points"], c["tfs"], c["thr2"])
    got = sm.mesh_transform_residuals(c["pos"], c["faces"], c["points"], c["tfs"], c["thr2"], wrong=wrong)
    assert not all(np.array_equal(_bits(g), _bits(r)) for g, r in zip(got, ref)), (wrong, case)


def threshold_case():
    """thresholds exactly on a value of the matrix and one ulp either side of it: `>` and `>=` differ in exactly one count"""
    c = next(c for c in sc.kernel_cases() if c["name"] == "box three transforms")
    d2 = sm.mesh_transform_residuals(c["pos"], c["faces"], c["points"], c["tfs"])[2]
    v = np.sort(d2[1])[len(d2[1]) // 2]
    assert v > 0
    thr2 = np.array([np.nextafter(v, f32(0)), v, np.nextafter(v, f32(np.inf)), np.nan], f32)
    return dict(c, name="thresholds on values", thr2=thr2)


def test_thresholds_on_a_value_and_one_ulp_either_side():
    c = threshold_case()
    max_d2, over, dist2 = sm.mesh_transform_residuals(c["pos"], c["faces"], c["points"], c["tfs"], c["thr2"])
    n_eq = int((dist2[1] == c["thr2"][1]).sum())
    assert n_eq >= 1 and over[1, 0] - over[1, 1] == n_eq and over[1, 1] - over[1, 2] <= n_eq and (over[:, 3] == 0).all()
    assert over[1, 0] > over[1, 1] >= over[1, 2]


def test_square_thresholds_rounds_once():
    t = np.array([0.1, 1e-3, 3.3333], np.float64)
    assert np.array_equal(_bits(sm.square_thresholds(t)), _bits(t.astype(f32) * t.astype(f32)))
    assert sm.square_thresholds(None).shape == (0,)


# ------------------------------------------------------------------ 2. the detector's pieces
def test_coarse_bound_holds_on_random_axis_pairs():
    """|R_a(theta) v - R_a'(theta) v| <= 4 sin(theta/2) sin(delta/2) |v| for axes delta apart (symmetry.coarse_bound has the proof):
    checked as the operator norm of the difference, on random pairs, small and large angles, every tested order"""
    from foundationpose_amd.symmetry import axis_rotation, coarse_bound, covering_angle, hemisphere_axes
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(2000):
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        p = np.cross(a, rng.normal(size=3))
        p /= np.linalg.norm(p)
        delta = float(rng.choice([1e-3, 0.02, 0.08, 0.3, 1.0, math.pi / 2, 3.0])) * rng.uniform(0.5, 1.0)
        b = math.cos(delta) * a + math.sin(delta) * p
        theta = 2 * math.pi / int(rng.choice([2, 3, 4, 5, 6, 7, 11]))
        diff = np.linalg.norm(axis_rotation(a, theta) - axis_rotation(b, theta), 2)
        bound = coarse_bound(theta, delta, 1.0)
        assert diff <= bound * (1 + 1e-9) + 1e-15, (delta, theta, diff, bound)
        worst = max(worst, diff / bound)
    assert worst > 0.99                                            # and it is tight: nothing is given away
    # the covering angle covers: no random direction is farther from the spiral (up to sign) than it says
    for n in (8, 100, 800):
        ax = hemisphere_axes(n)
        assert np.allclose(np.linalg.norm(ax, axis=1), 1.0) and (ax[:, 2] > 0).all()
        d = rng.normal(size=(20000, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        far = np.arccos(np.clip(np.abs(d @ ax.T).max(axis=1), -1, 1)).max()
        assert far <= covering_angle(ax), (n, far, covering_angle(ax))
    assert covering_angle(hemisphere_axes(800)) < math.radians(6.0)


HALF = dict(samples=(64, 256))     # half the default fine samples where the refinement steps are most of the time: the same groups
SHAPES = {
    "cube": (lambda: sc.box_shape(1, 1, 1), sc.cube_group, {}),
    "box 1x2x3": (lambda: sc.box_shape(1, 2, 3), lambda: sc.dihedral(2), {}),
    "box 1x1x2": (lambda: sc.box_shape(1, 1, 2), lambda: sc.dihedral(4), {}),
    "pentagonal prism": (lambda: sc.prism(5, 1.0, 1.5), lambda: sc.dihedral(5), HALF),
    "hexagonal prism": (lambda: sc.prism(6, 1.0, 1.5), lambda: sc.dihedral(6), HALF),
    "tetrahedron": (sc.tetrahedron, sc.tetrahedral_group, {}),
    "L-prism": (sc.l_prism_shape, lambda: np.stack([np.eye(3), np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, -1]])]), {}),
    "pulled box": (sc.pulled_box, lambda: np.eye(3)[None], HALF),
    # fewer axes and samples than the defaults: 200 faces make the restatement's refinement steps the cost of this file
    "50-gon prism": (lambda: sc.prism(50, 0.051, 0.140), lambda: sc.continuous_group(5, flip=True), dict(n_axes=120, samples=(48, 128), max_order=3)),
    "heptagonal prism": (lambda: sc.prism(7, 1.0, 1.5), lambda: sc.dihedral(7), HALF),
}
SIZES = {"cube": 24, "box 1x2x3": 4, "box 1x1x2": 8, "pentagonal prism": 10, "hexagonal prism": 12, "tetrahedron": 12, "L-prism": 2,
         "pulled box": 1, "50-gon prism": 144, "heptagonal prism": 14}


def group_tolerance(rec, radius):
    """How far a returned rotation may be from the expected one, as an angle.  A returned transform moves no fine sample by more than
    tol off the surface, but the surface may slide along itself, so tol / radius is no bound on the angle by itself; what is bounded
    is the axis: the detector treats axes within max(1 degree, 2 tol / radius) as one, and a rotation about an axis that far off
    differs from the true one by at most twice that angle (symmetry.coarse_bound: 4 sin(theta/2) sin(delta/2) <= 2 delta)."""
    return 2.0 * max(math.radians(1.0), 2.0 * rec.tol / radius)


@pytest.mark.parametrize("name", list(SHAPES))
def test_closed_form_groups(name):
    from foundationpose_amd.symmetry import surface_centre
    shape, group, kw = SHAPES[name]
    pos, faces, R, t = sc.posed(shape(), seed=3 + len(name))
    t0 = time.perf_counter()
    rec = sm.host_symmetries(pos, faces, **kw)
    dt = time.perf_counter() - t0
    centre, radius = surface_centre(pos, faces)
    expected = R @ group() @ R.T                                   # the group in the posed frame
    ok, worst = sc.match_groups(rec.tfs[:, :3, :3], expected, group_tolerance(rec, radius))
    print(f"{name}: {len(rec.tfs)} transforms (expected {SIZES[name]}), largest residual {rec.residuals.max() / (2 * radius):.2e} of the "
          f"diameter (tol {rec.tol / (2 * radius):.2e}), largest angle to the expected rotation {math.degrees(worst):.4f} deg, {dt:.1f} s")
    assert len(expected) == SIZES[name] and len(rec.tfs) == SIZES[name], (name, len(rec.tfs))
    assert ok, (name, worst)
    assert np.array_equal(rec.tfs[0], np.eye(4)) or np.allclose(rec.tfs[0], np.eye(4), atol=1e-12)
    assert (rec.residuals <= rec.tol).all() and len(rec.residuals) == len(rec.tfs)           # the postcondition
    assert np.abs(rec.tfs[:, :3, :3] @ centre + rec.tfs[:, :3, 3] - centre).max() <= 1e-9 * radius   # every transform fixes the centre
    orders = sorted({k for _, k in rec.axes}, key=float)
    if name == "50-gon prism":
        assert orders == [2, math.inf] and abs(abs(rec.continuous_axis @ R[:, 2]) - 1) < 1e-4
    if name == "heptagonal prism":
        assert orders == [2, 7]                                    # the order-7 axis comes from the probe order 7 passing while 11 fails
    record(f"symmetry_host {name}", dict(transforms=len(rec.tfs), residual_over_diameter=float(rec.residuals.max() / (2 * radius)),
                                         largest_angle_deg=math.degrees(worst), seconds=dt))


def test_a_sphere_is_refused():
    """two continuous axes that are not parallel: the callables of an exact sphere (every rotation about the centre leaves every
    sample on the surface, and the closest point of a moved sample is itself)"""
    from foundationpose_amd.symmetry import find_symmetries
    x = np.random.default_rng(1).normal(size=(64, 3))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    with pytest.raises(ValueError, match="two continuous axes"):
        find_symmetries(lambda tfs, which: np.zeros(len(tfs)), lambda tf: (x, x @ tf[:3, :3].T + tf[:3, 3]), np.zeros(3), 1.0, 0.01, n_axes=60)


# ------------------------------------------------------------------ 3. the project's can
def _about_z(angle):
    from foundationpose_amd.symmetry import about, axis_rotation
    return about(np.zeros(3), axis_rotation((0, 0, 1), angle))


def test_the_true_can_is_a_body_of_revolution_with_a_flip(scene):
    """make_can_mesh: 50 facets around, flat caps that are fans from their centres, the side's quads planar.  As a set of points it is
    the right prism over a regular 50-gon, centred at the origin with its axis along z: the rotations about z by multiples of 7.2
    degrees and the half turns about the 50 axes in the plane z = 0 through the vertices' and the edges' directions map it onto itself
    exactly (the caps are equal, so it is flip-symmetric); a rotation about z by any other angle moves it by at most the facet sag,
    r (1 - cos(pi / 50)) = 0.1006 mm, which is far below 1 % of its extent: the expected set is the continuous axis with one flip, 144
    transforms at 5 degrees.  Checked here on the full mesh with the kernel's restatement on 256 stratified samples."""
    from foundationpose_amd.symmetry import about, axis_rotation, surface_centre
    mesh = scene["mesh"]
    pos, faces = np.asarray(mesh.vertices, f32), np.asarray(mesh.faces, np.int32)
    centre, radius = surface_centre(pos, faces)
    assert np.abs(centre).max() < 1e-9 and abs(radius - math.hypot(tm.CAN_RADIUS, tm.CAN_HEIGHT / 2)) < 1e-6
    pts, _ = mm.sample_surface(pos, faces, 256)
    half = math.pi / 50
    tfs = np.stack([_about_z(2 * half), _about_z(2 * math.pi / 7), _about_z(2 * math.pi / 11), _about_z(math.radians(5)),
                    about(np.zeros(3), axis_rotation((1, 0, 0), math.pi)), about(np.zeros(3), axis_rotation((math.cos(half), math.sin(half), 0), math.pi)),
                    about(np.zeros(3), axis_rotation((math.cos(0.3), math.sin(0.3), 0), math.pi)), about(np.zeros(3), axis_rotation((0, 0.6, 0.8), math.pi))])
    res = np.sqrt(sm.mesh_transform_residuals(pos, faces, pts, tfs.astype(f32))[0].astype(np.float64))
    sag = facet_sag(tm.CAN_RADIUS, 50)
    print("true can, residuals in mm:", np.round(res * 1e3, 5).tolist(), f"(sag {sag * 1e3:.4f} mm)")
    # float32, u = 2^-24, coordinates below M = 0.1 m, to first order: a sample lies within 7 u M of its face (test_mesh_distance_host:
    # 4 u M a coordinate); the matrix entries are rounded (u each, three to a row), the row's three products and three sums round
    # once each: 9 u M a coordinate, 16 u M for the point; the distance's own arithmetic adds less than u M.  24 u M = 0.14 um.
    exact = 24 * 2.0 ** -24 * 0.1
    assert res[0] <= exact and res[4] <= exact and res[5] <= exact      # its own symmetries
    assert (res[[1, 2, 3, 6]] <= sag + exact).all()                # any angle about z, any flip axis in the plane: within the sag
    assert res[7] > 0.01                                           # a tilted half turn is none
    record("symmetry_true_can", dict(residuals_m=res.tolist(), facet_sag_m=sag))


FUSED_SAMPLES = 128      # 2 x 128 x ~84 000 pair tests for the restatement


def test_the_fused_cans_axis_residual(scene, can_model_volume):
    """The can fused by the host TSDF path at 2.5 mm from noiseless views: how far do the rotations by 2 pi / 7 and 2 pi / 11 about its
    true axis (z through the origin of the views' frame) move its surface off itself?  Measured here: 1.007 mm and 1.050 mm on 128
    samples, 0.4 voxels (the marching-tetrahedra facets of the 2.5 mm grid, not noise).  The detector's tolerance for a fused mesh is twice such a figure and no less than one voxel;
    FoundationPose.detect_symmetries takes two voxels.  (The detector itself is run on a fused can on the device,
    tests/test_gpu_mesh_symmetry.py: the coarse scan over ~84 000 faces is out of the restatement's reach.)"""
    pos, col, nrm, faces = tm.extract(can_model_volume)
    pts, _ = mm.sample_surface(pos, faces, FUSED_SAMPLES)
    tfs = np.stack([_about_z(2 * math.pi / 7), _about_z(2 * math.pi / 11)]).astype(f32)
    t0 = time.perf_counter()
    res = np.sqrt(sm.mesh_transform_residuals(pos, faces, pts, tfs)[0].astype(np.float64))
    print(f"fused can, {len(faces)} faces, {FUSED_SAMPLES} samples: residual of the true axis at 2pi/7 {res[0] * 1e3:.4f} mm, at 2pi/11 "
          f"{res[1] * 1e3:.4f} mm (voxel {tm.CAN_VOXEL * 1e3} mm), {time.perf_counter() - t0:.1f} s")
    assert (res <= tm.CAN_VOXEL).all()                             # the fusion's own gate: within one voxel of the true surface
    record("symmetry_fused_can_host", dict(faces=len(faces), samples=FUSED_SAMPLES, residual_2pi_7_m=float(res[0]), residual_2pi_11_m=float(res[1]),
                                           detector_tol_m=float(max(2 * res.max(), tm.CAN_VOXEL))))


# ------------------------------------------------------------------ 4. refusals that need no device
def test_wrappers_refuse_before_devices():
    from foundationpose_amd import _lib, ops
    from foundationpose_amd.reconstruct import detect_symmetries
    from foundationpose_amd.symmetry import find_symmetries
    pts, pos, faces, tfs = torch.zeros(4, 3), torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32), torch.zeros(2, 4, 4)
    for kw, exc, msg in ((dict(want=("max",)), ValueError, "unknown name 'max'"),
                         (dict(want=()), ValueError, "want is empty"),
                         (dict(thresholds=(1, 2, 3, 4, 5)), ValueError, "5 thresholds"),
                         (dict(thresholds=(0.1, -1.0)), ValueError, "lengths >= 0"),
                         (dict(thresholds=(float("nan"),)), ValueError, "lengths >= 0"),
                         (dict(mesh_tensors=dict(pos=pos, faces=faces), pos=pos), _lib.FpAmdError, "not both"),
                         (dict(mesh_tensors=dict(pos=pos)), _lib.FpAmdError, "has no 'faces'"),
                         (dict(pos=None), _lib.FpAmdError, "no mesh"),
                         (dict(pos=pos.numpy()), _lib.FpAmdError, "pos must be a tensor"),
                         (dict(pos=torch.zeros(3, 4)), _lib.FpAmdError, r"pos must be \(n,3\)"),
                         (dict(points=torch.zeros(3)), _lib.FpAmdError, r"points must be \(n,3\)"),
                         (dict(tfs=tfs.numpy()), _lib.FpAmdError, "tfs must be a tensor"),
                         (dict(tfs=torch.zeros(2, 3, 4)), _lib.FpAmdError, r"tfs must be \(T,4,4\)"),
                         (dict(tfs=torch.zeros(4, 4)), _lib.FpAmdError, r"tfs must be \(T,4,4\)"),
                         (dict(out=dict(normal=pts)), _lib.FpAmdError, "not among the wanted"),
                         (dict(out=dict(over=torch.zeros((2, 0), dtype=torch.int32))), _lib.FpAmdError, "not among the wanted"),
                         (dict(out=dict(dist2=torch.zeros(2, 4))), _lib.FpAmdError, "not among the wanted"),
                         (dict(want=("dist2",), out=dict(dist2=torch.zeros(4, 2))), _lib.FpAmdError, r"out\['dist2'\] must be a tensor of shape"),
                         (dict(thresholds=(0.1,), out=dict(over=torch.zeros((2, 2), dtype=torch.int32))), _lib.FpAmdError, r"out\['over'\] must be"),
                         (dict(), _lib.FpAmdError, "points: expected a CUDA")):
        args = dict(points=pts, tfs=tfs, pos=pos, faces=faces)
        args.update(kw)
        if "mesh_tensors" in kw and "pos" not in kw:
            args.pop("pos"), args.pop("faces")
        elif "mesh_tensors" in kw:
            args.pop("faces")
        with pytest.raises(exc, match=msg):
            ops.mesh_transform_residuals(**args)
    mesh = dict(pos=pos, faces=faces)
    for kw, msg in ((dict(mesh_tensors=7), "must be a mesh-tensor dict or a mesh"), (dict(mesh_tensors=dict(pos=pos)), "has no 'faces'"),
                    (dict(mesh_tensors=mesh, samples=5), "samples must be two counts"), (dict(mesh_tensors=mesh, samples=(0, 5)), r"samples\[0\] must be an int >= 1"),
                    (dict(mesh_tensors=mesh), "no area")):
        with pytest.raises(ValueError, match=msg):
            detect_symmetries(**kw)
    never = lambda *a: pytest.fail("a callable was used before the arguments were checked")     # noqa: E731
    for kw, msg in ((dict(tol=0.0), "tol must be a positive length"), (dict(tol=float("nan")), "tol must be a positive length"),
                    (dict(radius=0.0), "radius a positive length"), (dict(max_order=1), "max_order must be an int >= 2"),
                    (dict(max_order=2.5), "max_order must be an int >= 2"), (dict(n_axes=3), "n_axes must be an int >= 8"),
                    (dict(rot_angle_discrete=0), "rot_angle_discrete must be an angle")):
        args = dict(residuals=never, closest=never, centre=np.zeros(3), radius=1.0, tol=0.01)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            find_symmetries(**args)


def test_c_entry_point_reports_argument_errors_without_a_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(16)
    wsb = lib.fp_mesh_transform_residuals_workspace_bytes
    assert wsb(0, 5) == 0 == wsb(5, 0) == wsb(-3, 5) == wsb(5, -1) and wsb(800, 64) == 4 * 800 * 64 and wsb(1 << 20, 1 << 10) == 1 << 32

    def call(pos=p, Nv=3, faces=p, F=1, points=p, Q=4, tfs=p, T=2, thr2=p, L=1, max_d2=p, over=p, ws=p, ws_bytes=32):
        return lib.fp_mesh_transform_residuals(pos, Nv, faces, F, points, Q, tfs, T, thr2, L, max_d2, over, None, ws, ws_bytes, None)

    for kw, word in ((dict(Q=-1), b"Q=-1"), (dict(T=-1), b"T=-1"), (dict(T=1 << 20, Q=(1 << 10) + 1), b"above 2^30"), (dict(F=-1), b"F=-1"),
                     (dict(F=(1 << 30) + 1), b"F="), (dict(Nv=-1), b"Nv=-1"), (dict(L=5), b"L=5"), (dict(L=-1), b"L=-1"),
                     (dict(max_d2=None), b"NULL max_d2"), (dict(thr2=None), b"NULL thr2 or over"), (dict(over=None), b"NULL thr2 or over"),
                     (dict(points=None), b"NULL points or tfs"), (dict(tfs=None), b"NULL points or tfs"), (dict(faces=None), b"faces is NULL"),
                     (dict(pos=None), b"pos is NULL"), (dict(ws=None), b"workspace"), (dict(ws_bytes=31), b"workspace"),
                     (dict(ws=C.c_void_p(18)), b"4-byte aligned")):
        assert call(**kw) == -1, kw
        msg = lib.fp_last_error()
        assert msg.startswith(b"fp_mesh_transform_residuals") and word in msg, (kw, msg)
    assert call(T=0, points=None, tfs=None, max_d2=None, thr2=None, over=None, ws=None, ws_bytes=0) == 0        # nothing to do
