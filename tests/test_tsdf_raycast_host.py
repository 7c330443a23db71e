"""CPU: the definition of fp_tsdf_raycast (include/fp_amd.h) through its numpy restatement (tests/tsdf_raycast_model.py), which the GPU
tests then hold the kernel to bit by bit: what the definition gives on an analytic sphere, on a single fused view and on the can from 16
oracle renders (against the extracted mesh, through the ICP, and in sequential fusion), that each deliberately wrong variant of it is
told apart, that the generated cases reach every branch, and every refusal that needs no device.  Each test prints its figures before
it asserts.  The measured figures the gates rest on are in profiles/tsdf_raycast.json; FP_TSDF_RAYCAST_PROFILE_OUT=<file> collects the
figures of a run there."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest
import torch

import icp_model as im
import tsdf_model as tm
import tsdf_raycast_model as rm
from conftest import ROOT
from test_tsdf_host import can_model_volume, can_views, sphere_volume  # noqa: F401

f32 = np.float32


def profile():
    return json.load(open(os.path.join(ROOT, "profiles", "tsdf_raycast.json")))


def record(section, figures):
    path = os.environ.get("FP_TSDF_RAYCAST_PROFILE_OUT")
    if not path:
        return
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[section] = figures
    with open(path, "w") as f:
        json.dump(data, f, indent=1)


def _rays64(pose, K, oh, ow):
    """float64 rays of a full-frame view in the object frame -> (o (3,), d (oh,ow,3)); a point is o + z d"""
    T = np.asarray(pose, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    u, v = np.meshgrid(np.arange(ow) + 0.5, np.arange(oh) + 0.5)
    dc = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)
    return -R.T @ t, dc @ R


# ------------------------------------------------------------------ 1. the analytic sphere
def test_sphere_depth_and_normals():
    """The sphere of 10 voxels radius (sphere_volume: the exact distance at every voxel, fully observed) seen full frame at 64 x 64 from
    40 voxels away, under a tilted pose.  Every pixel whose exact ray passes at least one voxel inside the silhouette is a hit, none
    whose ray passes more than one voxel outside is.  Over the former, the depth against the exact ray-sphere intersection and the
    normal against the radial direction: measured here (no bound was derived: near the silhouette the depth error is the field's
    error over the cosine of the incidence, which is not bounded away from 0) and gated at twice the measured maxima, the margin of
    tests/test_icp_host.py's convergence gate -- profiles/tsdf_raycast.json "sphere": depth_max_voxels 0.0714 (median 0.0269),
    normal_max_deg 0.402, over 1677 pixels."""
    vol = sphere_volume()
    s, R = float(vol.voxel), 10 * float(vol.voxel)
    pose = np.eye(4)
    pose[:3, :3] = rm._rot((1.0, 0.4, 0.2), 25.0)
    pose[:3, 3] = (0.3 * s, -0.2 * s, 40 * s)
    K = np.array([[100.0, 0, 32.0], [0, 100.0, 32.0], [0, 0, 1]])
    out = rm.raycast(vol, pose.astype(f32)[None], K, 64, 64)
    o, d = _rays64(pose.astype(f32), K, 64, 64)
    # closest approach of each ray to the centre and the exact intersection depth
    dd, od = (d * d).sum(-1), d @ o
    closest = np.sqrt(np.maximum((o @ o) - od * od / dd, 0))
    disc = od * od - dd * ((o @ o) - R * R)
    z_exact = (-od - np.sqrt(np.maximum(disc, 0))) / dd
    inner, outer = closest <= R - s, closest > R + s
    hit = out["depth"][0] > 0
    assert inner.sum() > 500 and outer.sum() > 500
    assert hit[inner].all() and not hit[outer].any(), (int((~hit[inner]).sum()), int(hit[outer].sum()))
    err = np.abs(out["depth"][0].astype(np.float64) - z_exact)[inner] / s
    p = o + z_exact[..., None] * d
    radial_cam = (p / np.linalg.norm(p, axis=-1, keepdims=True)) @ pose[:3, :3].T
    cosang = np.clip((out["normal"][0].astype(np.float64) * radial_cam).sum(-1), -1, 1)[inner]
    ang = np.rad2deg(np.arccos(cosang))
    fig = dict(depth_max_voxels=float(err.max()), depth_median_voxels=float(np.median(err)), normal_max_deg=float(ang.max()),
               pixels=int(inner.sum()))
    record("sphere", fig)
    prof = profile()["sphere"]
    print(f"sphere: {fig}; gates: depth {2 * prof['depth_max_voxels']:.4f} voxels, normal {2 * prof['normal_max_deg']:.3f} degrees")
    assert err.max() <= 2 * prof["depth_max_voxels"] and ang.max() <= 2 * prof["normal_max_deg"]
    assert (out["color"][0][hit] == 128).all() and (out["xyz"][0][..., 2] == out["depth"][0]).all()


# ------------------------------------------------------------------ 2. wrong variants, 3. branch coverage
WRONG_CASE = "plane_17_64x64_N17"


@pytest.mark.parametrize("wrong", rm.WRONG)
def test_wrong_variants_change_a_named_case(wrong):
    c = rm.named_case(WRONG_CASE)
    ref, got = rm.run_case(c), rm.run_case(c, wrong=wrong)
    differ = {k: int((~((got[k].view(np.uint32) == ref[k].view(np.uint32)) | (np.isnan(got[k]) & np.isnan(ref[k])))).sum()) for k in ref}
    print(f"{wrong} on {WRONG_CASE}: values that differ {differ}")
    assert sum(differ.values()) > 0


def test_generated_cases_reach_every_branch():
    total = {}
    for name in rm.CASES:
        c = rm.named_case(name)
        st = rm.branches_reached(c)
        for k, v in st.items():
            total[k] = total.get(k, 0) + v
    # z_far cutting a hit off: pixels that hit without the limit and miss with it
    cut = 0
    for name in ("plane_17_zfar_64x64_N1", "random_17_zfar_7x5_N17"):
        c = rm.named_case(name)
        with_far = rm.run_case(c)["depth"]
        without = rm.run_case(dict(c, z_far=None))["depth"]
        cut += int(((without > 0) & (with_far == 0)).sum())
        assert not ((with_far > 0) & (without != with_far)).any()
    total["zfar_cut"] = cut
    print(total)
    assert all(v > 0 for v in total.values()), {k: v for k, v in total.items() if not v}
    assert "plane_2_fullframe_7x5_N1_V1table" in rm.TABLE_FOR_ONE_VIEW and rm.named_case("plane_2_fullframe_7x5_N1_V1table")["bbox2d"] is None


# ------------------------------------------------------------------ 4. one view fused and raycast
def test_one_fused_view_is_seen_again_within_trunc():
    """a sphere of 3 cm, 30 cm away, as one analytic depth image; fused into a fresh volume and raycast at the view's own pose, K and
    full frame: every hit lies within trunc of the view's depth at that pixel"""
    H = W = 48
    K = np.array([[220.0, 0, 24.0], [0, 220.0, 24.0], [0, 0, 1]])
    pose = np.eye(4, dtype=f32)
    pose[2, 3] = 0.3
    o, d = _rays64(pose, K, H, W)
    dd, od = (d * d).sum(-1), d @ o
    disc = od * od - dd * ((o @ o) - 0.03 ** 2)
    depth = np.where(disc > 0, (-od - np.sqrt(np.maximum(disc, 0))) / dd, 0).astype(f32)
    mask = (depth > 0).astype(np.uint8)
    s = 0.0025
    vol = tm.Volume((33, 33, 33), np.full(3, -16 * s), s, 4 * s)
    tm.integrate(vol, depth[None], np.full((1, H, W, 3), 200, f32), mask[None], pose[None], K[None])
    out = rm.raycast(vol, pose[None], K, H, W)
    drawn = out["depth"][0] > 0
    hit = drawn & (mask != 0)          # a silhouette pixel next to the mask can hit the surface its neighbours saw: no depth to compare
    err = np.abs(out["depth"][0] - depth)[hit]
    print(f"one view: {int(hit.sum())} hits of {int(mask.sum())} masked pixels, {int((drawn & (mask == 0)).sum())} beside the mask, |raycast - depth| max {err.max() / s:.3f} median {np.median(err) / s:.3f} voxels "
          f"(trunc = 4 voxels)")
    assert hit.sum() > 0.8 * mask.sum()
    assert (err <= float(vol.trunc)).all()
    # a weighted mean of equal colours: 8 weights of two products, 8 products, 2 x 8 additions and one division round once each
    assert (np.abs(out["color"][0][hit] - 200) <= 200 * 41 * 2.0 ** -24).all()


# ------------------------------------------------------------------ 5. consistency with the extraction
HELD_OUT = 1          # the held-out pose: between reference views, perturbed


def held_out_pose(can_views):
    return im.view_perturbations(can_views["ob_in_cams"][[3]], seed=11, max_trans=0.02, rot_deg=(15.0, 25.0))


def extraction_figures(vol, scene, can_views):
    from oracle import ops as oo
    pos, col, nrm, faces = tm.extract(vol)
    mesh_np = dict(pos=pos, vnormals=nrm, faces=faces.astype(np.int32), vertex_color=col / f32(255))
    P = held_out_pose(can_views)
    diam = rm.box_diameter(vol)
    oh, ow = im.CROP
    tf, bb = oo.crop_windows(P, scene["K"], diam, im.CROP_RATIO, (ow, oh))
    mesh_depth = oo.render_crops(mesh_np, P, bb, scene["K"], scene["H"], scene["W"], (oh, ow), diam, normalize_xyz=False, want=("depth",))["depth"][0]
    ray_depth = rm.raycast(vol, P, scene["K"], scene["H"], scene["W"], (oh, ow), bb)["depth"][0]
    a, b = mesh_depth > 0, ray_depth > 0
    diff = np.abs(mesh_depth - ray_depth)[a & b].astype(np.float64) * 1e3
    return dict(both=int((a & b).sum()), only_one_frac=float((a ^ b).sum() / max((a | b).sum(), 1)), median_mm=float(np.median(diff)),
                p99_mm=float(np.percentile(diff, 99)))


def test_raycast_agrees_with_the_extracted_mesh(scene, can_views, can_model_volume):
    """the can volume from 16 oracle renders at a held-out pose, through the ICP's window: the raycast depth against the oracle's
    render of the extracted mesh -- median and p99 |difference| over the pixels both draw, and the fraction of pixels only one of them
    draws; gated at twice the figures measured here (profiles/tsdf_raycast.json "extraction": median 0.053 mm, p99 2.21 mm, 0.76 % of
    the pixels drawn by one alone, 4164 by both)"""
    fig = extraction_figures(can_model_volume, scene, can_views)
    record("extraction", fig)
    prof = profile()["extraction"]
    print(f"raycast against the extracted mesh: {fig}; measured {prof}")
    assert fig["both"] > 1000
    assert fig["median_mm"] <= 2 * prof["median_mm"] and fig["p99_mm"] <= 2 * prof["p99_mm"] and fig["only_one_frac"] <= 2 * prof["only_one_frac"]


# ------------------------------------------------------------------ 6. alignment quality, 7. sequential fusion
ALIGN_MARGIN = 1.25   # both routes align to the same blurred surface; what differs is the surface interpolant


def _pose_errors(P, gt):
    """(translation mm, tilt of the can's axis in degrees: a turn about the axis of a solid of revolution is no error of its pose, as in
    icp_model.pose_errors) of poses against the true ones, per view"""
    P, gt = np.asarray(P, np.float64), np.asarray(gt, np.float64)
    dt = np.linalg.norm(P[:, :3, 3] - gt[:, :3, 3], axis=1) * 1e3
    a = P[:, :3, 2] / np.linalg.norm(P[:, :3, 2], axis=1, keepdims=True)
    ang = np.rad2deg(np.arccos(np.clip((a * gt[:, :3, 2]).sum(1), -1, 1)))
    return dt, ang


def test_alignment_to_the_volume_is_as_good_as_to_the_mesh(scene, can_views):
    """the 16 can views with icp_model.view_perturbations, fused as given; then 3 ICP iterations of every view against the volume
    (raycast) and against the extracted mesh (icp_model.refine_views_model): the volume route's median translation and axis-tilt
    errors are at most 1.25 x the mesh route's (profiles/tsdf_raycast.json "alignment": from 3.72 mm / 0.76 degrees to 2.30 mm / 0.22
    degrees against the volume and 2.29 mm / 0.24 degrees against the mesh: ratios 1.003 and 0.926)"""
    views, spec = can_views, tm.can_volume_spec()
    origin, dims, s, trunc = spec
    P0 = im.view_perturbations(views["ob_in_cams"], seed=0)
    vol = tm.integrate(tm.Volume(dims, origin, s, trunc), views["depth"], views["rgb"], views["masks"], P0, views["Ks"])
    Pv, status, _ = rm.align_views_model(vol, views, P0, scene["H"], scene["W"])
    Pm, status_m = im.refine_views_model(tm.extract(vol), views, P0, scene["H"], scene["W"])
    e0, ev, em = _pose_errors(P0, views["ob_in_cams"]), _pose_errors(Pv, views["ob_in_cams"]), _pose_errors(Pm, views["ob_in_cams"])
    fig = dict(start_trans_mm=float(np.median(e0[0])), start_rot_deg=float(np.median(e0[1])), volume_trans_mm=float(np.median(ev[0])),
               volume_rot_deg=float(np.median(ev[1])), mesh_trans_mm=float(np.median(em[0])), mesh_rot_deg=float(np.median(em[1])))
    fig["ratio_trans"], fig["ratio_rot"] = fig["volume_trans_mm"] / fig["mesh_trans_mm"], fig["volume_rot_deg"] / fig["mesh_rot_deg"]
    record("alignment", fig)
    print(f"alignment (medians over 16 views): {fig}; status volume {status} mesh {status_m}")
    assert status == [0] * 16 and status_m == [0] * 16
    assert fig["volume_trans_mm"] < fig["start_trans_mm"] and fig["volume_rot_deg"] < fig["start_rot_deg"]
    assert fig["ratio_trans"] <= ALIGN_MARGIN and fig["ratio_rot"] <= ALIGN_MARGIN
    prof = profile()["alignment"]       # and what was measured stays measured: twice the recorded errors at the most
    assert fig["volume_trans_mm"] <= 2 * prof["volume_trans_mm"] and fig["volume_rot_deg"] <= 2 * prof["volume_rot_deg"]


def test_sequential_fusion_beats_the_poses_as_given(scene, can_views):
    """integrate_aligned on the same perturbed views with trusted=1: the extracted mesh's median distance to the analytic cylinder is
    strictly below that of fusing the perturbed poses as given (profiles/tsdf_raycast.json "sequential": 1.242 mm against 1.361 mm;
    0.240 mm with the true poses; median translation error of the poses 3.72 -> 2.41 mm)"""
    views = can_views
    origin, dims, s, trunc = tm.can_volume_spec()
    P0 = im.view_perturbations(views["ob_in_cams"], seed=0)

    def median_mm(vol):
        return float(np.median(tm.cylinder_distance(tm.extract(vol)[0], tm.CAN_RADIUS, tm.CAN_HEIGHT)) * 1e3)

    fuse = lambda P: tm.integrate(tm.Volume(dims, origin, s, trunc), views["depth"], views["rgb"], views["masks"], P, views["Ks"])   # noqa: E731
    seq = tm.Volume(dims, origin, s, trunc)
    used = rm.integrate_aligned_model(seq, views, P0, scene["H"], scene["W"], trusted=1)
    e0, e1 = _pose_errors(P0, views["ob_in_cams"]), _pose_errors(used, views["ob_in_cams"])
    fig = dict(as_given_median_mm=median_mm(fuse(P0)), aligned_median_mm=median_mm(seq), true_median_mm=median_mm(fuse(views["ob_in_cams"])),
               as_given_trans_mm=float(np.median(e0[0])), aligned_trans_mm=float(np.median(e1[0])))
    record("sequential", fig)
    print(f"sequential fusion: {fig}")
    kept = [v for v in range(16) if np.array_equal(used[v], P0[v])]
    print(f"views that kept their poses (the trusted one, and those left out of the volume): {kept}")
    assert kept[0] == 0 and len(kept) < 8
    assert fig["aligned_median_mm"] < fig["as_given_median_mm"]
    assert fig["aligned_median_mm"] <= 2 * profile()["sequential"]["aligned_median_mm"]


# ------------------------------------------------------------------ 8. refusals and C errors
def _cpu_volume(dims=(4, 5, 6)):
    return [torch.ones(dims), torch.zeros(dims), torch.zeros(dims + (3,)), torch.zeros(dims)]


def test_wrappers_refuse_before_any_device_call():
    from foundationpose_amd import _lib, ops
    from foundationpose_amd.reconstruct import TsdfVolume, align_views_to_volume, reconstruct_object
    E = _lib.FpAmdError
    vol, K = _cpu_volume(), np.array([[50.0, 0, 4], [0, 50, 4], [0, 0, 1]])

    def call(vol=vol, origin=(0, 0, 0), voxel=0.01, poses=torch.eye(4).repeat(2, 1, 1), K=K, H=8, W=9, **kw):
        return ops.tsdf_raycast(*vol, origin, voxel, poses, K, H, W, **kw)

    with pytest.raises(E, match="poses must be"):
        call(poses=torch.eye(4))
    with pytest.raises(E, match="poses must be a tensor"):
        call(poses=np.eye(4)[None])
    with pytest.raises(E, match="weight must be"):
        call(vol=[vol[0], torch.zeros(4, 5, 5), vol[2], vol[3]])
    with pytest.raises(E, match="out_hw must be"):
        call(out_hw=(4, 4))
    with pytest.raises(E, match="out_hw is required"):
        call(bbox2d=torch.zeros(2, 4))
    with pytest.raises(E, match="bbox2d must be"):
        call(bbox2d=torch.zeros(3, 4), out_hw=(4, 4))
    with pytest.raises(E, match="2\\^20"):
        call(bbox2d=torch.zeros(2, 4), out_hw=(2048, 1024))
    with pytest.raises(ValueError, match="want"):
        call(want=("depth", "mask"))
    with pytest.raises(ValueError, match="want"):
        call(want=())
    with pytest.raises(ValueError, match="skew"):
        call(K=np.array([[50.0, 0.1, 4], [0, 50, 4], [0, 0, 1]]))
    with pytest.raises(E, match="views must be"):
        call(views=[K])
    with pytest.raises(ValueError, match="not in want"):
        call(want=("depth",), out=dict(xyz=torch.zeros(2, 8, 9, 3)))
    with pytest.raises(E, match=r"out\['depth'\] must be"):
        call(want=("depth",), out=dict(depth=torch.zeros(2, 8, 8)))
    for bad in (dict(voxel=0.0), dict(step=0.0), dict(step=float("nan")), dict(step=-1.0), dict(step=1e-9), dict(z_near=-0.1),
                dict(z_near=float("nan")), dict(z_far=float("inf")), dict(z_near=0.5, z_far=0.4), dict(min_weight=float("nan")),
                dict(origin=(0, float("inf"), 0))):
        with pytest.raises(ValueError):
            call(**bad)
    # values are refused before the device is looked at, and CPU tensors last of all
    with pytest.raises(E, match="CUDA"):
        call()
    with pytest.raises(E, match="CUDA"):
        call(bbox2d=torch.zeros(2, 4), out_hw=(4, 4), want=("xyz", "normal"))
    z = torch.zeros
    with pytest.raises(ValueError, match="refine_against"):
        reconstruct_object(z(1, 2, 2, 3), z(1, 2, 2), z(1, 2, 2), z(1, 4, 4), np.eye(3), refine_against="x")
    assert inspect.signature(reconstruct_object).parameters["refine_against"].default == "mesh"
    tv = TsdfVolume((0, 0, 0), (4, 4, 4), 0.01, device="cpu")
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="iterations"):
            align_views_to_volume(tv, z(1, 2, 2), z(1, 2, 2), z(1, 4, 4), np.eye(3), iterations=bad)
        with pytest.raises(ValueError, match="iterations"):
            tv.integrate_aligned(z(1, 2, 2, 3), z(1, 2, 2), z(1, 2, 2), z(1, 4, 4), np.eye(3), iterations=bad)
    with pytest.raises(ValueError, match="max_dist"):
        align_views_to_volume(tv, z(1, 2, 2), z(1, 2, 2), z(1, 4, 4), np.eye(3), max_dist=-1.0)
    with pytest.raises(ValueError, match="masks are required"):
        align_views_to_volume(tv, z(1, 2, 2), None, z(1, 4, 4), np.eye(3))
    with pytest.raises(ValueError, match="must be a TsdfVolume"):
        align_views_to_volume({}, z(1, 2, 2), z(1, 2, 2), z(1, 4, 4), np.eye(3))
    with pytest.raises(ValueError, match="trusted"):
        tv.integrate_aligned(z(1, 2, 2, 3), z(1, 2, 2), z(1, 2, 2), z(1, 4, 4), np.eye(3), trusted=-1)
    with pytest.raises(ValueError, match="masks are required"):
        tv.depth_agreement(z(1, 2, 2), None, z(1, 4, 4), np.eye(3))
    with pytest.raises(ValueError, match="tolerance"):
        tv.depth_agreement(z(1, 2, 2), z(1, 2, 2), z(1, 4, 4), np.eye(3), tol=-1.0)


def test_c_entry_point_reports_argument_errors_without_a_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    p, o = C.c_void_p(16), (C.c_float * 3)(0, 0, 0)
    bad_o = (C.c_float * 3)(0, float("inf"), 0)
    K = (C.c_float * 9)(50, 0, 4, 0, 50, 4, 0, 0, 1)
    skew = (C.c_float * 9)(50, 0.5, 4, 0, 50, 4, 0, 0, 1)

    def call(tsdf=p, nz=4, ny=4, nx=4, origin=o, voxel=0.01, mw=1.0, poses=p, K=K, Ks=None, view=None, V=0, bbox=p, H=8, W=8, N=2, oh=4, ow=4,
             step=0.01, zn=0.001, zf=1.0, depth=p, xyz=None, normal=None, color=None):
        return lib.fp_tsdf_raycast(tsdf, p, p, p, nz, ny, nx, origin, voxel, mw, poses, K, Ks, view, V, bbox, H, W, N, oh, ow, step, zn, zf, depth,
                                   xyz, normal, color, None)

    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(tsdf=None), b"NULL volume"), (dict(origin=None), b"NULL origin"), (dict(origin=bad_o), b"not finite"),
                     (dict(depth=None), b"every output is NULL"), (dict(poses=None), b"NULL poses"), (dict(nx=0), b"dimension"),
                     (dict(nz=5000), b"dimension"), (dict(nz=2048, ny=2048, nx=2048), b"2^30"), (dict(voxel=0.0), b"voxel"),
                     (dict(voxel=nan), b"voxel"), (dict(step=0.0), b"step"), (dict(step=inf), b"step"), (dict(step=nan), b"step"),
                     (dict(step=1e-9), b"samples"), (dict(zn=-0.1), b"z_near"), (dict(zn=nan), b"z_near"), (dict(zf=0.0005), b"z_far"),
                     (dict(zf=inf), b"z_far"), (dict(mw=nan), b"min_weight"), (dict(N=-1), b"N=-1"), (dict(N=65536), b"N=65536"),
                     (dict(oh=0), b"sizes"), (dict(W=0), b"sizes"), (dict(oh=2048, ow=1024), b"2^20"), (dict(bbox=None), b"without bbox2d"),
                     (dict(K=skew), b"skew"), (dict(K=None), b"exactly one"), (dict(Ks=p), b"exactly one"), (dict(view=p), b"view index needs"),
                     (dict(K=None, Ks=p, V=3), b"view is NULL"), (dict(K=None, Ks=p, V=0), b"V=0")):
        assert call(**kw) == -1, kw
        msg = lib.fp_last_error()
        assert msg.startswith(b"fp_tsdf_raycast") and word in msg, (kw, msg)
    # N == 0 does nothing, whatever poses is; a full-frame call is accepted with oh x ow = H x W
    assert call(N=0, poses=None) == 0 and call(N=0, bbox=None, oh=8, ow=8) == 0 and call(N=0, K=None, Ks=p, view=p, V=3) == 0
    assert call(N=0, depth=None, color=p) == 0 and call(N=0, nz=1) == 0
