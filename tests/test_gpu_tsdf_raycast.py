"""GPU: fp_tsdf_raycast and what is built on it (ops.tsdf_raycast, TsdfVolume.raycast / depth_agreement / integrate_aligned,
reconstruct.align_views_to_volume, reconstruct_object(refine_against="volume"), scripts/run_demo.py --ref_refine_against) from the kernel
to the script.  The kernel is held to the numpy restatement (tests/tsdf_raycast_model.py) bit for bit, NaN equal to NaN, on the
generated cases whose branch coverage tests/test_tsdf_raycast_host.py asserts; every other gate is a figure measured on the CPU from the
restatement (profiles/tsdf_raycast.json), none was chosen by looking at the device's output."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import icp_model as im
import tsdf_model as tm
import tsdf_raycast_model as rm
from conftest import ROOT
from test_gpu_icp import _arena, _cylinder
from test_gpu_multi_object import _t, dev  # noqa: F401
from test_gpu_tsdf import _noisy_reference_views

pytestmark = pytest.mark.gpu
f32 = np.float32
ALL = ("depth", "xyz", "normal", "color")


def profile():
    return json.load(open(os.path.join(ROOT, "profiles", "tsdf_raycast.json")))


def _device_volume(vol, dev):
    d = vol.dims
    return [_t(vol.tsdf.reshape(d), dev), _t(vol.weight.reshape(d), dev), _t(vol.color.reshape(d + (3,)), dev), _t(vol.color_weight.reshape(d), dev)]


def _model_volume(tv):
    """a TsdfVolume's device arrays as the restatement's Volume"""
    vol = tm.Volume(tv.dims, tv.origin, tv.voxel, tv.trunc)
    vol.tsdf, vol.weight = tv.tsdf.cpu().numpy().reshape(-1), tv.weight.cpu().numpy().reshape(-1)
    vol.color, vol.color_weight = tv.color.cpu().numpy().reshape(-1, 3), tv.color_weight.cpu().numpy().reshape(-1)
    return vol


def _run(c, dev, rows=None, want=ALL, arenas=False, table=False, arrays=None):
    """the op on a generated case (or on its rows `rows`) -> dict of numpy outputs"""
    from foundationpose_amd import ops
    rows = np.arange(len(c["poses"])) if rows is None else np.asarray(rows)
    n, (oh, ow) = len(rows), c["out_hw"]
    views = None
    if c["V"] > 1:
        views = ops.Views(list(c["K"]), np.zeros(n, np.int64), dev)
        views.dev = _t(c["view"][rows].astype(np.int32), dev)               # the raw index: values outside 0..V-1 included
    elif table:
        views = ops.Views([c["K"]], None, dev)
    out, checks = None, []
    if arenas:
        out = {}
        for name in want:
            out[name], chk = _arena((n, oh, ow) + ((3,) if name != "depth" else ()), torch.float32, dev)
            checks.append(chk)
    vol = c["vol"]
    arrays = _device_volume(vol, dev) if arrays is None else arrays
    bb = None if c["bbox2d"] is None else _t(c["bbox2d"][rows], dev)
    r = ops.tsdf_raycast(*arrays, vol.origin, float(vol.voxel), _t(c["poses"][rows], dev), None if views is not None else c["K"], c["H"], c["W"],
                         (oh, ow), bb, float(c["step"]), c["min_weight"], c["z_near"], c["z_far"], want, out=out, views=views)
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    assert set(r) == set(want)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _assert_bits(got, ref, what, rows=None):
    for k in got:
        want = ref[k] if rows is None else ref[k][rows]
        a, b = np.asarray(got[k], f32), np.asarray(want, f32)
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        differ = ~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))
        if differ.any():
            at = tuple(np.argwhere(differ)[0])
            raise AssertionError(f"{what}: {k}: {int(differ.sum())} of {differ.size} values differ in bits, the first at {at}: {a[at]!r} against {b[at]!r}")


# ------------------------------------------------------------------ 1. bit-equality on the generated cases, 2. poisoned arenas
@pytest.mark.parametrize("name", list(rm.CASES))
def test_generated_cases_equal_the_restatement(dev, name):
    c = rm.named_case(name)
    st = {}
    ref = rm.run_case(c, stats=st)
    got = _run(c, dev, arenas=True, table=name in rm.TABLE_FOR_ONE_VIEW)
    print(name, {k: v for k, v in st.items() if v})
    _assert_bits(got, ref, name)


SUBSETS = [w for k in range(1, 5) for w in itertools.combinations(ALL, k)]      # all 15: the outputs left out are passed as NULL


@pytest.mark.parametrize("want", SUBSETS, ids=["+".join(w) for w in SUBSETS])
def test_want_subsets_write_their_outputs_only(dev, want):
    c = rm.named_case("plane_17_7x5_N17_V3")
    ref = rm.run_case(c)
    got = _run(c, dev, want=want, arenas=True)
    _assert_bits(got, ref, f"want={want}")


# ------------------------------------------------------------------ 3. determinism
def test_rows_alone_reversed_repeated_and_replayed(dev):
    from foundationpose_amd import ops
    c = rm.named_case("random_33x20x9_9x64_N17_V3")
    N = len(c["poses"])
    ref = rm.run_case(c)
    arrays = _device_volume(c["vol"], dev)
    first = _run(c, dev, arrays=arrays)
    _assert_bits(first, ref, "batch")
    _assert_bits(_run(c, dev, arrays=arrays), first, "second call")
    rev = _run(c, dev, rows=np.arange(N)[::-1], arrays=arrays)
    _assert_bits({k: v[::-1] for k, v in rev.items()}, first, "reversed batch")
    for n in (0, 1, 5, N - 1):
        _assert_bits(_run(c, dev, rows=[n], arrays=arrays), first, f"row {n} alone", rows=[n])
    # a captured graph, replayed twice into poisoned buffers
    oh, ow = c["out_hw"]
    views = ops.Views(list(c["K"]), np.zeros(N, np.int64), dev)
    views.dev = _t(c["view"].astype(np.int32), dev)
    out = dict(depth=torch.empty((N, oh, ow), device=dev), xyz=torch.empty((N, oh, ow, 3), device=dev),
               normal=torch.empty((N, oh, ow, 3), device=dev), color=torch.empty((N, oh, ow, 3), device=dev))
    P, bb, vol = _t(c["poses"], dev), _t(c["bbox2d"], dev), c["vol"]

    def call():
        return ops.tsdf_raycast(*arrays, vol.origin, float(vol.voxel), P, None, c["H"], c["W"], (oh, ow), bb, float(c["step"]), c["min_weight"],
                                c["z_near"], c["z_far"], ALL, out=out, views=views)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.inference_mode():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        for _ in range(2):
            for t in out.values():
                t.fill_(-7.25)
            graph.replay()
            torch.cuda.synchronize()
            _assert_bits({k: v.cpu().numpy() for k, v in out.items()}, first, "replayed graph")


# ------------------------------------------------------------------ 4. TsdfVolume.raycast on the can, 7. depth_agreement
@pytest.fixture(scope="module")
def can(scene, dev):
    """16 noisy device renders of the can and the volume fused from them on the device at 2.5 mm"""
    from foundationpose_amd.reconstruct import TsdfVolume
    v = _noisy_reference_views(scene, dev)
    origin, dims, s, trunc = tm.can_volume_spec()
    vol = TsdfVolume(origin, dims, float(s), float(trunc), device=dev)
    vol.integrate(v["rgb"], v["depth"], v["masks"], v["ob_in_cams"], v["Ks"])
    return v, vol


def test_volume_raycast_on_the_can_equals_the_restatement(scene, dev, can):
    from foundationpose_amd import ops
    v, vol = can
    poses = im.view_perturbations(v["ob_in_cams"][[0, 5, 11]], seed=3)
    P = _t(poses, dev)
    diam = 2.0 * float(np.linalg.norm(np.maximum(np.abs(vol.origin), np.abs(vol.origin + (np.asarray(vol.dims[::-1]) - 1) * vol.voxel))))
    tf, bb = ops.crop_windows(P, scene["K"], diam, 1.2, (64, 64))
    got = vol.raycast(P, scene["K"], (64, 64), bbox2d=bb)
    assert set(got) == set(ALL) and got["depth"].shape == (3, 64, 64) and got["normal"].shape == (3, 64, 64, 3)
    st = {}
    ref = rm.raycast(_model_volume(vol), poses, scene["K"], scene["H"], scene["W"], (64, 64), bb.cpu().numpy(), stats=st)
    print("can, 3 poses at 64 x 64:", {k: n for k, n in st.items() if n})
    assert st["hit"] > 1000
    _assert_bits({k: t.cpu().numpy() for k, t in got.items()}, ref, "TsdfVolume.raycast")
    # full frame, one pose, depth alone: the frame-sized launch
    full = vol.raycast(P[:1], scene["K"], (scene["H"], scene["W"]), want=("depth",))
    ref = rm.raycast(_model_volume(vol), poses[:1], scene["K"], scene["H"], scene["W"])
    _assert_bits({"depth": full["depth"].cpu().numpy()}, {"depth": ref["depth"]}, "full frame")


def test_depth_agreement_of_the_volume_with_its_views(scene, dev, can):
    from foundationpose_amd import ops
    v, vol = can
    V, H, W = v["depth"].shape
    table = vol.depth_agreement(v["depth"], v["masks"], v["ob_in_cams"], v["Ks"])
    vt = ops.Views(list(v["Ks"]), np.arange(V), dev)
    d, m = _t(v["depth"].astype(f32), dev), _t(v["masks"], dev)
    xyz = ops.depth_to_xyz_frames(torch.where(m != 0, d, torch.zeros_like(d)).contiguous(), vt)
    depth = vol.raycast(_t(v["ob_in_cams"].astype(f32), dev), vt, (H, W), want=("depth",))["depth"]
    tf = _t(np.tile(np.asarray([[W / (W - 1.0), 0, -0.5], [0, H / (H - 1.0), -0.5], [0, 0, 1]], f32), (V, 1, 1)), dev)
    by_hand = ops.depth_agreement(depth, xyz, tf, 2.0 * vol.voxel, views=vt)
    rows = ops.DepthAgreement.rows(table)
    print("volume against its own views:", [(r.model, r.valid, r.agree, r.behind) for r in rows[:4]])
    assert table.dtype == torch.int32 and tuple(table.shape) == (V, 4) and torch.equal(table, by_hand)
    # the window that is the frame reads texel (i, j) for crop pixel (i, j): `valid` counts the raycast pixels with a masked depth
    valid = ((depth > 0) & (m != 0) & (d >= 0.001)).sum(dim=(1, 2)).cpu().numpy()
    assert np.array_equal(valid, [r.valid for r in rows]) and all(r.model > 0 and r.agree > 0 for r in rows)
    wide = ops.DepthAgreement.rows(vol.depth_agreement(v["depth"], v["masks"], v["ob_in_cams"], v["Ks"], tol=0.05))
    assert all(a.agree >= b.agree and a.model == b.model for a, b in zip(wide, rows))


# ------------------------------------------------------------------ 5. rasteriser versus raycast, through the ICP
def _errors(P, gt):
    """(median translation error mm, median tilt of the can's axis in degrees) over the views"""
    P = P.cpu().numpy() if torch.is_tensor(P) else np.asarray(P)
    P, gt = P.astype(np.float64), np.asarray(gt, np.float64)
    dt = np.linalg.norm(P[:, :3, 3] - gt[:, :3, 3], axis=1) * 1e3
    a = P[:, :3, 2] / np.linalg.norm(P[:, :3, 2], axis=1, keepdims=True)
    return float(np.median(dt)), float(np.median(np.rad2deg(np.arccos(np.clip((a * gt[:, :3, 2]).sum(1), -1, 1)))))


MARGIN = 1.25      # the margin of the CPU test of the alignment (tests/test_tsdf_raycast_host.py: ALIGN_MARGIN)


def test_one_icp_step_from_the_raycast_and_from_the_rasteriser(scene, dev, can):
    """the can volume's extracted mesh rendered and the volume raycast at the same perturbed poses through the same windows, each fed
    to one ICP step against the views' depth: the pair counts differ by no more than the fraction of pixels only one of the two draws,
    as measured by the CPU test of the two depths (profiles/tsdf_raycast.json "extraction": only_one_frac), and the step from the raycast leaves pose errors within the CPU test's
    margin of those the step from the render leaves"""
    from foundationpose_amd import ops
    from foundationpose_amd.reconstruct import ICP_CROP, ICP_CROP_RATIO, _AlignSide
    from foundationpose_amd.Utils import get_mesh_handle
    v, vol = can
    V, H, W = v["depth"].shape
    _, t = vol.extract()
    P = _t(im.view_perturbations(v["ob_in_cams"], seed=0), dev)
    side = _AlignSide(vol, _t(v["depth"].astype(f32), dev), _t(v["masks"], dev), v["Ks"])
    oh, ow = ICP_CROP
    tf, bb = ops.crop_windows(P, None, side.diam, ICP_CROP_RATIO, (ow, oh), views=side.vt)
    mesh = ops.render_crops(ops.MeshSet([get_mesh_handle(t)]), P, bb, None, H, W, (oh, ow), side.diam, normalize_xyz=False, want=("xyz", "normal"),
                            views=side.vt)
    ray = vol.raycast(P, side.vt, (oh, ow), bbox2d=bb, want=("xyz", "normal"))
    Pm, sm = ops.icp_point_plane(mesh["xyz"], mesh["normal"], side.xyz, tf, P, 0.01, views=side.vt)
    Pr, sr = ops.icp_point_plane(ray["xyz"], ray["normal"], side.xyz, tf, P, 0.01, views=side.vt)
    a, b = ops.IcpStep.rows(sm), ops.IcpStep.rows(sr)
    rel = max(abs(x.pairs - y.pairs) / max(x.pairs, y.pairs) for x, y in zip(a, b))
    em, er, e0 = _errors(Pm, v["ob_in_cams"]), _errors(Pr, v["ob_in_cams"]), _errors(P, v["ob_in_cams"])
    gate = profile()["extraction"]["only_one_frac"]
    print(f"pairs render {[x.pairs for x in a][:4]} raycast {[y.pairs for y in b][:4]}: largest relative difference {rel:.5f} (gate {gate:.5f}); "
          f"errors (mm, degrees) before {e0}, after the render's step {em}, after the raycast's {er}")
    assert all(x.status == 0 for x in a + b)
    assert rel <= gate
    assert er[0] <= MARGIN * em[0] and er[1] <= MARGIN * em[1]


# ------------------------------------------------------------------ 6. the device paths inside the gates of the CPU tests
def test_views_are_aligned_to_the_volume(scene, dev, can):
    """align_views_to_volume against refine_view_poses on the volume fused from the perturbed poses: errors within the CPU test's margin
    of the mesh route's, and below the start's"""
    from foundationpose_amd.reconstruct import TsdfVolume, align_views_to_volume, refine_view_poses
    v, true_vol = can
    P0 = im.view_perturbations(v["ob_in_cams"], seed=0)
    vol = TsdfVolume(true_vol.origin, true_vol.dims, true_vol.voxel, true_vol.trunc, device=dev)
    vol.integrate(v["rgb"], v["depth"], v["masks"], P0, v["Ks"])
    Pv, steps = align_views_to_volume(vol, v["depth"], v["masks"], P0, v["Ks"])
    Pm, steps_m = refine_view_poses(vol.extract()[1], v["depth"], v["masks"], P0, v["Ks"])
    e0, ev, em = _errors(P0, v["ob_in_cams"]), _errors(Pv, v["ob_in_cams"]), _errors(Pm, v["ob_in_cams"])
    print(f"errors (mm, degrees): start {e0}, aligned to the volume {ev}, to the mesh {em}; pairs {[s.pairs for s in steps][:4]}")
    assert tuple(Pv.shape) == (16, 4, 4) and Pv.dtype == torch.float32 and all(s.status == 0 for s in steps + steps_m)
    assert ev[0] < e0[0] and ev[0] <= MARGIN * em[0] and ev[1] <= MARGIN * em[1]


def test_reconstruct_object_refines_against_the_volume(scene, dev, can):
    """refine_against="volume": refined poses within the margin of the mesh route's, and a mesh closer to the cylinder than the fuse of
    the poses as given; refine_against="mesh" is the call without the argument, bit for bit"""
    from foundationpose_amd.reconstruct import reconstruct_object
    v, _ = can
    P0 = im.view_perturbations(v["ob_in_cams"], seed=0)
    args, kw = (v["rgb"], v["depth"], v["masks"], P0, v["Ks"]), dict(voxel=tm.CAN_VOXEL, device=dev)
    plain, _ = reconstruct_object(*args, **kw)
    by_mesh, mt = reconstruct_object(*args, refine_poses=2, **kw)
    named, nt = reconstruct_object(*args, refine_poses=2, refine_against="mesh", **kw)
    assert np.array_equal(by_mesh.vertices, named.vertices) and np.array_equal(by_mesh.faces, named.faces)
    assert np.array_equal(by_mesh.ob_in_cams, named.ob_in_cams) and torch.equal(mt["pos"], nt["pos"]) and torch.equal(mt["vertex_color"], nt["vertex_color"])
    by_vol, _ = reconstruct_object(*args, refine_poses=2, refine_against="volume", **kw)
    a, m, b = _cylinder(plain.vertices), _cylinder(by_mesh.vertices), _cylinder(by_vol.vertices)
    em, ev = _errors(by_mesh.ob_in_cams, v["ob_in_cams"]), _errors(by_vol.ob_in_cams, v["ob_in_cams"])
    print(f"distance to the cylinder (median, p99, max) mm: as given {a}, refined against the mesh {m}, against the volume {b}; pose errors (mm, "
          f"degrees) mesh route {em}, volume route {ev}")
    assert by_vol.ob_in_cams.shape == (16, 4, 4) and by_vol.ob_in_cams.dtype == np.float32
    assert b[0] < a[0]
    assert ev[0] <= MARGIN * em[0] and ev[1] <= MARGIN * em[1]


def test_integrate_aligned(scene, dev, can):
    """sequential fusion of the perturbed views (trusted=1): a mesh closer to the cylinder than the fuse of the poses as given; views
    that cannot be aligned keep their poses and stay out of the volume, which then holds the bits of integrate over the trusted views
    alone -- with an empty mask (no pairs; fused, such a view would carve the volume empty along all its rays: the fusion counts a
    pixel outside the mask as an observation of free space) and with a mask of 6 x 6 pixels on the can (36 pairs at most, fewer than
    min_pairs = 64; fused, it would also add its surface)"""
    from foundationpose_amd.reconstruct import TsdfVolume
    v, true_vol = can
    P0 = im.view_perturbations(v["ob_in_cams"], seed=0)
    fresh = lambda: TsdfVolume(true_vol.origin, true_vol.dims, true_vol.voxel, true_vol.trunc, device=dev)   # noqa: E731
    given = fresh()
    given.integrate(v["rgb"], v["depth"], v["masks"], P0, v["Ks"])
    seq = fresh()
    used = seq.integrate_aligned(v["rgb"], v["depth"], v["masks"], P0, v["Ks"], trusted=1)
    a, b = _cylinder(given.extract()[0].vertices), _cylinder(seq.extract()[0].vertices)
    e0, e1 = _errors(P0, v["ob_in_cams"]), _errors(used, v["ob_in_cams"])
    print(f"distance to the cylinder (median, p99, max) mm: as given {a}, aligned one after the other {b}; pose errors (mm, degrees) {e0} -> {e1}")
    assert tuple(used.shape) == (16, 4, 4) and used.dtype == torch.float32 and used.is_cuda
    assert np.array_equal(used[0].cpu().numpy(), P0[0]) and b[0] < a[0]
    # left_out names the views that kept their poses (they saw too little of what was fused before them); the others moved.  The views
    # are spread evenly over a sphere, so most of them overlap what their predecessors fused: fewer than half may be left out
    out = seq.left_out.cpu().numpy()
    same = (used.cpu().numpy().view(np.uint32) == P0.view(np.uint32)).all(axis=(1, 2))
    print(f"left out of the volume: views {np.nonzero(out)[0].tolist()}")
    assert seq.left_out.dtype == torch.bool and out.shape == (16,) and not out[0] and np.array_equal(same[1:], out[1:]) and out.sum() < 8
    # later views without a single masked pixel: every step has status 1
    masks = v["masks"].copy()
    masks[2:] = 0
    part, two = fresh(), fresh()
    used = part.integrate_aligned(v["rgb"], v["depth"], masks, P0, v["Ks"], iterations=2, trusted=2)
    two.integrate(v["rgb"][:2], v["depth"][:2], masks[:2], P0[:2], v["Ks"][:2])
    assert np.array_equal(used.cpu().numpy().view(np.uint32), P0.view(np.uint32))
    assert part.left_out.cpu().numpy().tolist() == [False] * 2 + [True] * 14
    for x, y in zip(part.arrays(), two.arrays()):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # fusing such a view as given would change the volume: the skip is what the equality above shows
    carved = fresh()
    carved.integrate(v["rgb"][:3], v["depth"][:3], masks[:3], P0[:3], v["Ks"][:3])
    assert not torch.equal(carved.weight, two.weight)
    # a later view with a mask too small for a step: 6 x 6 pixels in the middle of the can's own mask
    small = v["masks"].copy()
    small[2:] = 0
    for k in range(2, 5):
        ys, xs = np.nonzero(v["masks"][k])
        cy, cx = int(np.median(ys)), int(np.median(xs))
        small[k, cy - 3:cy + 3, cx - 3:cx + 3] = v["masks"][k, cy - 3:cy + 3, cx - 3:cx + 3]
        assert small[k].sum() > 0
    few, fused = fresh(), fresh()
    used = few.integrate_aligned(v["rgb"][:5], v["depth"][:5], small[:5], P0[:5], v["Ks"][:5], iterations=2, trusted=2)
    assert few.left_out.cpu().numpy().tolist() == [False, False, True, True, True]
    assert np.array_equal(used.cpu().numpy().view(np.uint32), P0[:5].view(np.uint32))
    for x, y in zip(few.arrays(), two.arrays()):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    fused.integrate(v["rgb"][:5], v["depth"][:5], small[:5], P0[:5], v["Ks"][:5])
    assert not torch.equal(fused.tsdf, two.tsdf)


# ------------------------------------------------------------------ 8. the script
def test_run_demo_refines_reference_poses_against_the_volume(tmp_path, dev):
    """the script in a child process, as a user starts it: it ends with the poses of both frames and the mesh it fused"""
    from foundationpose_amd.mesh_io import load_ply
    ply, out = str(tmp_path / "can.ply"), tmp_path / "d"
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "run_demo.py"), "--synthetic_ref_views", "16", "--ref_refine_poses", "1",
           "--ref_refine_against", "volume", "--synthetic", "2", "--standin_weights", "--save_mesh", ply, "--debug_dir", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    poses = sorted((out / "ob_in_cam").glob("*.txt"))
    assert len(poses) == 2
    for f in poses:
        pose = np.loadtxt(f)
        assert pose.shape == (4, 4) and np.isfinite(pose).all() and pose[2, 3] > 0
    mesh = load_ply(ply)
    d = tm.cylinder_distance(mesh.vertices, tm.CAN_RADIUS, tm.CAN_HEIGHT)
    print(f"run_demo --ref_refine_against volume: {len(mesh.vertices)} vertices, median {np.median(d) * 1e3:.2f} mm from the cylinder")
    assert len(mesh.faces) > 10000
