"""GPU: fp_mesh_ray_cast against the numpy restatement of its definition (tests/mesh_ray_model.py) on every generated case
(tests/mesh_ray_cases.py): t, bary and hit bit-equal, face equal, no tolerance; what it may write; the same bits alone, in another
order, on another stream, from a replayed graph and in a batch of more than 2048 ray tiles; and the layers above it against their
numpy stand-ins: ops.mesh_visibility, reconstruct.view_coverage, compare_meshes(seen_from=), FoundationPose.view_coverage (on the
can fused from 16 noisy device renders too, the setting of tests/test_gpu_tsdf.py) and scripts/run_demo.py --ref_coverage."""
import itertools
import json

import numpy as np
import pytest
import torch

import mesh_distance_model as mm
import mesh_ray_cases as rc
import mesh_ray_model as rm
import tsdf_model as tm
from test_gpu_multi_object import dev  # noqa: F401
from test_gpu_tsdf import Arena, _noisy_reference_views
from test_mesh_ray_host import CYL_SAMPLES, cylinder_coverage, squares_visibility

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = rc.all_cases()
NAMES = ("t", "face", "bary", "hit")
CULL = {0: "none", 1: "back", 2: "front"}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype.kind == "i" else a.view(np.uint32)


def _assert_equal(got, ref, what):
    """got: the wrapper's dict (any subset of the outputs); ref: the restatement's (t, face, bary, hit)"""
    for k, r in zip(NAMES, ref):
        if k in got:
            g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
            assert g.shape == r.shape and g.dtype == r.dtype, (what, k, g.shape, r.shape, g.dtype, r.dtype)
            bad = np.argwhere(_bits(g) != _bits(r))
            assert len(bad) == 0, (what, k, len(bad), "mismatches, first at", bad[0], g[tuple(bad[0])], r[tuple(bad[0])])


def _up(dev, c):
    return tuple(torch.as_tensor(c[k], device=dev) for k in ("origins", "dirs", "pos", "faces"))


def _cast(c, o, d, pos, faces, **kw):
    from foundationpose_amd import ops
    return ops.mesh_ray_cast(o, d, pos=pos, faces=faces, t_min=c["t_min"], t_max=c["t_max"], cull=CULL[c["cull"]], **kw)


# ------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["name"].replace(" ", "_") for c in CASES])
def test_every_generated_case_equals_the_restatement(dev, ci):
    c = CASES[ci]
    got = _cast(c, *_up(dev, c))
    assert sorted(got) == sorted(NAMES)
    _assert_equal(got, rc.references()[c["name"]], c["name"])


def test_many_ray_tiles_cut_the_faces_into_longer_chunks(dev):
    """2048 ray tiles and more leave one chunk of all the faces to a workgroup (5 tiles of 256 here, the last one partial): the call
    on all 2048 * 256 + 77 rays has the bits of the calls on slices of it, which scan chunks of 1024 faces, and a seeded subset
    equals the restatement"""
    c = rc.soup(1100, 2048 * 256 + 77, 991)
    o, d, pos, faces = _up(dev, c)
    whole = _cast(c, o, d, pos, faces)
    n = len(c["origins"])
    for lo, hi in ((0, 1000), (300_000, 300_257), (n - 65, n)):
        part = _cast(c, o[lo:hi].contiguous(), d[lo:hi].contiguous(), pos, faces)
        for k in whole:
            assert np.array_equal(_bits(part[k].cpu().numpy()), _bits(whole[k][lo:hi].cpu().numpy())), (k, lo)
    pick = np.random.default_rng(5).choice(n, 400, replace=False)
    ref = rm.mesh_ray_cast(c["pos"], c["faces"], c["origins"][pick], c["dirs"][pick])
    assert (ref[1] >= 0).sum() > 100
    _assert_equal({k: v[torch.as_tensor(pick, device=dev)] for k, v in whole.items()}, ref, "subset of the large batch")


# ------------------------------------------------------------------ 2. what it writes
def test_writes_nothing_outside_its_outputs_and_workspace_for_every_subset(dev):
    """poisoned arenas around t, face, bary, hit and the workspace (through the C ABI, where the workspace is the caller's), for every
    subset of the optional outputs; R = 0 and F = 0"""
    from foundationpose_amd import _lib, ops
    lib = _lib.lib()
    c = next(c for c in CASES if c["name"].startswith("soup F=1025 R=65"))
    o, d, pos, faces = _up(dev, c)
    ref = rc.references()[c["name"]]
    R, F, Nv = len(c["origins"]), len(c["faces"]), len(c["pos"])
    inf = float("inf")

    def call(F_, R_, t, fc, ba, hi, ws, faces_=faces):
        return lib.fp_mesh_ray_cast(ops._ptr(pos), Nv, ops._ptr(faces_), F_, ops._ptr(o), ops._ptr(d), R_, 0.0, inf, 0, ops._ptr(t),
                                    ops._ptr(fc), ops._ptr(ba), ops._ptr(hi), ops._ptr(ws), R * 8, ops._stream(o))

    for want in itertools.product((False, True), repeat=3):
        arena = Arena(dev)
        t = arena.new((R,), torch.float32)
        fc = arena.new((R,), torch.int32) if want[0] else None
        ba = arena.new((R, 2), torch.float32) if want[1] else None
        hi = arena.new((R, 3), torch.float32) if want[2] else None
        ws = arena.new((R,), torch.int64)
        assert call(F, R, t, fc, ba, hi, ws) == 0, lib.fp_last_error()
        torch.cuda.synchronize()
        arena.check()
        got = {k: v for k, v in (("t", t), ("face", fc), ("bary", ba), ("hit", hi)) if v is not None}
        _assert_equal(got, ref, f"outputs {sorted(got)}")
        # the wrapper's subsets: t is always there
        names = tuple(n for n, w in zip(NAMES[1:], want) if w) or ("t",)
        w = ops.mesh_ray_cast(o, d, pos=pos, faces=faces, want=names)
        assert sorted(w) == sorted(set(names) | {"t"})
        _assert_equal(w, ref, f"want={names}")
    # F = 0: every ray unanswered; R = 0: nothing happens, nothing is written
    arena = Arena(dev)
    t, fc, ba, hi, ws = (arena.new((R,), torch.float32), arena.new((R,), torch.int32), arena.new((R, 2), torch.float32),
                         arena.new((R, 3), torch.float32), arena.new((R,), torch.int64))
    assert call(0, R, t, fc, ba, hi, ws, faces_=None) == 0
    torch.cuda.synchronize()
    arena.check()
    assert bool(torch.isinf(t).all()) and bool((t > 0).all()) and bool((fc == -1).all()) and bool(torch.isnan(ba).all()) \
        and bool(torch.isnan(hi).all())
    before = [x.clone() for x in (t, fc, ba, hi, ws)]
    assert call(F, 0, t, fc, ba, hi, ws) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(before, (t, fc, ba, hi, ws)))
    empty = ops.mesh_ray_cast(o[:0].contiguous(), d[:0].contiguous(), pos=pos, faces=faces)
    assert tuple(empty["t"].shape) == (0,) and tuple(empty["bary"].shape) == (0, 2) and tuple(empty["hit"].shape) == (0, 3)
    none = ops.mesh_ray_cast(o, d, pos=pos, faces=faces[:0].contiguous())
    assert bool(torch.isinf(none["t"]).all()) and bool((none["face"] == -1).all()) and bool(torch.isnan(none["hit"]).all())


# ------------------------------------------------------------------ 3. the same bits every time
def test_alone_reversed_repeated_on_a_stream_and_from_a_graph(dev):
    c = next(c for c in CASES if c["name"] == "soup F=3000 R=1000 x1 (margins)")
    o, d, pos, faces = _up(dev, c)
    ref = rc.references()[c["name"]]
    R = len(c["origins"])
    _assert_equal(_cast(c, o, d, pos, faces), ref, "batch")
    for k in (0, 255, 256, 999):                                   # a ray alone
        one = _cast(c, o[k:k + 1].contiguous(), d[k:k + 1].contiguous(), pos, faces)
        _assert_equal(one, tuple(r[k:k + 1] for r in ref), f"ray {k} alone")
    rev = _cast(c, o.flip(0).contiguous(), d.flip(0).contiguous(), pos, faces)
    _assert_equal({k: v.flip(0) for k, v in rev.items()}, ref, "reversed")
    for _ in range(3):
        _assert_equal(_cast(c, o, d, pos, faces), ref, "repeated")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = _cast(c, o, d, pos, faces)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    _assert_equal(other, ref, "another stream")
    # a captured graph owns its outputs (out=) and takes its workspace from its own pool
    out = dict(t=torch.zeros(R, device=dev), face=torch.zeros(R, dtype=torch.int32, device=dev), bary=torch.zeros((R, 2), device=dev),
               hit=torch.zeros((R, 3), device=dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = _cast(c, o, d, pos, faces, out=out)
    assert all(r[k].data_ptr() == out[k].data_ptr() for k in out)
    for _ in range(3):
        for x in out.values():
            x.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        _assert_equal(out, ref, "graph replay")
    o.copy_(o.flip(0))                                             # new rays in the graph's input buffers: the replay computes them
    d.copy_(d.flip(0))
    g.replay()
    torch.cuda.synchronize()
    _assert_equal({k: v.flip(0) for k, v in out.items()}, ref, "graph replay on new rays")


def test_wrapper_refusals_on_device_tensors(dev):
    from foundationpose_amd import _lib, ops
    c = CASES[4]
    o, d, pos, faces = _up(dev, c)
    R = len(c["origins"])
    for kw, msg in ((dict(dirs=d.double()), "dirs: expected"), (dict(dirs=d.cpu()), "dirs: expected a CUDA"),
                    (dict(origins=o.t().contiguous().t()), "origins: tensor must be contiguous"), (dict(faces=faces.long()), "faces: expected"),
                    (dict(out=dict(t=torch.zeros(R, dtype=torch.float64, device=dev))), r"out\['t'\]: expected"),
                    (dict(out=dict(hit=o)), r"out\['hit'\] overlaps origins"), (dict(out=dict(hit=d)), r"out\['hit'\] overlaps dirs")):
        args = dict(origins=o, dirs=d, pos=pos, faces=faces)
        args.update(kw)
        with pytest.raises(_lib.FpAmdError, match=msg):
            ops.mesh_ray_cast(**args)


# ------------------------------------------------------------------ 4. the layers above
def test_mesh_visibility_equals_its_stand_in(dev):
    from foundationpose_amd import ops
    pos, faces, eye, pts, shadow, edge = squares_visibility()
    t = dict(pos=torch.as_tensor(pos, device=dev), faces=torch.as_tensor(faces, device=dev))
    eyes = np.concatenate([eye, [[0.5, 0.5, -2.0], [3.0, -1.0, 0.5]]]).astype(f32)
    for cull in (0, 1, 2):
        got = ops.mesh_visibility(torch.as_tensor(pts, device=dev), torch.as_tensor(eyes, device=dev), t, cull=CULL[cull])
        assert got.dtype == torch.bool and tuple(got.shape) == (3, len(pts))
        assert np.array_equal(got.cpu().numpy(), rm.mesh_visibility(pts, eyes, pos, faces, cull=cull))
    got = ops.mesh_visibility(torch.as_tensor(pts, device=dev), torch.as_tensor(eye, device=dev), t).cpu().numpy()
    assert np.array_equal(got[0][~edge], ~shadow[~edge])
    # the cylinder: its surface samples from the eyes of the ring
    from foundationpose_amd.reconstruct import _coverage_views
    cpos, cfaces, P, K, hw, _, _ = cylinder_coverage()
    cpts, _ = mm.sample_surface(cpos, cfaces, CYL_SAMPLES, 0)
    ceyes = _coverage_views(P, K, hw, 1e-4, 0.0, "test")[2]
    ct = dict(pos=torch.as_tensor(cpos, device=dev), faces=torch.as_tensor(cfaces, device=dev))
    for rel_tol in (1e-4, 1e-2):
        got = ops.mesh_visibility(torch.as_tensor(cpts, device=dev), torch.as_tensor(ceyes, device=dev), ct, rel_tol=rel_tol)
        ref = rm.mesh_visibility(cpts, ceyes, cpos, cfaces, rel_tol)
        assert np.array_equal(got.cpu().numpy(), ref) and 0.3 < ref.mean() < 0.7


def test_view_coverage_of_the_cylinder(dev):
    from foundationpose_amd.reconstruct import view_coverage
    pos, faces, P, K, hw, share, area = cylinder_coverage()
    t = dict(pos=torch.as_tensor(pos, device=dev), faces=torch.as_tensor(faces, device=dev))
    got = view_coverage(t, P, K, hw, samples=CYL_SAMPLES)
    ref = rm.view_coverage(pos, faces, P, K, hw, CYL_SAMPLES)
    assert got.seen.is_cuda and got.seen.dtype == torch.int32 and got.points.is_cuda and tuple(got.points.shape) == (CYL_SAMPLES, 3)
    assert np.array_equal(got.face.cpu().numpy(), ref.face)
    # the samples are the stand-in's to within the rounding of one barycentric combination, which moves no sample across a silhouette
    # here: the counts are equal, and so is every figure
    assert np.array_equal(got.seen.cpu().numpy(), ref.seen)
    assert got.fraction == ref.fraction and got.per_view == ref.per_view
    assert abs(got.unseen_area - ref.unseen_area) <= 1e-12 and abs(got.area - area.sum()) <= 1e-9 * area.sum()
    assert abs(got.fraction - share) <= len(faces) / CYL_SAMPLES
    print("cylinder:", got.describe())


# The float32 floor of the distance of a surface sample to the mesh it was drawn from, in spacings of the largest |coordinate|.
# test_gpu_mesh_icp allows the root mean square of a self-alignment 16 of them, and the mean holds that here.  The largest of the
# 2 500 samples of this cylinder measured 57 spacings (2.1e-7 m), the same figure on a's side, which fp_mesh_point_distance computed
# before seen_from existed: the instrument's own error, not the selection's.  The gate on the maximum is four times that measurement.
FLOOR_MEAN_SPACINGS = 16
FLOOR_MAX_SPACINGS_MEASURED = 57
FLOOR_MAX_SPACINGS = 4 * FLOOR_MAX_SPACINGS_MEASURED


def test_compare_meshes_seen_from(dev):
    """b: the closed cylinder; a: the same without its bottom cap.  Over all of b's samples completeness charges a for the missing
    cap at the order of the radius; over the samples a ring of views above the equator saw it is 0 to within the float32 floor of
    the distance of a sample to the face it was drawn from, which a holds too (the constants above).  seen_from=None is the call
    without the keyword; views that see nothing of b are refused."""
    from foundationpose_amd.reconstruct import compare_meshes, sample_surface
    pos, faces, P, K, hw, share, _ = cylinder_coverage()
    n = CYL_SAMPLES
    b = dict(pos=torch.as_tensor(pos, device=dev), faces=torch.as_tensor(faces, device=dev))
    a = dict(pos=b["pos"], faces=b["faces"][:3 * (len(faces) // 4)].contiguous())
    spacing = float(np.spacing(f32(np.abs(pos).max())))
    plain = compare_meshes(a, b, samples=n, unit=0.001)
    none = compare_meshes(a, b, samples=n, unit=0.001, seen_from=None)
    assert plain.coverage is None and none.coverage is None and "coverage" not in plain.as_dict()
    assert plain[:8] == none[:8] and torch.equal(plain.dist_a_to_b, none.dist_a_to_b) and torch.equal(plain.dist_b_to_a, none.dist_b_to_a)
    ref = mm.compare_meshes((pos, faces[:3 * (len(faces) // 4)]), (pos, faces), n, plain.thresholds)
    assert plain[:8] == ref[:8]
    assert 0.4 * 0.05 <= plain.completeness.max <= 0.05 + 1e-6                        # the cap's centre is a radius from the rim
    seen = compare_meshes(a, b, samples=n, unit=0.001, seen_from=dict(ob_in_cams=P, Ks=K, hw=hw))
    print(f"completeness max {plain.completeness.max:.4f} m over all of b; over the {100 * seen.coverage:.1f} % seen: max "
          f"{seen.completeness.max / spacing:.1f} spacings ({seen.completeness.max:.2e} m), mean {seen.completeness.mean / spacing:.2f}; "
          f"accuracy max {seen.accuracy.max / spacing:.1f} spacings")
    assert seen.completeness.max <= FLOOR_MAX_SPACINGS * spacing and seen.completeness.mean <= FLOOR_MEAN_SPACINGS * spacing
    assert seen.recall == (1.0,) * 4
    fb = sample_surface(b, n, 0)[1].cpu().numpy()
    kept = fb < 3 * (len(faces) // 4)                                                # the side and the top: what the ring sees
    assert abs(seen.coverage - share) <= len(faces) / n and seen.as_dict()["coverage"] == seen.coverage
    assert int(seen.dist_b_to_a.numel()) == round(seen.coverage * n) == int(kept.sum())
    assert torch.equal(seen.dist_b_to_a, plain.dist_b_to_a[torch.as_tensor(kept, device=dev)])      # exactly the seen samples' distances
    assert seen.accuracy == plain.accuracy and torch.equal(seen.dist_a_to_b, plain.dist_a_to_b)       # a's side is untouched
    assert seen.hausdorff == max(seen.accuracy.max, seen.completeness.max) and seen.chamfer == 0.5 * (seen.accuracy.mean + seen.completeness.mean)
    K_off = K.copy()
    K_off[0, 2] += 5000.0                                                            # every projection lands outside the frame
    with pytest.raises(ValueError, match="seen_from: none of b's"):
        compare_meshes(a, b, samples=n, unit=0.001, seen_from=dict(ob_in_cams=P, Ks=K_off, hw=hw))


def test_estimator_view_coverage(dev):
    """FoundationPose.view_coverage runs reconstruct.view_coverage on the mesh as handed over; with no arguments it needs the
    reference views that from_reference_views keeps"""
    from foundationpose_amd.mesh import SimpleMesh
    from foundationpose_amd.reconstruct import view_coverage
    from test_gpu_pose_errors import _estimator
    pos, faces, P, K, hw, share, _ = cylinder_coverage()
    mesh = SimpleMesh(pos.astype(np.float64), faces, vertex_colors=np.full((len(pos), 3), 128, np.uint8))
    est = _estimator(mesh, dev)
    got = est.view_coverage(P, K, hw, samples=CYL_SAMPLES)
    by_hand = view_coverage(dict(pos=torch.as_tensor(pos, device=dev), faces=torch.as_tensor(faces, device=dev)), P, K, hw,
                            samples=CYL_SAMPLES)
    assert got.fraction == by_hand.fraction and got.per_view == by_hand.per_view and torch.equal(got.seen, by_hand.seen)
    with pytest.raises(RuntimeError, match="no reference views"):
        est.view_coverage()
    with pytest.raises(ValueError, match="together"):
        est.view_coverage(P, K)
    est.ref_views = dict(ob_in_cams=P, Ks=K, hw=hw)                  # what from_reference_views keeps
    assert est.view_coverage(samples=CYL_SAMPLES).fraction == got.fraction


def test_estimator_reports_on_its_own_reference_views(scene, dev):
    """from_reference_views keeps the views' poses, intrinsics and frame size; view_coverage() with no arguments is view_coverage of
    the fused mesh as handed over from those views.  The can fused from views all round has nothing no view saw (what a view did not
    see was not fused), and one view alone sees under half of it."""
    from foundationpose_amd.estimater import FoundationPose
    from foundationpose_amd.reconstruct import view_coverage
    from test_gpu_pose_errors import _estimator
    v = _noisy_reference_views(scene, dev)
    nets = _estimator(scene["mesh"], dev)
    est = FoundationPose.from_reference_views(v["rgb"], v["depth"], v["masks"], v["ob_in_cams"], v["Ks"], voxel=tm.CAN_VOXEL,
                                              scorer=nets.scorer, refiner=nets.refiner, device=dev)
    V, H, W = (int(x) for x in v["depth"].shape)
    assert est.ref_views["hw"] == (H, W) and est.ref_views["ob_in_cams"].shape == (V, 4, 4)
    n = 2000
    got = est.view_coverage(samples=n)
    P = v["ob_in_cams"].cpu().numpy() if torch.is_tensor(v["ob_in_cams"]) else np.asarray(v["ob_in_cams"])
    Ks = v["Ks"].cpu().numpy() if torch.is_tensor(v["Ks"]) else np.asarray(v["Ks"])
    mesh = dict(pos=torch.as_tensor(np.asarray(est.mesh_ori.vertices, f32), device=dev),
                faces=torch.as_tensor(np.asarray(est.mesh_ori.faces, np.int32), device=dev))
    by_hand = view_coverage(mesh, P, Ks, (H, W), samples=n)
    assert got.fraction == by_hand.fraction and got.per_view == by_hand.per_view and torch.equal(got.seen, by_hand.seen)
    assert len(got.per_view) == V and got.fraction > 0.95 and all(0.05 < x < 0.6 for x in got.per_view)
    print("fused can:", got.describe())


def test_run_demo_ref_coverage(tmp_path, dev, capsys):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_demo", os.path.join(root, "scripts", "run_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    times = mod.main(["--synthetic_ref_views", "16", "--synthetic", "1", "--standin_weights", "--ref_coverage", "--compare_samples", "5000",
                      "--debug_dir", str(tmp_path / "d")])
    assert len(times) == 1
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{"ref_coverage"')]
    assert len(lines) == 1
    rep = json.loads(lines[0])["ref_coverage"]
    assert sorted(rep) == ["area", "fraction", "per_view", "samples", "unseen_area"]
    assert rep["samples"] == 5000 and len(rep["per_view"]) == 16 and 0.9 < rep["fraction"] <= 1.0
    assert abs(rep["unseen_area"] - (1 - rep["fraction"]) * rep["area"]) <= 1e-12 and 0.04 < rep["area"] < 0.08
    print("run_demo --ref_coverage:", lines[0])
