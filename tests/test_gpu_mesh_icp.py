"""GPU: fp_mesh_icp_step against the numpy restatement of its definition (tests/mesh_icp_model.py) on every generated case
(tests/mesh_icp_cases.py): dist2 bit-equal and face equal; the pair counts and the status equal; the float64 sums held to the
summation-error bound against exactly rounded sums, the step to the backward error bound of the factorisation on the device's own
system, the transform to one float32 ulp of the float64 update by the device's own step (the gates of tests/test_gpu_icp.py, no
tolerance of this file's); what it may write; the same bits alone, in another order, on another stream and from a replayed graph; the
wrapper's refusals on device tensors; and the layers above it: reconstruct.align_meshes on shapes whose pose is known and on the can
fused from 16 noisy device renders (the setting of tests/test_gpu_tsdf.py), compare_meshes(tf=), FoundationPose.align_to_mesh,
scripts/run_demo.py --align_mesh and scripts/bench_mesh_align.py.  Each test prints its figures before it asserts."""
import itertools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import icp_model as im
import mesh_icp_cases as ic
import mesh_icp_model as mi
import mesh_symmetry_cases as sc
import tsdf_model as tm
from test_gpu_mesh_distance import _bits, can_fusion  # noqa: F401
from test_gpu_multi_object import dev  # noqa: F401
from test_gpu_tsdf import Arena

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = ic.kernel_cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _up(dev, c, rows=None):
    tfs = c["tfs"] if rows is None else np.ascontiguousarray(c["tfs"][rows])
    return tuple(torch.as_tensor(x, device=dev) for x in (c["points"], tfs, c["pos"], c["faces"]))


def _run(dev, c, rows=None, min_pairs=6, damping=1e-3, want=("dist2", "face"), **kw):
    """ops.mesh_icp_step on a case (or on its transforms `rows`) -> dict of numpy arrays: tfs_out, system, dist2, face"""
    from foundationpose_amd import ops
    pts, tfs, pos, faces = _up(dev, c, rows)
    got = ops.mesh_icp_step(pts, tfs, pos=pos, faces=faces, max_dist=c["max_dist"], damping=damping, min_pairs=min_pairs, want=want, **kw)
    torch.cuda.synchronize()
    out = dict(tfs_out=got[0].cpu().numpy(), system=got[1].cpu().numpy())
    out.update({k: v.cpu().numpy() for k, v in (got[2] if len(got) > 2 else {}).items()})
    return out


def _check_against_model(c, got, rows=None, min_pairs=6, damping=1e-3):
    """every gate on one call's outputs (tests/test_gpu_icp.py's _check_against_model, with the sum of dd as a 29th sum) -> figures"""
    ref = ic.references()[c["name"]]
    sel = slice(None) if rows is None else np.asarray(rows)
    terms, S, absS, sdd, tfs = ref["terms"], ref["S"][sel], ref["absS"][sel], ref["sdd"][sel], c["tfs"][sel]
    system, out = got["system"], got["tfs_out"]
    for k in ("dist2", "face"):
        if k in got:
            r = terms[k][sel]
            assert got[k].shape == r.shape and got[k].dtype == r.dtype, (k, got[k].shape, r.shape, got[k].dtype)
            bad = np.argwhere(_bits(got[k]) != _bits(r))
            assert len(bad) == 0, (c["name"], k, len(bad), "mismatches, first at", bad[0], got[k][tuple(bad[0])], r[tuple(bad[0])])
    want_sys, _ = im.finish(S, tfs, damping, min_pairs)
    assert np.array_equal(system[:, 28], S[:, 28]), np.argwhere(system[:, 28] != S[:, 28])[:8]
    assert np.array_equal(system[:, 29], want_sys[:, 29]), (system[:, 29], want_sys[:, 29])
    assert (system[:, 37:] == 0).all()
    worst_sum = worst_res = worst_ulp = 0.0
    for n in range(len(S)):
        ref29 = np.concatenate([S[n, :28], sdd[n:n + 1]])
        abs29 = np.concatenate([absS[n], sdd[n:n + 1]])
        dev29 = np.concatenate([system[n, :28], system[n, 36:37]])
        ok = np.isfinite(ref29)
        # any order of summation of k terms is within (k - 1) u sum|term| of the exact sum, and the reference is its rounding
        bound = S[n, 28] * 2.0 ** -53 * abs29
        err = np.abs(dev29[ok] - ref29[ok])
        assert (err <= bound[ok]).all(), (n, err, bound)
        assert not np.isfinite(dev29[~ok]).any()
        if ok.any() and (bound[ok] > 0).any():
            worst_sum = max(worst_sum, float((err[bound[ok] > 0] / bound[ok][bound[ok] > 0]).max()))
        x = system[n, 30:36]
        if system[n, 29] != 0:
            assert (x == 0).all() and np.array_equal(out[n].view(np.uint32), tfs[n].view(np.uint32)), n
            continue
        A = im.damped(system[n], damping).astype(np.longdouble)
        res = float(np.abs(A @ x.astype(np.longdouble) - system[n, 21:27].astype(np.longdouble)).max())
        bound = im.ldl_backward_bound(A.astype(np.float64), x)
        assert res <= bound, (n, res, bound)
        worst_res = max(worst_res, res / bound if bound > 0 else 0.0)
        upd = im.update64(tfs[n], x)
        ulp = np.spacing(np.abs(upd.astype(f32))).astype(np.float64)
        d = np.abs(out[n].astype(np.float64) - upd) / ulp
        assert (d[:3] <= 1.0).all(), (n, d.max())
        assert np.array_equal(out[n, 3].view(np.uint32), tfs[n, 3].view(np.uint32))
        worst_ulp = max(worst_ulp, float(d[:3].max()))
    return dict(pairs=S[:, 28].astype(int), status=system[:, 29].astype(int), sum_in_bounds=worst_sum, residual_in_bounds=worst_res,
                tf_in_ulps=worst_ulp)


# ------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["name"].replace(" ", "_") for c in CASES])
def test_every_generated_case(dev, ci):
    c = CASES[ci]
    fig = _check_against_model(c, _run(dev, c))
    print(f"{c['name']}: T={len(c['tfs'])} Q={len(c['points'])} F={len(c['faces'])}; pairs {fig['pairs'][:8]}, status {fig['status'][:8]}; sums at "
          f"{fig['sum_in_bounds']:.3f} of their bound, residual at {fig['residual_in_bounds']:.3f}, transforms within {fig['tf_in_ulps']:.3f} ulp")
    if c["name"].endswith("special transforms"):
        # the NaN and the infinite transform are status 2; the overflowing one has finite entries (3e38 times a rotation), its points
        # overflow, no triangle answers them and it is status 1, as fp_icp_point_plane defines the status; all three rows are copied
        # (_check_against_model compares the bits of every row whose status is not 0)
        assert (fig["status"][3:5] == 2).all() and fig["status"][5] == 1 and fig["pairs"][5] == 0
    if c["name"] == "pairs on the threshold":
        assert fig["pairs"][0] == 12
    if c["name"] == "degenerate winning face":
        assert fig["pairs"][0] == 0 and fig["status"][0] == 1


def test_min_pairs_and_damping(dev):
    c = next(c for c in CASES if c["name"] == "soup F=40 Q=257 T=3")
    base = _run(dev, c)["system"]
    n = int(np.argmax(np.where(base[:, 29] == 0, base[:, 28], -1)))
    k = int(base[n, 28])
    assert k >= 6 and base[n, 29] == 0
    for mp, want in ((k + 1, 1), (k, 0)):
        got = _run(dev, c, min_pairs=mp)
        _check_against_model(c, got, min_pairs=mp)
        assert got["system"][n, 29] == want
    got = _run(dev, c, damping=1.0)
    _check_against_model(c, got, damping=1.0)
    assert np.array_equal(got["system"][:, :29], base[:, :29]) and not np.array_equal(got["system"][n, 30:36], base[n, 30:36])


# ------------------------------------------------------------------ 2. what it writes
def test_writes_nothing_outside_its_outputs_and_workspace_for_every_subset(dev):
    from foundationpose_amd import _lib, ops
    lib = _lib.lib()
    c = next(c for c in CASES if c["name"] == "three chunks T=5")
    pts, tfs, pos, faces = _up(dev, c)
    T, Q, F, Nv = len(c["tfs"]), len(c["points"]), len(c["faces"]), len(c["pos"])
    need = int(lib.fp_mesh_icp_workspace_bytes(T, Q))
    assert need == 8 * T * Q + T * 256 and need % 8 == 0

    def call(system, tfs_out, d2, fc, ws, ws_bytes, T_=T, Q_=Q, F_=F, pts_=pts):
        st = lib.fp_mesh_icp_step(ops._ptr(pos), Nv, ops._ptr(faces), F_, ops._ptr(pts_), Q_, ops._ptr(tfs), T_, c["max_dist"], 1e-3, 6,
                                  ops._ptr(system), ops._ptr(tfs_out), ops._ptr(d2), ops._ptr(fc), ops._ptr(ws), ws_bytes, ops._stream(pts))
        assert st == 0, lib.fp_last_error()
        torch.cuda.synchronize()

    for w_out, w_d2, w_face in itertools.product((False, True), repeat=3):
        arena = Arena(dev)
        system = arena.new((T, 40), torch.float64)
        tfs_out = arena.new((T, 4, 4), torch.float32) if w_out else None
        d2 = arena.new((T, Q), torch.float32) if w_d2 else None
        fc = arena.new((T, Q), torch.int32) if w_face else None
        ws = arena.new((need // 8,), torch.float64)
        call(system, tfs_out, d2, fc, ws, need)
        arena.check()
        got = dict(system=system.cpu().numpy(), tfs_out=tfs_out.cpu().numpy() if w_out else None)
        if w_d2:
            got["dist2"] = d2.cpu().numpy()
        if w_face:
            got["face"] = fc.cpu().numpy()
        if not w_out:                                               # the system alone: checked with the restatement's own update
            got["tfs_out"] = _run(dev, c)["tfs_out"]
        _check_against_model(c, got)
    # Q = 0 and F = 0: no pair, status 1, the transforms copied; T = 0: nothing happens
    for kw in (dict(Q_=0, pts_=None), dict(F_=0)):
        arena = Arena(dev)
        system, tfs_out, ws = arena.new((T, 40), torch.float64), arena.new((T, 4, 4), torch.float32), arena.new((need // 8,), torch.float64)
        d2 = arena.new((T, Q), torch.float32, fill=5.0)
        fc = arena.new((T, Q), torch.int32, fill=5)
        call(system, tfs_out, d2, fc, ws, need, **kw)
        arena.check()
        s = system.cpu().numpy()
        assert (s[:, :29] == 0).all() and (s[:, 29] == 1).all() and (s[:, 30:] == 0).all() and torch.equal(tfs_out.view(torch.int32), tfs.view(torch.int32))
        if "F_" in kw:
            assert bool(torch.isinf(d2).all()) and bool((fc == -1).all())
        else:
            assert bool((d2 == 5.0).all()) and bool((fc == 5).all())
    arena = Arena(dev)
    system, tfs_out = arena.new((T, 40), torch.float64, fill=3.0), arena.new((T, 4, 4), torch.float32, fill=3.0)
    call(system, tfs_out, None, None, None, 0, T_=0)
    arena.check()
    assert bool((system == 3.0).all()) and bool((tfs_out == 3.0).all())
    empty = ops.mesh_icp_step(pts[:0].contiguous(), tfs, pos=pos, faces=faces, max_dist=0.1, want=("dist2",))
    assert tuple(empty[2]["dist2"].shape) == (T, 0) and bool((empty[1][:, 29] == 1).all()) and torch.equal(empty[0].view(torch.int32), tfs.view(torch.int32))
    none = ops.mesh_icp_step(pts, tfs[:0].contiguous(), pos=pos, faces=faces, max_dist=0.1)
    assert tuple(none[0].shape) == (0, 4, 4) and tuple(none[1].shape) == (0, 40)


# ------------------------------------------------------------------ 3. the same bits every time
def _same(a, b, what):
    for k in ("tfs_out", "system", "dist2", "face"):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        u = np.uint64 if x.dtype == np.float64 else np.uint32
        assert np.array_equal(x.view(u), y.view(u)), (what, k)


def test_alone_reversed_repeated_on_a_stream_and_from_a_graph(dev):
    from foundationpose_amd import ops
    c = next(c for c in CASES if c["name"] == "three chunks T=5")
    T, Q = len(c["tfs"]), len(c["points"])
    whole = _run(dev, c)
    _check_against_model(c, whole)
    for t in range(T):                                             # a transform alone: the faces are then cut into other chunks
        _same(_run(dev, c, rows=[t]), {k: v[t:t + 1] for k, v in whole.items()}, f"transform {t} alone")
    rev = _run(dev, c, rows=np.arange(T)[::-1])
    _same({k: v[::-1] for k, v in rev.items()}, whole, "reversed")
    some = [3, 0, 4]
    _same(_run(dev, c, rows=some), {k: v[some] for k, v in whole.items()}, "a subset in another order")
    for _ in range(3):
        _same(_run(dev, c), whole, "repeated")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = _run(dev, c)
    torch.cuda.current_stream().wait_stream(s)
    _same(other, whole, "another stream")
    pts, tfs, pos, faces = _up(dev, c)
    out = dict(tfs_out=torch.zeros((T, 4, 4), device=dev), system=torch.zeros((T, 40), dtype=torch.float64, device=dev),
               dist2=torch.zeros((T, Q), device=dev), face=torch.zeros((T, Q), dtype=torch.int32, device=dev))
    ws = ops.mesh_icp_workspace(T, Q, dev)
    run = lambda: ops.mesh_icp_step(pts, tfs, pos=pos, faces=faces, max_dist=c["max_dist"], want=("dist2", "face"), out=out, workspace=ws)   # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = run()
    assert r[0].data_ptr() == out["tfs_out"].data_ptr() and r[1].data_ptr() == out["system"].data_ptr()
    for _ in range(3):
        for t in out.values():
            t.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        _same({k: v.cpu().numpy() for k, v in out.items()}, whole, "graph replay")
    tfs.copy_(tfs.flip(0))                                         # new transforms in the graph's input buffer: the replay computes them
    g.replay()
    torch.cuda.synchronize()
    _same({k: v.flip(0).cpu().numpy() for k, v in out.items()}, whole, "graph replay on new transforms")


def test_many_pair_tiles_leave_the_faces_in_one_chunk_with_the_same_bits(dev):
    """T * Q = 600 x 1000 pairs: 2 344 pair tiles, more than the 2 048 workgroups the grid wants, so the 3 000 faces stay one chunk;
    five of those transforms alone have 20 tiles and the faces in three chunks: the same bits, and those equal the restatement"""
    import mesh_distance_cases as mc
    from foundationpose_amd import ops
    c = mc.soup(3000, 1000, 993)
    tfs_h = sc.rigid_transforms(600, 31, 0.1)
    tfs_h[:, 3] = (0.0, 0.0, 0.0, 1.0)
    pts, pos, faces = (torch.as_tensor(c[k], device=dev) for k in ("points", "pos", "faces"))
    run = lambda m: ops.mesh_icp_step(pts, torch.as_tensor(np.ascontiguousarray(m), device=dev), pos=pos, faces=faces, max_dist=0.05,   # noqa: E731
                                      want=("dist2", "face"))
    whole = run(tfs_h)
    some = [0, 7, 299, 598, 599]
    part = run(tfs_h[some])
    idx = torch.as_tensor(some, device=dev)
    assert torch.equal(whole[0][idx].view(torch.int32), part[0].view(torch.int32)) and torch.equal(whole[1][idx].view(torch.int64), part[1].view(torch.int64))
    assert torch.equal(whole[2]["dist2"][idx].view(torch.int32), part[2]["dist2"].view(torch.int32)) and torch.equal(whole[2]["face"][idx], part[2]["face"])
    assert bool((whole[1][:, 29] == 0).all()) and int(whole[1][:, 28].min()) > 100
    ref = mi.pair_terms(c["pos"], c["faces"], c["points"][:100], tfs_h[some[:2]], 0.05)
    assert np.array_equal(_bits(part[2]["dist2"][:2, :100].cpu().numpy()), _bits(ref["dist2"]))
    assert np.array_equal(part[2]["face"][:2, :100].cpu().numpy(), ref["face"])


def test_wrapper_refusals_on_device_tensors(dev):
    from foundationpose_amd import _lib, ops
    c = next(c for c in CASES if c["name"] == "soup F=40 Q=65 T=3")
    pts, tfs, pos, faces = _up(dev, c)
    T, Q = len(c["tfs"]), len(c["points"])
    big = torch.zeros(T * Q + T * 16 + 4, device=dev)
    for kw, msg in ((dict(points=pts.double()), "points: expected dtype"), (dict(tfs=tfs.double()), "tfs: expected dtype"),
                    (dict(pos=pos.half()), "pos: expected dtype"), (dict(faces=faces.long()), "faces: expected dtype"),
                    (dict(faces=faces.cpu()), "faces: expected a CUDA"), (dict(tfs=tfs.cpu()), "tfs: expected a CUDA"),
                    (dict(tfs=torch.zeros((T, 4, 8), device=dev)[:, :, ::2]), "tfs: tensor must be contiguous"),
                    (dict(tfs=tfs[:, :3].contiguous()), r"tfs must be \(T,4,4\)"), (dict(points=pts[:, :2].contiguous()), r"points must be \(n,3\)"),
                    (dict(out=dict(system=torch.zeros((T, 39), dtype=torch.float64, device=dev))), r"out\['system'\] must be a tensor of shape"),
                    (dict(out=dict(system=torch.zeros((T, 40), device=dev))), r"out\['system'\]: expected dtype"),
                    (dict(out=dict(tfs_out=tfs)), r"out\['tfs_out'\] overlaps tfs"),
                    (dict(out=dict(tfs_out=tfs.view(-1)[:T * 16].view(T, 4, 4))), r"out\['tfs_out'\] overlaps tfs"),
                    (dict(out=dict(dist2=torch.zeros((T, Q), device=dev))), "not among the outputs"),
                    (dict(want=("dist2",), out=dict(dist2=torch.zeros((T, Q)))), r"out\['dist2'\]: expected a CUDA"),
                    (dict(want=("dist2",), out=dict(tfs_out=big[:T * 16].view(T, 4, 4), dist2=big[T * 16 - 1:T * 16 - 1 + T * Q].view(T, Q))), r"overlaps out\['"),
                    (dict(workspace=torch.zeros(8, dtype=torch.float64, device=dev)), "workspace of"),
                    (dict(workspace=torch.zeros(8, dtype=torch.float64)), "workspace must be")):
        args = dict(points=pts, tfs=tfs, pos=pos, faces=faces, max_dist=c["max_dist"])
        args.update(kw)
        with pytest.raises(_lib.FpAmdError, match=msg):
            ops.mesh_icp_step(**args)
    for kw, msg in ((dict(max_dist=-1.0), "max_dist"), (dict(max_dist=float("inf")), "max_dist"), (dict(damping=float("nan")), "damping"),
                    (dict(min_pairs=5), "min_pairs"), (dict(want=("closest",)), "unknown name")):
        args = dict(points=pts, tfs=tfs, pos=pos, faces=faces, max_dist=c["max_dist"])
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            ops.mesh_icp_step(**args)
    good = ops.mesh_icp_step(pts, tfs, pos=pos, faces=faces, max_dist=c["max_dist"], want=("dist2",),
                             out=dict(tfs_out=big[:T * 16].view(T, 4, 4), dist2=big[T * 16:T * 16 + T * Q].view(T, Q)))
    torch.cuda.synchronize()
    _check_against_model(c, dict(tfs_out=good[0].cpu().numpy(), system=good[1].cpu().numpy(), dist2=good[2]["dist2"].cpu().numpy()))
    rows = ops.IcpStep.rows(good[1])
    assert [r.pairs for r in rows] == good[1][:, 28].cpu().numpy().astype(int).tolist()


# ------------------------------------------------------------------ 4. alignment on the device
def _tensors(dev, pos, faces):
    return dict(pos=torch.as_tensor(np.asarray(pos, f32), device=dev), faces=torch.as_tensor(np.asarray(faces, np.int32), device=dev))


@pytest.mark.parametrize("shape,seed", [(s, k) for s in ic.SHAPES for k in (1, 2, 3)])
def test_exact_copies_are_recovered(dev, shape, seed):
    from foundationpose_amd.reconstruct import align_meshes
    from foundationpose_amd.symmetry import surface_centre
    v, f = ic.SHAPES[shape]()
    pos, faces, R, t = sc.posed((v, f), seed)
    _, radius = surface_centre(pos, faces)
    got = align_meshes(_tensors(dev, v, f), _tensors(dev, pos, faces))
    deg, frac = ic.rigid_error(got.tf, ic.truth_of(R, t), radius)
    gate_deg, gate_frac = ic.alignment_gates(shape, pos)
    print(f"{shape} seed {seed}: {deg:.3e} deg, {frac:.3e} of the radius (gates {gate_deg:.3e}, {gate_frac:.3e}); rmse {got.rmse:.3e}, "
          f"overlap {got.overlap:.3f}, runner-up {got.runner_up and (got.runner_up['mean_distance'] / radius, got.runner_up['angle_deg'])}")
    assert got.status == 0 and got.overlap == 1.0 and got.tf.dtype == np.float64 and got.tf.shape == (4, 4)
    assert deg <= gate_deg and frac <= gate_frac
    assert got.runner_up is not None and got.runner_up["cost"] > 100 * got.rmse ** 2


def test_the_cube(dev):
    from foundationpose_amd.reconstruct import align_meshes
    from foundationpose_amd.symmetry import surface_centre
    v, f = sc.box_shape(1.0, 1.0, 1.0)
    pos, faces, R, t = sc.posed((v, f), 5)
    _, radius = surface_centre(pos, faces)
    got = align_meshes(_tensors(dev, v, f), _tensors(dev, pos, faces))
    d = got.tf @ np.linalg.inv(ic.truth_of(R, t))
    g = R.T @ d[:3, :3] @ R
    ang = np.degrees(np.arccos(np.clip((np.einsum("aij,ij->a", sc.cube_group(), g) - 1) / 2, -1, 1)))
    gate_deg, gate_frac = ic.alignment_gates("pulled_box", pos)
    off = np.linalg.norm(got.tf[:3, 3] - t) / radius
    floor = 16 * np.spacing(f32(np.abs(pos).max()))
    print(f"cube: {ang.min():.3e} deg from the nearest of the 24, centre off by {off:.3e} of the radius; rmse {got.rmse:.3e}, runner-up rmse "
          f"{np.sqrt(got.runner_up['cost']):.3e} at {got.runner_up['angle_deg']:.2f} deg (both <= {floor:.3e})")
    assert ang.min() <= gate_deg and off <= gate_frac
    assert got.rmse <= floor and np.sqrt(got.runner_up["cost"]) <= floor
    assert min(abs(got.runner_up["angle_deg"] - k) for k in (90.0, 120.0, 180.0)) < 0.01


def _displacement():
    from foundationpose_amd.symmetry import about, axis_rotation
    D = about(np.array([0.01, -0.02, 0.03]), axis_rotation((1.0, -2.0, 0.5), math.radians(77.0)))
    D[:3, 3] += (0.21, -0.13, 0.34)
    return D


def _symmetry_of_the_can(S):
    """how far a rigid transform is from a symmetry of the can (a rotation about z, with or without a flip, that keeps the origin)
    -> (tilt of the image of the z axis from +-z in degrees, the distance the origin moves)"""
    tilt = math.degrees(math.acos(min(1.0, abs(float(S[2, 2])))))
    return tilt, float(np.linalg.norm(S[:3, 3]))


def test_the_fused_can_displaced_and_aligned_onto_the_true_can(scene, dev, can_fusion):
    """The can fused from 16 noisy device renders, moved by a seeded rigid transform D, aligned onto the true can and compared in the
    aligned frame.  The reference is the comparison of the fused mesh where it was fused (the frame of the true can); accuracy and
    completeness means may be 10 % above it (the steps minimise a one-sided point-to-plane cost on 2 048 samples, the report is the
    two-sided mean over 100 000).  The returned transform undoes D up to a symmetry of the can: the gates on that are the symmetry
    detector's on the same mesh (tests/test_gpu_mesh_symmetry.py): the axis within one degree, the centre within two voxels."""
    from foundationpose_amd.estimater import FoundationPose
    from foundationpose_amd.reconstruct import align_meshes, compare_meshes
    from test_gpu_pose_errors import _estimator
    v, mesh, tensors = can_fusion
    true = scene["mesh"]
    D = _displacement()
    moved = dict(pos=(tensors["pos"].double() @ torch.as_tensor(D[:3, :3].T, device=dev) + torch.as_tensor(D[:3, 3], device=dev)).float().contiguous(),
                 faces=tensors["faces"])
    base = compare_meshes(tensors, true, unit=tm.CAN_VOXEL)
    got = align_meshes(moved, true)
    rep = compare_meshes(moved, true, unit=tm.CAN_VOXEL, tf=got)
    by_hand = compare_meshes(moved, true, unit=tm.CAN_VOXEL, tf=got.tf)
    S = got.tf @ D
    tilt, off = _symmetry_of_the_can(S)
    ru = got.runner_up
    print(f"fused can ({int(tensors['faces'].shape[0])} faces) onto the true can: accuracy mean {rep.accuracy.mean * 1e3:.4f} mm (undisplaced "
          f"{base.accuracy.mean * 1e3:.4f}), completeness mean {rep.completeness.mean * 1e3:.4f} mm (undisplaced {base.completeness.mean * 1e3:.4f}); "
          f"rmse {got.rmse * 1e3:.4f} mm, overlap {got.overlap:.3f}; tf D is a symmetry of the can to {tilt:.4f} deg and {off * 1e3:.4f} mm; runner-up "
          f"{ru and (ru['cost'] / got.rmse ** 2, ru['angle_deg'])}")
    assert rep.accuracy.mean <= 1.1 * base.accuracy.mean and rep.completeness.mean <= 1.1 * base.completeness.mean
    assert by_hand[:8] == rep[:8]
    assert tilt <= 1.0 and off <= 2 * tm.CAN_VOXEL
    # the continuous symmetry: another basin, a turn about the can's axis (or a flip) away, at a cost of the same size.  Every turn
    # about the axis registers the fused can equally well up to the fusion's noise, which both costs are made of: within a factor 2
    assert ru is not None and ru["angle_deg"] > 5.0 and ru["cost"] <= 2.0 * got.rmse ** 2
    tilt_r, off_r = _symmetry_of_the_can(ru["tf"] @ D)
    assert tilt_r <= 1.0 and off_r <= 2 * tm.CAN_VOXEL
    # transfer_pose: the pose of the true can's frame from a pose of the displaced fused mesh, against the known displacement
    P = np.asarray(scene["gt"], np.float64)                         # the pose of the fused mesh's own frame (= the true can's)
    back = np.linalg.inv(P) @ got.transfer_pose(P @ np.linalg.inv(D))
    tilt_p, off_p = _symmetry_of_the_can(back)
    assert tilt_p <= 1.0 and off_p <= 2 * tm.CAN_VOXEL and np.allclose(back, np.linalg.inv(S), atol=1e-9)
    # through the estimator
    true_est = _estimator(true, dev)
    from foundationpose_amd.mesh import SimpleMesh
    moved_mesh = SimpleMesh(moved["pos"].cpu().numpy(), np.asarray(mesh.faces))
    est = FoundationPose(model_pts=moved_mesh.vertices, model_normals=moved_mesh.vertex_normals, mesh=moved_mesh,
                         scorer=true_est.scorer, refiner=true_est.refiner, device=dev)
    again = est.align_to_mesh(true)
    hand = align_meshes(est.mesh_ori, true, device=dev)
    assert np.array_equal(again.tf, hand.tf) and again[1:5] == hand[1:5]
    rep_e = est.compare_to_mesh(true, unit=tm.CAN_VOXEL, tf=again)
    assert rep_e.accuracy.mean <= 1.1 * base.accuracy.mean


def test_compare_meshes_without_tf_is_unchanged_and_refuses_a_bad_one(scene, dev):
    from foundationpose_amd.reconstruct import compare_meshes
    true = scene["mesh"]
    a = compare_meshes(true, true, samples=500, unit=1e-3)
    b = compare_meshes(true, true, samples=500, unit=1e-3, tf=None)
    c = compare_meshes(true, true, samples=500, unit=1e-3, tf=np.eye(4))
    assert a[:8] == b[:8] == c[:8] and torch.equal(a.dist_a_to_b, b.dist_a_to_b) and torch.equal(a.dist_a_to_b, c.dist_a_to_b)
    with pytest.raises(ValueError, match="tf must be"):
        compare_meshes(true, true, samples=500, unit=1e-3, tf=np.eye(3))


def test_run_demo_align_mesh(tmp_path, dev, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("run_demo", os.path.join(ROOT, "scripts", "run_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    times = mod.main(["--synthetic_ref_views", "16", "--synthetic", "1", "--standin_weights", "--compare_mesh", "synthetic", "--align_mesh",
                      "--compare_samples", "20000", "--debug_dir", str(tmp_path / "d")])
    assert len(times) == 1
    lines = capsys.readouterr().out.splitlines()
    al = [json.loads(ln)["align_mesh"] for ln in lines if ln.startswith('{"align_mesh"')]
    cm = [json.loads(ln)["compare_mesh"] for ln in lines if ln.startswith('{"compare_mesh"')]
    assert len(al) == 1 and len(cm) == 1
    print("run_demo --align_mesh:", al[0])
    assert np.asarray(al[0]["tf"]).shape == (4, 4) and al[0]["status"] == 0 and al[0]["overlap"] >= 0.5 and cm[0]["aligned"] is True
    assert al[0]["rmse_m"] < tm.CAN_VOXEL and cm[0]["accuracy"]["mean"] < tm.CAN_VOXEL
    with pytest.raises(SystemExit):
        mod.main(["--synthetic", "1", "--align_mesh", "--debug_dir", str(tmp_path / "e")])


def test_bench_script_runs(dev):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_mesh_align.py"), "--transforms", "40", "--iters", "2",
                          "--fused_faces", "0", "--skip_alignment"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["transforms"] == 40 and line["samples"] == 128 and line["cases"][0]["faces"] == 4900
    assert line["cases"][0]["fused_ms"] > 0 and line["cases"][0]["materialised_ms"] > 0
    print("bench_mesh_align:", line["cases"][0])
    # report only.  The two routes need not take the same step: a sample whose nearest point lies on an edge is equally far from both
    # faces of the edge, torch's transformed points differ from the kernel's in the last bit, and the tie may go to the other face
    assert math.isfinite(line["cases"][0]["largest_step_difference"])
