"""GPU: the three batched transform queries answered from the uniform grid (fp_mesh_grid_transform_residuals, fp_mesh_grid_icp_step,
fp_mesh_grid_penetration) on the cases and grids of tests/mesh_grid_pair_cases.py: every requested output bit-equal to the same call
without a grid (float32 on uint32 views, the float64 system on uint64 views) and to the restatements the case modules hold; a row
alone; what the calls may write; degenerate sizes; another stream and a replayed graph; the refusals; a larger mesh; accel="grid" in
the layers above (align_meshes, detect_symmetries, penetration_into); the three benchmark scripts with --accel grid."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_grid_cases as gcs
import mesh_grid_model as mg
import mesh_grid_pair_cases as pc
import mesh_icp_cases as ic
import mesh_signed_model as sgm
import mesh_symmetry_cases as sc
from test_gpu_multi_object import dev  # noqa: F401
from test_gpu_tsdf import Arena

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESIDUALS = sc.kernel_cases()
ICP = ic.kernel_cases()
RESIDUAL_OUTPUTS = ("max_d2", "over", "dist2")
ICP_OUTPUTS = ("tfs_out", "system", "dist2", "face")
PENETRATION = ("inside", "depth2", "deepest", "sign", "dist2")
THRESHOLDS = (0.004, 0.011, 0.02, 0.3)


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)
    a = np.ascontiguousarray(a)
    return a if a.dtype.kind in "iu" else a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(got, ref, what, names=None):
    """dicts of tensors or arrays, bit for bit"""
    for k in names or ref:
        g, r = _bits(got[k]), _bits(ref[k])
        assert g.shape == r.shape and g.dtype == r.dtype, (what, k, g.shape, r.shape, g.dtype, r.dtype)
        bad = np.argwhere(g != r)
        assert len(bad) == 0, (what, k, len(bad), "mismatches, first at", bad[0])


def _mesh(dev, pos, faces):
    return dict(pos=torch.as_tensor(np.ascontiguousarray(pos, f32), device=dev),
                faces=torch.as_tensor(np.ascontiguousarray(faces, np.int32), device=dev))


def _build(mesh, g):
    from foundationpose_amd import ops
    return ops.mesh_grid_build(pos=mesh["pos"], faces=mesh["faces"], cell=float(g.h), pad=float(g.pad), lo=g.lo, n=g.n)


def _residuals(pts, tfs, mesh, grid=None, thresholds=THRESHOLDS, **kw):
    from foundationpose_amd import ops
    return ops.mesh_transform_residuals(pts, tfs, mesh, thresholds=thresholds, want=RESIDUAL_OUTPUTS, grid=grid, **kw)


def _icp(pts, tfs, mesh, max_dist, grid=None, **kw):
    from foundationpose_amd import ops
    got = ops.mesh_icp_step(pts, tfs, mesh, max_dist=max_dist, want=("dist2", "face"), grid=grid, **kw)
    return dict(tfs_out=got[0], system=got[1], **got[2])


def _penetration(pts, tfs, mesh, grid=None, **kw):
    from foundationpose_amd import ops
    return ops.mesh_penetration(pts, tfs, mesh, want=PENETRATION, grid=grid, **kw)


def _ids(cases):
    return [c["name"].replace(" ", "_") for c in cases]


# ------------------------------------------------------------------ 1. every case under every admitted grid
@pytest.mark.parametrize("ci", range(len(RESIDUALS)), ids=_ids(RESIDUALS))
def test_residuals_of_every_case_under_every_grid_have_the_brute_force_bits(dev, ci):
    from foundationpose_amd import _lib, ops
    lib = _lib.lib()
    c = RESIDUALS[ci]
    mesh = _mesh(dev, c["pos"], c["faces"])
    pts, tfs = torch.as_tensor(c["points"], device=dev), torch.as_tensor(c["tfs"], device=dev)
    T, Q, L = len(c["tfs"]), len(c["points"]), len(c["thr2"])
    ref = dict(zip(RESIDUAL_OUTPUTS, sc.references()[c["name"]]))
    brute = _residuals(pts, tfs, mesh)
    _same(brute, ref, (c["name"], "brute force against the restatement"), ("max_d2", "dist2"))
    thr2 = torch.as_tensor(c["thr2"], device=dev) if L else None
    kinds = pc.admitted("residuals", c)
    assert len(kinds) >= 5
    for kind in kinds:
        grid = _build(mesh, pc.grid("residuals", c["name"], kind))
        _same(_residuals(pts, tfs, mesh, grid), brute, (c["name"], kind, "against the brute-force call"))
        # the C entry point on the case's own squared thresholds, against the restatement (over is (T, 0) on both sides when L = 0)
        out = dict(max_d2=torch.empty(T, device=dev), over=torch.empty((T, L), dtype=torch.int32, device=dev), dist2=torch.empty((T, Q), device=dev))
        need = int(lib.fp_mesh_transform_residuals_workspace_bytes(T, Q))
        ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
        st = lib.fp_mesh_grid_transform_residuals(ops._ptr(mesh["pos"]), len(c["pos"]), ops._ptr(mesh["faces"]), len(c["faces"]),
                                                  C.byref(grid.struct()), ops._ptr(pts), Q, ops._ptr(tfs), T, ops._ptr(thr2), L,
                                                  ops._ptr(out["max_d2"]), ops._ptr(out["over"]) if L else None, ops._ptr(out["dist2"]),
                                                  ops._ptr(ws), need, ops._stream(pts))
        assert st == 0, lib.fp_last_error()
        torch.cuda.synchronize()
        _same(out, ref, (c["name"], kind, "against the restatement"))


@pytest.mark.parametrize("ci", range(len(ICP)), ids=_ids(ICP))
def test_icp_steps_of_every_case_under_every_grid_have_the_brute_force_bits(dev, ci):
    c = ICP[ci]
    mesh = _mesh(dev, c["pos"], c["faces"])
    pts, tfs = torch.as_tensor(c["points"], device=dev), torch.as_tensor(c["tfs"], device=dev)
    terms = ic.references()[c["name"]]["terms"]
    brute = _icp(pts, tfs, mesh, c["max_dist"])
    kinds = pc.admitted("icp", c)
    assert len(kinds) >= 5
    for kind in kinds:
        got = _icp(pts, tfs, mesh, c["max_dist"], _build(mesh, pc.grid("icp", c["name"], kind)))
        _same(got, brute, (c["name"], kind, "against the brute-force call"), ICP_OUTPUTS)
        _same(got, terms, (c["name"], kind, "against the restatement"), ("dist2", "face"))


@pytest.mark.parametrize("T,Q", pc.PENETRATION_SIZES)
def test_penetration_of_every_case_under_every_grid_has_the_brute_force_bits(dev, T, Q):
    c, (vn, en), mesh, pts, tfs, grids = pc.penetration_case(dev, T, Q)
    ref = sgm.penetration(c["pos"], c["faces"], vn, en, pts, tfs)
    dpts, dtfs = torch.as_tensor(pts, device=dev), torch.as_tensor(tfs, device=dev)
    brute = _penetration(dpts, dtfs, mesh)
    assert len(grids) >= 5
    for kind, g in grids.items():
        got = _penetration(dpts, dtfs, mesh, _build(mesh, g))
        _same(got, brute, (T, Q, kind, "against the brute-force call"), PENETRATION)
        _same(got, ref, (T, Q, kind, "against the restatement"), PENETRATION)


def test_penetration_rows_that_are_not_finite_walk_nothing(dev):
    c, (vn, en), mesh, pts, tfs, grids = pc.penetration_case(dev, 7, 65)
    tfs[1, 0, 3] = np.nan
    tfs[2, 1, 1] = np.inf
    tfs[3, 2, 0] = -np.inf
    tfs[4, :3, :3] *= f32(3e38)                                       # overflows in the products
    tfs[5, 3, :] = np.nan                                             # row 3 is never read
    ref = sgm.penetration(c["pos"], c["faces"], vn, en, pts, tfs)
    assert sorted(grids) == sorted(gcs.GRIDS)
    for kind, g in grids.items():
        got = _penetration(torch.as_tensor(pts, device=dev), torch.as_tensor(tfs, device=dev), mesh, _build(mesh, g))
        _same(got, ref, kind, PENETRATION)
        for t in (1, 2, 3, 4):
            assert int(got["inside"][t]) == 0 and int(got["deepest"][t]) == -1 and bool((got["sign"][t] == 0).all())


# ------------------------------------------------------------------ 2. a row alone
def test_a_row_alone_is_the_row_of_the_batch(dev):
    from foundationpose_amd import ops
    c = next(c for c in RESIDUALS if c["name"] == "three chunks T=5")
    mesh = _mesh(dev, c["pos"], c["faces"])
    grid = ops.mesh_grid_build(mesh)
    pts, tfs = torch.as_tensor(c["points"], device=dev), torch.as_tensor(c["tfs"], device=dev)
    T = len(c["tfs"])
    whole = _residuals(pts, tfs, mesh, grid)
    for t in sorted({0, T // 2, T - 1}):
        _same(_residuals(pts, tfs[t:t + 1].contiguous(), mesh, grid), {k: v[t:t + 1] for k, v in whole.items()}, ("residuals", t))
    c = next(c for c in ICP if c["name"] == "three chunks T=5")
    tfs = torch.as_tensor(c["tfs"], device=dev)
    whole = _icp(pts, tfs, mesh, c["max_dist"], grid)
    for t in sorted({0, T // 2, T - 1}):
        _same(_icp(pts, tfs[t:t + 1].contiguous(), mesh, c["max_dist"], grid), {k: v[t:t + 1] for k, v in whole.items()}, ("icp", t))
    T, Q = 70, 257
    c, _, mesh, pts, tfs, _ = pc.penetration_case(dev, T, Q, seed=2)
    grid = ops.mesh_grid_build(mesh)
    dpts, dtfs = torch.as_tensor(pts, device=dev), torch.as_tensor(tfs, device=dev)
    whole = _penetration(dpts, dtfs, mesh, grid)
    for t in sorted({0, T // 2, T - 1}):
        _same(_penetration(dpts, dtfs[t:t + 1].contiguous(), mesh, grid), {k: v[t:t + 1] for k, v in whole.items()}, ("penetration", t))


# ------------------------------------------------------------------ 3. what may be written
def test_poisoned_arenas_around_the_outputs_and_the_workspace_for_every_subset(dev):
    from foundationpose_amd import _lib, ops
    lib = _lib.lib()
    c = next(c for c in RESIDUALS if c["name"] == "skipped and degenerate special transforms")
    mesh = _mesh(dev, c["pos"], c["faces"])
    grid = ops.mesh_grid_build(mesh)
    cls = mg.tables(gcs.grid_of(c["pos"], c["faces"], "default"), c["pos"], c["faces"])["cls"]
    assert grid.n_entries > 0 and grid.n_overflow > 0 and (cls == mg.DROPPED).any()       # stored, overflow and dropped triangles at once
    st = grid.struct()
    pts, tfs = torch.as_tensor(c["points"], device=dev), torch.as_tensor(c["tfs"], device=dev)
    T, Q, F, Nv = len(c["tfs"]), len(c["points"]), len(c["faces"]), len(c["pos"])
    head = (ops._ptr(mesh["pos"]), Nv, ops._ptr(mesh["faces"]), F, C.byref(st))
    stream = ops._stream(pts)

    # residuals: over and dist2 are optional
    L = len(c["thr2"])
    thr2 = torch.as_tensor(c["thr2"], device=dev)
    ref = dict(zip(RESIDUAL_OUTPUTS, sc.references()[c["name"]]))
    for want_over, want_dist2 in itertools.product((False, True), repeat=2):
        a = Arena(dev)
        o = dict(max_d2=a.new((T,), torch.float32))
        if want_over:
            o["over"] = a.new((T, L), torch.int32)
        if want_dist2:
            o["dist2"] = a.new((T, Q), torch.float32)
        ws = a.new((T * Q,), torch.int32)
        assert lib.fp_mesh_grid_transform_residuals(*head, ops._ptr(pts), Q, ops._ptr(tfs), T, ops._ptr(thr2) if want_over else None,
                                                    L if want_over else 0, ops._ptr(o["max_d2"]), ops._ptr(o.get("over")),
                                                    ops._ptr(o.get("dist2")), ops._ptr(ws), 4 * T * Q, stream) == 0, lib.fp_last_error()
        torch.cuda.synchronize()
        a.check()
        _same(o, ref, ("residuals", want_over, want_dist2), tuple(o))

    # the ICP step: tfs_out, dist2 and face are optional
    ci = next(x for x in ICP if x["name"] == c["name"])
    itfs = torch.as_tensor(ci["tfs"], device=dev)
    brute = _icp(pts, itfs, mesh, ci["max_dist"])
    need = int(lib.fp_mesh_icp_workspace_bytes(T, Q))
    shapes = dict(tfs_out=((T, 4, 4), torch.float32), dist2=((T, Q), torch.float32), face=((T, Q), torch.int32))
    for wanted in itertools.product((False, True), repeat=3):
        a = Arena(dev)
        o = dict(system=a.new((T, 40), torch.float64))
        o.update({k: a.new(*shapes[k]) for k, w in zip(shapes, wanted) if w})
        ws = a.new((need // 8,), torch.float64)
        assert lib.fp_mesh_grid_icp_step(*head, ops._ptr(pts), Q, ops._ptr(itfs), T, ci["max_dist"], 1e-3, 6, ops._ptr(o["system"]),
                                         ops._ptr(o.get("tfs_out")), ops._ptr(o.get("dist2")), ops._ptr(o.get("face")), ops._ptr(ws), need,
                                         stream) == 0, lib.fp_last_error()
        torch.cuda.synchronize()
        a.check()
        _same(o, brute, ("icp", wanted), tuple(o))

    # the penetration: depth2, deepest, sign and dist2 are optional.  The mesh is open: the tables are what they are, on both sides
    tb = ops.mesh_pseudonormals(mesh)
    brute = _penetration(pts, tfs, mesh, tables=tb, allow_open=True)
    shapes = dict(depth2=((T,), torch.float32), deepest=((T,), torch.int32), sign=((T, Q), torch.int32), dist2=((T, Q), torch.float32))
    for wanted in itertools.product((False, True), repeat=4):
        a = Arena(dev)
        o = dict(inside=a.new((T,), torch.int32))
        o.update({k: a.new(*shapes[k]) for k, w in zip(shapes, wanted) if w})
        ws = a.new((T * Q,), torch.int64)
        assert lib.fp_mesh_grid_penetration(*head, ops._ptr(tb.vn), ops._ptr(tb.en), ops._ptr(pts), Q, ops._ptr(tfs), T, ops._ptr(o["inside"]),
                                            ops._ptr(o.get("depth2")), ops._ptr(o.get("deepest")), ops._ptr(o.get("sign")),
                                            ops._ptr(o.get("dist2")), ops._ptr(ws), 8 * T * Q, stream) == 0, lib.fp_last_error()
        torch.cuda.synchronize()
        a.check()
        _same(o, brute, ("penetration", wanted), tuple(o))


def test_degenerate_sizes(dev):
    from foundationpose_amd import ops
    pos = torch.as_tensor(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0]], f32), device=dev)
    pts = torch.as_tensor(np.array([[0.2, 0.2, 1.0], [5, 5, 5], [0.1, 0.3, -0.2]], f32), device=dev)
    tfs = torch.as_tensor(sc.rigid_transforms(3, 9, 1.0), device=dev)
    tfs[:, 3] = torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev)
    none = torch.zeros((0, 3), dtype=torch.int32, device=dev)
    wide_pos = torch.as_tensor(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32), device=dev)
    one = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)
    setups = ((pos, none, {}, (0, 0)),                                                                        # F = 0
              (pos, torch.tensor([[0, 1, 4], [-1, 1, 2]], dtype=torch.int32, device=dev), {}, (0, 0)),        # none stored: all dropped
              (pos, torch.tensor([[0, 1, 3], [3, 3, 3]], dtype=torch.int32, device=dev), {}, (0, 2)),         # every triangle in the overflow list
              (wide_pos, one, dict(cell=1.0 / 64), (0, 1)),                                                   # ... because its range is too wide
              (pos, one, {}, (1, 0)))
    for p, faces, kw, (n_e, n_o) in setups:
        mesh = dict(pos=p, faces=faces)
        grid = ops.mesh_grid_build(pos=p, faces=faces, **kw)
        assert (grid.n_entries > 0) == (n_e > 0) and grid.n_overflow == n_o, (faces.tolist(), grid.n_entries, grid.n_overflow)
        tb = ops.mesh_pseudonormals(mesh)
        calls = ((lambda P, M, g: _residuals(P, M, mesh, g)), (lambda P, M, g: _icp(P, M, mesh, 10.0, g)),
                 (lambda P, M, g: _penetration(P, M, mesh, g, tables=tb, allow_open=True)))
        for call in calls:
            _same(call(pts, tfs, grid), call(pts, tfs, None), faces.tolist())
            for P, M in ((pts[:0].contiguous(), tfs), (pts, tfs[:0].contiguous()), (pts[:0].contiguous(), tfs[:0].contiguous())):   # Q = 0, T = 0
                _same(call(P, M, grid), call(P, M, None), (faces.tolist(), tuple(P.shape), tuple(M.shape)))
    got = _icp(pts, tfs, dict(pos=pos, faces=one), 10.0, ops.mesh_grid_build(pos=pos, faces=one))
    assert got["face"].tolist() == [[0] * 3] * 3 and bool((got["system"][:, 28] == 3).all())


# ------------------------------------------------------------------ 4. launch variants and refusals
def test_another_stream_and_a_replayed_graph(dev):
    from foundationpose_amd import ops
    c = next(c for c in ICP if c["name"] == "three chunks T=5")
    mesh = _mesh(dev, c["pos"], c["faces"])
    grid = ops.mesh_grid_build(mesh)
    pts, tfs = torch.as_tensor(c["points"], device=dev), torch.as_tensor(c["tfs"], device=dev)
    T, Q = len(c["tfs"]), len(c["points"])
    pc_, _, pmesh, ppts, ptfs, _ = pc.penetration_case(dev, T, Q, seed=3)
    pgrid = ops.mesh_grid_build(pmesh)
    ppts, ptfs = torch.as_tensor(ppts, device=dev), torch.as_tensor(ptfs, device=dev)
    ref_r, ref_i, ref_p = _residuals(pts, tfs, mesh), _icp(pts, tfs, mesh, c["max_dist"]), _penetration(ppts, ptfs, pmesh)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got_r, got_i, got_p = _residuals(pts, tfs, mesh, grid), _icp(pts, tfs, mesh, c["max_dist"], grid), _penetration(ppts, ptfs, pmesh, pgrid)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    _same(got_r, ref_r, "another stream, residuals")
    _same(got_i, ref_i, "another stream, icp")
    _same(got_p, ref_p, "another stream, penetration")
    out_r = {k: torch.zeros_like(v) for k, v in ref_r.items()}
    out_i = {k: torch.zeros_like(v) for k, v in ref_i.items()}
    out_p = {k: torch.zeros_like(v) for k, v in ref_p.items()}
    ws_i, ws_p = ops.mesh_icp_workspace(T, Q, dev), ops.mesh_penetration_workspace(T, Q, dev)

    def run():
        _residuals(pts, tfs, mesh, grid, out=out_r)                                # its workspace is allocated inside the capture and kept by it
        _icp(pts, tfs, mesh, c["max_dist"], grid, out=out_i, workspace=ws_i)
        _penetration(ppts, ptfs, pmesh, pgrid, out=out_p, workspace=ws_p)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for _ in range(3):
        for t in itertools.chain(out_r.values(), out_i.values(), out_p.values()):
            t.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        _same(out_r, ref_r, "graph replay, residuals")
        _same(out_i, ref_i, "graph replay, icp")
        _same(out_p, ref_p, "graph replay, penetration")


def test_refusals(dev):
    from foundationpose_amd import _lib, ops, reconstruct
    c = gcs.cases()["box"]
    mesh, pts = _mesh(dev, c["pos"], c["faces"]), torch.as_tensor(c["points"][:64], device=dev)
    tfs = torch.eye(4, device=dev).repeat(3, 1, 1)
    grid = ops.mesh_grid_build(mesh)
    other = _mesh(dev, c["pos"], c["faces"])                            # equal values in other tensors
    calls = ((lambda m, g, **kw: ops.mesh_transform_residuals(pts, tfs, m, grid=g, **kw)),
             (lambda m, g, **kw: ops.mesh_icp_step(pts, tfs, m, max_dist=1.0, grid=g, **kw)),
             (lambda m, g, **kw: ops.mesh_penetration(pts, tfs, m, grid=g, allow_open=True, **kw)))
    for call in calls:
        for m in (other, dict(pos=mesh["pos"], faces=mesh["faces"][:-1])):
            with pytest.raises(_lib.FpAmdError, match="built for another mesh"):
                call(m, grid)
        with pytest.raises(_lib.FpAmdError, match="must be a MeshGrid"):
            call(mesh, (1, 2))
        # the grid is looked at after the shapes, the dtypes and the overlaps, as in mesh_point_distance
        with pytest.raises(_lib.FpAmdError, match="is not among"):
            call(mesh, (1, 2), out=dict(volume=pts))
    for fn, args in ((reconstruct.align_meshes, (mesh, other)), (reconstruct.detect_symmetries, (mesh,))):
        with pytest.raises(ValueError, match="accel must be"):
            fn(*args, accel="bvh")


# ------------------------------------------------------------------ 5. a larger mesh
def test_twenty_thousand_faces_and_sixty_four_placements(dev):
    import geometry_cases as gc
    from foundationpose_amd import ops, reconstruct
    m = gc.box(n=41)                                                    # 20 172 faces
    mesh = _mesh(dev, m.vertices, m.faces)
    grid = ops.mesh_grid_build(mesh)
    assert int(mesh["faces"].shape[0]) == 20_172 and grid.ncells > 1000
    pts, _ = reconstruct.sample_surface(mesh, 256, seed=4)
    v = np.asarray(m.vertices, np.float64)
    extent = float((v.max(0) - v.min(0)).max())
    centre = (v.max(0) + v.min(0)) / 2
    rng = np.random.default_rng(64)
    tfs = np.zeros((64, 4, 4))
    for t in range(64):                                                 # a rotation about the box's centre, then up to 5 % of the extent away
        R = sc.random_rotation(rng)
        tfs[t, :3, :3], tfs[t, :3, 3], tfs[t, 3, 3] = R, centre - R @ centre + rng.uniform(-0.05, 0.05, 3) * extent, 1.0
    tfs[0] = np.eye(4)
    tfs = torch.as_tensor(tfs.astype(f32), device=dev)
    _same(_residuals(pts, tfs, mesh, grid, thresholds=(0.01 * extent, 0.03 * extent)),
          _residuals(pts, tfs, mesh, thresholds=(0.01 * extent, 0.03 * extent)), "residuals")
    got, brute = _icp(pts, tfs, mesh, 0.1 * extent, grid), _icp(pts, tfs, mesh, 0.1 * extent)
    _same(got, brute, "icp", ICP_OUTPUTS)
    assert float(brute["dist2"][0].max()) < (1e-5 * extent) ** 2        # the identity leaves the samples on the surface
    got, brute = _penetration(pts, tfs, mesh, grid), _penetration(pts, tfs, mesh)
    _same(got, brute, "penetration", PENETRATION)
    assert 0 < int(brute["inside"].sum()) < 64 * 256


# ------------------------------------------------------------------ 6. the layers above
def _same_value(x, y, what):
    """field for field: arrays and tensors bit for bit, sequences and dicts element for element, everything else by its repr"""
    if torch.is_tensor(x) or isinstance(x, np.ndarray):
        assert type(x) is type(y) and np.array_equal(_bits(x), _bits(y)), what
    elif isinstance(x, dict):
        assert isinstance(y, dict) and sorted(x) == sorted(y), what
        for k in x:
            _same_value(x[k], y[k], (what, k))
    elif isinstance(x, (tuple, list)):
        assert type(x) is type(y) and len(x) == len(y), what
        for i, (a, b) in enumerate(zip(x, y)):
            _same_value(a, b, (what, i))
    else:
        assert repr(x) == repr(y), (what, x, y)


def test_align_meshes_with_accel_grid_is_align_meshes(dev):
    from foundationpose_amd import ops, reconstruct
    v, f = ic.SHAPES["pulled_box"]()
    pos, faces, _, _ = sc.posed((v, f), 2)
    a, b = _mesh(dev, v, f), _mesh(dev, pos, faces)
    kw = dict(starts=20, samples=(64, 256), iterations=(4, 6))
    plain = reconstruct.align_meshes(a, b, **kw)
    assert "grid" not in b
    fast = reconstruct.align_meshes(a, b, accel="grid", **kw)
    assert isinstance(fast, ops.MeshAlignment) and fast.status == 0
    _same_value(tuple(fast), tuple(plain), "align_meshes")
    assert isinstance(b.get("grid"), ops.MeshGrid) and "grid" not in a       # the grid of mesh b, kept with it


def test_detect_symmetries_with_accel_grid_is_detect_symmetries(dev):
    from foundationpose_amd import ops, reconstruct
    pos, faces, _, _ = sc.posed(sc.prism(6, 0.05, 0.08), 11)
    mesh = _mesh(dev, pos, faces)
    kw = dict(n_axes=100, samples=(32, 128))
    plain = reconstruct.detect_symmetries(mesh, **kw)
    assert "grid" not in mesh
    fast = reconstruct.detect_symmetries(mesh, accel="grid", **kw)
    assert len(plain.tfs) > 1                                           # something was found, so the policy ran its refinements too
    _same_value(tuple(fast), tuple(plain), "detect_symmetries")
    assert isinstance(mesh.get("grid"), ops.MeshGrid)


def test_penetration_into_with_accel_grid_is_penetration_into(dev):
    from foundationpose_amd import estimater, ops
    from foundationpose_amd.estimater import FoundationPose
    from test_gpu_mesh_signed import _box_mesh, _tf
    from test_gpu_pose_errors import _estimator
    import mesh_signed_cases as sgc
    a = _estimator(_box_mesh((0.05, 0.05, 0.05)), dev)
    mb = _box_mesh((0.05, 0.04, 0.06))
    mb.vertices = mb.vertices + np.array([0.2, -0.1, 0.3])
    b = FoundationPose(model_pts=mb.vertices, model_normals=mb.vertex_normals, mesh=mb, scorer=a.scorer, refiner=a.refiner, device=dev)
    pose_b = _tf(sgc.rigid(7)[0], [0.1, 0.0, 0.6])
    pose_a = pose_b @ _tf(sgc.rigid(8)[0], [0.06, 0.01, -0.02])
    a.pose_last = torch.as_tensor(pose_a, device=dev, dtype=torch.float)[None]
    b.pose_last = torch.as_tensor(pose_b, device=dev, dtype=torch.float)[None]
    plain = a.penetration_into(b, samples=512)
    assert "grid" not in b.mesh_tensors and 0 < plain.inside[0] < 1
    fast = a.penetration_into(b, samples=512, accel="grid")
    _same_value(tuple(fast), tuple(plain), "penetration_into")
    assert isinstance(b.mesh_tensors.get("grid"), ops.MeshGrid) and "grid" not in a.mesh_tensors
    hyp = a.grid_at(torch.as_tensor(pose_a[:3, 3], device=dev, dtype=torch.float))
    _same_value(tuple(a.penetration_into(b, poses=hyp, samples=256, accel="grid")), tuple(a.penetration_into(b, poses=hyp, samples=256)), "252 poses")
    both, both_fast = estimater.penetrations([a, b], samples=512), estimater.penetrations([a, b], samples=512, accel="grid")
    assert sorted(both) == sorted(both_fast) == [(0, 1), (1, 0)]
    for k in both:
        _same_value(tuple(both_fast[k]), tuple(both[k]), ("penetrations", k))
    assert isinstance(a.mesh_tensors.get("grid"), ops.MeshGrid)
    with pytest.raises(ValueError, match="accel must be"):
        a.penetration_into(b, accel="bvh")
    # the estimator's detector forwards accel and uses the grid kept with its tensors
    kept = a.mesh_tensors["grid"]
    kw = dict(rebuild_grid=False, n_axes=50, samples=(16, 64))
    _same_value(tuple(a.detect_symmetries(accel="grid", **kw)), tuple(a.detect_symmetries(**kw)), "FoundationPose.detect_symmetries")
    assert a.mesh_tensors["grid"] is kept


# ------------------------------------------------------------------ 7. the scripts
def _script(name, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", name), *args, "--accel", "grid"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _check_grid_rows(rows):
    assert len(rows) > 0
    for row in rows:
        g = row["grid"]
        assert g["equal_bits"] is True and g["query_ms"] > 0 and g["build_ms"] > 0, row


def test_the_symmetry_script_runs_with_accel_grid(dev):
    line = _script("bench_mesh_symmetry.py", "--transforms", "50", "--iters", "2", "--fused_faces", "0", "--skip_detection")
    _check_grid_rows(line["cases"])


def test_the_align_script_runs_with_accel_grid(dev):
    line = _script("bench_mesh_align.py", "--transforms", "40", "--iters", "2", "--fused_faces", "0", "--skip_alignment")
    _check_grid_rows(line["cases"])
    g = line["cases"][0]["grid"]
    assert g["morton"]["query_ms"] > 0 and len(g["near"]) == 2 and all(n["equal_bits"] is True and n["query_ms"] > 0 for n in g["near"])


def test_the_signed_script_runs_with_accel_grid(dev):
    line = _script("bench_mesh_signed.py", "--queries", "2000", "--transforms", "20", "--window", "0.01", "--rounds", "1", "--fused_faces", "0",
                   "--out", "")
    _check_grid_rows(line["cases"])
    far = line["cases"][0]["far"]
    assert far["brute_ms"] > 0 and (far.get("equal_bits") is True or "skipped" in far)
