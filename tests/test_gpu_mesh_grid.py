"""GPU: the uniform grid (fp_mesh_grid_count, fp_mesh_grid_fill) and the two queries answered from it (fp_mesh_grid_point_distance,
fp_mesh_grid_signed_distance) on the cases and grids of tests/mesh_grid_cases.py: dist2 and closest bit-equal and face equal to the
brute-force restatement and to the brute-force device call, feature and sign equal to fp_mesh_signed_distance's; the tables equal to
the model's (tests/mesh_grid_model.py); what the build and the queries may write; degenerate sizes; another stream and a replayed
graph; the refusal of a grid built for another mesh; a larger mesh; accel="grid" in the layers above; the benchmark script."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_grid_cases as gcs
import mesh_grid_model as mg
from test_gpu_multi_object import dev  # noqa: F401
from test_gpu_tsdf import Arena

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(gcs.cases())
TABLE_CASES = ("soup F=257 Q=64", "soup F=3000 Q=257", "ties x1", "skipped and degenerate", "every triangle skipped", "box", "crossed_boxes",
               "signed: torus 16x8", "signed: subdivided box F=1025")
SIGNED = ("dist2", "face", "closest", "feature", "sign")


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)
    return a if a.dtype.kind == "i" else a.view(np.uint32)


def _same(got, ref, what):
    for k in ref:
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


def _assert_tables(grid, tab, what):
    cs = grid.cell_start.cpu().numpy()
    assert np.array_equal(cs, tab["cell_start"]), what
    assert (grid.n_entries, grid.n_overflow) == (tab["n_entries"], tab["n_overflow"]), what
    cell_of_slot = np.repeat(np.arange(len(cs) - 1), np.diff(cs))
    e = grid.entries.cpu().numpy()
    assert np.array_equal(e[np.lexsort((e, cell_of_slot))], tab["entries"]), (what, "entries, per cell as sorted sets")
    assert np.array_equal(np.sort(grid.overflow.cpu().numpy()), tab["overflow"]), what


# ------------------------------------------------------------------ 1. every case under every grid
@pytest.mark.parametrize("name", NAMES, ids=[n.replace(" ", "_").replace(":", "") for n in NAMES])
def test_every_case_under_every_grid_has_the_brute_force_bits(dev, name):
    from foundationpose_amd import ops
    c = gcs.cases()[name]
    mesh = _mesh(dev, c["pos"], c["faces"])
    signed = name.startswith("signed: ")
    for kind in gcs.GRIDS:
        s = gcs.queries(name, kind)
        pts = torch.as_tensor(s["points"], device=dev)
        grid = _build(mesh, s["grid"])
        if name in TABLE_CASES:
            _assert_tables(grid, mg.tables(s["grid"], c["pos"], c["faces"]), (name, kind))
        got = ops.mesh_point_distance(pts, mesh, grid=grid)
        _same(got, dict(zip(("dist2", "face", "closest"), s["ref"])), (name, kind, "against the restatement"))
        _same(got, ops.mesh_point_distance(pts, mesh), (name, kind, "against the brute-force call"))
        if signed:
            brute = ops.mesh_signed_distance(pts, mesh, want=SIGNED)
            _same(ops.mesh_signed_distance(pts, mesh, want=SIGNED, grid=grid), brute, (name, kind, "signed"))
            _same(got, {k: brute[k] for k in got}, (name, kind, "signed against unsigned"))


def test_the_default_build_is_the_models_and_is_kept_on_the_dict(dev):
    from foundationpose_amd import ops
    for name in TABLE_CASES:
        c = gcs.cases()[name]
        mesh = _mesh(dev, c["pos"], c["faces"])
        grid = ops.mesh_grid_build(mesh)
        g = gcs.grid_of(c["pos"], c["faces"], "default")
        assert np.array_equal(grid.lo, g.lo) and grid.h == g.h and grid.n.tolist() == g.n.tolist() and grid.pad == g.pad
        _assert_tables(grid, mg.tables(g, c["pos"], c["faces"]), name)
        assert mesh["grid"] is grid and ops.mesh_grid_build(mesh) is grid
    s = gcs.ulp_plane()
    mesh = _mesh(dev, s["pos"], s["faces"])
    got = ops.mesh_point_distance(torch.as_tensor(s["points"], device=dev), mesh, grid=_build(mesh, s["grid"]))
    assert got["face"].tolist() == [1]


# ------------------------------------------------------------------ 2. what may be written
def _struct(g, cell_start, entries, overflow, n_entries, n_overflow):
    from foundationpose_amd import _lib
    st = _lib.MeshGridStruct()
    st.lo[:] = [float(x) for x in g.lo]
    st.n[:] = [int(x) for x in g.n]
    st.h, st.pad = float(g.h), float(g.pad)
    st.cell_start = cell_start.data_ptr()
    st.entries = entries.data_ptr() if n_entries else None
    st.overflow = overflow.data_ptr() if n_overflow else None
    st.n_entries, st.n_overflow = n_entries, n_overflow
    return st


def test_poisoned_arenas_around_the_tables_and_the_outputs(dev):
    from foundationpose_amd import _lib
    lib = _lib.lib()
    name = "skipped and degenerate"                     # stored, overflow and dropped triangles at once
    c = gcs.cases()[name]
    g = gcs.grid_of(c["pos"], c["faces"], "default")
    tab = mg.tables(g, c["pos"], c["faces"])
    assert tab["n_entries"] > 0 and tab["n_overflow"] > 0
    mesh = _mesh(dev, c["pos"], c["faces"])
    Nv, F = len(c["pos"]), len(c["faces"])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                                                   # noqa: E731
    for short_e, short_o in ((0, 0), (1, 0), (0, 1), (tab["n_entries"], tab["n_overflow"])):
        a = Arena(dev)
        cell_start, header = a.new((g.ncells + 1,), torch.int32), a.new((4,), torch.int32)
        cap_e, cap_o = tab["n_entries"] - short_e, tab["n_overflow"] - short_o
        entries, overflow = a.new((max(cap_e, 1),), torch.int32, -7), a.new((max(cap_o, 1),), torch.int32, -7)
        cursor = a.new((g.ncells + 1,), torch.int32)
        st = _struct(g, cell_start, entries, overflow, 0, 0)
        assert lib.fp_mesh_grid_count(ptr(mesh["pos"]), Nv, ptr(mesh["faces"]), F, C.byref(st), ptr(header), stream) == 0
        assert header.tolist() == [tab["n_entries"], tab["n_overflow"], 0, 0]
        assert np.array_equal(cell_start.cpu().numpy(), tab["cell_start"])
        st = _struct(g, cell_start, entries, overflow, cap_e, cap_o)
        assert lib.fp_mesh_grid_fill_workspace_bytes(C.byref(st)) == 4 * (g.ncells + 1)
        assert lib.fp_mesh_grid_fill(ptr(mesh["pos"]), Nv, ptr(mesh["faces"]), F, C.byref(st), ptr(header), ptr(cursor),
                                     4 * (g.ncells + 1), stream) == 0
        torch.cuda.synchronize()
        a.check()
        want = (1 if short_e else 0) | (2 if short_o else 0)
        assert header.tolist() == [tab["n_entries"], tab["n_overflow"], want, 0], (short_e, short_o)
        if cap_e < 1:
            assert entries.tolist() == [-7]
        if cap_o < 1:
            assert overflow.tolist() == [-7]
        if not want:
            e, cs = entries.cpu().numpy(), tab["cell_start"]
            assert np.array_equal(e[np.lexsort((e, np.repeat(np.arange(g.ncells), np.diff(cs))))], tab["entries"])
            assert np.array_equal(np.sort(overflow.cpu().numpy()), tab["overflow"])
            # the query through the C ABI: poisoned outputs and workspace, every subset of the optional outputs
            pts = torch.as_tensor(c["points"], device=dev)
            Q = len(c["points"])
            ref = gcs.reference(name)
            for mask in range(4):
                b = Arena(dev)
                dist2, ws = b.new((Q,), torch.float32), b.new((Q,), torch.int64)
                face = b.new((Q,), torch.int32) if mask & 1 else None
                closest = b.new((Q, 3), torch.float32) if mask & 2 else None
                assert lib.fp_mesh_grid_point_distance(ptr(mesh["pos"]), Nv, ptr(mesh["faces"]), F, C.byref(st), ptr(pts), Q, ptr(dist2),
                                                       ptr(face) if face is not None else None,
                                                       ptr(closest) if closest is not None else None, ptr(ws), 8 * Q, stream) == 0
                torch.cuda.synchronize()
                b.check()
                got = dict(dist2=dist2, **({"face": face} if face is not None else {}), **({"closest": closest} if closest is not None else {}))
                _same(got, {k: r for k, r in zip(("dist2", "face", "closest"), ref) if k in got}, (name, mask))


def test_degenerate_sizes(dev):
    from foundationpose_amd import ops
    pos = torch.as_tensor(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0]], f32), device=dev)
    pts = torch.as_tensor(np.array([[0.2, 0.2, 1.0], [5, 5, 5]], f32), device=dev)
    none = torch.zeros((0, 3), dtype=torch.int32, device=dev)
    for faces, (n_e, n_o), face in ((none, (0, 0), [-1, -1]),                                            # F = 0
                                    (torch.tensor([[0, 1, 4], [-1, 1, 2]], dtype=torch.int32, device=dev), (0, 0), [-1, -1]),   # all dropped
                                    (torch.tensor([[0, 1, 3], [3, 3, 3]], dtype=torch.int32, device=dev), (0, 2), [-1, -1]),    # all overflow
                                    (torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev), (1, 0), [0, 0])):
        grid = ops.mesh_grid_build(pos=pos, faces=faces)
        assert (grid.n_entries > 0) == (n_e > 0) and grid.n_overflow == n_o, (faces.tolist(), grid.n_entries, grid.n_overflow)
        got = ops.mesh_point_distance(pts, pos=pos, faces=faces, grid=grid)
        _same(got, ops.mesh_point_distance(pts, pos=pos, faces=faces), faces.tolist())
        assert got["face"].tolist() == face
        empty = ops.mesh_point_distance(pts[:0].contiguous(), pos=pos, faces=faces, grid=grid)               # Q = 0
        assert empty["dist2"].shape == (0,) and empty["closest"].shape == (0, 3)
    # every triangle in the overflow list because its range is too wide: a 64 x 65 x 1 range is above 4096 cells
    big = torch.as_tensor(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32), device=dev)
    tri = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)
    grid = ops.mesh_grid_build(pos=big, faces=tri, cell=1.0 / 64)
    assert (grid.n_entries, grid.n_overflow) == (0, 1)
    _same(ops.mesh_point_distance(pts, pos=big, faces=tri, grid=grid), ops.mesh_point_distance(pts, pos=big, faces=tri), "too wide")


# ------------------------------------------------------------------ 3. launch variants and refusals
def test_another_stream_and_a_replayed_graph(dev):
    from foundationpose_amd import ops
    name = "signed: subdivided box F=3000"
    c = gcs.cases()[name]
    mesh, pts = _mesh(dev, c["pos"], c["faces"]), torch.as_tensor(c["points"], device=dev)
    grid = ops.mesh_grid_build(mesh)
    tables = ops.mesh_pseudonormals(mesh)
    ref = ops.mesh_signed_distance(pts, mesh, want=SIGNED)
    ref3 = {k: ref[k] for k in ("dist2", "face", "closest")}
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = ops.mesh_point_distance(pts, mesh, grid=grid)
        other_signed = ops.mesh_signed_distance(pts, mesh, want=SIGNED, grid=grid, tables=tables)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    _same(other, ref3, "another stream")
    _same(other_signed, ref, "another stream, signed")
    Q = len(c["points"])
    out = dict(dist2=torch.zeros(Q, device=dev), face=torch.zeros(Q, dtype=torch.int32, device=dev), closest=torch.zeros((Q, 3), device=dev))
    out_s = dict(dist2=torch.zeros(Q, device=dev), sign=torch.zeros(Q, dtype=torch.int32, device=dev),
                 feature=torch.zeros(Q, dtype=torch.int32, device=dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.mesh_point_distance(pts, mesh, out=out, grid=grid)
        ops.mesh_signed_distance(pts, mesh, want=tuple(out_s), out=out_s, grid=grid, tables=tables)
    for _ in range(3):
        for t in list(out.values()) + list(out_s.values()):
            t.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        _same(out, ref3, "graph replay")
        _same(out_s, {k: ref[k] for k in out_s}, "graph replay, signed")


def test_a_grid_of_another_mesh_is_refused(dev):
    from foundationpose_amd import _lib, ops
    c = gcs.cases()["box"]
    mesh, pts = _mesh(dev, c["pos"], c["faces"]), torch.as_tensor(c["points"], device=dev)
    grid = ops.mesh_grid_build(mesh)
    other = _mesh(dev, c["pos"], c["faces"])                            # equal values in other tensors
    for m in (other, dict(pos=mesh["pos"], faces=mesh["faces"][:-1])):
        with pytest.raises(_lib.FpAmdError, match="built for another mesh"):
            ops.mesh_point_distance(pts, m, grid=grid)
        with pytest.raises(_lib.FpAmdError, match="built for another mesh"):
            ops.mesh_signed_distance(pts, m, grid=grid, allow_open=True)
    with pytest.raises(_lib.FpAmdError, match="must be a MeshGrid"):
        ops.mesh_point_distance(pts, mesh, grid=(1, 2))
    with pytest.raises(_lib.FpAmdError, match="below 2\\^-20"):
        ops.mesh_grid_build(mesh, pad=0.0)
    with pytest.raises(_lib.FpAmdError, match="above max_cells"):
        ops.mesh_grid_build(mesh, cell=1e-6)
    assert ops.mesh_grid_build(mesh, max_cells=64).ncells <= 64


# ------------------------------------------------------------------ 4. a larger mesh, the layers above, the script
def test_twenty_thousand_faces_and_fifty_thousand_queries(dev):
    import geometry_cases as gc
    from foundationpose_amd import ops
    m = gc.box(n=41)                                                    # 20 172 faces
    mesh = _mesh(dev, m.vertices, m.faces)
    rng = np.random.default_rng(41)
    v = np.asarray(m.vertices, np.float64)
    lo, hi = v.min(0), v.max(0)
    around = rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), (30_000, 3))
    near = v[rng.integers(0, len(v), 20_000)] + rng.normal(size=(20_000, 3)) * 1e-3
    pts = torch.as_tensor(np.concatenate([around, near]).astype(f32), device=dev)
    grid = ops.mesh_grid_build(mesh)
    assert int(mesh["faces"].shape[0]) >= 20_000 and grid.ncells > 1000
    _same(ops.mesh_point_distance(pts, mesh, grid=grid), ops.mesh_point_distance(pts, mesh), "box of 20 172 faces")
    _same(ops.mesh_signed_distance(pts, mesh, want=SIGNED, grid=grid), ops.mesh_signed_distance(pts, mesh, want=SIGNED), "signed")


def test_accel_grid_gives_the_reports_and_arrays_of_brute_force(dev):
    import geometry_cases as gc
    from foundationpose_amd import reconstruct
    a, b = gc.box(n=6), gc.box(size=(0.081, 0.049, 0.121), n=9)
    plain = reconstruct.compare_meshes(a, b, samples=5000, unit=0.001, device=dev)
    fast = reconstruct.compare_meshes(a, b, samples=5000, unit=0.001, device=dev, accel="grid")
    for x, y in zip(plain, fast):
        if torch.is_tensor(x):
            assert np.array_equal(_bits(x), _bits(y))
        else:
            assert repr(x) == repr(y)
    mesh = _mesh(dev, b.vertices, b.faces)
    rng = np.random.default_rng(5)
    pts = torch.as_tensor(rng.uniform(-0.1, 0.1, (4000, 3)).astype(f32), device=dev)
    assert np.array_equal(_bits(reconstruct.signed_distance(pts, mesh)), _bits(reconstruct.signed_distance(pts, mesh, accel="grid")))
    assert isinstance(mesh.get("grid"), __import__("foundationpose_amd").ops.MeshGrid)
    assert torch.equal(reconstruct.contains(pts, mesh), reconstruct.contains(pts, mesh, accel="grid"))
    assert repr(reconstruct.signed_bias(a, b, samples=3000, device=dev)) == repr(reconstruct.signed_bias(a, b, samples=3000, device=dev, accel="grid"))
    with pytest.raises(ValueError, match="accel must be"):
        reconstruct.signed_distance(pts, mesh, accel="bvh")


def test_the_benchmark_script_runs_with_accel_grid(tmp_path):
    out = tmp_path / "mesh_grid.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_mesh_distance.py"), "--queries", "2000", "--window", "0.01",
                        "--views", "4", "--host", "50", "50", "--accel", "grid", "--out", str(out)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert json.load(open(out)) == line
    for size in line["sizes"].values():
        assert size["grid"]["equal_bits"] is True and size["grid"]["query_ms"] > 0 and size["grid"]["build_ms"] > 0
