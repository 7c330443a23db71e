"""GPU: fp_mesh_signed_distance and fp_mesh_penetration against the numpy restatement of their definitions
(tests/mesh_signed_model.py) on the generated cases (tests/mesh_signed_cases.py): dist2, closest and depth2 bit-equal, face, feature,
sign, inside and deepest equal, no tolerance; dist2, face and closest the bits of ops.mesh_point_distance; what they may write; the same
bits alone, in another order, on another stream and from a replayed graph; the wrappers' refusals; and the layers above
(FoundationPose.penetration_into, estimater.penetrations, reconstruct.signed_bias on the can fused from 16 noisy device renders,
scripts/run_demo.py --compare_mesh --signed).

FP_MESH_SIGNED_PROFILE_OUT=<file> merges the figures of a run into that JSON file (profiles/mesh_signed.json)."""
import itertools
import json

import numpy as np
import pytest
import torch

import mesh_signed_cases as sc
import mesh_signed_model as sm
import tsdf_model as tm
from mesh_distance_model import sample_surface
from test_gpu_multi_object import dev  # noqa: F401
from test_gpu_tsdf import Arena, _noisy_reference_views
from test_mesh_signed_host import CLOSED, margin_of, record, restated

pytestmark = pytest.mark.gpu
f32 = np.float32
SIGNED = ("dist2", "face", "closest", "feature", "sign")
PENETRATION = ("inside", "depth2", "deepest", "sign", "dist2")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype.kind == "i" else a.view(np.uint32)


def _assert_equal(got, ref, what, names=None):
    """got: a dict of device tensors (any subset of the outputs); ref: the restatement's dict; every array bit for bit"""
    for k in names or got:
        g, r = got[k].cpu().numpy(), ref[k]
        assert g.shape == r.shape and g.dtype == r.dtype, (what, k, g.shape, r.shape, g.dtype, r.dtype)
        bad = np.argwhere(_bits(g) != _bits(r))
        assert len(bad) == 0, (what, k, len(bad), "mismatches, first at", bad[0], g[tuple(bad[0])], r[tuple(bad[0])])


def _mesh(dev, pos, faces):
    return dict(pos=torch.as_tensor(np.ascontiguousarray(pos, f32), device=dev), faces=torch.as_tensor(np.ascontiguousarray(faces, np.int32), device=dev))


# ------------------------------------------------------------------ 1. the signed distance against the restatement
@pytest.mark.parametrize("name", CLOSED, ids=[n.replace(" ", "_") for n in CLOSED])
def test_every_closed_case_equals_the_restatement_and_the_unsigned_call(dev, name):
    from foundationpose_amd import ops
    c = sc.case(name)
    vn, en, report, ref = restated(name)
    mesh, pts = _mesh(dev, c["pos"], c["faces"]), torch.as_tensor(c["points"], device=dev)
    tables = ops.mesh_pseudonormals(mesh)
    assert tables.vn.is_cuda and tables.report.tolist() == report.tolist() and mesh["pseudonormals"] is tables
    got = ops.mesh_signed_distance(pts, mesh, want=SIGNED)
    assert sorted(got) == sorted(SIGNED)
    # the device's tables are the host library's: within 2 ulps of the restatement's.  The sign is held to the restatement on the
    # restatement's own tables, so that a last-bit difference of the host's acos cannot show in it
    exact = ops.MeshPseudonormals(torch.as_tensor(vn, device=dev), torch.as_tensor(en, device=dev), report)
    _assert_equal(ops.mesh_signed_distance(pts, mesh, tables=exact, want=SIGNED), ref, name, SIGNED)
    _assert_equal(got, ref, name + " (the library's tables)", ("dist2", "face", "closest", "feature"))
    beyond = np.sqrt(ref["dist2"].astype(np.float64)) > margin_of(c)  # the host tests' margin: up to it a last bit of a table may show
    assert np.array_equal(got["sign"].cpu().numpy()[beyond], ref["sign"][beyond])
    plain = ops.mesh_point_distance(pts, pos=mesh["pos"], faces=mesh["faces"])
    for k in plain:
        assert np.array_equal(_bits(plain[k].cpu().numpy()), _bits(got[k].cpu().numpy())), k
    assert sorted(ops.mesh_signed_distance(pts, mesh)) == ["dist2", "sign"]


def test_open_and_crossed_meshes_follow_the_definition_too(dev):
    from foundationpose_amd import ops
    rng = np.random.default_rng(3)
    for name, (pos, faces, _) in list(sc.defects().items()) + [("crossed boxes", sc.crossed_boxes() + (None,))]:
        pos = pos.astype(f32)
        pts = rng.uniform(-0.8, 0.8, (300, 3)).astype(f32)
        vn, en, report = sm.pseudonormals(pos, faces)
        ref = sm.signed_distance(pos, faces, vn, en, pts)
        exact = ops.MeshPseudonormals(torch.as_tensor(vn, device=dev), torch.as_tensor(en, device=dev), report)
        got = ops.mesh_signed_distance(torch.as_tensor(pts, device=dev), _mesh(dev, pos, faces), tables=exact, want=SIGNED, allow_open=True)
        _assert_equal(got, ref, name, SIGNED)


def test_one_chunk_of_faces_and_three_give_the_same_bits(dev):
    """2048 query tiles and more leave one chunk of all 3000 faces to a workgroup; a call on up to 1000 queries scans three chunks of
    1024"""
    from foundationpose_amd import ops
    name = "subdivided box F=3000"
    c = sc.case(name)
    _, _, _, ref = restated(name)
    mesh = _mesh(dev, c["pos"], c["faces"])
    n = 2048 * 256 + 77
    idx = np.arange(n) % len(c["points"])
    whole = ops.mesh_signed_distance(torch.as_tensor(c["points"][idx], device=dev), mesh, want=SIGNED)
    for lo, hi in ((0, 1000), (300_000, 300_257), (n - 65, n)):
        part = ops.mesh_signed_distance(torch.as_tensor(c["points"][idx[lo:hi]], device=dev), mesh, want=SIGNED)
        for k in SIGNED:
            assert np.array_equal(_bits(part[k].cpu().numpy()), _bits(whole[k][lo:hi].cpu().numpy())), (k, lo)
    m = len(c["points"])
    _assert_equal({k: whole[k][:m] for k in ("dist2", "face", "closest", "feature")}, ref, "the first pass over the case in the large batch")


# ------------------------------------------------------------------ 2. the penetration against the restatement
def _placements(T, seed, extent):
    """T seeded rigid motions: any rotation, a translation of up to 0.4 of the extent"""
    return np.stack([_tf(*sc.rigid(seed + t, extent * 4 / 3)) for t in range(T)]).astype(f32)


def _tf(R, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return m


def _penetration_case(dev, T, Q, seed=0):
    """Q surface samples of a small box placed T times in and around the torus (256 faces), or around the icosphere (80 faces) for the
    largest T x Q: the restated call stays at about 2e7 pair tests"""
    from foundationpose_amd import ops
    name = "torus 16x8" if T * Q <= 20000 else "icosphere 80"
    c = sc.case(name)
    vn, en, report, _ = restated(name)
    bp, bf = sc.box((0.2 * c["extent"],) * 3)
    pts, _ = sample_surface(bp.astype(f32), bf, Q, seed)
    centre = (c["pos"].min(axis=0) + c["pos"].max(axis=0)) / 2
    tfs = _placements(T, 100 + seed, c["extent"])
    tfs[:, :3, 3] += centre
    mesh = _mesh(dev, c["pos"], c["faces"])
    mesh["pseudonormals"] = ops.MeshPseudonormals(torch.as_tensor(vn, device=dev), torch.as_tensor(en, device=dev), report)
    return c, (vn, en), mesh, pts, tfs


@pytest.mark.parametrize("T,Q", [(1, 1), (2, 63), (70, 64), (257, 65), (1, 255), (2, 256), (70, 257), (257, 1000)])
def test_penetration_equals_the_restatement(dev, T, Q):
    from foundationpose_amd import ops
    c, (vn, en), mesh, pts, tfs = _penetration_case(dev, T, Q)
    ref = sm.penetration(c["pos"], c["faces"], vn, en, pts, tfs)
    dpts, dtfs = torch.as_tensor(pts, device=dev), torch.as_tensor(tfs, device=dev)
    got = ops.mesh_penetration(dpts, dtfs, mesh, want=PENETRATION)
    _assert_equal(got, ref, f"T={T} Q={Q}", PENETRATION)
    assert T * Q < 64 or 0 < int(ref["inside"].sum()) < T * Q        # the case has points on both sides
    assert sorted(ops.mesh_penetration(dpts, dtfs, mesh)) == ["deepest", "depth2", "inside"]
    for t in sorted({0, T // 2, T - 1}):                              # row t alone is row t of the batch
        one = ops.mesh_penetration(dpts, dtfs[t:t + 1].contiguous(), mesh, want=PENETRATION)
        _assert_equal(one, {k: v[t:t + 1] for k, v in ref.items()}, f"row {t} alone", PENETRATION)
    # the (T,Q) matrices are the signed distance of the transformed points
    moved = torch.as_tensor(sm.transformed(pts, tfs).reshape(-1, 3), device=dev)
    flat = ops.mesh_signed_distance(moved, mesh)
    assert torch.equal(flat["sign"].view(T, Q), got["sign"]) and torch.equal(flat["dist2"].view(T, Q), got["dist2"])


def test_penetration_rows_that_are_not_finite(dev):
    from foundationpose_amd import ops
    c, (vn, en), mesh, pts, tfs = _penetration_case(dev, 7, 65)
    tfs[1, 0, 3] = np.nan
    tfs[2, 1, 1] = np.inf
    tfs[3, 2, 0] = -np.inf
    tfs[4, :3, :3] *= f32(3e38)                                       # overflows in the products
    tfs[5, 3, :] = np.nan                                             # row 3 is never read
    ref = sm.penetration(c["pos"], c["faces"], vn, en, pts, tfs)
    got = ops.mesh_penetration(torch.as_tensor(pts, device=dev), torch.as_tensor(tfs, device=dev), mesh, want=PENETRATION)
    _assert_equal(got, ref, "rows that are not finite", PENETRATION)
    for t in (1, 2, 3, 4):
        assert int(got["inside"][t]) == 0 and float(got["depth2"][t]) == 0 and int(got["deepest"][t]) == -1
        assert bool((got["sign"][t] == 0).all()) and bool(torch.isinf(got["dist2"][t]).all())
    assert int(got["inside"][5]) == int(ref["inside"][5]) > 0


# ------------------------------------------------------------------ 3. what they write
def test_signed_distance_writes_nothing_outside_its_outputs_and_workspace_for_every_subset(dev):
    from foundationpose_amd import _lib, ops
    lib = _lib.lib()
    name = "subdivided box F=1025"
    c = sc.case(name)
    vn, en, report, ref = restated(name)
    Q = 257
    ref = {k: v[:Q] for k, v in ref.items()}
    mesh, pts = _mesh(dev, c["pos"], c["faces"]), torch.as_tensor(c["points"][:Q], device=dev)
    dvn, den = torch.as_tensor(vn, device=dev), torch.as_tensor(en, device=dev)
    F, Nv = len(c["faces"]), len(c["pos"])
    shapes = dict(face=((Q,), torch.int32), closest=((Q, 3), torch.float32), feature=((Q,), torch.int32), sign=((Q,), torch.int32))

    def call(o, ws, F_=F, Q_=Q):
        st = lib.fp_mesh_signed_distance(ops._ptr(mesh["pos"]), Nv, ops._ptr(mesh["faces"]) if F_ else None, F_, ops._ptr(dvn), ops._ptr(den),
                                         ops._ptr(pts), Q_, ops._ptr(o["dist2"]), ops._ptr(o.get("face")), ops._ptr(o.get("closest")),
                                         ops._ptr(o.get("feature")), ops._ptr(o.get("sign")), ops._ptr(ws), Q * 8, ops._stream(pts))
        assert st == 0, lib.fp_last_error()
        torch.cuda.synchronize()

    for wanted in itertools.product((False, True), repeat=4):
        arena = Arena(dev)
        o = dict(dist2=arena.new((Q,), torch.float32))
        for (k, (shape, dt)), w in zip(shapes.items(), wanted):
            if w:
                o[k] = arena.new(shape, dt)
        ws = arena.new((Q,), torch.int64)
        call(o, ws)
        arena.check()
        _assert_equal(o, ref, f"subset {wanted}")
        names = tuple(k for k, w in zip(shapes, wanted) if w) or ("dist2",)
        w = ops.mesh_signed_distance(pts, mesh, tables=ops.MeshPseudonormals(dvn, den, report), want=names)
        assert sorted(w) == sorted(set(names) | {"dist2"})
        _assert_equal(w, ref, f"want={names}")
    # F = 0: every query unanswered; Q = 0: nothing happens, nothing is written
    arena = Arena(dev)
    o = dict(dist2=arena.new((Q,), torch.float32), **{k: arena.new(shape, dt) for k, (shape, dt) in shapes.items()})
    ws = arena.new((Q,), torch.int64)
    call(o, ws, F_=0)
    arena.check()
    assert bool(torch.isposinf(o["dist2"]).all()) and bool((o["face"] == -1).all()) and bool((o["closest"] == 0).all())
    assert bool((o["feature"] == -1).all()) and bool((o["sign"] == 0).all())
    before = {k: v.clone() for k, v in o.items()}
    keys = ws.clone()
    call(o, ws, Q_=0)
    assert all(torch.equal(before[k], o[k]) for k in o) and torch.equal(keys, ws)
    empty = ops.mesh_signed_distance(pts[:0].contiguous(), mesh, want=SIGNED)
    assert tuple(empty["sign"].shape) == (0,) and tuple(empty["closest"].shape) == (0, 3)
    none = ops.mesh_signed_distance(pts, pos=mesh["pos"], faces=mesh["faces"][:0].contiguous(), want=SIGNED, allow_open=True)
    assert bool((none["sign"] == 0).all()) and bool((none["feature"] == -1).all()) and bool(torch.isposinf(none["dist2"]).all())


def test_penetration_writes_nothing_outside_its_outputs_and_workspace_for_every_subset(dev):
    from foundationpose_amd import _lib, ops
    lib = _lib.lib()
    T, Q = 5, 257
    c, (vn, en), mesh, pts, tfs = _penetration_case(dev, T, Q, seed=1)
    ref = sm.penetration(c["pos"], c["faces"], vn, en, pts, tfs)
    dpts, dtfs = torch.as_tensor(pts, device=dev), torch.as_tensor(tfs, device=dev)
    tb = mesh["pseudonormals"]
    F, Nv = len(c["faces"]), len(c["pos"])
    shapes = dict(depth2=((T,), torch.float32), deepest=((T,), torch.int32), sign=((T, Q), torch.int32), dist2=((T, Q), torch.float32))

    def call(o, ws, F_=F, Q_=Q, T_=T):
        st = lib.fp_mesh_penetration(ops._ptr(mesh["pos"]), Nv, ops._ptr(mesh["faces"]) if F_ else None, F_, ops._ptr(tb.vn), ops._ptr(tb.en),
                                     ops._ptr(dpts), Q_, ops._ptr(dtfs), T_, ops._ptr(o["inside"]), ops._ptr(o.get("depth2")),
                                     ops._ptr(o.get("deepest")), ops._ptr(o.get("sign")), ops._ptr(o.get("dist2")), ops._ptr(ws), T * Q * 8,
                                     ops._stream(dpts))
        assert st == 0, lib.fp_last_error()
        torch.cuda.synchronize()

    for wanted in itertools.product((False, True), repeat=4):
        arena = Arena(dev)
        o = dict(inside=arena.new((T,), torch.int32))
        for (k, (shape, dt)), w in zip(shapes.items(), wanted):
            if w:
                o[k] = arena.new(shape, dt)
        ws = arena.new((T * Q,), torch.int64)
        call(o, ws)
        arena.check()
        _assert_equal(o, ref, f"subset {wanted}")
        names = tuple(k for k, w in zip(shapes, wanted) if w) or ("inside",)
        w = ops.mesh_penetration(dpts, dtfs, mesh, want=names, workspace=ops.mesh_penetration_workspace(T, Q, dev))
        assert sorted(w) == sorted(set(names) | {"inside"})
        _assert_equal(w, ref, f"want={names}")
    # F = 0 and Q = 0: every transform is empty; T = 0: nothing happens, nothing is written
    for kw in (dict(F_=0), dict(Q_=0)):
        arena = Arena(dev)
        o = dict(inside=arena.new((T,), torch.int32), depth2=arena.new((T,), torch.float32), deepest=arena.new((T,), torch.int32))
        if "F_" in kw:
            o.update(sign=arena.new((T, Q), torch.int32), dist2=arena.new((T, Q), torch.float32))
        ws = arena.new((T * Q,), torch.int64)
        call(o, ws, **kw)
        arena.check()
        assert bool((o["inside"] == 0).all()) and bool((o["depth2"] == 0).all()) and bool((o["deepest"] == -1).all())
        if "F_" in kw:
            assert bool((o["sign"] == 0).all()) and bool(torch.isposinf(o["dist2"]).all())
    before = {k: v.clone() for k, v in o.items()}
    call(o, ws, T_=0)
    assert all(torch.equal(before[k], o[k]) for k in o)
    empty = ops.mesh_penetration(dpts, dtfs[:0].contiguous(), mesh, want=PENETRATION)
    assert tuple(empty["inside"].shape) == (0,) and tuple(empty["sign"].shape) == (0, Q)
    no_points = ops.mesh_penetration(dpts[:0].contiguous(), dtfs, mesh, want=PENETRATION)
    assert no_points["inside"].tolist() == [0] * T and no_points["deepest"].tolist() == [-1] * T and tuple(no_points["dist2"].shape) == (T, 0)


# ------------------------------------------------------------------ 4. the same bits every time
def test_reversed_repeated_on_a_stream_and_from_a_graph(dev):
    from foundationpose_amd import ops
    name = "subdivided box F=3000"
    c = sc.case(name)
    vn, en, report, ref = restated(name)
    mesh, pts = _mesh(dev, c["pos"], c["faces"]), torch.as_tensor(c["points"][:1000], device=dev)
    ref = {k: v[:1000] for k, v in ref.items()}
    mesh["pseudonormals"] = ops.MeshPseudonormals(torch.as_tensor(vn, device=dev), torch.as_tensor(en, device=dev), report)
    _assert_equal(ops.mesh_signed_distance(pts, mesh, want=SIGNED), ref, "batch", SIGNED)
    for k in (0, 255, 256, 999):
        _assert_equal(ops.mesh_signed_distance(pts[k:k + 1].contiguous(), mesh, want=SIGNED), {n: v[k:k + 1] for n, v in ref.items()},
                      f"query {k} alone", SIGNED)
    rev = ops.mesh_signed_distance(pts.flip(0).contiguous(), mesh, want=SIGNED)
    _assert_equal({k: v.flip(0) for k, v in rev.items()}, ref, "reversed", SIGNED)
    for _ in range(3):
        _assert_equal(ops.mesh_signed_distance(pts, mesh, want=SIGNED), ref, "repeated", SIGNED)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = ops.mesh_signed_distance(pts, mesh, want=SIGNED)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    _assert_equal(other, ref, "another stream", SIGNED)
    out = {k: torch.zeros(ref[k].shape, dtype=ops._MESH_SIGNED_DTYPES[k], device=dev) for k in SIGNED}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = ops.mesh_signed_distance(pts, mesh, want=SIGNED, out=out)
    assert all(r[k].data_ptr() == out[k].data_ptr() for k in out)
    for _ in range(3):
        for t in out.values():
            t.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        _assert_equal(out, ref, "graph replay", SIGNED)
    pts.copy_(pts.flip(0))
    g.replay()
    torch.cuda.synchronize()
    _assert_equal({k: v.flip(0) for k, v in out.items()}, ref, "graph replay on new queries", SIGNED)


def test_penetration_reversed_repeated_on_a_stream_and_from_a_graph(dev):
    from foundationpose_amd import ops
    T, Q = 70, 257
    c, (vn, en), mesh, pts, tfs = _penetration_case(dev, T, Q, seed=2)
    ref = sm.penetration(c["pos"], c["faces"], vn, en, pts, tfs)
    dpts, dtfs = torch.as_tensor(pts, device=dev), torch.as_tensor(tfs, device=dev)
    rev = ops.mesh_penetration(dpts, dtfs.flip(0).contiguous(), mesh, want=PENETRATION)
    _assert_equal({k: v.flip(0) for k, v in rev.items()}, ref, "transforms reversed", PENETRATION)
    for _ in range(3):
        _assert_equal(ops.mesh_penetration(dpts, dtfs, mesh, want=PENETRATION), ref, "repeated", PENETRATION)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = ops.mesh_penetration(dpts, dtfs, mesh, want=PENETRATION)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    _assert_equal(other, ref, "another stream", PENETRATION)
    out = {k: torch.zeros(ref[k].shape, dtype=ops._MESH_PENETRATION_DTYPES[k], device=dev) for k in PENETRATION}
    ws = ops.mesh_penetration_workspace(T, Q, dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = ops.mesh_penetration(dpts, dtfs, mesh, want=PENETRATION, out=out, workspace=ws)
    assert all(r[k].data_ptr() == out[k].data_ptr() for k in out)
    for _ in range(3):
        for t in out.values():
            t.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        _assert_equal(out, ref, "graph replay", PENETRATION)
    dtfs.copy_(dtfs.flip(0))                                          # new transforms in the graph's input buffer
    g.replay()
    torch.cuda.synchronize()
    _assert_equal({k: v.flip(0) for k, v in out.items()}, ref, "graph replay on new transforms", PENETRATION)


# ------------------------------------------------------------------ 5. refusals
def test_wrapper_refusals_on_device_tensors(dev):
    from foundationpose_amd import _lib, ops
    c = sc.case("box")
    mesh, pts = _mesh(dev, c["pos"], c["faces"]), torch.as_tensor(c["points"], device=dev)
    Q, T = len(c["points"]), 3
    tfs = torch.eye(4, device=dev).repeat(T, 1, 1)
    tables = ops.mesh_pseudonormals(mesh)
    big = torch.zeros(4 * Q, device=dev)
    opened = _mesh(dev, c["pos"], c["faces"][2:])
    for call, base in ((ops.mesh_signed_distance, dict(points=pts)), (ops.mesh_penetration, dict(points=pts, tfs=tfs))):
        with pytest.raises(_lib.FpAmdError, match="not closed"):
            call(mesh_tensors=dict(opened), **base)
        assert "sign" in call(mesh_tensors=dict(opened), allow_open=True, want=("sign",), **base)
        for kw, msg in ((dict(points=pts.double()), "points: expected dtype"),
                        (dict(points=torch.zeros((2 * Q, 3), device=dev)[::2]), "points: tensor must be contiguous"),
                        (dict(points=pts.cpu()), "points: expected a CUDA"),
                        (dict(tables=ops.MeshPseudonormals(tables.vn.cpu(), tables.en, tables.report)), "tables.vn: expected a CUDA"),
                        (dict(tables=ops.MeshPseudonormals(tables.vn, tables.en.double(), tables.report)), "tables.en: expected dtype"),
                        (dict(tables=ops.MeshPseudonormals(tables.vn[:-1], tables.en, tables.report)), "another mesh"),
                        (dict(out=dict(sign=torch.zeros(Q, dtype=torch.int64, device=dev)), want=("sign",)), r"out\['sign'\]"),
                        (dict(out=dict(sign=tables.vn.view(-1).view(torch.int32)[:Q]), want=("sign",)), r"out\['sign'\]")):
            args = dict(base, mesh_tensors=dict(pos=mesh["pos"], faces=mesh["faces"]), tables=tables)
            args.update(kw)
            with pytest.raises(_lib.FpAmdError, match=msg):
                call(**args)
    with pytest.raises(_lib.FpAmdError, match=r"out\['closest'\] overlaps points"):
        ops.mesh_signed_distance(pts, mesh, want=("closest",), out=dict(closest=pts))
    with pytest.raises(_lib.FpAmdError, match=r"overlaps out\['"):
        ops.mesh_signed_distance(pts, mesh, want=("closest",), out=dict(dist2=big[:Q], closest=big[Q - 1:4 * Q - 1].view(Q, 3)))
    with pytest.raises(_lib.FpAmdError, match="tfs: expected dtype"):
        ops.mesh_penetration(pts, tfs.double(), mesh)
    with pytest.raises(_lib.FpAmdError, match=r"out\['inside'\] overlaps tfs"):
        ops.mesh_penetration(pts, tfs, mesh, out=dict(inside=tfs.view(-1).view(torch.int32)[:T]))
    with pytest.raises(_lib.FpAmdError, match="workspace of"):
        ops.mesh_penetration(pts, tfs, mesh, workspace=torch.zeros(T * Q - 1, dtype=torch.int64, device=dev))
    with pytest.raises(_lib.FpAmdError, match="workspace must be"):
        ops.mesh_penetration(pts, tfs, mesh, workspace=torch.zeros(T * Q, dtype=torch.int64))


# ------------------------------------------------------------------ 6. the estimator
def _box_mesh(half):
    from foundationpose_amd.mesh import SimpleMesh
    pos, faces = sc.box(half)
    return SimpleMesh(pos, faces, vertex_colors=np.full((len(pos), 3), 128, np.uint8))


def test_penetration_into_and_penetrations_equal_the_call_by_hand(dev):
    from foundationpose_amd import estimater, ops
    from foundationpose_amd.estimater import FoundationPose
    from foundationpose_amd.reconstruct import sample_surface as device_samples
    from test_gpu_pose_errors import _estimator
    a = _estimator(_box_mesh((0.05, 0.05, 0.05)), dev)
    mb = _box_mesh((0.05, 0.04, 0.06))
    mb.vertices = mb.vertices + np.array([0.2, -0.1, 0.3])              # a mesh whose model_center is not 0
    b = FoundationPose(model_pts=mb.vertices, model_normals=mb.vertex_normals, mesh=mb, scorer=a.scorer, refiner=a.refiner, device=dev)
    with pytest.raises(RuntimeError, match="no pose yet"):
        a.penetration_into(b)
    pose_b = _tf(sc.rigid(7)[0], [0.1, 0.0, 0.6])
    pose_a = pose_b @ _tf(sc.rigid(8)[0], [0.06, 0.01, -0.02])          # a's centre 0.06 off b's along b's x: the two overlap
    a.pose_last = torch.as_tensor(pose_a, device=dev, dtype=torch.float)[None]
    b.pose_last = torch.as_tensor(pose_b, device=dev, dtype=torch.float)[None]
    got = a.penetration_into(b, samples=512)
    assert isinstance(got, ops.Penetration) and got.inside.shape == (1,) and got.deepest.shape == (1, 3)
    pts, _ = device_samples(dict(pos=a.mesh_tensors["pos"], faces=a.mesh_tensors["faces"]), 512, 0)
    tf = np.linalg.inv(b.pose_last[0].cpu().numpy().astype(np.float64)) @ a.pose_last[0].cpu().numpy().astype(np.float64)
    hand = ops.mesh_penetration(pts, torch.as_tensor(tf.astype(f32), device=dev)[None], dict(pos=b.mesh_tensors["pos"], faces=b.mesh_tensors["faces"]))
    n, j = int(hand["inside"][0]), int(hand["deepest"][0])
    assert 0 < n < 512 and got.inside[0] == n / 512 and got.depth[0] == np.sqrt(np.float64(hand["depth2"][0].item()))
    assert np.array_equal(got.deepest[0], pts[j].cpu().numpy().astype(np.float64) + a.model_center)
    # the same numbers from the restatement, and a depth that the geometry allows: no deeper than b's smallest half side
    vn, en, rep = sm.pseudonormals(b.mesh_tensors["pos"].cpu().numpy(), b.mesh_tensors["faces"].cpu().numpy())
    ref = sm.penetration(b.mesh_tensors["pos"].cpu().numpy(), b.mesh_tensors["faces"].cpu().numpy(), vn, en, pts.cpu().numpy(), tf.astype(f32)[None])
    assert rep[6] == 1 and int(ref["inside"][0]) == n and int(ref["deepest"][0]) == j and 0 < got.depth[0] <= 0.04
    both = estimater.penetrations([a, b], samples=512)
    assert sorted(both) == [(0, 1), (1, 0)] and all(np.array_equal(x, y) for x, y in zip(both[0, 1], got))
    assert both[1, 0].inside[0] > 0
    far = a.penetration_into(b, poses=pose_b @ _tf(np.eye(3), [0.5, 0, 0]), samples=512)
    assert far.inside[0] == 0 and far.depth[0] == 0 and np.isnan(far.deepest).all()
    # 252 hypotheses of a around b's place arrive in one call
    hyp = a.grid_at(torch.as_tensor(pose_a[:3, 3], device=dev, dtype=torch.float))
    assert tuple(hyp.shape) == (252, 4, 4)
    many = a.penetration_into(b, poses=hyp, samples=256)
    pts, _ = device_samples(dict(pos=a.mesh_tensors["pos"], faces=a.mesh_tensors["faces"]), 256, 0)
    tfs = (np.linalg.inv(pose_b.astype(f32).astype(np.float64)) @ hyp.cpu().numpy().astype(np.float64)).astype(f32)
    ref = sm.penetration(b.mesh_tensors["pos"].cpu().numpy(), b.mesh_tensors["faces"].cpu().numpy(), vn, en, pts.cpu().numpy(), tfs)
    assert np.array_equal(many.inside * 256, ref["inside"]) and len(set(ref["inside"].tolist())) > 1


# ------------------------------------------------------------------ 7. the fused can
def _true_can(scene):
    """the can the views were rendered from, its UV seam column snapped together: make_can_mesh repeats the seam's vertices at
    sin(2 pi) = -2.4e-16 instead of 0, which position welding rightly keeps apart"""
    pos = np.round(np.asarray(scene["mesh"].vertices, np.float64), 12).astype(f32)
    return pos, np.asarray(scene["mesh"].faces, np.int32)


def test_signed_bias_of_the_fused_can(scene, dev):
    """The can fused from 16 noisy views, floaters dropped, is closed; its signed bias against the true can is recorded (no gate on
    its sign) and is, in absolute value, no larger than the unsigned accuracy mean of compare_meshes on the same samples; the
    device's figures are the restatement's on the device's own mesh arrays."""
    from foundationpose_amd import ops
    from foundationpose_amd.reconstruct import compare_meshes, contains, reconstruct_object, signed_bias, signed_distance
    v = _noisy_reference_views(scene, dev)
    mesh, fused = reconstruct_object(v["rgb"], v["depth"], v["masks"], v["ob_in_cams"], v["Ks"], voxel=tm.CAN_VOXEL, device=dev,
                                     keep_components="largest")
    report = ops.mesh_pseudonormals(fused)
    print("fused can:", report.describe(), f"{len(mesh.faces)} faces")
    assert report.closed
    pos, faces = _true_can(scene)
    true = _mesh(dev, pos, faces)
    assert ops.mesh_pseudonormals(true).closed and not ops.mesh_pseudonormals(_mesh(dev, scene["mesh"].vertices, faces)).closed
    n = 200
    bias = signed_bias(fused, true, samples=n)
    back = signed_bias(true, fused, samples=n)
    acc = compare_meshes(fused, true, samples=n, unit=tm.CAN_VOXEL)
    print(f"fused against true: {bias}; true against fused: {back}; unsigned accuracy mean {acc.accuracy.mean * 1e3:.4f} mm, "
          f"completeness mean {acc.completeness.mean * 1e3:.4f} mm")
    assert abs(bias.mean) <= acc.accuracy.mean and abs(back.mean) <= acc.completeness.mean
    assert bias.p5 <= bias.p50 <= bias.p95 and 0.0 <= bias.inside <= 1.0
    ref = sm.signed_bias((fused["pos"].cpu().numpy(), fused["faces"].cpu().numpy()), (pos, faces), n)
    # (the stand-in's samples are the device's to within the rounding of one barycentric combination, 4 * 2^-24 * 0.1 m)
    assert abs(bias.mean - ref[0]) <= 1e-7 and abs(bias.inside - ref[1]) <= 2 / n
    # signed_distance and contains: the centre of the can is inside both meshes, a point a metre away in neither
    probe = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [float("nan"), 0.0, 0.0]], device=dev)
    for m in (fused, true):
        d = signed_distance(probe, m)
        assert d[0] < -0.04 and 0.9 < d[1] < 1.0 and bool(torch.isposinf(d[2])) and contains(probe, m).tolist() == [True, False, False]
    record("can_device", dict(faces=len(mesh.faces), samples=n, mesh_report=report.describe(), voxel_m=tm.CAN_VOXEL,
                              fused_against_true_m=bias._asdict(), true_against_fused_m=back._asdict(),
                              unsigned_accuracy_mean_m=acc.accuracy.mean, unsigned_completeness_mean_m=acc.completeness.mean))


def test_run_demo_compare_mesh_signed(tmp_path, dev, capsys):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_demo", os.path.join(root, "scripts", "run_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    times = mod.main(["--synthetic_ref_views", "16", "--synthetic", "1", "--standin_weights", "--compare_mesh", "synthetic", "--signed",
                      "--compare_samples", "20000", "--ref_keep_components", "largest", "--debug_dir", str(tmp_path / "d")])
    assert len(times) == 1
    out = capsys.readouterr().out.splitlines()
    lines = [ln for ln in out if ln.startswith('{"signed_bias"')]
    assert len(lines) == 1 and len([ln for ln in out if ln.startswith('{"compare_mesh"')]) == 1
    rep = json.loads(lines[0])["signed_bias"]
    acc = json.loads(next(ln for ln in out if ln.startswith('{"compare_mesh"')))["compare_mesh"]["accuracy"]
    assert sorted(rep) == ["closed", "inside", "mean_m", "mesh_report", "p50_m", "p5_m", "p95_m"]
    assert abs(rep["mean_m"]) <= acc["mean"] and rep["p5_m"] <= rep["p50_m"] <= rep["p95_m"] and 0.0 <= rep["inside"] <= 1.0
    print("run_demo --compare_mesh --signed:", lines[0])
