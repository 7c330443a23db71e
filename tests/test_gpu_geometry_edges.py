"""GPU: the geometry kernels (csrc/raster.hip, warp.hip, and the per-frame / per-pose kernels of frame_ops.hip) against the CPU oracle
on the generated cases of tests/geometry_cases.py -- the meshes, cameras, windows, frames and poses that the one scene of
tests/conftest.py never reaches (tests/test_geometry_cases_host.py shows on the CPU that every case reaches its target and that
the cases tell wrong variants of each stage from the right one).  Integer outputs bit for bit; floats within the project's gates.

Non-finite rows: the reads they could steer are guarded by the kernels' own tests -- csrc/warp.hip guards every frame read with
vx0 / vx1 / vy0 / vy1, q_in, and the px / rx range tests on the converted integers (a NaN converts to 0, an infinity saturates, and
x0 + 1 of a saturated x0 wraps below 0: all refused); csrc/raster.hip culls a vertex unless zc > FP_ZNEAR and both snapped
coordinates pass the guard band, comparisons a NaN fails, so a row with a non-finite pose or window draws nothing and indexes
nothing.  The oracle's float-to-int conversion of a NaN is undefined in C, so the warp's non-finite rows are not compared by value.

The measured differences are written to $FP_GEOMETRY_REPORT_DIR/geometry_edges.json when that variable names a directory (nothing
is written otherwise); the record of the MI355X run is committed as profiles/geometry_edges.json."""
import json
import os

import numpy as np
import pytest
import torch

import geometry_cases as gc
from conftest import ROOT

pytestmark = pytest.mark.gpu

F = np.float32
REPORT = {}
ALL_OUT = ("A", "color", "depth", "xyz", "normal", "zbuf", "tri_id")
FLOATS = ("A", "color", "depth", "xyz", "normal")
PAD = 4096


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    out = os.environ.get("FP_GEOMETRY_REPORT_DIR")
    if REPORT and out:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "geometry_edges.json")
        merged = {}
        if os.path.exists(path):
            try:
                with open(path) as f:
                    merged = json.load(f)
            except Exception:
                merged = {}
        merged.update(REPORT)
        with open(path, "w") as f:
            json.dump(merged, f, indent=1, sort_keys=True)


def _t(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x), device=dev)


def _same(a, b):
    """bit for bit, with NaN == NaN whatever its payload"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _ordered(a):
    b = np.ascontiguousarray(a, F).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def _diff(out, ref):
    """-> dict(max_abs, max_ulp, not_bit_equal) over the elements finite on both sides; NaN / infinity patterns must agree"""
    out, ref = np.asarray(out, F), np.asarray(ref, F)
    fin = np.isfinite(out) & np.isfinite(ref)
    same = out.view(np.uint32) == ref.view(np.uint32)
    nb = int((~same & ~(np.isnan(out) & np.isnan(ref)) & ~((out == 0) & (ref == 0))).sum())
    if not fin.any():
        return dict(max_abs=0.0, max_ulp=0, not_bit_equal=nb)
    return dict(max_abs=float(np.abs(out[fin].astype(np.float64) - ref[fin]).max()),
                max_ulp=int(np.abs(_ordered(out[fin]) - _ordered(ref[fin])).max()), not_bit_equal=nb)


def _worst(a, b):
    return dict(max_abs=max(a["max_abs"], b["max_abs"]), max_ulp=max(a["max_ulp"], b["max_ulp"]),
                not_bit_equal=a["not_bit_equal"] + b["not_bit_equal"]) if a else b


class Arena:
    """an output placed inside a poisoned buffer"""

    def __init__(self, shape, dtype, dev, poison=-7):
        n = int(np.prod(shape))
        self.poison = poison
        self.buf = torch.full((n + 2 * PAD,), poison, dtype=dtype, device=dev)
        self.view = self.buf[PAD:PAD + n].view(*shape)
        self.n = n

    def intact(self):
        return bool((self.buf[:PAD] == self.poison).all()) and bool((self.buf[PAD + self.n:] == self.poison).all())


@pytest.fixture(scope="module")
def handles(scene, dev):
    from foundationpose_amd import ops
    out = {}
    for name, m in gc.meshes(scene).items():
        t = m["np"]
        g = lambda k: None if t.get(k) is None else _t(t[k], dev)
        tex = g("tex")
        out[name] = ops.MeshHandle(g("pos"), g("vnormals"), _t(np.asarray(t["faces"], np.int32), dev),
                                   uv=g("uv") if tex is not None else None,
                                   uv_idx=_t(np.asarray(t["uv_idx"], np.int32), dev) if tex is not None and t.get("uv_idx") is not None else None,
                                   tex=tex, vertex_color=g("vertex_color") if tex is None else None)
    return out


def _render_in_arenas(handle, P, bb, K, H, W, out_hw, diameter, dev, normalize=True, f16=False):
    """fp_render_crops (one mesh, one host K) with every output inside a poisoned arena -> (dict of tensors, arenas)"""
    import ctypes as C
    from foundationpose_amd import _lib, ops
    N, (oh, ow) = int(P.shape[0]), out_hw
    ar = dict(A=Arena((N, 6, oh, ow), torch.float16 if f16 else torch.float32, dev),
              color=Arena((N, oh, ow, 3), torch.float32, dev), depth=Arena((N, oh, ow), torch.float32, dev),
              xyz=Arena((N, oh, ow, 3), torch.float32, dev), normal=Arena((N, oh, ow, 3), torch.float32, dev),
              zbuf=Arena((N, oh, ow), torch.int32, dev), tri_id=Arena((N, oh, ow), torch.int32, dev))
    L = _lib.lib()
    ws = ops._workspace(L.fp_workspace_bytes(N, handle.V, handle.T, oh, ow), dev)
    K9 = ops._hostK32(K)
    p = lambda k: C.c_void_p(ar[k].view.data_ptr())
    flags = (ops.FLAG_NORMALIZE_XYZ if normalize else 0) | (ops.FLAG_OUT_F16 if f16 else 0)
    st = L.fp_render_crops(handle.handle, None, None, None, float(np.float32(diameter)), C.c_void_p(P.data_ptr()),
                           C.c_void_p(bb.data_ptr()), K9.ctypes.data_as(C.c_void_p), None, None, 0, int(H), int(W), N, oh, ow, 0.8, 0.5,
                           0.001, flags, p("A"), p("color"), p("depth"), p("xyz"), p("normal"), p("zbuf"), p("tri_id"),
                           C.c_void_p(ws.data_ptr()), ws.numel(), ops._stream(P))
    _lib.check(st, "fp_render_crops")
    torch.cuda.synchronize()
    return {k: a.view for k, a in ar.items()}, ar


def _oracle_render(scene, c, P=None, bb=None):
    from oracle import ops as oo
    m = gc.meshes(scene)[c["mesh"]]
    return oo.render_crops(m["np"], c["poses"] if P is None else P, c["bbox"] if bb is None else bb, c["K"], c["H"], c["W"], c["out_hw"],
                           c["diameter"], 0.001, True, want=ALL_OUT)


# ---------------------------------------------------------------------------------------------------------- rasteriser
def test_render_every_case_bit_exact_in_arenas(scene, dev, handles):
    """tri_id and zbuf of every case and pose bit for bit, the float outputs within 1e-5 absolute where they are O(1) (no pixel
    excluded), the fp16 tensor = the fp32 one rounded once, every output inside an intact poisoned arena"""
    failures = []
    rep = {}
    for c in gc.raster_cases(scene):
        ref = _oracle_render(scene, c)
        out, ar = _render_in_arenas(handles[c["mesh"]], _t(c["poses"], dev), _t(c["bbox"], dev), c["K"], c["H"], c["W"], c["out_hw"],
                                    c["diameter"], dev)
        assert all(a.intact() for a in ar.values()), f"{c['name']}: a write outside an output"
        tid, zb = out["tri_id"].cpu().numpy(), out["zbuf"].cpu().numpy().view(np.uint32)
        bad = [n for n in range(len(c["poses"])) if not (np.array_equal(tid[n], ref["tri_id"][n]) and np.array_equal(zb[n], ref["zbuf"][n]))]
        r = dict(poses=len(c["poses"]), poses_with_integer_mismatch=bad, covered=float((ref["tri_id"] >= 0).mean()))
        if bad:
            failures.append(f"{c['name']}: tri_id / zbuf differ from the oracle at poses {bad}")
        if "floats" in c["tags"]:
            for k in FLOATS:
                d = _diff(out[k].cpu().numpy(), ref[k])
                r[k] = d
                print(f"{c['name']:>16s} {k:>6s} {d}")
                if not d["max_abs"] <= 1e-5:
                    failures.append(f"{c['name']}: {k} differs by {d['max_abs']:.3e} > 1e-5")
            o16, ar16 = _render_in_arenas(handles[c["mesh"]], _t(c["poses"], dev), _t(c["bbox"], dev), c["K"], c["H"], c["W"], c["out_hw"],
                                          c["diameter"], dev, f16=True)
            assert all(a.intact() for a in ar16.values()), f"{c['name']}: a write outside an output (fp16)"
            a16 = o16["A"].cpu().numpy()
            if not np.array_equal(a16.view(np.uint16), out["A"].half().cpu().numpy().view(np.uint16)):
                failures.append(f"{c['name']}: the fp16 tensor is not the fp32 one rounded once")
            r16 = ref["A"].astype(np.float16)
            r["A_f16_mismatch_frac"] = float((a16 != r16).mean())
            if not ((a16 != r16).mean() < 1e-5 or np.abs(a16.astype(F) - r16.astype(F)).max() <= 1e-3):
                failures.append(f"{c['name']}: fp16 tensor against the oracle rounded once")
            if not (torch.equal(o16["tri_id"], out["tri_id"]) and torch.equal(o16["zbuf"], out["zbuf"])):
                failures.append(f"{c['name']}: integers change with the fp16 flag")
        rep[c["name"]] = r
    REPORT["render"] = rep
    assert not failures, "\n".join(failures)


def test_render_through_a_mesh_set_with_interleaved_objects(scene, dev, handles):
    """the 480 x 640 / 160 x 160 cases tagged 'multi' in one MeshSet call, rows interleaved: every row the oracle's integers"""
    from foundationpose_amd import ops
    from oracle import ops as oo
    K0 = np.asarray(scene["K"], np.float64)
    cs = [c for c in gc.raster_cases(scene) if "multi" in c["tags"] and c["out_hw"] == (160, 160) and (c["H"], c["W"]) == (480, 640)
          and np.array_equal(c["K"], K0)]
    assert len(cs) >= 4
    names = [c["mesh"] for c in cs]
    mset = ops.MeshSet([handles[n] for n in names])
    M = gc.meshes(scene)
    diam = ops.object_diameters([M[n]["diameter"] for n in names], dev)
    P = np.concatenate([c["poses"][:12] for c in cs])
    bb = np.concatenate([c["bbox"][:12] for c in cs])
    obj = np.concatenate([np.full(min(12, len(c["poses"])), k, np.int32) for k, c in enumerate(cs)])
    perm = np.random.default_rng(5).permutation(len(P))
    P, bb, obj = P[perm], bb[perm], obj[perm]
    assert (np.diff(obj) != 0).mean() > 0.5
    A = Arena((len(P), 6, 160, 160), torch.float32, dev)
    out = ops.render_crops(mset, _t(P, dev), _t(bb, dev), K0, 480, 640, (160, 160), diam, 0.001, True, want=("zbuf", "tri_id", "depth"),
                           A_out=A.view, obj=_t(obj, dev))
    torch.cuda.synchronize()
    assert A.intact()
    tid, zb = out["tri_id"].cpu().numpy(), out["zbuf"].cpu().numpy().view(np.uint32)
    bad = []
    for n in range(len(P)):
        ref = oo.render_crops(M[names[obj[n]]]["np"], P[n:n + 1], bb[n:n + 1], K0, 480, 640, (160, 160), M[names[obj[n]]]["diameter"],
                              0.001, True, want=("zbuf", "tri_id", "A"))
        if not (np.array_equal(tid[n], ref["tri_id"][0]) and np.array_equal(zb[n], ref["zbuf"][0])):
            bad.append((names[obj[n]], int(perm[n])))
        np.testing.assert_allclose(A.view[n].cpu().numpy(), ref["A"][0], rtol=0, atol=1e-5, err_msg=f"{names[obj[n]]} row {n}")
    assert not bad, f"(mesh, row) whose integers differ from the oracle through the mesh set: {bad}"
    REPORT["render_mesh_set"] = dict(rows=len(P), meshes=names, rows_with_integer_mismatch=len(bad))


@pytest.mark.parametrize("name", ["crossed_boxes", "can_near", "twin_faces"])
def test_render_rows_with_non_finite_pose_or_window(scene, dev, handles, name):
    """a NaN or infinite pose / window fails every cull comparison: that row is empty and equals the oracle (NaN where the oracle
    has NaN), and no other row of the batch changes a bit"""
    c = {c["name"]: c for c in gc.raster_cases(scene)}[name]
    c = dict(c, poses=c["poses"][:8], bbox=c["bbox"][:8])
    P, bb, bad = gc.nonfinite_rows(c)
    ref = _oracle_render(scene, c, P, bb)
    args = (c["K"], c["H"], c["W"], c["out_hw"], c["diameter"], dev)
    clean, _ = _render_in_arenas(handles[c["mesh"]], _t(c["poses"], dev), _t(c["bbox"], dev), *args)
    out, ar = _render_in_arenas(handles[c["mesh"]], _t(P, dev), _t(bb, dev), *args)
    assert all(a.intact() for a in ar.values())
    good = [n for n in range(len(P)) if n not in bad]
    for k in ALL_OUT:
        o, cl = out[k].cpu().numpy(), clean[k].cpu().numpy()
        assert np.array_equal(o[good].view(np.uint32), cl[good].view(np.uint32)), (k, "a clean row changed")
        if k in ("tri_id", "zbuf"):
            assert np.array_equal(o[bad].view(np.uint32), ref[k][bad].view(np.uint32)), k
            assert (o[bad].view(np.uint32) == 0xFFFFFFFF).all(), "a non-finite row drew something"
        else:
            np.testing.assert_allclose(o[bad], ref[k][bad], rtol=0, atol=1e-5, equal_nan=True, err_msg=k)
            assert np.array_equal(np.isnan(o[bad]), np.isnan(ref[k][bad])), k


# ---------------------------------------------------------------------------------------------------------------- warp
def _warp_tol(ref):
    return np.maximum(1e-6, 2.0 * np.spacing(np.abs(ref).astype(F)).astype(np.float64))


def test_warp_every_case_both_modes(scene, dev):
    """ops.warp_crops against the oracle in both modes, normalize_xyz on and off, into a poisoned arena.  The issue's bound is
    max(1e-6, 2 ulp of |ref|); on the MI355X not one element of any case differed in a bit (profiles/geometry_edges.json:
    warp_not_bit_equal_total = 0), so the test asserts equality, bit for bit.  The zero pattern of the xyz channels (the two
    thresholds) is checked on its own so that a failure names it; the count of elements that are not bit-equal is recorded."""
    from foundationpose_amd import ops
    from oracle import ops as oo
    rep = {}
    failures = []
    for c in gc.warp_cases(scene):
        rgb, xyz, depth = _t(c["rgb"], dev), _t(c["xyz"], dev), _t(c["depth"], dev)
        tf, P = _t(c["tf"], dev), _t(c["poses"], dev)
        worst = None
        for mode in (oo.MODE_REFINE, oo.MODE_SCORE):
            for normalize in (True, False):
                ref = oo.warp_crops(c["rgb"], c["xyz"], c["depth"], c["tf"], c["K"], c["poses"], c["diameter"], mode, normalize, c["out_hw"])
                B = Arena(ref.shape, torch.float32, dev)
                ops.warp_crops(rgb, xyz if mode == oo.MODE_REFINE else None, depth if mode == oo.MODE_SCORE else None, tf, c["K"], P,
                               c["diameter"], mode, normalize, out_hw=c["out_hw"], B_out=B.view)
                torch.cuda.synchronize()
                assert B.intact(), (c["name"], mode, normalize)
                out = B.view.cpu().numpy()
                worst = _worst(worst, _diff(out, ref))
                over = np.abs(out.astype(np.float64) - ref) > _warp_tol(ref)
                if over.any() or not np.array_equal(np.isnan(out), np.isnan(ref)):
                    failures.append(f"{c['name']} mode {mode} normalize {normalize}: {int(over.sum())} elements beyond the bound")
                if not _same(out, ref):
                    failures.append(f"{c['name']} mode {mode} normalize {normalize}: {int((out.view(np.uint32) != ref.view(np.uint32)).sum())} "
                                    f"elements are not the oracle's bits")
                if not np.array_equal(out[:, 3:] == 0, ref[:, 3:] == 0):
                    failures.append(f"{c['name']} mode {mode} normalize {normalize}: the thresholds fall on another side than the oracle's")
        print(f"{c['name']:>28s} {worst}")
        rep[c["name"]] = worst
    REPORT["warp"] = rep
    REPORT["warp_not_bit_equal_total"] = int(sum(r["not_bit_equal"] for r in rep.values()))
    assert not failures, "\n".join(failures)


def test_warp_rows_with_non_finite_windows(scene, dev):
    """non-finite windows, and finite ones beyond 2^31 px: nothing is read or written outside the buffers and every other row keeps
    its bits (the rows' own values are not compared: the oracle's conversion of a NaN or of such a coordinate to an integer is
    undefined in C; the device's gives 0 and saturates).  The infinite and the huge offsets are the case that found the signed
    overflow of x0 + 1 in warp_pixel: a load 2^31 texels past the frame."""
    from foundationpose_amd import ops
    from oracle import ops as oo
    cases = {c["out_hw"]: c for c in gc.warp_cases(scene) if (c["H"], c["W"]) == (480, 640)}
    for hw in ((160, 160), (17, 33), (5, 1023)):
        c = cases[hw]
        tfb, P, bad = gc.warp_nonfinite(c)
        good = [n for n in range(len(tfb)) if n not in bad]
        rgb, xyz, depth = _t(c["rgb"], dev), _t(c["xyz"], dev), _t(c["depth"], dev)
        for mode in (oo.MODE_REFINE, oo.MODE_SCORE):
            res = []
            for tf in (c["tf"], tfb):
                B = Arena((len(tf), 6) + hw, torch.float32, dev)
                ops.warp_crops(rgb, xyz if mode == oo.MODE_REFINE else None, depth if mode == oo.MODE_SCORE else None, _t(tf, dev), c["K"],
                               _t(P, dev), c["diameter"], mode, True, out_hw=hw, B_out=B.view)
                torch.cuda.synchronize()
                assert B.intact(), (hw, mode)
                res.append(B.view.cpu().numpy())
            assert np.array_equal(res[0][good].view(np.uint32), res[1][good].view(np.uint32)), (hw, mode)


# ----------------------------------------------------------------------------------------- filters and back-projection
def test_filters_and_back_projection_every_case(dev):
    """erode_depth and depth_to_xyz (both variants, several zfar) bit for bit with NaN == NaN; bilateral_filter_depth within
    max(2e-6, 17 ulp of |ref|) -- expf differs by ulps between libm and the GPU -- with the oracle's zero pattern exactly; the
    *_frames entry points return the bits of the per-frame calls"""
    from foundationpose_amd import ops
    from oracle import ops as oo
    rep = {}
    failures = []
    by_shape = {}
    for c in gc.filter_cases():
        d, zfar = c["depth"], c["zfar"]
        dt = _t(d, dev)
        by_shape.setdefault(d.shape, []).append(c)
        worst = None
        for radius in range(4):
            e_ref = oo.erode_depth(d, radius, 0.001, 0.8, zfar)
            e = ops.erode_depth(dt, radius, 0.001, 0.8, zfar).cpu().numpy()
            if not _same(e, e_ref):
                failures.append(f"{c['name']} radius {radius}: erode_depth differs at {int((e.view(np.uint32) != e_ref.view(np.uint32)).sum())} pixels")
            b_ref = oo.bilateral_filter_depth(d, radius, zfar)
            b = ops.bilateral_filter_depth(dt, radius, zfar).cpu().numpy()
            worst = _worst(worst, _diff(b, b_ref))
            tol = np.maximum(2e-6, 17.0 * np.spacing(np.abs(b_ref)).astype(np.float64))
            with np.errstate(invalid="ignore"):
                over = np.abs(b.astype(np.float64) - b_ref) > tol
            if over.any() or not np.array_equal(np.isnan(b), np.isnan(b_ref)):
                failures.append(f"{c['name']} radius {radius}: bilateral_filter_depth beyond the bound at {int(over.sum())} pixels")
            if not np.array_equal(b == 0, b_ref == 0):
                failures.append(f"{c['name']} radius {radius}: bilateral_filter_depth's zero pattern differs")
        for K in (gc.K_SKEW, gc.K_DYADIC):
            for f64, zf in ((True, np.inf), (False, zfar), (False, 0.9), (False, np.inf)):
                ref = oo.depth2xyzmap(d, K, zfar=zf, f64_internal=f64)
                out = ops.depth_to_xyz(dt, K, zfar=float(zf), f64_internal=f64).cpu().numpy()
                if not _same(out, ref):
                    failures.append(f"{c['name']} f64 {f64} zfar {zf}: depth_to_xyz differs at {int((out.view(np.uint32) != ref.view(np.uint32)).sum())} values")
        rep[c["name"]] = dict(bilateral=worst)
    for shape, cs in by_shape.items():
        stack = _t(np.stack([c["depth"] for c in cs]), dev)
        for radius in (0, 2, 3):
            ef = ops.erode_depth_frames(stack, radius, 0.001, 0.8, 2.0)
            bf = ops.bilateral_filter_depth_frames(stack, radius, 2.0)
            for f in range(len(cs)):
                assert torch.equal(ef[f].view(torch.int32), ops.erode_depth(stack[f].contiguous(), radius, 0.001, 0.8, 2.0).view(torch.int32)), (shape, f)
                assert torch.equal(bf[f].view(torch.int32), ops.bilateral_filter_depth(stack[f].contiguous(), radius, 2.0).view(torch.int32)), (shape, f)
        Ks = [gc.K_SKEW if f % 2 else gc.K_DYADIC for f in range(len(cs))]
        views = ops.Views(Ks, np.arange(len(cs)), dev)
        for f64 in (True, False):
            xf = ops.depth_to_xyz_frames(stack, views, zfar=2.0, f64_internal=f64)
            for f in range(len(cs)):
                assert torch.equal(xf[f].view(torch.int32), ops.depth_to_xyz(stack[f].contiguous(), Ks[f], zfar=2.0, f64_internal=f64).view(torch.int32)), (shape, f)
    REPORT["filters"] = rep
    assert not failures, "\n".join(failures[:40])


# -------------------------------------------------------------------------------------------------------- crop windows
def test_crop_windows_ties_collapse_and_sizes(dev):
    """bit for bit with NaN == NaN: half-integer ties (half to even), tz of 0 / negative / tiny, collapsed windows (an infinite
    scale and a NaN bbox), N of 0, 1 and 257; the same through the per-object form with the same diameters"""
    from foundationpose_amd import ops
    from oracle import ops as oo
    for c in gc.crop_window_cases():
        tf_ref, bb_ref = oo.crop_windows(c["poses"], c["K"], c["diameter"], c["ratio"], c["out_size"])
        P = _t(c["poses"].reshape(-1, 4, 4), dev)
        tf, bb = ops.crop_windows(P, c["K"], c["diameter"], c["ratio"], c["out_size"])
        assert _same(tf.cpu().numpy(), tf_ref), (c["name"], tf.cpu().numpy(), tf_ref)
        assert _same(bb.cpu().numpy(), bb_ref), (c["name"], bb.cpu().numpy(), bb_ref)
        N = len(c["poses"])
        if N == 0:
            continue                      # an empty index tensor has no address to pass
        obj = (np.arange(N) % 3).astype(np.int32)
        diam = ops.object_diameters([c["diameter"]] * 3, dev)
        tf2, bb2 = ops.crop_windows(P, c["K"], diam, c["ratio"], c["out_size"], obj=_t(obj, dev))
        assert torch.equal(tf2.view(torch.int32), tf.view(torch.int32)) and torch.equal(bb2.view(torch.int32), bb.view(torch.int32)), c["name"]
    REPORT["crop_windows"] = dict(cases=[c["name"] for c in gc.crop_window_cases()], bit_exact=True)
