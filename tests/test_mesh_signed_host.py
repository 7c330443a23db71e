"""Host tests of the signed point-to-mesh distance (no GPU): fp_mesh_pseudonormals (a host entry point) against its numpy restatement
and against closed forms; the restatement of the sign (tests/mesh_signed_model.py) against an independent inside test by the summed
solid angle, on every closed case of tests/mesh_signed_cases.py; the deliberately wrong variants told apart; signed_bias and the
penetration restatement against closed forms on boxes; the refusals that need no device.

The sign gate.  Measured on this restatement: the farthest query of any case whose sign disagrees with the solid-angle answer is one
of the points placed ON the surface, whose float32 coordinates are 1.5e-8 of the mesh extent off it; no random, directed or probe
query disagrees at all.  Four times that is below 16 float32 ulps of the extent, so the margin is MARGIN_ULPS = 16 ulps of the extent
(1.9e-6 of it): beyond it the signs must be equal.  FP_MESH_SIGNED_PROFILE_OUT=<file> merges the figures of a run into that JSON file
(profiles/mesh_signed.json)."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import mesh_signed_cases as sc
import mesh_signed_model as sm

f32 = np.float32
EPS = float(np.finfo(f32).eps)
MARGIN_ULPS = 16


def record(key, value):
    path = os.environ.get("FP_MESH_SIGNED_PROFILE_OUT")
    if not path:
        return
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")


def margin_of(case):
    return MARGIN_ULPS * float(np.spacing(f32(case["extent"])))


@functools.lru_cache(maxsize=None)
def restated(name):
    """a closed case through the restatement, once (the GPU tests share it): (vn, en, report, dict of the outputs)"""
    c = sc.case(name)
    vn, en, report = sm.pseudonormals(c["pos"], c["faces"])
    return vn, en, report, sm.signed_distance(c["pos"], c["faces"], vn, en, c["points"])


@functools.lru_cache(maxsize=None)
def evaluated(name):
    """a closed case through the restatement and through the float64 references, once: dict(tables, got, finite, inside, dist)"""
    c = sc.case(name)
    vn, en, report, got = restated(name)
    finite = np.isfinite(c["points"]).all(axis=1)
    inside = np.zeros(len(finite), bool)
    dist = np.full(len(finite), np.inf)
    inside[finite] = sm.inside_solid_angle(c["pos"], c["faces"], c["points"][finite])
    dist[finite] = sm.distance_float64(c["pos"], c["faces"], c["points"][finite])
    return dict(vn=vn, en=en, report=report, got=got, finite=finite, inside=inside, dist=dist)


CLOSED = [c["name"] for c in sc.closed_cases()]


def _ulps(x, ref):
    top = np.abs(ref).max() if ref.size else 0.0
    return np.abs(x.astype(np.float64) - ref.astype(np.float64)).max() / float(np.spacing(f32(top))) if ref.size and top > 0 else 0.0


def _c_tables(pos, faces):
    from foundationpose_amd import ops
    return ops.mesh_pseudonormals(pos=torch.from_numpy(np.ascontiguousarray(pos, f32)), faces=torch.from_numpy(np.ascontiguousarray(faces, np.int32)))


@pytest.mark.parametrize("name", CLOSED)
def test_the_tables_equal_the_restatement_on_closed_meshes(name):
    c = sc.case(name)
    e = evaluated(name)
    got = _c_tables(c["pos"], c["faces"])
    assert got.report.tolist() == e["report"].tolist() and got.closed
    assert got.vn.dtype == torch.float32 and tuple(got.en.shape) == (len(c["faces"]), 3, 3)
    assert _ulps(got.vn.numpy(), e["vn"]) <= 2 and _ulps(got.en.numpy(), e["en"]) <= 2


@pytest.mark.parametrize("name", list(sc.defects()))
def test_every_defect_is_named_by_its_counter(name):
    pos, faces, slots = sc.defects()[name]
    got = _c_tables(pos, faces)
    vn, en, report = sm.pseudonormals(pos.astype(f32), faces)
    assert got.report.tolist() == report.tolist()
    assert _ulps(got.vn.numpy(), vn) <= 2 and _ulps(got.en.numpy(), en) <= 2
    rep = dict(zip(sm.REPORT, got.report.tolist()))
    assert not got.closed and rep["closed"] == 0
    for k in ("boundary", "nonmanifold", "inconsistent", "degenerate"):
        assert (rep[k] > 0) == (k in slots), (k, rep)


def test_reports_of_particular_meshes():
    rep = lambda m: dict(zip(sm.REPORT, _c_tables(*m).report.tolist()))   # noqa: E731
    assert rep(sc.box()) == dict(edges=18, boundary=0, nonmanifold=0, inconsistent=0, degenerate=0, welded=0, closed=1, zero=0)
    assert rep(sc.unwelded(*sc.box())) == dict(edges=18, boundary=0, nonmanifold=0, inconsistent=0, degenerate=0, welded=28, closed=1, zero=0)
    assert rep(sc.with_zero_area(*sc.box()))["degenerate"] == 2 and rep(sc.with_zero_area(*sc.box()))["closed"] == 1
    assert rep(sc.crossed_boxes())["closed"] == 1                     # the report cannot see a self-intersection
    pos, faces = sc.box()
    assert rep((pos, faces[:0]))["closed"] == 0                       # no face: nothing is closed
    minus = np.concatenate([pos, -0.0 * np.ones((1, 3)), 0.0 * np.ones((1, 3)), np.full((2, 3), np.nan)])
    assert rep((minus, faces))["welded"] == 1                         # -0 welds to +0; a NaN welds to nothing


def test_closed_forms_on_the_axis_aligned_box():
    pos, faces = sc.box((0.5, 0.5, 0.5))
    got = _c_tables(pos, faces)
    vn, en = got.vn.numpy().astype(np.float64), got.en.numpy().astype(np.float64)
    want_vn = (math.pi / 2) * np.sign(pos)
    assert np.abs(vn - want_vn).max() <= 2 * np.spacing(f32(math.pi / 2))
    unit = np.cross(pos[faces[:, 1]] - pos[faces[:, 0]], pos[faces[:, 2]] - pos[faces[:, 0]])
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    for f in range(len(faces)):
        for k in range(3):
            a, b = pos[faces[f, k]], pos[faces[f, (k + 1) % 3]]
            shared = np.sign(a) * (np.sign(a) == np.sign(b))          # the axes on which both ends sit on the same side
            want = shared if shared.astype(bool).sum() == 2 else 2 * unit[f]   # a box edge: two axes; a face diagonal: its face twice
            assert np.array_equal(en[f, k], want), (f, k, en[f, k], want)


@pytest.mark.parametrize("name", CLOSED)
def test_sign_gate_the_restatement_agrees_with_the_solid_angle(name):
    c, e = sc.case(name), evaluated(name)
    margin = margin_of(c)
    fin, group = e["finite"], c["group"]
    wrong = fin & ((e["got"]["sign"] < 0) != e["inside"])
    worst = float(e["dist"][wrong].max()) if wrong.any() else 0.0
    left_out = fin & (e["dist"] <= margin)
    print(f"{name}: extent {c['extent']:.4g}, margin {margin:.3g}; {int(wrong.sum())} of {int(fin.sum())} finite queries disagree, the farthest "
          f"{worst:.3g} ({worst / c['extent']:.3g} of the extent) from the surface; left out by the margin: "
          f"{int((left_out & (group == sc.RANDOM)).sum())} random, {int((left_out & (group == sc.DIRECTED)).sum())} directed")
    assert e["report"][6] == 1
    assert 4 * worst <= margin                                       # the margin is four times what was measured, and no less than 16 ulps
    assert not (wrong & ~left_out).any()                             # the gate
    n_random = int((group == sc.RANDOM).sum())
    assert (left_out & (group == sc.RANDOM)).sum() <= 0.01 * n_random
    assert not (left_out & (group == sc.DIRECTED)).any()
    # the directed queries are where they were meant to be, by the reference alone: on the intended side, about a step away
    d = group == sc.DIRECTED
    assert np.array_equal(e["inside"][d], c["directed_inside"])
    assert e["dist"][d].min() > 0.05 * sc.DIRECTED_STEP * c["extent"] and e["dist"][d].max() <= 1.001 * sc.DIRECTED_STEP * c["extent"]
    answered = e["got"]["face"] >= 0                                 # not: the points that are not finite, and 1e30, whose dd overflows
    assert not answered[~fin].any() and answered[fin & (np.abs(c["points"]).max(axis=1) < 1e6)].all()
    assert (e["got"]["sign"][~answered] == 0).all() and (e["got"]["feature"][~answered] == -1).all()
    assert set(np.unique(e["got"]["sign"][answered]).tolist()) <= {-1, 1}


def test_the_margin_on_record():
    worst = 0.0
    for name in CLOSED:
        c, e = sc.case(name), evaluated(name)
        wrong = e["finite"] & ((e["got"]["sign"] < 0) != e["inside"])
        if wrong.any():
            worst = max(worst, float((e["dist"][wrong] / c["extent"]).max()))
    print(f"largest distance of a disagreeing query: {worst:.3g} of the extent; margin {MARGIN_ULPS} ulps = {MARGIN_ULPS * EPS / 2:.3g}..{MARGIN_ULPS * EPS:.3g} of it")
    record("sign_gate", dict(cases=len(CLOSED), queries=int(sum(len(sc.case(n)["points"]) for n in CLOSED)),
                             largest_disagreeing_distance_over_extent=worst, margin_ulps=MARGIN_ULPS, margin_over_extent=MARGIN_ULPS * EPS))
    assert 4 * worst <= MARGIN_ULPS * EPS / 2


def test_every_feature_is_met():
    met = set()
    for name in CLOSED:
        met |= set(np.unique(evaluated(name)["got"]["feature"]).tolist())
    assert met == {-1, 0, 1, 2, 3, 4, 5, 6}


# a wrong variant, the case on which it shows, and the groups of queries among which it must turn a sign the gate covers
WRONG = (("uniform", "fan spike", (sc.PROBE,)), ("face_normal", "tetrahedron", (sc.RANDOM, sc.DIRECTED)),
         ("q_minus_p", "box", (sc.RANDOM, sc.DIRECTED)), ("en_order", "fan spike", (sc.RANDOM, sc.DIRECTED, sc.PROBE)),
         ("unwelded", "tetrahedron OBJ style", (sc.RANDOM, sc.DIRECTED)))
# (On a box every one of these but q_minus_p is harmless: its face normals are orthogonal, so any non-negative combination of the normals
# around a vertex or an edge has the right sign over that feature's whole region.  Hence the tetrahedron and the spike.)


@pytest.mark.parametrize("wrong,name,groups", WRONG)
def test_wrong_variants_turn_a_sign_the_gate_covers(wrong, name, groups):
    c, e = sc.case(name), evaluated(name)
    if wrong in ("uniform", "unwelded"):
        vn, en, _ = sm.pseudonormals(c["pos"], c["faces"], wrong=wrong)
        bad = sm.signed_distance(c["pos"], c["faces"], vn, en, c["points"])
    else:
        bad = sm.signed_distance(c["pos"], c["faces"], e["vn"], e["en"], c["points"], wrong=wrong)
    covered = e["finite"] & (e["dist"] > margin_of(c)) & np.isin(c["group"], groups)
    turned = covered & (bad["sign"] != e["got"]["sign"])
    print(f"{wrong} on {name}: {int(turned.sum())} of {int(covered.sum())} covered queries change sign")
    assert turned.any()
    assert np.array_equal(e["got"]["sign"][turned] < 0, e["inside"][turned])     # and there the definition is right
    for k in ("dist2", "face", "closest", "feature"):
        assert np.array_equal(bad[k], e["got"][k], equal_nan=True)                # a wrong sign leaves the distance alone


def test_points_on_the_surface_are_outside_and_le_is_told_apart():
    turned = 0
    for name in CLOSED:
        c, e = sc.case(name), evaluated(name)
        on = np.nonzero(c["group"] == sc.ON)[0]
        assert len(on) == 3
        vertex = on[0]                                                # the float32 vertex itself: p - q = 0 exactly, s = +0
        assert e["got"]["dist2"][vertex] == 0 and e["got"]["s"][vertex] == 0 and e["got"]["sign"][vertex] == 1
        le = sm.signed_distance(c["pos"], c["faces"], e["vn"], e["en"], c["points"][on], wrong="le")
        assert le["sign"][0] == -1
        turned += int((le["sign"] != e["got"]["sign"][on]).sum())
    assert turned >= len(CLOSED)


def test_crossed_boxes_are_the_documented_counterexample():
    """inside the first box, beside the part of the second box's surface that lies in it: the nearest face is the second box's, seen
    from its outside.  The winding number (2 in the crossing, 1 in either arm) says inside; the sign says outside."""
    pos, faces = sc.crossed_boxes()
    pos = pos.astype(f32)
    vn, en, report = sm.pseudonormals(pos, faces)
    assert report[6] == 1
    p = np.array([[0.25, 0.0, 0.0], [0.0, 0.0, 0.0]], f32)           # in the first arm, 0.05 from the second box; in the crossing
    got = sm.signed_distance(pos, faces, vn, en, p)
    assert np.allclose(sm.winding_number(pos, faces, p), [1.0, 2.0], atol=1e-9)
    assert got["sign"].tolist() == [1, -1] and got["face"][0] >= 12 and abs(float(got["dist2"][0]) - 0.05 ** 2) < 1e-6


def _mean_gap_outside(h, delta, n=64):
    """the mean distance of the surface of a cube of half side h to the cube of half side h - delta inside it: over a face the
    distance is sqrt(delta^2 + ey^2 + ez^2) with ey, ez how far the point is beyond the smaller face's edges (Gauss-Legendre over the
    rim strips and the corners; delta over the middle)"""
    x, w = np.polynomial.legendre.leggauss(n)
    x, w = (x + 1) / 2 * delta, w / 2 * delta
    strip = float((w * np.sqrt(delta ** 2 + x ** 2)).sum())                                   # integral over one strip's width
    corner = float((w[:, None] * w[None, :] * np.sqrt(delta ** 2 + x[:, None] ** 2 + x[None, :] ** 2)).sum())
    inner = 2 * (h - delta)
    return (inner * inner * delta + 4 * inner * strip + 4 * corner) / (2 * h) ** 2


def test_signed_bias_of_a_box_against_its_scaled_copies():
    pos, faces = sc.box()
    n, h = 20000, 0.5
    a = (pos.astype(f32), faces)
    grown = sm.signed_bias(a, ((pos * 1.01).astype(f32), faces), n)
    shrunk = sm.signed_bias(a, ((pos * 0.99).astype(f32), faces), n)
    delta = 0.01 * h
    # a inside the copy grown by 1 %: every sample is delta under the nearest face.  float32: coordinates of 0.5, a few operations
    assert grown[1] == 1.0 and abs(grown[0] + delta) <= 8 * EPS and abs(grown[3] + delta) <= 8 * EPS
    # a around the copy shrunk by 1 %: outside everywhere.  Sampling: the distance differs from delta only over the rim strips, a share
    # p of the area, by at most (sqrt 3 - 1) delta; the stratified samples err by no more than independent ones do, 3 sigma
    want = _mean_gap_outside(h, delta)
    p = 1 - (2 * (h - delta)) ** 2 / (2 * h) ** 2
    tol = (math.sqrt(3) - 1) * delta * 3 * math.sqrt(p * (1 - p) / n) + 8 * EPS
    print(f"shrunk copy: mean {shrunk[0]:.6g}, closed form {want:.6g}, tolerance {tol:.2g}; grown copy: mean {grown[0]:.6g}")
    assert shrunk[1] == 0.0 and abs(shrunk[0] - want) <= tol and shrunk[0] > delta
    assert shrunk[2] >= delta - 8 * EPS and shrunk[4] <= math.sqrt(3) * delta + 8 * EPS


SHIFT_YZ = (0.3, 0.2)


@pytest.mark.parametrize("overlap", (0.1, 0.25, 0.0, -0.1))
def test_penetration_of_two_unit_boxes(overlap):
    """unit cube a moved by (1 - overlap, 0.3, 0.2) into unit cube b.  Inside b are a's face x = -0.5 where y' < 0.5 and z' < 0.5
    (0.7 x 0.8 of it) and strips of width `overlap` of its faces y = -0.5 (0.8 long) and z = -0.5 (0.7 long); the deepest points are
    on the first, `overlap` under b's face x = 0.5."""
    Q = 2048
    pos, faces, pts, tf = sc.box_pair(overlap, Q)
    tf[1, 3], tf[2, 3] = SHIFT_YZ
    vn, en, report = sm.pseudonormals(pos, faces)
    got = sm.penetration(pos, faces, vn, en, pts, tf[None])
    share, depth = got["inside"][0] / Q, math.sqrt(float(got["depth2"][0]))
    ov = max(overlap, 0.0)
    want = (0.56 + 1.5 * ov) / 6 if overlap > 0 else 0.0
    tol = 3 * math.sqrt(max(want * (1 - want), 1e-12) / Q)
    print(f"overlap {overlap}: inside {share:.4f} (closed form {want:.4f} +- {tol:.4f}), depth {depth:.7f}, deepest {int(got['deepest'][0])}")
    assert abs(depth - ov) <= 8 * EPS                                 # coordinates up to 1: a translation, a difference, a square, a root
    if overlap > 0:
        assert abs(share - want) <= tol
        j = int(got["deepest"][0])
        assert got["sign"][0, j] == -1 and got["dist2"][0, j] == got["depth2"][0] == got["dist2"][0][got["sign"][0] < 0].max()
        assert j == np.nonzero((got["sign"][0] < 0) & (got["dist2"][0] == got["depth2"][0]))[0][0]
    elif overlap < 0:
        assert got["inside"][0] == 0 and got["deepest"][0] == -1 and got["depth2"][0] == 0
    else:                                                             # touching: a sample is inside only by the rounding of its own coordinates
        assert share <= 0.56 / 6 + tol


def test_penetration_rows_that_are_not_finite_are_empty():
    pos, faces, pts, tf = sc.box_pair(0.25, 64)
    vn, en, _ = sm.pseudonormals(pos, faces)
    tfs = np.stack([tf] * 5)
    tfs[1, 0, 3] = np.nan
    tfs[2, 1, 1] = np.inf
    tfs[3, :3, :3] *= f32(3e38)                                       # overflows in the products
    tfs[4, 3, :] = np.nan                                             # row 3 is never read
    got = sm.penetration(pos, faces, vn, en, pts, tfs)
    assert got["inside"][0] > 0 and got["inside"][4] == got["inside"][0] and got["deepest"][4] == got["deepest"][0]
    for t in (1, 2, 3):
        assert got["inside"][t] == 0 and got["depth2"][t] == 0 and got["deepest"][t] == -1
        assert (got["sign"][t] == 0).all() and np.isposinf(got["dist2"][t]).all()


def test_signed_stats():
    from foundationpose_amd import ops
    s = ops.SignedStats.of([-1.0, -1.0, 1.0, 3.0])
    assert s.mean == 0.5 and s.inside == 0.5 and s.p50 == 0.0 and s.p5 == -1.0 and abs(s.p95 - 2.7) < 1e-12
    assert all(math.isnan(x) for x in ops.SignedStats.of([]))


def test_refusals_that_need_no_device():
    from foundationpose_amd import _lib, ops
    pos, faces = sc.box()
    t = dict(pos=torch.from_numpy(pos.astype(f32)), faces=torch.from_numpy(faces.astype(np.int32)))
    pts = torch.zeros((4, 3))
    tfs = torch.eye(4)[None]
    opened = dict(pos=t["pos"], faces=t["faces"][2:].contiguous())
    for call in (lambda m, **kw: ops.mesh_signed_distance(pts, m, **kw), lambda m, **kw: ops.mesh_penetration(pts, tfs, m, **kw)):
        with pytest.raises(_lib.FpAmdError, match="not closed.*boundary=4"):
            call(dict(opened))
        with pytest.raises(_lib.FpAmdError, match="no CPU path"):     # allowed through: the next refusal is the device's
            call(dict(opened), allow_open=True)
        with pytest.raises(_lib.FpAmdError, match="no CPU path"):
            call(dict(t))
        with pytest.raises(ValueError, match="unknown name"):
            call(dict(t), want=("sign", "winding"))
        with pytest.raises(_lib.FpAmdError, match="tables must be"):
            call(dict(t), tables=(1, 2))
        with pytest.raises(_lib.FpAmdError, match="another mesh"):
            call(dict(t), tables=ops.mesh_pseudonormals(dict(opened)), allow_open=True)
        with pytest.raises(_lib.FpAmdError, match="not both"):
            call(dict(t), pos=t["pos"])
        with pytest.raises(_lib.FpAmdError, match="out has 'volume'"):
            call(dict(t), out=dict(volume=pts))
    with pytest.raises(_lib.FpAmdError, match=r"points must be \(n,3\)"):
        ops.mesh_signed_distance(torch.zeros(4, 2), dict(t))
    with pytest.raises(_lib.FpAmdError, match=r"tfs must be \(T,4,4\)"):
        ops.mesh_penetration(pts, torch.eye(4), dict(t))
    with pytest.raises(_lib.FpAmdError, match="tfs must be a tensor"):
        ops.mesh_penetration(pts, None, dict(t))
    with pytest.raises(_lib.FpAmdError, match="faces must be torch.int32"):
        ops.mesh_pseudonormals(pos=t["pos"], faces=t["faces"].long())
    with pytest.raises(_lib.FpAmdError, match="no mesh"):
        ops.mesh_pseudonormals()
    kept = dict(t)
    first = ops.mesh_pseudonormals(kept)
    assert kept["pseudonormals"] is first and ops.mesh_pseudonormals(kept) is first and first.closed and "edges=18" in first.describe()


def test_c_entry_points_report_argument_errors_without_a_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    assert lib.fp_version() == 234
    p = C.c_void_p(4096)
    assert lib.fp_mesh_signed_distance_workspace_bytes(0) == 0 == lib.fp_mesh_signed_distance_workspace_bytes(-4)
    assert lib.fp_mesh_signed_distance_workspace_bytes(257) == 8 * 257
    wsb = lib.fp_mesh_penetration_workspace_bytes
    assert wsb(0, 5) == 0 == wsb(5, 0) == wsb(-3, 5) == wsb(5, -1) == wsb(1 << 20, (1 << 10) + 1) and wsb(300, 128) == 8 * 300 * 128

    def sd(pos=p, Nv=3, faces=p, F=1, vn=p, en=p, points=p, Q=4, dist2=p, ws=p, ws_bytes=32):
        return lib.fp_mesh_signed_distance(pos, Nv, faces, F, vn, en, points, Q, dist2, None, None, None, None, ws, ws_bytes, None)

    for kw, word in ((dict(Q=-1), b"Q=-1"), (dict(Q=(1 << 30) + 1), b"Q="), (dict(F=-1), b"F=-1"), (dict(Nv=-1), b"Nv=-1"),
                     (dict(points=None), b"NULL points or dist2"), (dict(dist2=None), b"NULL points or dist2"), (dict(faces=None), b"faces is NULL"),
                     (dict(pos=None), b"pos is NULL"), (dict(vn=None), b"vn is NULL"), (dict(en=None), b"en is NULL"), (dict(ws=None), b"workspace"),
                     (dict(ws_bytes=31), b"workspace"), (dict(ws=C.c_void_p(4100)), b"8-byte aligned")):
        assert sd(**kw) == -1, kw
        msg = lib.fp_last_error()
        assert msg.startswith(b"fp_mesh_signed_distance") and word in msg, (kw, msg)
    assert sd(Q=0, points=None, dist2=None, ws=None, ws_bytes=0) == 0

    def pn(pos=p, Nv=3, faces=p, F=1, vn=p, en=p, points=p, Q=4, tfs=p, T=2, inside=p, ws=p, ws_bytes=64):
        return lib.fp_mesh_penetration(pos, Nv, faces, F, vn, en, points, Q, tfs, T, inside, None, None, None, None, ws, ws_bytes, None)

    for kw, word in ((dict(Q=-1), b"Q=-1"), (dict(T=-1), b"T=-1"), (dict(T=1 << 20, Q=(1 << 10) + 1), b"above 2^30"), (dict(F=-1), b"F=-1"),
                     (dict(Nv=-1), b"Nv=-1"), (dict(inside=None), b"NULL inside"), (dict(points=None), b"NULL points or tfs"),
                     (dict(tfs=None), b"NULL points or tfs"), (dict(faces=None), b"faces is NULL"), (dict(pos=None), b"pos is NULL"),
                     (dict(vn=None), b"vn is NULL"), (dict(en=None), b"en is NULL"), (dict(ws=None), b"workspace"), (dict(ws_bytes=63), b"workspace"),
                     (dict(ws=C.c_void_p(4100)), b"8-byte aligned")):
        assert pn(**kw) == -1, kw
        msg = lib.fp_last_error()
        assert msg.startswith(b"fp_mesh_penetration") and word in msg, (kw, msg)
    assert pn(T=0, points=None, tfs=None, inside=None, ws=None, ws_bytes=0) == 0

    rep = (C.c_int32 * 8)()
    for args, word in (((p, -1, p, 1, p, p, rep), b"Nv=-1"), ((p, 3, p, -1, p, p, rep), b"F=-1"), ((p, 3, p, 1, p, p, None), b"NULL report"),
                       ((None, 3, p, 1, p, p, rep), b"NULL pos or vn"), ((p, 3, p, 1, None, p, rep), b"NULL pos or vn"),
                       ((p, 3, None, 1, p, p, rep), b"NULL faces or en"), ((p, 3, p, 1, p, None, rep), b"NULL faces or en")):
        assert lib.fp_mesh_pseudonormals(*args) == -1, args
        msg = lib.fp_last_error()
        assert msg.startswith(b"fp_mesh_pseudonormals") and word in msg, msg
    assert lib.fp_mesh_pseudonormals(None, 0, None, 0, None, None, rep) == 0 and list(rep) == [0] * 8
