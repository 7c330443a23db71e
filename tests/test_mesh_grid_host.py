"""CPU: the uniform grid of include/fp_amd.h through its numpy restatement (tests/mesh_grid_model.py) on the cases and grids of
tests/mesh_grid_cases.py.  The model under every grid is bit-equal to the brute-force restatement (mesh_distance_model) in dist2 and
closest and equal in face; the header's precondition (no computed closest point more than pad / 4 outside its triangle's box) holds
for every case and grid used; each deliberately wrong variant changes a named case; the share of the pairs that are tested at all is
gated; the shell form of the walk equals the literal walk over the tables; and the wrappers' and the C entry points' refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_distance_model as mm
import mesh_grid_cases as gcs
import mesh_grid_model as mg

f32 = np.float32
NAMES = list(gcs.cases())
# pairs tested / (Q * F) of the model on lattice_box (4 332 faces, 1 500 samples of its own surface) under the default grid: 0.0076959
# as measured with the model (33.3 pair tests a query); the gate is twice that.  The device walks the same cells.
PRUNING_MEASURED = 0.0076959
PRUNING_GATE = 2 * PRUNING_MEASURED


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype.kind == "i" else a.view(np.uint32)


def _run(name, kind, wrong=None):
    c, s = gcs.cases()[name], gcs.setup(name, kind)
    got, tab = mg.mesh_grid_point_distance(c["pos"], c["faces"], s["points"], s["grid"], wrong=wrong, dd=s["dd"])
    return got, tab, s


def _differs(got, ref):
    return int((_bits(got[0]) != _bits(ref[0])).sum() + (got[1] != ref[1]).sum())


# ------------------------------------------------------------------ 1. the same bits as brute force, and the precondition
@pytest.mark.parametrize("name", NAMES, ids=[n.replace(" ", "_").replace(":", "") for n in NAMES])
def test_the_model_equals_the_brute_force_restatement_under_every_grid(name):
    for kind in gcs.GRIDS:
        (dist2, face, closest, pairs), tab, s = _run(name, kind)
        ref = s["ref"]
        assert np.array_equal(_bits(dist2), _bits(ref[0])), (name, kind, "dist2")
        assert np.array_equal(face, ref[1]) and face.dtype == ref[1].dtype, (name, kind, "face")
        assert np.array_equal(_bits(closest), _bits(ref[2])), (name, kind, "closest")
        # the precondition of the header, from the brute-force pair tests alone
        worst = float(s["exc"].max()) if s["exc"].size else 0.0
        assert worst <= float(s["grid"].pad) / 4, (name, kind, worst, float(s["grid"].pad))
        assert int(tab["cell_start"][-1]) == tab["n_entries"] == len(tab["entries"])
        Q, F = s["dd"].shape
        assert pairs.max(initial=0) <= tab["n_entries"] + tab["n_overflow"] and (Q == 0 or F == 0 or pairs.sum() <= Q * max(tab["n_entries"], F))


def test_the_grids_are_what_their_names_say():
    over = stored_outside = on_planes = 0
    for name in NAMES:
        c = gcs.cases()[name]
        g = {k: gcs.grid_of(c["pos"], c["faces"], k) for k in gcs.GRIDS}
        assert g["1x1x1"].n.tolist() == [1, 1, 1] and g["2x3x1"].n.tolist() == [2, 3, 1]
        assert all(1 <= x.ncells <= 1 << 21 for x in g.values())
        over += mg.tables(g["tiny cells"], c["pos"], c["faces"])["n_overflow"]
        cls, i0, i1 = mg.classify(g["half box"], c["pos"], c["faces"])
        cls2, _, _ = mg.classify(g["half box"], c["pos"], c["faces"], wrong="drop_outside")
        stored_outside += int(((cls == mg.STORED) & (cls2 == mg.DROPPED)).sum())
        # under "aligned" the plane queries sit exactly on planes, and planes pass through vertices of the unit cases
        s = gcs.queries(name, "aligned")
        ga = s["grid"]
        for p in s["points"][len(s["points"]) - s["extra"]:]:
            assert any(p[k] == mg.plane(ga, k, int(mg.cell(ga, k, p[k]))) or p[k] == mg.plane(ga, k, int(mg.cell(ga, k, p[k])) + 1)
                       for k in range(3)), (name, p)
        if name in ("regions x1", "ties x1"):
            v = c["pos"][np.isfinite(c["pos"]).all(axis=1)]
            on_planes += sum(int((v[:, k] == mg.plane(ga, k, mg.cell(ga, k, v[:, k]))).sum()) for k in range(3))
    assert over > 500 and stored_outside > 1000 and on_planes >= 6
    box = gcs.cases()["signed: box"]                                      # 12 faces as large as the box
    tab = mg.tables(gcs.grid_of(box["pos"], box["faces"], "tiny cells"), box["pos"], box["faces"])
    assert tab["n_overflow"] == 12 and tab["n_entries"] == 0
    sk = gcs.cases()["skipped and degenerate"]
    cls, _, _ = mg.classify(gcs.grid_of(sk["pos"], sk["faces"], "default"), sk["pos"], sk["faces"])
    assert cls.tolist() == [2, 2, 2, 2, 0, 0, 0, 1, 1, 2, 2, 2, 2]      # an index outside: dropped; a NaN or infinite vertex: overflow


def test_the_shell_form_equals_the_literal_walk_over_the_tables():
    for name in ("soup F=257 Q=64", "ties x1", "skipped and degenerate", "box", "regions x50"):
        c = gcs.cases()[name]
        for kind in gcs.GRIDS:
            s = gcs.setup(name, kind)
            if s["grid"].ncells > 4096:
                continue
            pts, dd = s["points"][:40], s["dd"][:40]
            tab = mg.tables(s["grid"], c["pos"], c["faces"])
            best, face, pairs, _ = mg.walk(s["grid"], tab, dd, pts)
            b2, f2, p2 = mg.walk_cells(s["grid"], tab, dd, pts)
            assert np.array_equal(_bits(best), _bits(b2)) and np.array_equal(face, f2) and np.array_equal(pairs, p2), (name, kind)


# ------------------------------------------------------------------ 2. the wrong variants
def test_no_pad_changes_the_triangle_one_ulp_below_a_plane():
    s = gcs.ulp_plane()
    g = s["grid"]
    assert s["below"] < s["plane"] and int(mg.cell(g, 0, s["below"])) == 9 and int(mg.cell(g, 0, s["points"][0, 0])) == 8
    ref = mm.mesh_point_distance(s["pos"], s["faces"], s["points"])
    got, _ = mg.mesh_grid_point_distance(s["pos"], s["faces"], s["points"], g)
    bad, _ = mg.mesh_grid_point_distance(s["pos"], s["faces"], s["points"], g, wrong="no_pad")
    assert ref[1].tolist() == [1] and got[1].tolist() == [1] and np.array_equal(_bits(got[0]), _bits(ref[0]))
    assert bad[1].tolist() == [0] and bad[0][0] > ref[0][0]
    dd, exc = mg.pair_matrix(s["pos"], s["faces"], s["points"])
    assert float(exc.max()) <= float(g.pad) / 4


@pytest.mark.parametrize("wrong, name, kind", [("plane_too_far", "soup F=3000 Q=1000", "default"), ("plane_too_far", "box", "default"),
                                               ("first_met", "ties x1", "default"), ("first_met", "ties x50", "1x1x1"),
                                               ("no_overflow", "signed: box", "tiny cells"), ("no_overflow", "signed: tetrahedron", "tiny cells"),
                                               ("drop_outside", "box", "half box"), ("drop_outside", "soup F=1023 Q=1000", "half box")])
def test_wrong_variants_change_a_named_case(wrong, name, kind):
    right, _, s = _run(name, kind)
    assert _differs(right, s["ref"]) == 0
    got, _, _ = _run(name, kind, wrong)
    assert _differs(got, s["ref"]) > 0, (wrong, name, kind)


def test_the_plane_at_c_plus_r_is_conservative_and_shows_in_the_pair_count():
    """with the rule "m > 0" a plane behind the query never stops the walk: this variant can only test more pairs (ten times as many
    here), so the case it changes is the pruning figure, not an answer"""
    right, _, s = _run("soup F=3000 Q=1000", "default")
    got, _, _ = _run("soup F=3000 Q=1000", "default", "plane_c_plus_r")
    assert _differs(got, s["ref"]) == 0 and got[3].sum() > 3 * right[3].sum()


def test_overflow_triangles_with_an_infinite_vertex_can_answer():
    """the reason the overflow list exists: pairs of the skipped case whose triangle has an infinite vertex and whose dd is finite"""
    c = gcs.cases()["skipped and degenerate"]
    dd, _ = gcs.pairs_of("skipped and degenerate")
    tri = mm.face_vertices(c["pos"], c["faces"])
    inf_vertex = np.isinf(tri).any(axis=(1, 2))
    assert inf_vertex.sum() == 1 and int(np.isfinite(dd[:, inf_vertex]).sum()) == 3


# ------------------------------------------------------------------ 3. pruning
def test_pruning_on_a_closed_mesh_of_4332_faces():
    c = gcs.lattice_box()
    assert len(c["faces"]) >= 4096
    g = gcs.grid_of(c["pos"], c["faces"], "default")
    (dist2, face, closest, pairs), tab = mg.mesh_grid_point_distance(c["pos"], c["faces"], c["points"], g)
    ref = mm.mesh_point_distance(c["pos"], c["faces"], c["points"])
    assert np.array_equal(_bits(dist2), _bits(ref[0])) and np.array_equal(face, ref[1]) and np.array_equal(_bits(closest), _bits(ref[2]))
    share = pairs.sum() / (len(c["points"]) * len(c["faces"]))
    print(f"pairs tested / (Q F) = {share:.7f} ({pairs.mean():.1f} a query; measured {PRUNING_MEASURED}, gate {PRUNING_GATE})")
    assert share <= PRUNING_GATE


# ------------------------------------------------------------------ 4. the shape rule, refusals
def test_the_default_shape_rule():
    from foundationpose_amd import _lib, ops
    c = gcs.cases()["box"]
    lo, h, n, pad = ops.mesh_grid_shape(c["pos"], c["faces"])
    tri = c["pos"][c["faces"]].astype(np.float64)
    mean_edge = (tri.max(axis=1) - tri.min(axis=1)).max(axis=1).mean()
    assert h == f32(ops.MESH_GRID_CELL_OVER_FACE * mean_edge) and np.array_equal(lo, c["pos"].min(axis=0))
    ext = c["pos"].max(axis=0).astype(np.float64) - lo
    assert n.tolist() == (np.floor(ext / float(h)) + 1).astype(int).tolist()
    M = f32(max(np.abs(lo).max(), np.abs(lo + n.astype(f32) * h).max()))
    assert pad == f32(2.0 ** -16) * M
    assert int(n.prod()) > 8
    small = ops.mesh_grid_shape(c["pos"], c["faces"], max_cells=8)
    assert int(small[2].prod()) <= 8 and small[1] > h
    assert ops.mesh_grid_shape(np.zeros((0, 3), f32), np.zeros((0, 3), np.int32))[2].tolist() == [1, 1, 1]
    nanmesh = ops.mesh_grid_shape(np.full((3, 3), np.nan, f32), [[0, 1, 2]])
    assert nanmesh[2].tolist() == [1, 1, 1] and nanmesh[1] == 1
    for kw, word in ((dict(cell=0.0), "cell="), (dict(cell=float("nan")), "cell="), (dict(cell=1e-7), "above max_cells"),
                     (dict(pad=0.0), "below 2\\^-20"), (dict(pad=float("inf")), "below 2\\^-20"), (dict(max_cells=0), "max_cells"),
                     (dict(max_cells=(1 << 21) + 1), "max_cells"), (dict(lo=(0, 0, 0)), "together"),
                     (dict(lo=(0, 0, 0), n=(0, 1, 1), cell=1.0), "1 <= cells"), (dict(lo=(0, 0, 0), n=(1 << 11, 1 << 11, 1), cell=1.0), "1 <= cells"),
                     (dict(lo=(np.inf, 0, 0), n=(1, 1, 1), cell=1.0), "finite")):
        with pytest.raises(_lib.FpAmdError, match=word):
            ops.mesh_grid_shape(c["pos"], c["faces"], **kw)


def test_refusals_that_need_no_device():
    from foundationpose_amd import _lib, ops, reconstruct
    c = gcs.cases()["box"]
    t = dict(pos=torch.from_numpy(c["pos"]), faces=torch.from_numpy(c["faces"]))
    with pytest.raises(_lib.FpAmdError, match="no CPU path"):
        ops.mesh_grid_build(t)
    with pytest.raises(_lib.FpAmdError, match="no mesh"):
        ops.mesh_grid_build()
    with pytest.raises(_lib.FpAmdError, match=r"faces must be \(n,3\)"):
        ops.mesh_grid_build(pos=t["pos"], faces=t["faces"].reshape(-1))
    with pytest.raises(_lib.FpAmdError, match="not both"):
        ops.mesh_grid_build(t, pos=t["pos"])
    with pytest.raises(ValueError, match="accel must be"):
        reconstruct._accel_grid("bvh", t, "compare_meshes")
    assert reconstruct._accel_grid(None, t, "compare_meshes") is None


def test_c_entry_points_report_argument_errors_without_a_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(4096)

    def grid(**kw):
        g = _lib.MeshGridStruct()
        g.lo[:] = kw.pop("lo", (0.0, 0.0, 0.0))
        g.n[:] = kw.pop("n", (4, 4, 4))
        g.h, g.pad = kw.pop("h", 1.0), kw.pop("pad", 1e-3)
        g.cell_start, g.entries, g.overflow = kw.pop("cell_start", 4096), kw.pop("entries", 4096), kw.pop("overflow", 4096)
        g.n_entries, g.n_overflow = kw.pop("n_entries", 5), kw.pop("n_overflow", 2)
        assert not kw
        return g

    bad_grids = ((dict(h=0.0), b"h=0"), (dict(h=-1.0), b"h=-1"), (dict(h=float("nan")), b"non-finite"), (dict(h=float("inf")), b"non-finite"),
                 (dict(lo=(float("inf"), 0, 0)), b"non-finite"), (dict(pad=float("nan")), b"non-finite"), (dict(n=(0, 4, 4)), b"at least 1"),
                 (dict(n=(129, 128, 128)), b"more than 2^21"), (dict(n=(1 << 30, 1 << 30, 4)), b"more than 2^21"), (dict(pad=0.0), b"below 2^-20"),
                 (dict(pad=3e-6), b"below 2^-20"), (dict(lo=(3.4e38, 0, 0), h=1e30, n=(1 << 21, 1, 1), pad=1e38), b"far corner"),
                 (dict(cell_start=None), b"NULL cell_start"), (dict(entries=None), b"entries is NULL"), (dict(overflow=None), b"overflow is NULL"),
                 (dict(n_entries=-1), b"negative"), (dict(n_overflow=-1), b"negative"))
    calls = {
        "fp_mesh_grid_count": lambda g, **kw: lib.fp_mesh_grid_count(kw.get("pos", p), kw.get("Nv", 3), kw.get("faces", p), kw.get("F", 1),
                                                                     g, kw.get("header", p), None),
        "fp_mesh_grid_fill": lambda g, **kw: lib.fp_mesh_grid_fill(kw.get("pos", p), kw.get("Nv", 3), kw.get("faces", p), kw.get("F", 1), g,
                                                                   kw.get("header", p), kw.get("ws", p), kw.get("ws_bytes", 4 * 65), None),
        "fp_mesh_grid_point_distance": lambda g, **kw: lib.fp_mesh_grid_point_distance(
            kw.get("pos", p), kw.get("Nv", 3), kw.get("faces", p), kw.get("F", 1), g, kw.get("points", p), kw.get("Q", 4), kw.get("dist2", p),
            None, None, kw.get("ws", p), kw.get("ws_bytes", 32), None),
        "fp_mesh_grid_signed_distance": lambda g, **kw: lib.fp_mesh_grid_signed_distance(
            kw.get("pos", p), kw.get("Nv", 3), kw.get("faces", p), kw.get("F", 1), g, kw.get("vn", p), kw.get("en", p), kw.get("points", p),
            kw.get("Q", 4), kw.get("dist2", p), None, None, None, None, kw.get("ws", p), kw.get("ws_bytes", 32), None)}
    for name, call in calls.items():
        for kw, word in bad_grids:
            if name == "fp_mesh_grid_count" and ("entries" in kw or "overflow" in kw or "n_entries" in kw or "n_overflow" in kw):
                continue                                     # count does not read the lists
            assert call(C.byref(grid(**kw))) == -1, (name, kw)
            msg = lib.fp_last_error()
            assert msg.startswith(name.encode()) and word in msg, (name, kw, msg)
        assert call(None) == -1 and b"NULL grid" in lib.fp_last_error()
        g = C.byref(grid())
        for kw, word in ((dict(F=-1), b"F=-1"), (dict(Nv=-1), b"Nv=-1"), (dict(faces=None), b"faces is NULL"), (dict(pos=None), b"pos is NULL")):
            assert call(g, **kw) == -1, (name, kw)
            msg = lib.fp_last_error()
            assert msg.startswith(name.encode()) and word in msg, (name, kw, msg)
    g = C.byref(grid())
    for name in ("fp_mesh_grid_count", "fp_mesh_grid_fill"):
        assert calls[name](g, header=None) == -1 and b"NULL header" in lib.fp_last_error()
    for kw in (dict(ws=None), dict(ws_bytes=4 * 65 - 1), dict(ws=C.c_void_p(4098))):
        assert calls["fp_mesh_grid_fill"](g, **kw) == -1 and b"workspace" in lib.fp_last_error(), kw
    assert lib.fp_mesh_grid_fill_workspace_bytes(g) == 4 * 65 and lib.fp_mesh_grid_fill_workspace_bytes(None) == 0
    assert lib.fp_mesh_grid_fill_workspace_bytes(C.byref(grid(n=(129, 128, 128)))) == 0
    for name in ("fp_mesh_grid_point_distance", "fp_mesh_grid_signed_distance"):
        for kw, word in ((dict(Q=-1), b"Q=-1"), (dict(Q=(1 << 30) + 1), b"Q="), (dict(points=None), b"NULL points or dist2"),
                         (dict(dist2=None), b"NULL points or dist2"), (dict(ws=None), b"workspace"), (dict(ws_bytes=31), b"workspace"),
                         (dict(ws=C.c_void_p(4100)), b"8-byte aligned")):
            assert calls[name](g, **kw) == -1, (name, kw)
            msg = lib.fp_last_error()
            assert msg.startswith(name.encode()) and word in msg, (name, kw, msg)
        assert calls[name](g, Q=0, points=None, dist2=None, ws=None, ws_bytes=0) == 0
    for kw, word in ((dict(vn=None), b"vn is NULL"), (dict(en=None), b"en is NULL")):
        assert calls["fp_mesh_grid_signed_distance"](g, **kw) == -1 and word in lib.fp_last_error()
