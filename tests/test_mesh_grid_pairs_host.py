"""Host: what the grid forms of the batched transform queries (fp_mesh_grid_transform_residuals, fp_mesh_grid_icp_step,
fp_mesh_grid_penetration) promise without a device.  Their argument errors, each beginning with the new entry point's name: a NULL
grid, every refused grid and every error of the parent.  The claim that the stop rule needs nothing new for a transformed point:
tests/mesh_grid_model.py's walk on the float32 p' of six named pair cases, under every grid they run under, returns the dist2 (and,
for the ICP cases, the face) of the references that the brute-force tests hold the kernels to -- this passes without the grid
forms, it pins the model the GPU tests lean on.  And the counts of the (case, grid) pairs that tests/mesh_grid_pair_cases.py leaves
out."""
import ctypes as C

import numpy as np
import pytest

import mesh_grid_cases as gcs
import mesh_grid_model as mg
import mesh_grid_pair_cases as pc
import mesh_icp_cases as ic
import mesh_symmetry_cases as sc
import mesh_symmetry_model as sm

f32 = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype.kind == "i" else a.view(np.uint32)


# ------------------------------------------------------------------ 1. argument errors
def test_c_entry_points_report_argument_errors_without_a_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    p, q = C.c_void_p(4096), C.c_void_p(8192)

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
    # T = 3 transforms of Q = 4 points: 12 pairs, so 48 bytes of cells, 96 of keys and 96 + 3 * 256 for the ICP step
    calls = {
        "fp_mesh_grid_transform_residuals": lambda g, **kw: lib.fp_mesh_grid_transform_residuals(
            kw.get("pos", p), kw.get("Nv", 3), kw.get("faces", p), kw.get("F", 1), g, kw.get("points", p), kw.get("Q", 4), kw.get("tfs", p),
            kw.get("T", 3), kw.get("thr2", p), kw.get("L", 2), kw.get("max_d2", p), kw.get("over", p), None, kw.get("ws", p),
            kw.get("ws_bytes", 48), None),
        "fp_mesh_grid_icp_step": lambda g, **kw: lib.fp_mesh_grid_icp_step(
            kw.get("pos", p), kw.get("Nv", 3), kw.get("faces", p), kw.get("F", 1), g, kw.get("points", p), kw.get("Q", 4), kw.get("tfs", p),
            kw.get("T", 3), kw.get("max_dist", 0.1), kw.get("damping", 1e-3), kw.get("min_pairs", 6), kw.get("system", p),
            kw.get("tfs_out", q), None, None, kw.get("ws", p), kw.get("ws_bytes", 96 + 3 * 256), None),
        "fp_mesh_grid_penetration": lambda g, **kw: lib.fp_mesh_grid_penetration(
            kw.get("pos", p), kw.get("Nv", 3), kw.get("faces", p), kw.get("F", 1), g, kw.get("vn", p), kw.get("en", p), kw.get("points", p),
            kw.get("Q", 4), kw.get("tfs", p), kw.get("T", 3), kw.get("inside", p), None, None, None, None, kw.get("ws", p),
            kw.get("ws_bytes", 96), None)}
    shared = ((dict(T=-1), b"T=-1 or Q=4 is negative"), (dict(Q=-1), b"is negative"), (dict(T=1 << 20, Q=(1 << 10) + 1), b"above 2^30"),
              (dict(F=-1), b"F=-1"), (dict(F=(1 << 30) + 1), b"outside 0..2^30"), (dict(Nv=-1), b"Nv=-1"), (dict(faces=None), b"faces is NULL"),
              (dict(pos=None), b"pos is NULL"), (dict(ws=None), b"workspace"), (dict(ws=C.c_void_p(4098)), b"aligned"))
    own = {
        "fp_mesh_grid_transform_residuals": ((dict(L=-1), b"L=-1"), (dict(L=5), b"L=5"), (dict(max_d2=None), b"NULL max_d2"),
                                             (dict(thr2=None), b"NULL thr2 or over"), (dict(over=None), b"NULL thr2 or over"),
                                             (dict(points=None), b"NULL points or tfs"), (dict(tfs=None), b"NULL points or tfs"),
                                             (dict(ws_bytes=47), b"fp_mesh_transform_residuals_workspace_bytes")),
        "fp_mesh_grid_icp_step": ((dict(max_dist=-1.0), b"max_dist"), (dict(max_dist=float("inf")), b"max_dist"),
                                  (dict(damping=float("nan")), b"damping"), (dict(damping=-1e-3), b"damping"), (dict(min_pairs=5), b"min_pairs=5"),
                                  (dict(tfs=None), b"NULL tfs_in or system"), (dict(system=None), b"NULL tfs_in or system"),
                                  (dict(points=None), b"NULL points"), (dict(ws_bytes=96 + 3 * 256 - 1), b"fp_mesh_icp_workspace_bytes"),
                                  (dict(tfs_out=p), b"overlap"), (dict(tfs_out=C.c_void_p(4096 + 3 * 64 - 4)), b"overlap")),
        "fp_mesh_grid_penetration": ((dict(inside=None), b"NULL inside"), (dict(points=None), b"NULL points or tfs"),
                                     (dict(tfs=None), b"NULL points or tfs"), (dict(vn=None), b"vn is NULL"), (dict(en=None), b"en is NULL"),
                                     (dict(ws_bytes=95), b"fp_mesh_penetration_workspace_bytes"))}
    for name, call in calls.items():
        prefix = name.encode() + b": "
        for kw, word in bad_grids:
            assert call(C.byref(grid(**kw))) == -1, (name, kw)
            msg = lib.fp_last_error()
            assert msg.startswith(prefix) and word in msg, (name, kw, msg)
        assert call(None) == -1
        assert lib.fp_last_error() == prefix + b"NULL grid"
        g = C.byref(grid())
        for kw, word in shared + own[name]:
            assert call(g, **kw) == -1, (name, kw)
            msg = lib.fp_last_error()
            assert msg.startswith(prefix) and word in msg, (name, kw, msg)
        # the order: the sizes first, then the grid, then the parent's own values and pointers
        assert call(None, T=-1) == -1 and b"is negative" in lib.fp_last_error()
        assert call(None, T=0) == -1 and b"NULL grid" in lib.fp_last_error()                 # as Q = 0 of the point forms: the grid is still checked
        assert call(C.byref(grid(h=0.0)), pos=None, faces=None, points=None) == -1 and b"h=0" in lib.fp_last_error()
        # T = 0 does nothing whatever the pointers are
        assert call(g, T=0, pos=None, faces=None, points=None, tfs=None, ws=None, ws_bytes=0, max_d2=None, system=None, inside=None) == 0
    assert calls["fp_mesh_grid_transform_residuals"](C.byref(grid(h=0.0)), L=9) == -1 and b"h=0" in lib.fp_last_error()
    assert calls["fp_mesh_grid_transform_residuals"](g, L=0, thr2=None, over=None, T=0) == 0


# ------------------------------------------------------------------ 2. the walk needs nothing new for a transformed point
@pytest.mark.parametrize("what,name", pc.MODEL_CASES, ids=[f"{w}-{n}".replace(" ", "_") for w, n in pc.MODEL_CASES])
def test_the_models_walk_on_transformed_points_returns_the_references(what, name):
    c = pc.case(what, name)
    moved = sm.transform_points(c["points"], c["tfs"]).reshape(-1, 3)                  # the float32 p' of every pair, n = t * Q + i
    T, Q = len(c["tfs"]), len(c["points"])
    if what == "residuals":
        ref_d2, ref_face = sc.references()[name][2], None
    else:
        terms = ic.references()[name]["terms"]
        ref_d2, ref_face = terms["dist2"], terms["face"]
    assert ref_d2.shape == (T, Q)
    dd, exc = mg.pair_matrix(c["pos"], c["faces"], moved)
    kinds = pc.admitted(what, c)
    assert len(kinds) >= 5
    walked = 0
    for kind in kinds:
        g = pc.grid(what, name, kind)
        assert float(exc.max(initial=0.0)) <= float(g.pad) / 4, (name, kind)        # the header's precondition, for these p'
        tab = mg.tables(g, c["pos"], c["faces"])
        best, face, _, shells = mg.walk(g, tab, dd, moved)
        assert np.array_equal(_bits(best.reshape(T, Q)), _bits(ref_d2)), (name, kind, "dist2")
        if ref_face is not None:
            assert np.array_equal(face.reshape(T, Q), ref_face), (name, kind, "face")
        finite = np.isfinite(moved).all(axis=1)
        assert (shells[~finite] == -1).all() and np.isinf(best[~finite]).all()       # a non-finite p' walks nothing and answers nothing
        walked += int((shells > 0).sum())
    if "special" in name:
        assert not np.isfinite(moved).all() and np.isfinite(moved).any()
    assert walked > 0 or len(c["faces"]) < 3, (name, "no query ever left its own cell")


# ------------------------------------------------------------------ 3. what the cap leaves out
def test_the_cap_leaves_out_tiny_cells_of_a_few_cases_and_nothing_else():
    got = pc.check_omissions()
    assert (len(sc.kernel_cases()), len(ic.kernel_cases())) == (41, 44)
    for what in ("residuals", "icp"):
        assert all(len(got[what][k]) == 0 for k in gcs.GRIDS if k != "tiny cells")
    assert len(got["residuals"]["tiny cells"]) == pc.OMITTED_RESIDUALS == 8 and len(got["icp"]["tiny cells"]) == pc.OMITTED_ICP == 10
    # the special transforms, whose scaled and far rows walk whole grids, stay under every grid
    for what in ("residuals", "icp"):
        for name in ("box special transforms", "skipped and degenerate special transforms", "box without faces T=3"):
            assert pc.admitted(what, pc.case(what, name)) == gcs.GRIDS, (what, name)
    assert pc.admitted_by_size(1, 1, 1 << 21) and pc.admitted_by_size(1 << 7, 1, 1 << 21) and not pc.admitted_by_size(129, 1, 1 << 21)
