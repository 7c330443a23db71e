"""CPU: the definition of the texture bake (include/fp_amd.h: fp_texture_bake; ops.texture_bake's atlas layout; reconstruct.bake_texture's
rounding) through its numpy restatement (tests/texture_bake_model.py), which the GPU tests then hold the kernel to bit by bit: that the
layout keeps every bilinear tap of the rasteriser inside the face's own block, that each deliberately wrong variant is told apart, what
the definition gives on the can from 16 oracle renders against renders of the true mesh, every refusal that needs no device, and the
OBJ round trip of a mesh with its own uv index table.  Each test prints its figures before it asserts.

Measured (the restatement, CPU): the can at 2.5 mm from 16 oracle renders, 83 024 faces, T = 4 (an atlas of 1156 x 1152), on five
held-out views (360 632 pixels covered by both renders): mean absolute colour error 21.33 levels of 255 with the atlas against 25.12 with
the vertex colours (ratio 0.849; the bound is 0.90), no texel of a real block without a view (the bound is 1 %), 5.45 views a texel."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import texture_bake_model as tb
import tsdf_model as tm
from test_tsdf_host import can_model_volume, can_views  # noqa: F401

f32 = np.float32


# ------------------------------------------------------------------ the layout
def _layout_leak(T, F, Bx, f, inset=0.5, n=400, seed=0):
    """the largest total bilinear weight, over barycentrics inside face f (its corners, edge points and seeded interior points), that
    tex_fetch puts on texels outside the face's block, for the restatement's uv"""
    rng = np.random.default_rng(seed)
    Ht, Wt = tb.atlas_shape(F, T, Bx)
    uv, uv_idx = tb.atlas_uv(F, T, Bx, inset)
    r = rng.dirichlet(np.ones(3), n)
    t = rng.random(n // 4)
    edges = np.concatenate([np.stack([t, 1 - t, 0 * t], 1), np.stack([0 * t, t, 1 - t], 1), np.stack([1 - t, 0 * t, t], 1)])
    bary = np.concatenate([np.eye(3), edges, r]).astype(f32)
    bary[:, 2] = (f32(1) - bary[:, 0]) - bary[:, 1]                   # as the rasteriser forms the third one
    bary = bary[bary[:, 2] >= 0]
    t_uv = tb.interpolate_uv(uv[uv_idx[f]], bary)
    cols, rows, w = tb.tex_fetch_taps(t_uv[:, 0], t_uv[:, 1], Ht, Wt)
    bx, by = f % Bx, f // Bx
    col_in = (cols >= bx * T) & (cols < (bx + 1) * T)                 # (N,2)
    row_in = (rows >= by * T) & (rows < (by + 1) * T)
    inside = row_in[:, :, None] & col_in[:, None, :]
    assert np.allclose(w.sum((1, 2)), 1)
    return float(np.where(inside, 0, w).sum((1, 2)).max())


@pytest.mark.parametrize("T", [2, 3, 4, 5, 8, 16])
def test_the_layout_keeps_every_tap_inside_the_faces_block(T):
    """The corners sit half a texel inside the block, so in exact arithmetic the tap coordinates u * Wt - 0.5 of a point of the triangle
    lie in [bx * T, bx * T + T - 1]: the two taps are the block's, or the outer one has weight exactly 0.  In float32 a coordinate on
    the block's first or last texel centre can come out a rounding error beyond it, which gives the neighbouring block that error as
    its weight.  The error: uv is rounded once (relative 2^-24), the interpolation rounds three times and tex_fetch's fmaf once, each
    relative 2^-24 of a value <= 1, scaled by the atlas side: at most 5 * 2^-24 * max(Wt, Ht) texels.  That is the bound on the weight
    outside the block (2e-4 at the largest atlas the entry point takes; 1.4e-5 here at most); an inset of 0 in place of 0.5 puts half
    of the weight there."""
    F, Bx = 11, 4                                                      # three block rows, the last with three of four columns
    Ht, Wt = tb.atlas_shape(F, T, Bx)
    bound = 5 * 2.0 ** -24 * max(Ht, Wt)
    for f in (0, 4, 3, 7, 8, 10):                                      # first column, last column, last row
        leak = _layout_leak(T, F, Bx, f)
        wrong = _layout_leak(T, F, Bx, f, inset=0.0)
        print(f"T={T} face {f}: weight outside the block {leak:.3e} (bound {bound:.3e}); with an inset of 0: {wrong:.3f}")
        assert leak <= bound
        assert wrong >= 0.25
    # one face, one block: the atlas is the block (the taps that leave it wrap around into it on the other side)
    assert _layout_leak(T, 1, 1, 0) <= 5 * 2.0 ** -24 * T


def test_the_uv_are_the_blocks_corners_and_the_default_width_is_square():
    for F, bx in ((0, 1), (1, 1), (2, 2), (4, 2), (5, 3), (63, 8), (64, 8), (65, 9), (257, 17), (83024, 289)):
        assert tb.default_bx(F) == bx
    uv, idx = tb.atlas_uv(5, 4, 3)
    assert uv.dtype == f32 and uv.shape == (15, 2) and idx.dtype == np.int32 and np.array_equal(idx, np.arange(15).reshape(5, 3))
    want = np.asarray([[4.5 / 12, 4.5 / 8], [7.5 / 12, 4.5 / 8], [4.5 / 12, 7.5 / 8]])         # face 4: block column 1, block row 1
    assert np.array_equal(uv[12:15], want.astype(f32))


# ------------------------------------------------------------------ wrong variants are told apart
def _differ(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def test_generated_cases_reach_every_way_through_the_definition():
    total = {}
    for c in tb.CASES:
        st = {}
        tex, cov = tb.bake_case(tb.case_of(c), stats=st)
        assert np.isfinite(tex).all() and tex.shape[:2] == cov.shape
        for k, v in st.items():
            total[k] = total.get(k, 0) + v
    print(total)
    assert all(v > 0 for v in total.values()), total


def test_wrong_variants_change_the_atlas():
    case = tb.case_of(tb.CASES[6])                                     # 64 faces, T = 8, 3 views, masks and colours
    tex, cov = tb.bake_case(case)
    for wrong in ("no_clamp", "backfacing", "unweighted"):
        got, gcov = tb.bake_case(case, wrong=wrong)
        print(f"{wrong}: {_differ(got, tex)} of {tex.size} texel values differ, {int((gcov != cov).sum())} coverages")
        assert _differ(got, tex) > 0
    # without the clamp the texels beyond the hypotenuse are points outside the face: with it they are points of the hypotenuse
    T = case["T"]
    a = np.arange(T, dtype=f32)[None, :] / f32(T - 1)
    beyond = (a + a.T) > 1
    block = lambda t, f: t[(f // case["Bx"]) * T:(f // case["Bx"] + 1) * T, (f % case["Bx"]) * T:(f % case["Bx"] + 1) * T]     # noqa: E731
    got, _ = tb.bake_case(case, wrong="no_clamp")
    assert _differ(block(got, 0)[~beyond], block(tex, 0)[~beyond]) == 0 and _differ(block(got, 0)[beyond], block(tex, 0)[beyond]) > 0
    # unweighted: the coverage is the same, only the blend differs
    assert np.array_equal(tb.bake_case(case, wrong="unweighted")[1], cov)


def test_an_occluder_in_one_view_is_kept_out_by_the_depth_test():
    """view 1 sees a plane 0.1 m in front of the slab: with the depth test it colours no texel; without it, it does"""
    case = tb.generated_case(64, 4, None, 2, 37, 53, 0, seed=5, occluder=True)
    st = {}
    tex, cov = tb.bake_case(case, stats=st)
    only0 = dict(case, depth=case["depth"][:1], rgb=case["rgb"][:1], masks=case["masks"][:1], ob_in_cams=case["ob_in_cams"][:1], Ks=case["Ks"][:1])
    tex0, cov0 = tb.bake_case(only0)
    got, gcov = tb.bake_case(case, wrong="no_depth_test")
    print(f"occluder: {st['hidden']} (view, texel) pairs hidden; without the depth test {_differ(got, tex)} texel values differ")
    assert st["hidden"] > 100 and _differ(tex, tex0) == 0 and np.array_equal(cov, cov0)
    assert _differ(got, tex) > 0 and int(gcov.sum()) > int(cov.sum())


def test_truncation_in_place_of_rounding_changes_the_stored_atlas():
    tex, _ = tb.bake_case(tb.case_of(tb.CASES[6]))
    r, t = tb.round_atlas(tex), tb.round_atlas(tex, wrong="trunc")
    print(f"truncation: {int((r != t).sum())} of {r.size} stored values differ")
    assert (r != t).sum() > r.size // 4 and np.abs(r - tex).max() <= 0.5 and r.min() >= 0 and r.max() <= 255
    assert np.array_equal(tb.round_atlas(np.asarray([-3.0, 0.49, 0.5, 254.5, 300.0], f32)), np.asarray([0, 0, 1, 255, 255], f32))


# ------------------------------------------------------------------ the can from 16 oracle renders
def _mesh_dict(pos, faces, nrm, **kw):
    return dict(pos=np.asarray(pos, f32), faces=np.asarray(faces, np.int32), vnormals=np.asarray(nrm, f32), **kw)


def _render(scene, mesh_np, poses):
    from oracle import ops as oo
    return oo.render_crops(mesh_np, poses, None, scene["K"], scene["H"], scene["W"], (scene["H"], scene["W"]), normalize_xyz=False,
                           want=("color", "depth"))


def test_the_can_with_an_atlas_is_closer_to_the_true_mesh_than_with_vertex_colours(scene, can_views, can_model_volume):
    """The can fused at 2.5 mm from 16 oracle renders, T = 4, tol = two voxels, min_cos = 0.2; renders by the oracle at five held-out
    poses against renders of the true mesh.  Bounds: textured error <= 0.90 x the vertex-colour error (measured 0.849: 21.33 against
    25.12 levels; both carry the reference views' shading, which the render applies again), at most 1 % of the real blocks' texels
    without a view (measured 0)."""
    v = can_views
    pos, col, nrm, faces = tm.extract(can_model_volume)
    vcol = np.clip(np.floor(col + f32(0.5)), 0, 255).astype(f32)              # as TsdfVolume.extract rounds them
    F, T = len(faces), 4
    Bx = tb.default_bx(F)
    st = {}
    tex, cov = tb.bake(pos, faces, vcol, v["depth"], v["rgb"], v["masks"], v["ob_in_cams"], v["Ks"], T, Bx, 2 * tm.CAN_VOXEL, 0.2, stats=st)
    uv, uv_idx = tb.atlas_uv(F, T, Bx)
    share = st["fallback"] / (F * T * T)
    poses = tb.held_out_poses()
    true = _render(scene, scene["mesh_np"], poses)
    scale = f32(1.0) / f32(255.0)
    plain = _render(scene, _mesh_dict(pos, faces, nrm, vertex_color=vcol * scale), poses)
    textured = _render(scene, _mesh_dict(pos, faces, nrm, tex=tb.round_atlas(tex) * scale, uv=uv, uv_idx=uv_idx), poses)
    e_plain, n_plain = tb.colour_error(plain["color"], true["color"], plain["depth"], true["depth"])
    e_tex, n_tex = tb.colour_error(textured["color"], true["color"], textured["depth"], true["depth"])
    print(f"can: {F} faces, atlas {tex.shape[0]} x {tex.shape[1]}, {cov[cov > 0].mean() if (cov > 0).any() else 0:.2f} views a covered texel, "
          f"fallback share {share:.4%}; colour error over {n_tex} pixels: atlas {e_tex:.2f}, vertex colours {e_plain:.2f} levels "
          f"(ratio {e_tex / e_plain:.3f}, bound 0.90)")
    assert F > 80000 and n_plain == n_tex > 300000
    assert share <= 0.01
    assert e_tex <= 0.90 * e_plain


# ------------------------------------------------------------------ refusals that need no device
def _cpu_call(**kw):
    from foundationpose_amd import ops
    V, H, W = 2, 8, 9
    a = dict(pos=torch.zeros(5, 3), faces=torch.zeros(4, 3, dtype=torch.int32), vertex_color=torch.zeros(5, 3), depth=torch.ones(V, H, W),
             rgb=torch.zeros(V, H, W, 3), masks=torch.ones(V, H, W, dtype=torch.uint8), ob_in_cams=torch.eye(4).repeat(V, 1, 1),
             Ks=[np.array([[50.0, 0, 4], [0, 50, 4], [0, 0, 1]])] * V, tol=0.005, min_cos=0.2, texels=4, Bx=None, min_depth=0.001)
    a.update(kw)
    return ops.texture_bake(a["pos"], a["faces"], a["vertex_color"], a["depth"], a["rgb"], a["masks"], a["ob_in_cams"], a["Ks"], a["tol"],
                            a["min_cos"], a["texels"], a["Bx"], a["min_depth"])


def test_wrappers_refuse_shapes_and_values_before_devices():
    from foundationpose_amd import _lib
    from foundationpose_amd.reconstruct import bake_texture, reconstruct_object
    E = _lib.FpAmdError
    for kw, word in ((dict(pos=torch.zeros(5, 4)), "pos must be"), (dict(faces=torch.zeros(4, dtype=torch.int32)), "faces must"),
                     (dict(vertex_color=torch.zeros(4, 3)), "vertex_color must be"), (dict(rgb=torch.zeros(2, 8, 9, 4)), "rgb must be"),
                     (dict(depth=torch.ones(8, 9)), "depth must"), (dict(masks=torch.ones(2, 8, 8, dtype=torch.uint8)), "masks must be"),
                     (dict(ob_in_cams=torch.eye(4).repeat(3, 1, 1)), "ob_in_cams must be"),
                     (dict(Ks=[np.eye(3)]), "intrinsic matrices"), (dict(pos=np.zeros((5, 3))), "pos must be a tensor")):
        with pytest.raises(E, match=word):
            _cpu_call(**kw)
    with pytest.raises(ValueError, match="skew"):
        _cpu_call(Ks=[np.array([[50.0, 0.1, 4], [0, 50, 4], [0, 0, 1]])] * 2)
    for bad in (dict(texels=1), dict(texels=17), dict(Bx=0), dict(texels=16, Bx=2000), dict(tol=-1.0), dict(tol=float("nan")),
                dict(min_cos=0.0), dict(min_cos=1.5), dict(min_cos=float("nan")), dict(min_depth=-0.1), dict(min_depth=float("inf"))):
        with pytest.raises(ValueError):
            _cpu_call(**bad)
    # values are refused before the device is looked at, and CPU tensors last of all
    with pytest.raises(ValueError, match="tol"):
        _cpu_call(tol=float("inf"))
    with pytest.raises(E, match="CUDA"):
        _cpu_call()
    t = dict(pos=torch.zeros(5, 3), faces=torch.zeros(4, 3, dtype=torch.int32), vnormals=torch.zeros(5, 3))
    views = (np.zeros((2, 8, 9, 3)), np.ones((2, 8, 9)), np.ones((2, 8, 9)), np.tile(np.eye(4), (2, 1, 1)), np.eye(3))
    with pytest.raises(ValueError, match="tol is required"):
        bake_texture(t, *views)
    with pytest.raises(ValueError, match="vnormals"):
        bake_texture(dict(pos=t["pos"], faces=t["faces"]), *views, tol=0.005)
    with pytest.raises(ValueError, match="texels must be"):
        reconstruct_object(*views, texture=1, device="cpu")
    with pytest.raises(ValueError, match="uv_faces"):
        from foundationpose_amd.mesh import SimpleMesh
        SimpleMesh(np.zeros((3, 3)), np.asarray([[0, 1, 2]]), uv=np.zeros((3, 2)), texture=np.zeros((2, 2, 3), np.uint8), uv_faces=np.zeros((2, 3)))


def test_the_c_entry_point_reports_argument_errors_without_a_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(16)

    def bake(pos=p, Nv=5, faces=p, F=4, depth=p, V=2, H=8, W=8, T=4, Bx=2, tol=0.005, min_cos=0.2, min_depth=0.001, tex=p, coverage=p):
        return lib.fp_texture_bake(pos, Nv, faces, F, None, depth, p, None, p, p, V, H, W, T, Bx, tol, min_cos, min_depth, tex, coverage, None)

    for kw, word in ((dict(pos=None), b"NULL pos"), (dict(faces=None), b"NULL pos"), (dict(tex=None), b"NULL pos"), (dict(coverage=None), b"NULL pos"),
                     (dict(depth=None), b"NULL depth"), (dict(T=1), b"T=1"), (dict(T=17), b"T=17"), (dict(Bx=0), b"Bx=0"),
                     (dict(Bx=1025, T=16), b"atlas"), (dict(F=4097, Bx=1), b"atlas"), (dict(F=-1), b"F=-1"), (dict(F=(1 << 24) + 1), b"F="),
                     (dict(Nv=-1), b"Nv=-1"), (dict(V=-1), b"V=-1"), (dict(V=4097), b"V=4097"), (dict(H=0), b"H=0"), (dict(W=0), b"W=0"),
                     (dict(H=1 << 15, W=1 << 15), b"2^28"), (dict(tol=-1.0), b"tol"), (dict(tol=float("nan")), b"tol"),
                     (dict(tol=float("inf")), b"tol"), (dict(min_depth=-1.0), b"min_depth"), (dict(min_depth=float("nan")), b"min_depth"),
                     (dict(min_cos=0.0), b"min_cos"), (dict(min_cos=1.0001), b"min_cos"), (dict(min_cos=float("nan")), b"min_cos")):
        assert bake(**kw) == -1, kw
        msg = lib.fp_last_error()
        assert msg.startswith(b"fp_texture_bake") and word in msg, (kw, msg)
    assert bake(F=0, pos=None, faces=None, tex=None, coverage=None, depth=None) == 0            # nothing to do


# ------------------------------------------------------------------ a mesh with its own uv index table through OBJ
def test_save_obj_and_load_obj_keep_the_picture_of_a_mesh_with_uv_faces(scene, tmp_path):
    """a coarse can (120 faces) with a baked atlas from two of the scene's views: the oracle's render of the mesh as reconstruct.py
    hands it over (uv with its own index table) against that of the mesh read back from OBJ + MTL + PNG (one vertex per distinct
    (v, vt) pair, uv_idx = faces), within 1e-5"""
    from foundationpose_amd.mesh import SimpleMesh, make_can_mesh
    from foundationpose_amd.mesh_io import load_obj, save_obj, save_ply, load_ply
    from foundationpose_amd.Utils import make_mesh_tensors  # noqa: F401  (the device twin of mesh_tensors_np: the same uv_faces rule)
    from oracle import pipeline as op
    coarse = make_can_mesh(n_ang=12, n_axial=4, textured=False)
    pos, faces, nrm = np.asarray(coarse.vertices, f32), np.asarray(coarse.faces), np.asarray(coarse.vertex_normals, f32)
    poses = tm.can_view_poses(16, 0.5)[[0, 7]].astype(f32)
    ref = _render(scene, scene["mesh_np"], poses)
    rgb = np.ascontiguousarray(np.clip(ref["color"], 0, 1) * 255, f32)
    F, T = len(faces), 4
    Bx = tb.default_bx(F)
    vcol = np.asarray(coarse.visual.vertex_colors, f32)
    tex, cov = tb.bake(pos, faces, vcol, ref["depth"], rgb, (ref["depth"] > 0).astype(np.uint8), poses, np.tile(scene["K"][None], (2, 1, 1)),
                       T, Bx, 0.01, 0.2)
    assert (cov > 0).mean() > 0.2
    image = tb.round_atlas(tex).astype(np.uint8)
    uv, uv_idx = tb.atlas_uv(F, T, Bx)
    uv_file = uv.astype(np.float64)
    uv_file[:, 1] = 1 - uv_file[:, 1]
    mesh = SimpleMesh(pos, faces, vertex_normals=nrm, uv=uv_file, texture=image, uv_faces=uv_idx, vertex_colors=vcol.astype(np.uint8))
    path = str(tmp_path / "can.obj")
    save_obj(mesh, path)
    assert os.path.exists(str(tmp_path / "can.mtl")) and os.path.exists(str(tmp_path / "can.png"))
    a, b, c = faces[1] + 1
    assert [line.strip() for line in open(path) if line.startswith("f ")][1] == f"f {a}/4/{a} {b}/5/{b} {c}/6/{c}"
    back = load_obj(path)
    assert back.visual.material.image.shape == image.shape and np.array_equal(back.visual.material.image, image)
    assert len(back.faces) == F and len(back.vertices) == 3 * F                  # one vertex per (v, vt) pair: every corner has its own uv
    view = tb.held_out_poses()[:2]
    direct = _render(scene, _mesh_dict(pos, faces, nrm, tex=image.astype(f32) * (f32(1.0) / f32(255.0)), uv=uv, uv_idx=uv_idx), view)
    loaded = _render(scene, op.mesh_tensors_np(back), view)
    diff = float(np.abs(direct["color"] - loaded["color"]).max())
    print(f"OBJ round trip: largest colour difference {diff:.2e}, depth {float(np.abs(direct['depth'] - loaded['depth']).max()):.2e}")
    assert (direct["depth"] > 0).sum() > 10000 and np.array_equal(direct["depth"] > 0, loaded["depth"] > 0)
    assert diff <= 1e-5
    # the vertex colours stay beside the texture: PLY output is what it was
    save_ply(mesh, str(tmp_path / "can.ply"))
    assert np.array_equal(load_ply(str(tmp_path / "can.ply")).visual.vertex_colors, vcol.astype(np.uint8))
