"""CPU: the order in which the reconstruction entry points (fp_tsdf_integrate / fp_tsdf_count_triangles / fp_tsdf_emit_triangles /
fp_tsdf_label_components / fp_tsdf_raycast / fp_texture_bake) and their wrappers in ops.py refuse their arguments.  The host tests
beside this one (test_tsdf_host.py, test_tsdf_raycast_host.py, test_tsdf_components_host.py, test_texture_bake_host.py) pass one bad
argument at a time; here every call has two, adjacent in the entry point's order, and the refusal has to name the earlier one.  The
checks these entry points share live in one place (csrc/recon_common.h, ops._view_stack and its neighbours): this is what holds each
entry point's own checks where they have always been between them.  Nothing is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

nan, inf = float("nan"), float("inf")
P = C.c_void_p(16)                         # a pointer that is not NULL: no call here gets as far as reading it
O = (C.c_float * 3)(0, 0, 0)
BAD_O = (C.c_float * 3)(0, inf, 0)
K9 = (C.c_float * 9)(50, 0, 4, 0, 50, 4, 0, 0, 1)
SKEW9 = (C.c_float * 9)(50, 0.5, 4, 0, 50, 4, 0, 0, 1)
HUGE = dict(nz=2048, ny=2048, nx=2048)     # 2^33 voxels, every dimension within 1..4096


def _integrate(lib, V=1, H=8, W=8, nz=4, ny=4, nx=4, origin=O, voxel=0.01, trunc=0.04, min_depth=0.001, depth=P, tsdf=P):
    return lib.fp_tsdf_integrate(depth, P, None, P, P, V, H, W, nz, ny, nx, origin, voxel, trunc, min_depth, tsdf, P, P, P, None)


def _count(lib, tsdf=P, nz=4, ny=4, nx=4, mw=1.0, counts=P):
    return lib.fp_tsdf_count_triangles(tsdf, P, nz, ny, nx, mw, counts, None)


def _emit(lib, tsdf=P, nz=4, ny=4, nx=4, origin=O, voxel=0.01, mw=1.0, total=10, keys=P):
    return lib.fp_tsdf_emit_triangles(tsdf, P, P, P, nz, ny, nx, origin, voxel, mw, P, total, keys, P, P, P, None)


def _label(lib, nz=4, ny=4, nx=4, counts=P, labels=P, sizes=P):
    return lib.fp_tsdf_label_components(counts, nz, ny, nx, labels, sizes, None)


def _raycast(lib, tsdf=P, nz=4, ny=4, nx=4, origin=O, voxel=0.01, mw=1.0, poses=P, K=K9, Ks=None, view=None, V=0, bbox=P, H=8, W=8, N=2,
             oh=4, ow=4, step=0.01, zn=0.001, zf=1.0, depth=P):
    return lib.fp_tsdf_raycast(tsdf, P, P, P, nz, ny, nx, origin, voxel, mw, poses, K, Ks, view, V, bbox, H, W, N, oh, ow, step, zn, zf, depth,
                               None, None, None, None)


def _bake(lib, pos=P, Nv=5, F=4, depth=P, V=2, H=8, W=8, T=4, Bx=2, tol=0.005, min_cos=0.2, min_depth=0.001, tex=P):
    return lib.fp_texture_bake(pos, Nv, P, F, None, depth, P, None, P, P, V, H, W, T, Bx, tol, min_cos, min_depth, tex, P, None)


# (the call, the entry point, [(two faults, the word of the earlier one)], [calls with nothing to do: 0 whatever the pointers are])
C_TABLE = [
    (_integrate, b"fp_tsdf_integrate",
     [(dict(V=-1, H=0), b"V=-1"), (dict(V=5000, H=0), b"V=5000 outside 0..4096 (fuse the views in several calls)"), (dict(H=0, nx=0), b"H=0"),
      (dict(H=1 << 15, W=1 << 15, nx=0), b"2^28"), (dict(nx=0, origin=None), b"dimension"), (dict(HUGE, origin=None), b"2^30"),
      (dict(origin=None, trunc=0.0), b"NULL origin"), (dict(origin=None, voxel=0.0), b"NULL origin"), (dict(origin=BAD_O, voxel=0.0), b"not finite"),
      (dict(voxel=0.0, trunc=0.0), b"voxel"), (dict(trunc=0.0, min_depth=-1.0), b"trunc"), (dict(min_depth=-1.0, tsdf=None), b"min_depth"),
      (dict(tsdf=None, V=0), b"NULL volume"), (dict(tsdf=None, depth=None), b"NULL volume")],
     [dict(V=0, depth=None)]),
    (_count, b"fp_tsdf_count_triangles",
     [(dict(ny=0, mw=nan), b"dimension"), (dict(HUGE, mw=nan), b"2^30"), (dict(mw=nan, tsdf=None), b"min_weight"),
      (dict(mw=nan, ny=1), b"min_weight")],
     [dict(ny=1, tsdf=None, counts=None)]),
    (_emit, b"fp_tsdf_emit_triangles",
     [(dict(nz=0, origin=None), b"dimension"), (dict(HUGE, origin=None), b"2^30"), (dict(origin=None, voxel=-1.0), b"NULL origin"),
      (dict(origin=BAD_O, voxel=-1.0), b"not finite"), (dict(voxel=-1.0, mw=inf), b"voxel"), (dict(mw=inf, total=-1), b"min_weight"),
      (dict(total=-1, keys=None), b"total"), (dict(total=-1, nz=1), b"total"), (dict(tsdf=None, keys=None), b"NULL volume")],
     [dict(total=0, tsdf=None, keys=None), dict(nz=1, tsdf=None, keys=None)]),
    (_label, b"fp_tsdf_label_components",
     [(dict(nx=0, counts=None), b"dimension"), (dict(nz=5000, ny=1), b"dimension"), (dict(HUGE, counts=None), b"2^30")],
     [dict(ny=1, counts=None, labels=None, sizes=None)]),
    (_raycast, b"fp_tsdf_raycast",
     [(dict(N=-1, oh=0), b"N=-1"), (dict(oh=0, nx=0), b"sizes"), (dict(oh=2048, ow=1024, bbox=None), b"2^20"),
      (dict(bbox=None, nx=0), b"without bbox2d"), (dict(nx=0, origin=None), b"dimension"), (dict(HUGE, origin=None), b"2^30"),
      (dict(origin=None, voxel=0.0), b"NULL origin"), (dict(origin=BAD_O, voxel=0.0), b"not finite"), (dict(voxel=0.0, step=0.0), b"voxel"),
      (dict(step=0.0, zn=-0.1), b"step"), (dict(zn=-0.1, zf=inf), b"z_near"), (dict(zf=inf, mw=nan), b"z_far"),
      (dict(mw=nan, step=1e-9), b"min_weight"), (dict(step=1e-9, tsdf=None), b"samples"), (dict(tsdf=None, depth=None), b"NULL volume"),
      (dict(depth=None, K=None), b"every output is NULL"), (dict(K=None, poses=None), b"exactly one"),
      (dict(view=P, K=SKEW9), b"view index needs"), (dict(K=SKEW9, poses=None), b"skew"), (dict(K=None, Ks=P, V=0, N=0), b"V=0"),
      (dict(K=None, Ks=P, V=3, poses=None), b"view is NULL")],
     [dict(N=0, poses=None)]),
    (_bake, b"fp_texture_bake",
     [(dict(F=-1, Nv=-1), b"F=-1"), (dict(Nv=-1, V=5000), b"Nv=-1"), (dict(V=5000, H=0), b"V=5000 outside 0..4096\x00"), (dict(H=0, T=1), b"H=0"),
      (dict(H=1 << 15, W=1 << 15, T=1), b"2^28"), (dict(T=1, Bx=0), b"T=1"), (dict(Bx=0, tol=-1.0), b"Bx=0"),
      (dict(Bx=1025, T=16, tol=-1.0), b"atlas"), (dict(tol=-1.0, min_depth=-1.0), b"tol"), (dict(min_depth=-1.0, min_cos=0.0), b"min_depth"),
      (dict(min_cos=0.0, F=0), b"min_cos"), (dict(min_cos=0.0, pos=None), b"min_cos"), (dict(pos=None, depth=None), b"NULL pos")],
     [dict(F=0, pos=None, depth=None, tex=None)]),
]


def test_c_entry_points_name_the_earlier_of_two_faults():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    for call, who, pairs, nothing_to_do in C_TABLE:
        for kw, word in pairs:
            assert call(lib, **kw) == -1, (who, kw)
            msg = lib.fp_last_error() + b"\x00"          # so that a word can say "and the message ends here"
            assert msg.startswith(who + b": ") and word in msg, (who, kw, msg)
        for kw in nothing_to_do:
            assert call(lib, **kw) == 0, (who, kw)


def _volume(dims=(4, 5, 6)):
    return [torch.ones(dims), torch.zeros(dims), torch.zeros(dims + (3,)), torch.zeros(dims)]


def test_wrappers_name_the_earlier_of_two_faults():
    """on CPU tensors: a wrong shape before a wrong value, a wrong value before the tensor that is not on the device, and each of them
    in its place among its own kind"""
    from foundationpose_amd import _lib, ops
    E = _lib.FpAmdError
    V, H, W = 2, 8, 9
    K = np.array([[50.0, 0, 4], [0, 50, 4], [0, 0, 1]])
    K_skew = np.array([[50.0, 0.1, 4], [0, 50, 4], [0, 0, 1]])
    vol = _volume()
    bad_weight = [vol[0], torch.zeros(4, 5, 5), vol[2], vol[3]]
    views = dict(depth=torch.ones(V, H, W), rgb=torch.zeros(V, H, W, 3), masks=torch.ones(V, H, W, dtype=torch.uint8),
                 ob_in_cams=torch.eye(4).repeat(V, 1, 1), Ks=[K] * V)
    bad_rgb, bad_masks, bad_poses = torch.zeros(V, H, W, 4), torch.ones(V, H, 8, dtype=torch.uint8), torch.eye(4).repeat(3, 1, 1)

    def integrate(vol=vol, origin=(0, 0, 0), voxel=0.01, trunc=0.04, min_depth=0.001, **kw):
        a = dict(views, **kw)
        return ops.tsdf_integrate(*vol, a["depth"], a["rgb"], a["masks"], a["ob_in_cams"], a["Ks"], origin, voxel, trunc, min_depth)

    def bake(**kw):
        a = dict(views, pos=torch.zeros(5, 3), faces=torch.zeros(4, 3, dtype=torch.int32), vertex_color=torch.zeros(5, 3), tol=0.005, min_cos=0.2,
                 texels=4, Bx=None, min_depth=0.001)
        a.update(kw)
        return ops.texture_bake(a["pos"], a["faces"], a["vertex_color"], a["depth"], a["rgb"], a["masks"], a["ob_in_cams"], a["Ks"], a["tol"],
                                a["min_cos"], a["texels"], a["Bx"], a["min_depth"])

    def raycast(vol=vol, origin=(0, 0, 0), voxel=0.01, poses=torch.eye(4).repeat(2, 1, 1), K=K, **kw):
        return ops.tsdf_raycast(*vol, origin, voxel, poses, K, H, W, **kw)

    def extract(vol=vol, origin=(0, 0, 0), voxel=0.01, **kw):
        return ops.tsdf_extract(*vol, origin, voxel, **kw)

    def components(counts=torch.zeros((3, 4, 5), dtype=torch.int32), dims=(4, 5, 6)):
        return ops.tsdf_components(counts, dims)

    table = [
        (integrate, dict(rgb=np.zeros((V, H, W, 3)), depth=torch.ones(H, W)), E, "depth must have 3"),
        (integrate, dict(rgb=np.zeros((V, H, W, 3)), ob_in_cams=torch.eye(4)), E, "rgb must be a tensor"),
        (integrate, dict(depth=torch.ones(4097, 1, 1), rgb=bad_rgb), E, "4097 views in one call, at most 4096 \\(fuse them in several calls\\)"),
        (integrate, dict(depth=torch.ones(V, 0, W), rgb=bad_rgb), E, "frames of 0 x 9"),
        (integrate, dict(rgb=bad_rgb, trunc=0.0), E, "rgb must be"),
        (integrate, dict(rgb=bad_rgb, masks=bad_masks), E, "rgb must be"),
        (integrate, dict(masks=bad_masks, ob_in_cams=bad_poses), E, "masks must be"),
        (integrate, dict(ob_in_cams=bad_poses, vol=bad_weight), E, "ob_in_cams must be"),
        (integrate, dict(vol=bad_weight, origin=(0, 0)), E, "weight must be"),
        (integrate, dict(vol=[torch.ones(4, 0, 6)] + vol[1:], origin=(0, 0)), E, "dimension"),
        (integrate, dict(origin=(0, nan, 0), voxel=0.0), ValueError, "origin"),
        (integrate, dict(voxel=0.0, trunc=0.0), ValueError, "voxel"),
        (integrate, dict(trunc=0.0, min_depth=-1.0), ValueError, "trunc"),
        (integrate, dict(min_depth=-1.0, Ks=[K]), ValueError, "min_depth"),
        (integrate, dict(trunc=0.0), ValueError, "trunc"),                       # the value before the CPU tensors
        (integrate, dict(Ks=[K_skew] * V), ValueError, "skew.*projection of a voxel"),
        (integrate, dict(Ks=[K]), E, "1 intrinsic matrices for 2 views"),
        (integrate, dict(), E, "CUDA"),
        (bake, dict(pos=torch.zeros(5), depth=torch.ones(H, W)), E, "pos must have 2"),
        (bake, dict(pos=np.zeros((5, 3)), depth=torch.ones(H, W)), E, "pos must be a tensor"),
        (bake, dict(faces=torch.zeros(4, dtype=torch.int32), depth=torch.ones(H, W)), E, "faces must have 2"),
        (bake, dict(pos=torch.zeros(5, 4), rgb=bad_rgb), E, "pos must be \\(Nv,3\\)"),
        (bake, dict(vertex_color=torch.zeros(4, 3), depth=torch.ones(4097, 1, 1)), E, "vertex_color must be"),
        (bake, dict(depth=torch.ones(4097, 1, 1), rgb=bad_rgb), E, "4097 views in one call, at most 4096$"),
        (bake, dict(rgb=bad_rgb, texels=1), E, "rgb must be"),
        (bake, dict(ob_in_cams=bad_poses, texels=1), E, "ob_in_cams must be"),
        (bake, dict(texels=1, tol=-1.0), ValueError, "texels"),
        (bake, dict(tol=-1.0, min_cos=0.0), ValueError, "tol"),
        (bake, dict(min_cos=0.0, min_depth=-1.0), ValueError, "min_cos"),
        (bake, dict(min_depth=-1.0, Ks=[K]), ValueError, "min_depth"),
        (bake, dict(Ks=[K_skew] * V), ValueError, "skew.*projection of a texel"),
        (bake, dict(Ks=[K]), E, "1 intrinsic matrices for 2 views"),
        (bake, dict(), E, "CUDA"),
        (raycast, dict(vol=bad_weight, poses=torch.eye(4)), E, "weight must be"),
        (raycast, dict(voxel=0.0, poses=torch.eye(4)), ValueError, "voxel"),
        (raycast, dict(poses=torch.eye(4), step=0.0), E, "poses must be"),
        (raycast, dict(out_hw=(4, 4), want=()), E, "out_hw must be"),
        (raycast, dict(want=(), step=0.0), ValueError, "want"),
        (raycast, dict(step=0.0, z_near=-0.1), ValueError, "step"),
        (raycast, dict(step=1e-9, z_near=-0.1), ValueError, "samples"),
        (raycast, dict(z_near=-0.1, z_far=inf), ValueError, "z_near"),
        (raycast, dict(z_far=inf, min_weight=nan), ValueError, "z_far"),
        (raycast, dict(min_weight=nan, K=K_skew), ValueError, "min_weight"),
        (raycast, dict(K=K_skew, out=dict(xyz=torch.zeros(1))), ValueError, "skew"),
        (raycast, dict(), E, "CUDA"),
        (extract, dict(vol=bad_weight, min_weight=nan), E, "weight must be"),
        (extract, dict(voxel=-1.0, min_weight=nan), ValueError, "voxel"),
        (extract, dict(min_weight=nan, keep=0), ValueError, "min_weight"),
        (extract, dict(keep=0), ValueError, "keep must be"),
        (extract, dict(), E, "CUDA"),
        (components, dict(dims=(4, 5)), ValueError, "dims must be"),
        (components, dict(dims=(4, 0, 6), counts=np.zeros(60, np.int32)), E, "dimension"),
        (components, dict(counts=np.zeros(61, np.int32)), E, "tensor"),
        (components, dict(dims=(4, 5, 7)), E, "cubes"),
        (components, dict(), E, "CUDA"),
    ]
    for call, kw, exc, word in table:
        with pytest.raises(exc, match=word):
            call(**kw)
