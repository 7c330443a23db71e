"""ctypes binding of libfp_amd.so (the C ABI declared in include/fp_amd.h).

Fails loudly: there is no fallback path.  torch is imported first so that the HIP runtime
already mapped by PyTorch-ROCm (soname libamdhip64.so.7) is the one our library binds to.
"""
import ctypes as C
import os

import torch  # noqa: F401  (must precede CDLL: shares the HIP runtime with PyTorch)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FP_AMD_LIB") or os.path.join(_HERE, "csrc", "libfp_amd.so")   # FP_AMD_LIB: A/B builds
ABI_VERSION = 234  # = FP_AMD_ABI_VERSION of include/fp_amd.h (tests/test_abi.py keeps the two in step)
_lib = None

vp, ci, cf, cd, sz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t



class MeshGridStruct(C.Structure):
    """fp_mesh_grid of include/fp_amd.h"""
    _fields_ = [("lo", cf * 3), ("h", cf), ("n", C.c_int32 * 3), ("pad", cf), ("cell_start", vp), ("entries", vp), ("overflow", vp),
                ("n_entries", C.c_int32), ("n_overflow", C.c_int32)]


gp = C.POINTER(MeshGridStruct)

# name -> (restype, argtypes); must list every symbol of include/fp_amd.h (checked by tests/test_abi.py)
SIGNATURES = {
    "fp_last_error": (C.c_char_p, []),
    "fp_version": (ci, []),
    "fp_mesh_create": (ci, [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, C.POINTER(vp)]),
    "fp_mesh_destroy": (None, [vp]),
    "fp_mesh_set_create": (ci, [vp, ci, C.POINTER(vp)]),
    "fp_mesh_set_destroy": (None, [vp]),
    "fp_mesh_set_workspace_bytes": (sz, [vp, ci, ci, ci]),
    "fp_depth_erode": (ci, [vp, vp, ci, ci, ci, cf, cf, cf, vp]),
    "fp_depth_bilateral": (ci, [vp, vp, ci, ci, ci, cf, cf, cf, vp]),
    "fp_depth_to_xyz": (ci, [vp, vp, cf, ci, vp, ci, ci, vp]),
    "fp_crop_windows": (ci, [vp, vp, vp, vp, ci, cd, vp, vp, ci, cd, ci, ci, ci, vp, vp, vp]),
    "fp_depth_erode_frames": (ci, [vp, vp, ci, ci, ci, ci, cf, cf, cf, vp]),
    "fp_depth_bilateral_frames": (ci, [vp, vp, ci, ci, ci, ci, cf, cf, cf, vp]),
    "fp_depth_to_xyz_frames": (ci, [vp, vp, cf, ci, vp, ci, ci, ci, vp]),
    "fp_mask_depth_stats": (ci, [vp, vp, vp, ci, ci, ci, ci, cf, vp, vp]),
    "fp_depth_agreement": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, cf, vp, vp]),
    "fp_icp_workspace_bytes": (sz, [ci, ci, ci]),
    "fp_icp_point_plane": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, vp, ci, ci, ci, cf, cd, ci, vp, vp, vp, sz, vp]),
    "fp_pose_errors_workspace_bytes": (sz, [ci, ci, ci]),
    "fp_pose_errors": (ci, [vp, ci, vp, ci, vp, vp, vp, ci, ci, ci, vp, vp, sz, vp]),
    "fp_vsd_counts": (ci, [vp, vp, vp, ci, ci, ci, ci, vp, vp, ci, ci, ci, ci, cf, vp, ci, vp, vp]),
    "fp_mspd": (ci, [vp, ci, vp, ci, vp, vp, vp, ci, ci, vp, vp, vp]),
    "fp_mesh_point_distance_workspace_bytes": (sz, [ci]),
    "fp_mesh_point_distance": (ci, [vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, sz, vp]),
    "fp_mesh_ray_cast_workspace_bytes": (sz, [ci]),
    "fp_mesh_ray_cast": (ci, [vp, ci, vp, ci, vp, vp, ci, cf, cf, ci, vp, vp, vp, vp, vp, sz, vp]),
    "fp_mesh_transform_residuals_workspace_bytes": (sz, [ci, ci]),
    "fp_mesh_transform_residuals": (ci, [vp, ci, vp, ci, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, sz, vp]),
    "fp_mesh_icp_workspace_bytes": (sz, [ci, ci]),
    "fp_mesh_icp_step": (ci, [vp, ci, vp, ci, vp, ci, vp, ci, cf, cd, ci, vp, vp, vp, vp, vp, sz, vp]),
    "fp_mesh_pseudonormals": (ci, [vp, ci, vp, ci, vp, vp, vp]),
    "fp_mesh_signed_distance_workspace_bytes": (sz, [ci]),
    "fp_mesh_signed_distance": (ci, [vp, ci, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, sz, vp]),
    "fp_mesh_penetration_workspace_bytes": (sz, [ci, ci]),
    "fp_mesh_penetration": (ci, [vp, ci, vp, ci, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, sz, vp]),
    "fp_mesh_grid_count": (ci, [vp, ci, vp, ci, gp, vp, vp]),
    "fp_mesh_grid_fill_workspace_bytes": (sz, [gp]),
    "fp_mesh_grid_fill": (ci, [vp, ci, vp, ci, gp, vp, vp, sz, vp]),
    "fp_mesh_grid_point_distance": (ci, [vp, ci, vp, ci, gp, vp, ci, vp, vp, vp, vp, sz, vp]),
    "fp_mesh_grid_signed_distance": (ci, [vp, ci, vp, ci, gp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, sz, vp]),
    "fp_mesh_grid_transform_residuals": (ci, [vp, ci, vp, ci, gp, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, sz, vp]),
    "fp_mesh_grid_icp_step": (ci, [vp, ci, vp, ci, gp, vp, ci, vp, ci, cf, cd, ci, vp, vp, vp, vp, vp, sz, vp]),
    "fp_mesh_grid_penetration": (ci, [vp, ci, vp, ci, gp, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, sz, vp]),
    "fp_tsdf_integrate": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, cf, cf, cf, vp, vp, vp, vp, vp]),
    "fp_tsdf_count_triangles": (ci, [vp, vp, ci, ci, ci, cf, vp, vp]),
    "fp_tsdf_emit_triangles": (ci, [vp, vp, vp, vp, ci, ci, ci, vp, cf, cf, vp, C.c_longlong, vp, vp, vp, vp, vp]),
    "fp_tsdf_label_components": (ci, [vp, ci, ci, ci, vp, vp, vp]),
    "fp_tsdf_raycast": (ci, [vp, vp, vp, vp, ci, ci, ci, vp, cf, cf, vp, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci, cf, cf, cf, vp, vp, vp, vp, vp]),
    "fp_texture_bake": (ci, [vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, cf, cf, cf, vp, vp, vp]),
    "fp_workspace_bytes": (sz, [ci, ci, ci, ci, ci]),
    "fp_raster_lds_bytes": (sz, [ci]),
    "fp_render_crops": (ci, [vp, vp, vp, vp, cf, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, cf, cf, cf, ci, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "fp_warp_crops": (ci, [vp, vp, vp, vp, vp, vp, vp, ci, vp, cf, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp]),
    "fp_pose_update": (ci, [vp, vp, vp, ci, ci, vp, cf, cf, vp, vp, ci, ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, cf, vp]),
    "fp_conv7x7s2_bn_relu_fwd": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "fp_igemm_f16_fwd": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, vp]),
    "fp_pack_conv3x3_tiles_f16": (ci, [vp, vp, ci, ci, vp]),
    "fp_pack_conv3x3_tiles_direct_f16": (ci, [vp, vp, ci, ci, vp]),
    "fp_conv3x3_sw_lds_bytes": (ci, []),
    "fp_igemm_splitk_workspace_bytes": (sz, [ci, ci, ci]),
    "fp_igemm_f16_splitk_fwd": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, ci, vp, sz, vp]),
    "fp_add_pe_f16_fwd": (ci, [vp, vp, vp, ci, ci, ci, vp]),
    "fp_replicate_rows_f16": (ci, [vp, vp, ci, ci, ci, ci, ci, C.c_longlong, vp]),
    "fp_replicate_segments_f16": (ci, [vp, vp, ci, ci, ci, ci, ci, C.c_longlong, vp]),
    "fp_layernorm_res_fwd": (ci, [vp, vp, vp, ci, vp, vp, vp, cf, vp, vp, ci, ci, vp]),
    "fp_pack_linear512_f16": (ci, [vp, vp, vp]),
    "fp_linear512_f16_fwd": (ci, [vp, vp, vp, vp, ci, ci, ci, vp]),
    "fp_pack_linear512_direct_f16": (ci, [vp, vp, vp]),
    "fp_linear512_flags_f16_fwd": (ci, [vp, vp, vp, vp, ci, ci, ci, vp]),
    "fp_linear_layernorm_fwd": (ci, [vp, vp, vp, vp, vp, vp, ci, vp, vp, cf, vp, vp, ci, ci, ci, ci, vp]),
    "fp_ffn_layernorm_mean_fwd": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, cf, vp, vp, C.c_size_t, ci, ci, vp]),
    "fp_encoder_tail_workspace_bytes": (sz, [ci, ci]),
    "fp_encoder_tail_mean_fwd": (ci, [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, cf, vp, vp, sz, ci, ci, vp]),
    "fp_colmean_f16_fwd": (ci, [vp, vp, vp, vp, cf, vp, ci, ci, ci, vp]),
    "fp_rows_linear_fwd": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "fp_attention_f16_fwd": (ci, [vp, vp, ci, ci, ci, ci, ci, vp]),
    "fp_attention_segments_f16_fwd": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, vp]),
    "fp_cluster_poses": (ci, [cf, cf, vp, ci, vp, ci, vp]),
}


class FpAmdError(RuntimeError):
    pass


def lib():
    """Load libfp_amd.so or raise (build it with `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FpAmdError(
                f"{LIB_PATH} is missing: the HIP extension is not built (run __graft_entry__.build() or "
                f"`make -C foundationpose_amd/csrc`). There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is absent: loud by design
            fn.restype = res
            fn.argtypes = args
        got = int(handle.fp_version())
        if got != ABI_VERSION:
            raise FpAmdError(f"{LIB_PATH} reports ABI version {got}, this binding was written for {ABI_VERSION}: rebuild the library "
                             f"(`make -C foundationpose_amd/csrc`) -- entry points changed meaning between versions (include/fp_amd.h)")
        _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().fp_last_error()
        raise FpAmdError(f"{what} failed ({status}): {msg.decode() if msg else '?'}")
