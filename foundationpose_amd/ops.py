"""torch-tensor front-end of the C ABI (device pointers + current HIP stream).  Plumbing only."""
import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib

FLAG_NORMALIZE_XYZ = 1
FLAG_OUT_F16 = 2
MODE_REFINE = 0
MODE_SCORE = 1
ROT_AXIS_ANGLE = 0
ROT_6D = 1
TRANS_TRACKNET, TRANS_DEEPIM, TRANS_RAW = 0, 1, 2


def _stream(t=None):
    """HIP stream the launch goes to: PyTorch's current stream of the tensor's device.  A tensor on another device than
    the thread's current one is refused (launches go to the current device): use torch.cuda.set_device / torch.cuda.device."""
    if t is None:
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dev = t.device
    if dev.index is not None and dev.index != torch.cuda.current_device():
        raise _lib.FpAmdError(f"tensor on {dev} but the current device is cuda:{torch.cuda.current_device()}: wrap the call in "
                              f"`with torch.cuda.device({dev.index}):` (kernels launch on the current device)")
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _dev(t, dtype, name):
    if t is None:
        return None
    if not (torch.is_tensor(t) and t.is_cuda):
        raise _lib.FpAmdError(f"{name}: expected a CUDA(HIP) tensor; there is no CPU path in foundationpose_amd")
    if t.dtype != dtype:
        raise _lib.FpAmdError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.FpAmdError(f"{name}: tensor must be contiguous")
    return t


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _overlap(a, b):
    """do the bytes of two contiguous tensors intersect (None: no)"""
    if not (torch.is_tensor(a) and torch.is_tensor(b)) or a.device != b.device or a.numel() == 0 or b.numel() == 0:
        return False
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _hostK64(K):
    return np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(9))


def _hostK32(K):
    if torch.is_tensor(K):
        K = K.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(9).astype(np.float32))


class MeshHandle:
    """Device mesh tensors + the fp_mesh handle (Utils.py:104-130 make_mesh_tensors)."""

    def __init__(self, pos, vnormals, faces, uv=None, uv_idx=None, tex=None, vertex_color=None):
        self.pos = _dev(pos, torch.float32, "pos")
        self.vnormals = _dev(vnormals, torch.float32, "vnormals")
        self.faces = _dev(faces, torch.int32, "faces")
        self.uv = _dev(uv, torch.float32, "uv")
        self.uv_idx = _dev(uv_idx, torch.int32, "uv_idx")
        self.tex = _dev(tex, torch.float32, "tex")
        self.vertex_color = _dev(vertex_color, torch.float32, "vertex_color")
        self.V, self.T = int(pos.shape[0]), int(faces.shape[0])
        Ht = Wt = 0
        if self.tex is not None:
            Ht, Wt = int(self.tex.shape[-3]), int(self.tex.shape[-2])
        h = C.c_void_p()
        st = _lib.lib().fp_mesh_create(_ptr(self.pos), _ptr(self.vnormals), _ptr(self.faces), _ptr(self.uv),
                                       _ptr(self.uv_idx), _ptr(self.tex), _ptr(self.vertex_color), self.V, self.T,
                                       Ht, Wt, C.byref(h))
        _lib.check(st, "fp_mesh_create")
        self.handle = h
        self.device = self.pos.device

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.lib().fp_mesh_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class MeshSet:
    """Several objects' meshes for one call (fp_mesh_set): the descriptors of `handles` (MeshHandle) in one device table, built
    once.  Where render_crops takes a MeshHandle it takes a MeshSet with a per-hypothesis object index `obj` (int32 device tensor,
    values 0..M-1) and the per-object diameters (object_diameters).  V / T are the largest of the set: what sizes the grids and the
    rasteriser scratch (workspace_bytes(N, set.V, set.T, ...))."""

    def __init__(self, handles):
        self.meshes = list(handles)           # the set points at their tensors: keep them alive
        if not self.meshes:
            raise _lib.FpAmdError("MeshSet: empty list of meshes")
        devs = {h.device for h in self.meshes}
        if len(devs) != 1:
            raise _lib.FpAmdError(f"MeshSet: meshes on several devices {sorted(map(str, devs))}")
        self.device = self.meshes[0].device
        self.M = len(self.meshes)
        self.V = max(h.V for h in self.meshes)
        self.T = max(h.T for h in self.meshes)
        arr = (C.c_void_p * self.M)(*[h.handle.value for h in self.meshes])
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().fp_mesh_set_create(arr, self.M, C.byref(h)), "fp_mesh_set_create")
        self.handle = h

    def workspace_bytes(self, N, oh=160, ow=160):
        return int(_lib.lib().fp_mesh_set_workspace_bytes(self.handle, int(N), int(oh), int(ow)))

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.lib().fp_mesh_set_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def object_diameters(diameters, device):
    """the per-object diameter table of the multi-object entry points: (M,) float64 on `device`, the values exactly as the scalar
    entry points receive them (fp_crop_windows takes the double, the others round it to float on the device as ops does here)"""
    return torch.tensor([float(d) for d in diameters], dtype=torch.float64, device=device)


def _objects(mesh_diameter, obj, what):
    """the multi-object form of an entry point: (diameter table, obj or None, M), or None for the scalar form"""
    if not torch.is_tensor(mesh_diameter):
        if obj is not None:
            raise _lib.FpAmdError(f"{what}: an object index needs the per-object diameters (object_diameters), not a scalar")
        return None
    d = _dev(mesh_diameter, torch.float64, f"{what}: diameters")
    if d.dim() != 1 or d.numel() < 1:
        raise _lib.FpAmdError(f"{what}: diameters must be a (M,) float64 tensor")
    M = int(d.numel())
    o = _dev(obj, torch.int32, f"{what}: obj")
    if o is None and M > 1:
        raise _lib.FpAmdError(f"{what}: {M} objects need a per-hypothesis object index obj")
    return d, o, M


class PairRows:
    """The rows of the reference's two-pose quirk in one call (predict_pose_refine.two_pose_pairs) as a device table, built once from
    host data so a captured refine loop copies nothing.  pairs: sorted [(i, j)]"""

    def __init__(self, pairs, device):
        self.pairs = list(pairs)
        self._pairs_dev = torch.as_tensor(np.asarray(self.pairs, dtype=np.int64).reshape(-1, 2), device=device)
        self._first = np.asarray([i for i, _ in self.pairs], dtype=np.int64)

    def pair_rows(self, a, b):
        """(P, 2) device rows of the quirk pairs inside rows a..b, relative to a; None when there are none (parts_for_pairs keeps a
        pair from straddling two parts)"""
        k0, k1 = int(np.searchsorted(self._first, a)), int(np.searchsorted(self._first, b))
        if k0 == k1:
            return None
        return self._pairs_dev[k0:k1] - a


class Views:
    """The view table of a call over several camera frames of one size (the Ks / view / V of the C ABI): hypothesis n reads frame
    view[n] of the frame stacks and the intrinsics Ks[view[n]].  Built once from host data, like predict_pose_refine.ObjectIndex and Segments:
    the (V, 9) K tables in float64 (crop windows, back-projection) and float32 (render, warp, pose update) -- exactly the values the
    single-view paths pass from the host -- and the int32 device index (None for one view without an index: all hypotheses view 0).
    `pairs` / pair_rows: the two-pose quirk grouped per view (every hypothesis one object; with several objects the ObjectIndex built
    with view=... carries the (view, object) grouping)."""

    def __init__(self, Ks, view, device):
        Ks = [np.asarray(K, dtype=np.float64).reshape(-1) for K in Ks]
        if not Ks:
            raise _lib.FpAmdError("Views: no intrinsics (need V >= 1)")
        if any(K.size != 9 for K in Ks):
            raise _lib.FpAmdError("Views: every K must be a 3x3 matrix")
        self.V = len(Ks)
        if view is None:
            if self.V > 1:
                raise _lib.FpAmdError(f"Views: {self.V} views need a per-hypothesis view index")
            self.host = None
        else:
            self.host = np.asarray(view, dtype=np.int64).reshape(-1)
            if self.host.size and (self.host.min() < 0 or self.host.max() >= self.V):
                raise _lib.FpAmdError(f"Views: view index outside 0..{self.V - 1}")
        self.device = torch.device(device)
        self.K64 = torch.as_tensor(np.stack([_hostK64(K) for K in Ks]), device=self.device)
        self.K32 = torch.as_tensor(np.stack([_hostK32(K) for K in Ks]), device=self.device)
        self.dev = None if self.host is None else torch.as_tensor(self.host.astype(np.int32), device=self.device)
        self._rows = None
        if self.host is not None:
            from .predict_pose_refine import two_pose_pairs
            self._rows = PairRows(two_pose_pairs(np.zeros_like(self.host), self.host), self.device)

    def __len__(self):
        return 0 if self.host is None else int(self.host.size)

    @property
    def pairs(self):
        return [] if self._rows is None else self._rows.pairs

    def pair_rows(self, a, b):
        return None if self._rows is None else self._rows.pair_rows(a, b)

    def _cut(self, host, dev):
        v = object.__new__(Views)
        v.__dict__.update(self.__dict__, host=host, dev=dev, _rows=None)
        return v

    def rows(self, a, b):
        """the table for hypotheses a..b of the call (shares the K tables; the index is a slice: nothing is copied)"""
        return self._cut(None, None) if self.host is None else self._cut(self.host[a:b], self.dev[a:b])

    def take(self, idx):
        """the table for the hypotheses idx (host indices into this table's rows; shares the K tables, uploads the gathered index)"""
        host = None if self.host is None else self.host[np.asarray(idx, dtype=np.int64)]
        return self._cut(host, None if host is None else torch.as_tensor(host.astype(np.int32), device=self.device))


def _views(views, what, N=None):
    if not isinstance(views, Views):
        raise _lib.FpAmdError(f"{what}: views must be an ops.Views")
    if N is not None and views.dev is not None and int(views.dev.numel()) != N:
        raise _lib.FpAmdError(f"{what}: {N} hypotheses but a view index of {views.dev.numel()}")
    return views


def _scene(what, N, K, mesh_diameter, obj, views, k64=False, need_K=True):
    """The scene of a crop-stage call as the flat arguments its entry point takes (include/fp_amd.h, "The crop stage"):
    camera = (K, Ks, view, V), one host K (float64 for crop windows, else float32; NULL when not needed) or the tables of an
    ops.Views, and objects = (mesh_diameter, diameters, obj, M), one scalar or the table of object_diameters with the per-hypothesis
    index.  Views go with the table."""
    objs = _objects(mesh_diameter, obj, what)
    if views is not None:
        vt = _views(views, what, N)
        if objs is None:
            raise _lib.FpAmdError(f"{what}: views need the per-object diameter table (object_diameters), not a scalar")
        camera = (None, _ptr(vt.K64 if k64 else vt.K32), _ptr(vt.dev), vt.V)
    else:
        Kh = (_hostK64 if k64 else _hostK32)(K) if need_K else None
        camera = (None if Kh is None else Kh.ctypes.data_as(C.c_void_p), None, None, 0)    # the pointer object keeps Kh alive
    if objs is None:
        return camera, (float(mesh_diameter) if k64 else float(np.float32(mesh_diameter)), None, None, 0)
    d, o, M = objs
    return camera, (0.0, _ptr(d), _ptr(o), M)


def erode_depth(depth, radius=2, depth_diff_thres=0.001, ratio_thres=0.8, zfar=100.0):
    d = _dev(depth, torch.float32, "depth")
    out = torch.empty_like(d)
    H, W = d.shape
    _lib.check(_lib.lib().fp_depth_erode(_ptr(d), _ptr(out), H, W, int(radius), depth_diff_thres, ratio_thres, zfar,
                                         _stream(d)), "fp_depth_erode")
    return out


def bilateral_filter_depth(depth, radius=2, zfar=100.0, sigmaD=2.0, sigmaR=100000.0):
    d = _dev(depth, torch.float32, "depth")
    out = torch.empty_like(d)
    H, W = d.shape
    _lib.check(_lib.lib().fp_depth_bilateral(_ptr(d), _ptr(out), H, W, int(radius), zfar, sigmaD, sigmaR, _stream(d)),
               "fp_depth_bilateral")
    return out


def depth_to_xyz(depth, K, zfar=float("inf"), f64_internal=False):
    d = _dev(depth, torch.float32, "depth")
    H, W = d.shape
    out = torch.empty((H, W, 3), dtype=torch.float32, device=d.device)
    Kd = _hostK64(K)
    _lib.check(_lib.lib().fp_depth_to_xyz(_ptr(d), Kd.ctypes.data_as(C.c_void_p), float(zfar), int(bool(f64_internal)),
                                          _ptr(out), H, W, _stream(d)), "fp_depth_to_xyz")
    return out


def ingest_frame(depth, K, f64_internal=False):
    """the tracking ingest (erode -> bilateral -> back-projection, estimater.py:255-257) of one (H,W) depth frame in the three
    one-frame launches -> xyz (H,W,3); ingest_frames is the same for a stack"""
    d = bilateral_filter_depth(erode_depth(depth, radius=2), radius=2)
    return depth_to_xyz(d, K, zfar=float("inf"), f64_internal=f64_internal)     # f64_internal=False: the depth2xyzmap_batch variant


def _frames(t, what, ndim):
    d = _dev(t, torch.float32, what)
    if d.dim() != ndim:
        raise _lib.FpAmdError(f"{what}: expected a {ndim}-d frame stack, got shape {tuple(d.shape)}")
    return d


def erode_depth_frames(depth, radius=2, depth_diff_thres=0.001, ratio_thres=0.8, zfar=100.0):
    """erode_depth on every frame of a (V,H,W) stack, one launch (fp_depth_erode_frames)"""
    d = _frames(depth, "depth", 3)
    out = torch.empty_like(d)
    V, H, W = d.shape
    _lib.check(_lib.lib().fp_depth_erode_frames(_ptr(d), _ptr(out), H, W, V, int(radius), depth_diff_thres, ratio_thres, zfar,
                                                _stream(d)), "fp_depth_erode_frames")
    return out


def bilateral_filter_depth_frames(depth, radius=2, zfar=100.0, sigmaD=2.0, sigmaR=100000.0):
    """bilateral_filter_depth on every frame of a (V,H,W) stack, one launch (fp_depth_bilateral_frames)"""
    d = _frames(depth, "depth", 3)
    out = torch.empty_like(d)
    V, H, W = d.shape
    _lib.check(_lib.lib().fp_depth_bilateral_frames(_ptr(d), _ptr(out), H, W, V, int(radius), zfar, sigmaD, sigmaR, _stream(d)),
               "fp_depth_bilateral_frames")
    return out


def depth_to_xyz_frames(depth, views, zfar=float("inf"), f64_internal=False):
    """depth_to_xyz of frame v of a (V,H,W) stack with K = views' K v (fp_depth_to_xyz_frames) -> (V,H,W,3)"""
    d = _frames(depth, "depth", 3)
    vt = _views(views, "depth_to_xyz_frames")
    V, H, W = d.shape
    if V != vt.V:
        raise _lib.FpAmdError(f"depth_to_xyz_frames: {V} frames but {vt.V} views")
    out = torch.empty((V, H, W, 3), dtype=torch.float32, device=d.device)
    _lib.check(_lib.lib().fp_depth_to_xyz_frames(_ptr(d), _ptr(vt.K64), float(zfar), int(bool(f64_internal)), _ptr(out), H, W, V,
                                                 _stream(d)), "fp_depth_to_xyz_frames")
    return out


def ingest_frames(depth, views, f64_internal=False):
    """the tracking ingest (erode -> bilateral -> back-projection, estimater.py:255-257) of a (V,H,W) depth stack in three launches
    -> xyz (V,H,W,3)"""
    d = bilateral_filter_depth_frames(erode_depth_frames(depth, radius=2), radius=2)
    return depth_to_xyz_frames(d, views, zfar=float("inf"), f64_internal=f64_internal)


def mask_depth_stats(depth, masks, view=None, min_depth=0.001):
    """the statistics of estimater.guess_translation and register()'s valid-depth count for M masks in one launch
    (fp_mask_depth_stats): depth a (V,H,W) f32 stack, masks (M,H,W) uint8 (nonzero = inside), view the (M,) int32 device frame index of
    every mask (None for one frame) -> (M, 8) int32 device tensor, per mask [v0, v1, u0, u1, n, lo, hi, 0]: the bounding box (-1 when
    the mask is empty), the count n of depths >= min_depth inside, and as float32 bits the (n-1)//2-th and n//2-th smallest of them
    (NaN when n == 0).  One device-to-host copy of it serves every mask (mask_depth_stats_host)."""
    d = _frames(depth, "depth", 3)
    mk = _dev(masks, torch.uint8, "masks")
    if mk.dim() != 3 or tuple(mk.shape[1:]) != tuple(d.shape[1:]):
        raise _lib.FpAmdError(f"mask_depth_stats: masks must be (M,{d.shape[1]},{d.shape[2]}), got {tuple(mk.shape)}")
    V, H, W = (int(x) for x in d.shape)
    M = int(mk.shape[0])
    vw = _dev(view, torch.int32, "view")
    if vw is not None and int(vw.numel()) != M:
        raise _lib.FpAmdError(f"mask_depth_stats: {M} masks but a view index of {vw.numel()}")
    out = torch.empty((M, 8), dtype=torch.int32, device=d.device)
    _lib.check(_lib.lib().fp_mask_depth_stats(_ptr(d), _ptr(mk), _ptr(vw), V, M, H, W, float(min_depth), _ptr(out), _stream(d)),
               "fp_mask_depth_stats")
    return out


def mask_depth_stats_host(stats):
    """mask_depth_stats' table on the host (one copy) -> (box (M,4) int64 [v0, v1, u0, u1], n (M,) int64, lo (M,) f32, hi (M,) f32)"""
    a = np.ascontiguousarray(stats.cpu().numpy() if torch.is_tensor(stats) else np.asarray(stats, dtype=np.int32))
    return a[:, :4].astype(np.int64), a[:, 4].astype(np.int64), a[:, 5].view(np.float32).copy(), a[:, 6].view(np.float32).copy()


def crop_windows(poses, K, mesh_diameter, crop_ratio, out_size=(160, 160), obj=None, views=None):
    """-> tf_to_crops (N,3,3) f32, bbox2d (N,4) f32 (fp_crop_windows).  out_size = (width, height).  Several objects: mesh_diameter =
    the (M,) table of object_diameters, obj = the per-hypothesis object index.  Several views: views = an ops.Views (K unused)."""
    P = _dev(poses, torch.float32, "poses")
    N = int(P.shape[0])
    tf = torch.empty((N, 3, 3), dtype=torch.float32, device=P.device)
    bb = torch.empty((N, 4), dtype=torch.float32, device=P.device)
    (Kp, Ks, view, V), (dia, d, o, M) = _scene("crop_windows", N, K, mesh_diameter, obj, views, k64=True)
    _lib.check(_lib.lib().fp_crop_windows(_ptr(P), Kp, Ks, view, V, dia, d, o, M, float(crop_ratio), int(out_size[0]),
                                          int(out_size[1]), N, _ptr(tf), _ptr(bb), _stream(P)), "fp_crop_windows")
    return tf, bb


_WS = {}


def workspace_bytes(N, V, T, oh=160, ow=160):
    return int(_lib.lib().fp_workspace_bytes(int(N), int(V), int(T), int(oh), int(ow)))


def _workspace(nbytes, device):
    """library-side default scratch: one per (device, stream) -- launches on different streams may overlap.

    Inside a stream capture the stream-keyed scratch is NEVER handed out (round 5, the advisor's finding: torch.cuda.graph uses one
    shared capture stream, so two graphs captured one after the other baked in the SAME scratch address; replayed on different
    streams -- the PartGraphs pattern -- they raced on it and tri_id / zbuf came out silently wrong).  A capture without a caller-owned
    `workspace` gets a fresh allocation made inside the capture: it comes from the capturing graph's private pool, lives exactly as
    long as that graph, and no other graph or eager launch can hold its address."""
    if nbytes == 0:
        return None
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _WS[key] = ws
    return ws


def render_crops(mesh, poses, bbox2d, K, H, W, out_hw=(160, 160), mesh_diameter=1.0, xyz_thr=0.001,
                 normalize_xyz=True, out_f16=False, w_ambient=0.8, w_diffuse=0.5,
                 want=("A",), A_out=None, workspace=None, obj=None, views=None):
    """Fused render of N hypotheses (see fp_render_crops).  Returns dict of requested outputs.  workspace: caller-owned
    uint8 scratch of at least workspace_bytes(...) bytes (a captured hipGraph must own its scratch); default: a
    per-device scratch that grows on demand.  Several objects: mesh = a MeshSet, obj = the per-hypothesis object index, mesh_diameter =
    the (M,) table of object_diameters (hypothesis n draws mesh obj[n]).  Several views: views = an ops.Views with a MeshSet (K
    unused: hypothesis n projects with K view[n])."""
    multi = isinstance(mesh, MeshSet)
    if views is not None and not multi:
        raise _lib.FpAmdError("render_crops: views need a MeshSet")
    if multi and not (torch.is_tensor(mesh_diameter) and mesh_diameter.dim() == 1 and mesh_diameter.numel() == mesh.M):
        raise _lib.FpAmdError(f"render_crops: a MeshSet of {mesh.M} meshes needs a ({mesh.M},) diameter table")
    if not multi and obj is not None:
        raise _lib.FpAmdError("render_crops: an object index needs a MeshSet")
    P = _dev(poses, torch.float32, "poses")
    N = int(P.shape[0])
    (Kp, Ks, view, V), (dia, d, o, _) = _scene("render_crops", N, K, mesh_diameter if multi else float(mesh_diameter), obj, views)
    bb = _dev(bbox2d, torch.float32, "bbox2d")
    oh, ow = int(out_hw[0]), int(out_hw[1])
    dev = P.device
    outs = {}

    def alloc(name, shape, dt):
        if name in want:
            outs[name] = torch.empty(shape, dtype=dt, device=dev)
            return outs[name]
        return None

    if A_out is not None:
        A = A_out
        outs["A"] = A
    else:
        A = alloc("A", (N, 6, oh, ow), torch.float16 if out_f16 else torch.float32)
    color = alloc("color", (N, oh, ow, 3), torch.float32)
    depth = alloc("depth", (N, oh, ow), torch.float32)
    xyz = alloc("xyz", (N, oh, ow, 3), torch.float32)
    normal = alloc("normal", (N, oh, ow, 3), torch.float32)
    zbuf = alloc("zbuf", (N, oh, ow), torch.int32)  # u32 payload, viewed as int32 by torch
    tri = alloc("tri_id", (N, oh, ow), torch.int32)
    L = _lib.lib()
    need = mesh.workspace_bytes(N, oh, ow) if multi else L.fp_workspace_bytes(N, mesh.V, mesh.T, oh, ow)
    if workspace is not None:
        ws = _dev(workspace, torch.uint8, "workspace")
        if ws.numel() < need:
            raise _lib.FpAmdError(f"render_crops: workspace has {ws.numel()} bytes, {need} needed")
    else:
        ws = _workspace(need, dev)
    flags = (FLAG_NORMALIZE_XYZ if normalize_xyz else 0) | (FLAG_OUT_F16 if (A is not None and A.dtype == torch.float16) else 0)
    one, mset = (None, mesh.handle) if multi else (mesh.handle, None)
    st = L.fp_render_crops(one, mset, o, d, dia, _ptr(P), _ptr(bb), Kp, Ks, view, V, int(H), int(W), N, oh, ow, w_ambient, w_diffuse,
                           xyz_thr, flags, _ptr(A), _ptr(color), _ptr(depth), _ptr(xyz), _ptr(normal), _ptr(zbuf), _ptr(tri), _ptr(ws),
                           0 if ws is None else ws.numel(), _stream(P))
    _lib.check(st, "fp_render_crops")
    return outs


def warp_crops(rgb, xyz_map, depth, tf_to_crops, K, poses, mesh_diameter, mode, normalize_xyz=True, out_f16=False,
               out_hw=(160, 160), B_out=None, obj=None, views=None):
    """fp_warp_crops.  Several objects: mesh_diameter = the (M,) table of object_diameters, obj = the per-hypothesis object
    index.  Several views: views = an ops.Views, rgb / xyz_map / depth = (V,H,W,3) / (V,H,W,3) / (V,H,W) frame stacks (K unused)."""
    rgbf = _dev(rgb, torch.float32, "rgb")
    H, W = (int(rgbf.shape[0]), int(rgbf.shape[1])) if views is None else (int(rgbf.shape[1]), int(rgbf.shape[2]))
    xm = _dev(xyz_map, torch.float32, "xyz_map")
    dp = _dev(depth, torch.float32, "depth")
    tf = _dev(tf_to_crops, torch.float32, "tf_to_crops")
    P = _dev(poses, torch.float32, "poses")
    N = int(P.shape[0])
    oh, ow = int(out_hw[0]), int(out_hw[1])
    B = B_out if B_out is not None else torch.empty((N, 6, oh, ow), dtype=torch.float16 if out_f16 else torch.float32,
                                                    device=P.device)
    flags = (FLAG_NORMALIZE_XYZ if normalize_xyz else 0) | (FLAG_OUT_F16 if B.dtype == torch.float16 else 0)
    if views is not None and (rgbf.dim() != 4 or int(rgbf.shape[0]) != _views(views, "warp_crops", N).V):
        raise _lib.FpAmdError(f"warp_crops: views need a ({views.V},H,W,3) rgb stack, got {tuple(rgbf.shape)}")
    (Kp, Ks, view, V), (dia, d, o, M) = _scene("warp_crops", N, K, mesh_diameter, obj, views)
    st = _lib.lib().fp_warp_crops(_ptr(rgbf), _ptr(xm), _ptr(dp), _ptr(tf), Kp, Ks, view, V, _ptr(P), dia, d, o, M, flags, int(mode),
                                  H, W, N, oh, ow, _ptr(B), _stream(P))
    _lib.check(st, "fp_warp_crops")
    return B


def _check_tol(tol, what):
    """the tolerance of a depth-agreement check: a finite number >= 0 (metres), refused with ValueError before any device work"""
    try:
        t = float(tol)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: agreement tolerance must be a number, got {tol!r}") from None
    if not (np.isfinite(t) and t >= 0.0):
        raise ValueError(f"{what}: agreement tolerance must be finite and >= 0 (metres), got {tol!r}")
    return t


def depth_agreement(depth_crops, xyz_map, tf_to_crops, tol, views=None, out=None):
    """fp_depth_agreement: per hypothesis, how the render's depth crops (N,oh,ow) -- render_crops(want=("depth",)) at the pose through
    the crop windows tf_to_crops (N,3,3) -- agree with the observed xyz map (H,W,3) through the same windows (the texel the REFINE warp
    reads).  -> (N, 4) int32 device tensor [model, valid, agree, behind] (include/fp_amd.h); `tol` absolute, in metres.  out: a
    caller-owned (N, 4) int32 tensor to fill (a captured graph owns its output).  Several views: views = an ops.Views and xyz_map the
    (V,H,W,3) stack."""
    t = _check_tol(tol, "depth_agreement")
    dc = _dev(depth_crops, torch.float32, "depth_crops")
    xm = _dev(xyz_map, torch.float32, "xyz_map")
    tf = _dev(tf_to_crops, torch.float32, "tf_to_crops")
    if dc.dim() != 3:
        raise _lib.FpAmdError(f"depth_agreement: depth_crops must be (N,oh,ow), got {tuple(dc.shape)}")
    N, oh, ow = (int(x) for x in dc.shape)
    if tuple(tf.shape[-2:]) != (3, 3) or tf.numel() != 9 * N:
        raise _lib.FpAmdError(f"depth_agreement: {N} depth crops but tf_to_crops of shape {tuple(tf.shape)}")
    if views is not None:
        vt = _views(views, "depth_agreement", N)
        if xm.dim() != 4 or int(xm.shape[0]) != vt.V or int(xm.shape[3]) != 3:
            raise _lib.FpAmdError(f"depth_agreement: views need a ({vt.V},H,W,3) xyz stack, got {tuple(xm.shape)}")
        V, H, W = int(xm.shape[0]), int(xm.shape[1]), int(xm.shape[2])
        vw = vt.dev
    else:
        if xm.dim() != 3 or int(xm.shape[2]) != 3:
            raise _lib.FpAmdError(f"depth_agreement: xyz_map must be (H,W,3), got {tuple(xm.shape)}")
        V, H, W = 1, int(xm.shape[0]), int(xm.shape[1])
        vw = None
    if out is None:
        out = torch.empty((N, 4), dtype=torch.int32, device=dc.device)
    else:
        out = _dev(out, torch.int32, "out")
        if tuple(out.shape) != (N, 4):
            raise _lib.FpAmdError(f"depth_agreement: out must be ({N}, 4), got {tuple(out.shape)}")
    _lib.check(_lib.lib().fp_depth_agreement(_ptr(dc), _ptr(xm), _ptr(tf), _ptr(vw), V, H, W, N, oh, ow, t, _ptr(out), _stream(dc)),
               "fp_depth_agreement")
    return out


class DepthAgreement(NamedTuple):
    """one row of depth_agreement's table on the host: crop pixels the model covers (`model`), those of them with an observed depth
    (`valid`), those whose observed depth is within tol of the model's (`agree`) and those where the sensor sees more than tol past the
    model's surface (`behind`).  `front` = valid - agree - behind: something in front of the model.  A fraction over 0 is NaN."""
    model: int
    valid: int
    agree: int
    behind: int

    @property
    def front(self):
        return self.valid - self.agree - self.behind

    @staticmethod
    def _frac(a, b):
        return a / b if b else float("nan")

    @property
    def valid_frac(self):
        return self._frac(self.valid, self.model)

    @property
    def agree_frac(self):
        return self._frac(self.agree, self.valid)

    @property
    def behind_frac(self):
        return self._frac(self.behind, self.valid)

    @classmethod
    def rows(cls, table):
        """[DepthAgreement] per row of a (N, 4) table (a device tensor: one device-to-host copy)"""
        a = table.cpu().numpy() if torch.is_tensor(table) else np.asarray(table)
        return [cls(*(int(x) for x in r)) for r in np.asarray(a, dtype=np.int64).reshape(-1, 4)]


def _check_icp(max_dist, damping, min_pairs, what):
    """the numbers of an ICP step: max_dist (metres) and damping finite and >= 0, min_pairs an int >= 6; refused with ValueError
    before any device work"""
    vals = []
    for name, v in (("max_dist", max_dist), ("damping", damping)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: {name} must be a number, got {v!r}") from None
        if not (np.isfinite(f) and f >= 0.0):
            raise ValueError(f"{what}: {name} must be finite and >= 0, got {v!r}")
        vals.append(f)
    if isinstance(min_pairs, bool) or not isinstance(min_pairs, (int, np.integer)) or int(min_pairs) < 6:
        raise ValueError(f"{what}: min_pairs must be an int >= 6 (the unknowns of a step), got {min_pairs!r}")
    return vals[0], vals[1], int(min_pairs)


def icp_workspace(N, oh, ow, device):
    """the workspace of icp_point_plane for N hypotheses at (oh, ow) crops (a captured graph owns its buffers)"""
    nbytes = int(_lib.lib().fp_icp_workspace_bytes(int(N), int(oh), int(ow)))
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=device)


def icp_point_plane(xyz_crops, normal_crops, xyz_map, tf_to_crops, poses, max_dist, damping=1e-3, min_pairs=64, views=None,
                    system=None, poses_out=None, workspace=None):
    """fp_icp_point_plane: one Gauss-Newton step of point-to-plane ICP per hypothesis.  xyz_crops / normal_crops (N,oh,ow,3): the
    render of the model at `poses` (N,4,4) through the crop windows tf_to_crops (N,3,3) -- render_crops(want=("xyz", "normal"),
    normalize_xyz=False); xyz_map (H,W,3): the observed points, read through the same windows as depth_agreement reads them.  Pairs
    farther apart than max_dist (metres) are dropped; damping scales diag(A); fewer than min_pairs pairs leave the pose as it is.
    -> (poses_out (N,4,4) f32, system (N,40) f64) device tensors; IcpStep.rows reads `system` on the host (include/fp_amd.h has the
    definition and the layout).  system / poses_out / workspace: caller-owned buffers ((N,40) float64; (N,4,4) float32, not
    overlapping `poses`; icp_workspace) for a captured graph.  Several views: views = an ops.Views and xyz_map the (V,H,W,3) stack."""
    md, dmp, mp = _check_icp(max_dist, damping, min_pairs, "icp_point_plane")
    xc = _dev(xyz_crops, torch.float32, "xyz_crops")
    nc = _dev(normal_crops, torch.float32, "normal_crops")
    xm = _dev(xyz_map, torch.float32, "xyz_map")
    tf = _dev(tf_to_crops, torch.float32, "tf_to_crops")
    P = _dev(poses, torch.float32, "poses")
    if xc.dim() != 4 or int(xc.shape[3]) != 3:
        raise _lib.FpAmdError(f"icp_point_plane: xyz_crops must be (N,oh,ow,3), got {tuple(xc.shape)}")
    N, oh, ow = (int(x) for x in xc.shape[:3])
    if tuple(nc.shape) != tuple(xc.shape):
        raise _lib.FpAmdError(f"icp_point_plane: normal_crops must be {tuple(xc.shape)} like xyz_crops, got {tuple(nc.shape)}")
    if tuple(tf.shape[-2:]) != (3, 3) or tf.numel() != 9 * N:
        raise _lib.FpAmdError(f"icp_point_plane: {N} crops but tf_to_crops of shape {tuple(tf.shape)}")
    if tuple(P.shape) != (N, 4, 4):
        raise _lib.FpAmdError(f"icp_point_plane: {N} crops but poses of shape {tuple(P.shape)}")
    if views is not None:
        vt = _views(views, "icp_point_plane", N)
        if xm.dim() != 4 or int(xm.shape[0]) != vt.V or int(xm.shape[3]) != 3:
            raise _lib.FpAmdError(f"icp_point_plane: views need a ({vt.V},H,W,3) xyz stack, got {tuple(xm.shape)}")
        V, H, W = int(xm.shape[0]), int(xm.shape[1]), int(xm.shape[2])
        vw = vt.dev
    else:
        if xm.dim() != 3 or int(xm.shape[2]) != 3:
            raise _lib.FpAmdError(f"icp_point_plane: xyz_map must be (H,W,3), got {tuple(xm.shape)}")
        V, H, W = 1, int(xm.shape[0]), int(xm.shape[1])
        vw = None
    if system is None:
        system = torch.empty((N, 40), dtype=torch.float64, device=xc.device)
    else:
        system = _dev(system, torch.float64, "system")
        if tuple(system.shape) != (N, 40):
            raise _lib.FpAmdError(f"icp_point_plane: system must be ({N}, 40), got {tuple(system.shape)}")
    if poses_out is None:
        poses_out = torch.empty((N, 4, 4), dtype=torch.float32, device=xc.device)
    else:
        poses_out = _dev(poses_out, torch.float32, "poses_out")
        if tuple(poses_out.shape) != (N, 4, 4):
            raise _lib.FpAmdError(f"icp_point_plane: poses_out must be ({N}, 4, 4), got {tuple(poses_out.shape)}")
        if _overlap(poses_out, P):
            raise _lib.FpAmdError("icp_point_plane: poses_out must not overlap poses (there is no in-place update)")
    need = int(_lib.lib().fp_icp_workspace_bytes(N, oh, ow))
    if workspace is None:
        workspace = icp_workspace(N, oh, ow, xc.device)
    else:
        if not (torch.is_tensor(workspace) and workspace.is_cuda and workspace.is_contiguous()):
            raise _lib.FpAmdError("icp_point_plane: workspace must be a contiguous CUDA(HIP) tensor")
        if workspace.numel() * workspace.element_size() < need:
            raise _lib.FpAmdError(f"icp_point_plane: workspace of {workspace.numel() * workspace.element_size()} bytes, {need} needed "
                                  f"(icp_workspace)")
    _lib.check(_lib.lib().fp_icp_point_plane(_ptr(xc), _ptr(nc), _ptr(xm), _ptr(tf), _ptr(vw), V, H, W, _ptr(P), N, oh, ow, md, dmp, mp,
                                             _ptr(system), _ptr(poses_out), _ptr(workspace),
                                             workspace.numel() * workspace.element_size(), _stream(xc)), "fp_icp_point_plane")
    return poses_out, system


class IcpStep(NamedTuple):
    """one row of icp_point_plane's `system` on the host: `pairs` the model / sensor point pairs the step was solved over, `rms` their
    point-to-plane RMS BEFORE the step in metres (NaN without pairs), `status` 0 solved / 1 fewer than min_pairs pairs / 2 degenerate
    (a pivot of the factorisation <= 0 or a non-finite pose), `twist` the step (w0, w1, w2, v0, v1, v2): rotation vector in radians
    about the pose's origin and translation in metres, zeros unless status is 0."""
    pairs: int
    rms: float
    status: int
    twist: tuple

    @classmethod
    def rows(cls, table):
        """[IcpStep] per row of a (N, 40) system (a device tensor: one device-to-host copy)"""
        a = table.cpu().numpy() if torch.is_tensor(table) else np.asarray(table)
        a = np.asarray(a, dtype=np.float64).reshape(-1, 40)
        return [cls(int(r[28]), float(np.sqrt(r[27] / r[28])) if r[28] > 0 else float("nan"), int(r[29]),
                    tuple(float(x) for x in r[30:36])) for r in a]


_POSE_ERROR_FLAGS = {"add": 1, "adds": 2, "sym": 4}     # FP_ERR_ADD / FP_ERR_ADDS / FP_ERR_SYM (include/fp_amd.h)


def _tf_table(t, name, what="pose_errors"):
    """a (n,4,4) / (4,4) table of transforms, numpy or tensor of any float type -> a (n,4,4) float tensor where it lives (shape and
    type refused here, before any device work)"""
    if torch.is_tensor(t):
        a = t.detach()
    else:
        a = np.asarray(t)
        if a.dtype.kind in "iub":
            a = a.astype(np.float64)
        if a.dtype.kind != "f":
            raise _lib.FpAmdError(f"{what}: {name} must be of a float type, got {a.dtype}")
        a = torch.from_numpy(np.ascontiguousarray(a))
    if not a.is_floating_point():
        raise _lib.FpAmdError(f"{what}: {name} must be of a float type, got {a.dtype}")
    if a.dim() == 2:
        a = a[None]
    if a.dim() != 3 or tuple(a.shape[1:]) != (4, 4):
        raise _lib.FpAmdError(f"{what}: {name} must be (4,4) or (n,4,4), got {tuple(a.shape)}")
    return a


def _pose_tables(what, model_pts, poses, gt, gt_index, symmetry_tfs):
    """the shape refusals pose_errors and mspd share, in their one order (they need no device): model_pts (P,3), poses (N,4,4), the
    gt_index length, the gt table against N, the symmetry table -> (N, P, gt (G,4,4), G, symmetries (S,4,4) or None, S)"""
    for name, t in (("model_pts", model_pts), ("poses", poses)):
        if not torch.is_tensor(t):
            raise _lib.FpAmdError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if model_pts.dim() != 2 or int(model_pts.shape[1]) != 3 or int(model_pts.shape[0]) < 1:
        raise _lib.FpAmdError(f"{what}: model_pts must be (P,3) with P >= 1, got {tuple(model_pts.shape)}")
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4):
        raise _lib.FpAmdError(f"{what}: poses must be (N,4,4), got {tuple(poses.shape)}")
    N, P = int(poses.shape[0]), int(model_pts.shape[0])
    if gt_index is not None and (not torch.is_tensor(gt_index) or int(gt_index.numel()) != N):
        raise _lib.FpAmdError(f"{what}: {N} poses need a gt_index tensor of {N} entries")
    g = _tf_table(gt, "gt", what)
    G = int(g.shape[0])
    if G < 1 or (gt_index is None and G not in (1, N)):
        raise _lib.FpAmdError(f"{what}: {G} ground truths for {N} poses need a gt_index")
    sym = None if symmetry_tfs is None else _tf_table(symmetry_tfs, "symmetry_tfs", what)
    return N, P, g, G, sym, 0 if sym is None else int(sym.shape[0])


def _pose_operands(what, model_pts, poses, gt_index, out, out_shape):
    """the device / dtype / layout refusals that follow them -> (model_pts, poses, gt_index, out) as the kernels take them"""
    pts = _dev(model_pts, torch.float32, "model_pts")
    ps = _dev(poses, torch.float32, "poses")
    gi = _dev(gt_index, torch.int32, "gt_index")
    if out is not None:
        out = _dev(out, torch.float64, "out")
        if tuple(out.shape) != out_shape:
            raise _lib.FpAmdError(f"{what}: out must be {out_shape}, got {tuple(out.shape)}")
    return pts, ps, gi, out


def pose_errors_workspace(N, P, S, device):
    """the workspace of pose_errors for N poses, P model points and S symmetries (a captured graph owns its buffers)"""
    nbytes = int(_lib.lib().fp_pose_errors_workspace_bytes(int(N), int(P), int(S)))
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=device)


def pose_errors(model_pts, poses, gt, gt_index=None, symmetry_tfs=None, want=("add", "adds"), out=None, workspace=None):
    """fp_pose_errors: how far each of the N poses (N,4,4) f32 is from its ground truth, over the model points (P,3) f32 ->
    (N, 4) float64 device tensor [add, adds, add_sym, mssd] in metres (include/fp_amd.h has the definition; PoseErrors.rows reads it
    on the host).  gt: (4,4) or (G,4,4), numpy or tensor; gt_index: the (N,) int32 device index of every pose's ground truth (None:
    all against the one for G == 1, pose n against gt n for G == N).  want: names out of "add", "adds", "sym" ("sym" = add_sym and
    mssd over symmetry_tfs (S,4,4)); the other columns are NaN.  Poses, ground truths, symmetries and points share one object frame.
    out / workspace: caller-owned buffers ((N,4) float64; pose_errors_workspace) for a captured graph.  Wrong shapes and tables are
    refused first, then tensors that are not on the device, of another dtype or not contiguous, then the buffers (FpAmdError)."""
    names = (want,) if isinstance(want, str) else tuple(want)
    flags = 0
    for w in names:
        if w not in _POSE_ERROR_FLAGS:
            raise ValueError(f"pose_errors: unknown name {w!r} in want (known: {sorted(_POSE_ERROR_FLAGS)})")
        flags |= _POSE_ERROR_FLAGS[w]
    if not flags:
        raise ValueError("pose_errors: want is empty")
    # shapes first (they need no device), then device / dtype / layout, then the buffers: all before any device work
    N, P, g, G, sym, S = _pose_tables("pose_errors", model_pts, poses, gt, gt_index, symmetry_tfs)
    if flags & 4 and S == 0:
        raise _lib.FpAmdError('pose_errors: want "sym" needs symmetry_tfs with at least one transform')
    pts, ps, gi, out = _pose_operands("pose_errors", model_pts, poses, gt_index, out, (N, 4))
    need = int(_lib.lib().fp_pose_errors_workspace_bytes(N, P, S))
    if workspace is not None:
        if not (torch.is_tensor(workspace) and workspace.is_cuda and workspace.is_contiguous()):
            raise _lib.FpAmdError("pose_errors: workspace must be a contiguous CUDA(HIP) tensor")
        if workspace.numel() * workspace.element_size() < need:
            raise _lib.FpAmdError(f"pose_errors: workspace of {workspace.numel() * workspace.element_size()} bytes, {need} needed "
                                  f"(pose_errors_workspace)")
    g = g.to(device=ps.device, dtype=torch.float64).contiguous()          # float64 input never passes through float32
    sym = None if sym is None else sym.to(device=ps.device, dtype=torch.float64).contiguous()
    if out is None:
        out = torch.empty((N, 4), dtype=torch.float64, device=ps.device)
    if workspace is None:
        workspace = pose_errors_workspace(N, P, S, ps.device)
    _lib.check(_lib.lib().fp_pose_errors(_ptr(pts), P, _ptr(sym), S, _ptr(ps), _ptr(g), _ptr(gi), G, N, flags, _ptr(out),
                                         _ptr(workspace), workspace.numel() * workspace.element_size(), _stream(ps)),
               "fp_pose_errors")
    return out


class PoseErrors(NamedTuple):
    """one row of pose_errors' table on the host, in metres: `add` the mean distance of corresponding model points, `adds` the mean
    distance to the nearest point, `add_sym` / `mssd` the minimum over the symmetry set of the mean / the maximum corresponding
    distance.  NaN where a column was not computed."""
    add: float
    adds: float
    add_sym: float
    mssd: float

    @classmethod
    def rows(cls, table):
        """[PoseErrors] per row of a (N, 4) table (a device tensor: one device-to-host copy)"""
        a = table.cpu().numpy() if torch.is_tensor(table) else np.asarray(table)
        return [cls(*(float(x) for x in r)) for r in np.asarray(a, dtype=np.float64).reshape(-1, 4)]


MESH_DISTANCE_OUTPUTS = ("dist2", "face", "closest")
_MESH_DISTANCE_DTYPES = {"dist2": torch.float32, "face": torch.int32, "closest": torch.float32}


def _mesh_pos_faces(what, mesh_tensors, pos, faces):
    """the mesh of a call that takes mesh_tensors (a dict with pos and faces) or pos= and faces= themselves -> (pos, faces)"""
    if mesh_tensors is not None:
        if pos is not None or faces is not None:
            raise _lib.FpAmdError(f"{what}: pass mesh_tensors or pos / faces, not both")
        for k in ("pos", "faces"):
            if k not in mesh_tensors:
                raise _lib.FpAmdError(f"{what}: mesh_tensors has no '{k}'")
        pos, faces = mesh_tensors["pos"], mesh_tensors["faces"]
    if pos is None or faces is None:
        raise _lib.FpAmdError(f"{what}: no mesh (pass mesh_tensors, or pos and faces)")
    return pos, faces


def _mesh_names(what, want, known, always=(), required=False):
    """the outputs a mesh query makes, in the order of `known`: those named in want (a name or a sequence of names) and those in always"""
    names = (want,) if isinstance(want, str) else tuple(want)
    for w in names:
        if w not in known:
            raise ValueError(f"{what}: unknown name {w!r} in want (known: {list(known)})")
    if required and not names:
        raise ValueError(f"{what}: want is empty")
    return tuple(n for n in known if n in names or n in always)


def _mesh_n3(what, **tensors):
    for name, t in tensors.items():
        if not torch.is_tensor(t):
            raise _lib.FpAmdError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
        if t.dim() != 2 or int(t.shape[1]) != 3:
            raise _lib.FpAmdError(f"{what}: {name} must be (n,3), got {tuple(t.shape)}")


# the sizes a mesh query refuses, each with its own words (T is None in a call without transforms) -> the message, or None
def _mesh_limit_points(T, Q, F):
    if max(Q, F) > (1 << 30):
        return f"{Q} points against {F} faces (at most 2^30 of either)"
    return None


def _mesh_limit_pairs(T, Q, F):
    if T * Q > (1 << 30) or max(T, F) > (1 << 30):
        return f"{T} transforms of {Q} points against {F} faces (at most 2^30 pairs, transforms or faces)"
    return None


def _mesh_limit_signed(T, Q, F):
    if (T or 1) * Q > (1 << 30) or max(T or 0, Q, F) > (1 << 30):
        return f"{T or 1} x {Q} points against {F} faces (at most 2^30 pairs, transforms, points or faces)"
    return None


class _MeshCall(NamedTuple):
    """_mesh_call's result: the checked device tensors (tfs is None without pairs, vn and en without signed), the out dict with every
    output of the call in it, the workspace and its size, and the sizes (T is None without pairs)"""
    points: torch.Tensor
    tfs: Optional[torch.Tensor]
    pos: torch.Tensor
    faces: torch.Tensor
    vn: Optional[torch.Tensor]
    en: Optional[torch.Tensor]
    out: dict
    ws: torch.Tensor
    ws_bytes: int
    Q: int
    Nv: int
    F: int
    T: Optional[int]


def _mesh_call(what, points, tfs, mesh_tensors, pos, faces, out, *, names, dtypes, shapes_of, limit, workspace_bytes, pairs=False,
               among="the wanted outputs", signed=None, workspace=None, workspace_maker=None, points_name="points"):
    """What the mesh queries do before they call the library, in the documented order of refusals: the mesh (mesh_tensors or pos /
    faces); shapes: points, pos, faces (n,3) and, with pairs, tfs (T,4,4), the sizes `limit` refuses, with signed = (tables, allow_open)
    the pseudonormal tables, the names and shapes (shapes_of(T, Q)) of the caller's out buffers; device, dtype and contiguity of
    each; overlaps of an out buffer with an input or another; the caller's workspace (None: the per-stream scratch) against
    workspace_bytes(T, Q) and the out buffers (points_name: what the messages call `points`).  Then the outputs of `names` the
    caller did not give are allocated.  -> _MeshCall."""
    pos, faces = _mesh_pos_faces(what, mesh_tensors, pos, faces)
    _mesh_n3(what, **{points_name: points}, pos=pos, faces=faces)
    T = None
    if pairs:
        if not torch.is_tensor(tfs):
            raise _lib.FpAmdError(f"{what}: tfs must be a tensor, got {type(tfs).__name__}")
        if tfs.dim() != 3 or tuple(tfs.shape[1:]) != (4, 4):
            raise _lib.FpAmdError(f"{what}: tfs must be (T,4,4), got {tuple(tfs.shape)}")
        T = int(tfs.shape[0])
    Q, Nv, F = int(points.shape[0]), int(pos.shape[0]), int(faces.shape[0])
    too_large = limit(T, Q, F)
    if too_large:
        raise _lib.FpAmdError(f"{what}: {too_large}")
    tables = None
    if signed is not None:
        tables = _mesh_tables(what, mesh_tensors, pos, faces, *signed)
        if tuple(tables.vn.shape) != (Nv, 3) or tuple(tables.en.shape) != (F, 3, 3):
            raise _lib.FpAmdError(f"{what}: the tables are of another mesh: vn {tuple(tables.vn.shape)}, en {tuple(tables.en.shape)} for "
                                  f"{Nv} vertices and {F} faces")
    shapes = shapes_of(T, Q)
    out = dict(out or {})
    for k, t in out.items():
        if k not in names:
            raise _lib.FpAmdError(f"{what}: out has '{k}', which is not among {among} {list(names)}")
        if not torch.is_tensor(t) or tuple(t.shape) != shapes[k]:
            raise _lib.FpAmdError(f"{what}: out['{k}'] must be a tensor of shape {shapes[k]}, got "
                                  f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    pts = _dev(points, torch.float32, points_name)
    m = _dev(tfs, torch.float32, "tfs") if pairs else None
    vp_ = _dev(pos, torch.float32, "pos")
    fc = _dev(faces, torch.int32, "faces")
    vn = _dev(tables.vn, torch.float32, "tables.vn") if signed is not None else None
    en = _dev(tables.en, torch.float32, "tables.en") if signed is not None else None
    for k in list(out):
        out[k] = _dev(out[k], dtypes[k], f"out['{k}']")
    srcs = [(points_name, pts), ("pos", vp_), ("faces", fc), ("tables.vn", vn), ("tables.en", en)]
    srcs.insert(1 if signed is None else len(srcs), ("tfs", m))   # the signed calls test tfs last, the others after points
    for k, t in out.items():
        for name, src in srcs:
            if _overlap(t, src):
                raise _lib.FpAmdError(f"{what}: out['{k}'] overlaps {name}")
        for k2, t2 in out.items():
            if k2 < k and _overlap(t, t2):
                raise _lib.FpAmdError(f"{what}: out['{k}'] overlaps out['{k2}']")
    need = int(workspace_bytes(T, Q))
    if workspace is None:
        ws, ws_bytes = _workspace(need, pts.device), need
    else:
        if not (torch.is_tensor(workspace) and workspace.is_cuda and workspace.is_contiguous()):
            raise _lib.FpAmdError(f"{what}: workspace must be a contiguous CUDA(HIP) tensor")
        ws, ws_bytes = workspace, workspace.numel() * workspace.element_size()
        if ws_bytes < need:
            raise _lib.FpAmdError(f"{what}: workspace of {ws_bytes} bytes, {need} needed ({workspace_maker})")
        for k, t in out.items():
            if _overlap(t, ws):
                raise _lib.FpAmdError(f"{what}: out['{k}'] overlaps workspace")
    for k in names:
        if k not in out:
            out[k] = torch.empty(shapes[k], dtype=dtypes[k], device=pts.device)
    return _MeshCall(pts, m, vp_, fc, vn, en, out, ws, ws_bytes, Q, Nv, F, T)


def mesh_point_distance(points, mesh_tensors=None, pos=None, faces=None, want=MESH_DISTANCE_OUTPUTS, out=None, grid=None):
    """fp_mesh_point_distance: the exact distance from the points (Q,3) f32 to the surface of a triangle mesh -> dict of device tensors:
    `dist2` (Q,) f32 the squared distance to the nearest point of any triangle, `face` (Q,) int32 that triangle, `closest` (Q,3) f32
    that point (include/fp_amd.h has the definition: Ericson's region walk in float32, the smallest (dist2, face) wins; +inf / -1 /
    zeros for a query that no triangle answers).  The mesh is mesh_tensors (a dict with pos (Nv,3) f32 and faces (F,3) int32, as
    make_mesh_tensors and TsdfVolume.extract give) or pos= and faces= themselves.  want: names out of "dist2", "face", "closest";
    dist2 is always computed and returned.  out: a dict of caller-owned buffers for some of the wanted names.  Brute force: Q x F pair
    tests.  The workspace (8 bytes a query) is the library's per-stream scratch, or a fresh allocation inside a stream capture.
    Wrong shapes are refused first, then tensors that are not on the device, of another dtype or not contiguous, then buffers that
    overlap an input or each other (FpAmdError).  grid: a MeshGrid of this mesh (mesh_grid_build) answers through
    fp_mesh_grid_point_distance instead: the same bits from far fewer pair tests; a grid built for other pos / faces tensors is
    refused."""
    what = "mesh_point_distance"
    names = _mesh_names(what, want, MESH_DISTANCE_OUTPUTS, always=("dist2",), required=True)
    c = _mesh_call(what, points, None, mesh_tensors, pos, faces, out, names=names, dtypes=_MESH_DISTANCE_DTYPES,
                   shapes_of=lambda T, Q: {"dist2": (Q,), "face": (Q,), "closest": (Q, 3)}, limit=_mesh_limit_points,
                   workspace_bytes=lambda T, Q: _lib.lib().fp_mesh_point_distance_workspace_bytes(Q))
    outs = (_ptr(c.out["dist2"]), _ptr(c.out.get("face")), _ptr(c.out.get("closest")), _ptr(c.ws), c.ws_bytes, _stream(c.points))
    if grid is not None:
        g = _grid_for(what, grid, c.pos, c.faces)
        _lib.check(_lib.lib().fp_mesh_grid_point_distance(_ptr(c.pos), c.Nv, _ptr(c.faces), c.F, C.byref(g), _ptr(c.points), c.Q, *outs),
                   "fp_mesh_grid_point_distance")
    else:
        _lib.check(_lib.lib().fp_mesh_point_distance(_ptr(c.pos), c.Nv, _ptr(c.faces), c.F, _ptr(c.points), c.Q, *outs),
                   "fp_mesh_point_distance")
    return {k: c.out[k] for k in names}


MESH_RAY_OUTPUTS = ("t", "face", "bary", "hit")
_MESH_RAY_DTYPES = {"t": torch.float32, "face": torch.int32, "bary": torch.float32, "hit": torch.float32}
MESH_RAY_CULL = {"none": 0, "back": 1, "front": 2}


def _mesh_ray_cull(what, cull):
    if cull not in MESH_RAY_CULL:
        raise ValueError(f"{what}: cull must be one of {list(MESH_RAY_CULL)}, got {cull!r}")
    return MESH_RAY_CULL[cull]


def mesh_ray_cast(origins, dirs, mesh_tensors=None, *, pos=None, faces=None, t_min=0.0, t_max=float("inf"), cull="none",
                  want=MESH_RAY_OUTPUTS, out=None):
    """fp_mesh_ray_cast: what the rays origins[i] + t * dirs[i] ((R,3) f32 each; dirs need not be unit vectors, t is in units of them)
    hit first on a triangle mesh -> dict of device tensors: `t` (R,) f32 the smallest t in t_min..t_max (both inclusive) at which the
    ray meets a triangle, `face` (R,) int32 that triangle, `bary` (R,2) f32 the hit's weights of the face's second and third vertex,
    `hit` (R,3) f32 the point origin + t * dir (include/fp_amd.h has the definition: Moeller-Trumbore in float32 without an epsilon,
    the smallest (t, face) wins; +inf / -1 / NaN / NaN for a ray that hits nothing).  cull: "none" keeps both sides of a face, "back"
    drops the hits on back faces (the ray runs along the face's normal ab x ac), "front" drops those on front faces.  The test is not
    watertight: a ray through an edge or a vertex that two faces share can miss both.  The mesh, want (t is always computed and
    returned), out, the workspace (8 bytes a ray) and the refusals are mesh_point_distance's.  Brute force: R x F pair tests."""
    what = "mesh_ray_cast"
    names = _mesh_names(what, want, MESH_RAY_OUTPUTS, always=("t",), required=True)
    code = _mesh_ray_cull(what, cull)
    t_min, t_max = float(t_min), float(t_max)
    if not 0.0 <= t_min <= t_max:
        raise ValueError(f"{what}: 0 <= t_min <= t_max is required, got t_min={t_min}, t_max={t_max}")
    _mesh_n3(what, origins=origins, dirs=dirs)
    if tuple(dirs.shape) != tuple(origins.shape):
        raise _lib.FpAmdError(f"{what}: dirs must be {tuple(origins.shape)} like origins, got {tuple(dirs.shape)}")
    c = _mesh_call(what, origins, None, mesh_tensors, pos, faces, out, names=names, dtypes=_MESH_RAY_DTYPES,
                   shapes_of=lambda T, R: {"t": (R,), "face": (R,), "bary": (R, 2), "hit": (R, 3)}, limit=_mesh_limit_points,
                   workspace_bytes=lambda T, R: _lib.lib().fp_mesh_ray_cast_workspace_bytes(R), points_name="origins")
    d = _dev(dirs, torch.float32, "dirs")
    for k in names:
        if _overlap(c.out[k], d):
            raise _lib.FpAmdError(f"{what}: out['{k}'] overlaps dirs")
    _lib.check(_lib.lib().fp_mesh_ray_cast(_ptr(c.pos), c.Nv, _ptr(c.faces), c.F, _ptr(c.points), _ptr(d), c.Q, t_min, t_max, code,
                                           _ptr(c.out["t"]), _ptr(c.out.get("face")), _ptr(c.out.get("bary")), _ptr(c.out.get("hit")),
                                           _ptr(c.ws), c.ws_bytes, _stream(c.points)), "fp_mesh_ray_cast")
    return {k: c.out[k] for k in names}


def _check_rel_tol(what, rel_tol):
    rel_tol = float(rel_tol)
    if not 0.0 <= rel_tol < 1.0:
        raise ValueError(f"{what}: rel_tol must be in [0, 1), got {rel_tol!r}")
    return rel_tol


def mesh_visibility(points, eyes, mesh_tensors=None, rel_tol=1e-4, cull="none", *, pos=None, faces=None):
    """Which of the points (Q,3) f32 each of the eyes (E,3) f32 sees past a mesh -> (E,Q) bool on the device, True where nothing of the
    mesh lies between.  Segment (e, q) is the ray from eyes[e] with the direction points[q] - eyes[e] (one float32 subtraction), and
    it is blocked when mesh_ray_cast with t_min = 0 and t_max = 1 - rel_tol answers with a face.  rel_tol is relative to the distance
    from the eye to the point: the last rel_tol of the segment is not tested, so a point on the mesh's own surface is not blocked by
    the face it lies on (1e-4 is 30-100 micrometres at the 0.3-1 m a camera stands from a hand-sized object), and whatever lies
    nearer to the point than that does not block it either.  A segment that is not finite is not blocked.  cull as mesh_ray_cast's.
    Brute force: E x Q x F pair tests, and 32 bytes of temporaries a segment."""
    what = "mesh_visibility"
    rel_tol = _check_rel_tol(what, rel_tol)
    _mesh_ray_cull(what, cull)
    _mesh_n3(what, points=points, eyes=eyes)
    p, e = _dev(points, torch.float32, "points"), _dev(eyes, torch.float32, "eyes")
    E, Q = int(e.shape[0]), int(p.shape[0])
    origins = e[:, None, :].expand(E, Q, 3).reshape(E * Q, 3).contiguous()
    dirs = (p[None, :, :] - e[:, None, :]).reshape(E * Q, 3).contiguous()
    got = mesh_ray_cast(origins, dirs, mesh_tensors, pos=pos, faces=faces, t_min=0.0, t_max=1.0 - rel_tol, cull=cull, want=("t", "face"))
    return (got["face"] < 0).reshape(E, Q)


MESH_GRID_MAX_CELLS = 1 << 21            # FP_MESH_GRID_MAX_CELLS
MESH_GRID_DEFAULT_PAD = 2.0 ** -16       # of M, the grid box's largest coordinate; the library refuses less than 2^-20
MESH_GRID_CELL_OVER_FACE = 2.0           # the default cell edge, in mean face box edges
MESH_GRID_STATUS = {1: "the entries list was too small", 2: "the overflow list was too small",
                    4: "more than 2^31 - 1 (cell, triangle) entries"}


def mesh_grid_shape(pos, faces, cell=None, max_cells=MESH_GRID_MAX_CELLS, pad=None, lo=None, n=None):
    """The grid mesh_grid_build lays over a mesh, from host arrays pos (Nv,3) f32 and faces (F,3) int -> (lo (3,) f32, h f32, n (3,)
    int32, pad f32).  The box is that of the finite vertices of the faces whose three indices are valid (none: one unit cell at the
    origin).  h = cell, or by default MESH_GRID_CELL_OVER_FACE times the mean over those faces (all vertices finite) of the longest
    edge of the face's bounding box (the box's longest edge when that is zero), times 1.25 until the count fits; n_k = floor((hi_k -
    lo_k) / h) + 1; a given cell that needs more than max_cells cells is refused.  pad defaults to 2^-16 * M, M = the largest
    |coordinate| of the grid box in float32.  lo= and n= (with cell=) lay an explicit box instead: triangles outside it land in its
    boundary cells."""
    f32 = np.float32
    pos = np.asarray(pos, f32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    max_cells = int(max_cells)
    if not 1 <= max_cells <= MESH_GRID_MAX_CELLS:
        raise _lib.FpAmdError(f"mesh_grid_build: max_cells={max_cells} outside 1..2^21")
    if (lo is None) != (n is None) or (lo is not None and cell is None):
        raise _lib.FpAmdError("mesh_grid_build: an explicit box needs lo=, n= and cell= together")
    if cell is not None and not (np.isfinite(cell) and 2.0 ** -100 <= float(f32(cell)) <= 2.0 ** 100):
        raise _lib.FpAmdError(f"mesh_grid_build: cell={cell} must be a positive finite length (2^-100..2^100)")
    if lo is not None:
        lo = np.asarray(lo, f32).reshape(3)
        n = np.asarray(n, np.int64).reshape(3)
        h = f32(cell)
        if not np.isfinite(lo).all() or (n < 1).any() or int(n.prod()) > max_cells:
            raise _lib.FpAmdError(f"mesh_grid_build: box lo={lo.tolist()} n={n.tolist()}: lo must be finite and 1 <= cells <= {max_cells}")
    else:
        ok = ((faces >= 0) & (faces < len(pos))).all(axis=1) if len(faces) else np.zeros(0, bool)
        tri = pos[faces[ok]] if ok.any() else np.zeros((0, 3, 3), f32)
        fin = np.isfinite(tri).all(axis=2)                              # (n, 3): per vertex
        verts = tri[fin]
        if len(verts) == 0:
            lo, ext = np.zeros(3, f32), np.zeros(3)
        else:
            lo = verts.min(axis=0).astype(f32)
            ext = verts.max(axis=0).astype(np.float64) - lo.astype(np.float64)
        if cell is not None:
            h = float(f32(cell))
        else:
            whole = tri[fin.all(axis=1)].astype(np.float64)
            h = MESH_GRID_CELL_OVER_FACE * float((whole.max(axis=1) - whole.min(axis=1)).max(axis=1).mean()) if len(whole) else 0.0
            if not (np.isfinite(h) and h > 0):
                h = float(ext.max()) if ext.max() > 0 else 1.0
            h = float(f32(min(max(h, 2.0 ** -100), 2.0 ** 100)))
        while True:
            cnt = np.floor(ext / h) + 1
            if cnt.prod() <= max_cells:
                break
            if cell is not None:
                raise _lib.FpAmdError(f"mesh_grid_build: cell={cell} needs {cnt.astype(np.int64).tolist()} cells, above max_cells={max_cells}")
            h = float(f32(h * 1.25))
        n, h = cnt.astype(np.int64), f32(h)
    with np.errstate(all="ignore"):
        M = f32(max(np.abs(lo).max(), np.abs(lo + n.astype(f32) * h).max()))
    if not np.isfinite(M):
        raise _lib.FpAmdError("mesh_grid_build: the grid's far corner is not finite")
    pad = f32(MESH_GRID_DEFAULT_PAD) * M if pad is None else f32(pad)
    if not (np.isfinite(pad) and pad >= f32(2.0 ** -20) * M):
        raise _lib.FpAmdError(f"mesh_grid_build: pad={pad} is below 2^-20 of the grid's largest coordinate {M} (or not finite)")
    return lo, h, n.astype(np.int32), f32(pad)


class MeshGrid:
    """A uniform grid over a mesh's triangles (mesh_grid_build): the shape (`lo`, `h`, `n`, `pad`: include/fp_amd.h), the device tables
    `cell_start` (ncells + 1,), `entries` (n_entries,), `overflow` (n_overflow,) int32, and which pos / faces tensors it was built
    for (data pointers and shapes: a grid is refused for any other pair)."""

    def __init__(self, lo, h, n, pad, cell_start, entries, overflow, pos, faces):
        self.lo, self.h, self.n, self.pad = np.asarray(lo, np.float32), np.float32(h), np.asarray(n, np.int32), np.float32(pad)
        self.cell_start, self.entries, self.overflow = cell_start, entries, overflow
        self.n_entries, self.n_overflow = int(entries.numel()), int(overflow.numel())
        self.mesh_key = self.key_of(pos, faces)

    @staticmethod
    def key_of(pos, faces):
        return (pos.data_ptr(), tuple(pos.shape), faces.data_ptr(), tuple(faces.shape))

    @property
    def ncells(self):
        return int(self.n[0]) * int(self.n[1]) * int(self.n[2])

    def struct(self, entries=None, overflow=None):
        """the fp_mesh_grid of a call (entries / overflow: other lists than the grid's own, for the fill)"""
        e = self.entries if entries is None else entries
        o = self.overflow if overflow is None else overflow
        g = _lib.MeshGridStruct()
        g.lo[:] = [float(x) for x in self.lo]
        g.n[:] = [int(x) for x in self.n]
        g.h, g.pad = float(self.h), float(self.pad)
        g.cell_start = self.cell_start.data_ptr()
        g.entries = e.data_ptr() if e.numel() else None
        g.overflow = o.data_ptr() if o.numel() else None
        g.n_entries, g.n_overflow = int(e.numel()), int(o.numel())
        return g


def _grid_for(what, grid, pos, faces):
    if not isinstance(grid, MeshGrid):
        raise _lib.FpAmdError(f"{what}: grid must be a MeshGrid (mesh_grid_build), got {type(grid).__name__}")
    if grid.mesh_key != MeshGrid.key_of(pos, faces):
        raise _lib.FpAmdError(f"{what}: the grid was built for another mesh (other pos / faces tensors): build one for this mesh")
    return grid.struct()


def mesh_grid_build(mesh_tensors=None, pos=None, faces=None, cell=None, max_cells=MESH_GRID_MAX_CELLS, pad=None, lo=None, n=None):
    """fp_mesh_grid_count + fp_mesh_grid_fill: a uniform grid over the triangles of a mesh -> MeshGrid, for
    mesh_point_distance(grid=), mesh_signed_distance(grid=) and the batched mesh_transform_residuals(grid=), mesh_icp_step(grid=) and
    mesh_penetration(grid=), which then give the brute force's bits from a few dozen pair tests a query near the surface
    (include/fp_amd.h has the definition and the proof).  The mesh is mesh_tensors (pos (Nv,3) f32, faces (F,3) int32, on the device)
    or pos= and faces=.  cell: the cell edge; max_cells, pad, lo, n: mesh_grid_shape, which states the
    default rule.  The sequence is count, one read of the header, the allocation of exactly n_entries and n_overflow slots, fill, and
    a read of the status word, which raises FpAmdError when set.  Done once per mesh: it copies the mesh to the host for the box,
    synchronises twice and allocates, so it is not capturable.  With mesh_tensors the grid is kept in the dict under "grid" and
    returned from there the next time when every argument is a default: the caller drops the key when pos or faces change."""
    what = "mesh_grid_build"
    defaults = cell is None and pad is None and lo is None and n is None and int(max_cells) == MESH_GRID_MAX_CELLS
    if mesh_tensors is not None and pos is None and faces is None and defaults and isinstance(mesh_tensors.get("grid"), MeshGrid):
        g = mesh_tensors["grid"]
        if g.mesh_key == MeshGrid.key_of(mesh_tensors["pos"], mesh_tensors["faces"]):
            return g
    pos, faces = _mesh_pos_faces(what, mesh_tensors, pos, faces)
    _mesh_n3(what, pos=pos, faces=faces)
    Nv, F = int(pos.shape[0]), int(faces.shape[0])
    if F > (1 << 30):
        raise _lib.FpAmdError(f"{what}: {F} faces (at most 2^30)")
    vp_ = _dev(pos, torch.float32, "pos")
    fc = _dev(faces, torch.int32, "faces")
    glo, h, gn, gpad = mesh_grid_shape(vp_.detach().cpu().numpy(), fc.detach().cpu().numpy(), cell, max_cells, pad, lo, n)
    dev = vp_.device
    ncells = int(gn[0]) * int(gn[1]) * int(gn[2])
    cell_start = torch.empty((ncells + 1,), dtype=torch.int32, device=dev)
    header = torch.empty((4,), dtype=torch.int32, device=dev)
    none = torch.empty((0,), dtype=torch.int32, device=dev)
    grid = MeshGrid(glo, h, gn, gpad, cell_start, none, none, vp_, fc)
    L = _lib.lib()
    _lib.check(L.fp_mesh_grid_count(_ptr(vp_), Nv, _ptr(fc), F, C.byref(grid.struct()), _ptr(header), _stream(vp_)), "fp_mesh_grid_count")
    n_entries, n_overflow, status, _ = (int(x) for x in header.cpu())
    if status:
        raise _lib.FpAmdError(f"{what}: {MESH_GRID_STATUS.get(status, status)}: use a larger cell")
    entries = torch.empty((n_entries,), dtype=torch.int32, device=dev)
    overflow = torch.empty((n_overflow,), dtype=torch.int32, device=dev)
    g = grid.struct(entries, overflow)
    need = int(L.fp_mesh_grid_fill_workspace_bytes(C.byref(g)))
    ws = torch.empty(((need + 3) // 4,), dtype=torch.int32, device=dev)
    _lib.check(L.fp_mesh_grid_fill(_ptr(vp_), Nv, _ptr(fc), F, C.byref(g), _ptr(header), _ptr(ws), need, _stream(vp_)), "fp_mesh_grid_fill")
    status = int(header[2])
    if status:
        raise _lib.FpAmdError(f"{what}: fp_mesh_grid_fill: " + "; ".join(v for k, v in MESH_GRID_STATUS.items() if status & k)
                              + " (did pos or faces change between the count and the fill?)")
    grid = MeshGrid(glo, h, gn, gpad, cell_start, entries, overflow, vp_, fc)
    if mesh_tensors is not None and defaults:
        mesh_tensors["grid"] = grid
    return grid


MESH_RESIDUAL_OUTPUTS =("max_d2", "over", "dist2")
_MESH_RESIDUAL_DTYPES = {"max_d2": torch.float32, "over": torch.int32, "dist2": torch.float32}
MESH_RESIDUAL_MAX_THRESHOLDS = 4


def mesh_transform_residuals(points, tfs, mesh_tensors=None, pos=None, faces=None, thresholds=None, want=("max_d2", "over"), out=None,
                             grid=None):
    """fp_mesh_transform_residuals: how far each of the transforms tfs (T,4,4) f32 moves the points (Q,3) f32 (surface samples of the
    mesh, as a rule) off the surface of the mesh -> dict of device tensors: `max_d2` (T,) f32 the largest squared distance of a
    transformed point to the surface, `over` (T,L) int32 the number of points whose squared distance is strictly above each threshold
    squared, `dist2` (T,Q) f32 the whole matrix (include/fp_amd.h has the definition: p' = ((r0*x + r1*y) + r2*z) + t per row in
    float32, then fp_mesh_point_distance's dist2; +inf where no triangle answers).  The mesh is mesh_tensors or pos= and faces=, as
    for mesh_point_distance.  thresholds: up to four lengths (a sequence of floats, or None for none); they are rounded to float32
    and squared in float32 on the host (thr2 = f32(thr) * f32(thr), one rounding), and that table goes to the device.  want: names out
    of "max_d2", "over", "dist2"; max_d2 is always computed and returned, over is left out when there is no threshold.  out: a dict of
    caller-owned buffers for some of the wanted names.  The rows of tfs are used as given (row 3 is not read).  T x Q x F pair
    tests.  The workspace (4 bytes a pair) is the library's per-stream scratch, or a fresh allocation inside a stream capture.  Wrong
    shapes are refused first, then tensors that are not on the device, of another dtype or not contiguous, then buffers that overlap
    an input or each other (FpAmdError).  grid: a MeshGrid of this mesh (mesh_grid_build) answers through
    fp_mesh_grid_transform_residuals instead: the same bits; a grid built for other pos / faces tensors is refused, where
    mesh_point_distance refuses it.  It pays only where the transformed points stay within about a cell of the surface of a mesh of tens
    of thousands of faces or more (measured: 17.6 times at 401 672 faces, 3.7 times at 85 796, slower at 4 900); points a few cells
    away already cost more than the brute force on every mesh, and a transformed point far from the mesh walks the whole grid and tests
    every stored triangle from global memory, minutes for milliseconds."""
    what = "mesh_transform_residuals"
    names = _mesh_names(what, want, MESH_RESIDUAL_OUTPUTS, always=("max_d2",), required=True)
    thr = np.zeros(0, np.float32) if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1).astype(np.float32)
    L = len(thr)
    if L > MESH_RESIDUAL_MAX_THRESHOLDS:
        raise ValueError(f"{what}: {L} thresholds (at most {MESH_RESIDUAL_MAX_THRESHOLDS})")
    if L and not bool((thr >= 0).all()):
        raise ValueError(f"{what}: thresholds must be lengths >= 0, got {thresholds!r}")
    if L == 0:
        names = tuple(n for n in names if n != "over")
    c = _mesh_call(what, points, tfs, mesh_tensors, pos, faces, out, pairs=True, names=names, dtypes=_MESH_RESIDUAL_DTYPES,
                   shapes_of=lambda T, Q: {"max_d2": (T,), "over": (T, L), "dist2": (T, Q)}, limit=_mesh_limit_pairs,
                   workspace_bytes=lambda T, Q: _lib.lib().fp_mesh_transform_residuals_workspace_bytes(T, Q))
    g = None if grid is None else _grid_for(what, grid, c.pos, c.faces)
    thr2 = None
    if L:
        sq = thr * thr                                                        # float32 * float32: one rounding, on the host
        if torch.cuda.is_current_stream_capturing():                          # no host-to-device copy inside a capture: L fills
            thr2 = torch.empty(L, dtype=torch.float32, device=c.points.device)
            for l in range(L):
                thr2[l].fill_(float(sq[l]))
        else:
            thr2 = torch.as_tensor(sq, device=c.points.device)
    rest = (_ptr(c.points), c.Q, _ptr(c.tfs), c.T, _ptr(thr2), L, _ptr(c.out["max_d2"]), _ptr(c.out.get("over")), _ptr(c.out.get("dist2")),
            _ptr(c.ws), c.ws_bytes, _stream(c.points))
    if g is not None:
        _lib.check(_lib.lib().fp_mesh_grid_transform_residuals(_ptr(c.pos), c.Nv, _ptr(c.faces), c.F, C.byref(g), *rest),
                   "fp_mesh_grid_transform_residuals")
    else:
        _lib.check(_lib.lib().fp_mesh_transform_residuals(_ptr(c.pos), c.Nv, _ptr(c.faces), c.F, *rest), "fp_mesh_transform_residuals")
    return {k: c.out[k] for k in names}


MESH_ICP_OUTPUTS = ("dist2", "face")
_MESH_ICP_DTYPES = {"tfs_out": torch.float32, "system": torch.float64, "dist2": torch.float32, "face": torch.int32}


def mesh_icp_workspace(T, Q, device):
    """the workspace of mesh_icp_step for T transforms of Q points (a captured graph owns its buffers)"""
    nbytes = int(_lib.lib().fp_mesh_icp_workspace_bytes(int(T), int(Q)))
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=device)


def mesh_icp_step(points, tfs, mesh_tensors=None, pos=None, faces=None, *, max_dist, damping=1e-3, min_pairs=6, want=(), out=None,
                  workspace=None, grid=None):
    """fp_mesh_icp_step: one Gauss-Newton step of point-to-plane ICP for each of the transforms tfs (T,4,4) f32 of the points (Q,3) f32
    (surface samples of a mesh a) against the surface of a mesh b -> (tfs_out (T,4,4) f32, system (T,40) f64[, dict of `dist2` (T,Q)
    f32 / `face` (T,Q) int32 for the names in want]) device tensors.  include/fp_amd.h has the definition: each transformed point is
    paired with its exact closest point on b (fp_mesh_point_distance's) and that face's normal; pairs farther apart than max_dist are
    dropped; damping scales diag(A); fewer than min_pairs pairs leave the transform as it is.  system has icp_point_plane's layout
    (IcpStep.rows reads it) with [36] = the sum of the pairs' squared distances.  The mesh b is mesh_tensors or pos= and faces=, as
    for mesh_point_distance.  out: a dict of caller-owned buffers out of "tfs_out", "system" and the wanted names; workspace:
    mesh_icp_workspace (None: the library's per-stream scratch, or a fresh allocation inside a stream capture).  T x Q x F pair
    tests.  Wrong shapes are refused first, then tensors that are not on the device, of another dtype or not contiguous, then
    buffers that overlap an input or each other (FpAmdError).  grid: a MeshGrid of mesh b (mesh_grid_build) answers through
    fp_mesh_grid_icp_step instead: the same bits, float64 sums included; a grid built for other pos / faces tensors is refused, where
    mesh_point_distance refuses it.  It pays only where the transformed points stay within about a cell of the surface of a mesh of tens
    of thousands of faces or more (measured: 17.6 times at 401 672 faces, 3.7 times at 85 796, slower at 4 900); points a few cells
    away already cost more than the brute force on every mesh, and a transformed point far from the mesh walks the whole grid and tests
    every stored triangle from global memory, minutes for milliseconds."""
    what = "mesh_icp_step"
    md, dmp, mp = _check_icp(max_dist, damping, min_pairs, what)
    names = _mesh_names(what, want, MESH_ICP_OUTPUTS)
    c = _mesh_call(what, points, tfs, mesh_tensors, pos, faces, out, pairs=True, names=("tfs_out", "system") + names,
                   among="the outputs", dtypes=_MESH_ICP_DTYPES,
                   shapes_of=lambda T, Q: {"tfs_out": (T, 4, 4), "system": (T, 40), "dist2": (T, Q), "face": (T, Q)},
                   limit=_mesh_limit_pairs, workspace_bytes=lambda T, Q: _lib.lib().fp_mesh_icp_workspace_bytes(T, Q),
                   workspace=workspace, workspace_maker="mesh_icp_workspace")
    out = c.out
    rest = (_ptr(c.points), c.Q, _ptr(c.tfs), c.T, md, dmp, mp, _ptr(out["system"]), _ptr(out["tfs_out"]), _ptr(out.get("dist2")),
            _ptr(out.get("face")), _ptr(c.ws), c.ws_bytes, _stream(c.points))
    if grid is not None:
        g = _grid_for(what, grid, c.pos, c.faces)
        _lib.check(_lib.lib().fp_mesh_grid_icp_step(_ptr(c.pos), c.Nv, _ptr(c.faces), c.F, C.byref(g), *rest), "fp_mesh_grid_icp_step")
    else:
        _lib.check(_lib.lib().fp_mesh_icp_step(_ptr(c.pos), c.Nv, _ptr(c.faces), c.F, *rest), "fp_mesh_icp_step")
    if names:
        return out["tfs_out"], out["system"], {k: out[k] for k in names}
    return out["tfs_out"], out["system"]


MESH_REPORT_FIELDS = ("edges", "boundary", "nonmanifold", "inconsistent", "degenerate", "welded", "closed")


class MeshPseudonormals(NamedTuple):
    """fp_mesh_pseudonormals of a mesh: `vn` (Nv,3) f32 and `en` (F,3,3) f32 on the mesh's device, `report` (8,) int32 on the host
    (MESH_REPORT_FIELDS, then a zero)."""
    vn: torch.Tensor
    en: torch.Tensor
    report: np.ndarray

    @property
    def closed(self):
        return bool(self.report[6])

    def describe(self):
        return ", ".join(f"{k}={int(v)}" for k, v in zip(MESH_REPORT_FIELDS, self.report))


def mesh_pseudonormals(mesh_tensors=None, pos=None, faces=None):
    """fp_mesh_pseudonormals: the angle-weighted pseudonormals of a mesh's vertices and face edges and the report of what keeps it from
    being closed -> MeshPseudonormals (include/fp_amd.h has the definition; float64 on the host, adjacency by vertex position).  The
    mesh is mesh_tensors (a dict with pos (Nv,3) f32 and faces (F,3) int32) or pos= and faces=, on any device; the tables come back on
    that device.  A setup call: it copies the mesh to the host and synchronises.  With mesh_tensors the result is kept in the dict
    under "pseudonormals" and returned from there the next time: the caller drops the key when pos or faces change."""
    what = "mesh_pseudonormals"
    if mesh_tensors is not None and pos is None and faces is None and isinstance(mesh_tensors.get("pseudonormals"), MeshPseudonormals):
        return mesh_tensors["pseudonormals"]
    pos, faces = _mesh_pos_faces(what, mesh_tensors, pos, faces)
    for name, t, dt in (("pos", pos, torch.float32), ("faces", faces, torch.int32)):
        if not torch.is_tensor(t):
            raise _lib.FpAmdError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
        if t.dim() != 2 or int(t.shape[1]) != 3:
            raise _lib.FpAmdError(f"{what}: {name} must be (n,3), got {tuple(t.shape)}")
        if t.dtype != dt:
            raise _lib.FpAmdError(f"{what}: {name} must be {dt}, got {t.dtype}")
    Nv, F = int(pos.shape[0]), int(faces.shape[0])
    if max(Nv, F) > (1 << 30):
        raise _lib.FpAmdError(f"{what}: {Nv} vertices and {F} faces (at most 2^30 of either)")
    hp = np.ascontiguousarray(pos.detach().cpu().numpy())
    hf = np.ascontiguousarray(faces.detach().cpu().numpy())
    vn, en, report = np.zeros((Nv, 3), np.float32), np.zeros((F, 3, 3), np.float32), np.zeros(8, np.int32)
    _lib.check(_lib.lib().fp_mesh_pseudonormals(hp.ctypes.data if Nv else None, Nv, hf.ctypes.data if F else None, F,
                                                vn.ctypes.data if Nv else None, en.ctypes.data if F else None, report.ctypes.data),
               "fp_mesh_pseudonormals")
    out = MeshPseudonormals(torch.from_numpy(vn).to(pos.device), torch.from_numpy(en).to(pos.device), report)
    if mesh_tensors is not None:
        mesh_tensors["pseudonormals"] = out
    return out


def _mesh_tables(what, mesh_tensors, pos, faces, tables, allow_open):
    """the pseudonormal tables of a signed call (given, cached in mesh_tensors, or computed now), refused for a mesh that is not closed"""
    if tables is None:
        tables = mesh_pseudonormals(mesh_tensors) if mesh_tensors is not None else mesh_pseudonormals(pos=pos, faces=faces)
    if not isinstance(tables, MeshPseudonormals):
        raise _lib.FpAmdError(f"{what}: tables must be a MeshPseudonormals (mesh_pseudonormals), got {type(tables).__name__}")
    if not tables.closed and not allow_open:
        raise _lib.FpAmdError(f"{what}: the mesh is not closed ({tables.describe()}): inside and outside are not defined.  "
                              f"allow_open=True gives the side of the nearest face instead")
    return tables


MESH_SIGNED_OUTPUTS = ("dist2", "face", "closest", "feature", "sign")
_MESH_SIGNED_DTYPES = {"dist2": torch.float32, "face": torch.int32, "closest": torch.float32, "feature": torch.int32, "sign": torch.int32}
MESH_FEATURES = ("vertex a", "vertex b", "vertex c", "edge ab", "edge bc", "edge ca", "interior")


def mesh_signed_distance(points, mesh_tensors=None, pos=None, faces=None, tables=None, want=("dist2", "sign"), out=None,
                         allow_open=False, grid=None):
    """fp_mesh_signed_distance: mesh_point_distance and the side of the surface -> dict of device tensors: `dist2`, `face`, `closest`
    as mesh_point_distance gives them (the same bits), `feature` (Q,) int32 the part of the nearest face the closest point lies on
    (MESH_FEATURES; -1 without an answer), `sign` (Q,) int32: -1 inside, +1 outside or on the surface, 0 for a query that no triangle
    answers.  The signed distance is sign * sqrt(dist2).  include/fp_amd.h has the definition: the sign of (p - closest) . n for the
    angle-weighted pseudonormal n of that feature.  tables: mesh_pseudonormals of the mesh (None: taken from mesh_tensors, where it
    is kept after the first call, or computed now -- a host computation that synchronises, so a caller that captures a graph or
    passes pos= / faces= in a loop makes them beforehand).  The sign means inside / outside only for a closed, outward-oriented mesh
    that does not cross itself: a mesh whose report is not closed is refused (FpAmdError) unless allow_open=True, and then the sign is
    the side of the nearest face (a boundary edge carries its one face's normal).  want, out, the workspace and the order of the
    refusals are mesh_point_distance's; dist2 is always computed and returned.  grid: a MeshGrid of this mesh (mesh_grid_build)
    answers through fp_mesh_grid_signed_distance: the same bits from far fewer pair tests."""
    what = "mesh_signed_distance"
    names = _mesh_names(what, want, MESH_SIGNED_OUTPUTS, always=("dist2",))
    c = _mesh_call(what, points, None, mesh_tensors, pos, faces, out, signed=(tables, allow_open), names=names,
                   dtypes=_MESH_SIGNED_DTYPES,
                   shapes_of=lambda T, Q: {"dist2": (Q,), "face": (Q,), "closest": (Q, 3), "feature": (Q,), "sign": (Q,)},
                   limit=_mesh_limit_signed, workspace_bytes=lambda T, Q: _lib.lib().fp_mesh_signed_distance_workspace_bytes(Q))
    rest = (_ptr(c.vn), _ptr(c.en), _ptr(c.points), c.Q, _ptr(c.out["dist2"]), _ptr(c.out.get("face")), _ptr(c.out.get("closest")),
            _ptr(c.out.get("feature")), _ptr(c.out.get("sign")), _ptr(c.ws), c.ws_bytes, _stream(c.points))
    if grid is not None:
        g = _grid_for(what, grid, c.pos, c.faces)
        _lib.check(_lib.lib().fp_mesh_grid_signed_distance(_ptr(c.pos), c.Nv, _ptr(c.faces), c.F, C.byref(g), *rest),
                   "fp_mesh_grid_signed_distance")
    else:
        _lib.check(_lib.lib().fp_mesh_signed_distance(_ptr(c.pos), c.Nv, _ptr(c.faces), c.F, *rest), "fp_mesh_signed_distance")
    return {k: c.out[k] for k in names}


MESH_PENETRATION_OUTPUTS = ("inside", "depth2", "deepest", "sign", "dist2")
_MESH_PENETRATION_DTYPES = {"inside": torch.int32, "depth2": torch.float32, "deepest": torch.int32, "sign": torch.int32,
                            "dist2": torch.float32}


def mesh_penetration_workspace(T, Q, device):
    """the workspace of mesh_penetration for T transforms of Q points (a captured graph owns its buffers)"""
    nbytes = int(_lib.lib().fp_mesh_penetration_workspace_bytes(int(T), int(Q)))
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=device)


def mesh_penetration(points, tfs, mesh_tensors=None, pos=None, faces=None, tables=None, want=("inside", "depth2", "deepest"), out=None,
                     workspace=None, allow_open=False, grid=None):
    """fp_mesh_penetration: how far each of the transforms tfs (T,4,4) f32 of the points (Q,3) f32 (surface samples of another object,
    as a rule) reaches into the mesh -> dict of device tensors: `inside` (T,) int32 the number of transformed points inside, `depth2`
    (T,) f32 the largest squared distance of one of those to the surface (0 when there is none), `deepest` (T,) int32 its index (the
    smaller of equals; -1 when there is none), `sign` (T,Q) int32 and `dist2` (T,Q) f32 the whole matrices.  include/fp_amd.h has the
    definition: the point as mesh_transform_residuals forms it, then mesh_signed_distance's dist2 and sign; a transform whose rows
    0..2 are not finite moves every point to nowhere and has inside 0, depth2 0, deepest -1.  tables, allow_open and the refusal of a
    mesh that is not closed are mesh_signed_distance's.  want: names out of MESH_PENETRATION_OUTPUTS; inside is always computed and
    returned.  out: a dict of caller-owned buffers for some of the wanted names; workspace: mesh_penetration_workspace (None: the
    library's per-stream scratch, or a fresh allocation inside a stream capture).  T x Q x F pair tests.  grid: a MeshGrid of this
    mesh (mesh_grid_build) answers through fp_mesh_grid_penetration instead: the same bits; a grid built for other pos / faces
    tensors is refused, where mesh_point_distance refuses it.  It pays only where the transformed points stay within about a cell of the
    surface of a mesh of tens of thousands of faces or more; points a few cells away already cost more than the brute force on every
    mesh, and a placement far from the mesh walks the whole grid and tests every stored triangle from global memory, minutes for
    milliseconds."""
    what = "mesh_penetration"
    names = _mesh_names(what, want, MESH_PENETRATION_OUTPUTS, always=("inside",))
    c = _mesh_call(what, points, tfs, mesh_tensors, pos, faces, out, pairs=True, signed=(tables, allow_open), names=names,
                   dtypes=_MESH_PENETRATION_DTYPES,
                   shapes_of=lambda T, Q: {"inside": (T,), "depth2": (T,), "deepest": (T,), "sign": (T, Q), "dist2": (T, Q)},
                   limit=_mesh_limit_signed, workspace_bytes=lambda T, Q: _lib.lib().fp_mesh_penetration_workspace_bytes(T, Q),
                   workspace=workspace, workspace_maker="mesh_penetration_workspace")
    out = c.out
    rest = (_ptr(c.vn), _ptr(c.en), _ptr(c.points), c.Q, _ptr(c.tfs), c.T, _ptr(out["inside"]), _ptr(out.get("depth2")),
            _ptr(out.get("deepest")), _ptr(out.get("sign")), _ptr(out.get("dist2")), _ptr(c.ws), c.ws_bytes, _stream(c.points))
    if grid is not None:
        g = _grid_for(what, grid, c.pos, c.faces)
        _lib.check(_lib.lib().fp_mesh_grid_penetration(_ptr(c.pos), c.Nv, _ptr(c.faces), c.F, C.byref(g), *rest), "fp_mesh_grid_penetration")
    else:
        _lib.check(_lib.lib().fp_mesh_penetration(_ptr(c.pos), c.Nv, _ptr(c.faces), c.F, *rest), "fp_mesh_penetration")
    return {k: out[k] for k in names}


class Penetration(NamedTuple):
    """FoundationPose.penetration_into: per pose, `inside` (N,) float64 the share of the object's surface samples inside the other
    object, `depth` (N,) float64 the distance of the deepest of them to the other's surface (0 when none is inside), `deepest` (N,3)
    float64 that sample in the object's own frame (NaN when none)."""
    inside: np.ndarray
    depth: np.ndarray
    deepest: np.ndarray

    @classmethod
    def rows(cls, got, points, offset=(0.0, 0.0, 0.0)):
        """of mesh_penetration's dict (inside, depth2, deepest), the points it was called with and the offset from their frame to the
        object's own; float64 on the host (one device-to-host copy each)"""
        pts = points.detach().cpu().numpy().astype(np.float64) + np.asarray(offset, dtype=np.float64).reshape(1, 3)
        idx = got["deepest"].cpu().numpy()
        deepest = np.where((idx >= 0)[:, None], pts[np.maximum(idx, 0)] if len(pts) else np.nan, np.nan)
        return cls(got["inside"].cpu().numpy().astype(np.float64) / max(1, len(pts)), np.sqrt(got["depth2"].cpu().numpy().astype(np.float64)),
                   deepest)


class MeshAlignment(NamedTuple):
    """a rigid registration of mesh a onto mesh b (reconstruct.align_meshes): `tf` (4,4) float64 maps a's coordinates into b's frame;
    `mean_distance` / `rmse` the mean and the root mean square of the distances of a's samples to b's surface over the pairs, in the
    meshes' unit; `overlap` the fraction of the samples that are pairs; `status` that of the last step at the winner (0 solved);
    `runner_up` None, or a dict(tf, mean_distance, angle_deg) of the best other basin: its transform, its cost and its rotation angle
    from the winner -- for a symmetric or nearly symmetric object its cost is the winner's, and the caller decides what that means."""
    tf: np.ndarray
    mean_distance: float
    rmse: float
    overlap: float
    status: int
    runner_up: Optional[dict]

    def transfer_pose(self, ob_in_cam):
        """the pose of b's frame given the pose(s) of a's frame ((4,4) or (n,4,4)): ob_in_cam @ inv(tf)"""
        return np.asarray(ob_in_cam, dtype=np.float64) @ np.linalg.inv(self.tf)


class DistanceStats(NamedTuple):
    """the distances of one mesh's surface samples to another mesh's surface, in the meshes' unit"""
    mean: float
    median: float
    p99: float
    max: float

    @classmethod
    def of(cls, d):
        d = np.asarray(d, dtype=np.float64).reshape(-1)
        if d.size == 0:
            return cls(*(float("nan"),) * 4)
        if not np.isfinite(d).all():                 # a sample that no triangle answered: no interpolation between +inf and +inf
            return cls(float(np.mean(d)), float(np.median(d)), float(np.percentile(d, 99, method="higher")), float(np.max(d)))
        return cls(float(np.mean(d)), float(np.median(d)), float(np.percentile(d, 99)), float(np.max(d)))


class SignedStats(NamedTuple):
    """reconstruct.signed_bias(a, b): the signed distances of a's surface samples to b's surface, negative inside b, in the meshes'
    unit: `mean`, `inside` the share of the samples inside b, and the 5th, 50th and 95th percentiles.  A positive mean says a is
    inflated against b, a negative one that it is shrunk."""
    mean: float
    inside: float
    p5: float
    p50: float
    p95: float

    @classmethod
    def of(cls, d):
        d = np.asarray(d, dtype=np.float64).reshape(-1)
        if d.size == 0:
            return cls(*(float("nan"),) * 5)
        pct = dict(method="higher") if not np.isfinite(d).all() else {}
        return cls(float(np.mean(d)), float(np.mean(d < 0)), *(float(x) for x in np.percentile(d, [5, 50, 95], **pct)))


class MeshComparison(NamedTuple):
    """reconstruct.compare_meshes(a, b): how a mesh that was built (a) compares with its reference (b), from surface samples of both.
    `accuracy`: the distances of a's samples to b's surface; `completeness`: those of b's samples to a's surface (DistanceStats);
    `chamfer` the mean of the two means; `hausdorff` the larger of the two maxima (of the samples, so a lower bound of the surfaces');
    per threshold: `precision` the fraction of a's samples within it of b, `recall` that of b's samples within it of a, `fscore`
    their harmonic mean (0 when both are 0).  dist_a_to_b / dist_b_to_a: the two distance arrays where they were computed (device
    tensors from compare_meshes).  `coverage`: None, or with compare_meshes(seen_from=) the fraction of b's samples that a view saw
    and that completeness, recall and b's side of chamfer and hausdorff are taken over."""
    accuracy: DistanceStats
    completeness: DistanceStats
    chamfer: float
    hausdorff: float
    thresholds: tuple
    precision: tuple
    recall: tuple
    fscore: tuple
    dist_a_to_b: object
    dist_b_to_a: object
    coverage: Optional[float] = None

    @classmethod
    def from_distances(cls, d_ab, d_ba, thresholds):
        """the report of two distance arrays (numpy, or device tensors: one device-to-host copy each); float64 on the host"""
        host = lambda d: (d.detach().cpu().numpy() if torch.is_tensor(d) else np.asarray(d)).astype(np.float64).reshape(-1)   # noqa: E731
        ha, hb = host(d_ab), host(d_ba)
        thr = tuple(float(t) for t in thresholds)
        acc, comp = DistanceStats.of(ha), DistanceStats.of(hb)
        prec = tuple(float(np.mean(ha <= t)) if ha.size else float("nan") for t in thr)
        rec = tuple(float(np.mean(hb <= t)) if hb.size else float("nan") for t in thr)
        fs = tuple((2.0 * p * r / (p + r)) if p + r > 0 else 0.0 for p, r in zip(prec, rec))
        return cls(acc, comp, 0.5 * (acc.mean + comp.mean), max(acc.max, comp.max), thr, prec, rec, fs, d_ab, d_ba)

    def as_dict(self):
        """what json.dumps takes: everything but the distance arrays"""
        d = dict(accuracy=self.accuracy._asdict(), completeness=self.completeness._asdict(), chamfer=self.chamfer,
                 hausdorff=self.hausdorff, thresholds=list(self.thresholds), precision=list(self.precision),
                 recall=list(self.recall), fscore=list(self.fscore), samples=[int(np.prod(tuple(self.dist_a_to_b.shape))),
                                                                              int(np.prod(tuple(self.dist_b_to_a.shape)))])
        if self.coverage is not None:
            d["coverage"] = self.coverage
        return d


class ViewCoverage(NamedTuple):
    """reconstruct.view_coverage(mesh, views): what of a mesh's surface a set of views saw, from area-stratified surface samples (a
    fraction of the samples is a fraction of the area).  `seen` (n,) int32 on the device: the number of views that see each sample;
    `points` (n,3) f32 and `face` (n,) the samples and their faces (sample_surface's); `fraction` the share of the samples that at
    least one view sees; `per_view` (V,) the share each view sees; `unseen_area` the area no view sees, in the mesh's unit squared;
    `area` the mesh's area.  The statistics are float64 on the host."""
    seen: object
    points: object
    face: object
    fraction: float
    per_view: tuple
    unseen_area: float
    area: float

    @classmethod
    def from_seen(cls, seen_by_view, points, face, area):
        """the report of the (V,n) bool table "view v sees sample i" (numpy, or a device tensor: one device-to-host copy)"""
        if torch.is_tensor(seen_by_view):
            seen = seen_by_view.sum(dim=0, dtype=torch.int32)
            table = seen_by_view.detach().cpu().numpy()
        else:
            table = np.asarray(seen_by_view, dtype=bool)
            seen = table.sum(axis=0, dtype=np.int32)
        V, n = table.shape
        fraction = float(np.mean(table.any(axis=0))) if V and n else 0.0
        per_view = tuple(float(np.mean(row)) if n else 0.0 for row in table)
        return cls(seen, points, face, fraction, per_view, (1.0 - fraction) * float(area), float(area))

    def describe(self):
        """one line for a log"""
        worst = min(self.per_view) if self.per_view else float("nan")
        best = max(self.per_view) if self.per_view else float("nan")
        return (f"{len(self.per_view)} views see {100.0 * self.fraction:.1f} % of the surface ({self.unseen_area:.6g} of {self.area:.6g} "
                f"unit^2 unseen); a view sees {100.0 * worst:.1f} % to {100.0 * best:.1f} %")

    def as_dict(self):
        """what json.dumps takes: everything but the arrays"""
        return dict(fraction=self.fraction, per_view=list(self.per_view), unseen_area=self.unseen_area, area=self.area,
                    samples=int(np.prod(tuple(self.seen.shape))))


BOP_TAUS = tuple(0.05 * k for k in range(1, 11))       # BOP's misalignment tolerances of VSD, in units of the object's diameter
VSD_MAX_T = 16                                         # FP_VSD_MAX_T (include/fp_amd.h)
_VSD_FAC = {}                                          # (K bytes, H, W, device) -> the depth-to-distance factor on the device


def vsd_dist_factor(K, H, W):
    """the (H,W) float32 depth-to-distance factor of fp_vsd_counts on the host: sqrt(1 + ((u - cx)/fx)^2 + ((v - cy)/fy)^2) in float64
    with integer u, v (BOP's depth_im_to_dist_im_fast), rounded once"""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    a = (np.arange(W, dtype=np.float64)[None, :] - K[0, 2]) / K[0, 0]
    b = (np.arange(H, dtype=np.float64)[:, None] - K[1, 2]) / K[1, 1]
    return np.sqrt(1.0 + a * a + b * b).astype(np.float32)


def _hostK33(K, what, no_skew="the BOP errors are defined without one"):
    """K as a finite (3,3) float64 host matrix without skew and with positive focal lengths (ValueError otherwise)"""
    if torch.is_tensor(K):
        K = K.detach().cpu().numpy()
    K = np.asarray(K, dtype=np.float64)
    if K.size != 9:
        raise ValueError(f"{what}: K must have 9 entries, got shape {K.shape}")
    K = K.reshape(3, 3)
    if not np.isfinite(K).all() or K[0, 0] <= 0 or K[1, 1] <= 0:
        raise ValueError(f"{what}: K must be finite with positive focal lengths, got {K.tolist()}")
    if K[0, 1] != 0:
        raise ValueError(f"{what}: K has a skew of {K[0, 1]}; {no_skew}")
    return K


def vsd_counts(est_depth, gt_depth, obs_depth, K, diameter, taus=BOP_TAUS, delta=0.015, gt_index=None, origin=(0, 0), out=None):
    """fp_vsd_counts: the pixel counts of BOP's visible surface discrepancy of N rendered depth maps est_depth (N,h,w) f32 against the
    renders gt_depth (G,h,w) of their ground truths and the raw sensor depth obs_depth (H,W), all in metres with 0 = nothing ->
    (N, 4+T) int32 device table [n_gt_vis, n_est_vis, n_inter, n_union, c_0 .. c_{T-1}] (include/fp_amd.h has the definition;
    VsdCounts.rows reads it on the host and gives the T errors).  K: the frame's intrinsics (the depth-to-distance factor is built from
    them on the host in float64 and kept per (K, H, W, device)); diameter: the object's, metres; taus: the T <= 16 tolerances in
    units of it (the thresholds tau * diameter are formed in float64 and rounded to float32); delta: the visibility tolerance,
    metres.  gt_index: the (N,) int32 device index of every map's ground truth (None: all against the one for G == 1, map n against
    gt n for G == N).  origin = (x0, y0): the frame pixel of the maps' top-left pixel, for renders of a window of the frame (the full
    frame: (0, 0) and h x w = H x W).  out: a caller-owned (N, 4+T) int32 tensor (a captured graph owns its output; the first call for
    a (K, H, W, device) uploads the factor, so make one call before the capture).  One camera and
    one object per call (no ops.Views, no MeshSet).  Wrong shapes and values are refused first, then tensors that are not on the
    device, of another dtype or not contiguous, then the buffer."""
    what = "vsd_counts"
    for name, t, nd in (("est_depth", est_depth, 3), ("gt_depth", gt_depth, 3), ("obs_depth", obs_depth, 2)):
        if not torch.is_tensor(t):
            raise _lib.FpAmdError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
        if t.dim() != nd:
            raise _lib.FpAmdError(f"{what}: {name} must be {'(n,h,w)' if nd == 3 else '(H,W)'}, got {tuple(t.shape)}")
    N, h, w = (int(x) for x in est_depth.shape)
    G, H, W = int(gt_depth.shape[0]), int(obs_depth.shape[0]), int(obs_depth.shape[1])
    if h < 1 or w < 1 or H < 1 or W < 1:
        raise _lib.FpAmdError(f"{what}: empty images (est_depth {tuple(est_depth.shape)}, obs_depth {tuple(obs_depth.shape)})")
    if tuple(gt_depth.shape[1:]) != (h, w):
        raise _lib.FpAmdError(f"{what}: gt_depth must be (G,{h},{w}) like est_depth, got {tuple(gt_depth.shape)}")
    try:
        x0, y0 = (int(v) for v in origin)
    except (TypeError, ValueError):
        raise _lib.FpAmdError(f"{what}: origin must be (x0, y0), got {origin!r}") from None
    if x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
        raise _lib.FpAmdError(f"{what}: the {h} x {w} window at origin ({x0}, {y0}) is not inside the {H} x {W} frame")
    if gt_index is not None and (not torch.is_tensor(gt_index) or int(gt_index.numel()) != N):
        raise _lib.FpAmdError(f"{what}: {N} maps need a gt_index tensor of {N} entries")
    if G < 1 or (gt_index is None and G not in (1, N)):
        raise _lib.FpAmdError(f"{what}: {G} ground truths for {N} maps need a gt_index")
    tau = np.asarray(taus, dtype=np.float64).reshape(-1)
    T = int(tau.size)
    if not 1 <= T <= VSD_MAX_T:
        raise ValueError(f"{what}: {T} taus, 1..{VSD_MAX_T} are supported")
    if not (np.isfinite(tau).all() and (tau >= 0).all()):
        raise ValueError(f"{what}: taus must be finite and >= 0, got {tau.tolist()}")
    d, diam = float(delta), float(diameter)
    if not (np.isfinite(d) and d >= 0):
        raise ValueError(f"{what}: delta must be finite and >= 0 (metres), got {delta!r}")
    if not (np.isfinite(diam) and diam > 0):
        raise ValueError(f"{what}: diameter must be finite and > 0 (metres), got {diameter!r}")
    K33 = _hostK33(K, what)
    with np.errstate(over="ignore"):
        thr = np.ascontiguousarray((tau * diam).astype(np.float32))
    if not np.isfinite(thr).all():
        raise ValueError(f"{what}: tau * diameter is beyond float32")
    est = _dev(est_depth, torch.float32, "est_depth")
    gtd = _dev(gt_depth, torch.float32, "gt_depth")
    obs = _dev(obs_depth, torch.float32, "obs_depth")
    gi = _dev(gt_index, torch.int32, "gt_index")
    if out is not None:
        out = _dev(out, torch.int32, "out")
        if tuple(out.shape) != (N, 4 + T):
            raise _lib.FpAmdError(f"{what}: out must be ({N}, {4 + T}), got {tuple(out.shape)}")
    key = (K33.tobytes(), H, W, str(est.device))
    fac = _VSD_FAC.get(key)
    if fac is None:
        if len(_VSD_FAC) >= 8:               # a handful of cameras; a stream of new intrinsics does not grow it without bound
            _VSD_FAC.clear()
        fac = _VSD_FAC[key] = torch.from_numpy(vsd_dist_factor(K33, H, W)).to(est.device)
    if out is None:
        out = torch.empty((N, 4 + T), dtype=torch.int32, device=est.device)
    _lib.check(_lib.lib().fp_vsd_counts(_ptr(est), _ptr(gtd), _ptr(gi), G, N, h, w, _ptr(obs), _ptr(fac), H, W, x0, y0, d,
                                        thr.ctypes.data_as(C.c_void_p), T, _ptr(out), _stream(est)), "fp_vsd_counts")
    return out


class VsdCounts(NamedTuple):
    """one row of vsd_counts' table on the host: pixels where the ground truth's render is visible (`n_gt_vis`), where the
    estimate's is (`n_est_vis`), their intersection and union, and per tolerance tau_t the pixels of the intersection whose two
    distances differ by tau_t * diameter or more (`c`, a tuple of T)."""
    n_gt_vis: int
    n_est_vis: int
    n_inter: int
    n_union: int
    c: tuple

    def errors(self):
        """the T values of VSD, float64: (c_t + n_union - n_inter) / n_union, and 1 when nothing is visible"""
        if self.n_union == 0:
            return np.ones(len(self.c))
        return (np.asarray(self.c, dtype=np.float64) + (self.n_union - self.n_inter)) / float(self.n_union)

    @classmethod
    def rows(cls, table):
        """[VsdCounts] per row of a (N, 4+T) table (a device tensor: one device-to-host copy)"""
        a = table.cpu().numpy() if torch.is_tensor(table) else np.asarray(table)
        a = np.asarray(a, dtype=np.int64)
        return [cls(int(r[0]), int(r[1]), int(r[2]), int(r[3]), tuple(int(x) for x in r[4:])) for r in a.reshape(-1, a.shape[-1])]


def mspd(model_pts, poses, gt, K, gt_index=None, symmetry_tfs=None, out=None):
    """fp_mspd: BOP's maximum symmetry-aware projection distance of each of the N poses (N,4,4) f32 to its ground truth, in pixels
    of the camera K over the model points (P,3) f32 -> (N,) float64 device tensor (include/fp_amd.h has the definition): the
    minimum over symmetry_tfs (S,4,4; None: the identity alone) of the largest distance between a point's two projections.  gt,
    gt_index and symmetry_tfs as in pose_errors; a row is NaN for a gt_index out of range, a transform that is not finite or a
    point at or behind the camera plane.  One camera and one object per call.  Refusals in pose_errors' order."""
    N, P, g, G, sym, S = _pose_tables("mspd", model_pts, poses, gt, gt_index, symmetry_tfs)
    K9 = np.ascontiguousarray(_hostK33(K, "mspd").reshape(9).astype(np.float32))
    pts, ps, gi, out = _pose_operands("mspd", model_pts, poses, gt_index, out, (N,))
    g = g.to(device=ps.device, dtype=torch.float64).contiguous()
    sym = None if S == 0 else sym.to(device=ps.device, dtype=torch.float64).contiguous()
    if out is None:
        out = torch.empty((N,), dtype=torch.float64, device=ps.device)
    _lib.check(_lib.lib().fp_mspd(_ptr(pts), P, _ptr(sym), S, _ptr(ps), _ptr(g), _ptr(gi), G, N, K9.ctypes.data_as(C.c_void_p), _ptr(out),
                                  _stream(ps)), "fp_mspd")
    return out


TSDF_MAX_DIM = 4096                                    # FP_TSDF_MAX_DIM (include/fp_amd.h)


def _metres(what, name, x, positive=True):
    """x as a float that is finite and > 0 (positive) or >= 0, and still so once rounded to float32; ValueError otherwise"""
    v = float(x)
    if not (np.isfinite(np.float32(v)) and (np.float32(v) > 0 if positive else v >= 0)):
        raise ValueError(f"{what}: {name} must be finite and {'> 0' if positive else '>= 0'} (metres), got {x!r}")
    return v


def _tensors_nd(what, *named):
    """each (name, t, nd) is a tensor of nd dimensions, refused in the order given"""
    for name, t, nd in named:
        if not torch.is_tensor(t):
            raise _lib.FpAmdError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
        if t.dim() != nd:
            raise _lib.FpAmdError(f"{what}: {name} must have {nd} dimensions, got {tuple(t.shape)}")


def _view_stack(what, depth, rgb, masks, ob_in_cams, too_many=""):
    """the shapes of a stack of posed views (tensors of the right ndim: _tensors_nd) -> (V, H, W); too_many ends the refusal of V > 4096"""
    V, H, W = (int(x) for x in depth.shape)
    if V > 4096:
        raise _lib.FpAmdError(f"{what}: {V} views in one call, at most 4096{too_many}")
    if H < 1 or W < 1 or H * W > 1 << 28:
        raise _lib.FpAmdError(f"{what}: frames of {H} x {W} pixels (1 .. 2^28 pixels are supported)")
    if tuple(rgb.shape) != (V, H, W, 3):
        raise _lib.FpAmdError(f"{what}: rgb must be ({V},{H},{W},3) like depth, got {tuple(rgb.shape)}")
    if masks is not None and (not torch.is_tensor(masks) or tuple(masks.shape) != (V, H, W)):
        raise _lib.FpAmdError(f"{what}: masks must be a ({V},{H},{W}) tensor like depth or None")
    if tuple(ob_in_cams.shape) != (V, 4, 4):
        raise _lib.FpAmdError(f"{what}: ob_in_cams must be ({V},4,4), got {tuple(ob_in_cams.shape)}")
    return V, H, W


def _view_Ks(what, Ks, V, no_skew):
    """a (V,3,3) device tensor, taken as is, or V host matrices, each checked (_hostK33; no_skew: why a skew is refused) and returned as
    one (V,3,3) float64 array: the caller uploads it once nothing can be refused any more (torch.as_tensor passes a device tensor on)"""
    if torch.is_tensor(Ks) and Ks.is_cuda:
        if tuple(Ks.shape) != (V, 3, 3):
            raise _lib.FpAmdError(f"{what}: device Ks must be ({V},3,3), got {tuple(Ks.shape)}")
        return Ks
    Kh = [_hostK33(K, what, no_skew) for K in Ks]
    if len(Kh) != V:
        raise _lib.FpAmdError(f"{what}: {len(Kh)} intrinsic matrices for {V} views")
    return np.asarray(Kh, dtype=np.float64).reshape(V, 3, 3)


def _view_stack_dev(depth, rgb, masks, ob_in_cams, K):
    """the views (K: _view_Ks') as device tensors of their dtypes, contiguous -> (depth, rgb, masks | None, ob_in_cams, K)"""
    return (_dev(depth, torch.float32, "depth"), _dev(rgb, torch.float32, "rgb"), _dev(masks, torch.uint8, "masks"),
            _dev(ob_in_cams, torch.float32, "ob_in_cams"), _dev(K, torch.float64, "Ks") if torch.is_tensor(K) else K)


def _volume_dev(tsdf, weight, color, color_weight):
    return [_dev(t, torch.float32, name) for name, t in (("tsdf", tsdf), ("weight", weight), ("color", color), ("color_weight", color_weight))]


def _check_volume_dims(what, dims):
    if min(dims) < 1 or max(dims) > TSDF_MAX_DIM or dims[0] * dims[1] * dims[2] > 1 << 30:
        raise _lib.FpAmdError(f"{what}: a volume of {dims} voxels; every dimension must be 1..{TSDF_MAX_DIM} and their product <= 2^30")


def _tsdf_grid(what, tsdf, weight, color, color_weight, origin, voxel):
    """shapes and values of a TSDF volume's arrays -> ((nz, ny, nx), origin as 3 float32 on the host, voxel); nothing about devices"""
    for name, t in (("tsdf", tsdf), ("weight", weight), ("color", color), ("color_weight", color_weight)):
        if not torch.is_tensor(t):
            raise _lib.FpAmdError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if tsdf.dim() != 3:
        raise _lib.FpAmdError(f"{what}: tsdf must be (nz,ny,nx), got {tuple(tsdf.shape)}")
    dims = tuple(int(x) for x in tsdf.shape)
    _check_volume_dims(what, dims)
    for name, t, shape in (("weight", weight, dims), ("color", color, dims + (3,)), ("color_weight", color_weight, dims)):
        if tuple(t.shape) != shape:
            raise _lib.FpAmdError(f"{what}: {name} must be {shape} like tsdf, got {tuple(t.shape)}")
    try:
        o = np.asarray(origin, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: origin must be 3 numbers, got {origin!r}") from None
    if o.size != 3 or not np.isfinite(o).all() or not np.isfinite(o.astype(np.float32)).all():
        raise ValueError(f"{what}: origin must be 3 finite numbers (metres), got {origin!r}")
    return dims, np.ascontiguousarray(o.astype(np.float32)), _metres(what, "voxel", voxel)


def tsdf_integrate(tsdf, weight, color, color_weight, depth, rgb, masks, ob_in_cams, Ks, origin, voxel, trunc, min_depth=0.001):
    """fp_tsdf_integrate: fuses V posed RGB-D views into a truncated-signed-distance volume, in place (include/fp_amd.h has the
    definition).  The volume: tsdf, weight, color_weight (nz,ny,nx) and color (nz,ny,nx,3), float32 on the device, a fresh one being
    tsdf = 1 and zeros; voxel (ix, iy, iz) is at origin + (ix, iy, iz) * voxel in the object frame (metres); trunc: the truncation
    distance, metres.  The views: depth (V,H,W) f32 metres, rgb (V,H,W,3) f32, masks (V,H,W) uint8 or None (pixels with mask 0 saw
    past the object and carve the volume empty: the views are assumed to show the object unoccluded), ob_in_cams (V,4,4) f32
    object-to-camera, Ks: V intrinsic matrices on the host (a skew is refused; uploaded as float64) or a (V,3,3) float64 device tensor
    (taken as is: a view whose K has a skew or is not finite is skipped, like one whose pose is not finite).  Depths below min_depth
    are holes.  One launch, no allocation with device Ks, no synchronisation: capturable in a graph; views can be streamed in over
    several calls, with the bits of one call.  Wrong shapes and values are refused first, then tensors that are not on the device, of
    another dtype or not contiguous, then the volume's arrays."""
    what = "tsdf_integrate"
    _tensors_nd(what, ("depth", depth, 3), ("rgb", rgb, 4), ("ob_in_cams", ob_in_cams, 3))
    V, H, W = _view_stack(what, depth, rgb, masks, ob_in_cams, " (fuse them in several calls)")
    dims, o, s = _tsdf_grid(what, tsdf, weight, color, color_weight, origin, voxel)
    tr = _metres(what, "trunc", trunc)
    md = _metres(what, "min_depth", min_depth, positive=False)
    K = _view_Ks(what, Ks, V, "the projection of a voxel is defined without one")
    d, c, m, P, K = _view_stack_dev(depth, rgb, masks, ob_in_cams, K)
    vol = _volume_dev(tsdf, weight, color, color_weight)
    if V == 0:
        return
    K_dev = torch.as_tensor(K, device=d.device)
    _lib.check(_lib.lib().fp_tsdf_integrate(_ptr(d), _ptr(c), _ptr(m), _ptr(P), _ptr(K_dev), V, H, W, dims[0], dims[1], dims[2],
                                            o.ctypes.data_as(C.c_void_p), s, tr, md, _ptr(vol[0]), _ptr(vol[1]), _ptr(vol[2]), _ptr(vol[3]),
                                            _stream(d)), "fp_tsdf_integrate")


def tsdf_components(counts, dims):
    """fp_tsdf_label_components: the face-connected components of the cubes with triangles (include/fp_amd.h has the definition).
    counts: fp_tsdf_count_triangles' int32 device tensor, one element per cube of a volume of dims = (nz, ny, nx) voxels, in any shape
    -> (labels, sizes), int32 device tensors shaped (nz-1, ny-1, nx-1): labels = the smallest cube index of a cube's component, -1
    where counts <= 0; sizes = the component's triangles at that smallest cube, 0 elsewhere.  Integer atomics only: the same bits every
    time.  Three launches, no synchronisation: capturable in a graph (the two outputs are allocated before them)."""
    what = "tsdf_components"
    try:
        nz, ny, nx = (int(n) for n in dims)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: dims must be (nz, ny, nx), got {dims!r}") from None
    _check_volume_dims(what, (nz, ny, nx))
    if not torch.is_tensor(counts):
        raise _lib.FpAmdError(f"{what}: counts must be a tensor, got {type(counts).__name__}")
    shape = (nz - 1, ny - 1, nx - 1)
    if counts.numel() != shape[0] * shape[1] * shape[2]:
        raise _lib.FpAmdError(f"{what}: counts has {counts.numel()} elements, a volume of {(nz, ny, nx)} voxels has {shape[0] * shape[1] * shape[2]} cubes")
    n = _dev(counts, torch.int32, "counts")
    labels = torch.empty(shape, dtype=torch.int32, device=n.device)
    sizes = torch.empty(shape, dtype=torch.int32, device=n.device)
    _lib.check(_lib.lib().fp_tsdf_label_components(_ptr(n), nz, ny, nx, _ptr(labels), _ptr(sizes), _stream(n)), "fp_tsdf_label_components")
    return labels, sizes


def _check_keep(what, keep, name="keep"):
    """keep of tsdf_extract: None | 'largest' | an int >= 1"""
    if keep is None or (isinstance(keep, str) and keep == "largest"):
        return keep
    if isinstance(keep, bool) or not isinstance(keep, (int, np.integer)) or int(keep) < 1:
        raise ValueError(f"{what}: {name} must be None, 'largest' or an int >= 1 (the fewest triangles of a component that stays), got {keep!r}")
    return int(keep)


def _component_report(what, labels, sizes, keep):
    """-> (sizes of all components as a descending host list, labels of the kept ones as a device tensor); one host read"""
    roots = torch.nonzero(sizes.reshape(-1) > 0).reshape(-1)              # ascending labels
    tri = sizes.reshape(-1)[roots]
    host = tri.cpu().numpy().astype(np.int64)
    if host.size == 0:
        return [], roots
    if keep == "largest":
        kept = roots[int(np.argmax(host)):][:1]                            # argmax: the first of equals, the smaller label
    else:
        if int(host.max()) < keep:
            raise ValueError(f"{what}: keep={keep} triangles, the largest of the {host.size} components has {int(host.max())}")
        kept = roots[tri >= keep]
    return sorted((int(x) for x in host), reverse=True), kept


def _min_weight(what, min_weight):
    mw = float(min_weight)
    if not np.isfinite(mw):
        raise ValueError(f"{what}: min_weight must be finite, got {min_weight!r}")
    return mw


def tsdf_count_triangles(tsdf, weight, dims, min_weight):
    """fp_tsdf_count_triangles on a volume of dims = (nz, ny, nx) voxels (tsdf, weight: float32 device tensors; the caller has checked
    them, and that min_weight is a finite float) -> the cubes' triangle counts, int32 (nz-1)(ny-1)(nx-1), x fastest.  One launch."""
    nz, ny, nx = dims
    counts = torch.empty(((nz - 1) * (ny - 1) * (nx - 1),), dtype=torch.int32, device=tsdf.device)
    _lib.check(_lib.lib().fp_tsdf_count_triangles(_ptr(tsdf), _ptr(weight), nz, ny, nx, min_weight, _ptr(counts), _stream(tsdf)),
               "fp_tsdf_count_triangles")
    return counts


def tsdf_extract(tsdf, weight, color, color_weight, origin, voxel, min_weight=1.0, keep=None):
    """The surface of a TSDF volume (arrays, origin and voxel as in tsdf_integrate) as a welded triangle mesh on the device, by
    marching tetrahedra over the cubes whose corners all have weight >= min_weight (fp_tsdf_count_triangles -> torch.cumsum -> one
    host read of the total -> fp_tsdf_emit_triangles -> torch.unique over the corners' grid-edge keys; include/fp_amd.h has the
    definition) -> dict(pos (U,3) f32, vnormals (U,3) f32, vertex_color (U,3) f32 in the units of color, faces (T,3) int32), the
    vertices in the order of their sorted keys and the faces in the order cube, tetrahedron, table: the same bits every time.  No surface
    gives U = T = 0.  The host read of the total makes this a setup call: it synchronises and cannot be captured in a graph.
    keep drops floaters: None (the default) keeps every triangle and launches nothing more; 'largest' keeps the face-connected
    component of cubes (tsdf_components) with the most triangles, the one with the smaller label among equals; an int n >= 1 keeps
    every component of at least n triangles (ValueError, naming the largest, when none has that many).  The kept mesh is the
    unfiltered one without the dropped cubes' triangles: the triangles in their order, the vertices in the order of the sorted keys
    of the corners that remain; the dict then also holds components (the triangles of every component, a descending host list) and
    dropped_triangles.  Only the mesh is filtered: the volume stays as fused.
    Refusals in tsdf_integrate's order."""
    what = "tsdf_extract"
    dims, o, s = _tsdf_grid(what, tsdf, weight, color, color_weight, origin, voxel)
    mw = _min_weight(what, min_weight)
    keep = _check_keep(what, keep)
    f, w, c, cw = _volume_dev(tsdf, weight, color, color_weight)
    dev, L, st = f.device, _lib.lib(), _stream(f)
    nz, ny, nx = dims
    ncubes = (nz - 1) * (ny - 1) * (nx - 1)
    total = 0
    if ncubes > 0:
        counts = tsdf_count_triangles(f, w, dims, mw)
        ends = torch.cumsum(counts, 0, dtype=torch.int64)
        total = int(ends[-1].item())
    report = {} if keep is None else dict(components=[], dropped_triangles=0)
    if total == 0:
        e = torch.empty((0, 3), dtype=torch.float32, device=dev)
        return dict(report, pos=e, vnormals=e.clone(), vertex_color=e.clone(), faces=torch.empty((0, 3), dtype=torch.int32, device=dev))
    if total > 1 << 29:
        raise _lib.FpAmdError(f"{what}: {total} triangles, more than 2^29: use a coarser volume")
    keep_cube = None
    if keep is not None:
        labels, sizes = tsdf_components(counts, dims)
        report["components"], kept = _component_report(what, labels, sizes, keep)
        is_kept = torch.zeros((ncubes,), dtype=torch.bool, device=dev)
        is_kept[kept] = True
        labels = labels.reshape(-1)
        keep_cube = (labels >= 0) & is_kept[labels.clamp(min=0).long()]
    offsets = (ends - counts).contiguous()
    keys = torch.empty((3 * total,), dtype=torch.int64, device=dev)
    pos, col, nrm = (torch.empty((3 * total, 3), dtype=torch.float32, device=dev) for _ in range(3))
    _lib.check(L.fp_tsdf_emit_triangles(_ptr(f), _ptr(w), _ptr(c), _ptr(cw), nz, ny, nx, o.ctypes.data_as(C.c_void_p), s, mw, _ptr(offsets),
                                        total, _ptr(keys), _ptr(pos), _ptr(col), _ptr(nrm), st), "fp_tsdf_emit_triangles")
    if keep_cube is not None:
        # the rows of the kept cubes' triangles, in their order; what is welded below is what remains
        rows = torch.repeat_interleave(keep_cube, counts.long(), output_size=total).repeat_interleave(3)
        keys, pos, col, nrm = keys[rows], pos[rows], col[rows], nrm[rows]
        report["dropped_triangles"] = total - int(keys.numel()) // 3
        total = int(keys.numel()) // 3
    uk, inv = torch.unique(keys, return_inverse=True)
    # every corner on one grid edge carries the same bits; the first of them stands for the vertex
    first = torch.full((int(uk.numel()),), 3 * total, dtype=torch.int64, device=dev)
    first.scatter_reduce_(0, inv, torch.arange(3 * total, dtype=torch.int64, device=dev), "amin")
    return dict(report, pos=pos[first], vnormals=nrm[first], vertex_color=col[first], faces=inv.reshape(total, 3).to(torch.int32))


RAYCAST_OUTPUTS = ("depth", "xyz", "normal", "color")
TSDF_RAYCAST_MAX_SAMPLES = 65536       # FP_TSDF_RAYCAST_MAX_SAMPLES (include/fp_amd.h)
RAYCAST_NO_Z_FAR = float(np.finfo(np.float32).max)      # a z_far that cuts nothing: the box alone ends the rays


def tsdf_raycast(tsdf, weight, color, color_weight, origin, voxel, poses, K, H, W, out_hw=None, bbox2d=None, step=None, min_weight=1.0,
                 z_near=0.001, z_far=None, want=RAYCAST_OUTPUTS, out=None, views=None):
    """fp_tsdf_raycast: the zero surface of a TSDF volume (arrays, origin and voxel as in tsdf_integrate) seen from the N poses
    (N,4,4) f32 object-to-camera, through the crop windows bbox2d (N,4) f32 (crop_windows') into out_hw = (oh, ow) crops, or full
    frame (bbox2d None: out_hw None or (H, W)) -> dict of the outputs in `want`: depth (N,oh,ow) metres, xyz (N,oh,ow,3) camera-frame
    points, normal (N,oh,ow,3) camera-frame unit normals, color (N,oh,ow,3) in the units of the volume's; zeros where a ray meets no
    surface.  The pixel convention is render_crops': depth / xyz / normal stand where a render of the extracted mesh stands in
    depth_agreement and icp_point_plane (include/fp_amd.h has the definition).  K: one camera (3x3, no skew); several views: views = an
    ops.Views (K unused), row n sees through Ks[view[n]].  step: the distance between samples in metres of camera depth (None: one
    voxel); rays start at z_near and end at z_far (None: where they leave the volume).  Only voxels observed min_weight times count.
    out: a dict of caller-owned buffers for (some of) the wanted outputs, so that a loop allocates nothing.  One launch, no
    synchronisation: capturable in a graph.  Wrong shapes and values are refused first, then tensors that are not on the device, of
    another dtype or not contiguous."""
    what = "tsdf_raycast"
    dims, o, s = _tsdf_grid(what, tsdf, weight, color, color_weight, origin, voxel)
    if not torch.is_tensor(poses):
        raise _lib.FpAmdError(f"{what}: poses must be a tensor, got {type(poses).__name__}")
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4):
        raise _lib.FpAmdError(f"{what}: poses must be (N,4,4), got {tuple(poses.shape)}")
    N, H, W = int(poses.shape[0]), int(H), int(W)
    if N > 65535:
        raise _lib.FpAmdError(f"{what}: {N} poses in one call, at most 65535 (chunk the batch)")
    if H < 1 or W < 1:
        raise _lib.FpAmdError(f"{what}: a frame of {H} x {W} pixels")
    if bbox2d is None:
        oh, ow = (H, W) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        if (oh, ow) != (H, W):
            raise _lib.FpAmdError(f"{what}: without bbox2d the crop is the frame: out_hw must be ({H}, {W}), got ({oh}, {ow})")
    else:
        if out_hw is None:
            raise _lib.FpAmdError(f"{what}: out_hw is required with bbox2d")
        oh, ow = int(out_hw[0]), int(out_hw[1])
        if not torch.is_tensor(bbox2d) or tuple(bbox2d.shape) != (N, 4):
            raise _lib.FpAmdError(f"{what}: bbox2d must be a ({N},4) tensor, got "
                                  f"{tuple(bbox2d.shape) if torch.is_tensor(bbox2d) else type(bbox2d).__name__}")
    if oh < 1 or ow < 1 or oh * ow > 1 << 20:
        raise _lib.FpAmdError(f"{what}: crops of {oh} x {ow} pixels (1 .. 2^20 pixels are supported)")
    want = tuple(want)
    if not want or any(w not in RAYCAST_OUTPUTS for w in want):
        raise ValueError(f"{what}: want must name at least one of {RAYCAST_OUTPUTS}, got {want!r}")
    st = s if step is None else _metres(what, "step", step)
    diag = float(np.sqrt(sum((n - 1.0) ** 2 for n in dims))) * s
    if diag / st > TSDF_RAYCAST_MAX_SAMPLES - 2:
        raise ValueError(f"{what}: step={st!r} gives {diag / st:.0f} samples along the volume's diagonal, more than "
                         f"{TSDF_RAYCAST_MAX_SAMPLES - 2}: use a longer step")
    zn = _metres(what, "z_near", z_near, positive=False)
    zf = RAYCAST_NO_Z_FAR if z_far is None else float(z_far)
    if not (np.isfinite(zf) and zf >= zn):
        raise ValueError(f"{what}: z_far must be finite and >= z_near (metres; None for no limit), got {z_far!r}")
    mw = _min_weight(what, min_weight)
    K9 = vt = None
    if views is not None:
        vt = _views(views, what, N)
    else:
        K9 = np.ascontiguousarray(_hostK33(K, what, "the rays are defined without one").reshape(9).astype(np.float32))
    shapes = dict(depth=(N, oh, ow), xyz=(N, oh, ow, 3), normal=(N, oh, ow, 3), color=(N, oh, ow, 3))
    out = dict(out or {})
    for name in out:
        if name not in want:
            raise ValueError(f"{what}: out has a buffer for '{name}', which is not in want={want!r}")
        if not torch.is_tensor(out[name]) or tuple(out[name].shape) != shapes[name]:
            raise _lib.FpAmdError(f"{what}: out['{name}'] must be a {shapes[name]} tensor")
    P = _dev(poses, torch.float32, "poses")
    bb = _dev(bbox2d, torch.float32, "bbox2d")
    f, w, c, cw = _volume_dev(tsdf, weight, color, color_weight)
    res = {}
    for name in RAYCAST_OUTPUTS:
        if name in want:
            res[name] = _dev(out[name], torch.float32, f"out['{name}']") if name in out else torch.empty(shapes[name], dtype=torch.float32,
                                                                                                         device=P.device)
    if N == 0:
        return res
    nul = C.c_void_p(0)
    _lib.check(_lib.lib().fp_tsdf_raycast(_ptr(f), _ptr(w), _ptr(c), _ptr(cw), dims[0], dims[1], dims[2], o.ctypes.data_as(C.c_void_p), s, mw,
                                          _ptr(P), nul if K9 is None else K9.ctypes.data_as(C.c_void_p), nul if vt is None else _ptr(vt.K32),
                                          nul if vt is None else _ptr(vt.dev), 0 if vt is None else vt.V, _ptr(bb), H, W, N, oh, ow, st, zn,
                                          zf, _ptr(res.get("depth")), _ptr(res.get("xyz")), _ptr(res.get("normal")), _ptr(res.get("color")),
                                          _stream(P)), "fp_tsdf_raycast")
    return res


TEXTURE_BAKE_MAX_TEXELS, TEXTURE_BAKE_MAX_SIDE = 16, 16384       # FP_TEXTURE_BAKE_MAX_TEXELS / _SIDE (include/fp_amd.h)


def texture_atlas_layout(F, texels, Bx=None):
    """the per-triangle atlas of F faces with texels x texels blocks, Bx block columns (None: ceil(sqrt(F))) -> (Bx, Ht, Wt); ValueError
    for a block side outside 2..16, Bx < 1 or an atlas of more than 16384 texels a side"""
    what = "texture_bake"
    F, T = int(F), int(texels)
    if not 2 <= T <= TEXTURE_BAKE_MAX_TEXELS:
        raise ValueError(f"{what}: texels must be 2..{TEXTURE_BAKE_MAX_TEXELS} (the side of a face's block), got {texels!r}")
    if F > 1 << 24:
        raise ValueError(f"{what}: {F} faces, at most 2^24")
    if Bx is None:
        Bx = max(int(np.ceil(np.sqrt(F))), 1)
        while Bx * Bx < F:
            Bx += 1
        while Bx > 1 and (Bx - 1) * (Bx - 1) >= F:
            Bx -= 1
    Bx = int(Bx)
    if Bx < 1:
        raise ValueError(f"{what}: Bx must be >= 1 block columns, got {Bx}")
    Ht, Wt = -(-F // Bx) * T, Bx * T
    if max(Ht, Wt) > TEXTURE_BAKE_MAX_SIDE:
        raise ValueError(f"{what}: an atlas of {Ht} x {Wt} texels for {F} faces; at most {TEXTURE_BAKE_MAX_SIDE} a side (fewer texels a "
                         "face, or another Bx)")
    return Bx, Ht, Wt


def texture_atlas_uv(F, texels, Bx, device=None):
    """the texture coordinates that go with texture_bake's atlas -> uv (3F,2) float32 (float64, rounded once), uv_idx (F,3) int32:
    corner k of face f half a texel inside its block, at ((bx*T + 0.5 + dx_k) / Wt, (by*T + 0.5 + dy_k) / Ht) with (dx, dy) = (0,0),
    (T-1,0), (0,T-1): the rasteriser's convention (the row index grows with v), so a bilinear tap inside the triangle reads the
    block's own texels"""
    Bx, Ht, Wt = texture_atlas_layout(F, texels, Bx)
    T = int(texels)
    f = torch.arange(int(F), dtype=torch.float64, device=device)
    bx, by = torch.remainder(f, Bx), torch.div(f, Bx, rounding_mode="floor")
    dx = torch.tensor([0.0, T - 1.0, 0.0], dtype=torch.float64, device=device)
    dy = torch.tensor([0.0, 0.0, T - 1.0], dtype=torch.float64, device=device)
    uv = torch.stack([(bx[:, None] * T + 0.5 + dx[None]) / Wt, (by[:, None] * T + 0.5 + dy[None]) / Ht], -1)
    return uv.reshape(3 * int(F), 2).float().contiguous(), torch.arange(3 * int(F), dtype=torch.int32, device=device).view(int(F), 3)


def texture_bake(pos, faces, vertex_color, depth, rgb, masks, ob_in_cams, Ks, tol, min_cos, texels=4, Bx=None, min_depth=0.001):
    """fp_texture_bake: a per-triangle texture atlas for a mesh from the posed RGB-D views it was fused from (include/fp_amd.h has the
    definition) -> (tex (Ht,Wt,3) f32 in the units of rgb, coverage (Ht,Wt) uint8: the views blended into each texel, uv (3F,2) f32,
    uv_idx (F,3) int32).  pos (Nv,3) f32 and faces (F,3) int32 in the frame of the poses; vertex_color (Nv,3) f32 in the units of rgb
    or None: what a texel no view sees falls back to (None: 128).  The views as tsdf_integrate takes them.  tol (metres): a view
    colours a texel when its depth there is within tol of the texel's; min_cos: the smallest cosine between the face's normal and the
    ray.  Face f owns the texels x texels block (f % Bx, f / Bx); Bx=None: ceil(sqrt(F)).  One launch, no synchronisation: with device
    Ks capturable in a graph (the outputs are allocated before it).  Refusals in tsdf_integrate's order."""
    what = "texture_bake"
    _tensors_nd(what, ("pos", pos, 2), ("faces", faces, 2), ("depth", depth, 3), ("rgb", rgb, 4), ("ob_in_cams", ob_in_cams, 3))
    if pos.shape[1] != 3 or faces.shape[1] != 3:
        raise _lib.FpAmdError(f"{what}: pos must be (Nv,3) and faces (F,3), got {tuple(pos.shape)} and {tuple(faces.shape)}")
    Nv, F = int(pos.shape[0]), int(faces.shape[0])
    if vertex_color is not None and (not torch.is_tensor(vertex_color) or tuple(vertex_color.shape) != (Nv, 3)):
        raise _lib.FpAmdError(f"{what}: vertex_color must be a ({Nv},3) tensor like pos or None")
    V, H, W = _view_stack(what, depth, rgb, masks, ob_in_cams)
    Bx, Ht, Wt = texture_atlas_layout(F, texels, Bx)
    tl = _metres(what, "tol", tol, positive=False)
    mc = float(min_cos)
    if not (0 < np.float32(mc) <= 1):
        raise ValueError(f"{what}: min_cos must be in (0, 1], got {min_cos!r}")
    md = _metres(what, "min_depth", min_depth, positive=False)
    K = _view_Ks(what, Ks, V, "the projection of a texel is defined without one")
    p = _dev(pos, torch.float32, "pos")
    fc = _dev(faces, torch.int32, "faces")
    vc = _dev(vertex_color, torch.float32, "vertex_color")
    d, c, m, P, K = _view_stack_dev(depth, rgb, masks, ob_in_cams, K)
    tex = torch.empty((Ht, Wt, 3), dtype=torch.float32, device=p.device)
    coverage = torch.empty((Ht, Wt), dtype=torch.uint8, device=p.device)
    uv, uv_idx = texture_atlas_uv(F, texels, Bx, p.device)
    if F == 0:
        return tex, coverage, uv, uv_idx
    K_dev = torch.as_tensor(K, device=p.device) if V > 0 else None
    _lib.check(_lib.lib().fp_texture_bake(_ptr(p), Nv, _ptr(fc), F, _ptr(vc), _ptr(d), _ptr(c), _ptr(m), _ptr(P), _ptr(K_dev), V, H, W,
                                          int(texels), Bx, tl, mc, md, _ptr(tex), _ptr(coverage), _stream(p)), "fp_texture_bake")
    return tex, coverage, uv, uv_idx


def pose_update(trans, rot, poses, rot_rep="axis_angle", normalize_xyz=True, trans_normalizer=(1.0, 1.0, 1.0),
                rot_normalizer=1.0, mesh_diameter=1.0, out=None, trans_delta_out=None, rot_delta_out=None, trans_rep="tracknet",
                K=None, tf_to_crops=None, input_w=0, obj=None, views=None):
    """fp_pose_update.  trans_rep='deepim' needs K, tf_to_crops (N,3,3) and the crop width (predict_pose_refine.py:201-215);
    any trans_rep other than 'tracknet' / 'deepim' is the reference's plain `else` branch (:217-218): the raw output.  Several
    objects: mesh_diameter = the (M,) table of object_diameters, obj = the per-hypothesis object index.  Several views: views = an
    ops.Views (K unused).  `out` must not overlap `poses` (the kernel reads poses_in and writes poses_out as __restrict__ rows): an
    in-place update is refused."""
    if _overlap(out, poses):
        raise _lib.FpAmdError("pose_update: out must not overlap poses (poses_in / poses_out are __restrict__; there is no in-place update)")
    tr = _dev(trans, torch.float32, "trans")
    ro = _dev(rot, torch.float32, "rot")
    P = _dev(poses, torch.float32, "poses")
    N = int(P.shape[0])
    if rot_rep == "axis_angle":
        rr = ROT_AXIS_ANGLE
    elif rot_rep == "6d":
        rr = ROT_6D
    else:
        raise RuntimeError(f"unknown rot_rep {rot_rep}")
    tn = np.ascontiguousarray(np.broadcast_to(np.asarray(trans_normalizer, dtype=np.float32).reshape(-1), (3,)))
    O = out if out is not None else torch.empty_like(P)
    deepim = trans_rep == "deepim"
    tf = _dev(tf_to_crops, torch.float32, "tf_to_crops") if deepim else None
    tro = TRANS_DEEPIM if deepim else (TRANS_TRACKNET if trans_rep == "tracknet" else TRANS_RAW)
    (Kp, Ks, view, V), (dia, d, o, M) = _scene("pose_update", N, K, mesh_diameter, obj, views, need_K=deepim)
    st = _lib.lib().fp_pose_update(_ptr(tr), _ptr(ro), _ptr(P), rr, int(bool(normalize_xyz)), tn.ctypes.data_as(C.c_void_p),
                                   float(rot_normalizer), dia, d, o, M, N, _ptr(O),
                                   _ptr(_dev(trans_delta_out, torch.float32, "trans_delta_out")),
                                   _ptr(_dev(rot_delta_out, torch.float32, "rot_delta_out")), tro, Kp, Ks, view, V, _ptr(tf),
                                   float(input_w), _stream(P))
    _lib.check(st, "fp_pose_update")
    return O


def conv7x7s2_bn_relu(x, w_flat, bias, scale, shift, out, pad):
    """x (B,6,H,W) f16 NCHW -> interior of `out` (B, H/2 + 2 pad, W/2 + 2 pad, 64) f16 NHWC (border untouched), following
    the autocast op sequence conv -> fp16, + bias -> fp16, eval BatchNorm -> fp16, ReLU (fp_conv7x7s2_bn_relu_fwd).
    bias (fp16-representable values), scale, shift: (64) f32 or None."""
    x = _dev(x, torch.float16, "x")
    w = _dev(w_flat, torch.float16, "w")
    y = _dev(out, torch.float16, "out")
    Bn, Cin, H, W = x.shape
    if Cin != 6:
        raise _lib.FpAmdError("conv7x7s2_bn_relu: C_in must be 6")
    if tuple(y.shape) != (Bn, H // 2 + 2 * pad, W // 2 + 2 * pad, 64):
        raise _lib.FpAmdError(f"conv7x7s2_bn_relu: out has shape {tuple(y.shape)}")
    st = _lib.lib().fp_conv7x7s2_bn_relu_fwd(_ptr(x), _ptr(w), _ptr(_dev(bias, torch.float32, "bias")),
                                             _ptr(_dev(scale, torch.float32, "scale")), _ptr(_dev(shift, torch.float32, "shift")),
                                             _ptr(y), int(Bn), int(H), int(W), int(pad), _stream(x))
    _lib.check(st, "fp_conv7x7s2_bn_relu_fwd")
    return y


class IgemmGeom(C.Structure):
    """fp_igemm_geom (include/fp_amd.h): addressing of one NHWC fp16 operand of fp_igemm_f16_fwd"""
    _fields_ = [(n, C.c_int) for n in ("pixels_per_image", "width", "padded_h", "padded_w", "stride", "offset", "cstride",
                                       "coff", "bsplit", "cgroup")]

    @staticmethod
    def matrix(ld):
        return IgemmGeom(1, 1, 1, 1, 1, 0, int(ld), 0, 0, 0)

    @staticmethod
    def image(Ho, Wo, pad, C_, stride=1, offset=None, coff=0, bsplit=0, cgroup=0):
        """rows = output pixels (Ho x Wo per image) addressed in a buffer (B, Ho*stride + 2*pad, Wo*stride + 2*pad, C_)
        (for stride 1 that is the output / residual buffer itself; for the conv INPUT pass offset=0 so that the
        geometry addresses tap (0,0))"""
        return IgemmGeom(Ho * Wo, Wo, Ho * stride + 2 * pad, Wo * stride + 2 * pad, stride, pad if offset is None else offset,
                         C_, coff, bsplit, cgroup)


IGEMM_RELU = 1
IGEMM_ROUND_ACC = 2
IGEMM_HAS_W_TILES = 4
IGEMM_MFMA_16X16X32 = 16
IGEMM_MFMA_32X32X16 = 32
IGEMM_EPILOGUE_GENERIC = 64
IGEMM_DIRECT_STORE = 256
IGEMM_W_TILES_DIRECT = 512


class IgemmEpilogue(C.Structure):
    """fp_igemm_epilogue (include/fp_amd.h)"""
    _fields_ = [("bias", C.c_void_p), ("bn_scale", C.c_void_p), ("bn_shift", C.c_void_p), ("residual", C.c_void_p),
                ("r_geom", C.POINTER(IgemmGeom)), ("flags", C.c_int), ("pe", C.c_void_p), ("pe_period", C.c_int), ("y_pe", C.c_void_p),
                ("w_tiles", C.c_void_p)]


def pack_conv3x3_tiles(w, N, Cin):
    """(N, 9 * Cin) fp16 conv weight, k ordered (ky, kx, ci) -> the tile-packed copy fp_igemm_f16_fwd's shifted-window kernel reads as
    contiguous 8 KiB runs (fp_pack_conv3x3_tiles_f16); built once per weight by a plan"""
    w = _dev(w, torch.float16, "w")
    out = torch.empty_like(w)
    _lib.check(_lib.lib().fp_pack_conv3x3_tiles_f16(_ptr(w), _ptr(out), int(N), int(Cin), _stream(w)), "fp_pack_conv3x3_tiles_f16")
    return out


def pack_conv3x3_tiles_direct(w, N, Cin):
    """pack_conv3x3_tiles with the rows of each 128-channel tile in the order of the direct-store kernel (fp_pack_conv3x3_tiles_direct_f16):
    the w_tiles of an igemm_f16 call with w_tiles_direct=True"""
    w = _dev(w, torch.float16, "w")
    out = torch.empty_like(w)
    _lib.check(_lib.lib().fp_pack_conv3x3_tiles_direct_f16(_ptr(w), _ptr(out), int(N), int(Cin), _stream(w)), "fp_pack_conv3x3_tiles_direct_f16")
    return out


def _igemm_epilogue(bias, residual, r_geom, bn_scale, bn_shift, pe, y_pe, flags, w_tiles=None):
    """the fp_igemm_epilogue of igemm_f16 / igemm_f16_splitk: dtype and layout checks of its tensors, `flags` as the caller built them"""
    pe = _dev(pe, torch.float32, "pe")
    ep = IgemmEpilogue()
    ep.bias, ep.bn_scale = _ptr(_dev(bias, torch.float32, "bias")), _ptr(_dev(bn_scale, torch.float32, "bn_scale"))
    ep.bn_shift, ep.residual = _ptr(_dev(bn_shift, torch.float32, "bn_shift")), _ptr(_dev(residual, torch.float16, "residual"))
    ep.r_geom = C.pointer(r_geom) if r_geom is not None else None
    ep.flags = flags
    ep.pe, ep.pe_period, ep.y_pe = _ptr(pe), (int(pe.shape[-2]) if pe is not None else 0), _ptr(_dev(y_pe, torch.float16, "y_pe"))
    ep.w_tiles = _ptr(_dev(w_tiles, torch.float16, "w_tiles"))
    return ep


def igemm_f16(x, x_geom, w, bias, y, y_geom, M, N, Cin, taps, relu=False, residual=None, r_geom=None, bn_scale=None,
              bn_shift=None, conv_rounding=False, pe=None, y_pe=None, w_tiles=None, mfma16=None, direct_store=None, w_tiles_direct=False):
    """y = act(f16(epilogue(implicit_gemm(x, w))) (+ residual)) -- see fp_igemm_f16_fwd.  mfma16: the MFMA shape of the shifted-window
    conv's main loop (True 16x16x32, False 32x32x16); None = the engine switch CONV_MFMA_16X16X32.  direct_store: FP_IGEMM_DIRECT_STORE,
    the shifted-window conv's 512 x 128 tile stored from its accumulators where that kernel exists; None = the engine switch
    CONV_DIRECT_STORE, except that a w_tiles in the other kernel's layout keeps the launch on that kernel.  w_tiles_direct: w_tiles comes
    from pack_conv3x3_tiles_direct (the library refuses a pack that the launch's kernel cannot read).  conv_rounding: nn.Conv2d under
    autocast (accumulator rounded to fp16 before the bias add, optional BatchNorm as scale/shift with its own rounding);
    otherwise nn.Linear (one rounding of accumulator + bias).  pe (S, N) f32 + y_pe (M, N) fp16: second output
    f16(f32(y) + pe[m % S]).  All tensors are device buffers owned by the caller (y is written in place and returned)."""
    x = _dev(x, torch.float16, "x"); w = _dev(w, torch.float16, "w"); y = _dev(y, torch.float16, "y")
    from . import engine                   # engine imports this module
    if mfma16 is None:
        mfma16 = engine.CONV_MFMA_16X16X32
    if direct_store is None:
        direct_store = engine.CONV_DIRECT_STORE and (w_tiles is None or bool(w_tiles_direct))
    ep = _igemm_epilogue(bias, residual, r_geom, bn_scale, bn_shift, pe, y_pe,
                         (IGEMM_RELU if relu else 0) | (IGEMM_ROUND_ACC if conv_rounding else 0) | IGEMM_HAS_W_TILES |
                         (IGEMM_MFMA_16X16X32 if mfma16 else IGEMM_MFMA_32X32X16) |
                         (0 if engine.SPECIALIZED_EPILOGUE else IGEMM_EPILOGUE_GENERIC) |
                         (IGEMM_DIRECT_STORE if direct_store else 0) | (IGEMM_W_TILES_DIRECT if w_tiles_direct else 0), w_tiles)
    st = _lib.lib().fp_igemm_f16_fwd(_ptr(x), C.byref(x_geom), _ptr(w), _ptr(y), C.byref(y_geom), int(M), int(N), int(Cin),
                                     int(taps), C.byref(ep), _stream(x))
    _lib.check(st, "fp_igemm_f16_fwd")
    return y


def igemm_splitk_workspace_bytes(M, N, splits):
    return int(_lib.lib().fp_igemm_splitk_workspace_bytes(int(M), int(N), int(splits)))


def igemm_f16_splitk(x, x_geom, w, bias, y, y_geom, M, N, Cin, taps, splits, workspace, relu=False, residual=None, r_geom=None,
                     bn_scale=None, bn_shift=None, conv_rounding=False, pe=None, y_pe=None):
    """igemm_f16 for launches of a few dozen tiles (one or two hypotheses: the reference's track_one): the k range in `splits`
    pieces, partial sums through the caller-owned `workspace` (uint8, >= igemm_splitk_workspace_bytes), see
    fp_igemm_f16_splitk_fwd.  Equal to igemm_f16 up to fp32 summation order."""
    x = _dev(x, torch.float16, "x"); w = _dev(w, torch.float16, "w"); y = _dev(y, torch.float16, "y")
    ws = _dev(workspace, torch.uint8, "workspace")
    ep = _igemm_epilogue(bias, residual, r_geom, bn_scale, bn_shift, pe, y_pe, (IGEMM_RELU if relu else 0) | (IGEMM_ROUND_ACC if conv_rounding else 0))
    st = _lib.lib().fp_igemm_f16_splitk_fwd(_ptr(x), C.byref(x_geom), _ptr(w), _ptr(y), C.byref(y_geom), int(M), int(N), int(Cin),
                                            int(taps), C.byref(ep), int(splits), _ptr(ws), ws.numel(), _stream(x))
    _lib.check(st, "fp_igemm_f16_splitk_fwd")
    return y


def _work_igemm_splitk(x, x_geom, w, bias, y, y_geom, M, N, Cin, taps, splits, workspace, relu=False, residual=None, r_geom=None, **k):
    return _work_igemm(x, x_geom, w, bias, y, y_geom, M, N, Cin, taps, relu=relu, residual=residual, r_geom=r_geom)


def _work_igemm(x, x_geom, w, bias, y, y_geom, M, N, Cin, taps, relu=False, residual=None, r_geom=None, **k):
    by = 2 * (M * Cin * (1 if taps == 1 else 1.0 / (x_geom.stride ** 2)) + N * Cin * taps + M * N * (2 if residual is not None else 1))
    return by, 2.0 * M * N * Cin * taps


def add_pe_f16(tok, pe):
    """tok (B, S, 512) fp16, pe (S, 512) f32 -> f16(f32(tok) + pe): the in_proj operand (fp_add_pe_f16_fwd)"""
    tok = _dev(tok, torch.float16, "tok")
    pe = _dev(pe, torch.float32, "pe")
    S, D = int(pe.shape[-2]), int(pe.shape[-1])
    M = tok.numel() // D
    out = torch.empty_like(tok)
    _lib.check(_lib.lib().fp_add_pe_f16_fwd(_ptr(tok), _ptr(pe), _ptr(out), M, S, D, _stream(tok)), "fp_add_pe_f16_fwd")
    return out


def replicate_channels(buf, n, c0, c1):
    """buf (>= n, Hp, Wp, C) fp16 NHWC, contiguous: buf[1:n, :, :, c0:c1] = buf[0, :, :, c0:c1] (fp_replicate_rows_f16)"""
    buf = _dev(buf, torch.float16, "buf")
    if buf.dim() != 4 or not buf.is_contiguous() or buf.shape[0] < n:
        raise _lib.FpAmdError(f"replicate_channels: buf must be a contiguous (>= {n}, Hp, Wp, C) tensor, got {tuple(buf.shape)}")
    if n <= 1:
        return buf
    _, Hp, Wp, Ct = (int(v) for v in buf.shape)
    src = buf.data_ptr() + 2 * int(c0)
    st = _lib.lib().fp_replicate_rows_f16(C.c_void_p(src), C.c_void_p(src + 2 * Hp * Wp * Ct), int(n) - 1, Hp * Wp, int(c1) - int(c0), Ct, Ct,
                                          Hp * Wp * Ct, _stream(buf))
    _lib.check(st, "fp_replicate_rows_f16")
    return buf


def replicate_segments(buf, segments, c0, c1):
    """buf (>= segments.total, Hp, Wp, C) fp16 NHWC, contiguous; segments an ops.Segments without empty segments: every image i of
    segment s gets buf[i, :, :, c0:c1] = buf[s, :, :, c0:c1], in place -- the sources (images 0..S-1) are read before they are
    overwritten (fp_replicate_segments_f16, one launch)"""
    buf = _dev(buf, torch.float16, "buf")
    n = int(segments.total)
    if buf.dim() != 4 or not buf.is_contiguous() or buf.shape[0] < n:
        raise _lib.FpAmdError(f"replicate_segments: buf must be a contiguous (>= {n}, Hp, Wp, C) tensor, got {tuple(buf.shape)}")
    if int(segments.lengths.min()) < 1:
        raise _lib.FpAmdError("replicate_segments: every segment must hold at least one image (its source)")
    if segments.dev.device != buf.device:
        raise _lib.FpAmdError(f"replicate_segments: offsets on {segments.dev.device}, buf on {buf.device}")
    _, Hp, Wp, Ct = (int(v) for v in buf.shape)
    st = _lib.lib().fp_replicate_segments_f16(C.c_void_p(buf.data_ptr() + 2 * int(c0)), _ptr(segments.dev), len(segments), n, Hp * Wp,
                                              int(c1) - int(c0), Ct, Hp * Wp * Ct, _stream(buf))
    _lib.check(st, "fp_replicate_segments_f16")
    return buf


def layernorm_res(branch16, gamma, beta, eps=1e-5, x32=None, tok16=None, pe=None, want32=True, want16=True):
    """LN(resid + f32(branch16)) * gamma + beta with resid = x32 or f32(tok16) + pe -> (y32 | None, y16 | None)
    (fp_layernorm_res_fwd: the fp32 residual stream / LayerNorms of nn.TransformerEncoderLayer under autocast)"""
    br = _dev(branch16, torch.float16, "branch16")
    D = int(br.shape[-1])
    M = br.numel() // D
    x32 = _dev(x32, torch.float32, "x32"); tok16 = _dev(tok16, torch.float16, "tok16"); pe = _dev(pe, torch.float32, "pe")
    S = int(pe.shape[-2]) if pe is not None else 0
    y32 = torch.empty(br.shape, dtype=torch.float32, device=br.device) if want32 else None
    y16 = torch.empty_like(br) if want16 else None
    st = _lib.lib().fp_layernorm_res_fwd(_ptr(x32), _ptr(tok16), _ptr(pe), S, _ptr(br), _ptr(_dev(gamma, torch.float32, "gamma")),
                                         _ptr(_dev(beta, torch.float32, "beta")), float(eps), _ptr(y32), _ptr(y16), M, D, _stream(br))
    _lib.check(st, "fp_layernorm_res_fwd")
    return y32, y16


class PackedLinear512:
    """fragment-packed copy of a (512 n, 512) fp16 nn.Linear weight (fp_pack_linear512_f16 per block of 512 output channels): what
    linear512, linear_layernorm_res and ffn_layernorm_mean take, whose waves read their weight rows straight from L2 into MFMA
    operand registers.  direct: the row order of linear512's direct-store kernel instead (fp_pack_linear512_direct_f16), which only
    that kernel reads: the row-owning fused kernels refuse such a pack, and a launch of either linear512 kernel refuses the other's.
    The object keeps a reference to w16 (not a copy), from which linear512 makes the pack in the other order when a call needs it."""

    def __init__(self, w16, direct=False):
        w = _dev(w16, torch.float16, "w16")
        if w.dim() != 2 or int(w.shape[1]) != 512 or int(w.shape[0]) % 512 or int(w.shape[0]) == 0:
            raise _lib.FpAmdError(f"PackedLinear512: weight {tuple(w.shape)}, must be (512 n, 512)")
        self.out_features = int(w.shape[0])
        self.direct = bool(direct)
        self.w16, self._other = w, None
        self.data = torch.empty_like(w)
        fn, name = (_lib.lib().fp_pack_linear512_direct_f16, "fp_pack_linear512_direct_f16") if self.direct else \
                   (_lib.lib().fp_pack_linear512_f16, "fp_pack_linear512_f16")
        for blk in range(self.out_features // 512):
            _lib.check(fn(_ptr(w[blk * 512:]), _ptr(self.data[blk * 512:]), _stream(w)), name)

    def in_order(self, direct):
        """this pack if it has that row order, else the pack of the same weight in the other order (made once, on first use)"""
        if bool(direct) == self.direct:
            return self
        if self._other is None:
            self._other = PackedLinear512(self.w16, direct=direct)
        return self._other


def _packed(w, name, out_features=512):
    if not isinstance(w, PackedLinear512):
        raise _lib.FpAmdError(f"{name}: the weight must be a PackedLinear512 (ops.PackedLinear512(w16))")
    if out_features is not None and w.out_features != out_features:
        raise _lib.FpAmdError(f"{name}: packed weight has {w.out_features} output features, expected {out_features}")
    if w.direct and name != "linear512":
        raise _lib.FpAmdError(f"{name}: the weight is packed in the row order of linear512's direct-store kernel (PackedLinear512(w16, direct=True)); "
                              "the row-owning fused kernels read the plain order")
    return w.data


LINEAR512_RELU = 1
LINEAR512_DIRECT_STORE = 2
LINEAR512_W_DIRECT = 4


def linear512(x16, w_packed, bias, relu=False, out=None, direct_store=None):
    """f16(x16 @ W^T + bias) for x16 (..., 512) fp16 and a PackedLinear512 of W (512 n, 512), n <= 6 (fp_linear512_flags_f16_fwd): the
    input tile of a workgroup is fetched once for all n column blocks; the bits of igemm_f16 with taps = 1.  direct_store: the kernel
    that stores its tiles from the accumulators (FP_LINEAR512_DIRECT_STORE; outputs below 2 GiB).  None = the engine switch
    LINEAR512_DIRECT_STORE, with w_packed brought into the order that kernel reads (PackedLinear512.in_order; a plan packs in the right
    order to begin with); True / False launch that kernel with w_packed as it is, and the library refuses a pack it cannot read."""
    x = _dev(x16, torch.float16, "x16")
    if int(x.shape[-1]) != 512:
        raise _lib.FpAmdError(f"linear512: x16 (..., {int(x.shape[-1])}), must be (..., 512)")
    _packed(w_packed, "linear512", None)
    N = w_packed.out_features
    M = x.numel() // 512
    if direct_store is None:
        from . import engine                   # engine imports this module
        direct_store = bool(engine.LINEAR512_DIRECT_STORE) and M * N * 2 < 2 ** 31
        w_packed = w_packed.in_order(direct_store)
    y = out if out is not None else torch.empty(tuple(x.shape[:-1]) + (N,), dtype=torch.float16, device=x.device)
    if y.dtype != torch.float16 or y.numel() != M * N or not y.is_contiguous():
        raise _lib.FpAmdError("linear512: out must be a contiguous fp16 tensor of M x N elements")
    flags = (LINEAR512_RELU if relu else 0) | (LINEAR512_DIRECT_STORE if direct_store else 0) | (LINEAR512_W_DIRECT if w_packed.direct else 0)
    _lib.check(_lib.lib().fp_linear512_flags_f16_fwd(_ptr(x), _ptr(w_packed.data), _ptr(_dev(bias, torch.float32, "bias")), _ptr(y), M, N, flags,
                                                     _stream(x)), "fp_linear512_flags_f16_fwd")
    return y


def linear_layernorm_res(x16, w_packed, bias, gamma, beta, eps=1e-5, x32=None, tok16=None, pe=None, want32=True, want16=True):
    """layernorm_res(f16(x16 @ w^T + bias), ...) in ONE launch, the product staying on chip (fp_linear_layernorm_fwd).
    x16 (..., 512) fp16, w_packed = PackedLinear512 of the (512, 512) weight -> (y32 | None, y16 | None) of shape (..., 512);
    bit-identical to the two-kernel path.  x16 may be a column block `wide[..., c:c + 512]` of a contiguous wider tensor (one head's
    half of a two-head attention output): the kernel reads it with the wide row stride"""
    w = _packed(w_packed, "linear_layernorm_res")
    if not (torch.is_tensor(x16) and x16.is_cuda and x16.dtype == torch.float16):
        raise _lib.FpAmdError("linear_layernorm_res: x16 must be a CUDA float16 tensor")
    K = int(x16.shape[-1])
    D = 512
    if K != 512:
        raise _lib.FpAmdError(f"linear_layernorm_res: x16 (..., {K}), must be (..., 512)")
    M = x16.numel() // K
    x, ldx = x16, _column_block(x16, "linear_layernorm_res: x16", sep="")
    x32 = _dev(x32, torch.float32, "x32"); tok16 = _dev(tok16, torch.float16, "tok16"); pe = _dev(pe, torch.float32, "pe")
    S = int(pe.shape[-2]) if pe is not None else 0
    shape = tuple(x.shape[:-1]) + (D,)
    y32 = torch.empty(shape, dtype=torch.float32, device=x.device) if want32 else None
    y16 = torch.empty(shape, dtype=torch.float16, device=x.device) if want16 else None
    st = _lib.lib().fp_linear_layernorm_fwd(_ptr(x), _ptr(w), _ptr(_dev(bias, torch.float32, "bias")), _ptr(x32), _ptr(tok16), _ptr(pe), S,
                                            _ptr(_dev(gamma, torch.float32, "gamma")), _ptr(_dev(beta, torch.float32, "beta")), float(eps),
                                            _ptr(y32), _ptr(y16), M, K, D, ldx, _stream(x))
    _lib.check(st, "fp_linear_layernorm_fwd")
    return y32, y16


def ffn_layernorm_mean(y16, w1_packed, b1, w2_packed, b2, x32, gamma, beta, eps=1e-5):
    """(G, R, 512) fp16 y16 (norm1's output) + (G, R, 512) f32 residual stream -> (G, 512) f32 =
    mean_r LN(x32 + linear2(relu(linear1(y16)))) * gamma + beta, one launch + a finish kernel (fp_ffn_layernorm_mean_fwd):
    the feed-forward half of the encoder layer and the token mean with both (G*R, 512) intermediates staying on chip;
    w1_packed / w2_packed: PackedLinear512 of the two (512, 512) weights"""
    y = _dev(y16, torch.float16, "y16")
    G_, R, D = (int(v) for v in y.shape)
    if D != 512:
        raise _lib.FpAmdError("ffn_layernorm_mean: d_model must be 512")
    x32 = _dev(x32, torch.float32, "x32")
    out = torch.empty((G_, D), dtype=torch.float32, device=y.device)
    if R % 16:
        raise _lib.FpAmdError(f"ffn_layernorm_mean: {R} rows per group, must be a multiple of 16")
    ws = torch.empty((max(G_ * R // 16, 1), 512), dtype=torch.float32, device=y.device)
    st = _lib.lib().fp_ffn_layernorm_mean_fwd(_ptr(y), _ptr(_packed(w1_packed, "ffn_layernorm_mean")), _ptr(_dev(b1, torch.float32, "b1")),
                                              _ptr(_packed(w2_packed, "ffn_layernorm_mean")), _ptr(_dev(b2, torch.float32, "b2")), _ptr(x32),
                                              _ptr(_dev(gamma, torch.float32, "gamma")), _ptr(_dev(beta, torch.float32, "beta")), float(eps),
                                              _ptr(out), _ptr(ws), ws.numel() * 4, G_, R, _stream(y))
    _lib.check(st, "fp_ffn_layernorm_mean_fwd")
    return out


def _column_block(x16, name, sep=":"):
    """-> row stride (fp16 values) of an (..., 512) fp16 tensor that is contiguous or a column block of a contiguous wider tensor (unit
    stride in the last dimension, every leading stride that of the wide tensor)"""
    if not (torch.is_tensor(x16) and x16.is_cuda and x16.dtype == torch.float16 and int(x16.shape[-1]) == 512):
        raise _lib.FpAmdError(f"{name}{sep} must be a CUDA float16 tensor (..., 512)")
    if x16.is_contiguous():
        return 512
    ldx = int(x16.stride(-2)) if x16.dim() >= 2 else 512
    ok = x16.stride(-1) == 1 and ldx % 8 == 0 and ldx >= 512 and x16.storage_offset() % 8 == 0
    for d in range(x16.dim() - 2, 0, -1):
        ok = ok and x16.stride(d - 1) == x16.stride(d) * x16.shape[d]
    if not ok:
        raise _lib.FpAmdError(f"{name}{sep} must be contiguous or a column block of a contiguous tensor")
    return ldx


_TAIL_WS = {}


def encoder_tail_mean(ctx16, wo_packed, bo, tok16, pe, gamma1, beta1, w1_packed, b1, w2_packed, b2, gamma2, beta2, eps=1e-5, workspace=None):
    """(G, R, 512) fp16 attention context (heads merged; may be a column block of a wider tensor) + the layer input f32(tok16) + pe ->
    (G, 512) f32 = mean_r LN2(y + linear2(relu(linear1(f16(y))))), y = LN1(f32(tok16) + pe + f16(ctx16 @ Wo^T + bo)): everything of the
    encoder layer behind the attention + the token mean in one launch (fp_encoder_tail_mean_fwd) = linear_layernorm_res followed by
    ffn_layernorm_mean, bit for bit, without norm1's fp16 output reaching HBM"""
    ldx = _column_block(ctx16, "encoder_tail_mean: ctx16")
    G_, R, _ = (int(v) for v in ctx16.shape)
    tok = _dev(tok16, torch.float16, "tok16")
    pe = _dev(pe, torch.float32, "pe")
    if int(pe.shape[-2]) != R or tuple(tok.shape) != (G_, R, 512):
        raise _lib.FpAmdError("encoder_tail_mean: tok16 must be (G, R, 512) and pe (R, 512)")
    if R % 16:
        raise _lib.FpAmdError(f"encoder_tail_mean: {R} rows per group, must be a multiple of 16")
    out = torch.empty((G_, 512), dtype=torch.float32, device=ctx16.device)
    need = int(_lib.lib().fp_encoder_tail_workspace_bytes(G_, R))
    ws = workspace if workspace is not None else torch.empty(need, dtype=torch.uint8, device=ctx16.device)
    f32 = lambda t, n: _ptr(_dev(t, torch.float32, n))
    st = _lib.lib().fp_encoder_tail_mean_fwd(_ptr(ctx16), ldx, _ptr(_packed(wo_packed, "encoder_tail_mean")), f32(bo, "bo"), _ptr(tok), _ptr(pe),
                                             f32(gamma1, "gamma1"), f32(beta1, "beta1"), _ptr(_packed(w1_packed, "encoder_tail_mean")), f32(b1, "b1"),
                                             _ptr(_packed(w2_packed, "encoder_tail_mean")), f32(b2, "b2"), f32(gamma2, "gamma2"), f32(beta2, "beta2"),
                                             float(eps), _ptr(out), _ptr(ws), ws.numel(), G_, R, _stream(ctx16))
    _lib.check(st, "fp_encoder_tail_mean_fwd")
    return out


def colmean_f16(x, gamma=None, beta=None, eps=1e-5, resid32=None):
    """x (G, R, 512) fp16 -> (G, 512) f32: mean over R of LN(resid32 + x)*gamma+beta (gamma given) or of x (fp_colmean_f16_fwd)"""
    x = _dev(x, torch.float16, "x")
    G_, R, D = (int(v) for v in x.shape)
    out = torch.empty((G_, D), dtype=torch.float32, device=x.device)
    st = _lib.lib().fp_colmean_f16_fwd(_ptr(x), _ptr(_dev(resid32, torch.float32, "resid32")), _ptr(_dev(gamma, torch.float32, "gamma")),
                                       _ptr(_dev(beta, torch.float32, "beta")), float(eps), _ptr(out), G_, R, D, _stream(x))
    _lib.check(st, "fp_colmean_f16_fwd")
    return out


ROWS_ROUND_F16, ROWS_X_F16, ROWS_Y_F16 = 1, 2, 4


def rows_linear(x, w, bias=None, round_f16=False, out_f16=False, out=None):
    """y = x @ w.T + bias for a few hundred rows: x (M,K) f32|f16, w (N,K) f16, bias (N) f32 -> (M,N) f32 (rounded to
    fp16 values if round_f16) or fp16 (out_f16) (fp_rows_linear_fwd).  out: optional (M,N) destination of that dtype"""
    if not (torch.is_tensor(x) and x.dtype in (torch.float32, torch.float16)):
        raise _lib.FpAmdError("rows_linear: x must be an f32 or f16 tensor")
    x = _dev(x, x.dtype, "x"); w = _dev(w, torch.float16, "w"); b = _dev(bias, torch.float32, "bias")
    M, K = (int(v) for v in x.shape)
    N = int(w.shape[0])
    ydt = torch.float16 if out_f16 else torch.float32
    y = torch.empty((M, N), dtype=ydt, device=x.device) if out is None else _dev(out, ydt, "out")
    if tuple(y.shape) != (M, N):
        raise _lib.FpAmdError(f"rows_linear: out has shape {tuple(y.shape)}, expected {(M, N)}")
    flags = (ROWS_ROUND_F16 if round_f16 else 0) | (ROWS_X_F16 if x.dtype == torch.float16 else 0) | (ROWS_Y_F16 if out_f16 else 0)
    _lib.check(_lib.lib().fp_rows_linear_fwd(_ptr(x), _ptr(w), _ptr(b), _ptr(y), M, K, N, flags, _stream(x)), "fp_rows_linear_fwd")
    return y


ATT_FP16_SCORES = 1


def _att_head_dim(D3, n_heads, name):
    """head size of a (.., 3*D) qkv row split into n_heads: the kernels derive the row stride from H and the head size, so a
    row that is not exactly 3 * n_heads heads wide would be read with the wrong stride"""
    n_heads = int(n_heads)
    if n_heads <= 0 or D3 % (3 * n_heads):
        raise _lib.FpAmdError(f"{name}: a qkv row of {D3} values is not [q | k | v] of {n_heads} equal heads")
    return D3 // (3 * n_heads)


def attention_f16(qkv, n_heads, fp16_scores=False):
    """qkv (B, S, 3*D) fp16 = in_proj output [q | k | v] -> (B, S, D) fp16 = softmax(q k^T / sqrt(hd)) v, heads merged
    (fp_attention_f16_fwd; head size D / n_heads must be 128).  fp16_scores: q * sqrt(1/hd) and the scores rounded to fp16
    (the need_weights=True branch of nn.MultiheadAttention under autocast, score_network.py:73,86)"""
    if qkv.dim() != 3:
        raise _lib.FpAmdError(f"attention_f16: qkv must be (B, S, 3*D), got {tuple(qkv.shape)}")
    hd = _att_head_dim(int(qkv.shape[2]), n_heads, "attention_f16")
    qkv = _dev(qkv, torch.float16, "qkv")
    B, S, D3 = (int(v) for v in qkv.shape)
    D = D3 // 3
    out = torch.empty((B, S, D), dtype=torch.float16, device=qkv.device)
    st = _lib.lib().fp_attention_f16_fwd(_ptr(qkv), _ptr(out), B, S, int(n_heads), hd,
                                         ATT_FP16_SCORES if fp16_scores else 0, _stream(qkv))
    _lib.check(st, "fp_attention_f16_fwd")
    return out


class Segments:
    """Ragged sequences packed row after row (several objects' hypotheses in one call): segment k is rows offsets[k] ..
    offsets[k + 1] - 1.  Built once from host lengths, like predict_pose_refine.ObjectIndex: the host offsets, the int32 device
    offset table the kernels read (so a captured graph copies nothing), the longest segment max_S and the row total."""

    def __init__(self, lengths, device):
        L = np.asarray(lengths).reshape(-1)
        if L.size == 0:
            raise ValueError("Segments: no segments")
        if L.dtype.kind not in "iu":
            raise ValueError(f"Segments: lengths must be integers, got {L.dtype}")
        L = L.astype(np.int64)
        if L.min() < 0:
            raise ValueError(f"Segments: negative length {int(L.min())}")
        self.lengths = L
        self.offsets = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
        self.total = int(self.offsets[-1])
        if self.total > np.iinfo(np.int32).max:
            raise ValueError(f"Segments: {self.total} rows do not fit the int32 offset table")
        self.max_S = int(L.max())
        self.B = int(L.size)
        self.dev = torch.as_tensor(self.offsets.astype(np.int32), device=device)

    def __len__(self):
        return self.B

    def rows(self, k):
        """the row range (a, b) of segment k"""
        return int(self.offsets[k]), int(self.offsets[k + 1])

    def row_ids(self):
        """(total,) int32 device tensor: the segment of every row (the per-hypothesis object index of a multi-object call); built
        at the first use and kept"""
        if getattr(self, "_row_ids", None) is None:
            self._row_ids = torch.as_tensor(np.repeat(np.arange(self.B), self.lengths).astype(np.int32), device=self.dev.device)
        return self._row_ids


def attention_f16_segments(qkv, segments, n_heads, fp16_scores=False):
    """qkv (Ntot, 3*D) fp16 packed as `segments` (Segments) -> (Ntot, D) fp16: attention_f16 over every segment on its own rows,
    never across segments (fp_attention_segments_f16_fwd; each segment gets the bits of attention_f16 on its slice)"""
    if qkv.dim() != 2 or qkv.shape[1] % 3:
        raise _lib.FpAmdError(f"attention_f16_segments: qkv must be (Ntot, 3*D), got {tuple(qkv.shape)}")
    hd = _att_head_dim(int(qkv.shape[1]), n_heads, "attention_f16_segments")
    qkv = _dev(qkv, torch.float16, "qkv")
    Ntot, D = int(qkv.shape[0]), int(qkv.shape[1]) // 3
    if Ntot != segments.total:
        raise _lib.FpAmdError(f"attention_f16_segments: {Ntot} rows but the segments cover {segments.total}")
    if segments.dev.device != qkv.device:
        raise _lib.FpAmdError(f"attention_f16_segments: offsets on {segments.dev.device}, qkv on {qkv.device}")
    out = torch.empty((Ntot, D), dtype=torch.float16, device=qkv.device)
    st = _lib.lib().fp_attention_segments_f16_fwd(_ptr(qkv), _ptr(out), _ptr(segments.dev), segments.B, segments.max_S, int(n_heads),
                                                  hd, ATT_FP16_SCORES if fp16_scores else 0, _stream(qkv))
    _lib.check(st, "fp_attention_segments_f16_fwd")
    return out


def cluster_poses(angle_diff, dist_diff, poses, symmetry_tfs):
    """Host op (init-time): returns indices of the kept poses (mycpp.cluster_poses semantics)."""
    P = np.ascontiguousarray(np.asarray(poses, dtype=np.float32).reshape(-1, 16))
    S = np.ascontiguousarray(np.asarray(symmetry_tfs, dtype=np.float32).reshape(-1, 16))
    keep = np.empty(P.shape[0], np.int32)
    n = _lib.lib().fp_cluster_poses(float(angle_diff), float(dist_diff), P.ctypes.data_as(C.c_void_p), P.shape[0],
                                    S.ctypes.data_as(C.c_void_p), S.shape[0], keep.ctypes.data_as(C.c_void_p))
    return keep[:n].copy()


# ---------------------------------------------------------------------------------------------------------------
# optional per-entry-point timing with HIP events on the launch stream (used by bench.py for the roofline numbers)
class KernelTimers:
    """with KernelTimers() as t: ...; t.summary() -> {name: dict(calls, avg_ms, bytes, flops)}; times come from
    HIP events recorded on the stream the kernels are launched on; bytes/flops are the ALGORITHMIC work of one
    launch (DESIGN.md 'Kernels'), averaged over the recorded launches."""

    active = None

    def __init__(self):
        self.records = {}

    def __enter__(self):
        KernelTimers.active = self
        return self

    def __exit__(self, *a):
        KernelTimers.active = None

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, evs in self.records.items():
            ms = [a.elapsed_time(b) for a, b, _, _ in evs]
            n = max(1, len(ms))
            out[name] = dict(calls=len(ms), avg_ms=float(sum(ms) / n), bytes=float(sum(e[2] for e in evs) / n),
                             flops=float(sum(e[3] for e in evs) / n))
        return out

    def busy(self, ref):
        """for launches recorded on SEVERAL streams: per entry point the BUSY time = length of the union of its launches'
        [start, end] intervals (timestamps relative to the event `ref`, recorded before the first launch), next to the sum of
        the launch durations, total algorithmic bytes / flops and the span first start .. last end.
        -> {name: dict(calls, sum_ms, busy_ms, bytes, flops, first_ms, last_ms)}"""
        torch.cuda.synchronize()
        out = {}
        for name, evs in self.records.items():
            iv = sorted((ref.elapsed_time(a), ref.elapsed_time(b)) for a, b, _, _ in evs)
            busy, cs, ce = 0.0, None, None
            for a, b in iv:
                if cs is None:
                    cs, ce = a, b
                elif a <= ce:
                    ce = max(ce, b)
                else:
                    busy += ce - cs
                    cs, ce = a, b
            if cs is not None:
                busy += ce - cs
            out[name] = dict(calls=len(iv), sum_ms=float(sum(b - a for a, b in iv)), busy_ms=float(busy),
                             bytes=float(sum(e[2] for e in evs)), flops=float(sum(e[3] for e in evs)),
                             first_ms=float(iv[0][0]) if iv else 0.0, last_ms=float(max(b for _, b in iv)) if iv else 0.0)
        return out


def _esz(t):
    return t.element_size() if t is not None else 4


def _work_render(mesh, poses, bbox2d, K, H, W, out_hw=(160, 160), *a, **k):
    N = int(poses.shape[0])
    A = k.get("A_out")
    esz = _esz(A) if A is not None else (2 if k.get("out_f16") else 4)
    return N * (6 * out_hw[0] * out_hw[1] * esz + 32 * mesh.V + 12 * mesh.T), 0.0


def _work_warp(rgb, xyz_map, depth, tf_to_crops, K, poses, *a, **k):
    N = int(poses.shape[0])
    B = k.get("B_out")
    oh, ow = k.get("out_hw", (160, 160))
    esz = _esz(B) if B is not None else (2 if k.get("out_f16") else 4)
    return N * 6 * oh * ow * esz + rgb.shape[0] * rgb.shape[1] * 24, 0.0


def _work_conv1(x, *a, **k):
    Bn, _, H, W = x.shape
    return Bn * (6 * H * W + 64 * (H // 2) * (W // 2)) * 2 + 64 * 294 * 2, 2.0 * Bn * (H // 2) * (W // 2) * 64 * 294


def _timed(name, fn, work=None):
    def wrapper(*a, **k):
        t = KernelTimers.active
        if t is None:
            return fn(*a, **k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn(*a, **k)
        e1.record()
        by, fl = work(*a, **k) if work is not None else (0.0, 0.0)
        t.records.setdefault(name, []).append((e0, e1, float(by), float(fl)))
        return r
    wrapper.__name__ = fn.__name__
    wrapper.__doc__ = fn.__doc__
    return wrapper


render_crops = _timed("fp_render_crops", render_crops, _work_render)
warp_crops = _timed("fp_warp_crops", warp_crops, _work_warp)
crop_windows = _timed("fp_crop_windows", crop_windows)
pose_update = _timed("fp_pose_update", pose_update)
conv7x7s2_bn_relu = _timed("fp_conv7x7s2_bn_relu_fwd", conv7x7s2_bn_relu, _work_conv1)
igemm_f16 = _timed("fp_igemm_f16_fwd", igemm_f16, _work_igemm)
igemm_f16_splitk = _timed("fp_igemm_f16_splitk_fwd", igemm_f16_splitk, _work_igemm_splitk)
add_pe_f16 = _timed("fp_add_pe_f16_fwd", add_pe_f16, lambda tok, pe: (4.0 * tok.numel(), 0.0))
replicate_channels = _timed("fp_replicate_rows_f16", replicate_channels,
                            lambda buf, n, c0, c1: (2.0 * n * buf.shape[1] * buf.shape[2] * (c1 - c0), 0.0))
replicate_segments = _timed("fp_replicate_segments_f16", replicate_segments,
                            lambda buf, seg, c0, c1: (2.0 * (seg.total - len(seg)) * buf.shape[1] * buf.shape[2] * (c1 - c0), 0.0))
mask_depth_stats = _timed("fp_mask_depth_stats", mask_depth_stats)
depth_agreement = _timed("fp_depth_agreement", depth_agreement)
pose_errors = _timed("fp_pose_errors", pose_errors)
mesh_point_distance = _timed("fp_mesh_point_distance", mesh_point_distance)
mesh_ray_cast = _timed("fp_mesh_ray_cast", mesh_ray_cast)
mesh_transform_residuals = _timed("fp_mesh_transform_residuals", mesh_transform_residuals)
mesh_icp_step = _timed("fp_mesh_icp_step", mesh_icp_step)
icp_point_plane = _timed("fp_icp_point_plane", icp_point_plane)
tsdf_components = _timed("fp_tsdf_label_components", tsdf_components)
vsd_counts = _timed("fp_vsd_counts", vsd_counts)
mspd = _timed("fp_mspd", mspd)
layernorm_res = _timed("fp_layernorm_res_fwd", layernorm_res,
                       lambda br, *a, **k: ((2.0 + (4.0 if k.get("x32") is not None else 2.0) + (4.0 if k.get("want32", True) else 0.0)
                                             + (2.0 if k.get("want16", True) else 0.0)) * br.numel(), 0.0))
linear512 = _timed("fp_linear512_f16_fwd", linear512,
                   lambda x, w, *a, **k: (2.0 * x.numel() + 2.0 * 512 * w.out_features + 2.0 * (x.numel() // 512) * w.out_features,
                                          2.0 * x.numel() * w.out_features))
linear_layernorm_res = _timed("fp_linear_layernorm_fwd", linear_layernorm_res,
                              lambda x, w, *a, **k: (2.0 * x.numel() + 2.0 * 512 * 512 + (x.numel() // x.shape[-1]) * 512 *
                                                     ((4.0 if k.get("x32") is not None else 2.0) + (4.0 if k.get("want32", True) else 0.0)
                                                      + (2.0 if k.get("want16", True) else 0.0)),
                                                     2.0 * x.numel() * 512))
ffn_layernorm_mean = _timed("fp_ffn_layernorm_mean_fwd", ffn_layernorm_mean,
                            lambda y, w1, b1, w2, *a, **k: (6.0 * y.numel() + 4.0 * 512 * 512, 4.0 * y.numel() * 512))
encoder_tail_mean = _timed("fp_encoder_tail_mean_fwd", encoder_tail_mean,
                           lambda ctx, *a, **k: (2.0 * ctx.numel() * 2 + 8.0 * ctx.numel() + 6.0 * 512 * 512, 6.0 * ctx.numel() * 512))
colmean_f16 = _timed("fp_colmean_f16_fwd", colmean_f16,
                     lambda x, *a, **k: ((6.0 if k.get("resid32") is not None else 2.0) * x.numel(), 0.0))
rows_linear = _timed("fp_rows_linear_fwd", rows_linear)
attention_f16 = _timed("fp_attention_f16_fwd", attention_f16,
                       lambda qkv, n_heads, **k: (2.0 * qkv.numel() * 4.0 / 3.0, 4.0 * qkv.shape[0] * qkv.shape[1] ** 2 * (qkv.shape[2] // 3)))
attention_f16_segments = _timed("fp_attention_segments_f16_fwd", attention_f16_segments,
                                lambda qkv, seg, n_heads, **k: (2.0 * qkv.numel() * 4.0 / 3.0,
                                                                4.0 * float((seg.lengths ** 2).sum()) * (qkv.shape[1] // 3)))
