"""Model-free object setup: an object's mesh from a few posed RGB-D reference views with masks, by truncated-signed-distance (TSDF)
fusion and marching tetrahedra on the device (ops.tsdf_integrate / ops.tsdf_extract; include/fp_amd.h has the definition).  It stands
where the reference trains a neural object field (bundlesdf/, not built: DESIGN.md section 7): what setup hands to FoundationPose is a
mesh in the object frame either way.  Colours are per vertex, as coarse as the voxel pitch; bake_texture (reconstruct_object's
texture=T) adds a per-triangle texture atlas blended from the same views at their own resolution (ops.texture_bake).  There is no
simplification: the masks do the carving, and the views are assumed to show the object unoccluded.  What the carving leaves behind
as a floater can be dropped from the mesh at extraction (keep= / keep_components=: ops.tsdf_components); the volume stays as fused."""
import numpy as np
import torch

from . import ops
from .mesh import SimpleMesh

PAD_VOXELS = 3          # voxels kept free around the observed points, so that the surface closes inside the volume


def _host(x):
    """a list of arrays / an array / a tensor -> an array or a tensor, where it is: shapes are checked before anything is uploaded"""
    if x is None or torch.is_tensor(x):
        return x
    return np.ascontiguousarray(np.asarray(x))


def _upload(x, dtype, device):
    if x is None:
        return None
    if not torch.is_tensor(x):
        x = torch.as_tensor(x)
    return x.to(device=device, dtype=dtype).contiguous()


def _views_in(rgbs, depths, masks, ob_in_cams, Ks, device, what):
    """the arguments every entry point here takes, their shapes checked where they are and then uploaded once -> device tensors (depth
    (V,H,W) f32, rgb (V,H,W,3) f32 in 0..255 | None, masks (V,H,W) uint8 | None, poses (V,4,4) f32) and the host Ks (V,3,3) float64"""
    d, c, m, P = _host(depths), _host(rgbs), _host(masks), _host(ob_in_cams)
    if d.ndim != 3:
        raise ValueError(f"{what}: depths must be (V,H,W), got {tuple(d.shape)}")
    V = int(d.shape[0])
    if V == 0:
        raise ValueError(f"{what}: no views")
    if c is not None and tuple(c.shape) != tuple(d.shape) + (3,):
        raise ValueError(f"{what}: rgbs must be {tuple(d.shape) + (3,)} like depths, got {tuple(c.shape)}")
    if m is not None and tuple(m.shape) != tuple(d.shape):
        raise ValueError(f"{what}: masks must be {tuple(d.shape)} like depths, got {tuple(m.shape)}")
    if tuple(P.shape) != (V, 4, 4):
        raise ValueError(f"{what}: ob_in_cams must be ({V},4,4), got {tuple(P.shape)}")
    K = np.asarray(Ks.detach().cpu().numpy() if torch.is_tensor(Ks) else Ks, dtype=np.float64)
    if K.shape == (3, 3):
        K = np.tile(K[None], (V, 1, 1))
    if K.shape != (V, 3, 3):
        raise ValueError(f"{what}: Ks must be ({V},3,3) or one (3,3) matrix, got {K.shape}")
    return (_upload(d, torch.float32, device), _upload(c, torch.float32, device), _upload(m, torch.uint8, device),
            _upload(P, torch.float32, device), K)


def _masked_xyz(d, m, K):
    """-> (the views' table: view v for row v, the views' masked depth back-projected unfiltered: (V,H,W,3), camera frame)"""
    vt = ops.Views(list(K), np.arange(int(d.shape[0])), d.device)
    return vt, ops.depth_to_xyz_frames(torch.where(m != 0, d, torch.zeros_like(d)).contiguous(), vt)


def _check_mesh_tensors(mesh_tensors, what):
    for k in ("pos", "faces", "vnormals"):
        if k not in mesh_tensors:
            raise ValueError(f"{what}: mesh_tensors has no '{k}'")


class TsdfVolume:
    """A TSDF volume on the device: dims = (nz, ny, nx) voxels of pitch `voxel` (metres), voxel (ix, iy, iz) at origin + (ix, iy, iz) *
    voxel in the object frame, truncation `trunc` (default 4 voxels)."""

    def __init__(self, origin, dims, voxel, trunc=None, device="cuda", min_depth=0.001):
        self.origin = np.asarray(origin, dtype=np.float64).reshape(3)
        self.dims = tuple(int(n) for n in dims)
        if len(self.dims) != 3:
            raise ValueError(f"TsdfVolume: dims must be (nz, ny, nx), got {dims!r}")
        self.voxel = float(voxel)
        self.trunc = 4.0 * self.voxel if trunc is None else float(trunc)
        self.min_depth = float(min_depth)
        self.device = torch.device(device)
        self.tsdf = torch.empty(self.dims, dtype=torch.float32, device=self.device)
        self.weight = torch.empty(self.dims, dtype=torch.float32, device=self.device)
        self.color = torch.empty(self.dims + (3,), dtype=torch.float32, device=self.device)
        self.color_weight = torch.empty(self.dims, dtype=torch.float32, device=self.device)
        self.left_out = None          # integrate_aligned: the views of its last call that it did not fuse
        self.reset()

    def arrays(self):
        return self.tsdf, self.weight, self.color, self.color_weight

    def reset(self):
        """nothing observed: tsdf = 1, everything else 0 (fills on the stream: capturable)"""
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        self.color.zero_()
        self.color_weight.zero_()

    def integrate(self, rgbs, depths, masks, ob_in_cams, Ks):
        """fuses V views: rgbs (V,H,W,3) uint8 or float in 0..255, depths (V,H,W) metres, masks (V,H,W) bool / uint8 or None,
        ob_in_cams (V,4,4), Ks (V,3,3) or one (3,3).  Views can be streamed in over several calls; the volume then holds the bits of
        one call over all of them."""
        if rgbs is None:
            raise ValueError("TsdfVolume.integrate: rgbs are required")
        self._integrate(*_views_in(rgbs, depths, masks, ob_in_cams, Ks, self.device, "TsdfVolume.integrate"))

    def _integrate(self, d, c, m, P, K):
        ops.tsdf_integrate(*self.arrays(), d, c, m, P, K, self.origin, self.voxel, self.trunc, self.min_depth)

    def components(self, min_weight=1):
        """the surface components extract(keep=...) chooses among, without extracting (ops.tsdf_components over the cubes'
        triangle counts) -> dict(labels (nz-1,ny-1,nx-1) int32 on the device: the smallest cube index of each cube's face-connected
        component, -1 where the cube has no triangle; components: the triangles of every component, a descending host list).  A
        setup call (it synchronises)."""
        nz, ny, nx = self.dims
        shape = (max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0))
        mw = ops._min_weight("TsdfVolume.components", min_weight)
        if 0 in shape:
            return dict(labels=torch.empty(shape, dtype=torch.int32, device=self.device), components=[])
        labels, sizes = ops.tsdf_components(ops.tsdf_count_triangles(self.tsdf, self.weight, self.dims, mw), self.dims)
        sizes = sizes[sizes > 0].cpu().numpy()
        return dict(labels=labels, components=sorted((int(x) for x in sizes), reverse=True))

    def extract(self, min_weight=1, keep=None):
        """the surface over the voxels observed at least min_weight times -> (SimpleMesh with uint8 vertex colours, mesh_tensors):
        the second is the device dict FoundationPose and the rasteriser take (pos, vnormals, faces, vertex_color in [0,1], _handle),
        made from the extraction's device tensors without a host round trip, with the colours rounded to the mesh's uint8 ones: the
        bits make_mesh_tensors(mesh) would give.  keep ('largest' or the fewest triangles of a component that stays; ops.tsdf_extract)
        drops floaters from the mesh, not from the volume; the mesh then carries components (the triangles of every component found,
        descending) and dropped_triangles.  A setup call (it synchronises).  ValueError when the volume holds no surface."""
        from .Utils import mesh_handle_from_tensors
        out = ops.tsdf_extract(*self.arrays(), self.origin, self.voxel, min_weight, keep)
        if int(out["faces"].shape[0]) == 0:
            raise ValueError("TsdfVolume.extract: no surface in the volume (no voxel pair on both sides of a surface was observed "
                             f"{min_weight} times: check the poses, the masks and the volume's bounds)")
        cols = out["vertex_color"].add(0.5).floor_().clamp_(0, 255)
        t = dict(pos=out["pos"], vnormals=out["vnormals"], faces=out["faces"], vertex_color=cols / 255.0)
        t["_handle"] = mesh_handle_from_tensors(t)
        cols = cols.to(torch.uint8).cpu().numpy()
        mesh = SimpleMesh(out["pos"].cpu().numpy(), out["faces"].cpu().numpy(), vertex_normals=out["vnormals"].cpu().numpy(),
                          vertex_colors=cols)
        if keep is not None:
            mesh.components, mesh.dropped_triangles = out["components"], out["dropped_triangles"]
        return mesh, t

    def raycast(self, ob_in_cams, K, size, bbox2d=None, step=None, min_weight=1, z_near=0.001, z_far=None,
                want=ops.RAYCAST_OUTPUTS):
        """what the volume looks like from the poses ob_in_cams (N,4,4), without extracting a mesh (ops.tsdf_raycast) -> a dict of
        device tensors: depth (N,h,w) metres, xyz and normal (N,h,w,3) in the camera frame, color (N,h,w,3) in the units of the
        fused rgb; zeros where a ray meets no surface.  K: one camera (3,3), or an ops.Views whose row n names the camera of pose n.
        size = (h, w): the frame, or with bbox2d ((N,4) device tensor, ops.crop_windows') the crops the windows are resampled into.
        step=None samples every voxel pitch of camera depth; z_far=None lets the rays run to the far side of the volume; only voxels
        observed min_weight times count.  One launch, no synchronisation."""
        P = _upload(_host(ob_in_cams), torch.float32, self.device)
        if P.dim() == 2:
            P = P[None]
        views = K if isinstance(K, ops.Views) else None
        h, w = int(size[0]), int(size[1])
        return ops.tsdf_raycast(*self.arrays(), self.origin, self.voxel, P.contiguous(), None if views is not None else K, h, w, (h, w),
                                bbox2d, step, min_weight, z_near, z_far, want, views=views)

    def depth_agreement(self, depths, masks, ob_in_cams, Ks, tol=None):
        """how well the volume, as fused so far, explains V posed views -> (V,4) int32 device tensor, the counts of
        ops.depth_agreement (ops.DepthAgreement.rows reads them) per view: the pixels where the volume shows a surface from the view's
        pose (`model`), those of them where the view has a masked depth (`valid`), those where the two depths are within tol
        (`agree`) and those where the view sees more than tol past the volume's surface (`behind`).  The volume's raycast depth, full
        frame, against each view's masked, back-projected depth; tol=None: two voxels."""
        what = "TsdfVolume.depth_agreement"
        if masks is None:
            raise ValueError(f"{what}: masks are required")
        tol = ops._check_tol(2.0 * self.voxel if tol is None else tol, what)
        d, _, m, P, K = _views_in(None, depths, masks, ob_in_cams, Ks, self.device, what)
        V, H, W = (int(x) for x in d.shape)
        if H < 2 or W < 2:
            raise ValueError(f"{what}: frames of {H} x {W} pixels (at least 2 x 2)")
        vt, xyz = _masked_xyz(d, m, K)
        r = ops.tsdf_raycast(*self.arrays(), self.origin, self.voxel, P.contiguous(), None, H, W, want=("depth",), views=vt)
        # the window that is the frame: crop pixel (i, j) reads texel (i, j)
        tf = torch.tensor([[W / (W - 1.0), 0.0, -0.5], [0.0, H / (H - 1.0), -0.5], [0.0, 0.0, 1.0]], dtype=torch.float32, device=self.device)
        return ops.depth_agreement(r["depth"], xyz, tf.repeat(V, 1, 1).contiguous(), tol, views=vt)

    def integrate_aligned(self, rgbs, depths, masks, ob_in_cams, Ks, iterations=3, max_dist=0.01, trusted=1):
        """fuses V views whose poses are only approximately known (a turntable, a robot arm, a previous tracker: a few millimetres and
        a degree or so off), one after the other: the first `trusted` views as given, every later view first aligned to the volume as
        fused so far (align_views_to_volume: `iterations` steps of point-to-plane ICP, pairs within max_dist) and then fused with the
        aligned pose -> the views' poses, (V,4,4) float32 on the device: the aligned pose of every view that was fused, the given one
        of the others.  A view one of whose steps could not be solved (too few pairs: it does not overlap what was fused before it)
        keeps the pose it was given and is left out of the volume, since nothing vouches for that pose; this is decided on the
        device, there is no host read per view.  Which views that were is `self.left_out` afterwards, a (V,) bool device tensor.
        This polishes pose guesses; it is not pose estimation from nothing: a view without a pose within reach of the ICP (about a
        centimetre) cannot be placed."""
        what = "TsdfVolume.integrate_aligned"
        if rgbs is None or masks is None:
            raise ValueError(f"{what}: rgbs and masks are required")
        iterations = _check_iterations(iterations, what)
        ops._check_icp(max_dist, 1e-3, 64, what)
        if isinstance(trusted, bool) or not isinstance(trusted, (int, np.integer)) or int(trusted) < 0:
            raise ValueError(f"{what}: trusted must be an int >= 0, got {trusted!r}")
        d, c, m, P, K = _views_in(rgbs, depths, masks, ob_in_cams, Ks, self.device, what)
        V = int(d.shape[0])
        t = min(int(trusted), V)
        self.left_out = torch.zeros((V,), dtype=torch.bool, device=self.device)
        if t > 0:
            self._integrate(d[:t], c[:t], m[:t], P[:t], K[:t])
        if t == V:
            return P
        side = _AlignSide(self, d, m, K)
        used = [P[:t]]
        nan = torch.full((1, 4, 4), float("nan"), dtype=torch.float32, device=self.device)
        for v in range(t, V):
            Q, bad = side.align(P[v:v + 1].contiguous(), side.vt.rows(v, v + 1), iterations, max_dist)
            self._integrate(d[v:v + 1], c[v:v + 1], m[v:v + 1], torch.where(bad[:, None, None], nan, Q), K[v:v + 1])   # a NaN pose: skipped
            used.append(torch.where(bad[:, None, None], P[v:v + 1], Q))
            self.left_out[v:v + 1] = bad
        return torch.cat(used)


def bake_texture(mesh_tensors, rgbs, depths, masks, ob_in_cams, Ks, texels=4, tol=None, min_cos=0.2, min_depth=0.001):
    """A texture atlas for a reconstructed mesh from the views it was fused from -> (SimpleMesh, mesh_tensors).  mesh_tensors: the
    device dict TsdfVolume.extract returns (pos, faces, vnormals, vertex_color in [0,1]); the views as TsdfVolume.integrate takes
    them.  Face f gets a texels x texels block of a square-ish atlas (ops.texture_bake: every texel is a point of its face, coloured
    from the views that face it within min_cos and whose depth there is within tol metres of it, blended by cos^2; a texel no view sees
    keeps the interpolated vertex colour).  tol is required: twice the voxel pitch of the fusion is what reconstruct_object passes.
    The atlas is rounded as the vertex colours are: floor(x + 0.5) clamped to 0..255.  The returned dict carries tex (1,Ht,Wt,3) in
    [0,1], uv (3F,2), uv_idx (F,3) and the unchanged pos, faces and vnormals; the SimpleMesh the same atlas as a uint8 image, uv in the
    file convention (u, 1 - v) with visual.uv_faces, and the vertex colours beside it (save_ply).  A setup call (it synchronises)."""
    what = "bake_texture"
    if tol is None:
        raise ValueError(f"{what}: tol is required (metres; about twice the voxel pitch the mesh was fused at)")
    if rgbs is None:
        raise ValueError(f"{what}: rgbs are required")
    _check_mesh_tensors(mesh_tensors, what)
    dev = mesh_tensors["pos"].device
    return _bake(mesh_tensors, *_views_in(rgbs, depths, masks, ob_in_cams, Ks, dev, what), texels, tol, min_cos, min_depth)


def _bake(t, d, c, m, P, K, texels, tol, min_cos, min_depth):
    """bake_texture of views that are on the device already"""
    from .Utils import mesh_handle_from_tensors
    vc = t.get("vertex_color")
    if vc is not None:
        vc = vc.mul(255.0).add_(0.5).floor_().clamp_(0, 255)               # the mesh's uint8 colours, in the units of rgb
    tex, coverage, uv, uv_idx = ops.texture_bake(t["pos"], t["faces"], vc, d, c, m, P, K, tol, min_cos, texels, None, min_depth)
    tex = tex.add_(0.5).floor_().clamp_(0, 255)
    out = dict(pos=t["pos"], vnormals=t["vnormals"], faces=t["faces"], tex=(tex / 255.0)[None], uv=uv, uv_idx=uv_idx)
    out["_handle"] = mesh_handle_from_tensors(out)
    uv_file = uv.double().cpu().numpy()
    uv_file[:, 1] = 1.0 - uv_file[:, 1]
    mesh = SimpleMesh(t["pos"].cpu().numpy(), t["faces"].cpu().numpy(), vertex_normals=t["vnormals"].cpu().numpy(), uv=uv_file,
                      texture=tex.to(torch.uint8).cpu().numpy(), uv_faces=uv_idx.cpu().numpy(),
                      vertex_colors=None if vc is None else vc.to(torch.uint8).cpu().numpy())
    mesh.visual.coverage = coverage.cpu().numpy()          # (Ht,Wt) uint8: how many views were blended into each texel
    return mesh, out


def bounds_from_views(depths, masks, ob_in_cams, Ks, margin=0.0, min_depth=0.001, device="cuda"):
    """the box (lo, hi: float64 (3,), object frame, metres) of the masked depth pixels of all views, grown by margin: the pixels are
    back-projected on the device (fp_depth_to_xyz_frames) and mapped to the object frame.  Every masked pixel counts, so a mask that
    covers background stretches the box.  ValueError when no masked pixel has a depth."""
    what = "bounds_from_views"
    if masks is None:
        raise ValueError(f"{what}: masks are required (without them the box is the whole scene's)")
    d, _, m, P, K = _views_in(None, depths, masks, ob_in_cams, Ks, device, what)
    return _bounds(d, m, P, K, margin, min_depth, what)


def _bounds(d, m, P, K, margin, min_depth, what):
    """bounds_from_views of views that are on the device already"""
    V = int(d.shape[0])
    xyz = ops.depth_to_xyz_frames(d, ops.Views(list(K), np.arange(V), d.device))          # (V,H,W,3), camera frame
    valid = (m != 0) & (d >= min_depth)
    cam_in_ob = torch.as_tensor(np.linalg.inv(P.double().cpu().numpy()), device=d.device, dtype=torch.float32)     # (V,4,4)
    R, t = cam_in_ob[:, :3, :3], cam_in_ob[:, :3, 3]
    lo, hi = [], []
    for k in range(3):
        q = (xyz[..., 0] * R[:, k, 0, None, None] + xyz[..., 1] * R[:, k, 1, None, None]) + xyz[..., 2] * R[:, k, 2, None, None] + t[:, k, None, None]
        lo.append(torch.where(valid, q, torch.full_like(q, float("inf"))).amin())
        hi.append(torch.where(valid, q, torch.full_like(q, float("-inf"))).amax())
    box = torch.stack(lo + hi).double().cpu().numpy()
    if not np.isfinite(box).all():
        raise ValueError(f"{what}: the masks are empty (no masked pixel of the {V} views has a depth of at least {min_depth} m)")
    return box[:3] - margin, box[3:] + margin


ICP_CROP = (160, 160)    # the crops refine_view_poses renders the mesh into, and their window's ratio to the mesh's sphere
ICP_CROP_RATIO = 1.2


def _check_iterations(iterations, what):
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or int(iterations) < 1:
        raise ValueError(f"{what}: iterations must be an int >= 1, got {iterations!r}")
    return int(iterations)


def refine_view_poses(mesh_tensors, depths, masks, ob_in_cams, Ks, iterations=3, max_dist=0.01):
    """Polish the poses of V reference views against a mesh of the object (a fused one: TsdfVolume.extract's mesh_tensors) by
    `iterations` Gauss-Newton steps of point-to-plane ICP per view (ops.icp_point_plane, view v for row v of an ops.Views): per
    iteration the crop windows around the object at the current poses, the mesh's camera-frame points and normals there, and one
    step against the view's own depth -- masked, and back-projected unfiltered.  The windows hold the sphere about the frame's origin
    that holds the mesh (the poses' frame need not be centred on it).  -> (poses (V,4,4) float32 device tensor, [ops.IcpStep] of the
    last iteration).  A view whose step cannot be solved (too few pairs) keeps its pose.  A setup call (it synchronises)."""
    what = "refine_view_poses"
    if masks is None:
        raise ValueError(f"{what}: masks are required")
    iterations = _check_iterations(iterations, what)
    ops._check_icp(max_dist, 1e-3, 64, what)
    _check_mesh_tensors(mesh_tensors, what)
    d, _, m, P, K = _views_in(None, depths, masks, ob_in_cams, Ks, mesh_tensors["pos"].device, what)
    return _refine_views(mesh_tensors, d, m, P, K, iterations, max_dist)


def _refine_views(t, d, m, P, K, iterations, max_dist):
    """refine_view_poses of views that are on the device already"""
    from .Utils import get_mesh_handle
    dev = d.device
    V, H, W = (int(x) for x in d.shape)
    vt, xyz = _masked_xyz(d, m, K)
    mset = ops.MeshSet([get_mesh_handle(t)])
    diam = ops.object_diameters([2.0 * float(t["pos"].norm(dim=1).max())], dev)
    oh, ow = ICP_CROP
    system = torch.empty((V, 40), dtype=torch.float64, device=dev)
    ws = ops.icp_workspace(V, oh, ow, dev)
    P = P.contiguous()
    for _ in range(iterations):
        tf, bb = ops.crop_windows(P, None, diam, ICP_CROP_RATIO, (ow, oh), views=vt)
        r = ops.render_crops(mset, P, bb, None, H, W, (oh, ow), diam, normalize_xyz=False, want=("xyz", "normal"), views=vt)
        P, _ = ops.icp_point_plane(r["xyz"], r["normal"], xyz, tf, P, max_dist, views=vt, system=system, workspace=ws)
    return P, ops.IcpStep.rows(system)


class _AlignSide:
    """what aligning views to a volume reuses from one step to the next: the views' table, their masked back-projected depth, the
    sphere about the frame's origin that holds the volume's box, and the buffers of the raycast and of the ICP step"""

    def __init__(self, vol, d, m, K):
        dev = d.device
        self.vol, self.H, self.W = vol, int(d.shape[1]), int(d.shape[2])
        self.vt, self.xyz = _masked_xyz(d, m, K)
        nz, ny, nx = vol.dims
        hi = vol.origin + (np.asarray([nx, ny, nz], dtype=np.float64) - 1.0) * vol.voxel
        self.diam = ops.object_diameters([2.0 * float(np.linalg.norm(np.maximum(np.abs(vol.origin), np.abs(hi))))], dev)
        self.bufs = {}

    def align(self, P, vt, iterations, max_dist, min_weight=1):
        """-> (poses (n,4,4), bad (n,) bool: a step of the row had a non-zero status), both on the device"""
        n, (oh, ow) = int(P.shape[0]), ICP_CROP
        if n not in self.bufs:
            dev = P.device
            self.bufs[n] = (dict(xyz=torch.empty((n, oh, ow, 3), dtype=torch.float32, device=dev),
                                 normal=torch.empty((n, oh, ow, 3), dtype=torch.float32, device=dev)),
                            torch.empty((n, 40), dtype=torch.float64, device=dev), ops.icp_workspace(n, oh, ow, dev))
        out, system, ws = self.bufs[n]
        vol = self.vol
        bad = torch.zeros((n,), dtype=torch.bool, device=P.device)
        for _ in range(iterations):
            tf, bb = ops.crop_windows(P, None, self.diam, ICP_CROP_RATIO, (ow, oh), views=vt)
            r = ops.tsdf_raycast(*vol.arrays(), vol.origin, vol.voxel, P, None, self.H, self.W, (oh, ow), bb, min_weight=min_weight,
                                 want=("xyz", "normal"), out=out, views=vt)
            P, _ = ops.icp_point_plane(r["xyz"], r["normal"], self.xyz, tf, P, max_dist, views=vt, system=system, workspace=ws)
            bad = bad | (system[:, 29] != 0)
        return P, bad


def align_views_to_volume(vol, depths, masks, ob_in_cams, Ks, iterations=3, max_dist=0.01):
    """refine_view_poses against the volume itself: the poses of V views polished by `iterations` Gauss-Newton steps of point-to-plane
    ICP per view against the zero surface of the TsdfVolume `vol`, raycast at the current poses (ops.tsdf_raycast) where
    refine_view_poses renders a mesh -- no extraction, no mesh handle, and no host synchronisation inside the loop.  The windows
    (ICP_CROP crops, ICP_CROP_RATIO) hold the sphere about the frame's origin that holds the volume's box; the sensor side is each
    view's own masked depth, back-projected unfiltered.  -> (poses (V,4,4) float32 device tensor, [ops.IcpStep] of the last iteration:
    read on the host after the loop).  A view whose step cannot be solved keeps its pose.  The poses must be within reach of the ICP
    (max_dist): this polishes pose guesses, it does not find a pose from nothing."""
    what = "align_views_to_volume"
    if not isinstance(vol, TsdfVolume):
        raise ValueError(f"{what}: vol must be a TsdfVolume, got {type(vol).__name__}")
    if masks is None:
        raise ValueError(f"{what}: masks are required")
    iterations = _check_iterations(iterations, what)
    ops._check_icp(max_dist, 1e-3, 64, what)
    d, _, m, P, K = _views_in(None, depths, masks, ob_in_cams, Ks, vol.device, what)
    side = _AlignSide(vol, d, m, K)
    P, _ = side.align(P.contiguous(), side.vt, iterations, max_dist)
    return P, ops.IcpStep.rows(side.bufs[int(d.shape[0])][1])


def reconstruct_object(rgbs, depths, masks, ob_in_cams, Ks, voxel=None, trunc=None, margin=None, min_weight=1, min_depth=0.001,
                       longest=128, device="cuda", texture=None, texture_min_cos=0.2, refine_poses=0, refine_iterations=3,
                       refine_max_dist=0.01, refine_against="mesh", keep_components=None):
    """V posed RGB-D reference views with masks -> (SimpleMesh, mesh_tensors) of the object, in the frame of the poses: the box of the
    masked depths (bounds_from_views) -> a TsdfVolume over it -> fuse -> extract.  voxel=None picks the pitch that gives the longest
    side `longest` voxels; margin defaults to three voxels around the observed points; trunc to four voxels.  texture=T (2..16) bakes a
    texture atlas of T x T texels a face from the same views onto the mesh (bake_texture with tol = two voxels): the mesh and the
    tensors then carry the atlas in place of the vertex colours alone.  refine_poses=R (default 0: the poses are trusted as given): R
    rounds of refine_view_poses of every view against the fused mesh (refine_iterations steps, pairs within refine_max_dist), each
    followed by a fresh fusion of the same volume from the refined poses and a new extraction; the texture is baked with the refined
    poses, and the mesh carries them as mesh.ob_in_cams ((V,4,4) float32).  refine_against="volume" polishes the views
    against the volume itself in those rounds (align_views_to_volume: no mesh is extracted between the rounds, only once at the end);
    "mesh" (the default) is the path described above.  keep_components ('largest', or the fewest triangles of a surface component
    that stays; None keeps all) drops floaters at every extraction of the call, those of the refine_poses rounds included
    (TsdfVolume.extract's keep): the mesh then carries components and dropped_triangles.  The volume is left as fused, so the
    rounds of refine_against="volume" still see a floater.  The mesh carries the pitch it was fused at as mesh.voxel.
    ValueError, naming the cause, when there are no views, the masks are empty or no surface was found."""
    what = "reconstruct_object"
    n = len(depths) if depths is not None else 0
    if n == 0:
        raise ValueError(f"{what}: no views")
    if rgbs is None or masks is None:
        raise ValueError(f"{what}: rgbs and masks are required")
    if isinstance(refine_poses, bool) or not isinstance(refine_poses, (int, np.integer)) or int(refine_poses) < 0:
        raise ValueError(f"{what}: refine_poses must be an int >= 0, got {refine_poses!r}")
    if refine_against not in ("mesh", "volume"):
        raise ValueError(f"{what}: refine_against must be 'mesh' or 'volume', got {refine_against!r}")
    keep_components = ops._check_keep(what, keep_components, "keep_components")
    if texture is not None:
        ops.texture_atlas_layout(1, texture)          # a block side outside 2..16 is refused before the fusion
    d, c, m, P, K = _views_in(rgbs, depths, masks, ob_in_cams, Ks, device, what)
    lo, hi = _bounds(d, m, P, K, 0.0, min_depth, what)
    side = float((hi - lo).max())
    if voxel is None:
        voxel = max(side, 1e-6) / (int(longest) - 1 - 2 * PAD_VOXELS)
    voxel = float(voxel)
    margin = PAD_VOXELS * voxel if margin is None else float(margin)
    lo, hi = lo - margin, hi + margin
    nx, ny, nz = (int(np.ceil(e / voxel - 1e-9)) + 1 for e in (hi - lo))
    vol = TsdfVolume(lo, (nz, ny, nx), voxel, trunc, device, min_depth)
    vol._integrate(d, c, m, P, K)
    by_volume = refine_against == "volume" and int(refine_poses) > 0
    side = _AlignSide(vol, d, m, K) if by_volume else None          # the views' side once for all rounds
    for _ in range(int(refine_poses) if by_volume else 0):          # no mesh and no host read between the rounds: one extraction, below
        P, _ = side.align(P.contiguous(), side.vt, int(refine_iterations), refine_max_dist, min_weight)
        vol.reset()
        vol._integrate(d, c, m, P, K)
    try:
        mesh, tensors = vol.extract(min_weight, keep_components)
    except ValueError as e:
        if "no surface" not in str(e):             # keep_components asks for more triangles than any component has
            raise
        raise ValueError(f"{what}: no surface found in the {n} views" + (" after refining their poses" if by_volume else "") + f" ({e})") from None
    for _ in range(0 if by_volume else int(refine_poses)):
        P, _ = _refine_views(tensors, d, m, P, K, int(refine_iterations), refine_max_dist)
        vol.reset()
        vol._integrate(d, c, m, P, K)
        try:
            mesh, tensors = vol.extract(min_weight, keep_components)
        except ValueError as e:
            if "no surface" not in str(e):
                raise
            raise ValueError(f"{what}: no surface found in the {n} views after refining their poses ({e})") from None
    report = (mesh.components, mesh.dropped_triangles) if keep_components is not None else None
    if texture is not None:
        mesh, tensors = _bake(tensors, d, c, m, P, K, int(texture), 2.0 * voxel, texture_min_cos, min_depth)
    if report is not None:
        mesh.components, mesh.dropped_triangles = report
    if int(refine_poses) > 0:
        mesh.ob_in_cams = P.cpu().numpy()
    mesh.voxel = voxel                                # the pitch it was fused at: the unit of compare_meshes' default thresholds
    return mesh, tensors


# ------------------------------------------------------------------ how good is a mesh: surface samples and their exact distances
_R2 = (0.7548776662466927, 0.5698402909980532)      # 1/g, 1/g^2 with g the plastic number: the R2 low-discrepancy sequence
SEED_STRIDE = 7919                                  # seed s shifts the sequence's index by s * SEED_STRIDE
DEFAULT_THRESHOLD_UNITS = (0.5, 1.0, 2.0, 4.0)      # compare_meshes' thresholds, in multiples of unit=


def _surface_strata(pos, faces, n, seed):
    """what sample_surface and its numpy stand-in share, float64 on the host (one order of summation): the cumulative face areas
    (F,), the n area coordinates (i + 0.5) / n * total, and the (n,3) float32 barycentric weights of the points.  pos (Nv,3), faces
    (F,3) host arrays.  A face whose area is not finite, or with an index outside the table, counts as 0."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < len(pos))).all(axis=1)
    fz = np.where(ok[:, None], faces, 0)
    with np.errstate(all="ignore"):
        a, b, c = (pos[fz[:, k]] for k in range(3)) if len(pos) else (np.zeros((len(faces), 3)),) * 3
        area = 0.5 * np.sqrt((np.cross(b - a, c - a) ** 2).sum(axis=1))
    area = np.where(ok & np.isfinite(area), area, 0.0)
    cum = np.cumsum(area)
    total = float(cum[-1]) if len(cum) else 0.0
    if not total > 0.0:
        raise ValueError("sample_surface: the mesh has no area (no face, or only degenerate ones)")
    i = np.arange(n, dtype=np.float64)
    target = (i + 0.5) / n * total
    k = i + 1.0 + float(int(seed)) * SEED_STRIDE
    r1, r2 = np.modf(0.5 + k * _R2[0])[0], np.modf(0.5 + k * _R2[1])[0]
    su = np.sqrt(r1)                                 # uniform over the triangle: (1 - sqrt r1, sqrt r1 (1 - r2), sqrt r1 r2)
    w = np.stack([1.0 - su, su * (1.0 - r2), su * r2], axis=1).astype(np.float32)
    return cum, target, w


def _mesh_arrays(m, device, what, name):
    """a mesh-tensor dict (pos, faces on a device) or a SimpleMesh -> (pos (Nv,3) float32, faces (F,3) int32) device tensors"""
    if isinstance(m, dict):
        for k in ("pos", "faces"):
            if k not in m:
                raise ValueError(f"{what}: {name} has no '{k}'")
        pos, faces = m["pos"], m["faces"]
        if not (torch.is_tensor(pos) and torch.is_tensor(faces)):
            raise ValueError(f"{what}: {name}'s pos and faces must be tensors")
    elif hasattr(m, "vertices") and hasattr(m, "faces"):
        pos, faces = torch.as_tensor(np.asarray(m.vertices, dtype=np.float32)), torch.as_tensor(np.asarray(m.faces).astype(np.int32))
    else:
        raise ValueError(f"{what}: {name} must be a mesh-tensor dict or a mesh with vertices and faces, got {type(m).__name__}")
    if pos.dim() != 2 or int(pos.shape[1]) != 3 or faces.dim() != 2 or int(faces.shape[1]) != 3:
        raise ValueError(f"{what}: {name} needs pos (Nv,3) and faces (F,3), got {tuple(pos.shape)} and {tuple(faces.shape)}")
    if device is None:
        device = pos.device
    return pos.to(device=device, dtype=torch.float32).contiguous(), faces.to(device=device, dtype=torch.int32).contiguous()


def _check_count(n, what, name):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) < 1:
        raise ValueError(f"{what}: {name} must be an int >= 1, got {n!r}")
    return int(n)


def sample_surface(mesh_tensors, n, seed=0):
    """n points on the surface of a mesh, area-weighted and reproducible -> (points (n,3) float32, face (n,) int64: the face of each),
    on the device of the mesh.  mesh_tensors: a dict with pos (Nv,3) f32 and faces (F,3) int32 on a device, or a SimpleMesh (then on
    the current device).  Stratified: point i sits at the area coordinate (i + 0.5) / n of the float64 cumulative face areas, found by
    searchsorted, so face f gets n * area_f / total points to within one; inside its face the point has the barycentrics of the
    R2 low-discrepancy pair at index i + 1 + seed * SEED_STRIDE, folded onto the triangle.  The area table and the weights are
    made on the host in float64 (the one summation order the definition has; a setup call: it reads the mesh back once); the search,
    the gather and the float32 combination (a*w0 + b*w1) + c*w2 run on the device in plain torch."""
    what = "sample_surface"
    n = _check_count(n, what, "n")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or int(seed) < 0:
        raise ValueError(f"{what}: seed must be an int >= 0, got {seed!r}")
    pos, faces = _mesh_arrays(mesh_tensors, None if isinstance(mesh_tensors, dict) else "cuda", what, "mesh_tensors")
    return _sample_surface_area(pos, faces, n, seed)[:2]


def _sample_surface_area(pos, faces, n, seed):
    """sample_surface on checked device tensors -> (points, face, the mesh's area: the total of the float64 table the strata are cut
    from), from the one read of the mesh"""
    cum, target, w = _surface_strata(pos.cpu().numpy(), faces.cpu().numpy(), n, seed)
    dev = pos.device
    f = torch.searchsorted(torch.as_tensor(cum, device=dev), torch.as_tensor(target, device=dev), right=True)
    f = f.clamp_(max=int(faces.shape[0]) - 1)
    idx = faces[f].long()
    w = torch.as_tensor(w, device=dev)
    a, b, c = pos[idx[:, 0]], pos[idx[:, 1]], pos[idx[:, 2]]
    return ((a * w[:, 0:1] + b * w[:, 1:2]) + c * w[:, 2:3]).contiguous(), f, float(cum[-1])


def _thresholds(thresholds, unit, what):
    if thresholds is None:
        if unit is None:
            raise ValueError(f"{what}: pass unit= (a length, for example the voxel pitch: the thresholds are "
                             f"{DEFAULT_THRESHOLD_UNITS} times it) or thresholds=")
        unit = float(unit)
        if not (np.isfinite(unit) and unit > 0):
            raise ValueError(f"{what}: unit must be a positive length, got {unit!r}")
        return tuple(m * unit for m in DEFAULT_THRESHOLD_UNITS)
    thr = tuple(float(t) for t in np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if not thr or not all(np.isfinite(t) and t >= 0 for t in thr):
        raise ValueError(f"{what}: thresholds must be finite lengths >= 0, got {thresholds!r}")
    return thr


def _rigid_tf(tf, what):
    """tf= of compare_meshes: a (4,4) transform or an ops.MeshAlignment -> (4,4) float64"""
    m = np.asarray(tf.tf if isinstance(tf, ops.MeshAlignment) else tf, dtype=np.float64)
    if m.shape != (4, 4) or not np.isfinite(m).all():
        raise ValueError(f"{what}: tf must be a finite (4,4) transform or a MeshAlignment, got shape {m.shape}")
    return m


def align_meshes(a, b, starts=300, samples=(128, 2048), iterations=(12, 20), max_dist=None, min_overlap=0.5, init=None, seed=0,
                 device=None, accel=None):
    """Register mesh a onto mesh b with no initial guess -> ops.MeshAlignment: `tf` (4,4) float64 maps a's coordinates into b's frame
    (one unit: no scale is estimated, and no reflection), with the mean and root-mean-square distance of a's samples to b's
    surface, the fraction of them that found a pair, and `runner_up`, the best other basin (a symmetric or nearly symmetric object
    has one of the same cost).  a, b: mesh-tensor dicts (pos, faces) or SimpleMeshes.  The direction is a's samples onto b's surface:
    a fused mesh may lack its underside, a CAD model does not.  mesh_align.align has the recipe -- `starts` seeded rotations and the
    identity, iterations[0] point-to-plane steps of all of them on samples[0] surface samples (sample_surface, seed + 1), the best
    distinct basins refined by iterations[1] steps on samples[1] samples (seed) under a shrinking gate on the pair distance, never
    above max_dist (None: no limit) -- and this function binds it to the device: every step of every candidate is one
    ops.mesh_icp_step call (starts x samples x faces pair tests), the transforms ping-pong between two device tables and come back to
    the host once per stage and per gate.  init: a (4,4) or (S,4,4) guess in the place of the starts (a local refinement).  A setup /
    evaluation call: it reads the meshes back once and synchronises a handful of times.  accel="grid": every step is answered through
    a uniform grid over mesh b (ops.mesh_grid_build, built here once and kept in b under "grid" when b is a dict of device tensors):
    the same alignment bit for bit.  It pays only for samples within about a cell of b's surface and a b of tens of thousands of
    faces or more: a local refinement from a good init= (the fine stage's step then took 0.9 ms against 16 ms at 401 672 faces).
    The default policy's starts put most samples several cells from b, where every measured size was 9 to 15 times slower through
    the grid, and a start that puts a far from b walks the whole grid and tests every stored triangle from global memory (DESIGN.md
    section 6): those stay on None, brute force, the default."""
    from . import mesh_align, symmetry
    what = "align_meshes"
    try:
        n_coarse, n_fine = samples
    except (TypeError, ValueError):
        raise ValueError(f"{what}: samples must be two counts (coarse, fine), got {samples!r}") from None
    n_coarse, n_fine = _check_count(n_coarse, what, "samples[0]"), _check_count(n_fine, what, "samples[1]")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or int(seed) < 0:
        raise ValueError(f"{what}: seed must be an int >= 0, got {seed!r}")
    if device is None:
        device = next((m["pos"].device for m in (a, b) if isinstance(m, dict) and torch.is_tensor(m.get("pos"))), "cuda")
    ta, tb = (dict(zip(("pos", "faces"), _mesh_arrays(m, device, what, name))) for m, name in ((a, "a"), (b, "b")))
    pts = {"coarse": sample_surface(ta, n_coarse, int(seed) + 1)[0], "fine": sample_surface(ta, n_fine, int(seed))[0]}
    centre_b, radius_b = symmetry.surface_centre(tb["pos"].cpu().numpy(), tb["faces"].cpu().numpy())
    centre_a = pts["coarse"].double().mean(dim=0).cpu().numpy()
    dev = tb["pos"].device
    grid = _accel_grid(accel, tb, what, keep=b)

    def steps(which, tfs, gate, n):
        p = pts[which]
        S, Q = len(tfs), int(p.shape[0])
        cur = torch.as_tensor(np.ascontiguousarray(tfs, dtype=np.float32), device=dev)
        nxt = torch.empty_like(cur)
        system = torch.empty((S, 40), dtype=torch.float64, device=dev)
        ws = ops.mesh_icp_workspace(S, Q, dev)
        for _ in range(n):
            ops.mesh_icp_step(p, cur, tb, max_dist=gate, out=dict(tfs_out=nxt, system=system), workspace=ws, grid=grid)
            cur, nxt = nxt, cur
        _, _, extra = ops.mesh_icp_step(p, cur, tb, max_dist=gate, want=("dist2",), out=dict(tfs_out=nxt, system=system), workspace=ws,
                                        grid=grid)
        return cur.cpu().numpy().astype(np.float64), system.cpu().numpy(), extra["dist2"].cpu().numpy()

    got = mesh_align.align(steps, centre_a, centre_b, radius_b, (n_coarse, n_fine), starts=starts, iterations=iterations,
                           max_dist=max_dist, min_overlap=min_overlap, init=init, seed=int(seed))
    return ops.MeshAlignment(*(got[k] for k in ops.MeshAlignment._fields))


def _accel_grid(accel, t, what, keep=None):
    """accel=None: no grid (brute force); "grid": ops.mesh_grid_build of the mesh-tensor dict t, kept in it under "grid" -- or in
    keep, the caller's own dict that t was made from, where t holds that dict's very tensors"""
    if accel is None:
        return None
    if accel != "grid":
        raise ValueError(f"{what}: accel must be None or 'grid', got {accel!r}")
    if isinstance(keep, dict) and ops.MeshGrid.key_of(keep["pos"], keep["faces"]) == ops.MeshGrid.key_of(t["pos"], t["faces"]):
        return ops.mesh_grid_build(keep)
    return ops.mesh_grid_build(t)


def _coverage_views(ob_in_cams, Ks, hw, rel_tol, min_cos, what):
    """the views of view_coverage and its numpy stand-in, checked, float64 on the host -> (P (V,4,4), K (V,3,3), eyes (V,3) float32:
    -R^T t of each pose taken through float64 and rounded once, (H, W), rel_tol, min_cos)"""
    P = np.asarray(_host(ob_in_cams), dtype=np.float64)
    if P.ndim != 3 or P.shape[1:] != (4, 4) or not np.isfinite(P).all():
        raise ValueError(f"{what}: ob_in_cams must be finite (V,4,4) poses, got shape {P.shape}")
    K = np.asarray(_host(Ks), dtype=np.float64)
    if K.shape == (3, 3):
        K = np.broadcast_to(K, (len(P), 3, 3))
    if K.shape != (len(P), 3, 3) or not np.isfinite(K).all():
        raise ValueError(f"{what}: Ks must be finite (3,3) or (V,3,3) intrinsics for {len(P)} views, got shape {K.shape}")
    try:
        H, W = (int(x) for x in hw)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: hw must be (height, width), got {hw!r}") from None
    if H < 1 or W < 1:
        raise ValueError(f"{what}: hw must be (height, width) >= 1, got {hw!r}")
    rel_tol, min_cos = ops._check_rel_tol(what, rel_tol), float(min_cos)
    if not 0.0 <= min_cos < 1.0:
        raise ValueError(f"{what}: min_cos must be in [0, 1), got {min_cos!r}")
    eyes = (-np.einsum("vji,vj->vi", P[:, :3, :3], P[:, :3, 3])).astype(np.float32)
    return P, np.ascontiguousarray(K), eyes, (H, W), rel_tol, min_cos


def _in_frame_and_facing(xp, p, n, P, K, eyes, hw, min_cos):
    """what view_coverage and its numpy stand-in share, float64, one order of operations: (V,n) bool, sample i projects inside view
    v's frame at positive depth and its face looks at the eye.  xp: torch or numpy; p (n,3) the samples and n (n,3) their faces'
    normals ab x ac, P (V,4,4), K (V,3,3), eyes (V,3), all float64 arrays of xp.  The pixel of a projection is floor(u + 0.5), as
    everywhere in the library; facing is cos > min_cos on the face normal, for min_cos = 0 the sign of a dot product."""
    H, W = hw
    x, y, z = (p[None, :, k] for k in range(3))
    cam = [((P[:, k, 0, None] * x + P[:, k, 1, None] * y) + P[:, k, 2, None] * z) + P[:, k, 3, None] for k in range(3)]
    Z = cam[2]
    front = Z > 0
    Zs = xp.where(front, Z, xp.ones_like(Z))
    u = xp.floor(((K[:, 0, 0, None] * cam[0]) / Zs + K[:, 0, 2, None]) + 0.5)
    v = xp.floor(((K[:, 1, 1, None] * cam[1]) / Zs + K[:, 1, 2, None]) + 0.5)
    inside = front & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    view = [eyes[:, k, None] - p[None, :, k] for k in range(3)]
    dotv = (n[None, :, 0] * view[0] + n[None, :, 1] * view[1]) + n[None, :, 2] * view[2]
    if min_cos == 0.0:
        return inside & (dotv > 0)
    nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    vv = (view[0] * view[0] + view[1] * view[1]) + view[2] * view[2]
    return inside & (dotv > min_cos * xp.sqrt(nn[None, :] * vv))


def view_coverage(mesh, ob_in_cams, Ks, hw, samples=100_000, seed=0, rel_tol=1e-4, min_cos=0.0, accel=None):
    """What of a mesh's surface did a set of views see -> ops.ViewCoverage: per surface sample the number of views that see it (`seen`,
    on the device), the fraction of the surface that at least one view sees, the fraction each view sees, and the unseen area.
    mesh: a mesh-tensor dict (pos, faces) or a SimpleMesh; ob_in_cams (V,4,4) the object's pose in each camera, Ks (3,3) or (V,3,3),
    hw = (height, width) of the views' frames, all in the mesh's frame and unit.  The samples are sample_surface's (area-stratified,
    so a fraction of samples is a fraction of area; seed).  View v sees sample i when the sample projects inside the frame at
    positive depth, its face looks at the eye (cos > min_cos on the face normal ab x ac: the texture bake's facing test), and
    ops.mesh_visibility from the view's eye (-R^T t, through float64, rounded once) says no face of the mesh lies between; rel_tol
    is relative to the distance from the eye to the sample (ops.mesh_visibility).  Brute force: V x samples x faces pair tests, a
    setup / evaluation call, and it synchronises (the mesh is read back once by the sampler, and the table once for the statistics,
    float64 on the host).  accel must be None: answering the rays through the uniform grid (a 3D-DDA walk) is not built yet."""
    what = "view_coverage"
    samples = _check_count(samples, what, "samples")
    if accel is not None:
        if accel == "grid":
            raise NotImplementedError(f"{what}: accel='grid' is not built yet: ray queries through the uniform grid (a 3D-DDA walk with "
                                      f"a float32 proof of its own) are the follow-up; pass accel=None (brute force)")
        raise ValueError(f"{what}: accel must be None, got {accel!r}")
    views = _coverage_views(ob_in_cams, Ks, hw, rel_tol, min_cos, what)
    t = dict(zip(("pos", "faces"), _mesh_arrays(mesh, None if isinstance(mesh, dict) else "cuda", what, "mesh")))
    return _coverage_of_samples(t, *_sample_surface_area(t["pos"], t["faces"], samples, seed), *views)


def _coverage_of_samples(t, pts, f, area, P, K, eyes, hw, rel_tol, min_cos):
    """view_coverage of the samples (pts, f) of the mesh-tensor dict t, whose area is `area`, from checked views (_coverage_views)"""
    dev = pts.device
    idx = t["faces"][f].long()
    a, b, c = (t["pos"][idx[:, k]].double() for k in range(3))
    ab, ac = b - a, c - a
    n = torch.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                     ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], dim=1)
    eyes_d = torch.as_tensor(eyes, device=dev)
    table = _in_frame_and_facing(torch, pts.double(), n, torch.as_tensor(P, device=dev), torch.as_tensor(K, device=dev),
                                 eyes_d.double(), hw, min_cos)
    table &= ops.mesh_visibility(pts, eyes_d, t, rel_tol=rel_tol)
    return ops.ViewCoverage.from_seen(table, pts, f, area)


def compare_meshes(a, b, samples=100_000, thresholds=None, seed=0, unit=None, device=None, tf=None, accel=None, seen_from=None):
    """How good is mesh a (what was built) against mesh b (the reference) -> ops.MeshComparison: accuracy (the exact distances of
    `samples` surface samples of a to the surface of b: mean / median / p99 / max), completeness (b's samples to a's surface), the
    chamfer distance (the mean of the two means), the Hausdorff distance of the samples, and per threshold precision, recall and
    F-score; the two distance arrays stay on the device.  a, b: mesh-tensor dicts (pos, faces) or SimpleMeshes, in one frame and one
    unit.  thresholds: lengths; None: DEFAULT_THRESHOLD_UNITS times unit= (for example the voxel pitch of the fusion).  The samples
    are sample_surface's (seed), the distances ops.mesh_point_distance's: brute force, samples x faces pair tests in each direction.
    A setup / evaluation call, and it synchronises: sample_surface reads each mesh back once for its float64 area table, and the two
    distance arrays are read once at the end for the statistics (float64 on the host).  tf: a (4,4) transform or an
    ops.MeshAlignment (align_meshes) that takes a's coordinates into b's frame, applied to a's vertices (in float64, rounded once)
    before anything is sampled; None: the meshes are in one frame already.  accel="grid": the distances are answered through a
    uniform grid over each mesh (ops.mesh_grid_build, built here once per mesh): the same report bit for bit, from far fewer pair
    tests; None: brute force.  seen_from: a dict(ob_in_cams=, Ks=, hw=) of views in b's frame (and rel_tol= / min_cos=, as
    view_coverage takes them): b's samples are restricted to those view_coverage reports seen by at least one of the views, so that
    completeness, recall and b's side of chamfer and hausdorff no longer charge a for what no view could see (the underside of an
    object fused from a ring of views); the report's `coverage` is the fraction of b's samples kept; views that see none of
    them are refused.  None: every sample of b."""
    what = "compare_meshes"
    samples = _check_count(samples, what, "samples")
    thr = _thresholds(thresholds, unit, what)
    views = None
    if seen_from is not None:
        if not isinstance(seen_from, dict) or not {"ob_in_cams", "Ks", "hw"} <= set(seen_from) <= {"ob_in_cams", "Ks", "hw", "rel_tol",
                                                                                                  "min_cos"}:
            raise ValueError(f"{what}: seen_from must be a dict with ob_in_cams, Ks, hw (and rel_tol, min_cos), got {seen_from!r}")
        views = _coverage_views(seen_from["ob_in_cams"], seen_from["Ks"], seen_from["hw"], seen_from.get("rel_tol", 1e-4),
                                seen_from.get("min_cos", 0.0), f"{what}: seen_from")
    if device is None:
        device = next((m["pos"].device for m in (a, b) if isinstance(m, dict) and torch.is_tensor(m.get("pos"))), "cuda")
    ta, tb = (dict(zip(("pos", "faces"), _mesh_arrays(m, device, what, name))) for m, name in ((a, "a"), (b, "b")))
    if tf is not None:
        m = torch.as_tensor(_rigid_tf(tf, what), device=ta["pos"].device)
        ta["pos"] = (ta["pos"].double() @ m[:3, :3].T + m[:3, 3]).float().contiguous()
    pa, _ = sample_surface(ta, samples, seed)
    pb, fb, area_b = _sample_surface_area(tb["pos"], tb["faces"], samples, seed)      # sample_surface(tb, samples, seed), and b's area
    coverage = None
    if views is not None:
        cov = _coverage_of_samples(tb, pb, fb, area_b, *views)
        if cov.fraction == 0.0:
            raise ValueError(f"{what}: seen_from: none of b's {samples} samples is seen by any of the {len(cov.per_view)} views (are the "
                             f"poses in b's frame and unit?): completeness over nothing is not a figure")
        pb, coverage = pb[cov.seen > 0].contiguous(), cov.fraction
    # the square root through float64: the correctly rounded float32 root whatever the device's float32 sqrt does in its last bit
    d_ab = ops.mesh_point_distance(pa, tb, want=("dist2",), grid=_accel_grid(accel, tb, what))["dist2"].double().sqrt_().float()
    d_ba = ops.mesh_point_distance(pb, ta, want=("dist2",), grid=_accel_grid(accel, ta, what))["dist2"].double().sqrt_().float()
    report = ops.MeshComparison.from_distances(d_ab, d_ba, thr)
    return report if coverage is None else report._replace(coverage=coverage)


def _signed(points, mesh, what, allow_open, accel=None):
    """-> (sign (Q,) int32, dist (Q,) float32) device tensors of the points against a mesh-tensor dict or a SimpleMesh"""
    if not torch.is_tensor(points):
        points = torch.as_tensor(np.asarray(points, dtype=np.float32))
    if points.dim() != 2 or int(points.shape[1]) != 3:
        raise ValueError(f"{what}: points must be (Q,3), got {tuple(points.shape)}")
    if isinstance(mesh, dict) and torch.is_tensor(mesh.get("pos")) and mesh["pos"].is_cuda and mesh["pos"].dtype == torch.float32 \
            and torch.is_tensor(mesh.get("faces")) and mesh["faces"].dtype == torch.int32:
        t = mesh                                       # the caller's dict as it is: its pseudonormal tables are kept in it
    else:
        t = dict(zip(("pos", "faces"), _mesh_arrays(mesh, points.device if points.is_cuda else "cuda", what, "mesh")))
    pts = points.to(device=t["pos"].device, dtype=torch.float32).contiguous()
    r = ops.mesh_signed_distance(pts, t, want=("dist2", "sign"), allow_open=allow_open, grid=_accel_grid(accel, t, what))
    # the square root through float64, as compare_meshes takes it
    return r["sign"], r["dist2"].double().sqrt_().float()


def signed_distance(points, mesh, allow_open=False, accel=None):
    """The signed distance of the points (Q,3) to the surface of a closed mesh -> (Q,) float32 on the mesh's device: negative inside,
    positive outside, +0 on the surface; +inf for a point that no triangle answers (a NaN point).  mesh: a mesh-tensor dict (pos,
    faces; the pseudonormal tables are computed at the first call and kept in it) or a SimpleMesh.  ops.mesh_signed_distance has the
    definition, the cost (points x faces pair tests) and the refusal of a mesh that is not closed (allow_open=True: the side of the
    nearest face).  accel="grid": answered through a uniform grid over the mesh (ops.mesh_grid_build; built at the first call and kept
    in a mesh-tensor dict beside the tables): the same bits from far fewer pair tests."""
    sign, dist = _signed(points, mesh, "signed_distance", allow_open, accel)
    return torch.where(sign < 0, -dist, dist)


def contains(points, mesh, allow_open=False, accel=None):
    """Is each of the points (Q,3) inside the closed mesh -> (Q,) bool on the mesh's device.  A point on the surface, and a point
    that is not finite, is not inside.  See signed_distance."""
    return _signed(points, mesh, "contains", allow_open, accel)[0] < 0


def signed_bias(a, b, samples=100_000, seed=0, tf=None, device=None, allow_open=False, accel=None):
    """On which side of mesh b (the reference, closed) does the surface of mesh a (what was built) lie -> ops.SignedStats: the mean
    signed distance of `samples` surface samples of a to b's surface (negative inside b: a positive mean says a is inflated, a
    negative one that it is shrunk), the share of the samples inside b, and the 5th, 50th and 95th percentiles.  The samples are
    compare_meshes's accuracy samples (sample_surface, the same seed), so abs(mean) is at most that comparison's accuracy mean; a, b,
    tf, device and accel as there.  A setup / evaluation call: it synchronises."""
    what = "signed_bias"
    samples = _check_count(samples, what, "samples")
    if device is None:
        device = next((m["pos"].device for m in (a, b) if isinstance(m, dict) and torch.is_tensor(m.get("pos"))), "cuda")
    ta, tb = (dict(zip(("pos", "faces"), _mesh_arrays(m, device, what, name))) for m, name in ((a, "a"), (b, "b")))
    if tf is not None:
        m = torch.as_tensor(_rigid_tf(tf, what), device=ta["pos"].device)
        ta["pos"] = (ta["pos"].double() @ m[:3, :3].T + m[:3, 3]).float().contiguous()
    pa, _ = sample_surface(ta, samples, seed)
    sign, dist = _signed(pa, tb, what, allow_open, accel)
    return ops.SignedStats.of((sign.double() * dist.double()).cpu().numpy())


# ------------------------------------------------------------------ which rotations map a mesh onto itself
def detect_symmetries(mesh_tensors, tol=None, max_order=6, rot_angle_discrete=5, samples=(64, 512), n_axes=800, accel=None):
    """The rotational symmetries of a mesh -> symmetry.Symmetries: tfs (S,4,4) float64 with the identity first (what the estimator's
    symmetry_tfs, make_rotation_grid, pose_errors(want="sym"), MSSD, MSPD and cluster_poses take), the axes with their orders
    (math.inf for a continuous one, which contributes a rotation every rot_angle_discrete degrees), tol and the residual of each
    transform.  mesh_tensors: a dict with pos and faces on a device, or a SimpleMesh (then on the current device).  tol: how far a
    symmetry may move the surface off itself, a length; None: 1 % of twice the largest vertex distance from the surface's centroid.
    For a fused mesh give it the noise of the fusion: a couple of voxels.  samples: the numbers of surface samples of the coarse scan
    (sample_surface, seed 1) and of the refinement and the final check (seed 0).  Only geometry is considered: a can whose label is
    not symmetric is still reported as symmetric; only proper rotations are looked for.  symmetry.find_symmetries has the recipe; this
    function binds its two callables to the device: ops.mesh_transform_residuals for the largest distance per candidate transform
    (one call per order over all n_axes candidate axes) and ops.mesh_point_distance for the closest points of a refinement step.  A
    setup call: it reads the mesh back once and synchronises at every step of the policy.  accel="grid": both callables are answered
    through a uniform grid over the mesh (ops.mesh_grid_build, built here once and kept in mesh_tensors under "grid" when that is a
    dict of device tensors): the same record bit for bit.  Measured, it does not pay here: a candidate rotation that is no symmetry
    puts the samples several cells from the surface, and the coarse scan's call was 9 to 13 times slower through the grid at 4 900
    to 401 672 faces (the grid is for samples within about a cell of the surface, and a transformed sample far
    from the mesh walks the whole grid and tests every stored triangle from global memory).  None: brute force, the default."""
    from . import symmetry
    what = "detect_symmetries"
    pos, faces = _mesh_arrays(mesh_tensors, None if isinstance(mesh_tensors, dict) else "cuda", what, "mesh_tensors")
    try:
        n_coarse, n_fine = samples
    except (TypeError, ValueError):
        raise ValueError(f"{what}: samples must be two counts (coarse, fine), got {samples!r}") from None
    n_coarse, n_fine = _check_count(n_coarse, what, "samples[0]"), _check_count(n_fine, what, "samples[1]")
    centre, radius = symmetry.surface_centre(pos.cpu().numpy(), faces.cpu().numpy())
    if tol is None:
        tol = 0.01 * 2.0 * radius
    tol = float(tol)
    if not (np.isfinite(tol) and tol > 0):
        raise ValueError(f"{what}: tol must be a positive length, got {tol!r}")
    mesh = dict(pos=pos, faces=faces)
    pts = {"coarse": sample_surface(mesh, n_coarse, seed=1)[0], "fine": sample_surface(mesh, n_fine, seed=0)[0]}
    fine64 = pts["fine"].cpu().numpy().astype(np.float64)
    grid = _accel_grid(accel, mesh, what, keep=mesh_tensors)

    def residuals(tfs, which):
        m = torch.as_tensor(np.ascontiguousarray(tfs, dtype=np.float32), device=pos.device)
        d2 = ops.mesh_transform_residuals(pts[which], m, mesh, want=("max_d2",), grid=grid)["max_d2"]
        return np.sqrt(d2.cpu().numpy().astype(np.float64))

    def closest(tf):
        m = torch.as_tensor(np.ascontiguousarray(tf, dtype=np.float32), device=pos.device)
        moved = (pts["fine"] @ m[:3, :3].T + m[:3, 3]).contiguous()
        return fine64, ops.mesh_point_distance(moved, mesh, want=("closest",), grid=grid)["closest"].cpu().numpy().astype(np.float64)

    return symmetry.find_symmetries(residuals, closest, centre, radius, tol, max_order=max_order, n_axes=n_axes,
                                    rot_angle_discrete=rot_angle_discrete)
