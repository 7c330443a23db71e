"""The crop stage both predictors run per call -- crop windows -> rendered crop (A) -> observed crop (B) -- in one copy (crop_stage),
and who looks at what in it (Scene: the cameras and objects of a call's hypotheses, in the form the geometry ops take)."""
import numpy as np
import torch

from . import ops


class Scene:
    """mesh: an ops.MeshHandle, or an ops.MeshSet with diameter = its ops.object_diameters table; K: the intrinsics (unused with views);
    H, W: the frame size; n hypotheses; obj: their object index -- a predict_pose_refine.ObjectIndex (it carries the rows of the two-pose
    quirk) or the bare int32 device tensor -- or None; views: their ops.Views or None.  `who` names the caller in a refusal."""

    def __init__(self, mesh, diameter, K, H, W, n, obj=None, views=None, who="Scene"):
        n = int(n)
        if obj is not None and len(obj) != n:
            raise ValueError(f"{who}: {n} poses but an object index of {len(obj)}")
        if views is not None:
            if not isinstance(views, ops.Views):
                raise ValueError(f"{who}: views must be an ops.Views")
            if views.dev is not None and len(views) != n:
                raise ValueError(f"{who}: {n} poses but a view index of {len(views)}")
            if isinstance(obj, ops.PairRows):
                vh = np.zeros(n, dtype=np.int64) if views.host is None else views.host
                if obj.view is None or not np.array_equal(obj.view, vh):
                    raise ValueError(f"{who}: with views, the ObjectIndex must be built with view=views.host "
                                     "(the two-pose quirk is grouped per (view, object))")
        self.mesh, self.K, self.H, self.W, self.n, self.views = mesh, K, int(H), int(W), n, views
        # the one float-versus-table decision: a table is the entry points' diameter table, anything else is one object's float
        self.diameter = diameter if torch.is_tensor(diameter) else float(diameter)
        self.obj = obj.dev if isinstance(obj, ops.PairRows) else obj
        # the index that knows the quirk's groups, and where this scene's rows start in it
        self._pairs, self._row0 = obj if isinstance(obj, ops.PairRows) else (views if obj is None else None), 0
        self.grouped = obj is not None or views is not None       # the quirk per object, view or both; else of the call as a whole
        self.pair_list = [] if self._pairs is None else self._pairs.pairs     # the whole call's quirk pairs, host rows (parts_for_pairs)

    @property
    def pairs(self):
        """(P, 2) device rows of the quirk pairs inside this scene's rows, relative to its first; None when there are none"""
        return None if self._pairs is None else self._pairs.pair_rows(self._row0, self._row0 + self.n)

    def _cut(self, **changed):
        s = object.__new__(Scene)
        s.__dict__.update(self.__dict__, **changed)
        return s

    def rows(self, a, b):
        """the scene of hypotheses a..b: slices of the object index and of the view table, nothing is copied"""
        return self._cut(n=b - a, obj=None if self.obj is None else self.obj[a:b], _row0=self._row0 + a,
                         views=None if self.views is None else self.views.rows(a, b))

    def take(self, idx, idx_dev=None):
        """the scene of the hypotheses idx (host indices into this scene's rows; idx_dev: the same on the device, uploaded here if not
        given): gathers the object index on the device and uploads the gathered view index (ops.Views.take).  Carries no quirk pairs."""
        idx = np.asarray(idx, dtype=np.int64)
        obj = None if self.obj is None else self.obj.index_select(0, torch.as_tensor(idx, device=self.obj.device) if idx_dev is None else idx_dev)
        return self._cut(n=int(idx.size), obj=obj, views=None if self.views is None else self.views.take(idx), _pairs=None, _row0=0)

    def workspace_bytes(self, n, oh, ow):
        """the rasteriser scratch of n hypotheses at (oh, ow), for a mesh and for a set (whose V / T are its largest mesh's)"""
        return max(16, ops.workspace_bytes(n, self.mesh.V, self.mesh.T, oh, ow))

    def workspace(self, n, oh, ow, device):
        return torch.empty(self.workspace_bytes(n, oh, ow), dtype=torch.uint8, device=device)

    def crop_windows(self, poses, crop_ratio, out_size):
        return ops.crop_windows(poses, self.K, self.diameter, crop_ratio, out_size, obj=self.obj, views=self.views)

    def render_crops(self, poses, bbox2d, out_hw, **kw):
        return ops.render_crops(self.mesh, poses, bbox2d, self.K, self.H, self.W, out_hw=out_hw, mesh_diameter=self.diameter,
                                obj=self.obj, views=self.views, **kw)

    def warp_crops(self, rgb, xyz_map, depth, tf_to_crops, poses, mode, **kw):
        return ops.warp_crops(rgb, xyz_map, depth, tf_to_crops, self.K, poses, self.diameter, mode, obj=self.obj, views=self.views, **kw)

    def pose_update(self, trans, rot, poses, **kw):
        return ops.pose_update(trans, rot, poses, mesh_diameter=self.diameter, K=self.K, obj=self.obj, views=self.views, **kw)

    def depth_agreement(self, depth_crops, xyz_map, tf_to_crops, tol, out=None):
        return ops.depth_agreement(depth_crops, xyz_map, tf_to_crops, tol, views=self.views, out=out)

    def icp_point_plane(self, xyz_crops, normal_crops, xyz_map, tf_to_crops, poses, max_dist, **kw):
        return ops.icp_point_plane(xyz_crops, normal_crops, xyz_map, tf_to_crops, poses, max_dist, views=self.views, **kw)


def crop_stage(scene, poses, rgb, xyz_map, depth, mode, crop_ratio, out_hw, xyz_thr, normalize_xyz, AB, workspace=None, adjust_bbox=None,
               warp_rows=None, chunk=None, window_hw=None):
    """The network input of the n = scene.n hypotheses `poses` on the current stream: fp_crop_windows, fp_render_crops into AB[:n]
    and fp_warp_crops into AB[n:] (mode ops.MODE_REFINE reads rgb + xyz_map, ops.MODE_SCORE rgb + depth).  adjust_bbox: the two-pose
    quirk, bbox2d -> bbox2d, applied before the render.  warp_rows = (rows, dest): warp only those hypotheses, into `dest` (rows of
    AB) -- rows a range (a, b), cut without a copy, or host indices, gathered.  chunk: render and warp at most so many rows per launch.
    window_hw: the size the crop windows map to when it is not out_hw (render_size).  -> tf_to_crops (n,3,3), bbox2d (n,4)"""
    n, (wh, ww) = scene.n, out_hw if window_hw is None else window_hw
    tf_to_crops, bbox2d = scene.crop_windows(poses, crop_ratio, (ww, wh))
    if adjust_bbox is not None:
        bbox2d = adjust_bbox(bbox2d)
    for c, e in [(0, n)] if chunk is None else [(c, min(n, c + chunk)) for c in range(0, n, chunk)]:
        part = scene if (c, e) == (0, n) else scene.rows(c, e)
        part.render_crops(poses[c:e], bbox2d[c:e], out_hw, xyz_thr=xyz_thr, normalize_xyz=normalize_xyz, A_out=AB[c:e], workspace=workspace)
        if warp_rows is None:
            part.warp_crops(rgb, xyz_map, depth, tf_to_crops[c:e], poses[c:e], mode, normalize_xyz=normalize_xyz, out_hw=out_hw,
                            B_out=AB[n + c:n + e])
    if warp_rows is not None:
        rows, dest = warp_rows
        if isinstance(rows, tuple):
            part, tf, P = scene.rows(*rows), tf_to_crops[slice(*rows)], poses[slice(*rows)]
        else:
            idx = torch.as_tensor(rows, device=poses.device)
            part, tf, P = scene.take(rows, idx), tf_to_crops.index_select(0, idx), poses.index_select(0, idx)
        part.warp_crops(rgb, xyz_map, depth, tf, P, mode, normalize_xyz=normalize_xyz, out_hw=out_hw, B_out=dest)
    return tf_to_crops, bbox2d
