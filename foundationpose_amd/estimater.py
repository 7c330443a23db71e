"""FoundationPose estimator facade -- drop-in for /root/reference/estimater.py:18-268
(``register`` / ``track_one`` / ``reset_object`` / ``to_device``), orchestrating the HIP hot path.

Differences that are deliberate and documented in DESIGN.md:
  * depth filtering, back-projection and the translation guess (masked median) stay on the device (the reference
    round-trips numpy<->GPU four times); register() moves a handful of scalars over PCIe, never the depth map;
  * open3d voxel down-sampling of ``self.pts``/``self.normals`` (computed but unused by the hot path)
    is replaced by the raw model points;
  * no global ``torch.set_default_tensor_type`` side effect.
"""
import logging
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import dr, ops
from .crops import Scene
from .Utils import (bilateral_filter_depth, cluster_poses, compute_mesh_diameter, erode_depth, euler_matrix, get_mesh_handle,
                    make_mesh_tensors, mesh_handle_from_tensors, sample_views_icosphere, set_seed, stack_frames)
from .predict_pose_refine import PoseRefinePredictor
from .predict_score import ScorePredictor


class FoundationPose:
    def __init__(self, model_pts, model_normals, symmetry_tfs=None, mesh=None, scorer: ScorePredictor = None,
                 refiner: PoseRefinePredictor = None, glctx=None, debug=0, debug_dir="/tmp/foundationpose_amd_debug",
                 device="cuda", track_graph=False, mesh_tensors=None):
        """track_graph=True replays track_one as one captured hipGraph per frame (same arithmetic; off by default so
        that the call sequence of the reference is followed literally); mesh_tensors: as in reset_object"""
        self.gt_pose = None
        self.track_graph = bool(track_graph)
        self._tracker = None
        self._tracker_key = None
        self.ignore_normal_flip = True
        self.debug = debug
        self.debug_dir = debug_dir
        if debug >= 1:
            os.makedirs(debug_dir, exist_ok=True)
        self.device = torch.device(device)
        self.reset_object(model_pts, model_normals, symmetry_tfs=symmetry_tfs, mesh=mesh, mesh_tensors=mesh_tensors)
        self.make_rotation_grid(min_n_views=40, inplane_step=60)
        self.glctx = glctx
        self.scorer = scorer if scorer is not None else ScorePredictor(device=device)
        self.refiner = refiner if refiner is not None else PoseRefinePredictor(device=device)
        self.pose_last = None  # used for tracking; w.r.t. the centred mesh
        self.depth_agreement = None   # ops.DepthAgreement of the last tracking call made with an agreement_tol (None without)

    @classmethod
    def from_reference_views(cls, rgbs, depths, masks, ob_in_cams, Ks, voxel=None, reconstruct_args=None, **kwargs):
        """An estimator for an object without a CAD model: its mesh is fused from V posed RGB-D reference views with masks
        (reconstruct.reconstruct_object: rgbs (V,H,W,3), depths (V,H,W) metres, masks (V,H,W), ob_in_cams (V,4,4), Ks (V,3,3) or one
        (3,3); voxel=None: the longest side gets 128 voxels; reconstruct_args: its further keywords), then the constructor as for any
        other mesh (kwargs: scorer, refiner, symmetry_tfs, device, ...).  Poses come out in the frame of ob_in_cams; reset_object
        centres the mesh as usual (model_center).  With reconstruct_args={"refine_poses": R} the view poses are polished against the
        fused mesh first (with "refine_against": "volume" beside it, against the volume itself); the estimator keeps them as ref_ob_in_cams
        ((V,4,4) float32; None without).  reconstruct_args={"keep_components": "largest"} (or an int: the fewest triangles of a
        surface component that stays) drops floaters from the mesh at every extraction of the call."""
        from .reconstruct import reconstruct_object
        args = dict(reconstruct_args or {})
        args.setdefault("device", kwargs.get("device", "cuda"))
        mesh, tensors = reconstruct_object(rgbs, depths, masks, ob_in_cams, Ks, voxel=voxel, **args)
        est = cls(model_pts=mesh.vertices, model_normals=mesh.vertex_normals, mesh=mesh, mesh_tensors=tensors, **kwargs)
        est.ref_ob_in_cams = getattr(mesh, "ob_in_cams", None)
        # what view_coverage() reports on without arguments: the views the mesh was fused from (their polished poses where there are)
        est.ref_views = dict(ob_in_cams=est.ref_ob_in_cams if est.ref_ob_in_cams is not None else ob_in_cams, Ks=Ks,
                             hw=tuple(int(x) for x in np.shape(depths)[-2:]))
        return est

    # ------------------------------------------------------------------ estimater.py:44-78
    def reset_object(self, model_pts, model_normals, symmetry_tfs=None, mesh=None, mesh_tensors=None):
        """mesh_tensors: the device tensors of `mesh` as given (not centred), where the caller has them already (a reconstruction's):
        they are centred on the device in place of a second upload of the mesh, to the bits make_mesh_tensors gives"""
        self._tracker = None   # a captured tracking graph holds the previous object's mesh
        self.poses = self.scores = None   # ranked hypotheses of the last registration (pose_errors reads them): none for a new object
        max_xyz = np.asarray(mesh.vertices).max(axis=0)
        min_xyz = np.asarray(mesh.vertices).min(axis=0)
        self.model_center = (min_xyz + max_xyz) / 2
        self.mesh_ori = mesh.copy()
        mesh = mesh.copy()
        mesh.vertices = np.asarray(mesh.vertices) - self.model_center.reshape(1, 3)
        model_pts = np.asarray(mesh.vertices)
        self.diameter = compute_mesh_diameter(model_pts=model_pts, n_sample=10000)
        self.vox_size = max(self.diameter / 20.0, 0.003)
        logging.info(f"self.diameter:{self.diameter}, vox_size:{self.vox_size}")
        self.dist_bin = self.vox_size / 2
        self.angle_bin = 20
        self.max_xyz = model_pts.max(axis=0)
        self.min_xyz = model_pts.min(axis=0)
        self.pts = torch.tensor(model_pts, dtype=torch.float32, device=self.device)
        nrm = np.asarray(model_normals if model_normals is not None else mesh.vertex_normals)
        self.normals = F.normalize(torch.tensor(nrm, dtype=torch.float32, device=self.device), dim=-1)
        self.mesh_path = None
        self.mesh = mesh
        if mesh_tensors is None:
            self.mesh_tensors = make_mesh_tensors(self.mesh, device=self.device)
        else:
            t = {k: v.to(self.device) for k, v in mesh_tensors.items() if k not in ("_handle", "pseudonormals")}   # of the uncentred mesh
            center = torch.as_tensor(self.model_center, dtype=torch.float64, device=self.device)
            t["pos"] = (t["pos"].double() - center).float()        # the host's float64 subtraction, rounded once
            t["_handle"] = mesh_handle_from_tensors(t)
            self.mesh_tensors = t
        self.symmetries = None                            # the record of the last detect_symmetries (None: the table was given)
        if symmetry_tfs is None:
            self.symmetry_tfs = torch.eye(4, device=self.device).float()[None]
        elif isinstance(symmetry_tfs, str):
            if symmetry_tfs != "detect":
                raise ValueError(f"symmetry_tfs must be None, a (S,4,4) table or 'detect', got {symmetry_tfs!r}")
            self.detect_symmetries(rebuild_grid=False)    # the constructor builds the grid next; after reset_object it is the caller's
        else:
            self.symmetry_tfs = torch.as_tensor(symmetry_tfs, device=self.device, dtype=torch.float)
        logging.info("reset done")

    def detect_symmetries(self, rebuild_grid=True, **kw):
        """Find the mesh's rotational symmetries (reconstruct.detect_symmetries on the centred mesh; kw: its tol, max_order,
        rot_angle_discrete, samples, n_axes), set self.symmetry_tfs from them, in the frame of the mesh handed to reset_object like a
        table given by the caller, rebuild the rotation grid with them and return the record (symmetry.Symmetries, in the centred
        frame; also kept as self.symmetries).  tol=None: for a mesh fused at a known pitch (from_reference_views) two voxels, otherwise
        1 % of the mesh's extent.  Only geometry is considered: a can whose label is not symmetric is still reported as symmetric.
        accel="grid": the same record through a uniform grid, kept in self.mesh_tensors under "grid"; measured slower than the
        default on every mesh size (reconstruct.detect_symmetries says why)."""
        from .reconstruct import detect_symmetries
        if kw.get("tol") is None:
            voxel = getattr(self.mesh_ori, "voxel", None)
            kw["tol"] = 2.0 * float(voxel) if voxel else None
        mesh = dict(pos=self.mesh_tensors["pos"], faces=self.mesh_tensors["faces"])
        if kw.get("accel") == "grid":
            mesh["grid"] = ops.mesh_grid_build(self.mesh_tensors)     # kept with the estimator's tensors, found by detect_symmetries
        rec = detect_symmetries(mesh, **kw)
        to_c, from_c = np.eye(4), np.eye(4)               # T(-model_center), T(+model_center): as _centred_frames, inverted
        to_c[:3, 3] = -np.asarray(self.model_center, dtype=np.float64)
        from_c[:3, 3] = np.asarray(self.model_center, dtype=np.float64)
        self.symmetry_tfs = torch.as_tensor(from_c @ rec.tfs @ to_c, device=self.device, dtype=torch.float)
        self.symmetries = rec
        if rebuild_grid:
            self.make_rotation_grid(min_n_views=40, inplane_step=60)
        return rec

    def get_tf_to_centered_mesh(self):
        tf_to_center = torch.eye(4, dtype=torch.float, device=self.device)
        tf_to_center[:3, 3] = -torch.as_tensor(self.model_center, device=self.device, dtype=torch.float)
        return tf_to_center

    # ------------------------------------------------------------------ estimater.py:88-102
    def to_device(self, s="cuda:0"):
        self.device = torch.device(s)
        for k, v in list(self.__dict__.items()):
            if torch.is_tensor(v) or isinstance(v, nn.Module):
                self.__dict__[k] = v.to(s)
        for k in list(self.mesh_tensors):
            if torch.is_tensor(self.mesh_tensors[k]):
                self.mesh_tensors[k] = self.mesh_tensors[k].to(s)
        self.mesh_tensors.pop("_handle", None)  # rebuilt lazily against the moved tensors
        self.mesh_tensors.pop("pseudonormals", None)  # ops.mesh_pseudonormals' tables: made again on the new device when asked for
        if self.refiner is not None:
            self.refiner.model.to(s)
        if self.scorer is not None:
            self.scorer.model.to(s)
        if self.glctx is not None:
            self.glctx = dr.RasterizeCudaContext(s)

    # ------------------------------------------------------------------ estimater.py:106-124
    def make_rotation_grid(self, min_n_views=40, inplane_step=60):
        cam_in_obs = sample_views_icosphere(n_views=min_n_views)
        rot_grid = []
        for i in range(len(cam_in_obs)):
            for inplane_rot in np.deg2rad(np.arange(0, 360, inplane_step)):
                cam_in_ob = cam_in_obs[i] @ euler_matrix(0, 0, inplane_rot)
                rot_grid.append(np.linalg.inv(cam_in_ob))
        rot_grid = np.asarray(rot_grid)
        rot_grid = cluster_poses(30, 99999, rot_grid, self.symmetry_tfs.data.cpu().numpy())
        rot_grid = np.asarray(rot_grid)
        logging.info(f"after cluster, rot_grid:{rot_grid.shape}")
        self.rot_grid = torch.as_tensor(rot_grid, device=self.device, dtype=torch.float)

    def generate_random_pose_hypo(self, K, rgb, depth, mask, scene_pts=None):
        return self.grid_at(self.guess_translation(depth=depth, mask=mask, K=K))

    def grid_at(self, center):
        """the rotation grid with every hypothesis at the one translation `center` (generate_random_pose_hypo, estimater.py:127-134)"""
        ob_in_cams = self.rot_grid.clone()
        ob_in_cams[:, :3, 3] = torch.as_tensor(center, device=self.device, dtype=torch.float).reshape(1, 3)
        return ob_in_cams

    # ------------------------------------------------------------------ estimater.py:137-156
    def guess_translation(self, depth, mask, K):
        """Initial translation of every hypothesis (semantics of estimater.py:137-156): the ray through the centre of the
        mask's bounding box, at the median of the valid depths inside the mask; zeros when the mask or the valid set is
        empty.  Computed on the device: the depth map never leaves HBM (the reference does this in numpy).  The centre itself is
        translation_from_stats', from the six numbers found here."""
        d = torch.as_tensor(depth, device=self.device, dtype=torch.float)
        m = torch.as_tensor(np.asarray(mask) if not torch.is_tensor(mask) else mask, device=self.device) > 0
        rows, cols = torch.nonzero(m.any(dim=1)).reshape(-1), torch.nonzero(m.any(dim=0)).reshape(-1)
        if rows.numel() == 0:
            logging.info("mask is all zero")
            return np.zeros((3))
        z = d[m & (d >= 0.001)]
        if z.numel() == 0:
            logging.info("valid is empty")
            return np.zeros((3))
        zs = torch.sort(z).values
        n = zs.numel()
        stats = torch.stack([rows[0], rows[-1], cols[0], cols[-1]]).to(torch.float64)
        mid = torch.stack([zs[(n - 1) // 2], zs[n // 2]])          # numpy's median: mean of the two middle values
        box = stats.tolist()                                       # six scalars cross PCIe, not a 640x480 image
        lo, hi = mid.tolist()
        return translation_from_stats(K, box, n, lo, hi)

    # ------------------------------------------------------------------ estimater.py:159-240
    def register(self, K, rgb, depth, ob_mask, ob_id=None, glctx=None, iteration=5):
        set_seed(0)
        if self.glctx is None:
            self.glctx = glctx if glctx is not None else dr.RasterizeCudaContext(self.device)
        depth_t = torch.as_tensor(depth, device=self.device, dtype=torch.float).contiguous()
        depth_t = ops.erode_depth(depth_t, radius=2)
        depth_t = ops.bilateral_filter_depth(depth_t, radius=2)
        ob_mask = np.asarray(ob_mask.data.cpu().numpy() if torch.is_tensor(ob_mask) else ob_mask)
        mask_t = torch.as_tensor(ob_mask, device=self.device) > 0
        if int(((depth_t >= 0.001) & mask_t).sum()) < 4:
            return _guess_pose(self.guess_translation(depth=depth_t, mask=mask_t, K=K))
        poses = self.generate_random_pose_hypo(K=K, rgb=rgb, depth=depth_t, mask=mask_t, scene_pts=None)
        xyz_map = ops.depth_to_xyz(depth_t, K, zfar=float("inf"), f64_internal=True)  # depth2xyzmap (numpy variant)
        poses, vis = self.refiner.predict(mesh=self.mesh, mesh_tensors=self.mesh_tensors, rgb=rgb, depth=depth_t, K=K,
                                          ob_in_cams=poses, normal_map=None, xyz_map=xyz_map, glctx=self.glctx,
                                          mesh_diameter=self.diameter, iteration=iteration, get_vis=self.debug >= 2,
                                          shared_translation=True)   # generate_random_pose_hypo: one centre for the whole grid
        scores, vis = self.scorer.predict(mesh=self.mesh, rgb=rgb, depth=depth_t, K=K, ob_in_cams=poses,
                                          normal_map=None, mesh_tensors=self.mesh_tensors, glctx=self.glctx,
                                          mesh_diameter=self.diameter, get_vis=self.debug >= 2)
        return _set_registration(self, poses, scores, depth_t.shape, K, ob_id, ob_mask)

    def compute_add_err_to_gt_pose(self, poses):
        """stub in the reference as well (estimater.py:243-247); the errors to a known pose are pose_errors' (below)"""
        return -torch.ones(len(poses), device=self.device, dtype=torch.float)

    def pose_errors(self, gt_pose, poses=None, want=("add", "adds", "sym")):
        """ADD, ADD-S and the symmetry-aware errors (not in the reference) of `poses` against a known pose -> (N, 4) float64 device
        table [add, adds, add_sym, mssd] in metres over the mesh's vertices (ops.pose_errors; ops.PoseErrors.rows reads it on the host).
        gt_pose: (4,4), or (G,4,4) with G == N for pose n against ground truth n, in the frame of the mesh handed to reset_object --
        what register / track_one return and the readers' get_gt_pose gives.  poses: (N,4,4) in the centred-mesh frame like pose_last;
        None = self.poses, the ranked hypotheses of the last register (row 0 = the returned pose).  The ground truth and
        self.symmetry_tfs move into the centred frame in float64 on the host."""
        if poses is None:
            poses = getattr(self, "poses", None)
            if poses is None:
                raise RuntimeError("pose_errors: no registration yet (register first, or pass poses)")
        poses = torch.as_tensor(poses, device=self.device, dtype=torch.float).reshape(-1, 4, 4).contiguous()
        gt_c, sym_c = self._centred_frames(gt_pose)
        return ops.pose_errors(self.pts, poses, gt_c, symmetry_tfs=sym_c, want=want)

    def align_to_mesh(self, mesh, **kw):
        """Register the estimator's mesh (as it was handed to reset_object, for example fused by from_reference_views in the frame of
        the reference poses) onto `mesh` (a SimpleMesh or a mesh-tensor dict, for example the object's CAD model in its own frame)
        -> ops.MeshAlignment (reconstruct.align_meshes; kw: its starts, samples, iterations, max_dist, min_overlap, init, seed, and
        accel="grid" for the same alignment through a uniform grid over `mesh`: for a local refinement from a good init= against a
        model of tens of thousands of faces; slower than the default from the default starts).
        Its transfer_pose turns a pose of the estimator's mesh into the pose of `mesh`'s frame; compare_to_mesh(mesh, tf=it) compares
        in the aligned frame.  A setup call (it synchronises)."""
        from .reconstruct import align_meshes
        return align_meshes(self.mesh_ori, mesh, device=self.device, **kw)

    def compare_to_mesh(self, mesh, samples=100_000, thresholds=None, seed=0, unit=None, tf=None, accel=None):
        """How the estimator's mesh compares with `mesh` (a SimpleMesh or a mesh-tensor dict in the frame of the mesh handed to
        reset_object, for example the CAD model of an object whose estimator was made by from_reference_views) ->
        ops.MeshComparison (reconstruct.compare_meshes: accuracy = this estimator's mesh against `mesh`, completeness the other way,
        chamfer, Hausdorff, precision / recall / F-score per threshold).  The estimator's side is its mesh as it was handed over, not
        the centred one.  unit: the length the default thresholds are multiples of; None: the voxel pitch the mesh was fused at, for
        an estimator made by from_reference_views (otherwise pass unit or thresholds).  tf: a (4,4) transform or an
        ops.MeshAlignment (align_to_mesh) from the estimator's mesh into `mesh`'s frame, where the two are not in one frame already.
        accel="grid": the same report from far fewer pair tests (compare_meshes).  An evaluation call (it synchronises)."""
        from .reconstruct import compare_meshes
        if unit is None and thresholds is None:
            unit = getattr(self.mesh_ori, "voxel", None)
        return compare_meshes(self.mesh_ori, mesh, samples=samples, thresholds=thresholds, seed=seed, unit=unit, device=self.device, tf=tf,
                              accel=accel)

    def view_coverage(self, ob_in_cams=None, Ks=None, hw=None, **kw):
        """What of the estimator's mesh (as it was handed to reset_object, not the centred one) the views saw -> ops.ViewCoverage
        (reconstruct.view_coverage: the fraction of the surface seen by at least one view, by each view, the unseen area, and per
        surface sample the number of views that see it).  ob_in_cams (V,4,4), Ks and hw = (height, width) in that mesh's frame;
        with none of them, the reference views of an estimator made by from_reference_views: where the next reference view is
        needed.  kw: samples, seed, rel_tol, min_cos.  An evaluation call (it synchronises)."""
        from .reconstruct import view_coverage
        if ob_in_cams is None and Ks is None and hw is None:
            views = getattr(self, "ref_views", None)
            if views is None:
                raise RuntimeError("view_coverage: no reference views (the estimator was not made by from_reference_views): pass "
                                   "ob_in_cams, Ks and hw")
            ob_in_cams, Ks, hw = views["ob_in_cams"], views["Ks"], views["hw"]
        elif ob_in_cams is None or Ks is None or hw is None:
            raise ValueError("view_coverage: pass ob_in_cams, Ks and hw together (or none of them: the reference views)")
        pos, faces = (torch.as_tensor(np.ascontiguousarray(x, dtype=dt), device=self.device)
                      for x, dt in ((self.mesh_ori.vertices, np.float32), (self.mesh_ori.faces, np.int32)))
        return view_coverage(dict(pos=pos, faces=faces), ob_in_cams, Ks, hw, **kw)

    def penetration_into(self, other, poses=None, samples=2048, seed=0, allow_open=False, accel=None):
        """How far this object, at `poses`, reaches into the object of estimator `other` at other.pose_last (not in the reference)
        -> ops.Penetration with one row per pose: `inside` the share of this object's `samples` surface samples (sample_surface,
        seed) that lie inside other's mesh, `depth` the distance in metres of the deepest of them to other's surface (0 when none is
        inside), `deepest` that sample in the frame of the mesh handed to this estimator's reset_object (NaN when none).  poses: (4,4)
        or (N,4,4) in the centred-mesh frame like pose_last, for example the hypotheses of a registration; None: pose_last.  Both
        poses are of centred meshes and both mesh tensors are centred, so the samples move by inv(other.pose_last) @ pose (float64 on
        the host, rounded once) with no centring transform; the deepest sample alone is moved back by model_center.  One
        ops.mesh_penetration call (N x samples x other's faces pair tests).  other's mesh must be closed (ops.mesh_pseudonormals,
        computed once and kept in other.mesh_tensors) unless allow_open=True.  accel="grid": answered through a uniform grid over
        other's mesh (ops.mesh_grid_build, built at the first call and kept in other.mesh_tensors under "grid"): the same rows bit for
        bit.  It pays only where every sample is within about a cell of other's surface (twice its mean face edge) and other has
        tens of thousands of faces; samples a few cells away already cost more than the brute force, and a pose that puts this object
        far from other walks the whole grid and tests every stored triangle from global memory, minutes for milliseconds (DESIGN.md
        section 6).  None: brute force, the default.  An evaluation call (it synchronises)."""
        from .reconstruct import _accel_grid, sample_surface
        what = "penetration_into"
        if not isinstance(other, FoundationPose):
            raise ValueError(f"{what}: other must be a FoundationPose, got {type(other).__name__}")
        if other.pose_last is None:
            raise RuntimeError(f"{what}: the other estimator has no pose yet (register or track it first)")
        if poses is None:
            poses = self.pose_last
            if poses is None:
                raise RuntimeError(f"{what}: no pose yet (register or track first, or pass poses)")
        host = lambda p: (p.detach().cpu().numpy() if torch.is_tensor(p) else np.asarray(p)).astype(np.float64).reshape(-1, 4, 4)   # noqa: E731
        tfs = np.linalg.inv(host(other.pose_last)[0]) @ host(poses)
        grid = _accel_grid(accel, other.mesh_tensors, what)
        dev = other.mesh_tensors["pos"].device
        pts, _ = sample_surface(dict(pos=self.mesh_tensors["pos"], faces=self.mesh_tensors["faces"]), samples, seed)
        got = ops.mesh_penetration(pts.to(dev), torch.as_tensor(tfs.astype(np.float32), device=dev).contiguous(), other.mesh_tensors,
                                   allow_open=allow_open, grid=grid)
        return ops.Penetration.rows(got, pts, self.model_center)

    # the depth maps bop_errors holds at a time: 48 MiB = 40 full 480 x 640 float32 frames.  Small against the 256 MiB last-level cache,
    # so a chunk's renders are still on the chip when the counting kernel reads them, and large enough that the raster launches of a
    # chunk are amortised over tens of poses (all 252 at once would be 310 MB that the rasteriser writes to HBM and the counter reads back)
    BOP_DEPTH_BUDGET = 48 << 20

    def _centred_frames(self, gt_pose):
        """ground truth(s) and self.symmetry_tfs in the centred-mesh frame, float64 on the host -> ((G,4,4), (S,4,4))"""
        to_c, from_c = np.eye(4), np.eye(4)               # T(-model_center), T(+model_center)
        to_c[:3, 3] = -np.asarray(self.model_center, dtype=np.float64)
        from_c[:3, 3] = np.asarray(self.model_center, dtype=np.float64)
        gt = gt_pose.detach().cpu().numpy() if torch.is_tensor(gt_pose) else np.asarray(gt_pose)
        gt_c = gt.astype(np.float64).reshape(-1, 4, 4) @ from_c
        sym_c = to_c @ self.symmetry_tfs.detach().cpu().numpy().astype(np.float64).reshape(-1, 4, 4) @ from_c
        return gt_c, sym_c

    def bop_errors(self, gt_pose, depth, K, poses=None, taus=ops.BOP_TAUS, delta=0.015, chunk=None):
        """The three pose errors BOP ranks by (not in the reference) of `poses` against a known pose -> dict of device tensors:
        `vsd` (N,T) float64 (visible surface discrepancy per tolerance tau), `mssd` (N,) float64 metres, `mspd` (N,) float64 pixels and
        `counts`, the (N, 4+T) int32 table VSD is made of (ops.vsd_counts; ops.VsdCounts.rows reads it).  gt_pose and poses as in
        pose_errors ((4,4) or one per pose; poses None = the ranked hypotheses of the last register), moved into the centred-mesh frame
        in float64 on the host.  depth: the RAW sensor depth (H,W) in metres, 0 = no measurement -- not the eroded / filtered map register
        makes of it; K: the camera's intrinsics.  VSD renders the object full-frame at every pose and at the ground truth (rounded to
        float32 once for the rasteriser; MSSD and MSPD keep the float64 one) with the estimator's own mesh, `chunk` poses at a time
        (None: as many as BOP_DEPTH_BUDGET holds -- 48 MiB, 40 frames of 480 x 640, instead of 310 MB for 252 poses at once: a chunk's
        maps are still in the 256 MiB last-level cache when they are counted, and on an MI355X the chunks cost 0.9 ms of raster
        launches more than one render of all 252); the result does not depend on the chunk.  mssd and mspd run over the mesh's vertices
        with self.symmetry_tfs.  Out of scope: several cameras (ops.Views) or objects (MeshSet) per call, rendering only a window
        around the two projections (vsd_counts' origin is there for it), BOP's result files and its matching of estimates to ground
        truths."""
        if poses is None:
            poses = getattr(self, "poses", None)
            if poses is None:
                raise RuntimeError("bop_errors: no registration yet (register first, or pass poses)")
        poses = torch.as_tensor(poses, device=self.device, dtype=torch.float).reshape(-1, 4, 4).contiguous()
        obs = torch.as_tensor(depth, device=self.device, dtype=torch.float).contiguous()
        if obs.dim() != 2:
            raise ValueError(f"bop_errors: depth must be (H,W), got {tuple(obs.shape)}")
        H, W = int(obs.shape[0]), int(obs.shape[1])
        N = int(poses.shape[0])
        gt_c, sym_c = self._centred_frames(gt_pose)
        G = len(gt_c)
        if G not in (1, N):
            raise ValueError(f"bop_errors: {G} ground truths for {N} poses (one, or one per pose)")
        T = int(np.asarray(taus).size)
        if chunk is None:
            chunk = self.BOP_DEPTH_BUDGET // (H * W * 4)
        chunk = max(1, min(int(chunk), 65535))
        handle = get_mesh_handle(self.mesh_tensors)
        gt32 = torch.as_tensor(gt_c.astype(np.float32), device=self.device)

        def render(p):
            return ops.render_crops(handle, p.contiguous(), None, K, H, W, (H, W), mesh_diameter=self.diameter, normalize_xyz=False,
                                    want=("depth",))["depth"]

        counts = torch.empty((N, 4 + T), dtype=torch.int32, device=self.device)
        gt_map = render(gt32) if G == 1 else None
        for a in range(0, N, chunk):
            b = min(a + chunk, N)
            ops.vsd_counts(render(poses[a:b]), gt_map if G == 1 else render(gt32[a:b]), obs, K, self.diameter, taus=taus, delta=delta,
                           out=counts[a:b])
        c = counts.to(torch.float64)
        union = c[:, 3:4]
        vsd = torch.where(union > 0, (c[:, 4:] + union - c[:, 2:3]) / union.clamp(min=1.0), torch.ones_like(c[:, 4:]))
        mssd = ops.pose_errors(self.pts, poses, gt_c, symmetry_tfs=sym_c, want=("sym",))[:, 3].contiguous()
        mspd = ops.mspd(self.pts, poses, gt_c, K, symmetry_tfs=sym_c)
        return dict(vsd=vsd, mssd=mssd, mspd=mspd, counts=counts)

    def hypothesis_report(self, gt_pose, metric="adds", depth=None, K=None):
        """Was a good hypothesis among the ranked ones of the last register, and where did the scorer put it?  -> dict: the error
        (`metric`: "add", "adds", "add_sym" or "mssd", metres; with the frame's raw `depth` and `K` also "vsd", the mean over BOP's
        taus, and "mspd", pixels -- bop_errors) and score of the returned pose (rank 0), the lowest error among the hypotheses, its
        rank and its score, and the number of hypotheses."""
        bop = ("vsd", "mspd")
        col = ops.PoseErrors._fields.index(metric) if metric in ops.PoseErrors._fields else None
        if col is None and metric not in bop:
            raise ValueError(f"hypothesis_report: unknown metric {metric!r} (known: {ops.PoseErrors._fields + bop})")
        if col is None:
            if K is None or (metric == "vsd" and depth is None):
                raise ValueError(f"hypothesis_report: metric {metric!r} needs the frame's {'depth and ' if metric == 'vsd' else ''}K")
            if getattr(self, "poses", None) is None:
                raise RuntimeError("hypothesis_report: no registration yet (register first)")
            if metric == "mspd":
                gt_c, sym_c = self._centred_frames(gt_pose)
                poses = torch.as_tensor(self.poses, device=self.device, dtype=torch.float).reshape(-1, 4, 4).contiguous()
                err = ops.mspd(self.pts, poses, gt_c, K, symmetry_tfs=sym_c).cpu().numpy()
            else:
                err = self.bop_errors(gt_pose, depth, K)["vsd"].mean(dim=1).cpu().numpy()
        else:
            table = self.pose_errors(gt_pose, want=("sym",) if col >= 2 else (metric,))
            err = table[:, col].cpu().numpy()
        scores = torch.as_tensor(self.scores).detach().cpu().numpy().astype(np.float64)
        best = int(np.argmin(err))
        return dict(metric=metric, n=int(len(err)), top_err=float(err[0]), top_score=float(scores[0]), best_err=float(err[best]),
                    best_rank=best, best_score=float(scores[best]))

    # ------------------------------------------------------------------ estimater.py:250-268
    def track_one(self, rgb, depth, K, iteration, extra={}, agreement_tol=None):
        """agreement_tol (metres; not in the reference's signature): also check the tracked pose against the observed depth
        (PoseRefinePredictor.depth_check on the xyz map the refine loop read) into self.depth_agreement and extra["depth_agreement"]
        (an ops.DepthAgreement); None: no check, self.depth_agreement = None.  The pose is the same either way."""
        tol = None if agreement_tol is None else ops._check_tol(agreement_tol, "track_one")
        if self.pose_last is None:
            logging.info("Please init pose by register first")
            raise RuntimeError
        self.depth_agreement = None
        if self.track_graph:
            # same arithmetic, one hipGraph launch per frame (foundationpose_amd/graphs.py); re-captured when the
            # frame size, intrinsics, iteration count or agreement tolerance change
            key = (tuple(np.asarray(depth).shape[:2]), np.asarray(K, dtype=np.float64).tobytes(), int(iteration), tol)
            if self._tracker is None or self._tracker_key != key:
                from .graphs import GraphedTracker
                H, W = key[0]
                self._tracker = GraphedTracker(self.refiner, self.mesh_tensors, self.diameter, K, H, W, n_hyp=1,
                                               iteration=iteration, device=self.device, agreement_tol=tol).capture()
                self._tracker_key = key
            pose = self._tracker.step(rgb, depth, self.pose_last.reshape(1, 4, 4)).clone()
            self.pose_last = pose
            if tol is not None:
                self.depth_agreement = extra["depth_agreement"] = ops.DepthAgreement.rows(self._tracker.agreement)[0]
            return (pose @ self.get_tf_to_centered_mesh()).data.cpu().numpy().reshape(4, 4)
        depth_t = torch.as_tensor(depth, device=self.device, dtype=torch.float).contiguous()
        xyz_map = ops.ingest_frame(depth_t, K)
        # depth=None: the refiner reads the xyz map alone (`depth` is the reference's signature), and the filtered depth stays inside
        # the ingest -- a predict() that began to read it would fail here, not see an unfiltered map
        pose, vis = self.refiner.predict(mesh=self.mesh, mesh_tensors=self.mesh_tensors, rgb=rgb, depth=None, K=K,
                                         ob_in_cams=self.pose_last.reshape(1, 4, 4), normal_map=None, xyz_map=xyz_map,
                                         mesh_diameter=self.diameter, glctx=self.glctx, iteration=iteration,
                                         get_vis=self.debug >= 2)
        if self.debug >= 2:
            extra["vis"] = vis
        self.pose_last = pose
        if tol is not None:
            with torch.inference_mode():
                H, W = int(depth_t.shape[0]), int(depth_t.shape[1])
                P = pose.reshape(-1, 4, 4).contiguous()
                table = self.refiner.depth_check(P, xyz_map, Scene(get_mesh_handle(self.mesh_tensors), self.diameter, K, H, W, P.shape[0]), tol)
            self.depth_agreement = extra["depth_agreement"] = ops.DepthAgreement.rows(table)[0]
        return (pose @ self.get_tf_to_centered_mesh()).data.cpu().numpy().reshape(4, 4)

    def polish(self, depth, K, iterations=3, max_dist=0.02, extra=None):
        """Polish pose_last against the observed depth by point-to-plane ICP (depth_polish of this one estimator; not in the
        reference): -> the pose as track_one returns it; with a dict `extra`, extra["icp"] = the last iteration's ops.IcpStep."""
        step = depth_polish([self], depth, K, iterations=iterations, max_dist=max_dist)[0]
        if extra is not None:
            extra["icp"] = step
        return (self.pose_last.reshape(4, 4) @ self.get_tf_to_centered_mesh()).data.cpu().numpy().reshape(4, 4)

    track = track_one  # the north-star calls it track(); the reference method is track_one


# ---------------------------------------------------------------------- the batched calls: several estimators per call
# track_objects / track_views / depth_agreement / register_objects / register_views share the argument rules, the cache on the shared
# refiner and the per-estimator epilogues below; what differs between them is which kernels they launch.

def _check_estimators(name, estimators, scorer=False, registered=False):
    """The rules every batched call puts on its estimator list, in one order: not empty, ONE refiner object, (scorer=True:) ONE scorer
    object, every estimator once, (registered=True:) everybody has a pose_last.  Reads `scorer` / `pose_last` only where the flag asks
    for the rule, and nothing else.  Every caller runs this first and its view, frame and mask rules (_check_views, _check_masks)
    after it: who is asked before what about, so a call that breaks a rule of each kind is told about its estimators (register_views
    used to name the view or mask first; within each kind the order is the one it had).
    -> (list of estimators, the refiner, the scorer or None)"""
    ests = list(estimators)
    if not ests:
        raise ValueError(f"{name}: no estimators")
    refiner, shared = ests[0].refiner, None
    if any(e.refiner is not refiner for e in ests):
        raise ValueError(f"{name}: the estimators must share one refiner object (FoundationPose(..., refiner=shared))")
    if scorer:
        shared = ests[0].scorer
        if any(e.scorer is not shared for e in ests):
            raise ValueError(f"{name}: the estimators must share one scorer object (FoundationPose(..., scorer=shared))")
    if len({id(e) for e in ests}) != len(ests):
        raise ValueError(f"{name}: an estimator is listed twice")
    if registered:
        for i, e in enumerate(ests):
            if e.pose_last is None:
                raise RuntimeError(f"{name}: estimator {i} is not registered (call register first)")
    return ests, refiner, shared


def _frame_hw(f):
    return tuple(f.shape[:2]) if torch.is_tensor(f) else tuple(np.asarray(f).shape[:2])


def _check_views(name, n, views, depths, Ks, rgbs=None):
    """The rules of a call over several camera frames: one view index per estimator (n of them), one depth frame and one K (and with
    rgbs one rgb frame) per view, every index inside 0..V-1, all frames of one size.  -> (views, rgbs, depths, Ks) as lists, (H, W)"""
    views = [int(v) for v in views]
    if len(views) != n:
        raise ValueError(f"{name}: {n} estimators but {len(views)} view indices")
    rgbs, depths, Ks = None if rgbs is None else list(rgbs), list(depths), list(Ks)
    V = len(depths)
    if V < 1 or len(Ks) != V or (rgbs is not None and len(rgbs) != V):
        have = ("" if rgbs is None else f"{len(rgbs)} rgb frames, ") + f"{V} depth frames and {len(Ks)} intrinsics"
        raise ValueError(f"{name}: {have}: need one of each per view")
    for i, v in enumerate(views):
        if not 0 <= v < V:
            raise ValueError(f"{name}: estimator {i} views frame {v}, outside 0..{V - 1}")
    hws = {_frame_hw(f) for f in (rgbs or []) + depths}
    if len(hws) != 1:
        raise ValueError(f"{name}: the frames differ in size {sorted(hws)}; all views must have one H x W")
    return views, rgbs, depths, Ks, hws.pop()


def _check_masks(name, n, ob_masks, ob_ids):
    """one mask and (unless ob_ids is None) one object id per estimator -> (masks, ob_ids) as lists"""
    masks = list(ob_masks)
    if len(masks) != n:
        raise ValueError(f"{name}: {n} estimators but {len(masks)} masks")
    ob_ids = [None] * n if ob_ids is None else list(ob_ids)
    if len(ob_ids) != n:
        raise ValueError(f"{name}: {n} estimators but {len(ob_ids)} object ids")
    return masks, ob_ids


def _objects_key(ests):
    return tuple((id(e), id(e.mesh_tensors)) for e in ests)


def _cached(refiner, attr, key, ests, build):
    """`build()`'s object, cached on the shared refiner as `attr` = (key, object, estimators, mesh dicts) until the key changes.  The
    keys hold _objects_key's ids; the entry keeps the estimators and their mesh dicts alive, so those ids cannot be reused while it
    is cached."""
    cached = getattr(refiner, attr, None)
    if cached is None or cached[0] != key:
        cached = (key, build(), ests, [e.mesh_tensors for e in ests])
        setattr(refiner, attr, cached)
    return cached[1]


def _object_tables(refiner, ests):
    """the MeshSet and diameter table of `ests`' objects, cached on the shared refiner under the estimators and their mesh tensors"""
    def build():
        return ops.MeshSet([get_mesh_handle(e.mesh_tensors) for e in ests]), ops.object_diameters([e.diameter for e in ests], ests[0].device)
    return _cached(refiner, "_objects_tables", _objects_key(ests), ests, build)


def _set_agreement(ests, trk):
    """each estimator's depth_agreement from a tracker's table (one copy; one hypothesis per estimator), or None without a check"""
    rows = [None] * len(ests) if trk.agreement is None else ops.DepthAgreement.rows(trk.agreement)
    for e, r in zip(ests, rows):
        e.depth_agreement = r


def _track(name, estimators, views, rgb, depth, K, iteration, agreement_tol):
    """track_objects (views=None: one frame rgb / depth with one K) and track_views (the frames and Ks as lists): the captured
    tracker over the estimators' meshes, cached on their refiner, stepped from every pose_last"""
    tol = None if agreement_tol is None else ops._check_tol(agreement_tol, name)
    ests, refiner, _ = _check_estimators(name, estimators, registered=True)
    if views is None:
        hw = _frame_hw(depth)
        key = (_objects_key(ests), hw, np.asarray(K, dtype=np.float64).tobytes(), int(iteration), tol)
    else:
        views, rgb, depth, K, hw = _check_views(name, len(ests), views, depth, K, rgbs=rgb)
        Kb = b"".join(np.asarray(k, dtype=np.float64).reshape(9).tobytes() for k in K)
        key = (_objects_key(ests), tuple(views), hw, Kb, int(iteration), tol)
    dev = ests[0].device

    def capture():
        from .graphs import GraphedTracker
        return GraphedTracker(refiner, [e.mesh_tensors for e in ests], [e.diameter for e in ests], K, hw[0], hw[1], n_hyp=1,
                              iteration=iteration, device=dev, views=views, agreement_tol=tol).capture()
    trk = _cached(refiner, "_objects_tracker" if views is None else "_views_tracker", key, ests, capture)
    start = torch.stack([e.pose_last.reshape(4, 4).to(dev, torch.float32) for e in ests])
    out = trk.step(rgb, depth, start).clone()
    _set_agreement(ests, trk)
    poses = []
    for k, e in enumerate(ests):
        e.pose_last = out[k:k + 1]
        poses.append((out[k] @ e.get_tf_to_centered_mesh()).data.cpu().numpy().reshape(4, 4))
    return poses


def track_objects(estimators, rgb, depth, K, iteration=2, agreement_tol=None):
    """track_one for several objects in one frame: ONE batched refine loop over the objects' hypotheses (one each, from every
    estimator's pose_last), replayed as captured hipGraphs (graphs.GraphedTracker over the objects' meshes) on one shared depth
    ingest, instead of len(estimators) separate calls.  Per object the result is what its own track_one computes (the hypotheses of
    a call never mix; each one draws its own mesh and uses its own diameter).  Every estimator must be registered, listed once, and
    all must share ONE refiner object (its network and configuration are the loop's).  The captured tracker is cached on that refiner
    under (estimators, frame size, K, iteration, agreement_tol), like track_one's.  -> [4x4 np.ndarray] per estimator, in its original
    mesh frame; updates each pose_last.  register_objects is the batched register().  agreement_tol (metres): also check every tracked
    pose against the observed depth (GraphedTracker agreement_tol) and set each estimator's depth_agreement (an ops.DepthAgreement;
    None without)."""
    return _track("track_objects", estimators, None, rgb, depth, K, iteration, agreement_tol)


def track_views(estimators, views, rgbs, depths, Ks, iteration=2, agreement_tol=None):
    """track_one for objects in several camera frames at once: estimator k is tracked on frame views[k] (rgbs[v], depths[v] with
    intrinsics Ks[v]), all in ONE batched refine loop over one hypothesis per estimator, replayed as captured hipGraphs
    (graphs.GraphedTracker with views) on one batched depth ingest of all frames.  Per estimator the result is what its own track_one
    on its frame computes; two estimators may share a mesh (one object seen by two cameras, each pose in its own camera's frame).
    Every estimator must be registered, listed once, and all must share ONE refiner object; the frames must have one size.  The
    captured tracker is cached on that refiner, like track_objects' (the two calls share their body, _track).  -> [4x4 np.ndarray] per
    estimator, in its original mesh frame; updates each pose_last.  agreement_tol (metres): also check every tracked pose against its
    frame's observed depth and set each estimator's depth_agreement, as track_objects does."""
    return _track("track_views", estimators, views, rgbs, depths, Ks, iteration, agreement_tol)


def depth_agreement(estimators, depths, Ks, views=None, tol=0.01):
    """How well each estimator's current pose_last agrees with the observed depth: estimator k's pose on frame views[k] of depths
    (intrinsics Ks[views[k]]), or with views=None on the one frame `depths` with the one K `Ks` -- the check the trackers run with
    agreement_tol, on a registration or re-registration (register / register_objects / register_views) without changing them.  The
    depth goes through the tracking ingest (erode, bilateral, back-projection in f32: ops.ingest_frame, or ops.ingest_frames for
    several views); the crop windows and crop size are those of the estimators' ONE shared refiner.  The argument rules are the
    trackers'.  tol: absolute, in metres.  -> [ops.DepthAgreement] per estimator (one device-to-host copy)."""
    t = ops._check_tol(tol, "depth_agreement")
    ests, refiner, _ = _check_estimators("depth_agreement", estimators, registered=True)
    if views is not None:
        views, _, depths, Ks, (H, W) = _check_views("depth_agreement", len(ests), views, depths, Ks)
    dev = ests[0].device
    with torch.inference_mode():
        if views is None:
            d = torch.as_tensor(depths, device=dev, dtype=torch.float).contiguous()
            xyz = ops.ingest_frame(d, Ks)
            H, W = int(d.shape[0]), int(d.shape[1])
            K, vt = Ks, None
        else:
            stack = stack_frames(depths, dev, torch.float)
            K, vt = None, ops.Views(Ks, views, dev)
            xyz = ops.ingest_frames(stack, vt, f64_internal=False)
        mset, diam = _object_tables(refiner, ests)
        obj = torch.arange(len(ests), dtype=torch.int32, device=dev)
        P = torch.stack([e.pose_last.reshape(4, 4).to(dev, torch.float32) for e in ests]).contiguous()
        table = refiner.depth_check(P, xyz, Scene(mset, diam, K, H, W, len(ests), obj=obj, views=vt, who="depth_agreement"), t)
    return ops.DepthAgreement.rows(table)


def depth_polish(estimators, depths, Ks, views=None, iterations=3, max_dist=0.02):
    """Polish each estimator's current pose_last against the observed depth by `iterations` steps of point-to-plane ICP
    (PoseRefinePredictor.depth_polish; include/fp_amd.h fp_icp_point_plane): estimator k's pose on frame views[k] of depths (intrinsics
    Ks[views[k]]), or with views=None on the one frame `depths` with the one K `Ks`.  The argument rules, the depth ingest and the crop
    windows are those of depth_agreement.  Sets each estimator's pose_last (a pose whose step could not be solved stays as it was) and
    -> [ops.IcpStep] of the last iteration per estimator (one device-to-host copy).  The trackers and their graphs are not touched."""
    ops._check_icp(max_dist, 1e-3, 64, "depth_polish")
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or int(iterations) < 1:
        raise ValueError(f"depth_polish: iterations must be an int >= 1, got {iterations!r}")
    ests, refiner, _ = _check_estimators("depth_polish", estimators, registered=True)
    if views is not None:
        views, _, depths, Ks, (H, W) = _check_views("depth_polish", len(ests), views, depths, Ks)
    dev = ests[0].device
    with torch.inference_mode():
        if views is None:
            d = torch.as_tensor(depths, device=dev, dtype=torch.float).contiguous()
            xyz = ops.ingest_frame(d, Ks)
            H, W = int(d.shape[0]), int(d.shape[1])
            K, vt = Ks, None
        else:
            stack = stack_frames(depths, dev, torch.float)
            K, vt = None, ops.Views(Ks, views, dev)
            xyz = ops.ingest_frames(stack, vt, f64_internal=False)
        mset, diam = _object_tables(refiner, ests)
        obj = torch.arange(len(ests), dtype=torch.int32, device=dev)
        P = torch.stack([e.pose_last.reshape(4, 4).to(dev, torch.float32) for e in ests]).contiguous()
        out, system = refiner.depth_polish(P, xyz, Scene(mset, diam, K, H, W, len(ests), obj=obj, views=vt, who="depth_polish"),
                                           iterations=int(iterations), max_dist=max_dist)
        out = out.clone()
    for k, e in enumerate(ests):
        e.pose_last = out[k:k + 1]
    return ops.IcpStep.rows(system)


def penetrations(estimators, samples=2048, seed=0, allow_open=False, accel=None):
    """penetration_into over every ordered pair of the estimators at their current pose_last -> {(i, j): ops.Penetration}: how far
    object i reaches into object j.  Two objects tracked or registered into each other show up as a non-zero share in one direction
    at least.  The estimators need not share a refiner; everybody needs a pose_last.  One ops.mesh_penetration call per pair; accel as
    penetration_into takes it (one grid per estimator, kept in its mesh_tensors)."""
    ests = list(estimators)
    for i, e in enumerate(ests):
        if e.pose_last is None:
            raise RuntimeError(f"penetrations: estimator {i} has no pose yet (register or track it first)")
    return {(i, j): a.penetration_into(b, samples=samples, seed=seed, allow_open=allow_open, accel=accel)
            for i, a in enumerate(ests) for j, b in enumerate(ests) if i != j}


def translation_from_stats(K, box, n, lo, hi):
    """guess_translation's centre (estimater.py:137-156) from the numbers fp_mask_depth_stats returns for one mask (the box
    [v0, v1, u0, u1], the valid count n, the two middle valid depths lo / hi as float32) -- and from the same numbers as
    guess_translation finds them with torch: this is the one place the centre is computed.  Zeros for an empty mask or an empty valid
    set, as there."""
    if int(box[1]) < 0 or int(n) == 0:
        return np.zeros((3))
    v0, v1, u0, u1 = (float(x) for x in box)
    lo, hi = float(lo), float(hi)
    zc = float(np.float32(np.float32(lo) + np.float32(hi)) / np.float32(2.0)) if lo != hi else lo
    center = (np.linalg.inv(K) @ np.asarray([(u0 + u1) / 2.0, (v0 + v1) / 2.0, 1]).reshape(3, 1)) * zc   # estimater.py:149
    return center.reshape(3)


def _guess_pose(center, who=""):
    """register()'s answer for a mask with fewer than 4 valid depths (estimater.py:174-178): no rotation, the guessed translation;
    the estimator keeps its state"""
    logging.info(f"{who}valid too small, return")
    pose = np.eye(4)
    pose[:3, 3] = center
    return pose


def _set_registration(e, poses, scores, hw, K, ob_id, ob_mask):
    """The end of a registration of estimator `e` (estimater.py:224-240): its refined hypotheses ranked by score, and the state
    register() leaves (H, W, K, ob_id, ob_mask, scores, poses, pose_last, best_id), all set here: a registration whose refine or
    scoring raises leaves the estimator as it was, the frame's K and mask included.  -> the best pose, 4x4 np.ndarray in the original
    mesh frame"""
    ids = torch.as_tensor(scores).argsort(descending=True)
    e.H, e.W = int(hw[0]), int(hw[1])
    e.K = K
    e.ob_id = ob_id
    e.ob_mask = ob_mask
    e.scores = scores[ids]
    e.poses = poses[ids]
    e.pose_last = e.poses[0]
    e.best_id = ids[0]
    return (e.poses[0] @ e.get_tf_to_centered_mesh()).data.cpu().numpy()


def register_objects(estimators, K, rgb, depth, ob_masks, ob_ids=None, iteration=5):
    """register() for several objects in one frame: ONE depth ingest, ONE batched refine loop over all objects' hypotheses
    (refine_device with a MeshSet and an ObjectIndex) and ONE scorer call (ScorePredictor.predict_objects, whose cross-hypothesis
    attention stays inside each object) instead of len(estimators) register() calls.  ob_masks[k] is estimator k's object mask,
    ob_ids[k] its id.  Per object the result, and the state set on the estimator (H, W, K, ob_id, ob_mask, pose_last, best_id,
    poses, scores), is what its own register() computes; an object whose mask holds fewer than 4 valid depths gets register()'s
    guess-translation pose and keeps its state, as there.  Every estimator is listed once and all must share ONE refiner and ONE
    scorer object.  -> [4x4 np.ndarray] per estimator, in its original mesh frame."""
    ests, refiner, scorer = _check_estimators("register_objects", estimators, scorer=True)
    masks, ob_ids = _check_masks("register_objects", len(ests), ob_masks, ob_ids)
    set_seed(0)
    dev = ests[0].device
    for e in ests:
        if e.glctx is None:
            e.glctx = dr.RasterizeCudaContext(e.device)
    # register()'s depth ingest, once for all objects
    depth_t = torch.as_tensor(depth, device=dev, dtype=torch.float).contiguous()
    depth_t = ops.erode_depth(depth_t, radius=2)
    depth_t = ops.bilateral_filter_depth(depth_t, radius=2)
    out, hyps, lengths, masks_np = [None] * len(ests), [], [], []
    for k, (e, m) in enumerate(zip(ests, masks)):
        m = np.asarray(m.data.cpu().numpy() if torch.is_tensor(m) else m)
        masks_np.append(m)
        mask_t = torch.as_tensor(m, device=dev) > 0
        if int(((depth_t >= 0.001) & mask_t).sum()) < 4:
            out[k] = _guess_pose(e.guess_translation(depth=depth_t, mask=mask_t, K=K), f"object {k}: ")
            lengths.append(0)
            continue
        P = e.generate_random_pose_hypo(K=K, rgb=rgb, depth=depth_t, mask=mask_t, scene_pts=None)
        hyps.append(P)
        lengths.append(int(P.shape[0]))
    if not hyps:
        return out
    from .predict_pose_refine import ObjectIndex
    seg = ops.Segments(lengths, dev)
    mset, diam = _object_tables(refiner, ests)
    with torch.inference_mode():
        xyz_t = ops.depth_to_xyz(depth_t, K, zfar=float("inf"), f64_internal=True).contiguous()   # depth2xyzmap (numpy variant)
        rgb_t = torch.as_tensor(rgb, device=dev).to(torch.float).contiguous()
        H, W = int(rgb_t.shape[0]), int(rgb_t.shape[1])
        poses, trans, rot = refiner.refine_device(rgb_t, xyz_t, torch.cat(hyps).contiguous(), K, H, W, mset, diam, iteration,
                                                  shared_translation=False, obj=ObjectIndex(np.repeat(np.arange(len(ests)), lengths), dev))
        refiner.last_trans_update, refiner.last_rot_update = trans, rot
        scores = scorer.predict_objects(rgb, depth_t, K, poses, mset, diam, seg)
    for k, e in enumerate(ests):
        a, b = seg.rows(k)
        if b > a:
            out[k] = _set_registration(e, poses[a:b], scores[a:b], depth_t.shape, K, ob_ids[k], masks_np[k])
    return out


def register_views(estimators, views, rgbs, depths, Ks, ob_masks, ob_ids=None, iteration=5):
    """register() for objects in several camera frames at once: estimator k is registered on frame views[k] (rgbs[v], depths[v] with
    intrinsics Ks[v]) with mask ob_masks[k], in ONE batched depth ingest of all frames, ONE fp_mask_depth_stats launch (every mask's
    translation guess and valid-depth count, one copy back), ONE refine_device call over all hypotheses (views, an ObjectIndex, and
    one shared translation per estimator: its first iteration warps one observed crop per estimator) and ONE scorer call
    (predict_objects with views).  Per estimator the result, and the state set on it (H, W, K = Ks[views[k]], ob_id, ob_mask,
    pose_last, best_id, poses, scores), is what its own register() on its frame computes; an estimator whose mask holds fewer than 4
    valid depths gets register()'s guess-translation pose and keeps its state.  The argument rules are track_views': every estimator
    listed once, all sharing ONE refiner and ONE scorer, the frames of one size (and every mask of that size); two estimators may
    share a mesh (one object seen by two cameras).  -> [4x4 np.ndarray] per estimator, each in its own camera's frame and the original
    mesh frame.  track_views is the batched track_one that follows."""
    ests, refiner, scorer = _check_estimators("register_views", estimators, scorer=True)
    views, rgbs, depths, Ks, hw = _check_views("register_views", len(ests), views, depths, Ks, rgbs=rgbs)
    masks, ob_ids = _check_masks("register_views", len(ests), ob_masks, ob_ids)
    masks_np = [np.asarray(m.data.cpu().numpy() if torch.is_tensor(m) else m) for m in masks]
    for i, m in enumerate(masks_np):
        if m.shape != hw:
            raise ValueError(f"register_views: mask {i} has shape {m.shape}, the frames are {hw}")
    set_seed(0)
    dev = ests[0].device
    for e in ests:
        if e.glctx is None:
            e.glctx = dr.RasterizeCudaContext(e.device)
    # register()'s depth ingest, once for all frames
    depth_t = stack_frames(depths, dev, torch.float)
    depth_t = ops.bilateral_filter_depth_frames(ops.erode_depth_frames(depth_t, radius=2), radius=2)
    # every mask's translation guess and valid-depth count: one launch, one copy back
    mk = torch.as_tensor(np.stack([m > 0 for m in masks_np]).astype(np.uint8), device=dev)
    box, cnt, lo, hi = ops.mask_depth_stats_host(ops.mask_depth_stats(depth_t, mk, torch.as_tensor(np.asarray(views, np.int32), device=dev)))
    out, hyps, lengths = [None] * len(ests), [], []
    for k, e in enumerate(ests):
        center = translation_from_stats(Ks[views[k]], box[k], cnt[k], lo[k], hi[k])
        if cnt[k] < 4:
            out[k] = _guess_pose(center, f"estimator {k}: ")
            lengths.append(0)
            continue
        P = e.grid_at(center)
        hyps.append(P)
        lengths.append(int(P.shape[0]))
    if not hyps:
        return out
    from .predict_pose_refine import ObjectIndex
    seg = ops.Segments(lengths, dev)
    mset, diam = _object_tables(refiner, ests)
    hyp_view = np.repeat(np.asarray(views, dtype=np.int64), lengths)
    vt = ops.Views(Ks, hyp_view, dev)
    with torch.inference_mode():
        xyz_t = ops.depth_to_xyz_frames(depth_t, vt, zfar=float("inf"), f64_internal=True).contiguous()   # depth2xyzmap (numpy variant)
        rgb_t = stack_frames(rgbs, dev, torch.float, convert_after_upload=True)
        poses, trans, rot = refiner.refine_device(rgb_t, xyz_t, torch.cat(hyps).contiguous(), None, hw[0], hw[1], mset, diam, iteration,
                                                  shared_translation=seg, views=vt,
                                                  obj=ObjectIndex(np.repeat(np.arange(len(ests)), lengths), dev, view=hyp_view))
        refiner.last_trans_update, refiner.last_rot_update = trans, rot
        scores = scorer.predict_objects(rgb_t, depth_t, None, poses, mset, diam, seg, views=vt)
    for k, e in enumerate(ests):
        a, b = seg.rows(k)
        if b > a:
            out[k] = _set_registration(e, poses[a:b], scores[a:b], hw, Ks[views[k]], ob_ids[k], masks_np[k])
    return out
