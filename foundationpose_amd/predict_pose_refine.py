"""PoseRefinePredictor -- drop-in for learning/training/predict_pose_refine.py:93-295.

``predict`` keeps the reference signature and return types.  Per iteration the reference launches ~60 kernels
(crop tf, nvdiffrast x7, kornia warps, dataset transform, concat, pose update); here it is four launches of
libfp_amd.so (fp_crop_windows, fp_render_crops, fp_warp_crops, fp_pose_update) around the network plan, with
no host round trip inside the loop.
"""
import os

import numpy as np
import torch

from . import ops
from .crops import Scene, crop_stage
from .Utils import get_mesh_handle, make_mesh_tensors
from .engine import RefinePlan
from .h5_dataset import PoseRefinePairH5Dataset
from .graphs import GraphCache, PartGraphs
from .overlap import SubBatches
from .pose_dataset import BatchPoseData
from .refine_network import RefineNet

_REFINE_DEFAULTS = dict(use_normal=False, use_mask=False, use_BN=False, c_in=4, crop_ratio=1.2, n_view=1,
                        trans_rep="tracknet", rot_rep="axis_angle", zfar=3, normalize_xyz=False, normal_uint8=False)


class _Cfg(dict):
    """dict with attribute access (stands in for OmegaConf's DictConfig, which is not available here)."""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def load_run(run_name, weights_root=None):
    """weights/<run_name>/{config.yml, model_best.pth} as in predict_pose_refine.py:97-141."""
    import yaml
    root = weights_root or os.environ.get("FOUNDATIONPOSE_WEIGHTS") or os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "weights")
    cfg_path = os.path.join(root, run_name, "config.yml")
    ckpt_path = os.path.join(root, run_name, "model_best.pth")
    if not (os.path.exists(cfg_path) and os.path.exists(ckpt_path)):
        raise FileNotFoundError(
            f"pretrained run '{run_name}' not found under {root}; pass cfg= and state_dict= explicitly "
            f"(e.g. foundationpose_amd.weights.random_state_dict) or set FOUNDATIONPOSE_WEIGHTS")
    with open(cfg_path) as f:
        cfg = yaml.safe_load(f)
    ckpt = torch.load(ckpt_path, map_location="cpu")
    if "model" in ckpt:
        ckpt = ckpt["model"]
    return cfg, ckpt, ckpt_path


def make_crop_data_batch(render_size, ob_in_cams, mesh, rgb, depth, K, crop_ratio, xyz_map, normal_map=None,
                         mesh_diameter=None, cfg=None, glctx=None, mesh_tensors=None, dataset=None, AB=None, depth_hw=None):
    """Reference: predict_pose_refine.py:26-89.  Returns a BatchPoseData whose rgbAs/xyz_mapAs/rgbBs/xyz_mapBs are
    views into one (2N,6,h,w) network-input buffer (``batch.AB``): A = rendered hypothesis, B = observed crop."""
    H, W = depth_hw if depth is None else depth.shape[:2]
    handle = get_mesh_handle(mesh_tensors)
    poseA = torch.as_tensor(ob_in_cams, dtype=torch.float, device=handle.device).reshape(-1, 4, 4).contiguous()
    N = poseA.shape[0]
    oh, ow = int(cfg["input_resize"][0]), int(cfg["input_resize"][1])
    if AB is None:
        AB = torch.empty((2 * N, 6, oh, ow), dtype=torch.float32, device=handle.device)
    normalize = bool(cfg["normalize_xyz"])
    tf_to_crops, bbox2d = crop_stage(Scene(handle, mesh_diameter, K, H, W, N), poseA, rgb, xyz_map, None, ops.MODE_REFINE, crop_ratio,
                                     (oh, ow), 0.001, normalize, AB, adjust_bbox=two_pose_call_quirk if N == 2 else None, chunk=4096,
                                     window_hw=render_size)
    normalAs = normalBs = None
    if cfg.get("use_normal", False):
        # predict_pose_refine.py:50,58,75-76: the rendered normals and the frame's normal map go through the SAME nearest
        # warp by tf_to_crops (the rendered crop is treated as if it were a frame -- reference behaviour, kept) into
        # BatchPoseData.normalAs / normalBs.  The reference never concatenates them into the network input (:187-188 take rgb
        # and xyz only), so this is bookkeeping off the hot path: plain torch ops, and refine_part() skips it.
        if normal_map is None:
            raise ValueError("use_normal=True needs a normal_map (the reference fails in torch.as_tensor(None) here)")
        from .Utils import warp_perspective_nearest
        nr = torch.cat([ops.render_crops(handle, poseA[b:b + 4096], bbox2d[b:b + 4096], K, H, W, out_hw=(oh, ow), mesh_diameter=mesh_diameter,
                                         xyz_thr=0.001, normalize_xyz=normalize, want=("normal",))["normal"] for b in range(0, N, 4096)])
        normalAs = warp_perspective_nearest(nr.permute(0, 3, 1, 2).contiguous(), tf_to_crops, render_size)
        nm = torch.as_tensor(normal_map, dtype=torch.float, device=handle.device).permute(2, 0, 1)[None].expand(N, -1, -1, -1)
        normalBs = warp_perspective_nearest(nm, tf_to_crops, render_size)
    Ks = torch.as_tensor(np.asarray(K, dtype=np.float64), device=handle.device, dtype=torch.float).reshape(1, 3, 3)
    mesh_diameters = torch.ones((N,), dtype=torch.float, device=handle.device) * float(mesh_diameter)
    batch = BatchPoseData(rgbAs=AB[:N, :3], rgbBs=AB[N:, :3], xyz_mapAs=AB[:N, 3:], xyz_mapBs=AB[N:, 3:], poseA=poseA,
                          normalAs=normalAs, normalBs=normalBs, tf_to_crops=tf_to_crops, Ks=Ks, mesh_diameters=mesh_diameters)
    batch.AB = AB
    batch.bbox2d = bbox2d
    if dataset is not None:
        batch = dataset.transform_batch(batch=batch, H_ori=H, W_ori=W, bound=1)
    return batch


def resolve_shared_translation(ob_in_cams, flag):
    """-> bool: may the first refine iteration treat the hypotheses as sharing one translation (PoseRefinePredictor.predict)?
    flag True: the caller says so -- and is checked: host poses on the host, a device tensor with one reduction on the device
    (one scalar read back; skipped only inside a stream capture, where nothing may synchronise); None: decided from host poses
    -- compared as the float32 values that are uploaded -- and False for a device tensor, which is not read back for a mere
    optimisation; False: no."""
    on_host = isinstance(ob_in_cams, np.ndarray) or (torch.is_tensor(ob_in_cams) and ob_in_cams.device.type == "cpu") or \
        isinstance(ob_in_cams, (list, tuple))
    if not on_host:
        if flag and torch.is_tensor(ob_in_cams) and ob_in_cams.is_cuda and not torch.cuda.is_current_stream_capturing():
            t = ob_in_cams.reshape(-1, 4, 4)[:, :3, 3].float()
            if t.shape[0] > 1 and not bool((t == t[:1]).all().item()):
                raise ValueError("shared_translation=True, but the hypotheses do not have one translation")
        return bool(flag)
    t = np.asarray(ob_in_cams, dtype=np.float32).reshape(-1, 4, 4)[:, :3, 3]
    same = bool(t.shape[0] > 1 and (t == t[:1]).all())
    if flag and t.shape[0] > 1 and not same:
        raise ValueError("shared_translation=True, but the hypotheses do not have one translation")
    return same if flag is None else bool(flag) and same


def two_pose_pairs(obj, view=None):
    """The reference's two-pose broadcasting quirk in a call that refines several objects: a call of exactly two
    poses renders both with [umin_0, vmin_0, umax_1, vmax_1], and in a multi-object call the quirk belongs to each object's own
    call, so it applies to an object with exactly two hypotheses -- pairing them in call order -- and never across objects.
    obj: per-hypothesis object index (host sequence).  view: per-hypothesis view index (host sequence) or None: a reference call is
    ONE frame of one object, so over several views the quirk is grouped per (view, object) and never pairs two frames.
    -> sorted [(i, j)]: the rows of every group with exactly two hypotheses"""
    obj = np.asarray(obj).reshape(-1).tolist()
    view = [0] * len(obj) if view is None else np.asarray(view).reshape(-1).tolist()
    if len(view) != len(obj):
        raise ValueError(f"two_pose_pairs: {len(obj)} object indices but {len(view)} view indices")
    rows = {}
    for n, key in enumerate(zip(view, obj)):
        rows.setdefault(key, []).append(n)
    return sorted(tuple(r) for r in rows.values() if len(r) == 2)


def parts_for_pairs(parts, pairs):
    """hypothesis sub-batches (row ranges) in which every quirk pair lies inside one part (both of its rows are rendered in the same
    launch): `parts` unchanged, or one part over the whole call"""
    for i, j in pairs:
        if not any(a <= i and j < b for a, b in parts):
            return [(parts[0][0], parts[-1][1])]
    return list(parts)


def segment_pieces(offsets, a, b):
    """the pieces of the segments (host offsets, ops.Segments.offsets) that fall into rows a..b of a call: [(start, end)] relative
    to a, in order, empty pieces dropped.  A segment may straddle the part boundary (each part gets its piece of it) and a piece may
    be a single row.  The first refine iteration warps one observed crop per piece (refine_part with a segmented
    shared_translation)."""
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    lo, hi = np.maximum(off[:-1], a), np.minimum(off[1:], b)
    keep = hi > lo
    return [(int(s) - a, int(e) - a) for s, e in zip(lo[keep], hi[keep])]


class ObjectIndex(ops.PairRows):
    """The per-hypothesis object index of a refine call over several objects: hypothesis n belongs to object obj[n] -- entry obj[n]
    of the MeshSet and of the diameter table (ops.object_diameters).  Built once from host data: the int32 device index the kernels
    read, and the rows of the two-pose quirk (two_pose_pairs) as a device table, so a captured refine loop copies nothing.
    view: the call's per-hypothesis view index (the host index of its ops.Views) when it spans several views: the quirk is then
    grouped per (view, object)."""

    def __init__(self, obj, device, view=None):
        self.host = np.asarray(obj, dtype=np.int64).reshape(-1)
        if self.host.size and self.host.min() < 0:
            raise ValueError("ObjectIndex: negative object index")
        self.view = None if view is None else np.asarray(view, dtype=np.int64).reshape(-1)
        self.dev = torch.as_tensor(self.host.astype(np.int32), device=device)
        super().__init__(two_pose_pairs(self.host, self.view), device)

    def __len__(self):
        return int(self.host.size)


def apply_two_pose_quirk(bbox2d, pairs):
    """bbox2d (n, 4), in place: both rows of every pair (i, j) get [umin_i, vmin_i, umax_j, vmax_j]"""
    q = torch.cat([bbox2d.index_select(0, pairs[:, 0])[:, :2], bbox2d.index_select(0, pairs[:, 1])[:, 2:]], 1)
    bbox2d.index_copy_(0, pairs[:, 0], q)
    bbox2d.index_copy_(0, pairs[:, 1], q)
    return bbox2d


def two_pose_call_quirk(bbox2d):
    """the quirk of a call of exactly two poses: transform_pts pairs pose i with corner i, so both are rendered with
    [umin_0, vmin_0, umax_1, vmax_1].  bbox2d (2, 4) -> a new one: apply_two_pose_quirk's values through the torch kernels a captured graph holds"""
    return torch.stack([bbox2d[0, 0], bbox2d[0, 1], bbox2d[1, 2], bbox2d[1, 3]])[None].expand(2, 4).contiguous()


class PoseRefinePredictor:
    run_name = "2023-10-28-18-33-37"

    def __init__(self, cfg=None, state_dict=None, weights_root=None, device="cuda", precision="fp16", channels_last=True,
                 n_streams=2, graph="auto"):
        """precision='fp16': the reference's deployed autocast configuration on libfp_amd.so (engine.py);
        'fp32': fp32 torch ops, no autocast (`amp=False` in the reference).  n_streams: hypothesis sub-batches that run
        concurrently (overlap.py); 1 = one launch sequence over the whole batch.  graph: hipGraph replay of predict()'s refine
        loop (fp16 plan only): True = capture at the first call of a (shape, intrinsics, mesh, iteration) key, "auto" = at the
        second (graphs.GraphCache), False = always eager launches; per call: predict(graph=...)"""
        self.sub = SubBatches(n_streams)
        self.graph = graph
        self._graphs = GraphCache()
        self.amp = precision != "fp32"
        if cfg is None or state_dict is None:
            cfg, state_dict, ckpt_dir = load_run(self.run_name, weights_root)
        else:
            ckpt_dir = None
        self.cfg = _Cfg(cfg)
        self.cfg["ckpt_dir"] = ckpt_dir
        self.cfg["enable_amp"] = True
        for k, v in _REFINE_DEFAULTS.items():  # backward-compat defaults, predict_pose_refine.py:107-130
            if k not in self.cfg or (k == "crop_ratio" and self.cfg[k] is None):
                self.cfg[k] = v
        if isinstance(self.cfg["zfar"], str) and "inf" in self.cfg["zfar"].lower():
            self.cfg["zfar"] = np.inf
        for k in ("input_resize", "trans_normalizer", "rot_normalizer"):
            if k not in self.cfg:
                raise KeyError(f"refiner cfg lacks required key '{k}'")
        # use_normal=True is accepted: in the reference it only adds normalAs / normalBs to the BatchPoseData of
        # make_crop_data_batch (above); predict() builds A and B from rgb and xyz alone (predict_pose_refine.py:187-188),
        # so the networks -- and refine_part() here -- never see the normals.  For the same reason c_in has to be 6: with any
        # other value the reference's own forward fails on the 6-channel A / B (channel mismatch in the first conv).
        if self.cfg["c_in"] != 6:
            raise NotImplementedError("c_in must be 6: predict() feeds cat([rgb, xyz]) to the network whatever use_normal says "
                                      "(predict_pose_refine.py:187-188); the reference fails in its first conv otherwise")
        self.dataset = PoseRefinePairH5Dataset(cfg=self.cfg, h5_file="", mode="test")
        self.device = torch.device(device)
        self.precision = precision
        self._plan_opts = dict(precision=precision, channels_last=channels_last)
        self.model = RefineNet(cfg=self.cfg, c_in=self.cfg["c_in"])
        self.model.load_state_dict(state_dict)
        self.model.to(self.device).eval()
        self._plan = None
        self.small_calls = True      # engine.RefinePlan.small_calls: False = a few-hypothesis call runs the kernels of a large one (dist.py)
        self.last_trans_update = None
        self.last_rot_update = None

    def plan(self):
        dev = next(self.model.parameters()).device
        if self._plan is None or self._plan_dev != dev:
            self._plan = RefinePlan(self.model, dev, **self._plan_opts)
            self._plan.two_stream_heads = self.sub.n_streams > 1      # n_streams=1 switches every use of the side stream off
            self._plan_dev = dev
            if self._plan.hip and self._plan.two_stream_heads and dev.type == "cuda" and not torch.cuda.is_current_stream_capturing():
                # create and probe the side stream NOW (spin kernels + the rasteriser canary synchronise): the first small call -- the
                # reference's track_one -- must not pay for it, and a capture must never meet an unprobed stream (engine._head_side_stream)
                from .overlap import reserve_streams
                reserve_streams(dev, 1)
        self._plan.small_calls = bool(self.small_calls)
        return self._plan

    def _loop_constants(self):
        oh, ow = int(self.cfg["input_resize"][0]), int(self.cfg["input_resize"][1])
        tn = self.cfg["trans_normalizer"]
        tn = [float(tn)] * 3 if isinstance(tn, (int, float)) else [float(v) for v in tn]
        return oh, ow, tn, bool(self.cfg["normalize_xyz"])

    def refine_part(self, slot, rows, rgb_t, xyz_t, poses, scene, iterations, outs, workspace=None, state=None, shared_translation=False):
        """Iterations `iterations` (a range) of the refine loop for the hypotheses rows=(a, b) of `poses`, on the CURRENT
        stream, with the activation-buffer set `slot`: per iteration crops.crop_stage (fp_crop_windows -> fp_render_crops (A) +
        fp_warp_crops (B)) -> RefineNet plan -> fp_pose_update.  scene: the crops.Scene of ALL of `poses` (rows a..b of it are this
        part's; with views rgb_t / xyz_t are (V,H,W,3) stacks).  outs = (poses_out (N,4,4), trans_delta (N,3), rot_delta (N,3,3),
        n_iterations_total): the last iteration writes rows a..b of them.  state: what the previous call for this part returned (None
        for the first iteration).  shared_translation: the hypotheses a..b all have the same translation (register(): estimater.py:132-133
        puts every rotation of the grid at the guessed centre), so in iteration 0 they share one crop window and one observed crop: it
        is warped once and the stem of the fp16 plan encodes it once (engine._HipEncoder, bit-identical to 252 copies).  Or an
        ops.Segments of the call's rows (a batched registration; the caller guarantees one translation per segment): iteration 0 warps
        one observed crop per piece of a segment in this part (segment_pieces), from the piece's first row, and the plan replicates each
        into its rows (engine._HipEncoder, segmented shared_b).  -> state"""
        plan = self.plan()
        a, b = rows
        n = b - a
        oh, ow, tn, normalize = self._loop_constants()
        poses_out, trans_delta, rot_delta, total = outs
        part = scene.rows(a, b)
        pairs = part.pairs if part.grouped else None        # the quirk per object / view (two_pose_pairs), or of the whole call
        quirk = (lambda bbox2d: apply_two_pose_quirk(bbox2d, pairs)) if pairs is not None else \
            two_pose_call_quirk if not part.grouped and poses.shape[0] == 2 else None
        segmented = isinstance(shared_translation, ops.Segments)
        if state is None:
            state = dict(P=poses[a:b], AB=torch.empty((2 * n, 6, oh, ow), dtype=plan.dtype, device=poses.device), raw=None)
        for it in iterations:
            last = it + 1 == total
            P, AB = state["P"], state["AB"]
            # iteration 0 of a shared translation: B rows n..n+S hold one observed crop per piece (S pieces), the plan replicates them
            pieces = segment_pieces(shared_translation.offsets, a, b) if segmented and it == 0 and plan.hip else None
            if pieces is not None and len(pieces) < n:
                warp_rows = (np.asarray([p0 for p0, _ in pieces], dtype=np.int64), AB[n:n + len(pieces)])
                shared_b = ops.Segments([e - p0 for p0, e in pieces], poses.device)
            elif bool(shared_translation) and not segmented and it == 0 and n > 1 and plan.hip:
                warp_rows, shared_b = ((0, 1), AB[n:n + 1]), True
            else:
                warp_rows = shared_b = None
            tf_to_crops, _ = crop_stage(part, P, rgb_t, xyz_t, None, ops.MODE_REFINE, self.cfg["crop_ratio"], (oh, ow), 0.001, normalize,
                                        AB, workspace=workspace, adjust_bbox=quirk, warp_rows=warp_rows)
            raw = plan(AB, slot=slot) if warp_rows is None else plan(AB[:n + warp_rows[1].shape[0]], slot=slot, shared_b=shared_b)
            state["raw"] = raw
            state["P"] = part.pose_update(raw["trans"], raw["rot"], P, rot_rep=self.cfg["rot_rep"], normalize_xyz=normalize,
                                          trans_normalizer=tn, rot_normalizer=float(self.cfg["rot_normalizer"]),
                                          out=poses_out[a:b] if last else None, trans_delta_out=trans_delta[a:b] if last else None,
                                          rot_delta_out=rot_delta[a:b] if last else None, trans_rep=str(self.cfg["trans_rep"]),
                                          tf_to_crops=tf_to_crops, input_w=float(self.cfg["input_resize"][0]))
        return state

    def depth_check(self, poses, xyz_t, scene, tol, out=None, workspace=None):
        """How well the poses (N,4,4) agree with the observed xyz map the refine loop read: the crop windows of the loop (crop_ratio,
        input_resize; the two-pose quirk is not applied: every pose is judged through its own window), the render's depth there and
        ops.depth_agreement against xyz_t through the same windows, on the CURRENT stream -> the (N, 4) int32 table [model, valid,
        agree, behind] (`out` if given).  scene: the crops.Scene of these poses (a part's: scene.rows(a, b)); workspace: the part's
        rasteriser scratch.  Writes only its own buffers."""
        oh, ow, _, _ = self._loop_constants()
        tf_to_crops, bbox2d = scene.crop_windows(poses, self.cfg["crop_ratio"], (ow, oh))
        depth = scene.render_crops(poses, bbox2d, (oh, ow), xyz_thr=0.001, normalize_xyz=False, want=("depth",), workspace=workspace)["depth"]
        return scene.depth_agreement(depth, xyz_t, tf_to_crops, tol, out=out)

    def depth_polish(self, poses, xyz_t, scene, iterations=3, max_dist=0.02, damping=1e-3, workspace=None):
        """Polish the poses (N,4,4) against the observed xyz map by `iterations` Gauss-Newton steps of point-to-plane ICP
        (ops.icp_point_plane; include/fp_amd.h has the definition), on the CURRENT stream.  Per iteration: the crop windows of the loop
        at the current poses (crop_ratio, input_resize; every pose through its own window: the two-pose quirk is not applied), the
        render's camera-frame xyz and normals there, and one step against xyz_t through the same windows.  The poses ping-pong between
        two buffers of the call's own; `poses` is only read.  scene: the crops.Scene of these poses; workspace: the rasteriser scratch.
        -> (poses (N,4,4), system (N,40) float64 of the LAST iteration: ops.IcpStep.rows reads it)."""
        if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or int(iterations) < 1:
            raise ValueError(f"depth_polish: iterations must be an int >= 1, got {iterations!r}")
        ops._check_icp(max_dist, damping, 64, "depth_polish")
        oh, ow, _, _ = self._loop_constants()
        N = int(poses.shape[0])
        P = poses
        buf = [torch.empty((N, 4, 4), dtype=torch.float32, device=poses.device) for _ in range(min(2, int(iterations)))]
        system = torch.empty((N, 40), dtype=torch.float64, device=poses.device)
        icp_ws = ops.icp_workspace(N, oh, ow, poses.device)
        for it in range(int(iterations)):
            tf_to_crops, bbox2d = scene.crop_windows(P, self.cfg["crop_ratio"], (ow, oh))
            r = scene.render_crops(P, bbox2d, (oh, ow), xyz_thr=0.001, normalize_xyz=False, want=("xyz", "normal"), workspace=workspace)
            P, _ = scene.icp_point_plane(r["xyz"], r["normal"], xyz_t, tf_to_crops, P, max_dist, damping=damping, system=system,
                                         poses_out=buf[it % 2], workspace=icp_ws)
        return P, system

    def refine_device(self, rgb_t, xyz_t, poses, K, H, W, mesh_handle, mesh_diameter, iteration, workspace=None,
                      shared_translation=False, obj=None, views=None):
        """The refine loop on device tensors only (predict_pose_refine.py:182-235).  No host round trip, no host-side
        tensor creation.  Hypotheses are independent through all iterations, so the parts of `self.sub.parts(N)` run the
        whole loop as independent launch sequences on concurrent streams (overlap.py), issued iteration by iteration and
        joined once at the end.  workspace: optional rasteriser scratch, one uint8 tensor per part.
        -> (poses (N,4,4), trans_delta (N,3) in metres, rot_mat_delta (N,3,3)) of the last iteration, as the reference
        keeps them in last_trans_update / last_rot_update (predict_pose_refine.py:238-239).
        K .. mesh_diameter, obj and views make the call's crops.Scene (which checks their rules).  Several objects: mesh_handle = an
        ops.MeshSet, mesh_diameter = its ops.object_diameters table, obj = an ObjectIndex of the N hypotheses (any order).  Several views:
        views = an ops.Views of the N hypotheses, rgb_t / xyz_t = (V,H,W,3) stacks, the ObjectIndex built with view=views.host.
        shared_translation=True is refused with views; an ops.Segments of the N rows (one translation each) works with obj, views or both."""
        self.plan()
        N = poses.shape[0]
        dev = poses.device
        segmented = isinstance(shared_translation, ops.Segments)
        if segmented and shared_translation.total != N:
            raise ValueError(f"refine_device: {N} poses but shared_translation segments cover {shared_translation.total}")
        if views is not None and shared_translation and not segmented:
            raise ValueError("refine_device: shared_translation (registration) is not supported with views")
        scene = Scene(mesh_handle, mesh_diameter, K, H, W, N, obj=obj, views=views, who="refine_device")
        parts = parts_for_pairs(self.sub.parts(N, dev), scene.pair_list)
        if workspace is not None and torch.is_tensor(workspace):
            workspace = [workspace]
        if workspace is not None and len(workspace) != len(parts):
            raise ValueError(f"refine_device: {len(parts)} parts need {len(parts)} workspaces, got {len(workspace)}")
        outs = self.alloc_outputs(N, dev) + (int(iteration),)
        if iteration <= 0:          # no update happened: the pose unchanged, a zero translation and an identity rotation delta
            outs[0].copy_(poses)
            outs[1].zero_()
            outs[2].copy_(torch.eye(3, dtype=torch.float32, device=dev).expand(N, 3, 3))
        streams = self.sub.streams(dev, len(parts))
        self.sub.fork(streams)
        state = [None] * len(parts)
        for it in range(iteration):
            for h, rows in enumerate(parts):
                with torch.cuda.stream(streams[h]):
                    state[h] = self.refine_part(h, rows, rgb_t, xyz_t, poses, scene, range(it, it + 1), outs,
                                                None if workspace is None else workspace[h], state[h], shared_translation=shared_translation)
        self.sub.join(streams)
        self._raw_parts = [None if st is None else st["raw"] for st in state]   # last_raw_output
        return outs[:3]

    def refine_graphed(self, rgb_t, xyz_t, poses, K, H, W, mesh_tensors, mesh_diameter, iteration, shared_translation, mode):
        """refine_device as a replay of hipGraphs: ONE linear graph per hypothesis sub-batch holding its whole `iteration`-deep
        launch sequence (~90 launches per iteration), replayed on the sub-batch streams (graphs.PartGraphs) -- the same kernels
        on the same streams in the same order, so the result is bit-identical to the eager loop
        (tests/test_gpu_parity.py::test_graphed_predict_is_the_eager_predict).  Everything a launch addresses by raw pointer is
        static and owned by the cache entry: copies of the frame (rgb, xyz_map) and of the start poses, the outputs, one
        rasteriser scratch per part; intermediates live in the graphs' private pools, activations in the plan (never dropped).
        -> (poses, trans_delta, rot_delta) as fresh tensors, or None when this call is to run eagerly (`mode`, GraphCache)"""
        plan = self.plan()
        if not plan.hip or iteration <= 0 or mode is False or mode is None or torch.cuda.is_current_stream_capturing() \
                or ops.KernelTimers.active is not None:
            return None
        dev, N = poses.device, int(poses.shape[0])
        handle = get_mesh_handle(mesh_tensors)
        parts = tuple(self.sub.parts(N, dev))
        key = (N, int(iteration), H, W, np.asarray(K, dtype=np.float64).tobytes(), id(handle), float(mesh_diameter),
               bool(shared_translation), parts, bool(self.sub.serial), dev.index, bool(plan.small_calls))

        def build():
            oh, ow, _, _ = self._loop_constants()
            scene = Scene(handle, mesh_diameter, K, H, W, N)
            g = dict(rgb=torch.empty_like(rgb_t), xyz=torch.empty_like(xyz_t), poses=torch.empty_like(poses), mesh=mesh_tensors,
                     outs=self.alloc_outputs(N, dev) + (int(iteration),), state=[None] * len(parts),
                     ws=[scene.workspace(b - a, oh, ow, dev) for a, b in parts])
            g["rgb"].copy_(rgb_t); g["xyz"].copy_(xyz_t); g["poses"].copy_(poses)

            def body(h):
                g["state"][h] = self.refine_part(h, parts[h], g["rgb"], g["xyz"], g["poses"], scene, range(int(iteration)), g["outs"],
                                                 g["ws"][h], None, shared_translation=shared_translation)
            g["graphs"] = PartGraphs(self.sub, dev, len(parts), body)
            return g
        g = self._graphs.get(key, mode, build)
        if g is None:
            return None
        g["rgb"].copy_(rgb_t); g["xyz"].copy_(xyz_t); g["poses"].copy_(poses)
        g["graphs"].replay()
        self._raw_parts = [st["raw"] for st in g["state"]]      # tensors of the graphs' pools, refreshed by every replay
        return tuple(t.clone() for t in g["outs"][:3])

    @staticmethod
    def alloc_outputs(N, dev):
        return (torch.empty((N, 4, 4), dtype=torch.float32, device=dev), torch.empty((N, 3), dtype=torch.float32, device=dev),
                torch.empty((N, 3, 3), dtype=torch.float32, device=dev))

    @property
    def last_raw_output(self):
        raw = getattr(self, "_raw_parts", None)
        if not raw or raw[0] is None:
            return None
        return {k: torch.cat([r[k] for r in raw], 0) for k in raw[0]}

    @torch.inference_mode()
    def predict(self, rgb, depth, K, ob_in_cams, xyz_map, normal_map=None, get_vis=False, mesh=None,
                mesh_tensors=None, glctx=None, mesh_diameter=None, iteration=5, shared_translation=None, graph=None):
        """@rgb (H,W,3) uint8/float np or tensor; @ob_in_cams (N,4,4) np or tensor.  -> ((N,4,4) f32 device tensor, vis).
        shared_translation (not in the reference's signature): True = the caller guarantees that all hypotheses have the
        same translation (register()); None = found out here when ob_in_cams is host data (a device tensor is not read
        back: treated as False); False = never share.  It only removes repeated work (refine_part), never changes a bit.
        graph (not in the reference's signature either): None = the predictor's setting (constructor), else True / "auto" /
        False as there -- hipGraph replay of the loop (refine_graphed), bit-identical to the eager launches."""
        self.plan()
        dev = self._plan_dev
        shared_translation = resolve_shared_translation(ob_in_cams, shared_translation)
        if mesh_tensors is None:
            mesh_tensors = make_mesh_tensors(mesh, device=dev)
        B_in_cams = torch.as_tensor(ob_in_cams, device=dev, dtype=torch.float).reshape(-1, 4, 4).contiguous()
        rgb_t = torch.as_tensor(rgb, device=dev).to(torch.float).contiguous()
        xyz_t = torch.as_tensor(xyz_map, device=dev, dtype=torch.float).contiguous()
        H, W = int(rgb_t.shape[0]), int(rgb_t.shape[1])
        done = self.refine_graphed(rgb_t, xyz_t, B_in_cams, K, H, W, mesh_tensors, mesh_diameter, int(iteration),
                                   bool(shared_translation), self.graph if graph is None else graph)
        B_in_cams, trans, rot = done if done is not None else \
            self.refine_device(rgb_t, xyz_t, B_in_cams, K, H, W, get_mesh_handle(mesh_tensors), mesh_diameter, iteration,
                               shared_translation=bool(shared_translation))
        self.last_trans_update = trans
        self.last_rot_update = rot
        if get_vis:
            # debug canvas (predict_pose_refine.py:241-291): network inputs at the initial poses above those at the refined poses
            from .vis import crop_rows_canvas, make_grid_image
            P_in = torch.as_tensor(ob_in_cams, device=dev, dtype=torch.float).reshape(-1, 4, 4).contiguous()
            canv = []
            for P in (P_in, B_in_cams):
                b = make_crop_data_batch(self.cfg["input_resize"], P, mesh, rgb_t, None, K, self.cfg["crop_ratio"], xyz_t, cfg=self.cfg,
                                         mesh_tensors=mesh_tensors, mesh_diameter=mesh_diameter, depth_hw=(H, W))
                n = P.shape[0]
                canv.append(crop_rows_canvas(b.AB[:n].cpu().numpy(), b.AB[n:].cpu().numpy()))
            return B_in_cams, make_grid_image(canv, nrow=2, padding=2, pad_value=255)
        return B_in_cams, None
