#!/usr/bin/env python
"""Demo driver with the reference's call sequence and arguments (run_demo.py:15-78): load a mesh, register on the
first frame, track the following frames, write ob_in_cam/<frame>.txt.  `--synthetic N` first writes an N-frame
synthetic sequence (the textured can moving in front of the camera) in the demo layout, because the reference's
demo_data and weights are not redistributable; with real data pass --mesh_file / --test_scene_dir and put the
checkpoints under $FOUNDATIONPOSE_WEIGHTS.  Visualisation (debug >= 1 overlays) is not implemented.
Without a CAD model: `--ref_views DIR` (a directory in the same layout whose frames each carry a mask and an annotated pose) fuses the
object's mesh from those reference views (foundationpose_amd/reconstruct.py) in place of --mesh_file; `--synthetic_ref_views N` writes
such a directory from the can first; `--ref_texture T` bakes a texture atlas of T x T texels a face onto that mesh from the same views;
`--ref_keep_components largest|N` drops floaters from it (all but the largest surface component, or those under N triangles);
`--ref_coverage` prints what of the fused surface the reference views saw (reconstruct.view_coverage) as one JSON line
{"ref_coverage": ...};
`--save_mesh PATH` writes the mesh that was used: a PLY (positions, normals, vertex colours), or with a path ending in .obj an OBJ with
its MTL and the texture as a PNG; `--compare_mesh PATH` (with the reference views) compares the fused mesh with the mesh file PATH, in the
frame of the views' poses -- `--compare_mesh synthetic` with --synthetic_ref_views takes the can the views were rendered from -- and
prints the report (reconstruct.compare_meshes: accuracy, completeness, chamfer, Hausdorff, precision / recall / F-score at 0.5, 1, 2 and
4 voxel pitches) as one JSON line {"compare_mesh": ...}, and with `--signed` a second line {"signed_bias": ...} that says on which side of
that mesh the fused surface lies (reconstruct.signed_bias; a mesh that is not closed is reported as such and its sign is the side of
the nearest face); `--align_mesh` with it registers the fused mesh onto that mesh first
(reconstruct.align_meshes: the mesh file may then be in any frame of the same unit), prints the alignment as one JSON line
{"align_mesh": ...} and compares in the aligned frame; `--detect_symmetry` finds the rotational symmetries of the mesh that is used,
registers with the rotation grid clustered by them and prints the axes as one JSON line {"detect_symmetry": ...}."""
import argparse
import logging
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_synthetic_demo(out_dir, n_frames, dev):
    """textured can, smooth motion, rendered with the product rasteriser; returns (mesh_file, scene_dir, gt poses)"""
    from foundationpose_amd import synthetic as syn
    from foundationpose_amd.datareader import write_sequence
    from foundationpose_amd.mesh import make_can_mesh
    from foundationpose_amd.mesh_io import save_obj
    from foundationpose_amd.Utils import euler_matrix, make_mesh_tensors, nvdiffrast_render
    mesh = make_can_mesh()
    os.makedirs(os.path.join(out_dir, "mesh"), exist_ok=True)
    mesh_file = os.path.join(out_dir, "mesh", "textured_simple.obj")
    save_obj(mesh, mesh_file)
    gm = make_mesh_tensors(mesh, device=dev)
    T0 = syn.gt_pose(0)
    poses = []
    for i in range(n_frames):
        T = T0.copy()
        T[:3, :3] = T0[:3, :3] @ euler_matrix(0.02 * i, 0.015 * i, 0.0)[:3, :3]
        T[:3, 3] = T0[:3, 3] + np.array([0.002 * i, -0.001 * i, 0.003 * i])
        poses.append(T)
    color, depth, _ = nvdiffrast_render(K=syn.YCBV_K, H=syn.H, W=syn.W, ob_in_cams=torch.as_tensor(np.stack(poses), device=dev, dtype=torch.float),
                                        mesh_tensors=gm, use_light=True, extra={})
    cs, ds, ms = [], [], []
    for i in range(n_frames):
        rgb, d, mask = syn.compose_frame(color[i].cpu().numpy(), depth[i].cpu().numpy(), seed=i)
        cs.append(rgb); ds.append(d); ms.append(mask)
    write_sequence(out_dir, syn.YCBV_K, cs, ds, ms, gt_poses=poses)
    return mesh_file, out_dir, poses


def write_synthetic_ref_views(out_dir, n_views, dev, distance=0.5):
    """n_views frames of the can seen from all around at `distance`, composed like the demo frames, with masks and poses"""
    from foundationpose_amd import synthetic as syn
    from foundationpose_amd.datareader import write_sequence
    from foundationpose_amd.mesh import make_can_mesh
    from foundationpose_amd.Utils import make_mesh_tensors, nvdiffrast_render
    gm = make_mesh_tensors(make_can_mesh(), device=dev)
    poses = syn.reference_view_poses(n_views, distance)
    color, depth, _ = nvdiffrast_render(K=syn.YCBV_K, H=syn.H, W=syn.W, ob_in_cams=torch.as_tensor(poses, device=dev, dtype=torch.float),
                                        mesh_tensors=gm, use_light=True, extra={})
    frames = [syn.compose_frame(color[i].cpu().numpy(), depth[i].cpu().numpy(), seed=100 + i) for i in range(n_views)]
    write_sequence(out_dir, syn.YCBV_K, [f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], gt_poses=list(poses))
    return out_dir


def read_ref_views(ref_dir):
    """-> rgbs, depths, masks, ob_in_cams, K of a reference-view directory; every frame needs its mask and its pose"""
    from foundationpose_amd.datareader import YcbineoatReader
    reader = YcbineoatReader(video_dir=ref_dir, shorter_side=None, zfar=np.inf)
    n = len(reader)
    if len(reader.gt_pose_files) != n:
        raise SystemExit(f"--ref_views {ref_dir}: {n} frames but {len(reader.gt_pose_files)} poses under annotated_poses/")
    poses = np.stack([reader.get_gt_pose(i) for i in range(n)])
    return (np.stack([reader.get_color(i) for i in range(n)]), np.stack([reader.get_depth(i) for i in range(n)]).astype(np.float32),
            np.stack([reader.get_mask(i) for i in range(n)]), poses.astype(np.float32), reader.K)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh_file", type=str, default=None)
    ap.add_argument("--test_scene_dir", type=str, default=None)
    ap.add_argument("--est_refine_iter", type=int, default=5)
    ap.add_argument("--track_refine_iter", type=int, default=2)
    ap.add_argument("--debug", type=int, default=0)
    ap.add_argument("--debug_dir", type=str, default=os.path.join(ROOT, "gpurun_out", "demo_debug"))
    ap.add_argument("--synthetic", type=int, default=0, help="write an N-frame synthetic demo sequence first and run on it")
    ap.add_argument("--track_graph", action="store_true", help="replay track_one as one captured hipGraph per frame")
    ap.add_argument("--standin_weights", action="store_true", help="seeded stand-in checkpoints instead of weights/")
    ap.add_argument("--ref_views", type=str, default=None, help="posed RGB-D reference views with masks, in place of --mesh_file")
    ap.add_argument("--synthetic_ref_views", type=int, default=0, help="write N reference views of the can first and use them")
    ap.add_argument("--ref_texture", type=int, default=0, help="with --ref_views: bake a texture atlas of T x T texels a face (2..16)")
    ap.add_argument("--ref_refine_poses", type=int, default=0,
                    help="with --ref_views: rounds of polishing the view poses against the fused mesh (point-to-plane ICP) and fusing again")
    ap.add_argument("--ref_refine_against", choices=("mesh", "volume"), default="mesh",
                    help="with --ref_refine_poses: polish the view poses against the extracted mesh, or against the volume itself (raycast)")
    ap.add_argument("--ref_keep_components", type=lambda v: v if v == "largest" else int(v), default=None, metavar="{largest,N}",
                    help="with --ref_views: drop floaters from the fused mesh: keep the surface component with the most triangles, or every "
                         "component of at least N triangles")
    ap.add_argument("--save_mesh", type=str, default=None, help="write the mesh that is used to this PLY (or .obj: OBJ + MTL + PNG)")
    ap.add_argument("--compare_mesh", type=str, default=None, metavar="PATH",
                    help="with --ref_views: compare the fused mesh with this mesh file (or 'synthetic': the can of --synthetic_ref_views) "
                         "and print the report as one JSON line")
    ap.add_argument("--compare_samples", type=int, default=100_000, help="surface samples per mesh for --compare_mesh and --ref_coverage")
    ap.add_argument("--ref_coverage", action="store_true",
                    help="with --ref_views: print what of the fused mesh's surface the reference views saw (reconstruct.view_coverage: "
                         "the fraction seen by any view and by each, the unseen area) as one JSON line")
    ap.add_argument("--signed", action="store_true",
                    help="with --compare_mesh: also print on which side of that mesh the fused surface lies (reconstruct.signed_bias: "
                         "the mean signed distance, negative inside, the share inside and three percentiles) as one JSON line")
    ap.add_argument("--align_mesh", action="store_true",
                    help="with --compare_mesh: register the fused mesh onto that mesh first (reconstruct.align_meshes: the two need not be "
                         "in one frame), print the alignment as one JSON line and compare in the aligned frame")
    ap.add_argument("--detect_symmetry", action="store_true",
                    help="find the mesh's rotational symmetries (FoundationPose.detect_symmetries), use them for the rotation grid and "
                         "print the axes as one JSON line")
    args = ap.parse_args(argv)
    if args.align_mesh and not args.compare_mesh:
        ap.error("--align_mesh needs --compare_mesh PATH (the mesh to register onto)")
    if args.signed and not args.compare_mesh:
        ap.error("--signed needs --compare_mesh PATH (the closed mesh whose sides are meant)")
    logging.basicConfig(level=logging.INFO, format="[%(funcName)s()] %(message)s")

    from foundationpose_amd import dr
    from foundationpose_amd.datareader import YcbineoatReader
    from foundationpose_amd.estimater import FoundationPose
    from foundationpose_amd.mesh_io import load_mesh, save_obj, save_ply
    from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
    from foundationpose_amd.predict_score import ScorePredictor
    from foundationpose_amd.Utils import set_seed
    from foundationpose_amd.weights import DEFAULT_REFINE_CFG, DEFAULT_SCORE_CFG, random_state_dict

    set_seed(0)
    dev = torch.device("cuda:0")
    gt = None
    if args.synthetic > 0:
        args.mesh_file, args.test_scene_dir, gt = write_synthetic_demo(os.path.join(args.debug_dir, "synthetic_scene"), args.synthetic, dev)
        args.standin_weights = True
    if args.synthetic_ref_views > 0:
        args.ref_views = write_synthetic_ref_views(os.path.join(args.debug_dir, "synthetic_ref_views"), args.synthetic_ref_views, dev)
    if not (args.mesh_file or args.ref_views) or not args.test_scene_dir:
        ap.error("--mesh_file (or --ref_views) and --test_scene_dir are required (or --synthetic N)")
    if args.ref_refine_poses and not args.ref_views:
        ap.error("--ref_refine_poses needs --ref_views (or --synthetic_ref_views N)")
    if args.ref_keep_components is not None and not args.ref_views:
        ap.error("--ref_keep_components needs --ref_views (or --synthetic_ref_views N)")
    if args.ref_coverage and not args.ref_views:
        ap.error("--ref_coverage needs --ref_views (or --synthetic_ref_views N)")
    if args.compare_mesh and not args.ref_views:
        ap.error("--compare_mesh needs --ref_views (or --synthetic_ref_views N)")
    if args.compare_mesh == "synthetic" and not args.synthetic_ref_views:
        ap.error("--compare_mesh synthetic needs --synthetic_ref_views N")
    if args.ref_views:
        from foundationpose_amd.reconstruct import reconstruct_object
        t0 = time.perf_counter()
        ref = read_ref_views(args.ref_views)
        mesh, fused = reconstruct_object(*ref, device=dev, texture=args.ref_texture or None,
                                         refine_poses=args.ref_refine_poses, refine_against=args.ref_refine_against,
                                         keep_components=args.ref_keep_components)
        atlas = getattr(getattr(mesh.visual, "material", None), "image", None)
        logging.info(f"mesh from {args.ref_views}: {len(mesh.vertices)} vertices, {len(mesh.faces)} faces"
                     + ("" if atlas is None else f", atlas {atlas.shape[0]} x {atlas.shape[1]}")
                     + (f", view poses refined {args.ref_refine_poses} x" if args.ref_refine_poses else "")
                     + ("" if args.ref_keep_components is None else f", {len(mesh.components)} surface components, {mesh.dropped_triangles} triangles dropped")
                     + f" in {time.perf_counter() - t0:.2f} s")
        if args.ref_coverage:
            import json
            from foundationpose_amd.reconstruct import view_coverage
            poses = getattr(mesh, "ob_in_cams", None)                      # the polished poses of --ref_refine_poses
            cov = view_coverage(fused, ref[3] if poses is None else poses, ref[4], ref[1].shape[-2:], samples=args.compare_samples)
            logging.info(cov.describe())
            print(json.dumps({"ref_coverage": cov.as_dict()}), flush=True)
        if args.compare_mesh:
            import json
            from foundationpose_amd.mesh import make_can_mesh
            from foundationpose_amd.reconstruct import align_meshes, compare_meshes, signed_bias
            truth = make_can_mesh() if args.compare_mesh == "synthetic" else load_mesh(args.compare_mesh)
            alignment = None
            if args.align_mesh:
                alignment = align_meshes(fused, truth, device=dev)
                ru = alignment.runner_up
                print(json.dumps({"align_mesh": dict(
                    tf=alignment.tf.tolist(), mean_distance_m=alignment.mean_distance, rmse_m=alignment.rmse, overlap=alignment.overlap,
                    status=alignment.status, runner_up=None if ru is None else dict(
                        tf=ru["tf"].tolist(), mean_distance_m=ru["mean_distance"], rmse_m=float(np.sqrt(ru["cost"])), angle_deg=ru["angle_deg"]))}),
                      flush=True)
            report = compare_meshes(fused, truth, samples=args.compare_samples, unit=mesh.voxel, device=dev, tf=alignment).as_dict()
            report.update(unit_m=mesh.voxel, faces=[len(mesh.faces), len(truth.faces)])
            if alignment is not None:
                report.update(aligned=True)
            print(json.dumps({"compare_mesh": report}), flush=True)
            if args.signed:
                from foundationpose_amd import ops
                truth_t = dict(pos=torch.as_tensor(np.asarray(truth.vertices, dtype=np.float32), device=dev),
                               faces=torch.as_tensor(np.asarray(truth.faces).astype(np.int32), device=dev))
                tables = ops.mesh_pseudonormals(truth_t)
                bias = signed_bias(fused, truth_t, samples=args.compare_samples, device=dev, tf=alignment, allow_open=True)
                print(json.dumps({"signed_bias": dict(mean_m=bias.mean, inside=bias.inside, p5_m=bias.p5, p50_m=bias.p50, p95_m=bias.p95,
                                                      closed=tables.closed, mesh_report=tables.describe())}), flush=True)
    else:
        mesh = load_mesh(args.mesh_file)
    if args.ref_texture and not args.ref_views:
        ap.error("--ref_texture needs --ref_views (or --synthetic_ref_views N)")
    if args.save_mesh:
        (save_obj if args.save_mesh.lower().endswith(".obj") else save_ply)(mesh, args.save_mesh)
    os.makedirs(os.path.join(args.debug_dir, "ob_in_cam"), exist_ok=True)
    if args.standin_weights:
        scorer = ScorePredictor(cfg=dict(DEFAULT_SCORE_CFG), state_dict=random_state_dict("score", seed=0), device=dev)
        refiner = PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), state_dict=random_state_dict("refine", seed=0), device=dev)
    else:
        scorer, refiner = ScorePredictor(device=dev), PoseRefinePredictor(device=dev)
    glctx = dr.RasterizeCudaContext()
    est = FoundationPose(model_pts=mesh.vertices, model_normals=mesh.vertex_normals, mesh=mesh, scorer=scorer, refiner=refiner,
                         debug_dir=args.debug_dir, debug=args.debug, glctx=glctx, device=dev, track_graph=args.track_graph)
    if args.detect_symmetry:
        import json
        import math
        rec = est.detect_symmetries()                     # a fused mesh: within two voxels of its pitch; a CAD model: 1 % of its extent
        print(json.dumps({"detect_symmetry": dict(
            transforms=len(rec.tfs), hypotheses=len(est.rot_grid), tol_m=rec.tol, largest_residual_m=float(rec.residuals.max()),
            axes=[dict(axis=[float(x) for x in a], order="continuous" if k == math.inf else int(k)) for a, k in rec.axes])}), flush=True)
    logging.info("estimator initialization done")
    reader = YcbineoatReader(video_dir=args.test_scene_dir, shorter_side=None, zfar=np.inf)
    times = []
    for i in range(len(reader.color_files)):
        color, depth = reader.get_color(i), reader.get_depth(i)
        t0 = time.perf_counter()
        if i == 0:
            mask = reader.get_mask(0).astype(bool)
            pose = est.register(K=reader.K, rgb=color, depth=depth, ob_mask=mask, iteration=args.est_refine_iter)
        else:
            pose = est.track_one(rgb=color, depth=depth, K=reader.K, iteration=args.track_refine_iter)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        np.savetxt(os.path.join(args.debug_dir, "ob_in_cam", f"{reader.id_strs[i]}.txt"), pose.reshape(4, 4))
    logging.info(f"register {times[0] * 1e3:.1f} ms; track_one median {np.median(times[1:]) * 1e3 if len(times) > 1 else float('nan'):.2f} ms/frame "
                 f"over {len(times) - 1} frames; poses in {args.debug_dir}/ob_in_cam")
    return times


if __name__ == "__main__":
    main()
