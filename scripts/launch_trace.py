"""Which entry points of libfp_amd.so the crop stage and the refine / score loops call, in which order and with which scalars, plus
the CRC32 of what the calls return: a fixed, seeded list of small eager calls on the synthetic scene, written as JSON.  Two commits
whose host code issues the same launches give files that are equal apart from the header; a refactor of the host code is checked by
running this script, unchanged, on both.

After the library is loaded a recording proxy stands in for it (foundationpose_amd._lib._lib): every fp_* call is recorded as its name,
its integer and float arguments (floats as hex) and, for a pointer, only whether it is null.  The calls of all scenarios share one table
(`calls`); a scenario's `trace` lists indices into it.  Sub-batch overlap is forced on (overlap.FORCE_OVERLAP), so the parts of a call
do not depend on a timing probe.  Uses only the package's public calls."""
import argparse, ctypes as C, json, os, subprocess, sys, zlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from foundationpose_amd import _lib, ops, overlap, synthetic as syn
from foundationpose_amd.estimater import FoundationPose, register_objects, register_views
from foundationpose_amd.graphs import GraphedTracker
from foundationpose_amd.mesh import make_can_mesh
from foundationpose_amd.predict_pose_refine import ObjectIndex, PoseRefinePredictor
from foundationpose_amd.predict_score import ScorePredictor
from foundationpose_amd.Utils import get_mesh_handle, make_mesh_tensors
from foundationpose_amd.weights import DEFAULT_REFINE_CFG, DEFAULT_SCORE_CFG, random_state_dict, trained_refiner_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/launch_trace.json")
ap.add_argument("--commit", default=None, help="the commit to name in the header (default: git rev-parse HEAD)")
args = ap.parse_args()


class Recorder:
    """stands in for the loaded library: forwards every call, records the fp_* ones"""

    def __init__(self, lib):
        self.lib, self.table, self.trace = lib, {}, []

    @staticmethod
    def _arg(a, ctype):
        if ctype in (C.c_float, C.c_double):
            return float(a).hex()
        if ctype in (C.c_int, C.c_size_t, C.c_longlong):
            return int(a)
        if a is None or (isinstance(a, C.c_void_p) and not a.value) or (isinstance(a, int) and a == 0):
            return "null"
        return "ptr"

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("fp_"):
            return fn
        types = _lib.SIGNATURES[name][1]

        def call(*a):
            rec = json.dumps([name] + [self._arg(x, t) for x, t in zip(a, types)])
            self.trace.append(self.table.setdefault(rec, len(self.table)))
            return fn(*a)
        return call


def crc(x):
    if isinstance(x, (list, tuple)):
        return [crc(v) for v in x]
    if x is None:
        return None
    a = x.detach().cpu().contiguous().numpy() if torch.is_tensor(x) else np.ascontiguousarray(x)
    return zlib.crc32(a.tobytes())


torch.manual_seed(0)
dev = torch.device("cuda:0")
overlap.FORCE_OVERLAP = True
H, W = syn.H, syn.W
sc = bench.build_scene(dev, 0, 64)
K0 = sc["K"]
K1 = K0.copy()
K1[0, 0] *= 0.94
K1[1, 2] -= 17.25
Ks = [K0, K1]
rgbs = [sc["rgb"], np.clip(sc["rgb"].astype(np.int16) + 5, 0, 255).astype(np.uint8)]
depths = [sc["depth"], (sc["depth"] + 0.003).astype(np.float32)]
meshes = [sc["mesh"], make_can_mesh(radius=0.034, height=0.09, n_ang=36, n_axial=20, textured=False, seed=1)]
gms = [sc["gm"], make_mesh_tensors(meshes[1], device=dev)]
diams = [sc["diameter"], float(np.linalg.norm(meshes[1].vertices.max(0) - meshes[1].vertices.min(0)))]
refiner = PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), state_dict=trained_refiner_state_dict(), device=dev, precision="fp16", graph=False)
scorer = ScorePredictor(cfg=dict(DEFAULT_SCORE_CFG), state_dict=random_state_dict("score", seed=0), device=dev, graph=False)
refiner.plan(), scorer.plan()
header = dict(commit=args.commit or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None,
              side_streams_overlap=bool(overlap.side_streams_overlap(dev, 1)), parts={})

_lib.lib()
rec = _lib._lib = Recorder(_lib._lib)
scenarios = {}


def scenario(name, n_rows, fn):
    """run fn() -> tensors; record its calls and the CRCs of what it returned"""
    rec.trace = []
    with torch.inference_mode():
        out = fn()
        torch.cuda.synchronize()
    header["parts"][name] = len(refiner.sub.parts(n_rows, dev))
    scenarios[name] = dict(crc=crc(out), trace=rec.trace)
    print(f"{name}: {len(rec.trace)} calls", file=sys.stderr, flush=True)


def perturbed(n, seed):
    return syn.perturbed_poses(sc["T"], n, seed=seed).astype(np.float32)


rgb_t = torch.as_tensor(sc["rgb"], device=dev).float().contiguous()
depth_t = torch.as_tensor(sc["depth"], device=dev)
xyz_t = ops.ingest_frame(depth_t, K0)
rgb_st = torch.stack([torch.as_tensor(r, device=dev).float() for r in rgbs]).contiguous()
depth_st = torch.stack([torch.as_tensor(d, device=dev) for d in depths]).contiguous()
mset = ops.MeshSet([get_mesh_handle(g) for g in gms])
dtab = ops.object_diameters(diams, dev)


def refine(P, **kw):
    pose, _ = refiner.predict(sc["rgb"], None, K0, P, xyz_t, mesh=sc["mesh"], mesh_tensors=sc["gm"], mesh_diameter=sc["diameter"],
                              iteration=2, graph=False, **kw)
    return pose, refiner.last_trans_update, refiner.last_rot_update


def score(P):
    return scorer.predict(sc["rgb"], sc["depth"], K0, P, mesh=sc["mesh"], mesh_tensors=sc["gm"], mesh_diameter=sc["diameter"], graph=False)[0]


# 1-3: the single-object predictors
for n in (1, 2, 5):
    scenario(f"refine_n{n}", n, lambda: refine(perturbed(n, 10 + n)))
scenario("refine_n64_shared", 64, lambda: refine(sc["poses"][:64], shared_translation=True))
for n in (5, 64):
    scenario(f"score_n{n}", n, lambda: score(perturbed(n, 20 + n)))

# 4: several objects, object 1 with exactly two rows (the quirk inside a multi-object call)
obj6 = [0, 1, 0, 0, 1, 0]
scenario("refine_device_objects", 6, lambda: refiner.refine_device(
    rgb_t, xyz_t, torch.as_tensor(perturbed(6, 31), device=dev), K0, H, W, mset, dtab, 2, obj=ObjectIndex(obj6, dev)))

# 5: 2 views x 2 objects, one translation per (view, object) segment
lengths, seg_view, seg_obj = [3, 2, 4, 1], [0, 0, 1, 1], [0, 1, 0, 1]
hyp_view, hyp_obj = np.repeat(seg_view, lengths), np.repeat(seg_obj, lengths)
P10 = sc["poses"][:10].copy()
for k, (a, b) in enumerate(zip(np.cumsum([0] + lengths[:-1]), np.cumsum(lengths))):
    P10[a:b, :3, 3] += np.float32(0.002 * k)
vt10 = ops.Views(Ks, hyp_view, dev)
xyz_st = ops.ingest_frames(depth_st, vt10, f64_internal=False)
scenario("refine_device_views_segments", 10, lambda: refiner.refine_device(
    rgb_st, xyz_st, torch.as_tensor(P10, device=dev), None, H, W, mset, dtab, 2, shared_translation=ops.Segments(lengths, dev),
    obj=ObjectIndex(hyp_obj, dev, view=hyp_view), views=vt10))

# 6: the scorer over several objects, then over several views
P7 = perturbed(7, 41)
scenario("predict_objects", 7, lambda: scorer.predict_objects(sc["rgb"], depth_t, K0, P7, mset, dtab, ops.Segments([3, 4], dev)))
scenario("predict_objects_views", 7, lambda: scorer.predict_objects(
    rgbs, depths, None, P7, mset, dtab, ops.Segments([3, 4], dev), views=ops.Views(Ks, [0, 1, 1, 1, 0, 0, 1], dev)))

# 7: the tracker, eager and captured
trackers = dict(
    single=(lambda: GraphedTracker(refiner, sc["gm"], sc["diameter"], K0, H, W, n_hyp=1, iteration=2, agreement_tol=0.01),
            sc["rgb"], sc["depth"], 1),
    objects=(lambda: GraphedTracker(refiner, gms, diams, K0, H, W, n_hyp=2, iteration=2, agreement_tol=0.01), sc["rgb"], sc["depth"], 4),
    views=(lambda: GraphedTracker(refiner, gms, diams, Ks, H, W, n_hyp=1, iteration=2, views=[0, 1], agreement_tol=0.01), rgbs, depths, 2))
for name, (make, rgb, depth, n) in trackers.items():
    def eager():
        trk = make()
        return trk.step_eager(rgb, depth, perturbed(n, 50 + n)), trk.agreement
    scenario(f"tracker_{name}_eager", n, eager)


def captured():
    trk = trackers["single"][0]()
    return trk.step(sc["rgb"], sc["depth"], perturbed(1, 51)), trk.agreement


scenario("tracker_single_captured", 1, captured)

# 8: the batched registrations
ests = [FoundationPose(model_pts=m.vertices, model_normals=m.vertex_normals, mesh=m, scorer=scorer, refiner=refiner, device=dev) for m in meshes]


def registered(poses):
    return [np.asarray(p, dtype=np.float64) for p in poses] + [e.poses for e in ests] + [e.scores for e in ests]


n_reg = 2 * int(ests[0].rot_grid.shape[0])
scenario("register_objects", n_reg, lambda: registered(register_objects(ests, K0, sc["rgb"], sc["depth"], [sc["mask"]] * 2, iteration=1)))
scenario("register_views", n_reg, lambda: registered(register_views(ests, [0, 1], rgbs, depths, Ks, [sc["mask"]] * 2, iteration=1)))

calls = [None] * len(rec.table)
for text, i in rec.table.items():
    calls[i] = json.loads(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(dict(header=header, scenarios=scenarios, calls=calls), f, separators=(",", ":"))
    f.write("\n")
print(json.dumps(dict(out=args.out, scenarios=len(scenarios), calls=sum(len(s["trace"]) for s in scenarios.values()), distinct=len(calls))))
