"""What a light kernel chain of one stream gains, and what the 3x3 convolution of the other pays, when both may be resident on a CU.

  stream A: R back-to-back launches of one stem-shaped convolution (128 -> 128 on 2 x 82 images of 40 x 40: 513 tiles of 512 x 128, two
            for every CU), residual and ReLU as in a ResnetBasicBlock -- long enough to cover stream B's work several times over
  stream B: fp_render_crops + fp_warp_crops of 126 hypotheses on the synthetic can (k_vertex, k_bin, k_raster, k_warp2), started
            once A is under way

HIP events around A and around B, on a common time base.  Printed as one JSON line: B alone, A alone, and both under each other
(medians of --reps rounds, with min / max), plus where B's window lay inside A's.  Run once per library to compare two builds:

    python scripts/conv_coresident_probe.py --tag new                       > new.json
    python scripts/conv_coresident_probe.py --tag parent --tree ../parent   > parent.json      # another checkout with its own library

--tree: import foundationpose_amd and bench from that checkout (the binding refuses a library of another ABI version)."""
import argparse, json, os, sys

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="product")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--convs", type=int, default=60, help="launches of the convolution per round (R)")
ap.add_argument("--hyps", type=int, default=126)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import numpy as np, torch
import bench
from foundationpose_amd import _lib, ops

dev = torch.device("cuda:0")
N, R = args.hyps, args.convs
# ---- stream A's work
Bimg, H, C = 2 * 82, 40, 128
g = torch.Generator(device="cpu").manual_seed(7)
x = torch.zeros((Bimg, H + 2, H + 2, C), dtype=torch.float16)
x[:, 1:-1, 1:-1] = torch.relu(torch.randn((Bimg, H, H, C), generator=g) * 0.5).half()
w = (torch.randn((C, 9 * C), generator=g) * (1.0 / (3 * C ** 0.5))).half().to(dev)
bias = (torch.randn(C, generator=g) * 0.1).to(dev)
r = torch.zeros_like(x)
r[:, 1:-1, 1:-1] = (torch.randn((Bimg, H, H, C), generator=g) * 0.5).half()
x, r = x.to(dev), r.to(dev)
y = torch.zeros_like(x)
gin, gout = ops.IgemmGeom.image(H, H, 1, C, stride=1, offset=0), ops.IgemmGeom.image(H, H, 1, C)
wt = ops.pack_conv3x3_tiles(w, C, C)
M = Bimg * H * H


def run_a():
    for _ in range(R):
        ops.igemm_f16(x, gin, w, bias, y, gout, M, C, C, 9, relu=True, residual=r, r_geom=gout, conv_rounding=True, w_tiles=wt)


# ---- stream B's work
sc = bench.build_scene(dev, 0, N)
gm, K, diam = sc["gm"], sc["K"], sc["diameter"]
P = torch.as_tensor(sc["poses"], device=dev)
rgb = torch.as_tensor(sc["rgb"], device=dev).float().contiguous()
depth = ops.bilateral_filter_depth(ops.erode_depth(torch.as_tensor(sc["depth"], device=dev)))
xyz = ops.depth_to_xyz(depth, K, f64_internal=True)
tf, bb = ops.crop_windows(P, K, diam, 1.2, (160, 160))
Hf, Wf = int(rgb.shape[0]), int(rgb.shape[1])
ws = torch.empty(ops.workspace_bytes(N, int(gm["pos"].shape[0]), int(gm["faces"].shape[0])), dtype=torch.uint8, device=dev)
A_out = torch.zeros((N, 6, 160, 160), dtype=torch.float16, device=dev)
B_out = torch.zeros((N, 6, 160, 160), dtype=torch.float16, device=dev)


def run_b():
    ops.render_crops(gm["_handle"], P, bb, K, Hf, Wf, (160, 160), diam, 0.001, True, want=("A",), A_out=A_out, workspace=ws)
    ops.warp_crops(rgb, xyz, None, tf, K, P, diam, ops.MODE_REFINE, normalize_xyz=True, out_hw=(160, 160), B_out=B_out)


sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
ev = lambda: torch.cuda.Event(enable_timing=True)


def round_(a, b):
    """one round: A and / or B, each between two events of its stream; -> ms relative to the first event"""
    e = [ev() for _ in range(4)]
    torch.cuda.synchronize()
    if a:
        with torch.cuda.stream(sa):
            e[0].record(); run_a(); e[1].record()
    if b:
        with torch.cuda.stream(sb):
            if a:
                sb.wait_event(e[0])            # not before A has begun
            e[2].record(); run_b(); e[3].record()
    torch.cuda.synchronize()
    t0 = e[0] if a else e[2]
    out = {}
    if a:
        out["A_ms"] = e[0].elapsed_time(e[1])
    if b:
        out["B_ms"] = e[2].elapsed_time(e[3])
        out["B_begin_ms"], out["B_end_ms"] = t0.elapsed_time(e[2]), t0.elapsed_time(e[3])
    return out


def stat(rows, key):
    v = sorted(rw[key] for rw in rows)
    return dict(median=round(float(np.median(v)), 4), min=round(v[0], 4), max=round(v[-1], 4))


for _ in range(2):
    round_(True, True)                       # warm-up: code objects, scratch, clocks
alone_a, alone_b, both = [], [], []
for _ in range(args.reps):                   # the three arrangements alternate
    alone_b.append(round_(False, True))
    alone_a.append(round_(True, False))
    both.append(round_(True, True))
res = dict(tag=args.tag, lib=os.path.realpath(_lib.LIB_PATH), abi=_lib.lib().fp_version(), hyps=N, convs_per_round=R, conv_tiles=-(-M // 512), reps=args.reps,
           B_alone_ms=stat(alone_b, "B_ms"), A_alone_ms=stat(alone_a, "A_ms"), A_alone_us_per_conv=round(stat(alone_a, "A_ms")["median"] / R * 1e3, 2),
           B_under_A_ms=stat(both, "B_ms"), A_under_B_ms=stat(both, "A_ms"),
           B_window_in_A_ms=[stat(both, "B_begin_ms")["median"], stat(both, "B_end_ms")["median"]])
res["A_pays_ms"] = round(res["A_under_B_ms"]["median"] - res["A_alone_ms"]["median"], 4)
res["B_pays_ms"] = round(res["B_under_A_ms"]["median"] - res["B_alone_ms"]["median"], 4)
print("COPROBE " + json.dumps(res), flush=True)
