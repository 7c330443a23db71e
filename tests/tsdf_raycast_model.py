"""numpy restatement of fp_tsdf_raycast (include/fp_amd.h has the definition): every value is a float32 array operation, one rounding
each, in the order the header writes; vectorised over the pixels of a row, a Python loop over the march's samples.  The `wrong` switches
restate the definition with one deliberate mistake each, for the tests that show the checks can tell:
  centre         the pixel centre at the integer instead of + 0.5
  gt             a hit needs f_prev > 0 instead of >= 0
  no_reset       an unknown sample does not forget the previous one
  backface_hit   a first known sample below 0 is reported as a hit (at its own z)
  no_interp      z* is the current sample's z, without the interpolation
  normal_object  the normal is left in the object frame
  weight_gt      a corner counts with weight > min_weight instead of >=
`stats` receives how many pixels took each way through the definition; generated_case builds the volumes, poses and windows that reach
all of them (CASES: the list the CPU coverage test and the GPU bit-equality test share).  Test infrastructure only."""
import numpy as np

import tsdf_model as tm

f32 = np.float32
WRONG = ("centre", "gt", "no_reset", "backface_hit", "no_interp", "normal_object", "weight_gt")
MAX_SAMPLES = 65536
NO_Z_FAR = np.finfo(f32).max
BRANCHES = ("hit", "miss_box", "zero_dir_inside", "zero_dir_outside", "camera_inside", "backface", "gap", "f_cur_zero", "f_prev_zero_hit",
            "hit_last_cell", "ran_out", "window_outside", "crop_1x1", "dim1", "bad_pose", "bad_view", "color_none", "color_some")


def _lerp(a, b, t):
    return a + t * (b - a)


def _trilinear(v, fx, fy, fz):
    """v[dx + 2 dy + 4 dz]: along x, then y, then z"""
    return _lerp(_lerp(_lerp(v[0], v[1], fx), _lerp(v[2], v[3], fx), fy), _lerp(_lerp(v[4], v[5], fx), _lerp(v[6], v[7], fx), fy), fz)


def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def _corners(base, sy, sz):
    return [base + (q & 1) + (q >> 1 & 1) * sy + (q >> 2) * sz for q in range(8)]


def raycast(vol, poses, K, H, W, out_hw=None, bbox2d=None, step=None, min_weight=1.0, z_near=0.001, z_far=None, view=None, wrong=None,
            stats=None):
    """vol: tsdf_model.Volume; poses (N,4,4); K (3,3), or (V,3,3) with view (N,) (indices outside 0..V-1 allowed: all misses)
    -> dict(depth (N,oh,ow), xyz, normal, color (N,oh,ow,3)) float32"""
    poses = np.asarray(poses, f32).reshape(-1, 16)
    N = len(poses)
    oh, ow = (H, W) if out_hw is None else out_hw
    if bbox2d is None:
        assert (oh, ow) == (H, W)
    K = np.asarray(K, np.float64)
    step = vol.voxel if step is None else f32(step)
    zf = NO_Z_FAR if z_far is None else f32(z_far)
    st = stats if stats is not None else {}
    for k in BRANCHES:
        st.setdefault(k, 0)
    if (oh, ow) == (1, 1):
        st["crop_1x1"] += N
    out = dict(depth=np.zeros((N, oh, ow), f32), xyz=np.zeros((N, oh, ow, 3), f32), normal=np.zeros((N, oh, ow, 3), f32),
               color=np.zeros((N, oh, ow, 3), f32))
    for n in range(N):
        Kn = K
        if K.ndim == 3:
            v = 0 if view is None else int(view[n])
            if not 0 <= v < len(K):
                st["bad_view"] += 1
                continue
            Kn = K[v]
        window = (f32(0), f32(0), f32(W), f32(H)) if bbox2d is None else tuple(np.asarray(bbox2d, f32)[n])
        with np.errstate(all="ignore"):
            d, x, m, c = _row(vol, poses[n], Kn.astype(f32), window, W, H, oh, ow, step, f32(min_weight), f32(z_near), zf, wrong, st)
        out["depth"][n], out["xyz"][n], out["normal"][n], out["color"][n] = d, x, m, c
    return out


def _row(vol, T, K, window, W, H, oh, ow, step, min_weight, z_near, z_far, wrong, st):
    nz, ny, nx = vol.dims
    dims = (nx, ny, nz)
    npx = oh * ow
    depth, xyz, nrm, col = np.zeros(npx, f32), np.zeros((npx, 3), f32), np.zeros((npx, 3), f32), np.zeros((npx, 3), f32)
    shaped = lambda: (depth.reshape(oh, ow), xyz.reshape(oh, ow, 3), nrm.reshape(oh, ow, 3), col.reshape(oh, ow, 3))   # noqa: E731
    fx, skew, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    if min(dims) < 2:
        st["dim1"] += 1
        return shaped()
    if not (np.isfinite(T).all() and np.isfinite([fx, fy, cx, cy]).all() and skew == 0):
        st["bad_pose"] += 1
        return shaped()
    umin, vmin, umax, vmax = window
    ax, ay = f32(ow) / (umax - umin), f32(oh) / (vmax - vmin)
    o = [-_dot3(T[k], T[3], T[4 + k], T[7], T[8 + k], T[11]) for k in range(3)]
    half = f32(0) if wrong == "centre" else f32(0.5)
    u = umin + (np.arange(ow, dtype=f32) + half) / ax
    v = vmin + (np.arange(oh, dtype=f32) + half) / ay
    st["window_outside"] += int((u < 0).sum() + (u > f32(W)).sum() + (v < 0).sum() + (v > f32(H)).sum())
    dcx = np.broadcast_to(((u - cx) / fx)[None, :], (oh, ow)).reshape(-1)
    dcy = np.broadcast_to(((v - cy) / fy)[:, None], (oh, ow)).reshape(-1)
    d = [(T[k] * dcx + T[4 + k] * dcy) + T[8 + k] for k in range(3)]
    s, lo = vol.voxel, vol.origin
    # clipping
    live = np.ones(npx, bool)
    z0, z1 = np.full(npx, z_near, f32), np.full(npx, z_far, f32)
    inside_box = np.ones(npx, bool)
    for a in range(3):
        hi = lo[a] + f32(dims[a] - 1) * s
        zero = d[a] == 0
        within = bool(o[a] >= lo[a] and o[a] <= hi)
        inside_box &= within
        st["zero_dir_inside"] += int(zero.sum()) if within else 0
        st["zero_dir_outside"] += 0 if within else int(zero.sum())
        live &= ~zero | within
        t1, t2 = (lo[a] - o[a]) / d[a], (hi - o[a]) / d[a]
        less = t1 < t2
        tmin, tmax = np.where(less, t1, t2), np.where(less, t2, t1)
        z0 = np.where(~zero & (tmin > z0), tmin, z0)
        z1 = np.where(~zero & (tmax < z1), tmax, z1)
    live &= z0 <= z1
    st["miss_box"] += int((~live).sum())
    st["camera_inside"] += int(live.sum()) if inside_box.all() else 0
    # march
    sy, sz = nx, nx * ny
    alive = live.copy()
    have_prev = np.zeros(npx, bool)
    f_prev, z_prev, zs = np.zeros(npx, f32), np.zeros(npx, f32), np.zeros(npx, f32)
    hit = np.zeros(npx, bool)
    was_known, gap_open = np.zeros(npx, bool), np.zeros(npx, bool)
    for k in range(MAX_SAMPLES):
        z = z0 + f32(k) * step
        ended = alive & ~(z <= z1)
        st["ran_out"] += int((ended & have_prev & (z1 == z_far) & (z_far != NO_Z_FAR)).sum())
        alive = alive & (z <= z1)
        idx = np.nonzero(alive)[0]
        if not len(idx):
            break
        zi = z[idx]
        inside = np.ones(len(idx), bool)
        c, fr = [], []
        for a in range(3):
            q = ((o[a] + zi * d[a][idx]) - lo[a]) / s
            ca = np.floor(q)
            c.append(ca)
            fr.append(q - ca)
            inside &= (ca >= 0) & (ca <= f32(dims[a] - 2))
        ci = [np.where(inside, ca, 0).astype(np.int64) for ca in c]
        base = ci[2] * sz + ci[1] * sy + ci[0]
        at = _corners(base, sy, sz)
        known = inside.copy()
        for q in range(8):
            w = vol.weight[at[q]]
            known &= (w > min_weight) if wrong == "weight_gt" else (w >= min_weight)
        f = _trilinear([vol.tsdf[a_] for a_ in at], fr[0], fr[1], fr[2])
        # bookkeeping of the branches only
        st["gap"] += int((known & gap_open[idx]).sum())
        gap_open[idx] = np.where(known, False, gap_open[idx] | was_known[idx])
        was_known[idx] |= known
        st["f_cur_zero"] += int((known & (f == 0)).sum())
        hp = have_prev[idx]
        neg = known & (f < 0)
        back = neg & ~hp
        st["backface"] += int(back.sum())
        h = neg & hp
        if wrong == "gt":
            h &= f_prev[idx] > 0
        st["f_prev_zero_hit"] += int((h & (f_prev[idx] == 0)).sum())
        zhit = z_prev[idx] + step * (f_prev[idx] / (f_prev[idx] - f))
        if wrong == "no_interp":
            zhit = zi
        if wrong == "backface_hit":
            h = neg
            zhit = np.where(back, zi, zhit)
        hit[idx[h]] = True
        zs[idx[h]] = zhit[h]
        alive[idx[neg]] = False
        pos = known & ~neg
        have_prev[idx[pos]] = True
        f_prev[idx[pos]] = f[pos]
        z_prev[idx[pos]] = zi[pos]
        if wrong != "no_reset":
            have_prev[idx[~known]] = False
    # outputs
    st["hit"] += int(hit.sum())
    idx = np.nonzero(hit)[0]
    if len(idx):
        zh = zs[idx]
        depth[idx] = zh
        xyz[idx, 0], xyz[idx, 1], xyz[idx, 2] = zh * dcx[idx], zh * dcy[idx], zh
        ci, fr = [], []
        for a in range(3):
            q = ((o[a] + zh * d[a][idx]) - lo[a]) / s
            cf = np.floor(q)
            cf = np.where(cf >= 0, cf, f32(0))
            cf = np.where(cf <= f32(dims[a] - 2), cf, f32(dims[a] - 2)).astype(f32)
            ci.append(cf.astype(np.int64))
            fr.append(q - cf)
        st["hit_last_cell"] += int(((ci[0] == nx - 2) & (ci[1] == ny - 2) & (ci[2] == nz - 2)).sum())
        base = ci[2] * sz + ci[1] * sy + ci[0]
        at = _corners(base, sy, sz)
        g = tm._gradient(vol)
        gi = [_trilinear([g[a_, comp] for a_ in at], fr[0], fr[1], fr[2]) for comp in range(3)]
        ln = np.sqrt((gi[0] * gi[0] + gi[1] * gi[1]) + gi[2] * gi[2])
        m = [gi[k] / ln for k in range(3)]
        for k in range(3):
            rot = m[k] if wrong == "normal_object" else _dot3(T[4 * k], m[0], T[4 * k + 1], m[1], T[4 * k + 2], m[2])
            nrm[idx, k] = np.where(ln > 0, rot, f32(0))
        acc, accw = np.zeros((len(idx), 3), f32), np.zeros(len(idx), f32)
        one = f32(1)
        for q in range(8):
            dx, dy, dz = q & 1, q >> 1 & 1, q >> 2
            w = ((fr[0] if dx else one - fr[0]) * (fr[1] if dy else one - fr[1])) * (fr[2] if dz else one - fr[2])
            has = vol.color_weight[at[q]] > 0
            acc = np.where(has[:, None], acc + w[:, None] * vol.color[at[q]], acc)
            accw = np.where(has, accw + w, accw)
        some = accw > 0
        st["color_none"] += int((~some).sum())
        st["color_some"] += int(some.sum())
        col[idx] = np.where(some[:, None], acc / accw[:, None], f32(128))
    return shaped()


# ------------------------------------------------------------------ generated cases
S = f32(2.0 ** -6)          # the pitch of the generated volumes: dyadic, so the axis-parallel rays land exactly on lattice points


def _rot(axis, deg):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    a = np.deg2rad(deg)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def plane_volume(dims, seed=0, last=False):
    """tsdf falls along z through 0 on the lattice plane iz = zp (exactly 0 on the line ix = nx // 2, iy = ny // 2 of it; tilted a
    little elsewhere), every voxel observed once except two gaps: the plane iz = 1 where ix < nx // 2 - 1 (a gap well before the
    surface) and the planes iz = zp, zp + 1 where ix > nx // 2 + 1 (a gap that swallows the crossing).  Colours are random, a quarter of
    the voxels without one and none in the block ix < nx // 2, iy < ny // 2.  last=True: the crossing lies in the last layer of cells
    instead (at iz = nz - 1.75), without tilt or gaps."""
    rng = np.random.default_rng(seed + 100)
    nz, ny, nx = dims
    vol = tm.Volume(dims, [-(nx // 2) * float(S), -(ny // 2) * float(S), -float(S)], S, 4 * S)
    ix, iy, iz = vol.coords()
    zp = nz // 2 if nz >= 3 else 0.5
    vol.tsdf[:] = (0.25 * (zp - iz) + 0.0625 * (ix - nx // 2) + 0.03125 * (iy - ny // 2)).astype(f32)
    vol.weight[:] = 1
    if last:
        vol.tsdf[:] = (0.25 * ((nz - 1.75) - iz)).astype(f32)
    elif nz >= 5:
        vol.weight[(iz == 1) & (ix < nx // 2 - 1)] = 0
        vol.weight[((iz == zp) | (iz == zp + 1)) & (ix > nx // 2 + 1)] = 0
    vol.color[:] = rng.uniform(0, 255, vol.color.shape).astype(f32)
    vol.color_weight[:] = rng.integers(0, 4, vol.color_weight.shape).astype(f32)
    vol.color_weight[(ix < nx // 2) & (iy < ny // 2)] = 0
    return vol


def random_volume(dims, seed=0):
    """a noisy sphere-like field about the middle of the volume, 4 % of the voxels unobserved, weights 1..3"""
    rng = np.random.default_rng(seed + 200)
    nz, ny, nx = dims
    vol = tm.Volume(dims, [-(nx - 1) * float(S) / 2 + 0.003, -(ny - 1) * float(S) / 2 - 0.002, -(nz - 1) * float(S) / 2 + 0.001], S, 4 * S)
    ix, iy, iz = vol.coords()
    r = np.sqrt((ix - (nx - 1) / 2) ** 2 + (iy - (ny - 1) / 2) ** 2 + (iz - (nz - 1) / 2) ** 2)
    vol.tsdf[:] = np.clip((r - 0.3 * max(dims)) / 4 + rng.normal(0, 0.08, r.shape), -1, 1).astype(f32)
    vol.weight[:] = rng.integers(1, 4, r.shape).astype(f32)
    vol.weight[rng.random(r.shape) < 0.04] = 0
    vol.color[:] = rng.uniform(0, 255, vol.color.shape).astype(f32)
    vol.color_weight[:] = np.where(rng.random(r.shape) < 0.5, vol.weight, 0).astype(f32)
    return vol


def generated_case(kind, dims, N, oh, ow, V=1, full_frame=False, seed=0, z_far=None):
    """kind 'plane' (and 'last': plane_volume(last=True)): plane_volume seen by cameras on the z axis -- row types in turn: (0) straight down the axis from outside (the
    middle pixel's ray has dc = (0, 0, 1): two direction components exactly 0, lattice points hit exactly), (1) the same camera
    shifted sideways past the box (the zero component outside its slab), (2) turned half round: looking at the surface from behind,
    (3) the camera inside the box, (4) a NaN in the pose, (5) a tilted view from far to the side (most rays miss the box).
    kind 'random': random_volume under random rotations, at a distance or inside.  Windows: full frame (oh x ow is then the frame), or a
    window of two frame pixels per crop pixel around the principal point, every third one shifted half out of the frame.  V > 1: the
    view table with one index above and (N >= 3) one below the table.  -> dict"""
    rng = np.random.default_rng(seed)
    nz, ny, nx = dims
    vol = random_volume(dims, seed) if kind == "random" else plane_volume(dims, seed, last=kind == "last")
    H, W = (oh, ow) if full_frame else (2 * oh + 6, 2 * ow + 10)
    i0, j0 = ow // 2, oh // 2
    Ks = np.zeros((V, 3, 3))
    for v in range(V):
        f = 8.0 * max(oh, ow) * (1.0 + 0.25 * v)
        cxy = (i0 + 0.5, j0 + 0.5) if full_frame else (W // 2 + 0.5, H // 2 + 0.5)
        Ks[v] = [[f, 0, cxy[0]], [0, f * (1.0 if v == 0 else 1.125), cxy[1]], [0, 0, 1]]
    view = (np.arange(N) % V).astype(np.int32)
    if V > 1:
        view[N - 1] = V
        if N >= 3:
            view[1] = -1
    poses = np.tile(np.eye(4, dtype=f32), (N, 1, 1))
    s = float(S)
    for n in range(N):
        if kind != "random":
            t = n % 6
            if t == 0:
                poses[n, 2, 3] = 0.25
            elif t == 1:
                poses[n, :3, 3] = (-(nx + 2) * s, 0, 0.25)
            elif t == 2:
                poses[n, :3, :3] = _rot((1, 0, 0), 180).round()
                poses[n, 2, 3] = 0.25 + nz * s
            elif t == 3:
                poses[n, 2, 3] = -0.5 * s if nz > 2 else 0.25 * s      # o = (0, 0, s / 2): inside the box
            elif t == 4:
                poses[n, 2, 3] = 0.25
                poses[n, 1, 2] = np.nan
            else:
                poses[n, :3, :3] = _rot((0.2, 1, 0.1), 35)
                poses[n, :3, 3] = (0.02, -0.01, 0.3)
        else:
            axis = rng.normal(size=3)
            poses[n, :3, :3] = _rot(axis, rng.uniform(0, 180))
            poses[n, :3, 3] = (rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), 0.0 if n % 4 == 3 else rng.uniform(0.2, 0.4))
    bbox = None
    if not full_frame:
        bbox = np.zeros((N, 4), f32)
        for n in range(N):
            cx, cy = Ks[max(min(int(view[n]), V - 1), 0), 0, 2], Ks[max(min(int(view[n]), V - 1), 0), 1, 2]
            u0, v0 = cx - (i0 + 0.5) * 2, cy - (j0 + 0.5) * 2
            if n % 3 == 2:
                u0, v0 = u0 - ow, v0 + oh * 0.75
            bbox[n] = (u0, v0, u0 + 2 * ow, v0 + 2 * oh)
    return dict(vol=vol, poses=poses, K=Ks if V > 1 else Ks[0], view=view if V > 1 else None, V=V, bbox2d=bbox, H=H, W=W, out_hw=(oh, ow),
                step=f32(0.7) * S if kind == "random" else f32(0.5) * S, min_weight=1.0, z_near=0.001, z_far=z_far)


# (kind, dims (nz, ny, nx), N, oh, ow, V, full_frame, z_far): volumes 2x2x2, 3x4x5, 17x17x17, 33x20x9 and 1x5x5; crops 1x1, 7x5, 9x64,
# 64x64 and one 160x160; N 1 / 3 / 17; V 1 / 3 with indices outside the table; one camera and the view table; windows and full frame
CASES = {
    "plane_17_64x64_N17": ("plane", (17, 17, 17), 17, 64, 64, 1, False, None),
    "plane_17_7x5_N17_V3": ("plane", (17, 17, 17), 17, 7, 5, 3, False, None),
    "plane_17_fullframe_9x64_N3": ("plane", (17, 17, 17), 3, 9, 64, 1, True, None),
    "plane_17_zfar_64x64_N1": ("plane", (17, 17, 17), 1, 64, 64, 1, False, 0.25 + 6.5 * float(S)),
    "plane_33x20x9_64x64_N3_V3": ("plane", (33, 20, 9), 3, 64, 64, 3, False, None),
    "last_17_64x64_N1": ("last", (17, 17, 17), 1, 64, 64, 1, False, None),
    "last_3x4x5_9x64_N3": ("last", (3, 4, 5), 3, 9, 64, 1, False, None),
    "plane_3x4x5_7x5_N17": ("plane", (3, 4, 5), 17, 7, 5, 1, False, None),
    "plane_2_1x1_N3": ("plane", (2, 2, 2), 3, 1, 1, 1, False, None),
    "plane_2_fullframe_7x5_N1_V1table": ("plane", (2, 2, 2), 1, 7, 5, 1, True, None),
    "plane_1x5x5_7x5_N3": ("plane", (1, 5, 5), 3, 7, 5, 1, False, None),
    "random_17_160x160_N3": ("random", (17, 17, 17), 3, 160, 160, 1, False, None),
    "random_33x20x9_9x64_N17_V3": ("random", (33, 20, 9), 17, 9, 64, 3, False, None),
    "random_3x4x5_fullframe_64x64_N3_V3": ("random", (3, 4, 5), 3, 64, 64, 3, True, None),
    "random_17_zfar_7x5_N17": ("random", (17, 17, 17), 17, 7, 5, 1, False, 0.3),
}
TABLE_FOR_ONE_VIEW = ("plane_2_fullframe_7x5_N1_V1table",)      # V == 1 through the view table, without an index


def named_case(name):
    kind, dims, N, oh, ow, V, full, z_far = CASES[name]
    return generated_case(kind, dims, N, oh, ow, V, full, seed=sum(map(ord, name)), z_far=z_far)


def run_case(c, wrong=None, stats=None):
    return raycast(c["vol"], c["poses"], c["K"], c["H"], c["W"], c["out_hw"], c["bbox2d"], c["step"], c["min_weight"], c["z_near"], c["z_far"],
                   c["view"], wrong, stats)


def branches_reached(c):
    """-> dict branch -> pixels (or rows) of the case that took it"""
    st = {}
    run_case(c, stats=st)
    return st


def bits_equal(a, b):
    """same float32 bits, any NaN equal to any NaN"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------ aligning views to a volume on the CPU
def box_diameter(vol):
    """twice the radius of the sphere about the frame's origin that holds the volume's box (reconstruct._AlignSide)"""
    nz, ny, nx = vol.dims
    lo = vol.origin.astype(np.float64)
    hi = lo + (np.asarray([nx, ny, nz], np.float64) - 1.0) * float(vol.voxel)
    return 2.0 * float(np.linalg.norm(np.maximum(np.abs(lo), np.abs(hi))))


def align_views_model(vol, views, poses, H, W, iterations=3, max_dist=0.01, which=None):
    """reconstruct.align_views_to_volume with the CPU oracle's crop windows, this restatement's raycast and icp_model's step: every
    view (or the views `which`) against its own masked, unfiltered depth -> (poses (n,4,4) float32, [status of the last step],
    [a step had a non-zero status])"""
    import icp_model as im
    from oracle import ops as oo
    diam = box_diameter(vol)
    oh, ow = im.CROP
    out, status, bad = [], [], []
    for v in (range(len(poses)) if which is None else which):
        d = np.where(views["masks"][v] != 0, views["depth"][v], f32(0)).astype(f32)
        K = views["Ks"][v]
        xyz = oo.depth2xyzmap(d, K, f64_internal=False)
        P, failed = np.asarray(poses[v:v + 1], f32), False
        for _ in range(iterations):
            tf, bb = oo.crop_windows(P, K, diam, im.CROP_RATIO, (ow, oh))
            r = raycast(vol, P, K, H, W, (oh, ow), bb)
            system, P = im.step(r["xyz"], r["normal"], xyz, tf, P, max_dist)
            failed = failed or system[0, 29] != 0
        out.append(P[0])
        status.append(int(system[0, 29]))
        bad.append(bool(failed))
    return np.stack(out), status, bad


def integrate_aligned_model(vol, views, poses, H, W, iterations=3, max_dist=0.01, trusted=1):
    """TsdfVolume.integrate_aligned: the first `trusted` views fused as given, every later one aligned to the volume so far and fused
    at the aligned pose; a view with a failed step keeps its pose and is not fused -> the poses used (V,4,4) float32"""
    V = len(poses)
    used = np.asarray(poses, f32).copy()
    sl = slice(0, min(trusted, V))
    tm.integrate(vol, views["depth"][sl], views["rgb"][sl], views["masks"][sl], used[sl], views["Ks"][sl])
    for v in range(min(trusted, V), V):
        P, _, bad = align_views_model(vol, views, used, H, W, iterations, max_dist, which=[v])
        if bad[0]:
            continue
        used[v] = P[0]
        tm.integrate(vol, views["depth"][v:v + 1], views["rgb"][v:v + 1], views["masks"][v:v + 1], used[v:v + 1], views["Ks"][v:v + 1])
    return used
