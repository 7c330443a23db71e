"""Generated inputs for fp_pose_update in its three forms (k_pose_update of csrc/frame_ops.hip), in the style of
tests/geometry_cases.py: sizes around the 64-thread block, rotations at the clamp of so3_exp_map, at saturated tanh and next to pi,
degenerate 6d pairs, 'deepim' windows and intrinsics the scene never has, object and view indices outside their tables.  Seeded, numpy
only.  cases(scene) returns a list of named records (plain dicts); every record carries its inputs, `targets` (what it is there
for), `tags` (tag -> the rows that carry that edge; tests/test_pose_update_cases_host.py checks that each tagged row really is where
it claims to be), `degenerate` (rows on which the float32 result is not determined: the error bound of tests/pose_update_model.py
says nothing there) and `nan_rows` (rows the header promises as NaN).  Test infrastructure only; not a conftest.

Which rows are degenerate is decided here, by construction, and the host test requires the bound to agree:
  * 6d pairs with a2 parallel to a1 (a2 = 3 a1, a2 = a1 + 1e-7 noise): u2 = a2 - (b1 . a2) b1 is rounding noise, its direction free;
  * 'deepim' rows with tz = 0 (a division by zero), with a window or a translation that is not finite (collapsed windows:
    tests/geometry_cases.py), and the 0.17 m object at 5 000 m whose window is one pixel wide (the rounding of a pixel coordinate
    alone is 2e-3 of its lateral translation); tz of -1, 1e-30 and 1e-6 are determined and are compared;
  * rows with a non-finite input (the non-finite cases).
No axis-angle rotation is degenerate: so3_exp_map's clamp keeps 1 / th finite, and next to pi the matrix is well conditioned."""
import functools

import numpy as np

import geometry_cases as gc
import pose_update_model as pm

F = np.float32
SIZES = (0, 1, 63, 64, 65, 257)
ROT_NORMALIZERS = (0.349, 1.0, float(np.pi / np.sqrt(3.0)), 0.0)
EPS2 = F(1e-4)
TN = (0.02, 0.02, 0.05)


# -------------------------------------------------------------------------------------------------------- input poses
def _signed_permutations():
    out = []
    for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)):
        for s in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            R = np.zeros((3, 3))
            R[0, perm[0]], R[1, perm[1]] = s[0], s[1]
            R[2, perm[2]] = 1.0
            R[2, perm[2]] = np.linalg.det(R)          # proper rotations only
            out.append(R)
    return out


def input_poses(N, scene, seed):
    """row k cycles through: identity at the origin, a pose of the scene, a rotation whose entries are exactly +-1 at 1e-3 m, a pose
    of the scene's grid at 50 m"""
    rng = np.random.default_rng(seed)
    sp = _signed_permutations()
    P = np.tile(np.eye(4, dtype=F), (N, 1, 1))
    for k in range(N):
        kind = k % 4
        if kind == 1:
            P[k] = scene["poses"][(7 * k) % len(scene["poses"])]
        elif kind == 2:
            P[k, :3, :3] = sp[(k // 4) % len(sp)]
            P[k, :3, 3] = (rng.uniform(-1, 1, 3) * 1e-3).astype(F)
        elif kind == 3:
            P[k] = scene["poses"][(11 * k) % len(scene["poses"])]
            P[k, :3, 3] = (np.array([3.0, -2.0, 50.0]) + rng.uniform(-1, 1, 3)).astype(F)
    return P


# ---------------------------------------------------------------------------------------------------- axis-angle rows
def _n2(rot, rn):
    """|w|^2 as the kernel forms it (float32; tanh through float64, rounded once)"""
    s = pm.Single()
    rot = np.asarray(rot, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        w = [s.tanh(rot[:, k]) * F(rn) for k in range(3)]
        return (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]


@functools.lru_cache(maxsize=None)
def clamp_rows(rn):
    """three raw rotations whose |w|^2 is one float32 step below 1e-4f, exactly 1e-4f, and one step above (found by walking the
    second component through consecutive floats: |w|^2 moves by a small fraction of its spacing per step)"""
    targets = (np.nextafter(EPS2, F(0)), EPS2, np.nextafter(EPS2, F(1)))
    r0, r2 = F(0.0085 / rn), F(0.0031 / rn)
    w0 = np.float64(np.tanh(np.float64(r0)) * rn) ** 2 + np.float64(np.tanh(np.float64(r2)) * rn) ** 2
    r1 = F(np.arctanh(np.sqrt(1e-4 - w0) / rn))
    cand = r1.view(np.uint32) + np.arange(-20000, 20001, dtype=np.int64)
    cand = cand.astype(np.uint32).view(F)
    rot = np.stack([np.full(len(cand), r0, F), cand, np.full(len(cand), r2, F)], 1)
    n2 = _n2(rot, rn)
    rows = []
    for t in targets:
        hit = np.flatnonzero(n2 == t)
        assert hit.size, (rn, t)
        rows.append(rot[hit[len(hit) // 2]])
    return np.asarray(rows, F)


def axis_angle_rows(rn, N, seed):
    """-> (rot (N,3) f32, tags).  The named rows come first (as many as fit), a random block N(0,1) fills the rest."""
    rows, tags = [], {}

    def put(tag, r):
        tags.setdefault(tag, []).append(len(rows))
        rows.append(np.asarray(r, F))
    put("zero_rot", (0, 0, 0))
    if rn > 0:
        for t, r in zip(("n2_below", "n2_at", "n2_above"), clamp_rows(rn)):
            put(t, r)
    for ax in range(3):
        for sgn in (1.0, -1.0):
            r = np.zeros(3)
            r[ax] = 0.3 * sgn
            put("single_axis", r)
    inf = np.inf
    for r in ((20, 20, 20), (-20, -20, -20), (20, -20, 20), (inf, inf, inf), (-inf, inf, -inf)):
        put("tanh_saturated", r)
        if abs(rn - np.pi / np.sqrt(3.0)) < 1e-6:
            tags.setdefault("th_near_pi", []).append(len(rows) - 1)
    for r in ((inf, 0, 0), (0, -inf, 0), (0, 0, 20)):
        put("tanh_saturated_one_axis", r)
    for r in ((1e-3, -2e-3, 5e-4), (1e-20, 0, 0), (0, -3e-3, 0)):
        put("inside_clamp", r)
    rng = np.random.default_rng(seed)
    rot = np.concatenate([np.asarray(rows, F).reshape(-1, 3), rng.normal(size=(max(N - len(rows), 0), 3)).astype(F)])[:N]
    tags = {t: [k for k in v if k < N] for t, v in tags.items()}
    tags["random"] = list(range(min(len(rows), N), N))
    return np.ascontiguousarray(rot), {t: v for t, v in tags.items() if v}


# ------------------------------------------------------------------------------------------------------------ 6d rows
def sixd_rows(N, seed):
    """-> (rot (N,6) f32, tags, degenerate rows)"""
    rng = np.random.default_rng(seed)
    rows, tags = [], {}

    def put(tag, a1, a2):
        tags.setdefault(tag, []).append(len(rows))
        rows.append(np.concatenate([np.asarray(a1, np.float64), np.asarray(a2, np.float64)]).astype(F))
    put("orthonormal", (1, 0, 0), (0, 1, 0))
    put("orthonormal", (0, 0, -1), (1, 0, 0))
    put("orthonormal", (0.6, 0.8, 0), (-0.8, 0.6, 0))            # 0.6 / 0.8 are not exact in float32: orthonormal to rounding
    a, b = rng.normal(size=3), rng.normal(size=3)
    put("scaled_1e-15", a * 1e-15, b * 1e-15)
    put("scaled_1e15", a * 1e15, b * 1e15)
    put("a1_zero", (0, 0, 0), b)
    put("a2_zero", a, (0, 0, 0))
    put("both_zero", (0, 0, 0), (0, 0, 0))
    a32 = a.astype(F)
    put("parallel", a32, F(3.0) * a32)
    put("parallel", (1, 0, 0), (3, 0, 0))
    put("near_parallel", a32, a32.astype(np.float64) + 1e-7 * rng.normal(size=3))
    rot = np.concatenate([np.asarray(rows, F).reshape(-1, 6), rng.normal(size=(max(N - len(rows), 0), 6)).astype(F)])[:N]
    tags = {t: [k for k in v if k < N] for t, v in tags.items()}
    tags["random"] = list(range(min(len(rows), N), N))
    deg = sorted(k for t in ("parallel", "near_parallel") for k in tags.get(t, []))
    return np.ascontiguousarray(rot), {t: v for t, v in tags.items() if v}, deg


# ------------------------------------------------------------------------------------------------------- translations
def tracknet_rows(N, seed, raw_edges):
    rng = np.random.default_rng(seed)
    tr = rng.normal(size=(N, 3)).astype(F)
    tags = {}
    if raw_edges and N >= 8:
        edge = np.array([[0, 0, 0], [20, -20, 20], [-20, 20, -20], [np.inf, -np.inf, np.inf], [-np.inf, np.inf, 0], [0, 20, -np.inf]], F)
        tr[1:1 + len(edge)] = edge
        tags["raw_trans_edges"] = list(range(1, 1 + len(edge)))
    return tr, tags


def _hand_windows(N, HW, seed):
    """unaligned windows with scales from 1/8 to 8, different in x and y (the hand-made ones of gc.warp_cases)"""
    rng = np.random.default_rng(seed)
    H, W = HW
    tfs = []
    for k in range(N):
        s = (0.125, 0.37, 1.0, 2.9, 8.0)[k % 5]
        sx, sy = s, s * float(rng.uniform(0.8, 1.25))
        left, top = float(rng.uniform(-20, W - 20)) + 0.3, float(rng.uniform(-20, H - 20)) + 0.71
        tfs.append([[sx, 0, -sx * left], [0, sy, -sy * top], [0, 0, 1]])
    return np.asarray(tfs, np.float64).astype(F)


def deepim_trans(N, seed):
    """(shift x, shift y) as a fraction of the crop width, depth ratio about 1; rows 0 / 1 have ratios of exactly 1 and 0.5"""
    rng = np.random.default_rng(seed)
    tr = (rng.normal(size=(N, 3)) * np.array([0.05, 0.05, 0.02]) + np.array([0, 0, 1.0])).astype(F)
    tags = {}
    if N >= 2:
        tr[0, 2], tr[1, 2] = 1.0, 0.5
        tags = dict(ratio_1=[0], ratio_half=[1])
    return tr, tags


# -------------------------------------------------------------------------------------------------------------- cases
def kwargs(c):
    """the keyword arguments of pose_update_model.pose_update / definition / restatement for a case (per-row diameter and K
    where the case is a multi or views one)"""
    kw = dict(rot_rep=c["rot_rep"], normalize_xyz=c["normalize_xyz"], trans_normalizer=c["trans_normalizer"],
              rot_normalizer=c["rot_normalizer"], diameter=row_diameters(c), trans_rep=c["trans_rep"])
    if c["trans_rep"] == "deepim":
        kw.update(K=row_Ks(c), tf=c["tf"], input_w=c["input_w"], input_h=c["input_h"])
    return kw


def row_diameters(c):
    if c["form"] == "single":
        return c["diameter"]
    N = len(c["poses"])
    d = np.asarray(c["diameters"], np.float64)
    o = np.zeros(N, np.int64) if c["obj"] is None else np.asarray(c["obj"], np.int64)
    ok = (o >= 0) & (o < len(d))
    return np.where(ok, d[np.where(ok, o, 0)], np.nan)


def row_Ks(c):
    if c["form"] != "views":
        return c["K"]
    N = len(c["poses"])
    Ks = np.asarray(c["Ks"], np.float64).reshape(-1, 3, 3)
    v = np.zeros(N, np.int64) if c["view"] is None else np.asarray(c["view"], np.int64)
    return Ks[np.clip(v, 0, len(Ks) - 1)]


def cases(scene):
    """-> the list of case records (see the module docstring); scene = the fixture of tests/conftest.py (its poses, K and diameter)"""
    out = []
    D = float(scene["diameter"])
    K0 = np.asarray(scene["K"], np.float64)

    def add(name, targets, trans, rot, poses, rot_rep, normalize_xyz, rn, diameter, trans_rep="tracknet", tags=None, degenerate=(),
            K=None, tf=None, input_w=0.0, input_h=None, form="single", diameters=None, obj=None, Ks=None, view=None, nan_rows=None):
        N = len(poses)
        deg = np.zeros(N, bool)
        deg[list(degenerate)] = True
        out.append(dict(name=name, targets=targets, trans=np.ascontiguousarray(trans, F).reshape(N, 3),
                        rot=np.ascontiguousarray(rot, F).reshape(N, 3 if rot_rep == "axis_angle" else 6),
                        poses=np.ascontiguousarray(poses, F).reshape(N, 4, 4), rot_rep=rot_rep, normalize_xyz=bool(normalize_xyz),
                        trans_normalizer=TN, rot_normalizer=float(F(rn)), diameter=float(diameter), trans_rep=trans_rep, tags=tags or {},
                        degenerate=deg, K=K, tf=None if tf is None else np.ascontiguousarray(tf, F).reshape(N, 3, 3), input_w=float(input_w),
                        input_h=None if input_h is None else float(input_h), form=form, diameters=diameters,
                        obj=None if obj is None else np.asarray(obj, np.int32), Ks=Ks, view=None if view is None else np.asarray(view, np.int32),
                        nan_rows=nan_rows or {}))

    # ---- axis-angle: every rot_normalizer, every N, the three plain translation forms, the four diameters
    plan = ((0.349, 257, "tracknet", True, D), (1.0, 65, "tracknet", False, D), (ROT_NORMALIZERS[2], 63, "raw", False, D),
            (0.0, 64, "tracknet", True, 2.0), (0.349, 1, "tracknet", True, 1e-3), (0.349, 0, "tracknet", True, D),
            (1.0, 64, "tracknet", True, 10.0), (ROT_NORMALIZERS[2], 65, "tracknet", False, D))
    for i, (rn, N, rep, norm, dia) in enumerate(plan):
        rot, tags = axis_angle_rows(rn, N, 100 + i)
        tr, ttags = tracknet_rows(N, 200 + i, raw_edges=rep == "tracknet" and not norm)
        tags.update(ttags)
        add("aa_rn%.3g_n%d_%s%s" % (rn, N, rep, "_norm" if norm else ""),
            "axis-angle, rot_normalizer %.6g, N = %d, %s, normalize_xyz %s, diameter %g: %s" % (rn, N, rep, norm, dia, ", ".join(tags)),
            tr, rot, input_poses(N, scene, 300 + i), "axis_angle", norm, rn, dia, rep, tags)

    # ---- 6d
    for i, (N, rep, norm, dia) in enumerate(((257, "raw", False, D), (65, "tracknet", True, D), (63, "tracknet", False, D), (64, "tracknet", True, 2.0),
                                              (1, "raw", False, D))):
        rot, tags, deg = sixd_rows(N, 400 + i)
        tr, ttags = tracknet_rows(N, 500 + i, raw_edges=rep == "tracknet" and not norm)
        tags.update(ttags)
        add("6d_n%d_%s%s" % (N, rep, "_norm" if norm else ""), "6d, N = %d, %s, normalize_xyz %s, diameter %g: %s" % (N, rep, norm, dia, ", ".join(tags)),
            tr, rot, input_poses(N, scene, 600 + i), "6d", norm, 0.349, dia, rep, tags, deg)

    # ---- deepim
    from oracle import ops as oo
    cw = {c["name"]: c for c in gc.crop_window_cases()}

    def windows(c):
        return oo.crop_windows(c["poses"], c["K"], c["diameter"], c["ratio"], c["out_size"])[0]

    def with_rotations(P, seed):
        P = P.copy()
        P[:, :3, :3] = input_poses(len(P), scene, seed)[:, :3, :3]
        return P
    c = cw["n_257"]                                    # K_SKEW, a 300 x 104 crop: input_w = 300 != input_h = 104
    N = 257
    tr, tags = deepim_trans(N, 700)
    rot, rtags = axis_angle_rows(0.349, N, 701)
    add("deepim_skew_300x104_n257", "deepim, K with skew, windows of crop_window_cases n_257, input_w 300 / input_h 104, depth ratios 1 and 0.5",
        tr, rot, with_rotations(c["poses"], 702), "axis_angle", True, 0.349, c["diameter"], "deepim", dict(tags, **rtags), (), K=gc.K_SKEW,
        tf=windows(c), input_w=300, input_h=104)
    N = 64
    tr, tags = deepim_trans(N, 710)
    rot, rtags, deg = sixd_rows(N, 711)
    ts = np.c_[np.random.default_rng(712).uniform(-0.05, 0.05, (N, 2)), np.random.default_rng(713).uniform(0.4, 2.0, (N, 1))]
    P = input_poses(N, scene, 714)
    P[:, :3, 3] = ts.astype(F)
    add("deepim_dyadic_hand_windows_6d", "deepim with 6d rotations (no libm anywhere), K_DYADIC, unaligned windows of scale 1/8 .. 8, normalize_xyz off",
        tr, rot, P, "6d", False, 0.349, D, "deepim", dict(tags, **rtags), deg, K=gc.K_DYADIC, tf=_hand_windows(N, (128, 128), 715), input_w=160,
        input_h=120)
    ca, cb = cw["half_integer_ties"], cw["degenerate_depths"]
    P = np.concatenate([ca["poses"], cb["poses"]])
    tfw = np.concatenate([windows(ca), windows(cb)])
    N = len(P)
    tr, tags = deepim_trans(N, 720)
    rot = sixd_rows(N + 16, 721)[0][16:]                # the random block only: this case's degenerate rows are the deepim ones
    tz = P[:, 2, 3].astype(np.float64)
    na = len(ca["poses"])
    tags.update(tz_zero=[k for k in range(N) if tz[k] == 0], tz_negative=[k for k in range(N) if tz[k] < 0],
                tz_tiny=[k for k in range(N) if 0 < tz[k] <= 1e-6], collapsed_window=[k for k in range(N) if not np.isfinite(tfw[k]).all()])
    # rows of crop_window_cases()['degenerate_depths'], by their index there: 0 and 4 tz = 0 (a division by zero, a NaN window);
    # 5 the 0.17 m object at 5 000 m (a window one pixel wide: a pixel coordinate's rounding, 2^-24 * 320 px * 5 000 m / 512 px, is
    # 2e-3 of its lateral translation); 6 a collapsed window (infinite scale); 7, 8 a NaN / infinite translation.  tz of -1, of
    # 1e-30 and of 1e-6 (rows 1, 2, 3) are NOT degenerate: the projection divides by tz and z_pred multiplies by it again.
    bad = [na + k for k in (0, 4, 5, 6, 7, 8)]
    add("deepim_ties_and_degenerate_depths", "deepim over the windows of crop_window_cases: half-integer ties; tz of 0, negative, 1e-30 and 1e-6; collapsed windows",
        tr, rot, P, "6d", True, 0.349, 0.17, "deepim", tags, bad, K=ca["K"], tf=tfw, input_w=160, input_h=160)
    assert na == 7 and len(cb["poses"]) == 9

    # ---- several objects: M = 3 interleaved, indices -1 and M; obj = NULL with M = 1
    N = 65
    rot, tags = axis_angle_rows(0.349, N, 800)
    tr, _ = tracknet_rows(N, 801, False)
    obj = (np.arange(N) * 2) % 3
    obj[[5, 40]] = (-1, 3)
    add("multi_m3_interleaved", "M = 3 diameters (2, the scene's, 10), obj interleaved, obj of -1 and of M: NaN translation",
        tr, rot, input_poses(N, scene, 802), "axis_angle", True, 0.349, D, "tracknet", tags, form="multi", diameters=(2.0, D, 10.0), obj=obj,
        nan_rows=dict(translation=[5, 40]))
    add("multi_m3_not_normalised", "the same without normalize_xyz: the diameter is not read, obj of -1 and of M change nothing",
        tr, rot, input_poses(N, scene, 802), "axis_angle", False, 0.349, D, "tracknet", tags, form="multi", diameters=(2.0, D, 10.0), obj=obj)
    add("multi_m1_obj_null", "obj = NULL with M = 1", tr[:7], rot[:7], input_poses(7, scene, 803), "axis_angle", True, 0.349, D, "tracknet",
        {}, form="multi", diameters=(D,), obj=None)

    # ---- several views: V = 3 in any order, -1 and V; view = NULL with V = 1
    N = 65
    c = cw["n_257"]
    tr, tags = deepim_trans(N, 810)
    rot, rtags = axis_angle_rows(0.349, N, 811)
    view = np.random.default_rng(812).integers(0, 3, N)
    view[[3, 64]] = (-1, 3)
    obj = (np.arange(N) + 1) % 3
    add("views_v3_deepim", "V = 3 intrinsics (skew, dyadic, the scene's) in any order, M = 3 objects, a view of -1 and of V: NaN rows",
        tr, rot, with_rotations(c["poses"][:N], 813), "axis_angle", True, 0.349, D, "deepim", dict(tags, **rtags), form="views",
        diameters=(0.21, D, 2.0), obj=obj, Ks=(gc.K_SKEW, gc.K_DYADIC, K0), view=view, tf=windows(c)[:N], input_w=300, input_h=104,
        nan_rows=dict(all=[3, 64]))
    add("views_v1_view_null", "view = NULL with V = 1, obj = NULL with M = 1, tracknet", tr[:9], rot[:9], input_poses(9, scene, 814), "axis_angle", True,
        0.349, D, "tracknet", {}, form="views", diameters=(D,), obj=None, Ks=(K0,), view=None)
    return out


def nonfinite_variants(c):
    """copies of a case with one row of trans, of rot or of the pose made NaN / +inf / -inf -> list of (what, case, bad row)"""
    N = len(c["poses"])
    out = []
    for what, row, val in (("trans", 2 % N, np.nan), ("trans", N - 1, np.inf), ("rot", N // 2, np.nan), ("rot", 1 % N, -np.inf),
                           ("poses", N // 3, np.nan), ("poses", N - 2, np.inf)):
        d = dict(c)
        a = c[what].copy()
        if what == "poses":
            a[row, 0, 3] = val
            a[row, 1, 1] = val
        else:
            a[row, 0] = val
        d[what] = a
        out.append((f"{what}[{row}] = {val}", d, row))
    return out


# ------------------------------------------------------------------------------------------- what a case has to give
def _nan_rows(c, arrays):
    """the rows the header promises as NaN: a view outside 0..V-1 -> every output of the row (an object index outside 0..M-1 gives a
    NaN diameter, which the model already carries into the translation)"""
    rows = c["nan_rows"].get("all", [])
    for a in arrays:
        a[rows] = np.nan
    return arrays


def definition(c, L_f, variant=None):
    """pose_update_model.definition for the case, with the promised NaN rows"""
    d = pm.definition(c["trans"], c["rot"], c["poses"], L_f, variant=variant, **kwargs(c))
    _nan_rows(c, [d["pose"], d["dt"], d["dR"], d["dt_closed"]])
    return d


def restatement(c):
    """-> (pose, trans_delta, rot_delta) of the float32 restatement, with the promised NaN rows"""
    return tuple(_nan_rows(c, list(pm.restatement(c["trans"], c["rot"], c["poses"], **kwargs(c)))))


def flagged(c):
    """the rows left out of the comparison with the bound: the degenerate ones and those promised as NaN"""
    f = c["degenerate"].copy()
    for rows in c["nan_rows"].values():
        f[list(rows)] = True
    return f


def uses_libm(c):
    """-> (the rotation block goes through tanh / sin / cos, the translation goes through tanh)"""
    return c["rot_rep"] == "axis_angle", c["trans_rep"] == "tracknet" and not c["normalize_xyz"]
