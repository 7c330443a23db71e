"""numpy restatement of fp_texture_bake (include/fp_amd.h has the definition) and of the atlas layout above it (ops.texture_bake's uv,
reconstruct.bake_texture's rounding): every value is a float32 array operation, one rounding each, in the order the header writes.  The
`wrong` switches restate the definition with one deliberate mistake each, for the tests that show the checks can tell.  Also: the
rasteriser's texel-index rule (csrc/raster.hip tex_fetch) applied to a uv, for the test of the layout, and the generated meshes and
views of the bit-equality tests."""
import numpy as np

import tsdf_model as tm

f32 = np.float32
STATS = ("bad_view", "behind", "back_facing", "grazing", "outside", "half", "masked", "hole", "nan_depth", "neg_depth", "below_min",
         "hidden", "on_tol", "ulp_past_tol", "blended")


# ------------------------------------------------------------------ the layout
def default_bx(F):
    """block columns of the default atlas: the smallest Bx with Bx * Bx >= F (at least 1)"""
    bx = int(np.ceil(np.sqrt(max(int(F), 1))))
    while bx * bx < F:
        bx += 1
    while bx > 1 and (bx - 1) * (bx - 1) >= F:
        bx -= 1
    return bx


def atlas_shape(F, T, Bx):
    return -(-int(F) // int(Bx)) * int(T), int(Bx) * int(T)


def atlas_uv(F, T, Bx, inset=0.5):
    """-> uv (3F,2) float32 (computed in float64, rounded once; row index growing with v) and uv_idx (F,3) int32.  inset: 0.5 is the
    definition, 0 the wrong variant that puts the corners on the block's border"""
    Ht, Wt = atlas_shape(F, T, Bx)
    f = np.arange(F, dtype=np.int64)
    bx, by = (f % Bx).astype(np.float64), (f // Bx).astype(np.float64)
    dx, dy = np.asarray([0.0, T - 1.0, 0.0]), np.asarray([0.0, 0.0, T - 1.0])
    u = (bx[:, None] * T + inset + dx[None]) / Wt
    v = (by[:, None] * T + inset + dy[None]) / Ht
    return np.stack([u, v], -1).reshape(3 * F, 2).astype(f32), np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def tex_fetch_taps(u, v, Ht, Wt):
    """csrc/raster.hip tex_fetch's index rule for float32 texture coordinates u, v (arrays): uu = fmaf(u, Wt, -0.5) (the product of two
    float32 is exact in float64, so rounding the float64 sum once is the fused operation), i0 = floor(uu), i1 = i0 + 1, wrapped into the
    atlas; the weights of the bilinear blend -> (columns (...,2), rows (...,2), weights (...,2 rows,2 columns))"""
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    uu = (u.astype(np.float64) * Wt - 0.5).astype(f32)
    vv = (v.astype(np.float64) * Ht - 0.5).astype(f32)
    fu0, fv0 = np.floor(uu), np.floor(vv)
    fu, fv = (uu - fu0).astype(np.float64), (vv - fv0).astype(np.float64)
    cols = np.stack([fu0.astype(np.int64) % Wt, (fu0.astype(np.int64) + 1) % Wt], -1)
    rows = np.stack([fv0.astype(np.int64) % Ht, (fv0.astype(np.int64) + 1) % Ht], -1)
    wu, wv = np.stack([1 - fu, fu], -1), np.stack([1 - fv, fv], -1)
    return cols, rows, wv[..., :, None] * wu[..., None, :]


def interpolate_uv(uv3, bary):
    """the rasteriser's interpolation of a face's three uv (3,2) float32 at barycentrics bary (N,3) float32:
    fmaf(b2, uv2, fmaf(b1, uv1, b0 * uv0)), then tu - floor(tu)"""
    uv3, b = np.asarray(uv3, f32).astype(np.float64), np.asarray(bary, f32).astype(np.float64)
    t = (b[:, 0, None] * uv3[0][None]).astype(f32).astype(np.float64)
    t = (b[:, 1, None] * uv3[1][None] + t).astype(f32).astype(np.float64)
    t = (b[:, 2, None] * uv3[2][None] + t).astype(f32)
    return t - np.floor(t)


# ------------------------------------------------------------------ the kernel
def bake(pos, faces, vertex_color, depth, rgb, masks, ob_in_cams, Ks, T, Bx, tol, min_cos, min_depth=0.001, wrong=None, stats=None):
    """-> tex (Ht,Wt,3) float32, coverage (Ht,Wt) uint8.  pos (Nv,3) f32, faces (F,3) ints, vertex_color (Nv,3) f32 | None, depth (V,H,W)
    f32, rgb (V,H,W,3) f32, masks (V,H,W) uint8 | None, ob_in_cams (V,4,4) f32, Ks (V,3,3) f64.  wrong: None | 'no_clamp' |
    'no_depth_test' | 'backfacing' | 'unweighted'.  stats: a dict that receives how many (view, texel) pairs of usable faces took each
    way through the definition, and 'unusable' / 'fallback' texel counts."""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    Nv, F, T, Bx = len(pos), len(faces), int(T), int(Bx)
    depth, rgb = np.asarray(depth, f32), np.asarray(rgb, f32)
    V, H, W = depth.shape
    poses = np.asarray(ob_in_cams, f32).reshape(V, 16)
    Ks = np.asarray(Ks, np.float64).reshape(V, 9)
    tol, min_depth, one = f32(tol), f32(min_depth), f32(1)
    mc2 = f32(min_cos) * f32(min_cos)
    Ht, Wt = atlas_shape(F, T, Bx)
    st = stats if stats is not None else {}
    for k in STATS + ("unusable", "fallback"):
        st.setdefault(k, 0)
    if F == 0:
        return np.zeros((Ht, Wt, 3), f32), np.zeros((Ht, Wt), np.uint8)
    jj, ii = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    with np.errstate(all="ignore"):
        a = (ii.reshape(-1).astype(f32) / f32(T - 1))[None]            # (1, T*T): texel j * T + i of a block
        b = (jj.reshape(-1).astype(f32) / f32(T - 1))[None]
        s = a + b
        if wrong != "no_clamp":
            over = s > one
            a, b = np.where(over, a / s, a), np.where(over, b / s, b)
        c = (one - a) - b
        inr = (faces >= 0) & (faces < Nv)
        safe = np.where(inr, faces, 0)
        table = pos if Nv else np.zeros((1, 3), f32)
        P = [table[safe[:, k]] for k in range(3)]                           # (F,3) each
        p = [(c * P[0][:, k, None] + a * P[1][:, k, None]) + b * P[2][:, k, None] for k in range(3)]      # (F, T*T) each
        e1, e2 = P[1] - P[0], P[2] - P[0]
        n = [e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]]
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        usable = inr.all(1) & (nn > 0) & (nn < f32(np.inf))
        if vertex_color is None:
            fallback = np.full((F, T * T, 3), 128, f32)
        else:
            vc = np.asarray(vertex_color, f32).reshape(-1, 3) if Nv else np.zeros((1, 3), f32)
            col = [np.where(inr[:, k, None], vc[safe[:, k]], f32(128)) for k in range(3)]
            fallback = (c[..., None] * col[0][:, None, :] + a[..., None] * col[1][:, None, :]) + b[..., None] * col[2][:, None, :]
        n = [x[:, None] for x in n]
        acc = np.zeros((F, T * T, 3), f32)
        accw = np.zeros((F, T * T), f32)
        cnt = np.zeros((F, T * T), np.int64)
        base = np.broadcast_to(usable[:, None], (F, T * T))
        for v in range(V):
            M = poses[v]
            K = Ks[v].astype(f32)
            fx, skew, cx, fy, cy = K[0], K[1], K[2], K[4], K[5]
            if not (np.isfinite(M).all() and np.isfinite([fx, fy, cx, cy]).all() and skew == 0):
                st["bad_view"] += 1
                continue
            X = ((M[0] * p[0] + M[1] * p[1]) + M[2] * p[2]) + M[3]
            Y = ((M[4] * p[0] + M[5] * p[1]) + M[6] * p[2]) + M[7]
            Z = ((M[8] * p[0] + M[9] * p[1]) + M[10] * p[2]) + M[11]
            live = base & (Z > 0)
            st["behind"] += int((base & ~live).sum())
            Nx = (M[0] * n[0] + M[1] * n[1]) + M[2] * n[2]
            Ny = (M[4] * n[0] + M[5] * n[1]) + M[6] * n[2]
            Nz = (M[8] * n[0] + M[9] * n[1]) + M[10] * n[2]
            d = (Nx * X + Ny * Y) + Nz * Z
            NN = (Nx * Nx + Ny * Ny) + Nz * Nz
            rr = (X * X + Y * Y) + Z * Z
            w = (d * d) / (NN * rr)
            front = (d < 0) if wrong != "backfacing" else (d != 0)
            st["back_facing"] += int((live & ~front).sum())
            st["grazing"] += int((live & front & ~(w >= mc2)).sum())
            live = live & front & (w >= mc2)
            xu, xv = (fx * X) / Z + cx, (fy * Y) / Z + cy
            uf, vf = np.floor(xu + f32(0.5)), np.floor(xv + f32(0.5))
            inside = (uf >= 0) & (uf < f32(W)) & (vf >= 0) & (vf < f32(H))
            st["outside"] += int((live & ~inside).sum())
            live = live & inside
            st["half"] += int((live & ((xu - np.floor(xu) == f32(0.5)) | (xv - np.floor(xv) == f32(0.5)))).sum())
            ui = np.where(live, uf, 0).astype(np.int64)
            vi = np.where(live, vf, 0).astype(np.int64)
            obj = np.ones(live.shape, bool) if masks is None else masks[v][vi, ui] != 0
            st["masked"] += int((live & ~obj).sum())
            live = live & obj
            dz = depth[v][vi, ui]
            good = dz >= min_depth
            st["hole"] += int((live & (dz == 0)).sum())
            st["nan_depth"] += int((live & np.isnan(dz)).sum())
            st["neg_depth"] += int((live & (dz < 0)).sum())
            st["below_min"] += int((live & (dz > 0) & ~good).sum())
            live = live & good
            err = np.abs(dz - Z)
            st["on_tol"] += int((live & (err == tol)).sum())
            st["ulp_past_tol"] += int((live & (err == np.nextafter(tol, f32(9)))).sum())
            seen = err <= tol
            st["hidden"] += int((live & ~seen).sum())
            if wrong != "no_depth_test":
                live = live & seen
            ww = np.where(live, one if wrong == "unweighted" else w, f32(0)).astype(f32)
            px = rgb[v][vi, ui]                                               # (F, T*T, 3)
            acc = np.where(live[..., None], acc + ww[..., None] * px, acc)
            accw = np.where(live, accw + ww, accw)
            cnt = cnt + live
            st["blended"] += int(live.sum())
        out = np.where((cnt > 0)[..., None], acc / accw[..., None], fallback).astype(f32)
    st["unusable"] += int((~usable).sum()) * T * T
    st["fallback"] += int((cnt == 0).sum())
    rows = Ht // T
    tex = np.zeros((rows * Bx, T, T, 3), f32)
    cov = np.zeros((rows * Bx, T, T), np.uint8)
    tex[:F] = out.reshape(F, T, T, 3)
    cov[:F] = np.minimum(cnt, 255).astype(np.uint8).reshape(F, T, T)
    return (np.ascontiguousarray(tex.reshape(rows, Bx, T, T, 3).transpose(0, 2, 1, 3, 4).reshape(Ht, Wt, 3)),
            np.ascontiguousarray(cov.reshape(rows, Bx, T, T).transpose(0, 2, 1, 3).reshape(Ht, Wt)))


def round_atlas(tex, wrong=None):
    """the atlas as the mesh stores it: floor(x + 0.5) clamped to 0..255, float32 (wrong='trunc': truncation)"""
    t = np.asarray(tex, f32)
    return np.clip(np.trunc(t) if wrong == "trunc" else np.floor(t + f32(0.5)), 0, 255).astype(f32)


def bake_case(case, wrong=None, stats=None):
    return bake(case["pos"], case["faces"], case["vertex_color"], case["depth"], case["rgb"], case["masks"], case["ob_in_cams"], case["Ks"],
                case["T"], case["Bx"], case["tol"], case["min_cos"], case["min_depth"], wrong, stats)


# ------------------------------------------------------------------ generated meshes and views of the bit-equality tests
def generated_case(F, T, Bx=None, V=3, H=24, W=32, kvariant=0, seed=0, with_masks=True, with_colors=True, occluder=False):
    """F faces over a thin slab of seeded vertices about the plane z = 0 and V views of it.
    Face 0 is a right triangle in the plane z = 0 on the lattice of pitch 2^-7 m with legs of T - 1 lattice steps, facing view 0, which
    looks straight down z from 2^-4 m with fx = fy = 8 and cx, cy on .5: its texels are one pixel apart and (where i / (T - 1) is exact)
    project exactly on x.5.  View 0's depth image holds, at the pixels of that face's first texels, depths that put |dz - Z| exactly on
    tol and one ulp of tol beyond it (2^-5 and 2^-5 - 2^-28 under Z = 2^-4, tol = 2^-5: both differences are exact), a hole, a NaN, a negative depth and a mask
    of 0.  With F >= 8 the last six faces are: an index of -1, an index of Nv, a vertex that is NaN, three collinear lattice points (no
    area, nn exactly 0), a repeated vertex, a vertex that is infinite.  The other views are seeded poses around the slab (every third one
    stands in it: texels behind the camera; many project outside the small frames), with seeded depths about the slab's and holes, NaNs,
    negatives and depths just below min_depth sprinkled in; view 2 (when there is one) has a NaN in its pose, view 4 a skewed K.
    occluder: view 1 sees a plane 0.1 m in front of the slab everywhere (its depth test fails for every texel).  -> dict."""
    rng = np.random.default_rng(seed)
    F, T = int(F), int(T)
    Bx = default_bx(F) if Bx is None else int(Bx)
    s, tol, min_depth, zp = f32(2.0 ** -7), f32(2.0 ** -5), f32(2.0 ** -6), f32(2.0 ** -4)
    n_rand = max(3, min(3 * F, 96))
    pos = np.concatenate([rng.uniform(-0.1, 0.1, (n_rand, 2)), rng.uniform(-float(s), float(s), (n_rand, 1))], 1).astype(f32)
    L = f32(T - 1) * s
    o = np.asarray([-4 * s, -4 * s, 0], f32)
    special = np.asarray([o, o + [0, L, 0], o + [L, 0, 0],                       # face 0: n = (0, 0, -L^2), towards view 0
                          o + [2 * s, 0, 0], o + [5 * s, 0, 0],                    # collinear with o
                          [np.nan, 0.01, 0.0], [0.02, np.inf, 0.0]], f32)
    pos = np.concatenate([pos, special]).astype(f32)
    Nv, k0 = len(pos), n_rand
    faces = np.zeros((F, 3), np.int32)
    for f in range(F):
        while True:
            tri = rng.choice(n_rand, 3, replace=False)
            q = pos[tri].astype(np.float64)
            if np.linalg.norm(np.cross(q[1] - q[0], q[2] - q[0])) ** 2 > 1e-12:     # nn well above 1e-30
                break
        faces[f] = tri
    faces[0] = [k0, k0 + 1, k0 + 2]
    if F >= 8:
        faces[F - 1] = [faces[F - 1, 0], -1, faces[F - 1, 2]]
        faces[F - 2] = [Nv, faces[F - 2, 1], faces[F - 2, 2]]
        faces[F - 3] = [faces[F - 3, 0], faces[F - 3, 1], k0 + 5]
        faces[F - 4] = [k0, k0 + 3, k0 + 4]
        faces[F - 5] = [faces[F - 5, 0], faces[F - 5, 0], faces[F - 5, 2]]
        faces[F - 6] = [k0 + 6, faces[F - 6, 1], faces[F - 6, 2]]
    Ks = np.zeros((V, 3, 3))
    poses = np.tile(np.eye(4, dtype=f32), (V, 1, 1))
    depth = np.zeros((V, H, W), f32)
    for v in range(V):
        if v == 0:
            Ks[v] = [[8, 0, W // 2 + 0.5], [0, 8, H // 2 + 0.5], [0, 0, 1]]
            poses[v, 2, 3] = zp
        else:
            fxy = (40.0, 55.5) if kvariant == 0 else (71.25, 33.0)
            Ks[v] = [[fxy[0], 0, W / 2 - 0.3 * v], [0, fxy[1], H / 2 + 0.2 * v], [0, 0, 1]]
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            ang = rng.uniform(0, np.pi)
            Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
            poses[v, :3, :3] = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
            poses[v, :3, 3] = [rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 0.02 if v % 3 == 1 else rng.uniform(0.3, 0.6)]
        zc = float(poses[v, 2, 3])
        depth[v] = (zc + rng.uniform(-1.5, 1.5, (H, W)) * float(tol)).astype(f32)
    r = rng.random((V, H, W))
    depth[r < 0.04] = 0.0
    depth[(r >= 0.04) & (r < 0.06)] = np.nan
    depth[(r >= 0.06) & (r < 0.08)] = -0.4
    depth[(r >= 0.08) & (r < 0.10)] = np.nextafter(min_depth, f32(0))
    masks = None
    if with_masks:
        masks = (rng.random((V, H, W)) < 0.8).astype(np.uint8) * np.uint8(255 if seed % 2 else 1)
    # view 0: texel (i, j) of face 0 lands on pixel (u0 + j, v0 + i)
    u0, v0 = W // 2 + 1 - 4, H // 2 + 1 - 4
    if masks is not None:
        masks[0, v0:v0 + 3, u0:u0 + 3] = 1
    depth[0, v0:v0 + 3, u0:u0 + 3] = zp
    depth[0, v0, u0] = zp - tol
    depth[0, v0, u0 + 1] = f32(zp - tol) - f32(2.0 ** -28)
    depth[0, v0 + 1, u0] = 0.0
    depth[0, v0, u0 + 2] = np.nan
    depth[0, v0 + 2, u0] = -0.4
    if masks is not None:
        masks[0, v0 + 1, u0 + 1] = 0
    if occluder and V >= 2:
        depth[1] = np.maximum(depth[1] - f32(0.1), f32(0.05))
        poses[1, 2, 3] = max(float(poses[1, 2, 3]), 0.3)
    if V >= 3:
        poses[2, 1, 2] = np.nan
    if V >= 5:
        Ks[4, 0, 1] = 0.01
    rgb = rng.uniform(0, 255, (V, H, W, 3)).astype(f32)
    vcol = rng.uniform(0, 255, (Nv, 3)).astype(f32) if with_colors else None
    return dict(pos=pos, faces=faces, vertex_color=vcol, depth=depth, rgb=rgb, masks=masks, ob_in_cams=poses, Ks=Ks, T=T, Bx=Bx, tol=tol,
                min_cos=f32(0.2), min_depth=min_depth)


# (F, T, Bx (None: the default), V, H, W, K variant, masks, vertex colours): every F, T, V, frame and K variant of the list, Bx = 1, a Bx
# that leaves the last block row partly filled, and the default
CASES = [
    (1, 2, None, 1, 24, 32, 0, True, True),
    (1, 16, 1, 3, 37, 53, 1, False, False),
    (2, 3, 1, 3, 24, 32, 0, True, False),
    (2, 5, None, 16, 37, 53, 1, True, True),
    (63, 4, None, 3, 24, 32, 1, True, True),
    (63, 3, 5, 16, 24, 32, 0, False, True),
    (64, 8, None, 3, 37, 53, 0, True, True),
    (64, 2, 7, 1, 24, 32, 0, True, False),
    (65, 5, 8, 3, 37, 53, 1, True, True),
    (65, 16, None, 16, 24, 32, 0, False, True),
    (257, 3, None, 16, 37, 53, 0, True, True),
    (257, 4, 10, 3, 24, 32, 1, True, False),
    (257, 8, 1, 1, 24, 32, 0, True, True),
    (65, 2, 1, 16, 37, 53, 1, True, True),
]


def case_id(c):
    F, T, Bx, V, H, W, kv, m, col = c
    return f"F{F}-T{T}-Bx{'d' if Bx is None else Bx}-V{V}-{H}x{W}-K{kv}{'-m' if m else ''}{'-c' if col else ''}"


def case_of(c):
    F, T, Bx, V, H, W, kv, m, col = c
    return generated_case(F, T, Bx, V, H, W, kv, seed=F + 3 * T + V + H, with_masks=m, with_colors=col)


# ------------------------------------------------------------------ the can's held-out views
HELD_OUT = [1, 5, 9, 14, 20]


def held_out_poses():
    return tm.can_view_poses(23, 0.5)[HELD_OUT].astype(f32)


def colour_error(color, ref_color, depth, ref_depth):
    """mean absolute colour error in 8-bit levels over the pixels both renders cover -> (error, pixels)"""
    both = (np.asarray(depth) > 0) & (np.asarray(ref_depth) > 0)
    d = np.abs(np.clip(np.asarray(color, np.float64), 0, 1) - np.clip(np.asarray(ref_color, np.float64), 0, 1))[both] * 255.0
    return float(d.mean()), int(both.sum())
