"""Generated inputs for the geometry kernels (csrc/raster.hip, warp.hip and the per-frame / per-pose kernels of frame_ops.hip):
meshes, cameras, windows, frames and poses chosen to reach the paths that the one scene of tests/conftest.py never reaches.
Seeded, numpy only.  Every generator returns a list of named records (plain dicts) that carry their inputs and, under "targets", a
short statement of what they are there for.  tests/test_geometry_cases_host.py (CPU: the oracle against the integer model of
tests/raster_model.py and against wrong variants) and tests/test_gpu_geometry_edges.py (GPU: the kernels against the oracle) use
the same records.  Test infrastructure only; not a conftest."""
import functools

import numpy as np

F = np.float32
OUT_SIZES = ((1, 1), (16, 16), (17, 33), (160, 160), (104, 300), (8, 1024), (1024, 8))      # (oh, ow)
K_SKEW = np.array([[900.0, 3.5, 300.25], [0.0, 1100.0, 210.75], [0.0, 0.0, 1.0]])          # skew, fx != fy, off-centre
K_DYADIC = np.array([[512.0, 0.0, 64.5], [0.0, 512.0, 64.5], [0.0, 0.0, 1.0]])
FRAMES = ((480, 640), (375, 501), (96, 128))                                                 # (H, W); the second is odd


# ------------------------------------------------------------------------------------------------------------ meshes
def _colors(n, seed):
    return (np.random.default_rng(seed).uniform(0.15, 1.0, size=(n, 3)) * 255).astype(np.uint8)


def _simple(verts, faces, seed, **kw):
    from foundationpose_amd.mesh import SimpleMesh
    verts = np.asarray(verts, np.float64)
    if "texture" not in kw:
        kw["vertex_colors"] = _colors(len(verts), seed)
    return SimpleMesh(verts, np.asarray(faces, np.int64), **kw)


def box(size=(0.08, 0.05, 0.12), n=6, seed=1, R=None, t=(0, 0, 0)):
    """_box of tests/test_gpu_multi_object.py (every face an n x n grid, outward orientation), optionally moved"""
    verts, faces = [], []
    half = np.asarray(size) / 2
    g = np.linspace(-1, 1, n + 1)
    for axis in range(3):
        for sgn in (-1.0, 1.0):
            u, v = [a for a in range(3) if a != axis]
            base = len(verts)
            for j in g:
                for i in g:
                    p = np.zeros(3)
                    p[axis], p[u], p[v] = sgn, i, j
                    verts.append(p * half)
            for j in range(n):
                for i in range(n):
                    a, b = base + j * (n + 1) + i, base + j * (n + 1) + i + 1
                    c, d = base + (j + 1) * (n + 1) + i, base + (j + 1) * (n + 1) + i + 1
                    outward = sgn * (1.0 if (u - axis) % 3 == 1 else -1.0)
                    faces += [[a, b, d], [a, d, c]] if outward > 0 else [[a, d, b], [a, c, d]]
    verts = np.asarray(verts)
    if R is not None:
        verts = verts @ np.asarray(R).T
    return _simple(verts + np.asarray(t), faces, seed)


def slab_stack(L=60, rising=True, seed=11):
    """L parallel quads 1 mm apart along z, the farther ones larger so that they show around the nearer ones.  Seen face on, every
    one of its 2 L triangles spans every 16-row strip of the crop: 2 L > 96 entries for the strip's queue of large triangles.
    rising: triangle ids rise with z; otherwise they fall."""
    verts, faces = [], []
    order = range(L) if rising else range(L - 1, -1, -1)
    for k in order:
        h = 0.03 + 0.0005 * k
        z = -0.03 + 0.001 * k
        b = len(verts)
        verts += [[-h, -h, z], [h, -h, z], [h, h, z], [-h, h, z]]
        faces += [[b, b + 1, b + 2], [b, b + 2, b + 3]]
    return _simple(verts, faces, seed)


def twin_faces(seed=12):
    """a box whose face list is followed by a permuted copy of itself (same vertices, same vertex order per face): every covered
    pixel is an exact tie of the depth key between triangle t < T/2 and its twin >= T/2"""
    m = box(seed=seed)
    f = np.asarray(m.faces)
    perm = np.random.default_rng(seed).permutation(len(f))
    return _simple(m.vertices, np.concatenate([f, f[perm]]), seed)


def sliver_soup(n=4000, n_twins=200, seed=13):
    """random thin triangles: a long edge A-B of 1 .. 5 cm and a third vertex at a distance w from A, w log-uniform over 1e-7 ..
    1e-2 m (at the cases' distance a crop pixel is about 1 mm, so from far below the 1/16 px snap up to ten pixels).  The last
    n_twins triangles repeat the first n_twins with vertices of their own: coplanar, identical depth, different ids and colours."""
    rng = np.random.default_rng(seed)
    A = rng.uniform(-0.05, 0.05, (n, 3)) * np.array([1, 1, 0.3])
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    B = A + d * rng.uniform(0.01, 0.05, (n, 1))
    e = rng.normal(size=(n, 3)); e /= np.linalg.norm(e, axis=1, keepdims=True)
    C = A + e * (10.0 ** rng.uniform(-7, -2, (n, 1)))
    verts = np.stack([A, B, C], 1).reshape(-1, 3)
    faces = np.arange(3 * n).reshape(n, 3)
    verts = np.concatenate([verts, verts[:3 * n_twins]])
    faces = np.concatenate([faces, 3 * n + np.arange(3 * n_twins).reshape(n_twins, 3)])
    return _simple(verts, faces, seed)


def half_cylinder(radius=0.05, height=0.12, n_ang=24, n_ax=10, seed=14):
    """an open half cylinder (no caps, no back): from inside only back faces are there to win"""
    verts, faces = [], []
    for iz in range(n_ax + 1):
        for ia in range(n_ang + 1):
            a = np.pi * ia / n_ang
            verts.append([radius * np.cos(a), radius * np.sin(a), -height / 2 + height * iz / n_ax])
    ring = n_ang + 1
    for iz in range(n_ax):
        for ia in range(n_ang):
            a0 = iz * ring + ia
            faces += [[a0, a0 + 1, a0 + ring + 1], [a0, a0 + ring + 1, a0 + ring]]
    return _simple(verts, faces, seed)


def crossed_boxes(seed=15):
    """two boxes that interpenetrate: the visible surface changes owner along curves inside triangles"""
    c, s = np.cos(0.7), np.sin(0.7)
    a = box((0.10, 0.03, 0.05), n=4, seed=seed)
    b = box((0.10, 0.03, 0.05), n=4, seed=seed + 1, R=[[c, -s, 0], [s, c, 0], [0, 0, 1]], t=(0.004, 0.0, 0.006))
    verts = np.concatenate([a.vertices, b.vertices])
    faces = np.concatenate([a.faces, np.asarray(b.faces) + len(a.vertices)])
    return _simple(verts, faces, seed)


def l_prism(seed=16):
    """a concave (L-shaped) prism of 20 triangles"""
    poly = np.array([[0, 0], [0.08, 0], [0.08, 0.03], [0.03, 0.03], [0.03, 0.09], [0, 0.09]]) - [0.035, 0.04]
    h = 0.025
    verts = [[x, y, -h] for x, y in poly] + [[x, y, h] for x, y in poly]
    cap = [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5]]
    faces = [[a, c, b] for a, b, c in cap] + [[a + 6, b + 6, c + 6] for a, b, c in cap]
    for i in range(6):
        j = (i + 1) % 6
        faces += [[i, j, j + 6], [i, j + 6, i + 6]]
    return _simple(verts, faces, seed)


def pixel_lattice(n=24, seed=17):
    """a planar n x n grid of quads with a vertex spacing of 2^-8 m: under K_DYADIC at z = 1 the vertices project exactly onto
    pixel centres two pixels apart, so every edge of the mesh runs through pixel centres (edge ownership decides them)"""
    g = (np.arange(n + 1) - n // 2) / 256.0
    verts = [[x, y, 0.0] for y in g for x in g]
    faces = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            faces += [[a, a + 1, a + n + 2], [a, a + n + 2, a + n + 1]]
    return _simple(verts, faces, seed)


def zero_normal_box(seed=18):
    """a box of which every third vertex normal is exactly zero (the 1e-12 floors of the Lambert term and of the normal output)"""
    m = box(seed=seed)
    vn = np.array(m.vertex_normals)
    vn[::3] = 0.0
    return _simple(m.vertices, m.faces, seed, vertex_normals=vn)


def _tensors(mesh):
    from oracle import pipeline as op
    return op.mesh_tensors_np(mesh)


def _diameter(mesh):
    v = np.asarray(mesh.vertices)
    return float(np.linalg.norm(v.max(0) - v.min(0)))


def textured(tex_hw, seed=19):
    """a small can with uv stretched to about [-1.5, 2.5] (wrap), a uv table of its own order addressed through a separate uv_idx,
    and a (Ht, Wt) texture.  -> (SimpleMesh, mesh tensors with the separate uv_idx)"""
    from foundationpose_amd.mesh import make_can_mesh, make_texture
    rng = np.random.default_rng(seed)
    Ht, Wt = tex_hw
    tex = make_texture(512, seed) if (Ht, Wt) == (512, 512) else rng.integers(0, 256, (Ht, Wt, 3)).astype(np.uint8)
    can = make_can_mesh(radius=0.04, height=0.10, n_ang=20, n_axial=8, textured=False, seed=seed)
    ang = np.arctan2(can.vertices[:, 1], can.vertices[:, 0]) / (2 * np.pi) + 0.5
    uv = np.stack([ang * 4.0 - 1.5, (can.vertices[:, 2] / 0.10 + 0.5) * 4.0 - 1.5], 1)
    from foundationpose_amd.mesh import SimpleMesh
    mesh = SimpleMesh(can.vertices, can.faces, uv=uv, texture=tex)
    t = _tensors(mesh)
    perm = rng.permutation(len(uv))                 # uv row perm[k] moves to row k; uv_idx points back through the inverse
    inv = np.empty_like(perm); inv[perm] = np.arange(len(perm))
    t["uv"] = np.ascontiguousarray(t["uv"][perm])
    t["uv_idx"] = np.ascontiguousarray(inv[t["faces"]].astype(np.int32))
    assert np.array_equal(t["uv"][t["uv_idx"]], _tensors(mesh)["uv"][t["faces"]])
    return mesh, t


@functools.lru_cache(maxsize=None)
def _mesh_table():
    out = {}

    def add(name, mesh, targets, tensors=None):
        out[name] = dict(name=name, mesh=mesh, np=tensors if tensors is not None else _tensors(mesh), diameter=_diameter(mesh),
                         targets=targets)
    add("slab_up", slab_stack(rising=True), "FP_BIG_MAX overflow, ids rising with depth")
    add("slab_down", slab_stack(rising=False), "FP_BIG_MAX overflow, ids falling with depth")
    add("twin_faces", twin_faces(), "equal depth keys between different triangles: the lower id wins")
    add("sliver_soup", sliver_soup(), "zero area after the 1/16 px snap, slivers, coplanar pairs")
    add("half_cylinder", half_cylinder(), "open mesh, back faces win")
    add("crossed_boxes", crossed_boxes(), "interpenetrating surfaces")
    add("l_prism", l_prism(), "concave prism")
    add("pixel_lattice", pixel_lattice(), "vertices and edges exactly on pixel centres and on snap halves")
    add("zero_normals", zero_normal_box(), "vertex normals exactly zero")
    for hw in ((1, 1), (2, 3), (512, 512)):
        m, t = textured(hw)
        add("tex_%dx%d" % hw, m, "uv outside [0, 1], separate uv_idx, %d x %d texture" % hw, t)
    return out


def meshes(scene):
    """name -> dict(mesh SimpleMesh, np mesh tensors for the oracle, diameter, targets); the scene's can and its scaled-up copy
    (for the far plane) included"""
    out = dict(_mesh_table())
    out["can"] = dict(name="can", mesh=scene["mesh"], np=scene["mesh_np"], diameter=scene["diameter"], targets="the scene's can")
    big = dict(scene["mesh_np"])
    big["pos"] = (scene["mesh_np"]["pos"].astype(np.float64) * 6000.0).astype(F)
    out["can_x6000"] = dict(name="can_x6000", mesh=None, np=big, diameter=scene["diameter"] * 6000.0,
                            targets="the can scaled to about 1 km, for the FP_ZMAXF clamp")
    return out


# ------------------------------------------------------------------------------------------------------ raster cases
def _pose(R, t):
    P = np.eye(4)
    P[:3, :3] = R
    P[:3, 3] = t
    return P


def _rz(deg):
    c, s = {0: (1.0, 0.0), 90: (0.0, 1.0), 180: (-1.0, 0.0), 270: (0.0, -1.0)}[deg]
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def _windows(poses, K, diameter, ratio, out_hw):
    from oracle import ops as oo
    return oo.crop_windows(np.asarray(poses, F), K, diameter, ratio, (out_hw[1], out_hw[0]))


def _centre_at(K, u, v, z):
    """translation whose projection through K (with skew) is pixel (u, v) at depth z"""
    y = (v - K[1, 2]) * z / K[1, 1]
    x = ((u - K[0, 2]) * z - K[0, 1] * y) / K[0, 0]
    return np.array([x, y, z])


def raster_cases(scene):
    """-> list of dict(name, mesh (key of meshes()), K, H, W, poses (N,4,4) f32, bbox (N,4) f32, out_hw, diameter, targets,
    tags).  tags: 'floats' = the float outputs are O(1) and are compared too, 'cull' = must cull some but not all vertices and
    still cover pixels, 'cull_empty' = culls and covers nothing, 'far' = every covered pixel sits on the FP_ZMAXF clamp,
    'big' = overflows the queue of large triangles, 'tie', 'soup', 'multi' = also run through a MeshSet."""
    rng = np.random.default_rng(20)
    M = meshes(scene)
    grid = scene["poses"][:, :3, :3].astype(np.float64)
    K0 = np.asarray(scene["K"], np.float64)
    cases = []

    def add(name, mesh, K, HW, poses, out_hw, targets, tags=(), ratio=1.2, bbox=None):
        poses = np.asarray(poses, np.float64).astype(F)
        if bbox is None:
            _, bbox = _windows(poses, K, M[mesh]["diameter"], ratio, out_hw)
        cases.append(dict(name=name, mesh=mesh, K=np.asarray(K, np.float64), H=HW[0], W=HW[1], poses=poses,
                          bbox=np.ascontiguousarray(bbox, F), out_hw=tuple(out_hw), diameter=M[mesh]["diameter"], targets=targets,
                          tags=tuple(tags)))

    def rots(n, whole=False):
        idx = np.arange(len(grid)) if whole else np.sort(rng.choice(len(grid), n, replace=False))
        return [np.eye(3)] + [grid[i] for i in idx]

    t0 = np.array([0.01, -0.02, 0.6])
    for nm in ("slab_up", "slab_down"):
        add(nm, nm, K0, FRAMES[0], [_pose(R, t0) for R in rots(11)], (160, 160), M[nm]["targets"], ("floats", "big", "multi"))
    add("twin_faces", "twin_faces", K0, FRAMES[0], [_pose(R, t0) for R in rots(0, whole=True)], (160, 160),
        M["twin_faces"]["targets"], ("floats", "tie", "multi"))
    add("sliver_soup", "sliver_soup", K0, FRAMES[0], [_pose(R, t0) for R in rots(7)], (160, 160), M["sliver_soup"]["targets"],
        ("floats", "soup"))
    add("half_cylinder", "half_cylinder", K_SKEW, FRAMES[1], [_pose(R, [0.0, 0.0, 0.4]) for R in rots(23)], (160, 160),
        M["half_cylinder"]["targets"] + "; K with skew; odd frame", ("floats", "multi"))
    add("crossed_boxes", "crossed_boxes", K_SKEW, FRAMES[1], [_pose(R, _centre_at(K_SKEW, 20.0, 360.0, 0.5)) for R in rots(23)],
        (104, 300), M["crossed_boxes"]["targets"] + "; K with skew; window over the frame's lower left corner", ("floats", "multi"))
    add("l_prism", "l_prism", K0, FRAMES[2], [_pose(R, [0.0, 0.0, 0.9]) for R in rots(0, whole=True)], (17, 33),
        M["l_prism"]["targets"] + "; 17 x 33 crop, small frame", ("floats",))
    add("zero_normals", "zero_normals", K0, FRAMES[0], [_pose(R, t0) for R in rots(7)], (160, 160), M["zero_normals"]["targets"],
        ("floats", "multi"))
    for nm in ("tex_1x1", "tex_2x3", "tex_512x512"):
        add(nm, nm, K_SKEW, FRAMES[0], [_pose(R, [0.02, 0.01, 0.45]) for R in rots(5)], (160, 160), M[nm]["targets"], ("floats",))

    # vertices and edges exactly on pixel centres: quarter turns, the back side, and shifts of exactly 1/32 px (snap halves)
    flip = np.diag([1.0, -1.0, -1.0])
    lat = [_pose(_rz(a), [0, 0, 1.0]) for a in (0, 90, 180, 270)] + [_pose(flip @ _rz(a), [0, 0, 1.0]) for a in (0, 90)]
    lat += [_pose(_rz(a), [s * 2.0 ** -14, s * 2.0 ** -14, 1.0]) for a in (0, 90) for s in (1.0, -1.0, 3.0)]
    add("pixel_lattice", "pixel_lattice", K_DYADIC, (128, 128), lat, (128, 128),
        M["pixel_lattice"]["targets"], ("floats",), bbox=np.tile(np.array([0, 0, 128, 128], F), (len(lat), 1)))

    # the can: near plane, guard band, far plane, window and crop sizes
    Rg = np.asarray(scene["gt"], np.float64)[:3, :3]
    near = [_pose(R, [0.0, 0.0, 0.04]) for R in [Rg] + rots(3)[1:]]
    add("can_near", "can", K0, FRAMES[0], near, (160, 160), "vertices at z <= FP_ZNEAR: their triangles go, the neighbours stay",
        ("floats", "cull"))
    P5 = np.asarray([_pose(R, [0.0, 0.0, 0.5]) for R in [Rg] + rots(2)[1:]])
    c = K0 @ np.array([0.0, 0.0, 0.5]) / 0.5
    for px, tag in ((12.0, "cull"), (6.0, "cull_empty")):
        bb = np.tile(np.array([c[0] - px / 2, c[1] - px / 2, c[0] + px / 2, c[1] + px / 2], F), (len(P5), 1))
        add("can_zoom%d" % px, "can", K0, FRAMES[0], P5, (160, 160), "a %d px window: vertices beyond the guard band" % px,
            ("floats", tag), bbox=bb)
    far = [_pose(R, [30.0, -20.0, 5000.0]) for R in [Rg] + rots(2)[1:]]
    add("can_far", "can_x6000", K0, FRAMES[0], far, (160, 160), "depth beyond 4095 m: the FP_ZMAXF clamp, zbuf 0xFFF00000", ("far",))
    tg = np.asarray(scene["gt"], np.float64)[:3, 3]
    for hw in OUT_SIZES:
        if hw == (160, 160):
            continue
        Ps = np.asarray([_pose(R, tg) for R in [Rg] + rots(3)[1:]])
        # a window needs two pixels per side to have an extent of its own (bbox = the corners' centres): a side of 1 takes the 160's
        _, bb = _windows(Ps, K0, M["can"]["diameter"], 1.2, (hw[0] if hw[0] > 1 else 160, hw[1] if hw[1] > 1 else 160))
        add("can_%dx%d" % hw, "can", K0, FRAMES[0], Ps, hw,
            "crop of %d x %d (oh x ow)%s" % (hw + ("; ow > 256: step_j = 0 in the resolve walk" if hw[1] > 256 else "",)),
            ("floats",), bbox=bb)
    # windows over each frame edge, over a corner, and wholly outside the frame
    H, W = FRAMES[0]
    spots = dict(left=(2.0, 240.0), right=(W - 3.0, 200.0), top=(300.0, 1.0), bottom=(350.0, H - 2.0), corner=(W - 1.0, H - 1.0),
                 outside=(-400.0, -300.0))
    add("frame_edges", "crossed_boxes", K0, FRAMES[0], [_pose(grid[7 * k], _centre_at(K0, u, v, 0.55))
                                                         for k, (u, v) in enumerate(spots.values())], (160, 160),
        "windows over " + ", ".join(spots), ("floats",))
    return cases


def nonfinite_rows(case, seed=21):
    """a copy of a raster case's poses and windows with rows made non-finite (NaN / infinite pose entries, NaN / infinite window):
    -> (poses, bbox, bad row indices).  Every comparison with NaN is false, so every vertex of such a row is culled."""
    P, bb = case["poses"].copy(), case["bbox"].copy()
    n = len(P)
    bad = [1 % n, 3 % n, 4 % n, (n - 1)]
    P[bad[0], 2, 3] = np.nan
    P[bad[1], 0, 0] = np.inf
    bb[bad[2], 0] = np.nan
    bb[bad[3], 2] = np.inf
    return P, bb, sorted(set(bad))


# -------------------------------------------------------------------------------------------------------- warp cases
WARP_SIZES = ((2, 2), (3, 2), (16, 16), (17, 33), (160, 160), (104, 300), (8, 1024), (1024, 8), (5, 1023), (7, 3))   # (oh, ow)


def warp_frame(HW, diameter, t, seed):
    """seeded rgb (0..255), depth and xyz map of one frame.  depth: a smooth surface near t[2] with holes (0), negative values and
    patches of exactly 0.001 and 0.1 (the two thresholds; bit-for-bit float32(0.001) / float32(0.1)).  xyz: the back-projection
    free stand-in the REFINE warp reads: t + offsets, with texels exactly `diameter` away from t along each axis (val exactly +-2
    after the normalisation by diameter / 2 when diameter is a power of two) and texels one float32 step inside."""
    rng = np.random.default_rng(seed)
    H, W = HW
    rgb = rng.uniform(0, 255, (H, W, 3)).astype(F)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (t[2] + 0.05 * np.sin(xx / 7.0) * np.cos(yy / 5.0)).astype(F)
    kind = rng.integers(0, 16, (H, W))
    depth[kind == 0] = 0.0
    depth[kind == 1] = -0.3
    depth[kind == 2] = F(0.001)
    depth[kind == 3] = F(0.1)
    depth[kind == 4] = np.nextafter(F(0.001), F(0))
    depth[kind == 5] = np.nextafter(F(0.1), F(0))
    depth[kind == 6] = F(t[2]) + F(diameter)                         # SCORE: z - t_z == +-diameter exactly, |val| == 2
    depth[kind == 7] = F(t[2]) - F(diameter)
    depth[kind == 8] = np.nextafter(F(t[2]) + F(diameter), F(0))     # one step inside
    xyz =(np.asarray(t, F) + rng.uniform(-0.4, 0.4, (H, W, 3)).astype(F) * F(diameter)).astype(F)
    xyz[..., 2] = np.abs(xyz[..., 2])
    tt = np.asarray(t, F)
    d = F(diameter)
    for ax in range(3):
        for k, sgn in ((6 + 2 * ax, 1.0), (7 + 2 * ax, -1.0)):
            sel = kind == k
            xyz[sel, ax] = tt[ax] + F(sgn) * d                       # |val| == 2 exactly (t and d chosen so that the sum is exact)
            half = sel & ((xx + yy) % 2 == 0)
            xyz[half, ax] = np.nextafter(tt[ax] + F(sgn) * d, tt[ax])   # one step inside
    xyz[kind == 12, 2] = F(0.001)
    xyz[kind == 13, 2] = np.nextafter(F(0.001), F(0))
    xyz[kind == 14] = 0.0
    return rgb, depth, xyz


def warp_cases(scene):
    """-> list of dict(name, H, W, K, rgb, depth, xyz, tf (N,3,3) f32, poses (N,4,4) f32, diameter, out_hw, targets, bad_rows).
    Windows: integer-aligned ones from crop_windows, hand-made unaligned ones, scales from 1/8 to 8, windows over every frame
    edge, over a corner and wholly outside.  diameter = 0.25 and dyadic translations make the |val| == 2 texels exact."""
    cases = []
    diameter = 0.25
    t = np.array([0.125, -0.0625, 1.0])
    for fi, (H, W) in enumerate(FRAMES):
        K = (np.asarray(scene["K"], np.float64), K_SKEW, K_DYADIC)[fi].copy()
        K[0, 1] = 0.0                       # the warp's back-projection has no skew term
        rgb, depth, xyz = warp_frame((H, W), diameter, t, 30 + fi)
        for oh, ow in WARP_SIZES:
            if fi > 0 and (oh, ow) not in ((2, 2), (17, 33), (160, 160), (5, 1023)):
                continue
            rng = np.random.default_rng(1000 * fi + 10 * oh + ow)
            tfs = []
            # aligned windows from crop_windows, centred on spots inside, on the edges, on a corner and outside the frame
            spots = [(W / 2, H / 2), (1.0, H / 2), (W - 2.0, H / 3), (W / 3, 0.0), (W / 2, H - 1.0), (W - 1.0, H - 1.0), (-3.0 * W, -2.0 * H)]
            Pw = np.asarray([_pose(np.eye(3), _centre_at(K, u, v, z)) for (u, v), z in zip(spots, (1.0, 0.5, 2.0, 4.0, 0.25, 1.0, 1.0))])
            tf_al, _ = _windows(Pw, K, diameter, 1.2, (oh, ow))
            tfs += list(tf_al)
            # unaligned: fractional left / top edges, scales 1/8 .. 8, different in x and y
            for s in (0.125, 0.37, 1.0, 2.9, 8.0):
                sx, sy = s, s * float(rng.uniform(0.8, 1.25))
                left, top = float(rng.uniform(-20, W - 20)) + 0.3, float(rng.uniform(-20, H - 20)) + 0.71
                tfs.append(np.array([[sx, 0, -sx * left], [0, sy, -sy * top], [0, 0, 1]]))
            tf = np.asarray(tfs, np.float64).astype(F)
            N = len(tf)
            poses = np.tile(_pose(np.eye(3), t).astype(F), (N, 1, 1))
            cases.append(dict(name="warp_%dx%d_to_%dx%d" % (H, W, oh, ow), H=H, W=W, K=K, rgb=rgb, depth=depth, xyz=xyz, tf=tf,
                              poses=poses, diameter=diameter, out_hw=(oh, ow),
                              targets="multiply-shift p / ow at ow = %d; aligned and unaligned windows; thresholds" % ow))
    return cases


def warp_nonfinite(case):
    """the case's windows with rows made non-finite, and one finite row whose offset puts the frame coordinates beyond 2^31 px
    (the float-to-int conversion saturates like an infinity's) -> (tf, poses, bad rows)"""
    tf, P = case["tf"].copy(), case["poses"].copy()
    bad = [0, 2, 4, 5, len(tf) - 1]
    tf[bad[0], 0, 0] = np.nan
    tf[bad[1], 1, 2] = np.inf
    tf[bad[2], 0, 2] = F(-4e9) * tf[bad[2], 0, 0]
    tf[bad[3], 1, 2] = F(-4e9) * tf[bad[3], 1, 1]
    tf[bad[4], 0, 2] = -np.inf
    return tf, P, bad


# ------------------------------------------------------------------------------------------------------ filter cases
FILTER_SIZES = ((1, 1), (1, 7), (5, 1), (3, 3), (33, 65), (481, 643))


def _ratio_tie_frame(H, W, zfar):
    """neighbourhoods of radius 2 in which bad / total is exactly 0.8 and one step either side of it.  Interior: 5 x 5 = 25 texels,
    20 / 19 / 21 bad.  Left border (w = 0, window 3 x 5 = 15 texels): 12 / 11 / 13 bad.  The centres are good texels (depth 1);
    bad texels are holes.  -> (depth, list of (h, w, bad, total))"""
    d = np.ones((H, W), F)
    marks = []

    def plant(h, w, nbad, cols):
        cells = [(h + dv, w + du) for du in cols for dv in range(-2, 3) if (du, dv) != (0, 0)]
        for (a, b) in cells[:nbad]:
            d[a, b] = 0.0
        marks.append((h, w, nbad, len(cells) + 1))
    if H >= 30 and W >= 40:
        for k, nbad in enumerate((20, 19, 21)):
            plant(5 + 8 * k, 10, nbad, range(-2, 3))
            plant(5 + 8 * k, 0, nbad - 8, range(0, 3))
    return d, marks


def filter_cases():
    """-> list of dict(name, depth (H,W) f32, zfar, targets, ties [(h, w, bad, total)]) for erode / bilateral / depth_to_xyz"""
    cases = []
    for (H, W) in FILTER_SIZES:
        rng = np.random.default_rng(100 * H + W)
        yy, xx = np.mgrid[0:H, 0:W]
        base = (0.8 + 0.0004 * xx + 0.0003 * yy).astype(F)
        pats = dict(constant=np.full((H, W), 0.75, F))
        ch = base.copy(); ch[(xx + yy) % 2 == 0] = 0.0
        pats["checker_holes"] = ch
        rh = base.copy(); rh[rng.random((H, W)) < 0.3] = 0.0
        pats["random_holes"] = rh
        sp = base.copy()
        kind = rng.integers(0, 12, (H, W))
        for k, v in enumerate((F(0.001), np.nextafter(F(0.001), F(0)), F(2.0), np.nextafter(F(2.0), F(0)), F(2.5), F(-0.5), F(np.inf),
                               F(np.nan), F(-np.inf))):
            sp[kind == k] = v
        pats["special_values"] = sp                                   # with zfar = 2: exactly at, just below and beyond zfar
        st = np.full((H, W), 1.0, F)
        st[:, 1::2] = F(1.0) + F(0.001)                                  # steps of exactly depth_diff_thres (in float32)
        st[1::3] = st[1::3] + np.spacing(F(1.0))
        pats["diff_steps"] = st
        pats["near_50m"] = (50.0 + 0.002 * rng.standard_normal((H, W))).astype(F)
        for nm, d in pats.items():
            cases.append(dict(name="%s_%dx%d" % (nm, H, W), depth=np.ascontiguousarray(d), zfar=2.0 if nm == "special_values" else 100.0,
                              targets=nm, ties=[]))
        d, marks = _ratio_tie_frame(H, W, 100.0)
        if marks:
            cases.append(dict(name="ratio_ties_%dx%d" % (H, W), depth=d, zfar=100.0, targets="bad / total == ratio_thres exactly", ties=marks))
    return cases


# ------------------------------------------------------------------------------------------------- crop-window poses
def crop_window_cases():
    """-> list of dict(name, K, poses (N,4,4) f32, diameter, ratio, out_size (w, h), targets).  With fx = fy = 512, cx = cy = 320.5,
    t = (0.25, 0.25, 1) and radius = diameter * ratio / 2 = 0.125 the window edges u0 -+ rad = 384.5 / 512.5 are exact half-integer
    ties (half to even: 384 and 512)."""
    K = np.array([[512.0, 0, 320.5], [0, 512.0, 320.5], [0, 0, 1.0]])
    out = []

    def P(ts):
        a = np.tile(np.eye(4, dtype=F), (len(ts), 1, 1))
        a[:, :3, 3] = np.asarray(ts, F)
        return a
    ties = [(0.25, 0.25, 1.0), (-0.25, 0.25, 1.0), (0.25, -0.25, 1.0), (0.251953125, 0.25, 1.0), (0.25, 0.248046875, 1.0),
            (0.5, 0.5, 2.0), (0.125, 0.125, 0.5)]
    out.append(dict(name="half_integer_ties", K=K, poses=P(ties), diameter=0.25, ratio=1.0, out_size=(160, 160),
                    targets="u0 -+ rad and v0 -+ rad exactly on k + 0.5"))
    odd = [(0.1, 0.1, 0.0), (0.1, -0.2, -1.0), (0.0, 0.0, 1e-30), (0.3, 0.2, 1e-6), (0.0, 0.0, 0.0), (0.1, 0.1, 5000.0), (10.0, 5.0, 5000.0),
           (np.nan, 0.0, 1.0), (0.0, 0.0, np.inf)]
    out.append(dict(name="degenerate_depths", K=K, poses=P(odd), diameter=0.17, ratio=1.2, out_size=(160, 160),
                    targets="tz of 0, negative and tiny; a window that collapses (0.17 m at 5 000 m: right == left)"))
    rng = np.random.default_rng(40)
    for N in (0, 1, 257):
        ts = np.c_[rng.uniform(-0.3, 0.3, (N, 2)), rng.uniform(0.3, 3.0, (N, 1))]
        out.append(dict(name="n_%d" % N, K=K_SKEW, poses=P(ts) if N else np.zeros((0, 4, 4), F), diameter=0.21, ratio=1.1,
                        out_size=(104, 300), targets="N = %d, K with skew, 300 x 104 crop" % N))
    return out
