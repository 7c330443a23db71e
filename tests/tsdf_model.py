"""numpy restatement of fp_tsdf_integrate / fp_tsdf_count_triangles / fp_tsdf_emit_triangles (include/fp_amd.h has the definition):
every value is a float32 array operation, one rounding each, in the order the header writes.  The marching-tetrahedra table is built
here by the rule csrc/gen_tsdf_tables.py follows (tests/test_tsdf_host.py compares the two, which guards the committed header against
edits, not the rule; the rule and the winding are checked by the sphere test: closed, Euler characteristic 2, positive volume).  The `wrong` switches restate the
definition with one deliberate mistake each, for the tests that show the checks can tell.  Also: the mesh checks the tests share
(closedness, Euler characteristic, signed volume), the generated views of the bit-equality tests and the can's reference views."""
import itertools

import numpy as np

f32 = np.float32
PERMS = list(itertools.permutations(range(3)))      # lexicographic


# ------------------------------------------------------------------ the volume
class Volume:
    def __init__(self, dims, origin, voxel, trunc):
        self.nz, self.ny, self.nx = (int(d) for d in dims)
        self.origin = np.asarray(origin, dtype=f32).reshape(3)
        self.voxel, self.trunc = f32(voxel), f32(trunc)
        n = self.nz * self.ny * self.nx
        self.tsdf = np.ones(n, f32)
        self.weight = np.zeros(n, f32)
        self.color = np.zeros((n, 3), f32)
        self.color_weight = np.zeros(n, f32)

    @property
    def dims(self):
        return self.nz, self.ny, self.nx

    def copy(self):
        v = Volume(self.dims, self.origin, self.voxel, self.trunc)
        v.tsdf, v.weight, v.color, v.color_weight = self.tsdf.copy(), self.weight.copy(), self.color.copy(), self.color_weight.copy()
        return v

    def arrays(self):
        return dict(tsdf=self.tsdf, weight=self.weight, color=self.color, color_weight=self.color_weight)

    def coords(self):
        """(ix, iy, iz) int64 of every voxel in linear order"""
        i = np.arange(self.nz * self.ny * self.nx, dtype=np.int64)
        return i % self.nx, i // self.nx % self.ny, i // (self.nx * self.ny)

    def positions(self):
        ix, iy, iz = self.coords()
        o, s = self.origin, self.voxel
        return o[0] + ix.astype(f32) * s, o[1] + iy.astype(f32) * s, o[2] + iz.astype(f32) * s


def integrate(vol, depth, rgb, masks, ob_in_cams, Ks, min_depth=0.001, wrong=None, stats=None):
    """fuses the views into vol in place.  depth (V,H,W) f32, rgb (V,H,W,3) f32, masks (V,H,W) uint8 | None, ob_in_cams (V,4,4) f32,
    Ks (V,3,3) f64.  wrong: None | 'round' (half-to-even in place of floor(x + 0.5)) | 'no_trunc_skip'.  stats: a dict that receives
    how many (view, voxel) pairs took each way through the definition."""
    depth, rgb = np.asarray(depth, f32), np.asarray(rgb, f32)
    V, H, W = depth.shape
    poses = np.asarray(ob_in_cams, f32).reshape(V, 16)
    Ks = np.asarray(Ks, np.float64).reshape(V, 9)
    px, py, pz = vol.positions()
    trunc, min_depth, one = vol.trunc, f32(min_depth), f32(1)
    f, w, c, cw = vol.tsdf, vol.weight, vol.color, vol.color_weight
    st = stats if stats is not None else {}
    for k in ("bad_view", "behind", "outside", "half", "empty", "hole", "nan_depth", "neg_depth", "below_min", "hidden", "on_trunc",
              "ulp_past_trunc", "fused", "coloured"):
        st.setdefault(k, 0)
    with np.errstate(all="ignore"):
        for v in range(V):
            T = poses[v]
            K = Ks[v].astype(f32)
            fx, skew, cx, fy, cy = K[0], K[1], K[2], K[4], K[5]
            if not (np.isfinite(T).all() and np.isfinite([fx, fy, cx, cy]).all() and skew == 0):
                st["bad_view"] += 1
                continue
            X = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3]
            Y = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7]
            Z = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11]
            live = Z > 0
            st["behind"] += int((~live).sum())
            xu, xv = (fx * X) / Z + cx, (fy * Y) / Z + cy
            if wrong == "round":
                uf, vf = np.round(xu), np.round(xv)
            else:
                uf, vf = np.floor(xu + f32(0.5)), np.floor(xv + f32(0.5))
            inside = (uf >= 0) & (uf < f32(W)) & (vf >= 0) & (vf < f32(H))
            st["outside"] += int((live & ~inside).sum())
            live &= inside
            st["half"] += int((live & ((xu - np.floor(xu) == f32(0.5)) | (xv - np.floor(xv) == f32(0.5)))).sum())
            ui = np.where(live, uf, 0).astype(np.int64)
            vi = np.where(live, vf, 0).astype(np.int64)
            obj = np.ones(live.shape, bool) if masks is None else masks[v][vi, ui] != 0
            d = depth[v][vi, ui]
            good = d >= min_depth
            st["empty"] += int((live & ~obj).sum())
            st["hole"] += int((live & obj & (d == 0)).sum())
            st["nan_depth"] += int((live & obj & np.isnan(d)).sum())
            st["neg_depth"] += int((live & obj & (d < 0)).sum())
            st["below_min"] += int((live & obj & (d > 0) & ~good).sum())
            sdf = d - Z
            hidden = sdf < -trunc
            st["hidden"] += int((live & obj & good & hidden).sum())
            st["on_trunc"] += int((live & obj & good & (sdf == -trunc)).sum())
            st["ulp_past_trunc"] += int((live & obj & good & (sdf == np.nextafter(-trunc, f32(-9)))).sum())
            if wrong == "no_trunc_skip":
                hidden = np.zeros_like(hidden)
            q = sdf / trunc
            obs = np.where(obj, np.where(q < one, q, one), one).astype(f32)
            upd = live & (~obj | (good & ~hidden))
            f[upd] = ((f * w + obs) / (w + one))[upd]
            w[upd] = (w + one)[upd]
            col = upd & obj & (np.abs(sdf) <= trunc)
            if col.any():
                px_rgb = rgb[v][vi[col], ui[col]]
                d1 = cw[col] + one
                c[col] = (c[col] * cw[col][:, None] + px_rgb) / d1[:, None]
                cw[col] = d1
            st["fused"] += int(upd.sum())
            st["coloured"] += int(col.sum())
    return vol


# ------------------------------------------------------------------ marching tetrahedra
def tet_corners(p):
    c = np.zeros((4, 3), np.int64)
    for k, axis in enumerate(p):
        c[k + 1:, axis] += 1
    return c


def perm_odd(p):
    return sum(p[i] > p[j] for i in range(3) for j in range(i + 1, 3)) % 2


def case_table():
    """per case 0..15 (bit k: corner k inside) the triangles as three tetrahedron edges (i, j), i < j, wound so that for a tetrahedron
    with det(p1-p0, p2-p0, p3-p0) > 0 the normal (v1-v0) x (v2-v0) points from the inside corners to the outside ones"""
    P = tet_corners((0, 1, 2)).astype(np.float64)
    assert np.linalg.det(P[1:] - P[0]) > 0
    table = []
    for case in range(16):
        ins = [k for k in range(4) if case >> k & 1]
        out = [k for k in range(4) if not case >> k & 1]
        tris = []
        if len(ins) == 1:
            tris = [[(ins[0], o) for o in out]]
        elif len(ins) == 3:
            tris = [[(i, out[0]) for i in ins]]
        elif len(ins) == 2:
            quad = [(ins[0], out[0]), (ins[0], out[1]), (ins[1], out[1]), (ins[1], out[0])]
            tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
        fixed = []
        for t in tris:
            mid = [(P[a] + P[b]) / 2 for a, b in t]
            if np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), P[out].mean(0) - P[ins].mean(0)) < 0:
                t = [t[0], t[2], t[1]]
            fixed.append(tuple((min(e), max(e)) for e in t))
        table.append(fixed)
    return table


CASES = case_table()


def _gradient(vol):
    """(n,3) float32: per axis 0.5 * (f[i+1] - f[i-1]) inside, one-sided at the faces (0 along an axis of one voxel)"""
    f = vol.tsdf.reshape(vol.dims)
    g = np.zeros(f.shape + (3,), f32)
    for axis, comp in ((2, 0), (1, 1), (0, 2)):
        if f.shape[axis] < 2:
            continue
        m = np.moveaxis(f, axis, 0)
        o = np.empty_like(m)
        o[1:-1] = f32(0.5) * (m[2:] - m[:-2])
        o[0] = m[1] - m[0]
        o[-1] = m[-1] - m[-2]
        g[..., comp] = np.moveaxis(o, 0, axis)
    return g.reshape(-1, 3)


def _cube_walk(vol, min_weight, wrong):
    """the surface triangles in output order -> (cube (T,), corners a and b of the 3 edges as voxel coordinates (T,3,3) each)"""
    nz, ny, nx = vol.dims
    if min(nz, ny, nx) < 2:
        return np.zeros(0, np.int64), np.zeros((0, 3, 3), np.int64), np.zeros((0, 3, 3), np.int64)
    c = np.arange((nz - 1) * (ny - 1) * (nx - 1), dtype=np.int64)
    base = np.stack([c % (nx - 1), c // (nx - 1) % (ny - 1), c // ((nx - 1) * (ny - 1))], 1)        # (C,3) x, y, z
    inside_of = (vol.tsdf <= 0) if wrong == "le" else (vol.tsdf < 0)
    seen_of = vol.weight >= f32(min_weight)
    lin = lambda p: (p[..., 2] * ny + p[..., 1]) * nx + p[..., 0]     # noqa: E731
    order, A, B = [], [], []
    for t, perm in enumerate(PERMS):
        offs = tet_corners(perm)
        corners = base[:, None, :] + offs[None]                    # (C,4,3)
        odd = np.full(len(c), perm_odd(perm))
        if wrong == "split":                                          # mirror the split along x in every other row of cubes
            flip = base[:, 1] % 2 == 1
            corners[flip, :, 0] = (base[flip, 0] + 1)[:, None] - offs[None, :, 0]
            odd = odd ^ flip
        li = lin(corners)
        case = (inside_of[li] << np.arange(4)).sum(1)
        valid = seen_of[li].all(1)
        for cs in range(1, 15):
            sel = np.nonzero(valid & (case == cs))[0]
            if not len(sel):
                continue
            for j, tri in enumerate(CASES[cs]):
                e = np.asarray(tri)                                   # (3,2)
                ea = np.where(odd[sel][:, None] == 1, e[[0, 2, 1], 0][None], e[:, 0][None])        # (S,3) tetrahedron corner ids
                eb = np.where(odd[sel][:, None] == 1, e[[0, 2, 1], 1][None], e[:, 1][None])
                pa = np.take_along_axis(corners[sel], ea[:, :, None].repeat(3, 2), 1)              # (S,3,3)
                pb = np.take_along_axis(corners[sel], eb[:, :, None].repeat(3, 2), 1)
                swap = lin(pa) > lin(pb)                                                           # a = the smaller linear index
                pa2 = np.where(swap[..., None], pb, pa)
                pb2 = np.where(swap[..., None], pa, pb)
                order.append(sel * 12 + t * 2 + j)
                A.append(pa2)
                B.append(pb2)
    if not order:
        return np.zeros(0, np.int64), np.zeros((0, 3, 3), np.int64), np.zeros((0, 3, 3), np.int64)
    order, A, B = np.concatenate(order), np.concatenate(A), np.concatenate(B)
    k = np.argsort(order, kind="stable")
    return order[k] // 12, A[k], B[k]


def count_triangles(vol, min_weight=1.0, wrong=None):
    nz, ny, nx = vol.dims
    cube, _, _ = _cube_walk(vol, min_weight, wrong)
    return np.bincount(cube, minlength=max(nz - 1, 0) * max(ny - 1, 0) * max(nx - 1, 0)).astype(np.int32)


def emit_triangles(vol, min_weight=1.0, wrong=None):
    """-> keys (3T,) int64, pos, col, nrm (3T,3) float32, in output order"""
    nz, ny, nx = vol.dims
    _, A, B = _cube_walk(vol, min_weight, wrong)
    A, B = A.reshape(-1, 3), B.reshape(-1, 3)
    a = (A[:, 2] * ny + A[:, 1]) * nx + A[:, 0]
    b = (B[:, 2] * ny + B[:, 1]) * nx + B[:, 0]
    keys = (a << 32) | b
    o, s = vol.origin, vol.voxel
    pa, pb = o[None] + A.astype(f32) * s, o[None] + B.astype(f32) * s
    fa, fb = vol.tsdf[a], vol.tsdf[b]
    g = _gradient(vol)
    with np.errstate(all="ignore"):
        if wrong == "from_b":
            t = (fb / (fb - fa))[:, None]
            lerp = lambda x, y: y + t * (x - y)      # noqa: E731
        else:
            t = (fa / (fa - fb))[:, None]
            lerp = lambda x, y: x + t * (y - x)      # noqa: E731
        pos = lerp(pa, pb)
        ha, hb = (vol.color_weight[a] > 0)[:, None], (vol.color_weight[b] > 0)[:, None]
        ca, cb = np.where(ha, vol.color[a], f32(128)), np.where(hb, vol.color[b], f32(128))
        col = np.where(ha & hb, lerp(ca, cb), np.where(ha, ca, cb))
        gn = lerp(g[a], g[b])
        ln = np.sqrt((gn[:, 0] * gn[:, 0] + gn[:, 1] * gn[:, 1]) + gn[:, 2] * gn[:, 2])[:, None]
        nrm = np.where(ln > 0, gn / ln, np.asarray([0, 0, 1], f32)[None])
    return keys.astype(np.int64), pos.astype(f32), col.astype(f32), nrm.astype(f32)


def weld(keys, pos, col, nrm):
    """vertices in the order of their sorted keys -> pos, col, nrm (U,3), faces (T,3) int64"""
    uk, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    return pos[first], col[first], nrm[first], inv.reshape(-1, 3).astype(np.int64)


def extract(vol, min_weight=1.0, wrong=None):
    return weld(*emit_triangles(vol, min_weight, wrong))


# ------------------------------------------------------------------ what a mesh is checked for
def edge_report(faces):
    """(directed edges whose reverse does not occur exactly once or that occur more than once, undirected edges, Euler characteristic
    V - E + F over the vertices the faces use)"""
    f = np.asarray(faces, np.int64)
    if not len(f):
        return 0, 0, 0
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1
    code, rev = d[:, 0] * n + d[:, 1], d[:, 1] * n + d[:, 0]
    uc, cnt = np.unique(code, return_counts=True)
    bad = int((cnt != 1).sum()) + int((~np.isin(rev, code)).sum())
    und = np.unique(np.minimum(code, rev))
    return bad, len(und), len(np.unique(f)) - len(und) + len(f)


def repeated_vertex_faces(faces):
    f = np.asarray(faces)
    return int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum()) if len(f) else 0


def signed_volume(pos, faces):
    p = np.asarray(pos, np.float64)
    p = p - p.mean(0)
    a, b, c = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def cylinder_distance(p, radius, height):
    """distance of points to the surface of the closed cylinder about z, centred at the origin (float64)"""
    p = np.asarray(p, np.float64)
    dr = np.hypot(p[:, 0], p[:, 1]) - radius
    dz = np.abs(p[:, 2]) - height / 2
    outside = np.hypot(np.maximum(dr, 0), np.maximum(dz, 0))
    inside = np.minimum(np.maximum(dr, dz), 0)
    return np.abs(outside + inside)


# ------------------------------------------------------------------ generated views of the bit-equality tests
def generated_case(dims, V, H, W, kvariant=0, seed=0, with_masks=True):
    """A volume of pitch 2^-7 m whose plane iz = 1 lies at camera z = 2^-4 of view 0, and V views of a slab of depth around it.
    View 0 looks straight down z with fx = fy = 8 and cx, cy on .5: every voxel of that plane projects exactly on x.5 (u = ix + cx).
    Its depth image holds, at fixed pixels, a hole, a NaN, a negative, a depth just below min_depth, and depths that put sdf exactly
    on -trunc and one ulp of sdf beyond it for the voxels of the plane (2^-5 and 2^-5 - 2^-28 under z = 2^-4: both differences are
    exact).  The other views are seeded poses around the volume (some voxels
    behind the camera, many outside the small frames); view 2 (when there is one) has a NaN in its pose.  -> dict."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = dims
    s, trunc = f32(2.0 ** -7), f32(2.0 ** -5)
    origin = np.asarray([-(nx // 2) * s, -(ny // 2) * s, -s], f32)
    min_depth, zp = f32(2.0 ** -6), f32(2.0 ** -4)
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
            # every third view stands inside the volume: voxels behind it
            poses[v, :3, 3] = [rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 0.02 if v % 3 == 1 else rng.uniform(0.3, 0.6)]
        zc = float(poses[v, 2, 3])
        depth[v] = (zc + rng.uniform(-1.5, 1.5, (H, W)) * float(trunc)).astype(f32)
    r = rng.random((V, H, W))
    depth[r < 0.04] = 0.0
    depth[(r >= 0.04) & (r < 0.06)] = np.nan
    depth[(r >= 0.06) & (r < 0.08)] = -0.4
    depth[(r >= 0.08) & (r < 0.10)] = np.nextafter(min_depth, f32(0))
    # view 0, the row of pixels the voxels (ix, iy = ny // 2, iz = 1) land on: u = ix - nx // 2 + W // 2 + 1, v = H // 2 + 1
    row, u0 = H // 2 + 1, W // 2 + 1 - nx // 2
    special = [zp - trunc, f32(zp - trunc - f32(2.0 ** -28)), f32(0.0), f32(np.nan), f32(-0.4), np.nextafter(min_depth, f32(0)), zp, zp + trunc]
    for k, val in enumerate(special):
        u = u0 + k
        if 0 <= u < W and 0 <= row < H and k < nx:
            depth[0, row, u] = val
    masks = None
    if with_masks:
        masks = (rng.random((V, H, W)) < 0.8).astype(np.uint8) * np.uint8(255 if seed % 2 else 1)
        if 0 <= row < H:
            masks[0, row, max(u0, 0):max(u0, 0) + len(special)] = 1
    if V >= 3:
        poses[2, 1, 2] = np.nan
    rgb = rng.uniform(0, 255, (V, H, W, 3)).astype(f32)
    return dict(dims=dims, origin=origin, voxel=s, trunc=trunc, min_depth=min_depth, depth=depth, rgb=rgb, masks=masks, ob_in_cams=poses,
                Ks=Ks)


def fuse_case(case, wrong=None, stats=None, views=None):
    vol = Volume(case["dims"], case["origin"], case["voxel"], case["trunc"])
    sl = slice(None) if views is None else views
    m = None if case["masks"] is None else case["masks"][sl]
    return integrate(vol, case["depth"][sl], case["rgb"][sl], m, case["ob_in_cams"][sl], case["Ks"][sl], case["min_depth"], wrong, stats)


# ------------------------------------------------------------------ the can
CAN_RADIUS, CAN_HEIGHT = 0.051, 0.140
CAN_VOXEL, CAN_TRUNC_VOXELS, CAN_DIMS = 0.0025, 4, (64, 48, 48)


def can_view_poses(n=16, distance=0.5):
    """object-in-camera poses (n,4,4) float64 of the can's reference views: spread evenly over the icosphere at `distance`"""
    from foundationpose_amd.synthetic import reference_view_poses
    return reference_view_poses(n, distance)


def can_volume_spec():
    """origin, dims (nz, ny, nx), voxel, trunc of the can's volume at 2.5 mm: 48 x 48 x 64 voxels centred on the can, which leaves
    three voxels around it"""
    s = CAN_VOXEL
    nz, ny, nx = CAN_DIMS
    lo = -np.asarray([nx - 1, ny - 1, nz - 1]) * s / 2
    return lo.astype(f32), CAN_DIMS, f32(s), f32(CAN_TRUNC_VOXELS * s)
