"""numpy restatement of fp_tsdf_label_components (include/fp_amd.h has the definition) and of the kept-mesh filter of
ops.tsdf_extract(keep=...): min-label propagation over the six face neighbours until nothing changes, then the filter on top of
tsdf_model's extraction.  The `wrong` switches restate the definition with one deliberate mistake each, for the tests that show the
checks can tell.  Also: the generated `counts` arrays the host and the GPU tests share, and the ball that is written into the can's
volume as a floater."""
import itertools

import numpy as np

import tsdf_model as tm

f32 = np.float32
FACES = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
ALL26 = [d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0)]       # one of each opposite pair


def cube_shape(dims):
    nz, ny, nx = (int(d) for d in dims)
    return max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0)


def _pairs(shape, d):
    """the slices of a (mz, my, mx) array that pair every cube with its neighbour at offset d = (dz, dy, dx)"""
    a, b = [], []
    for n, k in zip(shape, d):
        a.append(slice(max(-k, 0), n - max(k, 0)))
        b.append(slice(max(k, 0), n - max(-k, 0)))
    return tuple(a), tuple(b)


def label(counts, dims, wrong=None, sweeps=None):
    """-> labels, sizes (int32, flat, one per cube).  wrong: None | '26' | 'max_label' | 'cube_sizes'.  sweeps: a list that receives
    how many sweeps it took."""
    shape = cube_shape(dims)
    n = shape[0] * shape[1] * shape[2]
    counts = np.asarray(counts, np.int32).reshape(shape)
    active = counts > 0
    none = -1 if wrong == "max_label" else n          # what an inactive cube holds while the labels spread
    lab = np.where(active, np.arange(n, dtype=np.int64).reshape(shape), none)
    pick = np.maximum if wrong == "max_label" else np.minimum
    offsets = ALL26 if wrong == "26" else FACES
    k = 0
    while n:
        k += 1
        before = lab.copy()
        for d in offsets:
            a, b = _pairs(shape, d)
            both = active[a] & active[b]
            m = pick(lab[a], lab[b])
            lab[a] = np.where(both, m, lab[a])
            lab[b] = np.where(both, pick(m, lab[b]), lab[b])      # the two views overlap: never undo what the line above spread
        if np.array_equal(lab, before):
            break
    if sweeps is not None:
        sweeps.append(k)
    labels = np.where(active, lab, -1).reshape(-1).astype(np.int32)
    sizes = np.zeros(n, np.int64)
    on = labels >= 0
    np.add.at(sizes, labels[on], 1 if wrong == "cube_sizes" else counts.reshape(-1)[on])
    return labels, sizes.astype(np.int32)


def choose(labels, sizes, keep, wrong=None):
    """-> (the labels of the components `keep` keeps, ascending; the sizes of all components, descending).  keep: 'largest' | int >= 1.
    wrong: None | 'ties_high'."""
    roots = np.nonzero(sizes > 0)[0]
    tri = sizes[roots].astype(np.int64)
    report = sorted((int(x) for x in tri), reverse=True)
    if keep == "largest":
        if not len(roots):
            return roots, report
        best = np.nonzero(tri == tri.max())[0]
        return roots[[best[-1] if wrong == "ties_high" else best[0]]], report
    if len(roots) and tri.max() < keep:
        raise ValueError(f"keep={keep} triangles, the largest component has {int(tri.max())}")
    return roots[tri >= keep], report


def extract_kept(vol, keep, min_weight=1.0, wrong=None):
    """the kept mesh of ops.tsdf_extract(keep=...) -> dict(pos, col, nrm (U,3) float32, faces (T,3) int64, components,
    dropped_triangles, labels, sizes)"""
    counts = tm.count_triangles(vol, min_weight)
    labels, sizes = label(counts, vol.dims, wrong)
    kept, report = choose(labels, sizes, keep, wrong)
    keys, pos, col, nrm = tm.emit_triangles(vol, min_weight)
    rows = np.repeat(np.repeat(np.isin(labels, kept), counts), 3)
    p, c, n, faces = tm.weld(keys[rows], pos[rows], col[rows], nrm[rows])
    return dict(pos=p, col=c, nrm=n, faces=faces, components=report, dropped_triangles=int(counts.sum()) - len(faces), labels=labels,
                sizes=sizes)


def partition(labels):
    """the components as a canonical list of index arrays (for comparing two labellings whatever their label values)"""
    labels = np.asarray(labels).reshape(-1)
    on = np.nonzero(labels >= 0)[0]
    order = on[np.argsort(labels[on], kind="stable")]
    cuts = np.nonzero(np.diff(labels[order]))[0] + 1
    return sorted((tuple(np.sort(g)) for g in np.split(order, cuts) if len(g)), key=lambda g: g[0])


# ------------------------------------------------------------------ generated counts
BIG = (33, 20, 9)             # 32 x 19 x 8 cubes: a wave of 64 lanes covers eight rows of cubes
LONG = (3, 4, 131)            # 2 x 3 x 130 cubes: a row of cubes crosses two wave ends


def serpentine(dims):
    """one chain through the volume: every other row of cubes of every other layer, whole, joined at alternating ends through one
    cube of the row (or the layer) between them -- a chain needs inactive cubes beside it, so this is the longest the size allows up
    to those"""
    mz, my, mx = cube_shape(dims)
    a = np.zeros((mz, my, mx), bool)
    end = 0                                           # the x at which the chain leaves the current row
    for z in range(0, mz, 2):
        ys = list(range(0, my, 2))
        if (z // 2) % 2:
            ys.reverse()
        for i, y in enumerate(ys):
            a[z, y, :] = True
            end = mx - 1 - end
            if i + 1 < len(ys):
                a[z, (y + ys[i + 1]) // 2, end] = True
        if z + 2 < mz:
            a[z + 1, ys[-1], end] = True
    return a


def generated_cases():
    """-> list of (name, dims, counts (int32, flat))"""
    rng = np.random.default_rng(7)
    out = []

    def add(name, dims, active, values=None):
        shape = cube_shape(dims)
        active = np.broadcast_to(np.asarray(active, bool), shape)
        v = rng.integers(1, 13, shape) if values is None else np.broadcast_to(values, shape)
        out.append((name, tuple(dims), np.where(active, v, 0).astype(np.int32).reshape(-1)))

    add("one cube", (2, 2, 2), True)
    add("one cube, not active", (2, 2, 2), False)
    add("a dimension of 1", (5, 1, 7), False)
    for dims in ((2, 2, 9), (3, 3, 3), BIG, LONG):
        tag = "x".join(str(d) for d in dims)
        shape = cube_shape(dims)
        for density in (0.1, 0.3, 0.6):
            add(f"{tag} density {density}", dims, rng.random(shape) < density)
        add(f"{tag} all active", dims, True)
        add(f"{tag} none active", dims, False)
        z, y, x = np.indices(shape)
        add(f"{tag} checkerboard", dims, (x + y + z) % 2 == 0)
    add("serpentine", BIG, serpentine(BIG))
    # every value a cube can hold, and values that are not counts at all (negative: not active)
    shape = cube_shape(BIG)
    ramp = (np.arange(shape[0] * shape[1] * shape[2]).reshape(shape) % 14) - 1
    out.append(("counts -1..12", BIG, ramp.astype(np.int32).reshape(-1)))
    name, dims, counts = equal_sizes_case()
    out.append((name, dims, counts))
    return out


def equal_sizes_case():
    """two components of 7 triangles each: cubes 0 and 1 (3 + 4) and cube 5 (7)"""
    dims = (2, 2, 8)
    counts = np.zeros(7, np.int32)
    counts[[0, 1, 5]] = [3, 4, 7]
    return "two components of equal size", dims, counts


def edge_contact_case():
    """two cubes that share an edge only: (cx, cy, cz) = (0, 0, 0) and (1, 1, 0)"""
    counts = np.zeros((2, 2, 2), np.int32)
    counts[0, 0, 0], counts[0, 1, 1] = 2, 5
    return (3, 3, 3), counts.reshape(-1)


def corner_contact_case():
    """two cubes that share a corner only: (0, 0, 0) and (1, 1, 1)"""
    counts = np.zeros((2, 2, 2), np.int32)
    counts[0, 0, 0], counts[1, 1, 1] = 2, 5
    return (3, 3, 3), counts.reshape(-1)


# ------------------------------------------------------------------ the floater
BALL_RADIUS, BALL_CENTRE, BALL_REACH = 2.2, (3, 3, 3), 4.0         # voxels; centre as (ix, iy, iz)


def ball_footprint(dims, centre=BALL_CENTRE, reach=BALL_REACH):
    """-> (linear voxel indices within `reach` voxels of the centre, their distances in voxels).  reach = 4 holds both ends of every
    tetrahedron edge that crosses the ball's surface (a cube diagonal from a voxel inside 2.2 ends below 2.2 + sqrt(3) = 3.93); the
    centre is 3 voxels from the volume's faces, so the ball (inside up to 2 voxels from it) closes inside the volume."""
    nz, ny, nx = dims
    i = np.arange(nz * ny * nx, dtype=np.int64)
    ix, iy, iz = i % nx, i // nx % ny, i // (nx * ny)
    d = np.sqrt(((ix - centre[0]) ** 2 + (iy - centre[1]) ** 2 + (iz - centre[2]) ** 2).astype(np.float64))
    at = np.nonzero(d < reach)[0]
    return at, d[at]


def ball_values(dist, trunc_voxels=tm.CAN_TRUNC_VOXELS):
    """the signed distance to the ball in units of trunc, float32"""
    return ((dist - BALL_RADIUS) / trunc_voxels).astype(f32)
