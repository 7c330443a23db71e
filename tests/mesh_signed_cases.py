"""Generated cases of fp_mesh_pseudonormals, fp_mesh_signed_distance and fp_mesh_penetration.  A case is dict(name, pos (Nv,3) float32,
faces (F,3) int32, points (Q,3) float32, group (Q,) int8, extent): closed, outward-oriented meshes in seeded random rigid poses, and
queries in groups: RANDOM uniform in 1.5 x the bounding box; DIRECTED at 1e-3 of the extent inside and outside along every vertex's
pseudonormal, along every edge's bisector over its midpoint and over every face's centroid; ON the surface (a vertex, an edge
midpoint, a face centroid); NONFINITE; PROBE extra points of a case's own.  The host tests run the restatement
(tests/mesh_signed_model.py) over them and hold its sign to the solid-angle answer; the GPU tests hold the kernels to the restatement.

A closed triangle mesh has an even number of faces (3 F = 2 E), so the subdivided boxes with an odd face count carry one zero-area
face (0, 0, 0) at the end, which the tables leave out."""
import functools

import numpy as np

import mesh_signed_model as sm

f32 = np.float32
RANDOM, DIRECTED, ON, NONFINITE, PROBE = 0, 1, 2, 3, 4
DIRECTED_STEP = 1e-3            # of the extent
DIRECTED_MAX = 2400             # a mesh with more directed points than this keeps a seeded choice of so many (the restated calls stay
                                # below 2e7 pair tests); every mesh of up to 257 faces keeps them all
Q_SIZES = (1, 255, 256, 257, 1000)
CAN_RADIUS, CAN_HEIGHT, CAN_SIDES = 0.033, 0.123, 50

_BOX_V = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64)     # index = x + 2 y + 4 z (bits)
_BOX_QUADS = ((0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5))  # outward, counter-clockwise


def box(half=(0.5, 0.5, 0.5)):
    faces = [t for q in _BOX_QUADS for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return _BOX_V * np.asarray(half, np.float64), np.asarray(faces, np.int64)


def tetrahedron():
    pos = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * 0.4
    return pos, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int64)


def _extrude(poly, cap_tris, h):
    """a counter-clockwise polygon (n,2) with a triangulation of its inside, extruded from z = 0 to h"""
    n = len(poly)
    pos = np.concatenate([np.column_stack([poly, np.zeros(n)]), np.column_stack([poly, np.full(n, h)])])
    faces = [(c, b, a) for a, b, c in cap_tris] + [(a + n, b + n, c + n) for a, b, c in cap_tris]
    for i in range(n):
        j = (i + 1) % n
        faces += [(i, j, j + n), (i, j + n, i + n)]
    return pos, np.asarray(faces, np.int64)


def l_prism():
    """an L: the reflex edge runs through corner 3, whose two end vertices are reflex vertices"""
    poly = np.array([[0, 0], [1, 0], [1, 0.4], [0.4, 0.4], [0.4, 1], [0, 1]], np.float64)
    return _extrude(poly, [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)], 0.5)


def prism(sides=CAN_SIDES, radius=CAN_RADIUS, height=CAN_HEIGHT):
    """the can: a regular prism, caps fanned from a centre vertex"""
    a = 2 * np.pi * np.arange(sides) / sides
    ring = np.column_stack([radius * np.cos(a), radius * np.sin(a)])
    pos = np.concatenate([np.column_stack([ring, np.zeros(sides)]), np.column_stack([ring, np.full(sides, height)]),
                          [[0, 0, 0], [0, 0, height]]])
    faces = []
    for i in range(sides):
        j = (i + 1) % sides
        faces += [(i, j, j + sides), (i, j + sides, i + sides), (2 * sides, j, i), (2 * sides + 1, i + sides, j + sides)]
    return pos, np.asarray(faces, np.int64)


def icosphere(radius=0.5):
    """an icosahedron subdivided once: 80 faces"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    mid = {}

    def m(a, b):
        k = (min(a, b), max(a, b))
        if k not in mid:
            x = v[a] + v[b]
            v.append(x / np.linalg.norm(x))
            mid[k] = len(v) - 1
        return mid[k]
    out = []
    for a, b, c in f:
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    return np.asarray(v) * radius, np.asarray(out, np.int64)


def torus(nu=16, nv=8, R=0.4, r=0.15):
    """nu x nv quads, 2 nu nv = 256 faces; the vertices on the inner equator are saddles"""
    u, w = np.meshgrid(2 * np.pi * np.arange(nu) / nu, 2 * np.pi * np.arange(nv) / nv, indexing="ij")
    pos = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], axis=2).reshape(-1, 3)
    faces = []
    for i in range(nu):
        for j in range(nv):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            faces += [(a, b, c), (a, c, d)]
    return pos, np.asarray(faces, np.int64)


def unwelded(pos, faces):
    """OBJ style: every face has its own three vertices"""
    return pos[faces.reshape(-1)], np.arange(3 * len(faces)).reshape(-1, 3)


def subdivided_box(F):
    """a box whose largest face is split at its centroid (one face becomes three) until it has F faces; an odd F gets one zero-area
    face (0, 0, 0) at the end"""
    pos, faces = box((0.5, 0.4, 0.3))
    pos, faces = [p for p in pos], [tuple(f) for f in faces]
    area = [0.5 * np.linalg.norm(np.cross(pos[b] - pos[a], pos[c] - pos[a])) for a, b, c in faces]
    while len(faces) + 2 <= F:
        k = int(np.argmax(area))
        a, b, c = faces[k]
        pos.append((pos[a] + pos[b] + pos[c]) / 3)
        n = len(pos) - 1
        faces[k] = (a, b, n)
        faces += [(b, c, n), (c, a, n)]
        area[k] = area[k] / 3
        area += [area[k], area[k]]
    if len(faces) < F:
        faces.append((0, 0, 0))
    return np.asarray(pos), np.asarray(faces, np.int64)


FAN_SLIVERS = 20


def fan_box():
    """a unit box whose top face is a fan of 20 slivers from corner 4, to 9 points on each of the two far edges; the two side faces
    that own those edges are fanned to the same points from their far bottom corners.  Corner 4 carries 20 tiny angles of the top face
    beside one right angle of each of two side faces.  (A box's face normals are orthogonal, so every positive combination of them
    has the right sign over the corner's whole region: uniform weights bend this corner's normal but cannot turn a sign here.  The
    case where they do is fan_spike.)"""
    pos, _ = box()
    pos = [p for p in pos]

    def between(a, b, n):
        out = []
        for k in range(1, n + 1):
            pos.append(pos[a] + (pos[b] - pos[a]) * k / (n + 1))
            out.append(len(pos) - 1)
        return out
    n = (FAN_SLIVERS - 2) // 2
    e57, e76 = between(5, 7, n), between(7, 6, n)
    faces = []

    def fan(c, chain):
        faces.extend((c, chain[i], chain[i + 1]) for i in range(len(chain) - 1))
    fan(4, [5] + e57 + [7] + e76 + [6])                 # top (z = +): 4 5 7 6
    fan(1, [3, 7] + e57[::-1] + [5])                    # x = +: 1 3 7 5
    fan(2, [6] + e76[::-1] + [7, 3])                    # y = +: 2 6 7 3
    for q in (_BOX_QUADS[0], _BOX_QUADS[2], _BOX_QUADS[4]):
        faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return np.asarray(pos), np.asarray(faces, np.int64)


def fan_spike():
    """a thin three-sided spike, apex 0 over a small base; the side face (0, 1, 2) is a fan of 20 slivers from the apex to 19 points on
    the base edge 1-2, and the base is fanned to the same points from corner 3.  The side normals are 120 degrees apart, so the apex's
    region is nearly a half space; with uniform weights its normal is the slivered side's, and a point off the apex on another side
    comes out inside."""
    a = 2 * np.pi * np.arange(3) / 3
    pos = [np.array([0.0, 0.0, 1.0])] + [np.array([0.15 * np.cos(x), 0.15 * np.sin(x), 0.0]) for x in a]
    pts = []
    for k in range(1, FAN_SLIVERS):
        pos.append(pos[1] + (pos[2] - pos[1]) * k / FAN_SLIVERS)
        pts.append(len(pos) - 1)
    chain = [1] + pts + [2]
    faces = [(0, chain[i], chain[i + 1]) for i in range(len(chain) - 1)] + [(0, 2, 3), (0, 3, 1)]
    back = chain[::-1]
    faces += [(3, back[i], back[i + 1]) for i in range(len(back) - 1)]
    return np.asarray(pos), np.asarray(faces, np.int64)


def with_zero_area(pos, faces):
    """two zero-area faces on a closed mesh: an edge of face 0 as (a, b, b), and a single vertex three times"""
    a, b, c = faces[0]
    return pos, np.concatenate([faces, [[a, b, b], [c, c, c]]])


def crossed_boxes():
    """the documented counterexample: two closed boxes that cross, as one mesh.  Every edge has two faces, so the report says closed,
    but inside one box and near the part of the other's surface that lies in it the nearest face says "outside"."""
    p0, f0 = box((0.5, 0.2, 0.2))
    p1, f1 = box((0.2, 0.5, 0.2))
    return np.concatenate([p0, p1]), np.concatenate([f0, f1 + len(p0)])


# ------------------------------------------------------------------ defects, for the report
def defects():
    """name -> (pos, faces, the report slots that must be non-zero)"""
    pos, faces = box()
    extra = np.concatenate([pos, [[0.0, 0.0, 2.0]]])
    flipped = faces.copy()
    flipped[3] = flipped[3][::-1]
    outside = faces.copy()
    outside[5, 1] = len(pos)
    return {"two triangles removed": (pos, np.delete(faces, [2, 7], axis=0), ("boundary",)),
            "an edge with three faces": (extra, np.concatenate([faces, [[faces[0][0], faces[0][1], 8]]]), ("nonmanifold", "boundary")),
            "one face flipped": (pos, flipped, ("inconsistent",)),
            "an index outside the table": (pos, outside, ("degenerate", "boundary"))}


# ------------------------------------------------------------------ poses and queries
def rigid(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q, rng.uniform(-0.3, 0.3, 3) * scale


def directed_queries(pos, faces, extent):
    """points at DIRECTED_STEP * extent inside and outside of every welded vertex (along its float64 pseudonormal), of every edge's
    midpoint (along the sum of its faces' normals) and of every face's centroid -> (points (n,3) float64, inside (n,) bool)"""
    p32 = pos.astype(f32)
    vn, en, _ = sm.pseudonormals(p32, faces)
    w = sm.weld(p32)
    pts, ins = [], []
    step = DIRECTED_STEP * extent

    def add(x, n):
        ln = np.linalg.norm(n, axis=1)
        ok = ln > 0
        x, n = x[ok], n[ok] / ln[ok, None]
        pts.extend([x + step * n, x - step * n])
        ins.extend([np.zeros(len(x), bool), np.ones(len(x), bool)])
    heads = np.unique(w[faces[((faces >= 0) & (faces < len(pos))).all(axis=1)]])
    add(p32[heads].astype(np.float64), vn[heads].astype(np.float64))
    good = np.linalg.norm(en.astype(np.float64), axis=2).min(axis=1) > 0
    v = p32[faces[good]].astype(np.float64)
    add(((v + np.roll(v, -1, axis=1)) / 2).reshape(-1, 3), en[good].astype(np.float64).reshape(-1, 3))
    add(v.mean(axis=1), np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]))
    return np.concatenate(pts), np.concatenate(ins)


def _case(name, mesh, seed, Q, scale=1.0, nonfinite=False, probe=None):
    pos, faces = mesh
    R, t = rigid(seed, scale)
    pos = ((np.asarray(pos, np.float64) * scale) @ R.T + t).astype(f32)
    faces = np.asarray(faces, np.int64)
    lo, hi = pos.min(axis=0).astype(np.float64), pos.max(axis=0).astype(np.float64)
    extent = float((hi - lo).max())
    rng = np.random.default_rng(seed + 1000)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    groups = [(RANDOM, c + rng.uniform(-1.5, 1.5, (Q, 3)) * h)]
    d, d_inside = directed_queries(pos, faces, extent)
    if len(d) > DIRECTED_MAX:
        keep = np.sort(rng.choice(len(d), DIRECTED_MAX, replace=False))
        d, d_inside = d[keep], d_inside[keep]
    groups.append((DIRECTED, d))
    f0 = faces[0]
    v = pos[f0].astype(np.float64)
    groups.append((ON, np.array([v[0], (v[0] + v[1]) / 2, v.mean(axis=0)])))
    if nonfinite:
        groups.append((NONFINITE, np.array([[np.nan, 0, 0], [0, np.inf, 0], [-np.inf, 0, 0], [1e30, 1e30, 1e30]])))
    if probe is not None:
        groups.append((PROBE, (np.asarray(probe(pos.astype(np.float64), extent)))))
    points = np.concatenate([g[1] for g in groups]).astype(f32)
    group = np.concatenate([np.full(len(g[1]), g[0], np.int8) for g in groups])
    return dict(name=name, pos=np.ascontiguousarray(pos), faces=np.ascontiguousarray(faces.astype(np.int32)),
                points=np.ascontiguousarray(points), group=group, extent=extent, directed_inside=d_inside)


def _apex_probe(pos, extent):
    """a sphere of directions around the spike's apex (vertex 0), at 2e-3 of the extent"""
    rng = np.random.default_rng(5)
    d = rng.normal(size=(64, 3))
    return pos[0] + 2e-3 * extent * d / np.linalg.norm(d, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def closed_cases():
    """every closed case, built once"""
    out = [_case("box", box(), 1, Q_SIZES[4], nonfinite=True),
           _case("tetrahedron", tetrahedron(), 2, Q_SIZES[1]),
           _case("L-prism", l_prism(), 3, Q_SIZES[2]),
           _case("icosphere 80", icosphere(), 4, Q_SIZES[3]),
           _case("torus 16x8", torus(), 5, Q_SIZES[4]),
           _case("can prism 50", prism(), 6, Q_SIZES[2]),
           _case("box OBJ style", unwelded(*box()), 7, Q_SIZES[1]),
           _case("tetrahedron OBJ style", unwelded(*tetrahedron()), 13, Q_SIZES[2]),
           _case("fan box", fan_box(), 8, Q_SIZES[3]),
           _case("fan spike", fan_spike(), 12, Q_SIZES[1], probe=_apex_probe),
           _case("box with two zero-area faces", with_zero_area(*box()), 9, Q_SIZES[2]),
           _case("icosphere x1e-3", icosphere(), 10, Q_SIZES[0], scale=1e-3),
           _case("torus x50", torus(), 11, Q_SIZES[1], scale=50.0)]
    for i, F in enumerate((255, 256, 257, 1023, 1024, 1025, 3000)):
        out.append(_case(f"subdivided box F={F}", subdivided_box(F), 20 + i, Q_SIZES[i % 5] if F < 3000 else Q_SIZES[3]))
    return tuple(out)


def case(name):
    return next(c for c in closed_cases() if c["name"] == name)


# ------------------------------------------------------------------ penetration: two boxes
def box_pair(overlap, Q=2048, seed=0):
    """a unit cube b at the origin and the surface samples of a unit cube a shifted along x so that the two overlap by `overlap`
    (0: touching; negative: apart) -> (b's pos, b's faces, a's samples (Q,3) float32 in a's frame, the transform (4,4) a -> b)"""
    from mesh_distance_model import sample_surface
    pos, faces = box()
    pos = pos.astype(f32)
    pts, _ = sample_surface(pos, faces, Q, seed)
    tf = np.eye(4)
    tf[0, 3] = 1.0 - overlap
    return pos, faces.astype(np.int32), pts, tf.astype(f32)
