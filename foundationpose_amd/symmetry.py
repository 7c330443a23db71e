"""The rotational symmetries of a mesh, found from how far candidate rotations move its surface off itself.  Host code in float64: the
policy only.  The distances come from two callables, which reconstruct.detect_symmetries binds to the device ops
(ops.mesh_transform_residuals, ops.mesh_point_distance) and the host tests to their numpy restatement, so both drive the same policy.

Only geometry is considered: a can whose label is not symmetric is still reported as symmetric.  Only proper rotations are looked
for (a pose is a proper rotation: a mirror plane is no symmetry here), and at most one continuous axis is described.

The recipe (find_symmetries):
  1. A symmetry of a bounded surface fixes its area-weighted centroid c, so every candidate is [R | c - R c].
  2. n_axes candidate axes on a hemisphere (a Fibonacci spiral) with covering angle delta (every direction is within delta of an axis
     or of its opposite).  Orders k = 2..max_order, and two probe orders above max_order (the next two primes: 7 and 11 for 6); for
     each order only the generator angle theta = 2 pi / k is tested.
  3. Coarse scan: an axis survives at order k if its largest distance on the coarse samples is at most
     tol + 4 sin(theta/2) sin(delta/2) radius (coarse_bound: why no true axis is lost).
  4. Each survivor is refined on the fine samples: closest points of the transformed samples, the best rotation about c that takes the
     samples there (Kabsch), its axis kept and the rotation rebuilt at exactly theta, until the axis moves less than 1e-7 rad.  It is
     accepted if its largest distance on the fine samples is at most tol.
  5. Accepted axes within max(1 degree, 2 tol / radius) of each other, up to sign, are one axis (the one with the smallest residual
     is kept) with all their orders.  The group is the identity and R_axis(2 pi j / k), j = 1..k-1, for every accepted (axis, order),
     without repeats.  In a finite rotation group every element is a power of some axis' generator and the scan over the axes is
     exhaustive, so no closure by products is needed (and none is done: products of slightly wrong axes grow into near-duplicates).
  6. An axis accepted at both probe orders is continuous: rotations every rot_angle_discrete degrees; with a 2-fold axis perpendicular
     to it, those rotations times that one flip as well (every other perpendicular 2-fold is one of these products).  An axis
     accepted at one probe order only is a discrete axis of that order.  Two continuous axes that are not parallel: a ValueError.
  7. Every transform that is returned has been evaluated on the fine samples and is within tol; one that is not is left out.
The group is complete when every axis' order is at most max_order or one of the probe orders."""
import math
from fractions import Fraction
from typing import NamedTuple

import numpy as np

REFINE_STOP_RAD = 1e-7
REFINE_MAX_ITERATIONS = 80


class Symmetries(NamedTuple):
    """tfs (S,4,4) float64, identity first; axes: [(unit axis (3,), order)] with order an int or math.inf for the continuous axis,
    one entry per accepted (axis, order); tol: the length every transform is within; residuals (S,): the largest distance of a fine
    sample under each transform; centre: the point every transform fixes"""
    tfs: np.ndarray
    axes: list
    tol: float
    residuals: np.ndarray
    centre: np.ndarray

    @property
    def continuous_axis(self):
        return next((a for a, k in self.axes if k == math.inf), None)


def surface_centre(pos, faces):
    """the area-weighted centroid of a mesh's surface and the largest distance of a vertex from it, float64.  Faces with an index
    outside the table or without a finite area count for nothing."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < len(pos))).all(axis=1)
    tri = pos[faces[ok]]
    with np.errstate(all="ignore"):
        area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    good = np.isfinite(area) & (area > 0)
    if not good.any():
        raise ValueError("surface_centre: the mesh has no area (no face, or only degenerate ones)")
    tri, area = tri[good], area[good]
    c = (tri.mean(axis=1) * area[:, None]).sum(axis=0) / area.sum()
    used = np.unique(faces[ok][good])
    return c, float(np.linalg.norm(pos[used] - c, axis=1).max())


def axis_rotation(axis, angle):
    """Rodrigues: the rotation by `angle` about the unit vector `axis`, (3,3) float64"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def about(centre, R):
    """[R | c - R c]: the rotation R about the point c, (...,4,4) float64"""
    R = np.asarray(R, np.float64)
    out = np.zeros(R.shape[:-2] + (4, 4))
    out[..., :3, :3] = R
    out[..., :3, 3] = centre - R @ centre
    out[..., 3, 3] = 1.0
    return out


def hemisphere_axes(n):
    """n unit vectors on the hemisphere z >= 0, a Fibonacci spiral: point i at height (i + 0.5) / n, azimuth i times the golden angle"""
    i = np.arange(n, dtype=np.float64)
    z = (i + 0.5) / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def covering_angle(axes, probes=None):
    """An upper bound on the angle from any direction to the nearest of `axes` or their opposites.  Measured on a finer spiral of
    m probe directions, whose own covering angle is added: a spiral of m points on the hemisphere gives each an area of 2 pi / m,
    a cap of that area has the angular radius sqrt(2 / m), and twice that radius is a safe cover for the spiral's cells."""
    m = int(probes) if probes is not None else max(40 * len(axes), 4000)
    p = hemisphere_axes(m)
    worst = 0.0
    for lo in range(0, m, 4096):
        c = np.abs(p[lo:lo + 4096] @ axes.T).max(axis=1)
        worst = max(worst, float(np.arccos(np.clip(c, -1.0, 1.0)).max()))
    return worst + 2.0 * math.sqrt(2.0 / m)


def coarse_bound(theta, delta, radius):
    """How far two rotations by the same angle theta about one centre, whose axes are delta apart, can differ on a point within
    `radius` of the centre: 4 sin(theta/2) sin(delta/2) radius (<= 2 sin(theta/2) delta radius).
    Proof: as unit quaternions the two are (cos t, sin t a) and (cos t, sin t a'), t = theta/2.  The rotation that takes one to the
    other has the scalar part cos^2 t + sin^2 t (a . a') = 1 - u with u = 2 sin^2 t sin^2(delta/2), which is the cosine of half its
    angle phi; so sin^2(phi/2) = 1 - (1 - u)^2 = 2u - u^2 <= 2u, and the two rotations differ on a vector v by at most
    2 sin(phi/2) |v| <= 2 sqrt(2u) |v| = 4 sin t sin(delta/2) |v|.  The distance to a surface is 1-Lipschitz, so an axis within delta
    of a true one has a residual within this of the true one's: a true axis' nearest grid axis survives the coarse scan."""
    return 4.0 * math.sin(0.5 * theta) * math.sin(0.5 * delta) * radius


def _axis_of(R, like):
    """the axis of a rotation matrix, as the eigenvector of its symmetric part for the eigenvalue 1 (well separated from the other two,
    cos(angle), also at a half turn, where the skew part vanishes), signed like `like`"""
    w, v = np.linalg.eigh(0.5 * (R + R.T))
    a = v[:, int(np.argmax(w))]
    return a if a @ like >= 0 else -a


def _kabsch(x, q):
    """the rotation R minimising sum |R x_i - q_i|^2, (3,3)"""
    u, _, vt = np.linalg.svd(x.T @ q)
    d = np.sign(np.linalg.det(vt.T @ u.T))
    return vt.T @ np.diag([1.0, 1.0, d]) @ u.T


def _angle_between_axes(a, b):
    """the angle between two axes up to sign, radians"""
    return math.acos(min(1.0, abs(float(a @ b))))


def _next_primes(above, n=2):
    out, k = [], above + 1
    while len(out) < n:
        if k > 1 and all(k % d for d in range(2, int(math.isqrt(k)) + 1)):
            out.append(k)
        k += 1
    return out


def refine_axis(closest, centre, axis, theta, tol=None, radius=None, redundant=None):
    """step 4: -> the refined unit axis, or None where the iteration was given up.  It is given up when redundant(axis) says so (it is
    converging to an axis that has been accepted already, or to one more half turn of a body of revolution), and (with tol and radius) once the
    candidate cannot come within tol any more: the steps of a point-to-point iteration shrink geometrically, so with the last two
    steps m' and m the axis has at most about m r / (1 - r), r = m / m', left to go; a rotation about an axis that far away moves no
    point by more than coarse_bound of that angle, the surface distance is 1-Lipschitz, and so a candidate whose largest distance
    exceeds tol + coarse_bound(theta, 4 times that angle) stays above tol.  (Most survivors of the coarse scan are no symmetry at
    all and would otherwise creep for the full count of iterations.)"""
    a = np.asarray(axis, np.float64)
    before = None
    for _ in range(REFINE_MAX_ITERATIONS):
        tf = about(centre, axis_rotation(a, theta))
        x, q = closest(tf)
        ok = np.isfinite(q).all(axis=1) & np.isfinite(x).all(axis=1)
        if ok.sum() < 3:
            return None
        new = _axis_of(_kabsch(x[ok] - centre, q[ok] - centre), a)
        moved = math.acos(min(1.0, float(new @ a)))
        if tol is not None and before is not None and before > 0:
            rate = min(moved / before, 0.95)
            left = moved * rate / (1.0 - rate) + moved
            worst = float(np.linalg.norm(x[ok] @ tf[:3, :3].T + tf[:3, 3] - q[ok], axis=1).max())
            if worst > tol + coarse_bound(theta, 4.0 * left, radius):
                return None
        a, before = new, moved
        if redundant is not None and redundant(a):
            return None
        if moved < REFINE_STOP_RAD:
            break
    return a


def find_symmetries(residuals, closest, centre, radius, tol, max_order=6, n_axes=800, rot_angle_discrete=5):
    """The rotational symmetries of a surface -> Symmetries (the module's docstring has the recipe).
    residuals(tfs (T,4,4) float64, which) -> (T,) the largest distance of a sample from the surface under each transform, on the
    "coarse" or the "fine" sample set; closest(tf (4,4)) -> (the fine samples (Q,3), the closest surface points of the transformed fine
    samples (Q,3)), float64.  centre: the surface's area-weighted centroid, radius: the largest vertex distance from it
    (surface_centre), tol: the length a symmetry may move the surface off itself."""
    centre = np.asarray(centre, np.float64).reshape(3)
    radius, tol = float(radius), float(tol)
    if not (np.isfinite(centre).all() and np.isfinite(radius) and radius > 0):
        raise ValueError(f"find_symmetries: centre must be finite and radius a positive length, got {centre}, {radius!r}")
    if not (np.isfinite(tol) and tol > 0):
        raise ValueError(f"find_symmetries: tol must be a positive length, got {tol!r}")
    if isinstance(max_order, bool) or not isinstance(max_order, (int, np.integer)) or int(max_order) < 2:
        raise ValueError(f"find_symmetries: max_order must be an int >= 2, got {max_order!r}")
    if isinstance(n_axes, bool) or not isinstance(n_axes, (int, np.integer)) or int(n_axes) < 8:
        raise ValueError(f"find_symmetries: n_axes must be an int >= 8, got {n_axes!r}")
    step = float(rot_angle_discrete)
    if not (np.isfinite(step) and 0 < step <= 180):
        raise ValueError(f"find_symmetries: rot_angle_discrete must be an angle in (0, 180] degrees, got {rot_angle_discrete!r}")
    max_order = int(max_order)
    axes = hemisphere_axes(int(n_axes))
    delta = covering_angle(axes)
    merge = max(math.radians(1.0), 2.0 * tol / radius)
    probes = _next_primes(max_order)
    # Two axes of one order in a finite rotation group whose orders are at most P are at least pi / P apart (the half turns of a
    # dihedral group are the closest).  A survivor within `same` of an accepted axis of its order need not be refined: another true
    # axis is at least pi / P from the accepted one, and its own nearest grid axis, within delta of it, lies outside `same`.  (The
    # coarse scan lets axes through that are two or three delta from a true one, and they all converge to it.)
    same = max(merge, math.pi / probes[-1] - delta)
    accepted = []                                      # (axis, order, fine residual)
    continuous = None

    def perpendicular(a, b):
        return abs(0.5 * math.pi - _angle_between_axes(a, b)) <= merge

    # the probe orders first, then the high orders: the continuous axis is known before the 2-folds, whose survivors are many for
    # a body of revolution (every axis in its equatorial plane) and of which one is enough
    for n, k in enumerate(probes + list(range(max_order, 1, -1))):
        if n == len(probes):
            continuous = _continuous_axis(accepted, probes, merge)
        theta = 2.0 * math.pi / k
        coarse = np.asarray(residuals(about(centre, np.stack([axis_rotation(a, theta) for a in axes])), "coarse"), np.float64)
        keep = np.flatnonzero(coarse <= tol + coarse_bound(theta, delta, radius))
        have_flip = False
        for i in keep[np.argsort(coarse[keep], kind="stable")]:
            if k == 2 and continuous is not None and have_flip and perpendicular(axes[i], continuous):
                continue
            if any(o == k and _angle_between_axes(a, axes[i]) <= same for a, o, _ in accepted):
                continue
            known = [b for b, o, _ in accepted if o == k]
            skip_flips = k == 2 and continuous is not None and have_flip
            a = refine_axis(closest, centre, axes[i], theta, tol, radius,
                            lambda a: any(_angle_between_axes(a, b) <= merge for b in known) or (skip_flips and perpendicular(a, continuous)))
            if a is None:
                continue
            res = float(np.asarray(residuals(about(centre, axis_rotation(a, theta))[None], "fine"))[0])
            if res <= tol:
                accepted.append((a, k, res))
                if k == 2 and continuous is not None and perpendicular(a, continuous):
                    have_flip = True

    # step 5: one axis for the accepted axes within the merging angle of each other, the best one, with all their orders
    groups = []                                        # [axis, residual, set of orders]
    for a, k, res in sorted(accepted, key=lambda e: e[2]):
        g = next((g for g in groups if _angle_between_axes(g[0], a) <= merge), None)
        if g is None:
            groups.append([a, res, {k}])
        else:
            g[2].add(k)
    rotations, report = [], []
    flip = None
    for a, _, orders in groups:
        if continuous is not None and _angle_between_axes(a, continuous) <= merge:
            continue                                   # the continuous axis' own discrete orders are among its steps
        if continuous is not None and orders == {2} and perpendicular(a, continuous):
            if flip is None:
                flip = a
            continue                                   # every other perpendicular 2-fold is a step times the one flip
        seen = set()
        for k in sorted(orders):
            report.append((a, k))
            for j in range(1, k):
                f = Fraction(j, k)
                if f not in seen:
                    seen.add(f)
                    rotations.append(axis_rotation(a, 2.0 * math.pi * float(f)))
    if continuous is not None:
        report.insert(0, (continuous, math.inf))
        steps = [axis_rotation(continuous, math.radians(d)) for d in np.arange(0.0, 360.0, step)]
        rotations = steps[1:] + rotations
        if flip is not None:
            # the flip axis exactly perpendicular: its component along the continuous axis is its own refinement error
            f = flip - (flip @ continuous) * continuous
            Rf = axis_rotation(f / np.linalg.norm(f), math.pi)
            report.append((f / np.linalg.norm(f), 2))
            rotations += [s @ Rf for s in steps]
    tfs = about(centre, np.stack([np.eye(3)] + rotations))
    # step 7: the postcondition
    res = np.asarray(residuals(tfs, "fine"), np.float64)
    ok = res <= tol
    ok[0] = True
    return Symmetries(tfs=tfs[ok], axes=report, tol=tol, residuals=res[ok], centre=centre)


def _continuous_axis(accepted, probes, merge):
    """the axis accepted at both probe orders (the better of the two refinements), None without; two that are not parallel: ValueError"""
    found = []
    for a, k, res in accepted:
        if k != probes[0]:
            continue
        other = [(b, r) for b, o, r in accepted if o == probes[1] and _angle_between_axes(a, b) <= merge]
        if other:
            b, r = min(other, key=lambda e: e[1])
            found.append(a if res <= r else b)
    if not found:
        return None
    if any(_angle_between_axes(found[0], a) > merge for a in found[1:]):
        raise ValueError("find_symmetries: two continuous axes that are not parallel (a sphere?): more than one continuous axis is "
                         "not described by a list of transforms")
    return found[0]
