"""Register one mesh onto another with no initial guess: the policy around fp_mesh_icp_step, float64 on the host with no device call
of its own.  Like symmetry.find_symmetries it takes a callable, which reconstruct.align_meshes binds to the device
(ops.mesh_icp_step) and the host tests to the numpy restatement (tests/mesh_icp_model.py), so both drive the same policy.

The recipe (align):
 1. Starts.  `starts` seeded rotations, roughly uniform (unit quaternions of normal deviates), and the identity.  Each turns a about
    the centroid of a's coarse samples and puts that centroid on b's area centroid: point-to-plane ICP is a local method whose basin
    is a few tens of degrees wide, and the translation follows within a step or two once the rotation is near.
 2. Coarse stage.  iterations[0] steps of every start on the coarse samples, with no gate on the pair distance (or the caller's).
 3. Ranking.  By the mean squared distance of the pairs at the transform reached (system[36] / system[28] of one more evaluation),
    among the starts whose pair fraction is at least min_overlap.
 4. Basins.  Going down the ranking, a transform that agrees with a better one within BASIN_DEG and BASIN_FRACTION of b's radius (on
    where it sends a's centroid) is the same basin; the best `keep` distinct ones go on.
 5. Fine stage.  iterations[1] steps of those on the fine samples, in ROUNDS rounds; before each round the gate shrinks to
    GATE_FACTOR times the best candidate's root mean square distance, no smaller than GATE_FLOOR of b's radius and no larger than the
    caller's max_dist.  One gate for every candidate: they are ranked on the same footing, and a wrong basin loses its pairs.
 6. Ranking and basins again -> the winner and the best other basin (`runner_up`): a symmetric or nearly symmetric object shows up as
    a runner-up of the same cost, and the caller decides what that means.
Local mode: init= (4,4) or (S,4,4) takes the place of the starts."""
import math

import numpy as np

BASIN_DEG = 5.0            # two transforms within this angle ...
BASIN_FRACTION = 0.05      # ... and this fraction of b's radius are one basin
ROUNDS = 4                 # gate updates of the fine stage
GATE_FACTOR = 3.0          # the gate in units of the best candidate's rms distance
GATE_FLOOR = 0.02          # ... and its floor in units of b's radius
NO_GATE = 1e18             # "the whole extent": max_dist * max_dist stays finite in float32


def start_rotations(n, seed=0):
    """n seeded rotations, roughly uniform over SO(3) (unit quaternions of normal deviates), after the identity -> (n + 1, 3, 3)"""
    rng = np.random.default_rng(int(seed) + 9000)
    q = rng.normal(size=(int(n), 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)
    return np.concatenate([np.eye(3)[None], R.reshape(-1, 3, 3)], axis=0)


def start_transforms(rotations, centre_a, centre_b):
    """[R | cb - R ca]: each rotation about a's centre, that centre put on b's -> (S,4,4) float64"""
    R = np.asarray(rotations, np.float64).reshape(-1, 3, 3)
    out = np.tile(np.eye(4), (len(R), 1, 1))
    out[:, :3, :3] = R
    out[:, :3, 3] = np.asarray(centre_b, np.float64) - R @ np.asarray(centre_a, np.float64)
    return out


def rotation_angle(Ra, Rb):
    """the angle of Ra Rb^T in radians"""
    return math.acos(min(1.0, max(-1.0, (float(np.trace(Ra @ Rb.T)) - 1.0) / 2.0)))


def costs(system, n_samples, min_overlap):
    """per row of a (S,40) system: the mean squared pair distance, +inf where the row has too few pairs, was not solvable as given
    (status 2) or is not finite; and the pair fraction"""
    system = np.asarray(system, np.float64).reshape(-1, 40)
    pairs = system[:, 28]
    overlap = pairs / max(1, n_samples)
    with np.errstate(all="ignore"):
        cost = np.where(pairs > 0, system[:, 36] / pairs, np.inf)
    bad = (overlap < min_overlap) | (system[:, 29] == 2) | ~np.isfinite(cost)
    return np.where(bad, np.inf, cost), overlap


def distinct_basins(tfs, cost, centre_a, radius, keep):
    """indices of the best `keep` transforms no two of which are the same basin, best first"""
    order = [int(i) for i in np.argsort(cost, kind="stable") if np.isfinite(cost[i])]
    ca = np.asarray(centre_a, np.float64)
    kept = []
    for i in order:
        where = tfs[i, :3, :3] @ ca + tfs[i, :3, 3]
        same = any(rotation_angle(tfs[i, :3, :3], tfs[j, :3, :3]) <= math.radians(BASIN_DEG)
                   and np.linalg.norm(where - (tfs[j, :3, :3] @ ca + tfs[j, :3, 3])) <= BASIN_FRACTION * radius for j in kept)
        if not same:
            kept.append(i)
            if len(kept) == keep:
                break
    return kept


def align(steps, centre_a, centre_b, radius_b, n_samples, starts=300, iterations=(12, 20), max_dist=None, min_overlap=0.5, init=None,
          seed=0, keep=8):
    """-> dict(tf (4,4) float64, mean_distance, rmse, overlap, status, runner_up): the fields of ops.MeshAlignment.
    steps(which, tfs (S,4,4) float64, max_dist, n) -> (tfs' (S,4,4), system (S,40), dist2 (S,Q)): n steps of every transform on the
    "coarse" or the "fine" samples of a against b, then one more evaluation: tfs' is what the n steps reached, system and dist2
    (the squared distance of every sample) are those of the evaluation at tfs'.  centre_a: the centroid of a's coarse samples;
    centre_b, radius_b: symmetry.surface_centre of b; n_samples: (coarse, fine)."""
    what = "align_meshes"
    it = tuple(int(i) for i in iterations)
    if len(it) != 2 or it[0] < 0 or it[1] < 0:
        raise ValueError(f"{what}: iterations must be two counts >= 0 (coarse, fine), got {iterations!r}")
    if not (0.0 < float(min_overlap) <= 1.0):
        raise ValueError(f"{what}: min_overlap must lie in (0, 1], got {min_overlap!r}")
    if max_dist is not None and not (np.isfinite(float(max_dist)) and float(max_dist) > 0):
        raise ValueError(f"{what}: max_dist must be a positive length or None, got {max_dist!r}")
    if isinstance(keep, bool) or int(keep) < 1:
        raise ValueError(f"{what}: keep must be an int >= 1, got {keep!r}")
    cap = NO_GATE if max_dist is None else float(max_dist)
    radius_b = float(radius_b)
    if init is not None:
        tfs = np.asarray(init, np.float64)
        tfs = tfs[None] if tfs.ndim == 2 else tfs
        if tfs.ndim != 3 or tfs.shape[1:] != (4, 4) or len(tfs) < 1 or not np.isfinite(tfs).all():
            raise ValueError(f"{what}: init must be a finite (4,4) or (S,4,4) transform table, got shape {np.shape(init)}")
    else:
        if isinstance(starts, bool) or not isinstance(starts, (int, np.integer)) or int(starts) < 0:
            raise ValueError(f"{what}: starts must be an int >= 0, got {starts!r}")
        tfs = start_transforms(start_rotations(starts, seed), centre_a, centre_b)
    # coarse
    tfs, system, _ = steps("coarse", tfs, cap, it[0])
    tfs = np.asarray(tfs, np.float64)
    cost, _ = costs(system, n_samples[0], min_overlap)
    kept = distinct_basins(tfs, cost, centre_a, radius_b, int(keep))
    if not kept:
        raise ValueError(f"{what}: no start keeps {min_overlap:.0%} of the samples as pairs: the meshes do not overlap as given "
                         f"(other units? pass init= or a larger max_dist)")
    tfs = tfs[kept]
    # fine: rounds of steps under one shrinking gate
    rounds = max(1, min(ROUNDS, it[1]))
    per = [it[1] // rounds + (1 if k < it[1] % rounds else 0) for k in range(rounds)]
    gate = cap
    tfs, system, dist2 = steps("fine", tfs, gate, 0)
    for n in per:
        cost, _ = costs(system, n_samples[1], min_overlap)
        if np.isfinite(cost).any():
            gate = min(cap, max(GATE_FACTOR * math.sqrt(float(cost.min())), GATE_FLOOR * radius_b))
        tfs, system, dist2 = steps("fine", np.asarray(tfs, np.float64), gate, n)
    tfs = np.asarray(tfs, np.float64)
    cost, overlap = costs(system, n_samples[1], min_overlap)
    kept = distinct_basins(tfs, cost, centre_a, radius_b, 2)
    if not kept:
        raise ValueError(f"{what}: no candidate keeps {min_overlap:.0%} of the samples as pairs after the fine stage")
    w = kept[0]
    runner_up = None
    if len(kept) > 1:
        r = kept[1]
        runner_up = dict(tf=tfs[r].copy(), mean_distance=_mean_distance(np.asarray(dist2, np.float64)[r], gate),
                         cost=float(cost[r]), angle_deg=math.degrees(rotation_angle(tfs[r, :3, :3], tfs[w, :3, :3])))
    out = tfs[w].copy()
    out[3] = (0.0, 0.0, 0.0, 1.0)
    return dict(tf=out, mean_distance=_mean_distance(np.asarray(dist2, np.float64)[w], gate), rmse=math.sqrt(float(cost[w])),
                overlap=float(overlap[w]), status=int(np.asarray(system)[w, 29]), runner_up=runner_up, cost=float(cost[w]),
                max_dist=float(gate))


def _mean_distance(d2, gate):
    """the mean distance of the samples within the gate, from their squared distances"""
    near = d2[d2 <= np.float64(np.float32(gate)) ** 2]
    return float(np.sqrt(near).mean()) if len(near) else float("nan")
