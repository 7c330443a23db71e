"""CPU: the definition of fp_mesh_icp_step (tests/mesh_icp_model.py, the numpy restatement of include/fp_amd.h) against an
independent float64 formulation; the named wrong variants told apart; a degenerate winning face, the pair gate on its threshold and
min_pairs; the alignment policy (foundationpose_amd/mesh_align.py) driven by the restatement on shapes whose pose is known; its
refusals and the C entry point's argument errors (no GPU is touched: every refusal comes before the first launch).  Each test prints
its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import mesh_distance_model as mm
import mesh_icp_cases as ic
import mesh_icp_model as mi
import mesh_symmetry_cases as sc
import mesh_symmetry_model as sm

f32 = np.float32
U = 2.0 ** -24


def _bits_differ(a, b):
    return not (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)))


def _box_case(T=3, Q=300, seed=2):
    """the pulled box in a seeded pose as b, Q samples of its surface as a's points, T transforms a few degrees and a few per cent of
    the size from the identity"""
    pos, faces, _, _ = sc.posed(sc.pulled_box(), seed)
    pts = mm.sample_surface(pos, faces, Q, seed=seed)[0]
    rng = np.random.default_rng(seed)
    from foundationpose_amd.symmetry import axis_rotation
    tfs = np.tile(np.eye(4), (T, 1, 1))
    for t in range(T):
        tfs[t, :3, :3] = axis_rotation(rng.normal(size=3), np.radians(rng.uniform(1, 4)))
        tfs[t, :3, 3] = rng.uniform(-0.03, 0.03, 3)
    return pos, faces, pts, tfs.astype(f32)


# ------------------------------------------------------------------ 1. the restatement against float64
def test_rows_equal_a_float64_formulation_within_the_rounding_of_float32():
    """Where the nearest point is inside a face (region 7) the residual is the signed distance to the face's plane and the row is
    ((p - t) x m, m): rows_float64 computes both from float64 vertices.  Bound, u = 2^-24, M the largest coordinate magnitude of the
    mesh, the points and the translations (>= the size of every vector below):
      p: three products and three sums of terms <= M: |dp| <= 4 u (|R||x| + |t|) <= 4 (sqrt 3 + 1) u M < 11 u M per component;
      m: the edge vectors carry u M each, the cross product 2 u |ab||ac| + 2 u M (|ab| + |ac|) per component, and the division by
         |n| = |ab||ac| sin(angle) turns that into <= (2 + 4 M / min edge) u / sin(angle) -- the pulled box's faces have edges >= 1,
         M < 2 and angles >= 45 degrees: |dm| <= 15 u per component, and one more u for the rounding of m itself;
      r = m . (q - p): the error of q inside the plane is perpendicular to m (first order), its error across the plane is that of
         a + v ab + w ac, <= 4 u M; with |q - p| <= 0.1 M here, |dr| <= 3 (11 + 4) u M + 3 * 16 u * 0.1 M + 3 u |r| < 51 u M;
      J: m itself (16 u) and (p - c) x m: |p - c| <= 2 M, each component two products and a difference:
         <= 2 (12 u M + 2 M * 16 u) + 3 u * 2 M < 94 u M.
    Asserted at 51 u M for r and 94 u M for J; the measured figures are printed."""
    pos, faces, pts, tfs = _box_case(T=3, Q=400)
    terms = mi.pair_terms(pos, faces, pts, tfs, ic.NO_GATE)
    p = sm.transform_points(pts, tfs)
    M = float(max(np.abs(pos).max(), np.abs(p).max(), np.abs(tfs[:, :3, 3]).max()))
    worst_r = worst_j = 0.0
    n = 0
    for t in range(len(tfs)):
        reg = mm.mesh_point_distance(pos, faces, p[t], regions=True)[3]
        k = (reg == 7) & terms["pair"][t]
        assert k.sum() > 100
        J, r = mi.rows_float64(pos, faces, pts[k], tfs[t], terms["face"][t][k])
        worst_r = max(worst_r, float(np.abs(terms["r"][t][k] - r).max()))
        worst_j = max(worst_j, float(np.abs(terms["J"][t][k] - J).max()))
        n += int(k.sum())
        assert np.allclose(terms["dist2"][t][k], r * r, rtol=0, atol=2 * 51 * U * M * np.abs(r).max() + (51 * U * M) ** 2)
    print(f"{n} interior pairs, M = {M:.3f}: r within {worst_r / (U * M):.2f} u M (bound 51), J within {worst_j / (U * M):.2f} u M (bound 94)")
    assert worst_r <= 51 * U * M and worst_j <= 94 * U * M


def test_the_step_moves_a_displaced_copy_onto_the_mesh():
    """not a bound, a sanity check of the conventions all at once: three steps from a few degrees away leave an rms of the size of
    float32 rounding"""
    pos, faces, pts, tfs = _box_case(T=3, Q=400)
    m = tfs
    for _ in range(4):
        m, system, _ = mi.step(pos, faces, pts, m, ic.NO_GATE)
        assert (system[:, 29] == 0).all()
    _, system, _ = mi.step(pos, faces, pts, m, ic.NO_GATE)
    rms = np.sqrt(system[:, 36] / system[:, 28])
    print("rms after four steps:", rms)
    assert (rms < 1e-5).all()


# ------------------------------------------------------------------ 2. wrong variants
@pytest.mark.parametrize("wrong", mi.WRONG)
def test_wrong_variants_are_told_apart(wrong):
    if wrong == "lt":
        c = ic.threshold_case()
        args = (c["pos"], c["faces"], c["points"], c["tfs"], c["max_dist"])
    else:
        pos, faces, pts, tfs = _box_case(T=2, Q=200)
        args = (pos, faces, pts, tfs, 0.02)
    right = mi.step(*args)
    other = mi.step(*args, wrong=wrong)
    assert _bits_differ(right, other), wrong
    if wrong == "lt":
        assert right[1][0, 28] == 12 and other[1][0, 28] == 6           # the six samples exactly on the threshold
    else:
        assert 6 < right[1][0, 28] < 200                               # the gate cuts some and keeps some


def test_pairs_exactly_on_the_threshold_count():
    c = ic.threshold_case()
    terms = mi.pair_terms(c["pos"], c["faces"], c["points"], c["tfs"], c["max_dist"])
    h2 = f32(c["max_dist"]) * f32(c["max_dist"])
    assert (terms["dist2"][0, :6] == h2).all() and (terms["dist2"][0, 6:12] > h2).all()
    assert terms["pair"][0].tolist() == [True] * 6 + [False] * 6 + [True] * 6


def test_a_degenerate_winning_face_is_no_pair():
    c = ic.degenerate_winner_case()
    out, system, terms = mi.step(c["pos"], c["faces"], c["points"], c["tfs"], c["max_dist"])
    assert (terms["face"] == 0).all() and np.isfinite(terms["dist2"]).all() and not terms["pair"].any()
    assert system[0, 28] == 0 and system[0, 29] == 1 and (system[0, :28] == 0).all() and system[0, 36] == 0
    assert np.array_equal(out.view(np.uint32), c["tfs"].view(np.uint32))


def test_status_one_below_min_pairs():
    pos, faces, pts, tfs = _box_case(T=2, Q=200)
    base = mi.step(pos, faces, pts, tfs, 0.02)[1]
    k = int(base[0, 28])
    for mp, want in ((k + 1, 1), (k, 0)):
        out, system, _ = mi.step(pos, faces, pts, tfs[:1], 0.02, min_pairs=mp)
        assert system[0, 29] == want and np.array_equal(system[0, :29], base[0, :29])
        assert np.array_equal(out[0].view(np.uint32), tfs[0].view(np.uint32)) == (want == 1)
        assert (system[0, 30:36] == 0).all() == (want == 1)


# ------------------------------------------------------------------ 3. the policy on the restatement
@pytest.mark.parametrize("shape,seed", [(s, k) for s in ic.SHAPES for k in (1, 2, 3)])
def test_exact_copies_are_recovered(shape, seed):
    """a is the shape, b its exact copy in a seeded rigid pose: the truth is known.  Gates: four times the error measured with this
    restatement-driven policy (ic.MEASURED, COVERAGE.md), and no tighter than 16 float32 ulps of the mesh extent"""
    from foundationpose_amd.symmetry import surface_centre
    v, f = ic.SHAPES[shape]()
    pos, faces, R, t = sc.posed((v, f), seed)
    _, radius = surface_centre(pos, faces)
    got = mi.host_align((v.astype(f32), f), (pos, faces))
    deg, frac = ic.rigid_error(got.tf, ic.truth_of(R, t), radius)
    gate_deg, gate_frac = ic.alignment_gates(shape, pos)
    print(f"{shape} seed {seed}: {deg:.3e} deg, {frac:.3e} of the radius (gates {gate_deg:.3e}, {gate_frac:.3e}); rmse {got.rmse:.3e}, "
          f"overlap {got.overlap:.3f}, runner-up {got.runner_up and (got.runner_up['mean_distance'] / radius, got.runner_up['angle_deg'])}")
    assert got.status == 0 and got.overlap == 1.0
    assert deg <= gate_deg and frac <= gate_frac
    assert got.runner_up is not None and got.runner_up["cost"] > 100 * got.rmse ** 2        # no symmetry: the next basin is worse
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = sc.random_rotation(np.random.default_rng(seed)), (0.1, -0.2, 0.7)
    assert np.allclose(got.transfer_pose(pose) @ got.tf, pose, atol=1e-12)


def test_the_cube_lands_on_one_of_its_24_rotations_with_a_runner_up_of_equal_cost():
    from foundationpose_amd.symmetry import surface_centre
    v, f = sc.box_shape(1.0, 1.0, 1.0)
    pos, faces, R, t = sc.posed((v, f), 5)
    _, radius = surface_centre(pos, faces)
    got = mi.host_align((v.astype(f32), f), (pos, faces))
    d = got.tf @ np.linalg.inv(ic.truth_of(R, t))                       # a symmetry of b, in b's frame: R g R^T about t
    g = R.T @ d[:3, :3] @ R
    ang = np.degrees(np.arccos(np.clip((np.einsum("aij,ij->a", sc.cube_group(), g) - 1) / 2, -1, 1)))
    gate_deg, gate_frac = ic.alignment_gates("pulled_box", pos)
    off = np.linalg.norm(got.tf[:3, :3] @ np.zeros(3) + got.tf[:3, 3] - t) / radius       # the cube's centre goes to the copy's centre
    floor = 16 * np.spacing(f32(np.abs(pos).max()))
    print(f"cube: {ang.min():.3e} deg from the nearest of the 24, centre off by {off:.3e} of the radius; rmse {got.rmse:.3e}, runner-up rmse "
          f"{np.sqrt(got.runner_up['cost']):.3e} at {got.runner_up['angle_deg']:.2f} deg (both <= {floor:.3e})")
    assert ang.min() <= gate_deg and off <= gate_frac
    assert got.rmse <= floor and np.sqrt(got.runner_up["cost"]) <= floor               # equal: both are float32 rounding
    assert min(abs(got.runner_up["angle_deg"] - k) for k in (90.0, 120.0, 180.0)) < 0.01


@pytest.mark.parametrize("seed", [1, 2])
def test_a_noisy_partial_scan_costs_no_more_than_the_truth(seed):
    """128 / 2048 noisy samples (sigma 0.004 of the radius) of the pulled box without its first two triangles: the mean squared
    distance of the fine samples at the returned transform is at most 1.05 times that at the true transform (the margin: the
    steps minimise the point-to-plane cost, the figure is the point distance)"""
    a, b, pts, truth = ic.noisy_partial_box(seed)
    got = mi.host_align(a, b, points=pts)

    def cost(tf):
        p = sm.transform_points(pts[1], np.asarray(tf, f32)[None])[0]
        return float(mm.mesh_point_distance(b[0], b[1], p)[0].astype(np.float64).mean())
    c_got, c_true = cost(got.tf), cost(truth)
    from foundationpose_amd.symmetry import surface_centre
    deg, frac = ic.rigid_error(got.tf, truth, surface_centre(*b)[1])
    print(f"seed {seed}: cost {c_got:.4e} at the result, {c_true:.4e} at the truth (ratio {c_got / c_true:.4f}); {deg:.3f} deg, {frac:.2e} of the "
          f"radius off; runner-up at {got.runner_up['cost'] / got.rmse ** 2:.1f} times the cost")
    assert c_got <= 1.05 * c_true


def test_local_mode_and_refusals():
    from foundationpose_amd import mesh_align
    v, f = sc.pulled_box()
    pos, faces, R, t = sc.posed((v, f), 1)
    near = ic.truth_of(R, t)
    near[:3, 3] += 0.02
    got = mi.host_align((v.astype(f32), f), (pos, faces), init=near)
    from foundationpose_amd.symmetry import surface_centre
    deg, frac = ic.rigid_error(got.tf, ic.truth_of(R, t), surface_centre(pos, faces)[1])
    gate_deg, gate_frac = ic.alignment_gates("pulled_box", pos)
    assert deg <= gate_deg and frac <= gate_frac and got.runner_up is None       # one start: no other basin
    never = lambda *a: pytest.fail("the policy called the device before refusing")   # noqa: E731
    for kw, msg in ((dict(iterations=(3,)), "iterations"), (dict(iterations=(-1, 2)), "iterations"), (dict(min_overlap=0.0), "min_overlap"),
                    (dict(min_overlap=1.5), "min_overlap"), (dict(max_dist=-1.0), "max_dist"), (dict(max_dist=float("nan")), "max_dist"),
                    (dict(starts=-1), "starts"), (dict(starts=2.5), "starts"), (dict(init=np.eye(3)), "init"),
                    (dict(init=np.full((4, 4), np.nan)), "init"), (dict(keep=0), "keep")):
        with pytest.raises(ValueError, match=msg):
            mesh_align.align(never, np.zeros(3), np.zeros(3), 1.0, (8, 8), **kw)
    far = np.eye(4)
    far[:3, 3] = 1e3                                                              # nothing within the caller's max_dist: no pairs
    with pytest.raises(ValueError, match="do not overlap"):
        mi.host_align((v.astype(f32), f), (pos, faces), init=far, max_dist=0.1)


def test_c_entry_point_reports_argument_errors_without_a_gpu():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    p, q = C.c_void_p(16), C.c_void_p(4096)
    wsb = lib.fp_mesh_icp_workspace_bytes
    assert wsb(0, 5) == 0 == wsb(5, 0) == wsb(-3, 5) == wsb(5, -1) and wsb(300, 128) == 8 * 300 * 128 + 300 * 256
    assert wsb(2, 257) == 8 * 2 * 257 + 2 * 2 * 256

    def call(pos=p, Nv=3, faces=p, F=1, points=p, Q=4, tfs_in=p, T=2, max_dist=1.0, damping=1e-3, min_pairs=6, system=p, tfs_out=q, ws=p,
             ws_bytes=8 * 8 + 2 * 256):
        return lib.fp_mesh_icp_step(pos, Nv, faces, F, points, Q, tfs_in, T, max_dist, damping, min_pairs, system, tfs_out, None, None, ws,
                                    ws_bytes, None)

    for kw, word in ((dict(Q=-1), b"Q=-1"), (dict(T=-1), b"T=-1"), (dict(T=1 << 20, Q=(1 << 10) + 1), b"above 2^30"), (dict(F=-1), b"F=-1"),
                     (dict(F=(1 << 30) + 1), b"F="), (dict(Nv=-1), b"Nv=-1"), (dict(max_dist=-1.0), b"max_dist"),
                     (dict(max_dist=float("inf")), b"max_dist"), (dict(max_dist=float("nan")), b"max_dist"), (dict(damping=-1e-3), b"damping"),
                     (dict(damping=float("nan")), b"damping"), (dict(min_pairs=5), b"min_pairs=5"), (dict(tfs_in=None), b"NULL tfs_in or system"),
                     (dict(system=None), b"NULL tfs_in or system"), (dict(points=None), b"NULL points"), (dict(faces=None), b"faces is NULL"),
                     (dict(pos=None), b"pos is NULL"), (dict(ws=None), b"workspace"), (dict(ws_bytes=8 * 8 + 2 * 256 - 1), b"workspace"),
                     (dict(ws=C.c_void_p(20)), b"8-byte aligned"), (dict(tfs_out=p), b"overlap"), (dict(tfs_out=C.c_void_p(16 + 64)), b"overlap"),
                     (dict(tfs_in=C.c_void_p(4096 + 127)), b"overlap")):
        assert call(**kw) == -1, kw
        msg = lib.fp_last_error()
        assert msg.startswith(b"fp_mesh_icp_step") and word in msg, (kw, msg)
    assert call(T=0, points=None, tfs_in=None, system=None, tfs_out=None, ws=None, ws_bytes=0) == 0        # nothing to do
