"""CPU: the float64 definition of the pose update, its error bound and the float32 restatement (tests/pose_update_model.py) on the
generated cases of tests/pose_update_cases.py, against the C oracle (fpo_pose_update, host libm, L_f = 1):

  * the oracle lies within the bound of the definition on every element of every row the bound determines, and the rows it does
    not determine are exactly the ones the generator flags as degenerate -- named 6d and 'deepim' rows, no axis-angle row;
  * the restatement equals the oracle bit for bit wherever no libm call enters;
  * the closed-form 'deepim' delta lies within the bound of the definition with general inverses and reproduces the reference's
    own numbers (golden g6) within the tolerance the existing golden test uses;
  * each wrong variant of the definition leaves the bound, by a factor of two or more, on a named case;
  * every tagged row is where its tag says.
tests/test_gpu_pose_update_edges.py asks the same of the kernel."""
import os

import numpy as np
import pytest

import pose_update_cases as pc
import pose_update_model as pm

F = np.float32
U = np.uint32
# the wrong variant -> (the case that is there to catch it, a tag whose rows must show it or None for any determined row)
CAUGHT_BY = {"clamp_on_norm": ("aa_rn0.349_n257_tracknet_norm", "inside_clamp"), "eps_1e-6": ("aa_rn1_n65_tracknet", "inside_clamp"),
             "no_transpose": ("aa_rn0.349_n257_tracknet_norm", "inside_clamp"), "normalizer_inside_tanh": ("aa_rn0.349_n257_tracknet_norm", "single_axis"),
             "b3_is_b2_x_b1": ("6d_n257_raw", "orthonormal"), "full_diameter": ("aa_rn1_n64_tracknet_norm", None),
             "tanh_under_normalize_xyz": ("aa_rn0.349_n257_tracknet_norm", None), "deepim_ignores_skew": ("deepim_skew_300x104_n257", None),
             "deepim_uses_input_h": ("deepim_skew_300x104_n257", None)}


@pytest.fixture(scope="module")
def cases(scene):
    return pc.cases(scene)


def _same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(U) == b.view(U)) | (np.isnan(a) & np.isnan(b))


def _oracle_pose(c, dt32=None):
    """the oracle's pose for the case.  The oracle has the 'tracknet' translation only: a delta that is already metric ('raw', or the
    'deepim' delta dt32) goes in as a normalised translation with a diameter of 2, a factor of exactly 1.  Per-object diameters:
    one call per diameter."""
    from oracle import ops as oo
    N = len(c["poses"])
    if dt32 is not None or c["trans_rep"] == "raw":
        return oo.pose_update(c["trans"] if dt32 is None else dt32, c["rot"], c["poses"], c["rot_rep"], True, c["trans_normalizer"], c["rot_normalizer"], 2.0)
    d = np.broadcast_to(np.asarray(pc.row_diameters(c), np.float64), (N,))
    out = np.full((N, 4, 4), np.nan, F)
    for dia in np.unique(d[~np.isnan(d)]):
        rows = d == dia
        out[rows] = oo.pose_update(c["trans"], c["rot"], c["poses"], c["rot_rep"], c["normalize_xyz"], c["trans_normalizer"], c["rot_normalizer"],
                                   float(dia))[rows]
    if c["normalize_xyz"]:
        return out
    return oo.pose_update(c["trans"], c["rot"], c["poses"], c["rot_rep"], False, c["trans_normalizer"], c["rot_normalizer"], 1.0)


def test_cases_cover_what_the_issue_lists(cases):
    assert len({c["name"] for c in cases}) == len(cases) and all(c["targets"] for c in cases)
    assert {len(c["poses"]) for c in cases} >= set(pc.SIZES)
    aa = [c for c in cases if c["rot_rep"] == "axis_angle"]
    assert {c["rot_normalizer"] for c in aa} == {float(F(r)) for r in pc.ROT_NORMALIZERS}
    tags = set().union(*(c["tags"] for c in cases))
    assert tags >= {"zero_rot", "n2_below", "n2_at", "n2_above", "single_axis", "tanh_saturated", "th_near_pi", "inside_clamp", "random", "orthonormal",
                    "scaled_1e-15", "scaled_1e15", "a1_zero", "a2_zero", "parallel", "near_parallel", "raw_trans_edges", "ratio_1", "ratio_half",
                    "tz_zero", "tz_negative", "tz_tiny", "collapsed_window"}
    assert {c["trans_rep"] for c in cases} == {"tracknet", "raw", "deepim"}
    assert {(c["trans_rep"], c["normalize_xyz"]) for c in cases} >= {("tracknet", True), ("tracknet", False), ("deepim", True), ("deepim", False)}
    assert {c["diameter"] for c in cases if c["form"] == "single"} >= {2.0, 1e-3, 10.0}
    assert {c["form"] for c in cases} == {"single", "multi", "views"}
    assert any(c["form"] == "multi" and c["obj"] is None for c in cases) and any(c["form"] == "views" and c["view"] is None for c in cases)
    assert any(c["form"] == "multi" and c["obj"] is not None and c["obj"].min() < 0 and c["obj"].max() >= len(c["diameters"]) for c in cases)
    assert any(c["form"] == "views" and c["view"] is not None and c["view"].min() < 0 and c["view"].max() >= len(c["Ks"]) for c in cases)
    dk = [c for c in cases if c["trans_rep"] == "deepim"]
    assert any(np.asarray(pc.row_Ks(c)).reshape(-1, 3, 3)[0][0, 1] != 0 for c in dk) and any(c["input_w"] != c["input_h"] for c in dk)
    sx = np.concatenate([c["tf"][:, 0, 0] for c in dk])
    assert np.nanmin(sx[np.isfinite(sx) & (sx > 1e-3)]) <= 0.125 and np.nanmax(sx[np.isfinite(sx)]) >= 8.0


def test_every_tagged_row_is_where_its_tag_says(cases):
    I3 = np.eye(3, dtype=F)
    for c in cases:
        t = c["tags"]
        rot, rn = c["rot"], c["rot_normalizer"]
        rows = lambda tag: np.asarray(t.get(tag, []), np.int64)
        if c["rot_rep"] == "axis_angle":
            n2 = pc._n2(rot, rn)
            _, th = pm.rotation_angle_args(c["trans"], rot, rn, c["normalize_xyz"], c["trans_rep"], "axis_angle")
            pose, _, dR = pc.restatement(c)
            for k in rows("zero_rot"):
                assert not rot[k].any() and _same(dR[k], I3).all() and _same(pose[k, :3, :3], c["poses"][k, :3, :3]).all(), (c["name"], k)
            for tag, want in (("n2_below", np.nextafter(pc.EPS2, F(0))), ("n2_at", pc.EPS2), ("n2_above", np.nextafter(pc.EPS2, F(1)))):
                assert (n2[rows(tag)] == want).all(), (c["name"], tag, n2[rows(tag)])
            assert (n2[rows("n2_below")] < pc.EPS2).all() and (th[rows("n2_below")] == np.sqrt(pc.EPS2)).all()
            assert (n2[rows("inside_clamp")] < pc.EPS2).all()
            with np.errstate(all="ignore"):
                sat = pm.Single().tanh(rot)
            assert (np.abs(sat[rows("tanh_saturated")]) == 1).all()
            for k in rows("single_axis"):
                assert (rot[k] != 0).sum() == 1
            assert (np.abs(th[rows("th_near_pi")].astype(np.float64) - np.pi) <= 4 * np.spacing(F(np.pi))).all(), th[rows("th_near_pi")]
        else:
            a1, a2 = rot[:, :3].astype(np.float64), rot[:, 3:].astype(np.float64)
            with np.errstate(all="ignore"):
                n1, n2_ = np.linalg.norm(a1, axis=1), np.linalg.norm(a2, axis=1)
                sinang = np.linalg.norm(np.cross(a1, a2), axis=1) / (n1 * n2_)
            for k in rows("orthonormal"):
                assert abs(n1[k] - 1) < 1e-7 and abs(n2_[k] - 1) < 1e-7 and abs(a1[k] @ a2[k]) < 1e-7
            assert (n1[rows("scaled_1e-15")] < 1e-12).all() and (n1[rows("scaled_1e-15")] > 1e-16).all()     # F.normalize's eps is active
            assert (n1[rows("scaled_1e15")] > 1e14).all() and np.isfinite((rot[rows("scaled_1e15")] ** 2).sum(axis=1)).all()
            assert (n1[rows("a1_zero")] == 0).all() and (n2_[rows("a1_zero")] > 0).all()
            assert (n2_[rows("a2_zero")] == 0).all() and (n1[rows("a2_zero")] > 0).all()
            assert (sinang[rows("parallel")] < 1e-6).all() and (sinang[rows("near_parallel")] < 1e-6).all()
            assert (sinang[rows("random")] > 1e-3).all()
        if "raw_trans_edges" in t:
            e = c["trans"][rows("raw_trans_edges")]
            assert (e == 0).any() and (np.abs(e) == 20).any() and np.isinf(e).any() and not c["normalize_xyz"] and c["trans_rep"] == "tracknet"
        if c["trans_rep"] == "deepim":
            assert (c["trans"][rows("ratio_1"), 2] == 1).all() and (c["trans"][rows("ratio_half"), 2] == 0.5).all()
            tz = c["poses"][:, 2, 3]
            assert (tz[rows("tz_zero")] == 0).all() and (tz[rows("tz_negative")] < 0).all() and (tz[rows("tz_tiny")] > 0).all()
            assert (tz[rows("tz_tiny")] <= 1e-6).all() and F(1e-30) in tz[rows("tz_tiny")] if "tz_tiny" in t else True
            assert not np.isfinite(c["tf"][rows("collapsed_window")]).all(axis=(1, 2)).any()


def test_oracle_within_the_bound_and_only_the_flagged_rows_left_out(cases):
    worst = {}
    for c in cases:
        d = pc.definition(c, pm.L_HOST)
        und = pm.undetermined_rows(d, c["poses"])
        assert np.array_equal(und, pc.flagged(c)), (c["name"], np.flatnonzero(und), np.flatnonzero(pc.flagged(c)))
        if c["rot_rep"] == "axis_angle":
            ok = np.isfinite(d["dR"]).all(axis=(1, 2))
            assert (d["dR_e"][ok] <= 1e-3 * pm.ROT_SCALE).all(), (c["name"], "an axis-angle rotation the bound does not determine")
            assert not c["degenerate"].any() or c["trans_rep"] == "deepim"
        rs = pc.restatement(c)
        ref = _oracle_pose(c, rs[1] if c["trans_rep"] == "deepim" else None)
        keep = ~und
        ex = pm.excess(ref, d, "pose")[keep]
        worst[c["name"]] = float(ex.max(initial=0.0))
        print(f"{c['name']:42s} oracle / bound {worst[c['name']]:.3f}")
        assert (ex <= 1.0).all(), (c["name"], worst[c["name"]], np.argwhere(pm.excess(ref, d, "pose") * keep[:, None, None] > 1)[:5])
        for i, key in enumerate(("pose", "dt", "dR")):      # the restatement's own libm is float64 rounded once: 0.5 ulp
            assert (pm.excess(rs[i], d, key)[keep] <= 1.0).all(), (c["name"], key)
    assert max(worst.values()) > 0.5, "the bound is far from what float32 does: it would not see a subtle error"


def test_restatement_is_the_oracle_bit_for_bit_where_no_libm_enters(cases):
    compared = 0
    for c in cases:
        rot_libm, trans_libm = pc.uses_libm(c)
        if c["trans_rep"] == "deepim":
            continue                                     # the oracle has no closed-form 'deepim': see the test below
        pose = pc.restatement(c)[0]
        ref = _oracle_pose(c)
        bad_t = [k for k in c["nan_rows"].get("translation", [])]
        if not trans_libm:
            assert _same(pose[:, :3, 3], ref[:, :3, 3])[[k for k in range(len(pose)) if k not in bad_t]].all(), c["name"]
            assert np.isnan(pose[bad_t][:, :3, 3]).all()
            compared += 1
        if not rot_libm:
            assert _same(pose[:, :3, :3], ref[:, :3, :3]).all() and _same(pose[:, 3], ref[:, 3]).all(), c["name"]    # degenerate rows too
            compared += 1
    assert compared >= 12


def test_closed_form_deepim_delta_within_the_bound_and_the_golden(cases, scene):
    from oracle import ops as oo
    for c in cases:
        if c["trans_rep"] != "deepim":
            continue
        d = pc.definition(c, pm.L_HOST)
        keep = ~pm.undetermined_rows(d, c["poses"])
        dt = pc.restatement(c)[1]
        assert (pm.excess(dt, d, "dt")[keep] <= 1.0).all(), c["name"]
        # the closed forms are the general inverses: in float64 the two agree far inside the float32 bound
        assert (np.abs(d["dt_closed"] - d["dt"])[keep] <= pm.F64_SLACK * d["dt_e"][keep]).all(), c["name"]
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_golden.npz")))
    Pg = g["poses_in"]
    tfg, _ = oo.crop_windows(Pg, scene["K"], scene["diameter"], 1.2, (160, 160))
    _, dt, _ = pm.restatement(g["g4_raw_trans"], g["g4_raw_rot"], Pg, rot_rep="axis_angle", normalize_xyz=True, rot_normalizer=0.349,
                              diameter=scene["diameter"], trans_rep="deepim", K=scene["K"], tf=tfg, input_w=160)
    np.testing.assert_allclose(dt, g["g6_deepim_trans_delta"], atol=5e-6, rtol=0)


@pytest.mark.parametrize("variant", pm.VARIANTS)
def test_each_wrong_variant_leaves_the_bound_on_its_named_case(cases, variant):
    """at some element of a determined row the wrong definition is more than twice the bound away from the right one: nothing within
    the bound of the one is within the bound of the other"""
    name, tag = CAUGHT_BY[variant]
    c = {c["name"]: c for c in cases}[name]
    d, w = pc.definition(c, pm.L_DEVICE), pc.definition(c, pm.L_DEVICE, variant)
    keep = ~pm.undetermined_rows(d, c["poses"])
    if tag is not None:
        only = np.zeros_like(keep)
        only[c["tags"][tag]] = True
        keep &= only
    assert keep.any()
    far = max(float(pm.excess(w[k], d, k)[keep].max()) for k in ("pose", "dt", "dR"))
    print(f"{variant}: {far:.3g} bounds away on {name}" + (f" rows {tag}" if tag else ""))
    assert far > 2.0, f"{variant} is not told apart by {name}: {c['targets']}"


def test_a_non_finite_row_changes_no_other_row(cases):
    for name in ("aa_rn0.349_n257_tracknet_norm", "6d_n65_tracknet_norm", "deepim_skew_300x104_n257"):
        c = {c["name"]: c for c in cases}[name]
        clean = pc.restatement(c)
        for what, cb, row in pc.nonfinite_variants(c):
            out = pc.restatement(cb)
            others = np.arange(len(c["poses"])) != row
            assert all(_same(o[others], r[others]).all() for o, r in zip(out, clean)), (name, what)
            if not (what.startswith("rot") and "inf" in what and c["rot_rep"] == "axis_angle"):      # tanh(+-inf) = +-1: a finite row
                assert not np.isfinite(out[0][row]).all(), (name, what)


def test_pose_update_refuses_an_out_that_overlaps_poses():
    """poses_in and poses_out are __restrict__ in the kernel: ops.pose_update refuses an in-place update before anything else"""
    import torch
    from foundationpose_amd import _lib, ops
    buf = torch.zeros((6, 4, 4))
    tr, ro = torch.zeros((4, 3)), torch.zeros((4, 3))
    for out in (buf[:4], buf[1:5], buf[:4].view(4, 16)):
        with pytest.raises(_lib.FpAmdError, match="overlap"):
            ops.pose_update(tr, ro, buf[:4], out=out)
    with pytest.raises(_lib.FpAmdError) as e:                 # disjoint halves of one allocation are fine: the next check speaks
        ops.pose_update(tr[:3], ro[:3], buf[:3], out=buf[3:])
    assert "overlap" not in str(e.value)
