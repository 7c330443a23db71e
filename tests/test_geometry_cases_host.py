"""CPU: the generated geometry cases of tests/geometry_cases.py do what they are there for.

1. the integer model of the rasteriser's coverage half (tests/raster_model.py) gives the C oracle's tri_id and zbuf bit for bit on
   every case and pose -- a second implementation that pins oracle/fp_oracle.c;
2. every wrong variant of the model, of the warp and of the filters changes at least one element on the named cases: the cases
   discriminate (a kernel with that mistake would fail tests/test_gpu_geometry_edges.py, which runs the same records);
3. every case reaches what it targets, computed from the oracle and the model alone.

The warp's xyz half, erode_depth and depth_to_xyz are restated in numpy below (with the switches for their wrong variants); each
restatement equals the C oracle bit for bit with no switch set.  bilateral_filter_depth is not restated: its expf is libm's."""
import functools

import numpy as np
import pytest

import geometry_cases as gc
import raster_model as rm
from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

F = np.float32


@pytest.fixture(scope="module")
def sc(scene):
    return scene


@functools.lru_cache(maxsize=None)
def _raster(scene_id):
    scene = _SCENES[scene_id]
    from oracle import ops as oo
    M = gc.meshes(scene)
    out = {}
    for c in gc.raster_cases(scene):
        ref = oo.render_crops(M[c["mesh"]]["np"], c["poses"], c["bbox"], c["K"], c["H"], c["W"], c["out_hw"], c["diameter"],
                              want=("zbuf", "tri_id"))
        mod = [rm.render(M[c["mesh"]]["np"], c["poses"][n], c["bbox"][n], c["K"], c["H"], c["W"], c["out_hw"])
               for n in range(len(c["poses"]))]
        out[c["name"]] = (c, M[c["mesh"]], ref, mod)
    return out


_SCENES = {}


def _rc(scene):
    _SCENES[id(scene)] = scene
    return _raster(id(scene))


# ------------------------------------------------------------------------------------------------------ 1. model == oracle
def test_model_is_the_oracle_on_every_case(sc):
    bad = []
    for name, (c, m, ref, mod) in _rc(sc).items():
        for n, r in enumerate(mod):
            if not (np.array_equal(r["tri_id"], ref["tri_id"][n]) and np.array_equal(r["zbuf"], ref["zbuf"][n])):
                bad.append((name, n))
    assert not bad, f"(case, pose) whose tri_id / zbuf differ between the integer model and the C oracle: {bad}"
    assert len(_rc(sc)) >= 20


def test_fmaf_model_rounds_once():
    """the float32 fma of the model against exact rational arithmetic, on operands built to land on float32 midpoints"""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = rng.standard_normal(4000).astype(F)
    b = rng.standard_normal(4000).astype(F)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(F) * F(1 + 2.0 ** -12)     # heavy cancellation
    c[::2] = rng.standard_normal(2000).astype(F) * F(2.0 ** 20)                          # a * b far below one ulp of c
    c[1::4] = (F(1.0) + np.spacing(F(1.0)) / 2).astype(F)
    got = rm.fmaf(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = F(float(exact))                       # float(Fraction) rounds once to float64: use it only to bracket
        cands = [np.nextafter(lo, F(-np.inf)), lo, np.nextafter(lo, F(np.inf))]
        best = min(cands, key=lambda x: (abs(Fraction(float(x)) - exact), int(np.asarray(x, F).view(np.uint32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i])


# ------------------------------------------------------------------------------------------------ 2. variants are detected
VARIANT_CASES = {"tie_high_id": "twin_faces", "owner_mirror": "pixel_lattice", "draw_culled": "can_near",
                 "bbox_outward": "can_zoom12", "snap_away": "pixel_lattice"}


@pytest.mark.parametrize("variant", rm.VARIANTS)
def test_every_raster_variant_changes_a_pixel(sc, variant):
    c, m, ref, mod = _rc(sc)[VARIANT_CASES[variant]]
    changed = 0
    for n in range(min(len(c["poses"]), 12)):
        r = rm.render(m["np"], c["poses"][n], c["bbox"][n], c["K"], c["H"], c["W"], c["out_hw"], variant=variant)
        changed += int(((r["tri_id"] != ref["tri_id"][n]) | (r["zbuf"] != ref["zbuf"][n])).sum())
    assert changed > 0, f"{variant} is invisible on {c['name']}"


# ------------------------------------------------------------------------------------------------------ 3. reach conditions
def test_slab_stack_overflows_the_queue_of_large_triangles(sc):
    for name in ("slab_up", "slab_down"):
        c, m, ref, mod = _rc(sc)[name]
        assert c["out_hw"] == (160, 160)
        big = max(int(r["big_per_strip"].max()) for r in mod)
        assert big > rm.BIG_MAX, (name, big)
    # ids rising with depth in one, falling in the other: face on, the nearest slab is triangle 0 / 1 there and T-2 / T-1 here
    up, down = _rc(sc)["slab_up"], _rc(sc)["slab_down"]
    assert np.array_equal(up[2]["zbuf"][0], down[2]["zbuf"][0])
    T = len(up[1]["np"]["faces"])
    cu, cd = up[2]["tri_id"][0], down[2]["tri_id"][0]
    assert np.array_equal(np.where(cu >= 0, T - 2 - 2 * (cu // 2) + cu % 2, -1), cd)


def test_twin_faces_every_pixel_is_a_tie_won_by_the_lower_id(sc):
    c, m, ref, mod = _rc(sc)["twin_faces"]
    T = len(m["np"]["faces"])
    tid = ref["tri_id"]
    assert (tid[tid >= 0] < T // 2).all()
    assert min((tid[n] >= 0).mean() for n in range(len(tid))) > 0.10


def test_sliver_soup_degenerates_and_survivors(sc):
    c, m, ref, mod = _rc(sc)["sliver_soup"]
    for n, r in enumerate(mod):
        frac = float(r["zero_area"].mean())
        assert 0.10 < frac < 0.90, (n, frac)
        assert len(np.unique(ref["tri_id"][n][ref["tri_id"][n] >= 0])) >= 200, n
    # the coplanar pairs: where one of the first 200 triangles wins, its twin (the same key but for the id) never does
    T = len(m["np"]["faces"])
    assert not (ref["tri_id"] >= T - 200).any() and (ref["tri_id"][(ref["tri_id"] >= 0)] < 200).any()


def test_cull_cases_cull_some_vertices_and_still_draw(sc):
    seen = 0
    for name, (c, m, ref, mod) in _rc(sc).items():
        if "cull" in c["tags"]:
            seen += 1
            for n, r in enumerate(mod):
                culled = int((~r["valid"]).sum())
                assert 0 < culled < len(r["valid"]), (name, n, culled)
                assert (ref["tri_id"][n] >= 0).any(), (name, n)
        if "cull_empty" in c["tags"]:
            seen += 1
            r = mod[0]
            assert 0 < int((~r["valid"]).sum()) < len(r["valid"]) and not (ref["tri_id"][0] >= 0).any(), name
    assert seen >= 3


def test_far_case_sits_on_the_depth_clamp(sc):
    c, m, ref, mod = _rc(sc)["can_far"]
    cov = ref["tri_id"] >= 0
    assert cov.sum() > 3000 and (ref["zbuf"][cov] == 0xFFF00000).all()


def test_other_raster_targets(sc):
    R = _rc(sc)
    # back faces win: triangles whose snapped orientation is negative (swapped by the orientation fix) own pixels
    c, m, ref, mod = R["half_cylinder"]
    assert all((ref["tri_id"][n] >= 0).any() for n in range(len(mod)))
    # interpenetration: both boxes own pixels in one crop
    c, m, ref, mod = R["crossed_boxes"]
    half = len(m["np"]["faces"]) // 2
    both = [n for n in range(len(mod)) if ((ref["tri_id"][n] >= half).any() and ((ref["tri_id"][n] >= 0) & (ref["tri_id"][n] < half)).any())]
    assert len(both) >= len(mod) // 2
    # the lattice: every vertex on a pixel centre (snapped x = 8 mod 16) in the unshifted poses
    c, m, ref, mod = R["pixel_lattice"]
    xi, yi, _, ok = rm.project(m["np"]["pos"], c["poses"][0], c["bbox"][0], c["K"], c["H"], c["W"], *c["out_hw"])
    assert ok.all() and (xi % 16 == 8).all() and (yi % 16 == 8).all()
    # uv beyond [0, 1] and a uv table in another order than the vertices
    t = gc.meshes(sc)["tex_2x3"]["np"]
    assert t["uv"].min() < -1.4 and t["uv"].max() > 2.4 and not np.array_equal(t["uv_idx"], t["faces"]) and t["tex"].shape[:2] == (2, 3)
    assert (gc.meshes(sc)["zero_normals"]["np"]["vnormals"][::3] == 0).all()
    assert {c["out_hw"] for c, *_ in R.values()} >= set(gc.OUT_SIZES)
    assert {(c["H"], c["W"]) for c, *_ in R.values()} >= set(gc.FRAMES[:2])


# ------------------------------------------------------------------------------------------------ the warp, restated
def _nn(x, away):
    with np.errstate(all="ignore"):
        r = np.sign(x) * np.floor(np.abs(x) + F(0.5)) if away else np.rint(x)
    return np.clip(np.nan_to_num(r, nan=0.0), -2.0 ** 30, 2.0 ** 30).astype(np.int64)


def warp_xyz_np(c, mode, normalize, variant=None, tf=None, poses=None):
    """channels 3..5 of fpo_warp_crops (the nearest read of the xyz map / the scorer's depth chain, and the normalisation), float32
    op for op.  variant: 'nn_away' (nn_index rounds halves away), 'thr_le' (pt[2] <= thr), 'two_gt' (|val| > 2).
    -> (B[:, 3:6], pt_z, val before the threshold tests)"""
    from oracle import ops as oo
    tf = np.asarray(c["tf"] if tf is None else tf, F)
    P = np.asarray(c["poses"] if poses is None else poses, F)
    H, W, (oh, ow) = c["H"], c["W"], c["out_hw"]
    K9 = np.asarray(c["K"], np.float64).astype(F).reshape(9)
    away = variant == "nn_away"
    sx, tx, sy, ty = (tf[:, a, b][:, None, None] for a, b in ((0, 0), (0, 2), (1, 1), (1, 2)))
    with np.errstate(all="ignore"):
        i00, i11 = F(1) / sx, F(1) / sy
        i02, i12 = (-tx) / sx, (-ty) / sy
        cW, cH = F(W) / F(W - 1), F(H) / F(H - 1)
        cSw, cSh = F(ow) / F(ow - 1), F(oh) / F(oh - 1)
        ii = np.arange(ow, dtype=F)[None, None, :]
        jj = np.arange(oh, dtype=F)[None, :, None]
        ix = rm.fmaf(rm.fmaf(ii, i00, i02), cW, F(-0.5)) + np.zeros((1, oh, 1), F)
        iy = rm.fmaf(rm.fmaf(jj, i11, i12), cH, F(-0.5)) + np.zeros((1, 1, ow), F)
        qx, qy = _nn(ix, away), _nn(iy, away)
        q_in = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        cqx, cqy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
        if mode == oo.MODE_REFINE:
            pt = np.where(q_in[..., None], c["xyz"][cqy, cqx], F(0))
            thr = F(0.001)
        else:
            lfx, lfy = np.rint(i02), np.rint(i12)
            fqx, fqy = qx.astype(F), qy.astype(F)
            ccx = np.where(np.abs(i02 - lfx) <= F(1e-3), sx * (fqx - lfx), rm.fmaf(sx, fqx, tx))
            ccy = np.where(np.abs(i12 - lfy) <= F(1e-3), sy * (fqy - lfy), rm.fmaf(sy, fqy, ty))
            px, py = _nn(rm.fmaf(ccx, cSw, F(-0.5)), away), _nn(rm.fmaf(ccy, cSh, F(-0.5)), away)
            p_in = (px >= 0) & (px < ow) & (py >= 0) & (py < oh)
            rx = _nn(rm.fmaf(rm.fmaf(px.astype(F), i00, i02), cW, F(-0.5)), away)
            ry = _nn(rm.fmaf(rm.fmaf(py.astype(F), i11, i12), cH, F(-0.5)), away)
            r_in = (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
            z = np.where(q_in & p_in & r_in, c["depth"][np.clip(ry, 0, H - 1), np.clip(rx, 0, W - 1)], F(0))
            keep = q_in & ~(z < F(0.001))
            x = ((fqx - K9[2]) * z) / K9[0]
            y = ((fqy - K9[5]) * z) / K9[4]
            pt = np.where(keep[..., None], np.stack([x, y, z], -1), F(0))
            thr = F(0.1)
        invalid = (pt[..., 2] <= thr) if variant == "thr_le" else (pt[..., 2] < thr)
        val = pt - P[:, None, None, :3, 3]
        raw = val
        if normalize:
            inv_r = F(1) / (F(c["diameter"]) * F(0.5))
            val = val * inv_r
            raw = val
            big = (np.abs(val) > F(2)) if variant == "two_gt" else (np.abs(val) >= F(2))
            val = np.where(invalid[..., None] | big, F(0), val)
    return np.ascontiguousarray(np.moveaxis(val, -1, 1)), pt[..., 2], raw


@functools.lru_cache(maxsize=None)
def _warp(scene_id):
    return gc.warp_cases(_SCENES[scene_id])


def test_warp_restatement_is_the_oracle_and_variants_are_detected(sc):
    from oracle import ops as oo
    _SCENES[id(sc)] = sc
    changed = {v: 0 for v in ("nn_away", "thr_le", "two_gt")}
    on_thr = {oo.MODE_REFINE: 0, oo.MODE_SCORE: 0}
    on_two = {oo.MODE_REFINE: 0, oo.MODE_SCORE: 0}
    sizes = set()
    for c in _warp(id(sc)):
        sizes.add(c["out_hw"])
        for mode in (oo.MODE_REFINE, oo.MODE_SCORE):
            for normalize in (True, False):
                ref = oo.warp_crops(c["rgb"], c["xyz"], c["depth"], c["tf"], c["K"], c["poses"], c["diameter"], mode, normalize, c["out_hw"])
                got, ptz, raw = warp_xyz_np(c, mode, normalize)
                assert np.array_equal(got.view(np.uint32), ref[:, 3:6].view(np.uint32)), (c["name"], mode, normalize)
                if not normalize:
                    continue
                on_thr[mode] += int((ptz == (F(0.001) if mode == oo.MODE_REFINE else F(0.1))).sum())
                on_two[mode] += int((np.abs(raw) == F(2)).sum())
                for v in changed:
                    alt, _, _ = warp_xyz_np(c, mode, normalize, variant=v)
                    changed[v] += int((alt.view(np.uint32) != got.view(np.uint32)).sum())
    assert all(n > 0 for n in changed.values()), changed
    # elements exactly on each threshold, over all cases: at least 1000 per mode on pt[2] == thr and on |val| == 2
    assert min(on_thr.values()) >= 1000 and min(on_two.values()) >= 1000, (on_thr, on_two)
    assert {hw[1] for hw in sizes} >= {2, 3, 1023, 1024}


# --------------------------------------------------------------------------------------------- the filters, restated
def erode_np(d, radius=2, diff=0.001, ratio=0.8, zfar=100.0, variant=None):
    """fpo_erode_depth.  variant: 'ratio_ge' (bad / total >= ratio_thres), 'zfar_gt' (cur > zfar).  -> (out, bad, total)"""
    d = np.asarray(d, F)
    H, W = d.shape
    bad = np.zeros((H, W), F)
    total = np.zeros((H, W), F)
    diff, ratio, zfar = F(diff), F(ratio), F(zfar)
    with np.errstate(all="ignore"):
        for du in range(-radius, radius + 1):
            for dv in range(-radius, radius + 1):
                h0, h1, w0, w1 = max(0, -dv), min(H, H - dv), max(0, -du), min(W, W - du)
                if h0 >= h1 or w0 >= w1:
                    continue
                cur = d[h0 + dv:h1 + dv, w0 + du:w1 + du]
                d0 = d[h0:h1, w0:w1]
                far = (cur > zfar) if variant == "zfar_gt" else (cur >= zfar)
                isbad = (cur < F(0.001)) | far | (np.abs(cur - d0) > diff)
                total[h0:h1, w0:w1] += F(1)
                bad[h0:h1, w0:w1] += isbad.astype(F)
        r = bad / total
        zero = (r >= ratio) if variant == "ratio_ge" else (r > ratio)
    return np.where(zero, F(0), d), bad, total


def xyz_np(d, K, zfar, variant=None):
    """fpo_depth_to_xyz, the float32 (batch) variant.  variant 'zfar_ge': z >= zfar is dropped too"""
    d = np.asarray(d, F)
    H, W = d.shape
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = F(K[0, 0]), F(K[1, 1]), F(K[0, 2]), F(K[1, 2])
    u = np.arange(W, dtype=F)[None, :]
    v = np.arange(H, dtype=F)[:, None]
    with np.errstate(all="ignore"):
        drop = (d < F(0.001)) | ((d >= F(zfar)) if variant == "zfar_ge" else (d > F(zfar)))
        out = np.stack([((u - cx) * d) / fx, ((v - cy) * d) / fy, d + np.zeros_like(d)], -1)
    return np.where(drop[..., None], F(0), out).astype(F)


def test_filter_restatements_are_the_oracle_and_variants_are_detected():
    from oracle import ops as oo
    changed = dict(ratio_ge=0, zfar_gt=0, zfar_ge=0)
    ties = 0
    for c in gc.filter_cases():
        d, zfar = c["depth"], c["zfar"]
        for radius in range(4):
            ref = oo.erode_depth(d, radius, 0.001, 0.8, zfar)
            got, bad, total = erode_np(d, radius, 0.001, 0.8, zfar)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (c["name"], radius)
            for v in ("ratio_ge", "zfar_gt"):
                alt = erode_np(d, radius, 0.001, 0.8, zfar, variant=v)[0]
                changed[v] += int((alt.view(np.uint32) != got.view(np.uint32)).sum())
            if radius == 2:
                for (h, w, nbad, ntot) in c["ties"]:
                    assert bad[h, w] == nbad and total[h, w] == ntot, (c["name"], h, w, bad[h, w], total[h, w])
                if c["ties"]:
                    with np.errstate(all="ignore"):
                        ties += int((bad / total == F(0.8)).sum())
                    on = [(h, w) for (h, w, nbad, ntot) in c["ties"] if F(nbad) / F(ntot) == F(0.8)]
                    assert len(on) == 2 and all(ref[h, w] == d[h, w] != 0 for h, w in on)        # 20 / 25 and 12 / 15: kept
                    assert all(ref[h, w] == 0 for (h, w, nbad, ntot) in c["ties"] if nbad / ntot > 0.8)
        for K in (gc.K_SKEW, gc.K_DYADIC):
            ref = oo.depth2xyzmap(d, K, zfar=zfar, f64_internal=False)
            got = xyz_np(d, K, zfar)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), c["name"]
            changed["zfar_ge"] += int((xyz_np(d, K, zfar, "zfar_ge").view(np.uint32) != got.view(np.uint32)).sum())
    assert all(n > 0 for n in changed.values()), changed
    assert ties >= 4, ties                                  # at least the planted interior and border ties of both large frames
    assert {c["depth"].shape for c in gc.filter_cases()} == set(gc.FILTER_SIZES)


def test_crop_window_cases_hit_ties_and_collapse():
    from oracle import ops as oo
    cases = {c["name"]: c for c in gc.crop_window_cases()}
    c = cases["half_integer_ties"]
    tf, bb = oo.crop_windows(c["poses"], c["K"], c["diameter"], c["ratio"], c["out_size"])
    # t = (0.25, 0.25, 1): edges 384.5 / 512.5 -> 384 / 512 (half to even), so left = top = 384 and a scale of 160 / 128
    assert tf[0, 0, 0] == F(1.25) and tf[0, 0, 2] == F(-480.0) and tf[0, 1, 2] == F(-480.0)
    # t = (0.25 + 2^-9, ...): edges 385.5 / 513.5 -> 386 / 514
    assert tf[3, 0, 0] == F(1.25) and tf[3, 0, 2] == F(-482.5)
    P64 = c["poses"].astype(np.float64)
    u0 = c["K"][0, 0] * P64[:, 0, 3] / P64[:, 2, 3] + c["K"][0, 2]
    rad = c["K"][0, 0] * 0.125 / P64[:, 2, 3]
    assert (((u0 - rad) % 1.0 == 0.5) | ((c["K"][1, 1] * P64[:, 1, 3] / P64[:, 2, 3] + c["K"][1, 2] - rad) % 1.0 == 0.5)).all()
    c = cases["degenerate_depths"]
    tf, bb = oo.crop_windows(c["poses"], c["K"], c["diameter"], c["ratio"], c["out_size"])
    assert np.isinf(tf[6, 0, 0]) and np.isnan(bb[6]).any(), "0.17 m at 5 000 m: right == left"
    assert np.isfinite(tf[5]).all()          # the same object a little to the side straddles a half integer and keeps one pixel
    assert not np.isfinite(tf[0]).all() and not np.isfinite(tf[7]).all()
    assert {len(cases[k]["poses"]) for k in ("n_0", "n_1", "n_257")} == {0, 1, 257}
