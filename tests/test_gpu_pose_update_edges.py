"""GPU: k_pose_update (csrc/frame_ops.hip) through ops.pose_update in its three forms (fp_pose_update, _multi, _views) on the
generated cases of tests/pose_update_cases.py, against the float64 definition, its running error bound and the float32 restatement
of tests/pose_update_model.py (tests/test_pose_update_cases_host.py shows on the CPU that the oracle meets the same bound, that
every case reaches its target and that the cases tell wrong variants of the definition from the right one).

  * every element of every determined row lies within the bound of the definition with the device's L_f (pose_update_model.L_DEVICE,
    from the measured profiles/libm_ulp_gfx950.json); the rows left out are the ones the generator flags, nothing else;
  * wherever no libm call enters -- the 6d rotation, the 'deepim' delta, 'raw' and normalised 'tracknet' translations, R = I at a
    zero rotation -- the kernel's bits are the restatement's, NaN == NaN and degenerate rows included;
  * the multi and views forms give the bits of the single call with that row's diameter and K; indices outside their tables give
    the NaN the header promises;
  * outputs sit in poisoned arenas: only rows 0..N-1 change, nothing when N = 0; two calls and a captured graph give the same bits.

The worst error-to-bound ratio per case is merged into $FP_GEOMETRY_REPORT_DIR/pose_update_edges.json when that variable names a
directory (nothing is written otherwise); the record of the MI355X run is committed as profiles/pose_update_edges.json."""
import json
import os

import numpy as np
import pytest
import torch

import pose_update_cases as pc
import pose_update_model as pm

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
PAD = 4096
POISON = -7.0
REPORT = {}
KEYS = ("pose", "dt", "dR")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(scene):
    return pc.cases(scene)


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    out = os.environ.get("FP_GEOMETRY_REPORT_DIR")
    if REPORT and out:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "pose_update_edges.json")
        merged = {}
        if os.path.exists(path):
            try:
                with open(path) as f:
                    merged = json.load(f)
            except Exception:
                merged = {}
        merged.update(REPORT)
        with open(path, "w") as f:
            json.dump(merged, f, indent=1, sort_keys=True)


def _t(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x), device=dev)


def _same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(U) == b.view(U)) | (np.isnan(a) & np.isnan(b))


class Arena:
    """an output placed inside a poisoned buffer"""

    def __init__(self, shape, dev):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), POISON, dtype=torch.float32, device=dev)
        self.view = self.buf[PAD:PAD + n].view(*shape)
        self.n = n

    def intact(self):
        return bool((self.buf[:PAD] == POISON).all()) and bool((self.buf[PAD + self.n:] == POISON).all())


def _views_table(c, dev):
    """ops.Views refuses an index outside 0..V-1 on the host; the kernel's own promise for such an index is what is under test, so
    the device index is put in behind it"""
    from foundationpose_amd import ops
    if c["view"] is None:
        return ops.Views(list(c["Ks"]), None, dev)
    vt = ops.Views(list(c["Ks"]), np.clip(c["view"], 0, len(c["Ks"]) - 1), dev)
    vt.dev = _t(c["view"].astype(np.int32), dev)
    return vt


def _call(c, dev, rows=None, want=(True, True), form=None, diameter=None, K=None):
    """ops.pose_update on the case (or on its rows `rows`) -> (pose, dt | None, dR | None) as numpy, arenas.  form / diameter / K
    override the case's: the single form with one row's diameter and K."""
    from foundationpose_amd import ops
    sel = slice(None) if rows is None else rows
    tr, ro, P = _t(c["trans"][sel], dev), _t(c["rot"][sel], dev), _t(c["poses"][sel], dev)
    N = int(P.shape[0])
    form = form or c["form"]
    ar = (Arena((N, 4, 4), dev), Arena((N, 3), dev) if want[0] else None, Arena((N, 3, 3), dev) if want[1] else None)
    kw = dict(rot_rep=c["rot_rep"], normalize_xyz=c["normalize_xyz"], trans_normalizer=c["trans_normalizer"], rot_normalizer=c["rot_normalizer"],
              out=ar[0].view, trans_delta_out=None if ar[1] is None else ar[1].view, rot_delta_out=None if ar[2] is None else ar[2].view,
              trans_rep="raw_xyz" if c["trans_rep"] == "raw" else c["trans_rep"])
    if c["trans_rep"] == "deepim":
        kw.update(tf_to_crops=_t(c["tf"][sel], dev), input_w=c["input_w"])
    if form == "single":
        kw.update(mesh_diameter=c["diameter"] if diameter is None else diameter, K=c["K"] if K is None else K)
    else:
        kw.update(mesh_diameter=ops.object_diameters(c["diameters"], dev), obj=None if c["obj"] is None else _t(c["obj"][sel], dev))
        if form == "views":
            assert rows is None
            kw.update(views=_views_table(c, dev))
        else:
            kw.update(K=c["K"])
    ops.pose_update(tr, ro, P, **kw)
    torch.cuda.synchronize()
    return tuple(None if a is None else a.view.cpu().numpy() for a in ar), ar


def test_every_case_within_the_bound_bit_equal_where_exact_in_arenas(cases, dev):
    failures, rep = [], {}
    I3 = np.eye(3, dtype=F)
    for c in cases:
        name, N = c["name"], len(c["poses"])
        out, ar = _call(c, dev)
        assert all(a.intact() for a in ar), f"{name}: a write outside rows 0..N-1 of an output"
        again, _ = _call(c, dev)
        if not all(_same(a, b).all() for a, b in zip(out, again)):
            failures.append(f"{name}: two calls differ")
        d = pc.definition(c, pm.L_DEVICE)
        und = pm.undetermined_rows(d, c["poses"])
        assert np.array_equal(und, pc.flagged(c)), (name, np.flatnonzero(und), np.flatnonzero(pc.flagged(c)))
        keep = ~und
        r = dict(rows=N, rows_left_out=int(und.sum()))
        for o, key in zip(out, KEYS):
            ex = pm.excess(o, d, key)[keep]
            ok = np.isfinite(o[keep]).all()
            r[key + "_worst_error_to_bound"] = float(ex.max(initial=0.0))
            print(f"{name:42s} {key:5s} error / bound {r[key + '_worst_error_to_bound']:.3f}")
            if not (ok and (ex <= 1.0).all()):
                where = np.argwhere(~(pm.excess(o, d, key) <= 1.0) & keep.reshape((-1,) + (1,) * (o.ndim - 1)))[:4].tolist()
                failures.append(f"{name}: {key} leaves the bound (worst {ex.max(initial=0.0):.3g} bounds) at {where}")
        rs = pc.restatement(c)
        rot_libm, trans_libm = pc.uses_libm(c)
        nb = {}
        if not trans_libm:
            nb["translation"] = int((~_same(out[0][:, :3, 3], rs[0][:, :3, 3])).sum() + (~_same(out[1], rs[1])).sum())
        if not rot_libm:
            nb["rotation"] = int((~_same(out[0][:, :3, :3], rs[0][:, :3, :3])).sum() + (~_same(out[2], rs[2])).sum())
        nb["last_row"] = int((~_same(out[0][:, 3], rs[0][:, 3])).sum())
        for k in c["tags"].get("zero_rot", []) if c["rot_rep"] == "axis_angle" else []:
            if k not in c["nan_rows"].get("all", []):
                nb["zero_rot"] = nb.get("zero_rot", 0) + int((~_same(out[2][k], I3)).sum() + (~_same(out[0][k, :3, :3], c["poses"][k, :3, :3])).sum())
        r["not_bit_equal_to_the_restatement"] = nb
        for what, n in nb.items():
            if n:
                failures.append(f"{name}: {what}: {n} elements are not the restatement's bits")
        for k in c["nan_rows"].get("translation", []):
            if not (np.isnan(out[0][k, :3, 3]).all() and np.isnan(out[1][k]).all() and np.isfinite(out[0][k, :3, :3]).all()):
                failures.append(f"{name}: row {k} (obj outside 0..M-1) is not a NaN translation beside a finite rotation")
        for k in c["nan_rows"].get("all", []):
            if not all(np.isnan(o[k]).all() for o in out):
                failures.append(f"{name}: row {k} (view outside 0..V-1) is not NaN in every output")
        rep[name] = r
    REPORT["pose_update"] = rep
    REPORT["pose_update_L_f"] = pm.L_DEVICE
    assert not failures, "\n".join(failures)


def test_multi_and_views_rows_are_the_single_call_s_bits(cases, dev):
    """every row of a multi / views case against fp_pose_update called with that row's diameter and K (rows grouped by the pair);
    a row whose object index is outside the table has no single call: its rotation block is compared instead (any diameter)"""
    checked = 0
    for c in cases:
        if c["form"] == "single":
            continue
        N = len(c["poses"])
        out, _ = _call(c, dev)
        d = np.broadcast_to(np.asarray(pc.row_diameters(c), np.float64), (N,))
        v = np.zeros(N, np.int64) if c["form"] != "views" or c["view"] is None else c["view"].astype(np.int64)
        Ks = [c["K"]] if c["form"] != "views" else list(c["Ks"])
        skip = set(c["nan_rows"].get("all", []))
        groups = {}
        for n in range(N):
            if n not in skip:
                groups.setdefault((float(d[n]) if not np.isnan(d[n]) else None, int(v[n])), []).append(n)
        for (dia, vi), rows in groups.items():
            one, _ = _call(c, dev, rows=np.asarray(rows), form="single", diameter=1.0 if dia is None else dia, K=Ks[vi])
            for o, s, key in zip(out, one, KEYS):
                a, b = o[rows], s
                if dia is None and c["normalize_xyz"]:
                    if key == "dt":
                        continue
                    a, b = (a[:, :3, :3], b[:, :3, :3]) if key == "pose" else (a, b)
                assert _same(a, b).all(), (c["name"], key, dia, vi)
            checked += len(rows)
    assert checked > 100


@pytest.mark.parametrize("name", ["aa_rn0.349_n257_tracknet_norm", "deepim_dyadic_hand_windows_6d", "views_v3_deepim"])
def test_optional_outputs_in_every_combination(cases, dev, name):
    c = {c["name"]: c for c in cases}[name]
    full, _ = _call(c, dev)
    for want in ((True, False), (False, True), (False, False)):
        out, ar = _call(c, dev, want=want)
        assert all(a.intact() for a in ar if a is not None), (name, want)
        assert _same(out[0], full[0]).all(), (name, want)
        for k in (1, 2):
            assert (out[k] is None) == (not want[k - 1])
            assert out[k] is None or _same(out[k], full[k]).all(), (name, want, KEYS[k])


@pytest.mark.parametrize("name", ["aa_rn0.349_n257_tracknet_norm", "6d_n65_tracknet_norm", "deepim_skew_300x104_n257", "multi_m3_interleaved"])
def test_a_non_finite_row_changes_no_other_row(cases, dev, name):
    c = {c["name"]: c for c in cases}[name]
    clean, _ = _call(c, dev)
    for what, cb, row in pc.nonfinite_variants(c):
        out, ar = _call(cb, dev)
        assert all(a.intact() for a in ar), (name, what)
        others = np.arange(len(c["poses"])) != row
        for o, r, key in zip(out, clean, KEYS):
            assert _same(o[others], r[others]).all(), (name, what, key)
        rs = pc.restatement(cb)
        rot_libm, trans_libm = pc.uses_libm(cb)
        if not trans_libm:
            assert _same(out[1][row], rs[1][row]).all(), (name, what)          # NaN == NaN, an infinity's sign included
        if not rot_libm:
            assert _same(out[2][row], rs[2][row]).all(), (name, what)


@pytest.mark.parametrize("name", ["aa_rn0.349_n257_tracknet_norm", "multi_m3_interleaved", "views_v3_deepim"])
def test_a_captured_graph_replays_to_the_same_bits(cases, dev, name):
    from foundationpose_amd import ops
    c = {c["name"]: c for c in cases}[name]
    N = len(c["poses"])
    eager, _ = _call(c, dev)
    tr, ro, P = _t(c["trans"], dev), _t(c["rot"], dev), _t(c["poses"], dev)
    outs = (torch.zeros((N, 4, 4), device=dev), torch.zeros((N, 3), device=dev), torch.zeros((N, 3, 3), device=dev))
    kw = dict(rot_rep=c["rot_rep"], normalize_xyz=c["normalize_xyz"], trans_normalizer=c["trans_normalizer"], rot_normalizer=c["rot_normalizer"],
              out=outs[0], trans_delta_out=outs[1], rot_delta_out=outs[2], trans_rep=c["trans_rep"])
    if c["trans_rep"] == "deepim":
        kw.update(tf_to_crops=_t(c["tf"], dev), input_w=c["input_w"])
    if c["form"] == "single":
        kw.update(mesh_diameter=c["diameter"], K=c["K"])
    else:
        kw.update(mesh_diameter=ops.object_diameters(c["diameters"], dev), obj=None if c["obj"] is None else _t(c["obj"], dev))
        kw.update(views=_views_table(c, dev)) if c["form"] == "views" else kw.update(K=c["K"])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.pose_update(tr, ro, P, **kw)                 # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.pose_update(tr, ro, P, **kw)
    for rep in range(2):
        for o in outs:
            o.fill_(POISON)
        g.replay()
        torch.cuda.synchronize()
        for o, e, key in zip(outs, eager, KEYS):
            assert _same(o.cpu().numpy(), e).all(), (name, rep, key)
