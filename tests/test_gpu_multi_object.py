"""GPU: several objects per refine call -- a per-hypothesis object index from the multi-mesh rasteriser (fp_render_crops with a set) up to
estimater.track_objects.  Every hypothesis of a multi-object call must see what a call for its own object alone computes: the
kernels bit for bit against their scalar form, the refine loop against per-object calls, the graphed tracker against its
eager loop, and the estimator against per-object track_one."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ seeded test meshes (mesh.py only makes cans)
def _box(size=(0.08, 0.05, 0.12), n=6, seed=1):
    """vertex-coloured box, every face an n x n grid (separate vertices per face: sharp normals)"""
    from foundationpose_amd.mesh import SimpleMesh
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
                    a, b, c, d = base + j * (n + 1) + i, base + j * (n + 1) + i + 1, base + (j + 1) * (n + 1) + i, base + (j + 1) * (n + 1) + i + 1
                    # outward orientation: (u x v) points along +axis for the cyclic order (axis, u, v)
                    outward = sgn * (1.0 if (u - axis) % 3 == 1 else -1.0)
                    faces += [[a, b, d], [a, d, c]] if outward > 0 else [[a, d, b], [a, c, d]]
    rng = np.random.default_rng(seed)
    cols = (rng.uniform(0.15, 1.0, size=(len(verts), 3)) * 255).astype(np.uint8)
    return SimpleMesh(np.asarray(verts), np.asarray(faces), vertex_colors=cols)


def _torus(R=0.045, r=0.017, nu=48, nv=20, textured=True, seed=3):
    """the concave one: a torus, textured through a (nu+1) x (nv+1) uv grid"""
    from foundationpose_amd.mesh import SimpleMesh, make_texture
    verts, uvs, faces = [], [], []
    for j in range(nv + 1):
        b = 2 * np.pi * j / nv
        for i in range(nu + 1):
            a = 2 * np.pi * i / nu
            verts.append([(R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)])
            uvs.append([i / nu, j / nv])
    for j in range(nv):
        for i in range(nu):
            a0 = j * (nu + 1) + i
            a1, b0 = a0 + 1, a0 + nu + 1
            faces += [[a0, a1, b0 + 1], [a0, b0 + 1, b0]]
    if textured:
        return SimpleMesh(np.asarray(verts), np.asarray(faces), uv=np.asarray(uvs), texture=make_texture(256, seed))
    rng = np.random.default_rng(seed)
    return SimpleMesh(np.asarray(verts), np.asarray(faces), vertex_colors=(rng.uniform(0.2, 1, (len(verts), 3)) * 255).astype(np.uint8))


def _diameter(mesh):
    v = np.asarray(mesh.vertices)
    return float(np.linalg.norm(v.max(0) - v.min(0)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def meshes(scene):
    from foundationpose_amd.mesh import make_can_mesh
    m = dict(can=scene["mesh"], box=_box(), torus=_torus(),
             small_can=make_can_mesh(radius=0.03, height=0.07, n_ang=24, n_axial=10, textured=False, seed=7),
             big=make_can_mesh(radius=0.04, height=0.10, n_ang=300, n_axial=120, textured=False, seed=9))
    assert len(m["big"].faces) > 65535 and len(m["torus"].faces) <= 65535
    return m


@pytest.fixture(scope="module")
def gmeshes(meshes, dev):
    from foundationpose_amd.Utils import make_mesh_tensors
    return {k: make_mesh_tensors(v, device=dev) for k, v in meshes.items()}


@pytest.fixture(scope="module")
def frame(scene, dev):
    from oracle import ops as oo
    from oracle import pipeline as op
    d = op.preprocess_depth(scene["depth"])
    xyz = oo.depth2xyzmap(d, scene["K"], f64_internal=True)
    return dict(depth_f=d, xyz=xyz, rgb_t=torch.as_tensor(scene["rgb"], device=dev).float().contiguous(),
                depth_t=torch.as_tensor(d, device=dev), xyz_t=torch.as_tensor(xyz, device=dev))


def _t(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x), device=dev)


def _poses(scene, n, seed, max_trans=0.02, max_rot_deg=60.0):
    from foundationpose_amd import synthetic as syn
    return syn.perturbed_poses(scene["gt"], n, seed=seed, max_trans=max_trans, max_rot_deg=max_rot_deg).astype(np.float32)


def _interleaved(M, N, seed):
    """an object index in which every object occurs and neighbours mostly differ"""
    rng = np.random.default_rng(seed)
    obj = np.concatenate([np.arange(M), rng.integers(0, M, N - M)])
    rng.shuffle(obj)
    return obj.astype(np.int32)


def _set(names, meshes, gmeshes, dev):
    from foundationpose_amd import ops
    from foundationpose_amd.Utils import get_mesh_handle
    handles = [get_mesh_handle(gmeshes[k]) for k in names]
    return ops.MeshSet(handles), handles, [_diameter(meshes[k]) for k in names]


# ------------------------------------------------------------------ 1. the multi-mesh rasteriser
ALL_OUT = ("A", "color", "depth", "xyz", "normal", "zbuf", "tri_id")


@pytest.mark.parametrize("names", [("can", "box", "torus", "small_can"), ("box", "big", "can", "torus")], ids=["lists16", "lists32"])
def test_render_multi_is_the_per_mesh_render(scene, dev, meshes, gmeshes, names):
    """64 hypotheses over four distinct meshes (texture and vertex colour, different V / T, a concave one; the second set has a
    mesh over the 16-bit list limit), objects interleaved, 160 x 160 crops: every output of every hypothesis is bit-identical to
    fp_render_crops with that hypothesis' own mesh and diameter, and zbuf / tri_id bit-exact against the CPU oracle"""
    from foundationpose_amd import ops
    from oracle import ops as oo
    from oracle import pipeline as op
    mset, handles, diam = _set(names, meshes, gmeshes, dev)
    assert mset.M == 4 and mset.T == max(h.T for h in handles) and mset.V == max(h.V for h in handles)
    N = 64
    obj = _interleaved(4, N, seed=11)
    P = _poses(scene, N, seed=12)
    Pt, ot, dt = _t(P, dev), _t(obj, dev), ops.object_diameters(diam, dev)
    tf, bb = ops.crop_windows(Pt, scene["K"], dt, 1.2, (160, 160), obj=ot)
    out = ops.render_crops(mset, Pt, bb, scene["K"], 480, 640, (160, 160), mesh_diameter=dt, want=ALL_OUT, obj=ot)
    for k in range(4):
        rows = np.nonzero(obj == k)[0]
        r = torch.as_tensor(rows, device=dev)
        ref = ops.render_crops(handles[k], Pt[r].contiguous(), bb[r].contiguous(), scene["K"], 480, 640, (160, 160),
                               mesh_diameter=diam[k], want=ALL_OUT)
        for name in ALL_OUT:
            assert torch.equal(out[name][r], ref[name]), (names[k], name)
        sub = rows[:8]
        cpu = oo.render_crops(op.mesh_tensors_np(meshes[names[k]]), P[sub], bb[torch.as_tensor(sub, device=dev)].cpu().numpy(),
                              scene["K"], 480, 640, (160, 160), want=("zbuf", "tri_id"))
        assert np.array_equal(out["tri_id"][r[:8]].cpu().numpy(), cpu["tri_id"]), names[k]
        assert np.array_equal(out["zbuf"][r[:8]].cpu().numpy().view(np.uint32), cpu["zbuf"]), names[k]
        assert all((cpu["tri_id"][i] >= 0).mean() > 0.02 for i in range(len(sub))), names[k]      # every hypothesis draws something
        assert int(out["tri_id"][r].max()) < handles[k].T


def test_render_multi_full_frame(scene, dev, meshes, gmeshes):
    """the full-frame form (no bbox, 480 x 640): per hypothesis the bits of the single-mesh render, zbuf / tri_id the oracle's"""
    from foundationpose_amd import ops
    from oracle import ops as oo
    from oracle import pipeline as op
    names = ("can", "torus", "box", "big")
    mset, handles, diam = _set(names, meshes, gmeshes, dev)
    obj = np.asarray([2, 0, 3, 1, 0, 2, 1, 3], dtype=np.int32)
    P = _poses(scene, len(obj), seed=21)
    Pt, ot, dt = _t(P, dev), _t(obj, dev), ops.object_diameters(diam, dev)
    out = ops.render_crops(mset, Pt, None, scene["K"], 480, 640, (480, 640), mesh_diameter=dt, want=ALL_OUT, obj=ot)
    for k in range(4):
        rows = np.nonzero(obj == k)[0]
        r = torch.as_tensor(rows, device=dev)
        ref = ops.render_crops(handles[k], Pt[r].contiguous(), None, scene["K"], 480, 640, (480, 640), mesh_diameter=diam[k],
                               want=ALL_OUT)
        for name in ALL_OUT:
            assert torch.equal(out[name][r], ref[name]), (names[k], name)
        cpu = oo.render_crops(op.mesh_tensors_np(meshes[names[k]]), P[rows], None, scene["K"], 480, 640, (480, 640),
                              want=("zbuf", "tri_id"))
        assert np.array_equal(out["tri_id"][r].cpu().numpy(), cpu["tri_id"]) and (cpu["tri_id"] >= 0).any()
        assert np.array_equal(out["zbuf"][r].cpu().numpy().view(np.uint32), cpu["zbuf"])


def test_render_multi_one_mesh_and_argument_checks(scene, dev, meshes, gmeshes):
    """a set of one mesh with obj NULL is the single-mesh render; a set of several refuses a missing object index"""
    from foundationpose_amd import _lib, ops
    from foundationpose_amd.Utils import get_mesh_handle
    h = get_mesh_handle(gmeshes["can"])
    one = ops.MeshSet([h])
    P = _t(_poses(scene, 6, seed=31), dev)
    tf, bb = ops.crop_windows(P, scene["K"], scene["diameter"], 1.2, (160, 160))
    a = ops.render_crops(one, P, bb, scene["K"], 480, 640, mesh_diameter=ops.object_diameters([scene["diameter"]], dev), want=ALL_OUT)
    b = ops.render_crops(h, P, bb, scene["K"], 480, 640, mesh_diameter=scene["diameter"], want=ALL_OUT)
    assert all(torch.equal(a[k], b[k]) for k in ALL_OUT)
    two, _, diam = _set(("can", "box"), meshes, gmeshes, dev)
    with pytest.raises(_lib.FpAmdError, match="object index"):
        ops.render_crops(two, P, bb, scene["K"], 480, 640, mesh_diameter=ops.object_diameters(diam, dev))
    lib = _lib.lib()
    assert lib.fp_render_crops(None, two.handle, None, None, 0.0, _devptr(P), _devptr(bb), None, None, None, 0, 480, 640, 6, 160, 160,
                               0.8, 0.5, 0.001, 0, None, None, None, None, None, None, None, None, 0, None) == -1
    assert b"obj is NULL but the set has 2 meshes" in lib.fp_last_error()


def _devptr(t):
    import ctypes as C
    return C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------ 2. crop windows, warp, pose update with per-object diameters
def test_per_object_diameters_are_the_scalar_calls(scene, dev, meshes, gmeshes, frame):
    from foundationpose_amd import ops
    names = ("can", "box", "torus", "small_can")
    diam = [_diameter(meshes[k]) for k in names]
    N = 64
    obj = _interleaved(4, N, seed=41)
    P = _t(_poses(scene, N, seed=42), dev)
    ot, dt = _t(obj, dev), ops.object_diameters(diam, dev)
    tf, bb = ops.crop_windows(P, scene["K"], dt, 1.2, (160, 160), obj=ot)
    rng = np.random.default_rng(43)
    trans = _t(rng.normal(0, 0.5, (N, 3)).astype(np.float32), dev)
    rot = _t(rng.normal(0, 0.5, (N, 3)).astype(np.float32), dev)
    B = {nz: ops.warp_crops(frame["rgb_t"], frame["xyz_t"], None, tf, scene["K"], P, dt, ops.MODE_REFINE, normalize_xyz=nz, obj=ot)
         for nz in (True, False)}
    Bs = ops.warp_crops(frame["rgb_t"], None, frame["depth_t"], tf, scene["K"], P, dt, ops.MODE_SCORE, obj=ot)
    upd = {}
    for rep in ("tracknet", "deepim"):
        td, rd = torch.empty((N, 3), device=dev), torch.empty((N, 3, 3), device=dev)
        upd[rep] = (ops.pose_update(trans, rot, P, normalize_xyz=True, trans_normalizer=(0.2, 0.2, 0.2), rot_normalizer=0.35,
                                    mesh_diameter=dt, trans_delta_out=td, rot_delta_out=rd, trans_rep=rep, K=scene["K"],
                                    tf_to_crops=tf, input_w=160, obj=ot), td, rd)
    for k in range(4):
        r = torch.as_tensor(np.nonzero(obj == k)[0], device=dev)
        Pk = P[r].contiguous()
        tfk, bbk = ops.crop_windows(Pk, scene["K"], diam[k], 1.2, (160, 160))
        assert torch.equal(tf[r], tfk) and torch.equal(bb[r], bbk), names[k]
        for nz in (True, False):
            ref = ops.warp_crops(frame["rgb_t"], frame["xyz_t"], None, tfk, scene["K"], Pk, diam[k], ops.MODE_REFINE, normalize_xyz=nz)
            assert torch.equal(B[nz][r], ref), (names[k], nz)
        ref = ops.warp_crops(frame["rgb_t"], None, frame["depth_t"], tfk, scene["K"], Pk, diam[k], ops.MODE_SCORE)
        assert torch.equal(Bs[r], ref), names[k]
        for rep in ("tracknet", "deepim"):
            td, rd = torch.empty((len(r), 3), device=dev), torch.empty((len(r), 3, 3), device=dev)
            o = ops.pose_update(trans[r].contiguous(), rot[r].contiguous(), Pk, normalize_xyz=True, trans_normalizer=(0.2, 0.2, 0.2),
                                rot_normalizer=0.35, mesh_diameter=diam[k], trans_delta_out=td, rot_delta_out=rd, trans_rep=rep,
                                K=scene["K"], tf_to_crops=tfk, input_w=160)
            assert torch.equal(upd[rep][0][r], o) and torch.equal(upd[rep][1][r], td) and torch.equal(upd[rep][2][r], rd), (names[k], rep)
    # the diameters matter: a different table moves the windows
    tf2, _ = ops.crop_windows(P, scene["K"], ops.object_diameters(diam[::-1], dev), 1.2, (160, 160), obj=ot)
    assert not torch.equal(tf, tf2)


# ------------------------------------------------------------------ 3. / 4. the refine loop against per-object calls
def _trained(dev, **kw):
    from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
    from foundationpose_amd.weights import DEFAULT_REFINE_CFG, trained_refiner_state_dict
    return PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), state_dict=trained_refiner_state_dict(), device=dev, precision="fp16",
                               graph=False, **kw)


def _multi_vs_single(pred, scene, frame, dev, meshes, gmeshes, names, obj, P, iteration=2, same_size=False):
    """-> (poses of one multi-object refine_device call, poses of per-object single-object calls).  same_size: every single-object
    call refines ALL of P with that object's mesh (the launch shapes of the multi-object call, rows kept in place) and contributes
    the rows of its object; otherwise it refines just its own rows"""
    from foundationpose_amd import ops
    from foundationpose_amd.predict_pose_refine import ObjectIndex
    mset, handles, diam = _set(names, meshes, gmeshes, dev)
    Pt = _t(P, dev)
    multi = pred.refine_device(frame["rgb_t"], frame["xyz_t"], Pt, scene["K"], 480, 640, mset, ops.object_diameters(diam, dev),
                               iteration, obj=ObjectIndex(obj, dev))[0]
    single = torch.empty_like(multi)
    for k in range(len(names)):
        r = torch.as_tensor(np.nonzero(np.asarray(obj) == k)[0], device=dev)
        if same_size:
            single[r] = pred.refine_device(frame["rgb_t"], frame["xyz_t"], Pt, scene["K"], 480, 640, handles[k], diam[k], iteration)[0][r]
        else:
            single[r] = pred.refine_device(frame["rgb_t"], frame["xyz_t"], Pt[r].contiguous(), scene["K"], 480, 640, handles[k], diam[k],
                                           iteration)[0]
    return multi, single


def _first_inputs(pred, scene, frame, dev, meshes, gmeshes, names, obj, P):
    """the network input (A rendered | B observed, fp16) of the first refine iteration: multi-object call against per-object calls
    -> (multi (2N, 6, h, w), per-object rows arranged like the multi-object call)"""
    from foundationpose_amd import ops
    from foundationpose_amd.crops import Scene
    from foundationpose_amd.predict_pose_refine import ObjectIndex
    mset, handles, diam = _set(names, meshes, gmeshes, dev)
    Pt, N = _t(P, dev), len(P)
    st = pred.refine_part(0, (0, N), frame["rgb_t"], frame["xyz_t"], Pt,
                          Scene(mset, ops.object_diameters(diam, dev), scene["K"], 480, 640, N, obj=ObjectIndex(obj, dev)),
                          range(1), pred.alloc_outputs(N, dev) + (1,))
    multi = st["AB"].clone()
    single = torch.empty_like(multi)
    for k in range(len(names)):
        rows = np.nonzero(np.asarray(obj) == k)[0]
        r = torch.as_tensor(rows, device=dev)
        n = len(rows)
        sk = pred.refine_part(0, (0, n), frame["rgb_t"], frame["xyz_t"], Pt[r].contiguous(), Scene(handles[k], diam[k], scene["K"], 480, 640, n),
                              range(1), pred.alloc_outputs(n, dev) + (1,))
        single[r], single[r + N] = sk["AB"][:n], sk["AB"][n:]
    return multi, single


def _close(a, b):
    """the gates of test_gpu_amp.py::test_track_one_small_call_path_vs_exact on the worst hypothesis: <= 1e-4 m, <= 3e-4 rad"""
    from amp_util import geodesic
    a, b = a.reshape(-1, 4, 4).cpu().numpy(), b.reshape(-1, 4, 4).cpu().numpy()
    dR = geodesic(a[:, :3, :3], b[:, :3, :3])
    dt = np.linalg.norm(a[:, :3, 3].astype(np.float64) - b[:, :3, 3].astype(np.float64), axis=1)
    return dt.max() <= 1e-4 and dR.max() <= 3e-4, (dt.max(), dR.max())


# What still depends on the size of a call under the large-call overrides: fp_igemm_f16_fwd picks the shifted-window kernel for a
# 3x3 convolution only from two tile rows on (conv_sw.hip, fp_conv3x3_sw_applicable: M >= 2 x 256 | 2 x 512 rows), so on the 20 x 20
# map of the joint blocks (M = N x 400) a ONE-hypothesis call runs the generic implicit GEMM and a call of two or more the shifted-window
# kernel: another summation order, last-place differences in the poses.  Every hypothesis is still independent of the others within
# one launch shape, so a multi-object call is bit-identical to single-object calls of the SAME size, and its first network input --
# rendering, crop windows, warp: everything per object -- to the single-object calls of any size; against one-hypothesis calls the
# poses are gated like the small-call path against the exactly-rounded chain.
def test_refine_loop_three_objects_is_three_calls_on_the_large_call_kernels(scene, dev, meshes, gmeshes, frame):
    """K = 3 objects x 1 hypothesis, 2 iterations, with the kernels of a large call (no split-K, one stream for the heads)"""
    from foundationpose_amd import engine
    names, obj = ("can", "torus", "box"), [1, 0, 2]
    with engine.overrides(SPLITK_MAX_HYPS=0, HEADS_TWO_STREAMS_MAX_HYPS=0):
        pred = _trained(dev)
        P = _poses(scene, 3, seed=51, max_rot_deg=20)
        multi, same = _multi_vs_single(pred, scene, frame, dev, meshes, gmeshes, names, obj, P, same_size=True)
        assert torch.equal(multi, same), (multi - same).abs().max()
        a, b = _first_inputs(pred, scene, frame, dev, meshes, gmeshes, names, obj, P)
        assert torch.equal(a, b)
        _, one = _multi_vs_single(pred, scene, frame, dev, meshes, gmeshes, names, obj, P)
        ok, err = _close(multi, one)
        assert ok, err
    assert not torch.equal(multi, _t(P, dev))


def test_two_objects_one_hypothesis_each_is_not_the_two_pose_quirk(scene, dev, meshes, gmeshes, frame):
    """two objects x one hypothesis = two single-object calls: the reference's two-pose quirk belongs to an object's own call, so it
    must not pair the two objects' windows (a whole-call `N == 2` check would: the rendered crops would differ); one object with two
    hypotheses keeps it"""
    from foundationpose_amd import engine
    with engine.overrides(SPLITK_MAX_HYPS=0, HEADS_TWO_STREAMS_MAX_HYPS=0):
        pred = _trained(dev)
        P = _poses(scene, 2, seed=61, max_rot_deg=20)
        P[1, :3, 3] += [0.02, -0.01, 0.03]          # different windows, so that the quirk would change the render
        a, b = _first_inputs(pred, scene, frame, dev, meshes, gmeshes, ("can", "torus"), [0, 1], P)
        assert torch.equal(a, b)
        multi, one = _multi_vs_single(pred, scene, frame, dev, meshes, gmeshes, ("can", "torus"), [0, 1], P)
        ok, err = _close(multi, one)
        assert ok, err
        # one object, two hypotheses through the multi-object path: the quirk applies, as in the single-object call (same size)
        m1, s1 = _multi_vs_single(pred, scene, frame, dev, meshes, gmeshes, ("can",), [0, 0], P)
        assert torch.equal(m1, s1)
        # objects with two hypotheses each, interleaved: per object its own two-pose call
        P4 = np.concatenate([P, _poses(scene, 2, seed=62, max_rot_deg=20)])
        P4[3, :3, 3] += [-0.02, 0.01, 0.02]
        a, b = _first_inputs(pred, scene, frame, dev, meshes, gmeshes, ("can", "torus"), [0, 1, 0, 1], P4)
        assert torch.equal(a, b)


def test_refine_loop_small_call_path_vs_exact(scene, dev, meshes, gmeshes, frame):
    """the default small-call path (split-K, two-stream heads) in a multi-object call: can hypotheses from the trained stand-in's
    golden chain, interleaved with hypotheses of other meshes, meet the gates of test_gpu_amp's single-object small-call test"""
    from amp_util import geodesic
    from foundationpose_amd import engine, ops
    from foundationpose_amd.predict_pose_refine import ObjectIndex
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "acc64_trained_chain_golden.npz")))
    pred = _trained(dev)
    names = ("can", "box", "torus")
    mset, handles, diam = _set(names, meshes, gmeshes, dev)
    dt = ops.object_diameters(diam, dev)
    ids = list(range(0, 252, 11))[:16]
    obj = [0, 1, 0, 2, 0, 0, 1, 0, 0, 2, 0, 0]     # 8 can hypotheses among 12: a small call
    assert len(obj) <= engine.SPLITK_MAX_HYPS and obj.count(0) == 8
    got = []
    for c in range(2):
        P = _poses(scene, len(obj), seed=70 + c, max_rot_deg=20)
        can_rows = [i for i, o in enumerate(obj) if o == 0]
        P[can_rows] = g["start"][ids[8 * c:8 * c + 8]]
        with ops.KernelTimers() as kt:
            out = pred.refine_device(frame["rgb_t"], frame["xyz_t"], _t(P, dev), scene["K"], 480, 640, mset, dt, 2,
                                     obj=ObjectIndex(obj, dev))[0]
        assert kt.summary().get("fp_igemm_f16_splitk_fwd", dict(calls=0))["calls"] >= 10      # the path under test did run
        got.append(out.cpu().numpy()[can_rows])
    got = np.concatenate(got)
    ref = g["chain"][2][ids]
    dR = geodesic(got[:, :3, :3], ref[:, :3, :3])
    dtr = np.linalg.norm(got[:, :3, 3].astype(np.float64) - ref[:, :3, 3].astype(np.float64), axis=1)
    assert dtr.max() <= 1e-4 and np.median(dR) <= 5e-5 and dR.max() <= 3e-4 and np.mean(dR <= 1e-4) >= 0.8, (dR, dtr)


# ------------------------------------------------------------------ 5. graph and pipeline
@pytest.mark.parametrize("n_hyp", [1, 2])
def test_multi_object_tracker_graph_and_pipeline(scene, dev, meshes, gmeshes, n_hyp):
    """GraphedTracker over three meshes (n_hyp each; 2 = the per-object two-pose quirk inside the graph): the replay is the eager
    loop bit for bit, and FramePipeline over it returns the bits of the unpipelined loop"""
    from foundationpose_amd.graphs import FramePipeline, GraphedTracker
    from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
    from foundationpose_amd.weights import CONTRACTION_HEAD_SCALE, DEFAULT_REFINE_CFG, random_state_dict
    refiner = PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), device=dev,
                                  state_dict=random_state_dict("refine", seed=0, head_scale=CONTRACTION_HEAD_SCALE))
    names = ("can", "torus", "box")
    trk = GraphedTracker(refiner, [gmeshes[k] for k in names], [_diameter(meshes[k]) for k in names], scene["K"], 480, 640,
                         n_hyp=n_hyp, iteration=2, device=dev).capture()
    assert trk.N == 3 * n_hyp and len(trk.obj.pairs) == (3 if n_hyp == 2 else 0)
    F = 4
    rng = np.random.default_rng(80)
    rgb_h = torch.empty((F, 480, 640, 3), dtype=torch.uint8).pin_memory()
    depth_h = torch.empty((F, 480, 640), dtype=torch.float32).pin_memory()
    hyp_h = torch.empty((F, trk.N, 4, 4), dtype=torch.float32).pin_memory()
    for f in range(F):
        rgb_h[f].copy_(torch.from_numpy(np.clip(scene["rgb"].astype(np.float32) + rng.normal(0, 4, scene["rgb"].shape), 0, 255).astype(np.uint8)))
        depth_h[f].copy_(torch.from_numpy((scene["depth"] + 0.0005 * f).astype(np.float32)))
        P = _poses(scene, trk.N, seed=81 + f, max_rot_deg=20)
        if n_hyp == 2:
            P[1::2, :3, 3] += [0.01, -0.01, 0.02]
        hyp_h[f].copy_(torch.from_numpy(P))
    eager = [trk.step_eager(rgb_h[f].to(dev).float(), depth_h[f], hyp_h[f]).clone() for f in range(F)]
    ref = [trk.step(rgb_h[f].to(dev).float(), depth_h[f], hyp_h[f]).clone() for f in range(F)]
    assert all(torch.equal(a, b) for a, b in zip(eager, ref))
    assert not torch.equal(ref[0], ref[1])
    pipe = FramePipeline(trk)
    trk._have_output = False
    got = []
    pipe.submit(0, rgb_h[0], depth_h[0], hyp_h[0])
    for f in range(F):
        if f + 1 < F:
            pipe.submit((f + 1) % 2, rgb_h[f + 1], depth_h[f + 1], hyp_h[f + 1])
        got.append(pipe.run(f % 2).clone())
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, ref))


# ------------------------------------------------------------------ 6. the estimator
def _three_object_frame(scene, meshes, names, poses):
    """z-composite of the oracle's full-frame renders of the objects at `poses`, with the scene's noise model"""
    from foundationpose_amd import synthetic as syn
    from oracle import ops as oo
    from oracle import pipeline as op
    color = np.zeros((scene["H"], scene["W"], 3), np.float32)
    depth = np.zeros((scene["H"], scene["W"]), np.float32)
    for k, name in enumerate(names):
        r = oo.render_crops(op.mesh_tensors_np(meshes[name]), poses[k][None].astype(np.float32), None, scene["K"], scene["H"],
                            scene["W"], (scene["H"], scene["W"]), normalize_xyz=False, want=("color", "depth"))
        d, c = r["depth"][0], r["color"][0]
        front = (d > 0) & ((depth == 0) | (d < depth))
        depth[front] = d[front]
        color[front] = c[front]
    rgb, dep, _ = syn.compose_frame(color, depth)
    return rgb, dep


def test_track_objects_is_per_object_track_one(scene, dev, meshes):
    """a frame of three objects (z-composited oracle renders), one FoundationPose per object sharing one refiner, started from known
    poses: track_objects on three frames tracks like per-object track_one under the large-call overrides; it refuses an
    unregistered estimator and estimators with different refiners"""
    from foundationpose_amd import engine
    from foundationpose_amd.estimater import FoundationPose, track_objects
    from foundationpose_amd.predict_pose_refine import PoseRefinePredictor
    from foundationpose_amd.predict_score import ScorePredictor
    from foundationpose_amd.weights import DEFAULT_REFINE_CFG, DEFAULT_SCORE_CFG, random_state_dict, trained_refiner_state_dict
    names = ("can", "torus", "box")
    gt = np.stack([scene["gt"].copy() for _ in names])
    for k, dx in enumerate((-0.09, 0.0, 0.09)):
        gt[k, 0, 3] += dx
        gt[k, 2, 3] += 0.03 * k
    gt[1, :3, :3] = _poses(scene, 1, seed=91, max_rot_deg=50)[0, :3, :3]
    gt[2, :3, :3] = _poses(scene, 1, seed=92, max_rot_deg=50)[0, :3, :3]
    frames, starts = [], []
    for f in range(3):
        P = gt.copy()
        P[:, 0, 3] += 0.002 * f
        frames.append(_three_object_frame(scene, meshes, names, P))
        S = P.copy()
        S[:, :3, 3] += [0.004, -0.003, 0.006]
        starts.append(S)
    with engine.overrides(SPLITK_MAX_HYPS=0, HEADS_TWO_STREAMS_MAX_HYPS=0):
        refiner = PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), state_dict=trained_refiner_state_dict(), device=dev)
        scorer = ScorePredictor(cfg=dict(DEFAULT_SCORE_CFG), state_dict=random_state_dict("score", seed=0), device=dev)
        ests = [FoundationPose(model_pts=meshes[k].vertices, model_normals=meshes[k].vertex_normals, mesh=meshes[k], scorer=scorer,
                               refiner=refiner, device=dev) for k in names]
        with pytest.raises(RuntimeError, match="not registered"):
            track_objects(ests, frames[0][0], frames[0][1], scene["K"])

        def reset(f):
            for e, P in zip(ests, starts[f]):       # the meshes are centred: pose_last = the pose
                assert np.allclose(e.model_center, 0, atol=1e-9)
                e.pose_last = torch.as_tensor(P, device=dev, dtype=torch.float).reshape(1, 4, 4)
        # every frame from the same start poses for both (last-place differences must not be amplified along a chain of frames);
        # the captured multi-object tracker is cached and replayed from the second frame on
        one, many = [], []
        for f, (rgb, depth) in enumerate(frames):
            reset(f)
            one.append(np.stack([e.track_one(rgb, depth, scene["K"], iteration=2) for e in ests]))
            last = [e.pose_last.clone() for e in ests]
            reset(f)
            many.append(np.stack(track_objects(ests, rgb, depth, scene["K"], iteration=2)))
        assert refiner._objects_tracker[1].N == 3
        # one batched call of three hypotheses against three one-hypothesis calls: the kernel choice above (the comment before
        # test_refine_loop_three_objects...), so the poses are gated
        for f in range(len(frames)):
            ok, err = _close(torch.as_tensor(many[f]), torch.as_tensor(one[f]))
            assert ok, (f, err)
        for e, p, m in zip(ests, last, many[-1]):
            assert e.pose_last.shape == (1, 4, 4) and _close(e.pose_last, p)[0]
            assert torch.equal((e.pose_last[0] @ e.get_tf_to_centered_mesh()).cpu(), torch.as_tensor(m))
        # the stand-in refiner was trained on the can: that object is tracked (the others only have to be what track_one gives)
        assert np.abs(many[-1][0, :3, 3] - gt[0, :3, 3]).max() < 0.01
        other = PoseRefinePredictor(cfg=dict(DEFAULT_REFINE_CFG), state_dict=trained_refiner_state_dict(), device=dev)
        stranger = FoundationPose(model_pts=meshes["box"].vertices, model_normals=meshes["box"].vertex_normals, mesh=meshes["box"],
                                  scorer=scorer, refiner=other, device=dev)
        stranger.pose_last = ests[2].pose_last.clone()
        with pytest.raises(ValueError, match="share one refiner"):
            track_objects(ests[:2] + [stranger], frames[0][0], frames[0][1], scene["K"])
