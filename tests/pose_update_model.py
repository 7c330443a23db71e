"""fp_pose_update (k_pose_update of csrc/frame_ops.hip, fpo_pose_update of oracle/fp_oracle.c) in plain numpy: no GPU, no import of
the product.  Three things, one algorithm text (pose_update below) run over two kinds of number:

1. THE FLOAT64 DEFINITION of predict_pose_refine.py:195-234 as the reference states it -- pytorch3d's so3_exp_map with eps = 1e-4
   clamping the SQUARED norm, rotation_6d_to_matrix with F.normalize's eps = 1e-12, the transpose, the translation representations
   'tracknet', 'raw' and 'deepim', and the three outputs (pose, trans_delta, rot_delta).  The 'deepim' value of the definition is
   computed with general 3x3 inverses of K and tf_to_crops (deepim_delta_general); the algorithm text uses the closed forms of the
   kernel, which are the same function for an upper-triangular K and an axis-aligned window.

2. A FLOAT32 RESTATEMENT of the kernel's expression order (Single): every operation rounded to float32 in the order of
   k_pose_update / fpo_pose_update; tanh, sin and cos evaluated in float64 and rounded once.  Where no libm call enters (the 6d
   rotation, 'raw' and normalised 'tracknet' translations, the 'deepim' delta) the kernel has to reproduce it bit for bit.

3. A RUNNING ERROR BOUND per output element (Bounded), carried alongside the float64 value.  x~ denotes what a float32 evaluation
   holds for the exact x, e_x >= |x~ - x|, u = 2^-24 (round to nearest), t = 2^-150 (half the smallest subnormal: the rounding error
   of a result below the normal range is absolute, not relative).  For z = fl(x~ op y~):
     |z~ - z| <= |x~ op y~ - x op y| + u |x~ op y~| + t  <=  p (1 + u) + u |z| + t      with p the propagated part:
       +, -   : p = e_x + e_y
       *      : p = |x| e_y + |y| e_x + e_x e_y
       /      : p = (e_x + |x / y| e_y) / (|y| - e_y)                 (infinite when |y| <= e_y: the quotient is not determined)
       sqrt   : p = sqrt(x) - sqrt(max(x - e_x, 0))                    (concave: the downward deviation is the larger one)
       fmax(x, c): p = e_x, no rounding                                (1-Lipschitz, exact); x / 2: p = e_x / 2, no rounding
       f in {tanh, sin, cos}: |f~(x~) - f(x)| <= e_x sup|f'| + L_f ulp(f(x))   with the supremum over [x - e_x, x + e_x]:
           tanh' <= 1,  |sin'| <= min(1, |cos x| + e_x),  |cos'| <= min(1, |sin x| + e_x);  ulp = the float32 spacing at |f(x)|.
   Nothing is waved away: 1 - cos(th) is an ordinary subtraction whose operand carries L_f ulp(cos th) ~ L_f 2^-24, so at the
   clamped th = 0.01 the difference 5e-5 is known to about L_f 1e-3 of itself, and that is what the bound says of fac2.  The
   bound is first order in nothing: every line above is an inequality.  It is never tuned to the kernel: L_f is its one parameter.

L_f: the accuracy of the libm that evaluates tanhf / sinf / cosf, in ulp of the result.  Host: glibc documents 1 ulp for the three
(L_HOST).  Device: measured, not documented -- scripts/libm_ulp_probe evaluates the device functions on exactly the arguments the
cases of tests/pose_update_cases.py feed them plus a dense sweep of their ranges, and compares with float64;
profiles/libm_ulp_gfx950.json holds the measured maxima.  L_DEVICE = the largest measured maximum plus 1 ulp, because a sweep is a
sample.

`variant` names one deliberately wrong reading of the definition (VARIANTS): tests/test_pose_update_cases_host.py shows that the
generated cases tell each of them from the right one by more than the bound.  Test infrastructure only."""
import numpy as np

F = np.float32
U_RND = 2.0 ** -24
TINY = 2.0 ** -150
F64_SLACK = 2.0 ** -20        # the float64 evaluation of the definition itself: the same operations with u = 2^-53 = 2^-29 * 2^-24,
#                               times 512 for the different operation order of a general inverse; relative to the float32 bound
L_HOST = 1.0                  # glibc: tanhf, sinf, cosf within 1 ulp (libm's documented "Errors in Math Functions")
L_DEVICE = 2.54               # profiles/libm_ulp_gfx950.json: measured maxima tanhf 1.41, sinf 1.34, cosf 1.54 ulp; the largest + 1 ulp
VARIANTS = ("clamp_on_norm", "eps_1e-6", "no_transpose", "normalizer_inside_tanh", "b3_is_b2_x_b1", "full_diameter",
            "tanh_under_normalize_xyz", "deepim_ignores_skew", "deepim_uses_input_h")
ROT_SCALE = 1.0               # the scale of an element of a rotation block: rows and columns of a rotation have norm 1
T_FLOOR = 2.0 ** -126         # the smallest normal float32: below it a relative precision is not defined


# ------------------------------------------------------------------------------------------------------------ numbers
class Single:
    """float32 arrays; every operator is numpy's correctly rounded float32 operation (no contraction between ufunc calls)"""

    @staticmethod
    def const(x):
        return np.asarray(x, F)

    @staticmethod
    def zeros(n):
        return np.zeros(n, F)

    @staticmethod
    def sqrt(x):
        return np.sqrt(x, dtype=F)

    @staticmethod
    def fmax(x, c):
        return np.fmax(x, F(c))            # C's fmaxf: the other operand when one is NaN

    @staticmethod
    def halve(x):
        return x / F(2.0)

    @staticmethod
    def _once(f, x):
        return f(np.asarray(x, np.float64)).astype(F)

    def tanh(self, x):
        return self._once(np.tanh, x)

    def sin(self, x):
        return self._once(np.sin, x)

    def cos(self, x):
        return self._once(np.cos, x)

    @staticmethod
    def value(x):
        return np.asarray(x, F)


class BV:
    """exact value v (float64) and a bound e on |float32 evaluation - v|"""
    __slots__ = ("v", "e")
    __array_priority__ = 100

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, BV) else BV(np.asarray(x, np.float64))

    @staticmethod
    def _rnd(v, p):
        return BV(v, p * (1 + U_RND) + U_RND * np.abs(v) + TINY)

    def __neg__(self):
        return BV(-self.v, self.e)

    def __add__(self, o):
        o = BV.of(o)
        return BV._rnd(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = BV.of(o)
        return BV._rnd(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return BV.of(o) - self

    def __mul__(self, o):
        o = BV.of(o)
        return BV._rnd(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = BV.of(o)
        q = self.v / o.v
        den = np.abs(o.v) - o.e
        p = np.where(den > 0, (self.e + np.abs(q) * o.e) / np.where(den > 0, den, 1.0), np.inf)
        return BV._rnd(q, p)

    def __rtruediv__(self, o):
        return BV.of(o) / self


class Bounded:
    def __init__(self, L_f):
        self.L = float(L_f)

    @staticmethod
    def const(x):
        return BV(np.asarray(x, F).astype(np.float64))

    @staticmethod
    def zeros(n):
        return BV(np.zeros(n))

    @staticmethod
    def sqrt(x):
        r = np.sqrt(x.v)
        return BV._rnd(r, r - np.sqrt(np.maximum(x.v - x.e, 0.0)))

    @staticmethod
    def fmax(x, c):
        return BV(np.maximum(x.v, np.float64(F(c))), x.e)      # torch.clamp: a NaN stays a NaN

    @staticmethod
    def halve(x):
        return BV(x.v / 2.0, x.e / 2.0 + TINY)                  # exact unless the result is subnormal

    def _libm(self, f, x, slope):
        r = f(x.v)
        return BV(r, x.e * slope + self.L * np.spacing(np.abs(r).astype(F)).astype(np.float64) + TINY)

    def tanh(self, x):
        return self._libm(np.tanh, x, 1.0)

    def sin(self, x):
        return self._libm(np.sin, x, np.minimum(1.0, np.abs(np.cos(x.v)) + x.e))

    def cos(self, x):
        return self._libm(np.cos, x, np.minimum(1.0, np.abs(np.sin(x.v)) + x.e))

    @staticmethod
    def value(x):
        return BV.of(x)


# ---------------------------------------------------------------------------------------------------------- the update
def pose_update(num, trans, rot, poses, rot_rep="axis_angle", normalize_xyz=True, trans_normalizer=(1.0, 1.0, 1.0), rot_normalizer=1.0,
                diameter=1.0, trans_rep="tracknet", K=None, tf=None, input_w=0.0, input_h=None, variant=None):
    """The expression order of k_pose_update over the numbers of `num` (Single() or Bounded(L_f)).  trans (N,3), rot (N,3|6),
    poses (N,4,4), diameter a scalar or (N,), K (3,3) or (N,3,3), tf (N,3,3): float32 values.  -> (pose [16 numbers], trans_delta
    [3], rot_delta [9]), every number an (N,) array of `num`'s kind."""
    assert variant is None or variant in VARIANTS, variant
    c = num.const
    trans, rot = np.asarray(trans, F), np.asarray(rot, F)
    A = np.asarray(poses, F).reshape(-1, 16)
    N = len(A)
    tr = [c(trans[:, k]) for k in range(3)]
    half = c(np.broadcast_to(np.asarray(diameter, np.float64).astype(F), (N,)))
    if variant != "full_diameter":
        half = num.halve(half)
    tn = np.asarray(trans_normalizer, F)
    with np.errstate(all="ignore"):
        if trans_rep == "deepim":
            K9 = np.broadcast_to(np.asarray(K, np.float64).astype(F).reshape(-1, 9), (N, 9))
            T9 = np.asarray(tf, F).reshape(N, 9)
            Kv, tfv = [c(K9[:, k]) for k in range(9)], [c(T9[:, k]) for k in range(9)]
            if variant == "deepim_ignores_skew":
                Kv[1] = num.zeros(N)
            tx, ty, tz = c(A[:, 3]), c(A[:, 7]), c(A[:, 11])
            u = ((Kv[0] * tx + Kv[1] * ty) + Kv[2] * tz) / tz
            v = (Kv[4] * ty + Kv[5] * tz) / tz
            uc = (tfv[0] * u + tfv[1] * v) + tfv[2]
            vc = (tfv[3] * u + tfv[4] * v) + tfv[5]
            z_pred = tr[2] * tz
            iw = c(F(input_w))
            ucp = uc + tr[0] * iw
            vcp = vc + tr[1] * (c(F(input_h)) if variant == "deepim_uses_input_h" else iw)
            vp = (vcp - tfv[5]) / tfv[4]
            up = ((ucp - tfv[2]) - tfv[1] * vp) / tfv[0]
            yn = (vp - Kv[5]) / Kv[4]
            xn = ((up - Kv[2]) - Kv[1] * yn) / Kv[0]
            dt = [xn * z_pred - tx, yn * z_pred - ty, z_pred - tz]
            if normalize_xyz:
                dt = [d * half for d in dt]
        else:
            dt = []
            for k in range(3):
                if not normalize_xyz:
                    dt.append(tr[k] if trans_rep != "tracknet" else num.tanh(tr[k]) * c(tn[k]))
                elif variant == "tanh_under_normalize_xyz" and trans_rep == "tracknet":
                    dt.append(num.tanh(tr[k]) * half)
                else:
                    dt.append(tr[k] * half)
        if rot_rep == "axis_angle":
            rn = c(F(rot_normalizer))
            if variant == "normalizer_inside_tanh":
                w = [num.tanh(c(rot[:, k]) * rn) for k in range(3)]
            else:
                w = [num.tanh(c(rot[:, k])) * rn for k in range(3)]
            n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
            if variant == "clamp_on_norm":
                th = num.fmax(num.sqrt(n2), 1e-4)
            else:
                th = num.sqrt(num.fmax(n2, 1e-6 if variant == "eps_1e-6" else 1e-4))
            ith = c(F(1.0)) / th
            f1 = ith * num.sin(th)
            f2 = (ith * ith) * (c(F(1.0)) - num.cos(th))
            z = num.zeros(N)
            Kx = [z, -w[2], w[1], w[2], z, -w[0], -w[1], w[0], z]
            R = []
            for r in range(3):
                for cc in range(3):
                    k2 = (Kx[r * 3] * Kx[cc] + Kx[r * 3 + 1] * Kx[3 + cc]) + Kx[r * 3 + 2] * Kx[6 + cc]
                    R.append((f1 * Kx[r * 3 + cc] + f2 * k2) + c(F(1.0 if r == cc else 0.0)))
        else:
            a1, a2 = [c(rot[:, k]) for k in range(3)], [c(rot[:, 3 + k]) for k in range(3)]
            l1 = num.fmax(num.sqrt((a1[0] * a1[0] + a1[1] * a1[1]) + a1[2] * a1[2]), 1e-12)
            b1 = [a / l1 for a in a1]
            dp = (b1[0] * a2[0] + b1[1] * a2[1]) + b1[2] * a2[2]
            u2 = [a2[k] - dp * b1[k] for k in range(3)]
            l2 = num.fmax(num.sqrt((u2[0] * u2[0] + u2[1] * u2[1]) + u2[2] * u2[2]), 1e-12)
            b2 = [x / l2 for x in u2]
            p, q = (b2, b1) if variant == "b3_is_b2_x_b1" else (b1, b2)
            b3 = [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]
            R = b1 + b2 + b3
        if variant == "no_transpose":
            R = [R[cc * 3 + r] for r in range(3) for cc in range(3)]
        Ac = [c(A[:, k]) for k in range(16)]
        out = [None] * 16
        for r in range(3):
            for cc in range(3):
                out[r * 4 + cc] = (R[0 * 3 + r] * Ac[0 * 4 + cc] + R[1 * 3 + r] * Ac[1 * 4 + cc]) + R[2 * 3 + r] * Ac[2 * 4 + cc]
            out[r * 4 + 3] = Ac[r * 4 + 3] + dt[r]
        for k, x in zip(range(12, 16), (0.0, 0.0, 0.0, 1.0)):
            out[k] = c(np.full(N, x, F))
        dR = [R[cc * 3 + r] for r in range(3) for cc in range(3)]
    return [num.value(x) for x in out], [num.value(x) for x in dt], [num.value(x) for x in dR]


def rotation_angle_args(trans, rot, rot_normalizer, normalize_xyz, trans_rep, rot_rep):
    """the float32 arguments the update feeds tanh and sin / cos (the latter through the restatement) -> (tanh args, th args)"""
    tanh_args, th_args = [], []
    if trans_rep == "tracknet" and not normalize_xyz:
        tanh_args.append(np.asarray(trans, F).reshape(-1))
    if rot_rep == "axis_angle":
        rot = np.asarray(rot, F)
        tanh_args.append(rot.reshape(-1))
        s = Single()
        with np.errstate(all="ignore"):
            w = [s.tanh(rot[:, k]) * F(rot_normalizer) for k in range(3)]
            th_args.append(np.sqrt(np.fmax((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], F(1e-4)), dtype=F))
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, F)
    return cat(tanh_args), cat(th_args)


def restatement(trans, rot, poses, **kw):
    """the float32 restatement -> (pose (N,4,4), trans_delta (N,3), rot_delta (N,3,3)) float32"""
    o, dt, dR = pose_update(Single(), trans, rot, poses, **kw)
    N = len(np.asarray(poses).reshape(-1, 16))
    return np.stack(o, 1).reshape(N, 4, 4), np.stack(dt, 1).reshape(N, 3), np.stack(dR, 1).reshape(N, 3, 3)


def deepim_delta_general(trans, poses, K, tf, input_w, normalize_xyz, diameter, input_h=None, variant=None):
    """predict_pose_refine.py:201-215 in float64 with general 3x3 inverses of K and of every tf_to_crops (no structure assumed)"""
    tr = np.asarray(trans, F).astype(np.float64)
    P = np.asarray(poses, F).astype(np.float64).reshape(-1, 4, 4)
    N = len(P)
    t = P[:, :3, 3]
    Kd = np.broadcast_to(np.asarray(K, np.float64).astype(F).astype(np.float64).reshape(-1, 3, 3), (N, 3, 3)).copy()
    if variant == "deepim_ignores_skew":
        Kd[:, 0, 1] = 0.0
    tfd = np.asarray(tf, F).astype(np.float64).reshape(N, 3, 3)
    out = np.full((N, 3), np.nan)
    with np.errstate(all="ignore"):
        for n in range(N):
            uv = Kd[n] @ t[n]
            uv = uv / uv[2]
            uvc = (tfd[n] @ uv)[:2]
            zp = tr[n, 2] * t[n, 2]
            step = np.array([input_w, input_h if variant == "deepim_uses_input_h" else input_w], np.float64)
            uvp = uvc + tr[n, :2] * step
            if not (np.isfinite(tfd[n]).all() and np.isfinite(uvp).all() and abs(np.linalg.det(tfd[n])) > 0):
                continue
            tfi = np.linalg.inv(tfd[n])
            uvq = tfi[:2, :2] @ uvp + tfi[:2, 2]
            cp = np.linalg.inv(Kd[n]) @ np.array([uvq[0], uvq[1], 1.0]) * zp
            out[n] = cp - t[n]
    if normalize_xyz:
        d = np.broadcast_to(np.asarray(diameter, np.float64).astype(F).astype(np.float64), (N,))
        out = out * (d / (1.0 if variant == "full_diameter" else 2.0))[:, None]
    return out


def definition(trans, rot, poses, L_f=L_HOST, **kw):
    """the float64 definition and its bound -> dict(pose, pose_e (N,4,4), dt, dt_e (N,3), dR, dR_e (N,3,3), dt_closed (N,3):
    the float64 closed form of the 'deepim' delta, equal to dt for the other representations)"""
    o, dt, dR = pose_update(Bounded(L_f), trans, rot, poses, **kw)
    N = len(np.asarray(poses).reshape(-1, 16))
    st = lambda xs, f, shape: np.stack([getattr(x, f) for x in xs], 1).reshape(shape)
    d = dict(pose=st(o, "v", (N, 4, 4)), pose_e=st(o, "e", (N, 4, 4)), dt=st(dt, "v", (N, 3)), dt_e=st(dt, "e", (N, 3)),
             dR=st(dR, "v", (N, 3, 3)), dR_e=st(dR, "e", (N, 3, 3)))
    d["dt_closed"] = d["dt"].copy()
    if kw.get("trans_rep") == "deepim":
        g = deepim_delta_general(trans, poses, kw["K"], kw["tf"], kw["input_w"], kw.get("normalize_xyz", True), kw.get("diameter", 1.0),
                                 kw.get("input_h"), kw.get("variant"))
        d["dt"] = g
        d["pose"][:, :3, 3] = np.asarray(poses, F).astype(np.float64).reshape(N, 4, 4)[:, :3, 3] + g
        d["dt_e"] = d["dt_e"] * (1 + F64_SLACK)
        d["pose_e"][:, :3, 3] = d["pose_e"][:, :3, 3] * (1 + F64_SLACK)
    return d


def scales(defn, poses):
    """the scale of every output element, for the one question of which rows the bound says nothing about: 1 for the elements of a
    rotation block; for a translation element max(|t_in|, |delta|, the smallest normal float32)"""
    P = np.asarray(poses, F).astype(np.float64).reshape(-1, 4, 4)
    with np.errstate(invalid="ignore"):
        ts = np.fmax(np.fmax(np.abs(P[:, :3, 3]), np.abs(defn["dt"])), T_FLOOR)
    ps = np.full(defn["pose"].shape, ROT_SCALE)
    ps[:, :3, 3] = ts
    return dict(pose=ps, dt=ts, dR=np.full(defn["dR"].shape, ROT_SCALE))


def undetermined_rows(defn, poses, rel=1e-3):
    """the rows on which the bound itself exceeds `rel` of an element's scale (or is not finite): the float32 result is not
    determined there, and the comparison with the bound leaves them out"""
    s = scales(defn, poses)
    bad = np.zeros(len(defn["pose"]), bool)
    for k in ("pose", "dt", "dR"):
        flat = lambda a: a.reshape(len(bad), int(np.prod(a.shape[1:])))
        e = flat(defn[k + "_e"])
        with np.errstate(invalid="ignore"):
            bad |= (~np.isfinite(e) | ~np.isfinite(flat(defn[k])) | (e > rel * flat(s[k]))).any(axis=1)
    return bad


def excess(out, defn, key):
    """|out - definition| / bound per element (0 where both are exactly equal), the figure that must stay <= 1"""
    o = np.asarray(out, np.float64).reshape(defn[key].shape)
    with np.errstate(all="ignore"):
        d = np.abs(o - defn[key])
        r = d / defn[key + "_e"]
    return np.where(d == 0, 0.0, r)
