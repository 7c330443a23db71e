"""Measures the device tanhf / sinf / cosf against float64 with ./probe (make -C scripts/libm_ulp_probe first) and writes the record
tests/pose_update_model.py's L_DEVICE points to:

    python scripts/libm_ulp_probe/measure.py profiles/libm_ulp_gfx950.json

Arguments: exactly those the generated cases of tests/pose_update_cases.py feed the three functions (tanh: the raw rotation and
translation outputs; sin / cos: the rotation angle th, formed by the float32 restatement), plus a dense sweep of their ranges --
tanh over +-22 (linear) and +-[1e-8, 22] (logarithmic), sin / cos over [0.0099, 3.2], which holds the clamp 0.01 and pi, with every
float32 within 4096 steps of 0.01 and of pi.  The error of a result r~ against the float64 value r is |r~ - r| / ulp(r), ulp = the
float32 spacing at |r| -- the unit tests/pose_update_model.py multiplies L_f with."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
F = np.float32


def case_arguments():
    import conftest
    import pose_update_cases as pc
    import pose_update_model as pm
    ta, th = [], []
    for c in pc.cases(conftest._build_scene()):
        a, b = pm.rotation_angle_args(c["trans"], c["rot"], c["rot_normalizer"], c["normalize_xyz"], c["trans_rep"], c["rot_rep"])
        ta.append(a)
        th.append(b)
    return np.concatenate(ta), np.concatenate(th)


def around(x, steps=4096):
    b = np.int64(F(x).view(np.uint32)) + np.arange(-steps, steps + 1)
    return b.astype(np.uint32).view(F)


def sweeps():
    log = (10.0 ** np.linspace(-8, np.log10(22.0), 150000)).astype(F)
    tanh = np.concatenate([np.linspace(-22, 22, 300001).astype(F), log, -log, np.array([0.0, -0.0, np.inf, -np.inf], F)])
    sincos = np.concatenate([np.linspace(0.0099, 3.2, 400001).astype(F), around(0.01), around(np.pi), around(np.pi / 2)])
    return tanh, sincos


def run_probe(args):
    with tempfile.NamedTemporaryFile(suffix=".f32") as f:
        np.ascontiguousarray(args, F).tofile(f.name)
        txt = subprocess.run([os.path.join(HERE, "probe"), f.name], check=True, capture_output=True, timeout=240).stdout
    b = np.array([int(t, 16) for t in txt.split()], np.uint32).reshape(-1, 4)
    assert np.array_equal(b[:, 0], np.ascontiguousarray(args, F).view(np.uint32))
    return b[:, 1].view(F), b[:, 2].view(F), b[:, 3].view(F)


def ulp_error(got, x, f):
    r = f(x.astype(np.float64))
    err = np.abs(got.astype(np.float64) - r) / np.spacing(np.abs(r).astype(F)).astype(np.float64)
    k = int(np.argmax(err))
    return dict(max_ulp=float(err[k]), at_arg=float(x[k]), at_arg_bits="%08x" % int(x[k].view(np.uint32)), mean_ulp=float(err.mean()),
                not_correctly_rounded=float((got != r.astype(F)).mean()), arguments=int(len(x)))


def main(out_path):
    ta, th = case_arguments()
    st, ss = sweeps()
    rec = dict(what="device tanhf / sinf / cosf against float64, in ulp of the float32 result", arch="gfx950",
               flags="those of SRCS_EXACT (scripts/libm_ulp_probe/Makefile)")
    for name, args in (("cases", (ta, th)), ("sweep", (st, ss))):
        t, _, _ = run_probe(args[0])
        _, s, c = run_probe(args[1])
        rec[name] = dict(tanhf=ulp_error(t, args[0], np.tanh), sinf=ulp_error(s, args[1], np.sin), cosf=ulp_error(c, args[1], np.cos))
    rec["max_ulp"] = {f: max(rec["cases"][f]["max_ulp"], rec["sweep"][f]["max_ulp"]) for f in ("tanhf", "sinf", "cosf")}
    rec["max_ulp_all"] = max(rec["max_ulp"].values())
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec["max_ulp"]), rec["max_ulp_all"])


if __name__ == "__main__":
    main(sys.argv[1])
