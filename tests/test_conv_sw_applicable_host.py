"""CPU: the launcher predicate of the shifted-window 3x3 convolution, fp_conv3x3_sw_applicable (csrc/conv_sw.hip), and the divisions its
kernels run on what it lets through.

k_conv_sw divides by Wo and by HoWo as umulhi(n, mul) >> shr WITHOUT the divisor-1 case of ig_fastdiv (mul == 0 encodes a divisor of 1,
csrc/igemm_common.h): the predicate has to refuse every geometry with such a divisor, and for the geometries it accepts the form has to
return n / d for every n the kernel can feed it (rows below M, pixels below HoWo).

The predicate is host code of the library but not part of its C ABI, so a small host program -- compiled here against the library's own
headers, host side only, and linked to the built library -- builds the parameter block as igemm.hip does and prints what the predicate
says."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "foundationpose_amd", "csrc")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "igemm_common.h"
bool fp_conv3x3_sw_applicable(const IgemmParams& p);
static IgemmGeom geom(int H, int W, int pad, int C) {   // ig_geom of igemm.hip on IgemmGeom.image(H, W, pad, C, stride 1)
  IgemmGeom o;
  memset(&o, 0, sizeof(o));
  o.HoWo = H * W; o.Wo = W; o.Hp = H + 2 * pad; o.Wp = W + 2 * pad; o.stride = 1; o.off = pad; o.cstride = C;
  ig_fastdiv_init(o.HoWo, &o.mulP, &o.shrP);
  ig_fastdiv_init(o.Wo, &o.mulW, &o.shrW);
  ig_fastdiv_init(o.bsplit, &o.mulB, &o.shrB);
  return o;
}
static unsigned div_kernel(unsigned n, unsigned mul, unsigned shr) { return (unsigned)(((unsigned long long)n * mul) >> 32) >> shr; }
int main(int argc, char** argv) {
  for (int a = 1; a + 3 < argc; a += 4) {
    const int B = atoi(argv[a]), H = atoi(argv[a + 1]), W = atoi(argv[a + 2]), C = atoi(argv[a + 3]);
    IgemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = (const _Float16*)16; p.Wt = (const _Float16*)16; p.Y = (_Float16*)16; p.R = (const _Float16*)16;
    p.M = B * H * W; p.N = C; p.Cin = C; p.taps = 9; p.mfma16 = 1;
    p.in = geom(H, W, 1, C); p.in.off = 0;               // the conv input: tap (0,0)
    p.out = geom(H, W, 1, C); p.res = geom(H, W, 1, C);
    const bool ok = fp_conv3x3_sw_applicable(p);
    long long bad = 0;
    if (ok) {
      for (int n = 0; n <= p.M; ++n) bad += div_kernel(n, p.in.mulP, p.in.shrP) != (unsigned)(n / p.in.HoWo);
      for (int n = 0; n < p.in.HoWo; ++n) bad += div_kernel(n, p.in.mulW, p.in.shrW) != (unsigned)(n / p.in.Wo);
    }
    printf("%d %d %d %d applicable=%d mulP=%u mulW=%u wrong_quotients=%lld\n", B, H, W, C, (int)ok, p.in.mulP, p.in.mulW, bad);
  }
  return 0;
}
"""

# (images, height, width, channels)
#   served: the product's shapes, this suite's, and one whose divisors are powers of two (32, 1024: mul = 2^31): every quotient right
#   width 1: a divisor of 1 (Wo), with HoWo > 1 and with HoWo == 1 (both divisors 1): refused
SERVED = [(252, 40, 40, 128), (126, 20, 20, 512), (4, 40, 40, 128), (6, 20, 20, 512), (8, 32, 32, 128)]
REFUSED = [(2048, 1, 1, 128), (64, 40, 1, 128), (4096, 2, 1, 256)]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "the test compiles a host program with the ROCm compiler"
    from foundationpose_amd import _lib
    libdir, libname = os.path.split(_lib.LIB_PATH)
    assert os.path.exists(_lib.LIB_PATH), "build the library first"
    d = tmp_path_factory.mktemp("sw_applicable")
    src, exe = os.path.join(d, "applicable.cpp"), os.path.join(d, "applicable")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-I", CSRC, "-I", os.path.join(ROOT, "include"), src,
                    "-o", exe, "-L", libdir, "-l:" + libname, "-Wl,-rpath," + libdir], check=True, capture_output=True, text=True)
    args = [str(v) for case in SERVED + REFUSED for v in case]
    out = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
    print(out)
    res = {}
    for line in out.splitlines():
        f = line.split()
        res[tuple(int(v) for v in f[:4])] = dict(kv.split("=") for kv in f[4:])
    assert len(res) == len(SERVED) + len(REFUSED)
    return res


@pytest.mark.parametrize("case", SERVED)
def test_served_geometries_divide_exactly(verdicts, case):
    v = verdicts[case]
    assert v["applicable"] == "1", (case, v)
    assert int(v["mulP"]) != 0 and int(v["mulW"]) != 0, (case, v)      # no divisor of 1 reaches the kernel
    assert v["wrong_quotients"] == "0", (case, v)


@pytest.mark.parametrize("case", REFUSED)
def test_a_divisor_of_one_is_refused(verdicts, case):
    v = verdicts[case]
    assert int(v["mulW"]) == 0, (case, v)                               # the case in question: ig_fastdiv_init's encoding of a divisor of 1
    assert v["applicable"] == "0", (case, v)
