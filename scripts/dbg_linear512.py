"""phase timers of k_linear512 and k_linear512_direct (csrc/linear_ln.hip, profiling build): the share of a workgroup's life that wave 0
spends inside store_block, per column block, at the bench's in_proj shapes (M = 126 x 400 per sub-batch, N = 3072 and 1536); 100 MHz wall clock
    FP_AMD_LIB=foundationpose_amd/csrc/libfp_amd_profile.so python scripts/dbg_linear512.py [M ...]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from foundationpose_amd import ops

dev = torch.device("cuda:0")
L = C.CDLL(os.environ["FP_AMD_LIB"])
g = torch.Generator(device="cpu").manual_seed(4)
r = lambda *s, k=1.0: (torch.randn(s, generator=g) * k).to(dev)


def timed(f, reps=30):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for M in [int(a) for a in sys.argv[1:]] or [50400]:
    x = r(M, 512).half()
    for N in (3072, 1536):
        w, b = r(N, 512, k=0.05).half(), r(N, k=0.1)
        y = torch.empty((M, N), dtype=torch.float16, device=dev)
        for name, direct in (("k_linear512 (LDS transposition)", False), ("k_linear512_direct", True)):
            p = ops.PackedLinear512(w, direct=direct)
            f = lambda: ops.linear512(x, p, b, out=y, direct_store=direct)
            us = timed(f)
            out = (C.c_ulonglong * 4)()
            L.fp_dbg_linear512(out, 1)
            f(); torch.cuda.synchronize()
            L.fp_dbg_linear512(out, 0)
            st, life, wgs, blocks = (int(v) for v in out)
            print(f"M={M} N={N} {name}: {us:.1f} us per launch; {wgs} workgroups; per workgroup: life {life / wgs * 10 / 1e3:.2f} us, "
                  f"store_block {st / wgs * 10 / 1e3:.2f} us = {100.0 * st / life:.1f} % of it, {st / blocks * 10 / 1e3:.2f} us per column block", flush=True)
