"""CPU: what k_linear512_direct (csrc/linear_ln.hip), the in_proj kernel that stores its tiles from the accumulators, takes of a CU, read
from the kernel metadata of the built library's gfx950 code objects the way tests/test_conv_sw_resources_host.py reads it, next to the
kernel it takes the launches of.  Resource numbers only; no instruction is looked at.

Both kernels fill the CU they run on -- one workgroup of eight waves, two per SIMD, with up to 256 registers each -- so a register more
than the earlier kernel would not compile into the launch bounds, and a byte of scratch or a spilled register would put memory traffic
into the loops that the removed LDS round trips do not pay for.  (A direct-store patch-embed kernel was built in the same round, measured
no gain and is not part of the library: DESIGN.md section 3.)"""
from test_conv_sw_resources_host import _kernel_metadata

NEW, OLD = "k_linear512_direct(", "k_linear512("


def _one(meta, key):
    hits = [(k, v) for k, v in meta.items() if key in k]
    assert len(hits) == 1, (key, [k for k, _ in hits])
    return hits[0]


def test_direct_kernel_uses_no_scratch_and_no_more_registers():
    from foundationpose_amd import _lib
    meta = _kernel_metadata(_lib.LIB_PATH)
    (nname, nkv), (oname, okv) = _one(meta, NEW), _one(meta, OLD)
    res = {}
    for name, kv in ((nname, nkv), (oname, okv)):
        res[name] = dict(vgpr=int(kv["vgpr_count"]), agpr=int(kv.get("agpr_count", 0)), scratch=int(kv["private_segment_fixed_size"]),
                         vgpr_spills=int(kv.get("vgpr_spill_count", 0)), sgpr_spills=int(kv.get("sgpr_spill_count", 0)))
        print(f"{name}: {res[name]}")
    n, o = res[nname], res[oname]
    assert n["scratch"] == 0 and n["vgpr_spills"] == 0 and n["sgpr_spills"] == 0, (nname, n)
    # one unified register file: accumulation registers count
    assert n["vgpr"] + n["agpr"] <= o["vgpr"] + o["agpr"], (nname, n, oname, o)
    assert int(nkv["max_flat_workgroup_size"]) == int(okv["max_flat_workgroup_size"]) == 512      # two waves per SIMD
