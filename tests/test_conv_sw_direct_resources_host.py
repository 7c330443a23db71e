"""CPU: what one workgroup of k_conv_sw_direct (csrc/conv_sw.hip), the 3x3 convolution tile stored straight from its accumulators, takes
of a CU -- the budget tests/test_conv_sw_resources_host.py holds k_conv_sw<512,128,4,true> to, for the kernel that takes its launches: eight
waves at no more than 224 registers (a third wave of a light kernel fits beside two of them on a SIMD) and not a byte of LDS more than
fp_conv3x3_sw_lds_bytes() (a k_raster workgroup fits beside it).  Read from the kernel metadata of the built library's gfx950 code objects.
Resource numbers only; no instruction is looked at."""
from test_conv_sw_resources_host import CU_LDS, _kernel_metadata

KERNEL = "k_conv_sw_direct<"
OLD = "k_conv_sw<512, 128, 4, true>"


def _hit(meta, pat):
    hits = [(k, v) for k, v in meta.items() if pat in k]
    assert len(hits) == 1, (pat, [k for k in sorted(meta) if "k_conv_sw" in k])
    return hits[0]


def test_direct_tile_keeps_the_budget_of_the_tile_it_replaces():
    from foundationpose_amd import _lib
    meta = _kernel_metadata(_lib.LIB_PATH)
    name, kv = _hit(meta, KERNEL)
    assert OLD not in name                                       # the A/B arm keeps that name to itself
    vgpr, agpr = int(kv["vgpr_count"]), int(kv.get("agpr_count", 0))
    scratch, spills = int(kv["private_segment_fixed_size"]), int(kv.get("vgpr_spill_count", 0))
    lds_static = int(kv["group_segment_fixed_size"])
    print(f"{name}: vgpr {vgpr} agpr {agpr} scratch {scratch} spills {spills} static LDS {lds_static} max workgroup {kv.get('max_flat_workgroup_size')}")
    assert int(kv["max_flat_workgroup_size"]) == 512
    assert agpr == 0 and vgpr <= 224, (vgpr, agpr)
    assert scratch == 0 and spills == 0 and int(kv.get("sgpr_spill_count", 0)) == 0, (scratch, spills)
    # LDS: the kernel declares none of its own (the launcher passes fp_conv3x3_sw_lds_bytes(), as for k_conv_sw), so what a workgroup
    # holds is that request
    budget = int(_lib.lib().fp_conv3x3_sw_lds_bytes())
    assert lds_static <= budget <= 136192, (lds_static, budget)       # a granule more ends the co-residency with k_raster
    gran = lambda b: -(-b // 1280) * 1280
    assert gran(max(lds_static, budget)) + gran(int(_lib.lib().fp_raster_lds_bytes(160))) <= CU_LDS
    # ... and the old kernel has the same static request: the two differ in nothing the launcher would have to know
    assert int(_hit(meta, OLD)[1]["group_segment_fixed_size"]) == lds_static
