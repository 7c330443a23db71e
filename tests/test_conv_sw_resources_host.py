"""CPU: what one workgroup of the product's 3x3 convolution, k_conv_sw<512,128,4,true> (csrc/conv_sw.hip), takes of a CU, read from the
kernel metadata of the built library's gfx950 code objects (as csrc/check_no_pk_f32.py reads the objects) and from the two launchers.

A CU has 512 registers per SIMD lane and 160 KiB of LDS.  The kernel runs eight waves, two per SIMD; at 256 registers they fill the
register file and no wave of another stream's light kernel (rasteriser, warp, row kernels) can start beside a tile, and none of the
conv's tiles beside such a wave.  At 224 or fewer, 2 x 224 leaves 64 registers per lane: one wave of any light kernel.  The LDS side of
the same statement: a conv workgroup and a workgroup of k_raster, the one light kernel with a large LDS request, fit together.
Resource numbers only; no instruction is looked at."""
import os
import re
import subprocess
import sys
import tempfile

from conftest import ROOT

CSRC = os.path.join(ROOT, "foundationpose_amd", "csrc")
KERNEL = "k_conv_sw<512, 128, 4, true>"
CU_LDS = 160 * 1024


def _kernel_metadata(lib):
    """{demangled kernel name: {metadata key: int}} of every gfx950 code object in the library"""
    sys.path.insert(0, CSRC)
    try:
        import check_no_pk_f32 as ck
    finally:
        sys.path.remove(CSRC)
    assert ck.LLVM, "the LLVM tools of the ROCm toolchain are needed to read the code objects"
    out = {}
    for co in ck.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            txt = subprocess.run([os.path.join(ck.LLVM, "llvm-readelf"), "--notes", f.name], capture_output=True, text=True, check=True).stdout
        # one YAML map per kernel under amdhsa.kernels; a new list item ("- .key:") starts the next kernel (argument maps are nested deeper)
        for block in re.split(r"\n  - ", txt.split("amdhsa.kernels:", 1)[-1]):
            kv = dict(re.findall(r"^\s{4}\.?(\w+):\s*(\S+)\s*$", "    " + block, flags=re.M))
            if "symbol" in kv and "vgpr_count" in kv:
                out[kv["symbol"].strip("'\"").replace(".kd", "")] = kv
    names = list(out)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    return {d: out[n] for d, n in zip(dem, names)}


def test_conv_tile_leaves_room_for_a_light_wave():
    from foundationpose_amd import _lib
    meta = _kernel_metadata(_lib.LIB_PATH)
    hits = [(k, v) for k, v in meta.items() if KERNEL in k]
    assert len(hits) == 1, (KERNEL, sorted(meta)[:8], len(meta))
    name, kv = hits[0]
    vgpr, agpr = int(kv["vgpr_count"]), int(kv.get("agpr_count", 0))
    scratch, spills = int(kv["private_segment_fixed_size"]), int(kv.get("vgpr_spill_count", 0))
    print(f"{name}: vgpr {vgpr} agpr {agpr} scratch {scratch} spills {spills} max workgroup {kv.get('max_flat_workgroup_size')}")
    assert int(kv["max_flat_workgroup_size"]) == 512          # two waves per SIMD
    # one unified register file: with accumulation registers in use the two counts would have to be added up first
    assert agpr == 0 and vgpr <= 224, (vgpr, agpr)
    assert scratch == 0 and spills == 0, (scratch, spills)


def test_conv_and_raster_workgroups_share_the_lds():
    from foundationpose_amd import _lib
    lib = _lib.lib()
    conv, raster = int(lib.fp_conv3x3_sw_lds_bytes()), int(lib.fp_raster_lds_bytes(160))    # 160-pixel crops: every product render
    print(f"LDS: conv tile {conv} B + raster strip {raster} B = {conv + raster} of {CU_LDS}")
    assert conv >= 512 * 128 * 2 and raster >= 16 * 160 * 8                               # the E tile / the strip's z-buffer
    assert conv + raster <= CU_LDS
    # ... and in the hardware's 1280-byte allocation granules as well
    gran = lambda b: -(-b // 1280) * 1280
    assert gran(conv) + gran(raster) <= CU_LDS
