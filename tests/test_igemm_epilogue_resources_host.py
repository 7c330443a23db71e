"""CPU: the implicit-GEMM kernels of the built library (csrc/conv_sw.hip, igemm_pp.hip, igemm.hip) hold every value in registers.

Each of them carries the generic epilogue and one body per layer kind (csrc/igemm_epilogue.h); a kernel's register count is the
largest over its paths, and a path that spilled would put scratch traffic into every tile of every launch.  There is a second way to
scratch that no register count shows: past a bounded number of reads of the by-value kernel argument block the compiler copies the
whole block to private memory (IgEpiArgs in igemm_epilogue.h has the story), which the metadata reports as a private segment.
Read from the kernel metadata of the gfx950 code objects as tests/test_conv_sw_resources_host.py reads them.  Resource numbers only;
no instruction is looked at."""
import re

from test_conv_sw_resources_host import _kernel_metadata

FAMILIES = ("k_conv_sw", "k_igemm_pp", "k_igemm_f16")
# the shifted-window kernels of the library, exactly: two tiles x two MFMA shapes, and the direct-store kernel of the 512 x 128 tile
CONV_SW = {f"k_conv_sw<{tile}, 4, {s16}>" for tile in ("256, 256", "512, 128") for s16 in ("true", "false")} | {"k_conv_sw_direct<512, 128, 4, true>"}


def test_igemm_kernels_have_no_scratch_and_no_spills():
    from foundationpose_amd import _lib
    meta = _kernel_metadata(_lib.LIB_PATH)
    seen = {f: 0 for f in FAMILIES}
    conv_sw = set()
    bad = []
    for name, kv in sorted(meta.items()):
        fam = next((f for f in FAMILIES if re.search(r"\b" + f + r"(_direct)?<", name)), None)
        if fam is None:
            continue
        seen[fam] += 1
        if fam == "k_conv_sw":
            conv_sw.add(re.search(r"\bk_conv_sw(_direct)?<[^>]*>", name).group(0))
        scratch, spills = int(kv["private_segment_fixed_size"]), int(kv.get("vgpr_spill_count", 0))
        sgpr_spills = int(kv.get("sgpr_spill_count", 0))
        print(f"{name}: vgpr {kv['vgpr_count']} sgpr {kv.get('sgpr_count')} scratch {scratch} vgpr spills {spills} sgpr spills {sgpr_spills}")
        if scratch != 0 or spills != 0:
            bad.append((name, scratch, spills))
    assert all(n >= 1 for n in seen.values()), seen          # every family is in the library: the name patterns still match
    assert conv_sw == CONV_SW and seen["k_conv_sw"] == len(CONV_SW), sorted(conv_sw)
    assert not bad, bad
