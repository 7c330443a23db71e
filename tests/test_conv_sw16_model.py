"""CPU: numpy model of the addressing of k_conv_sw<.., S16 = true> (foundationpose_amd/csrc/conv_sw.hip), the shifted-window 3x3
convolution on v_mfma_f32_16x16x32_f16: the LDS-DMA lane -> (padded pixel, 16-byte chunk) map of the patch staging with the
swizzle of that loop (chunk ^ 2 * ((row >> 2) & 1)), the three-instruction tap address the kernel computes in the MFMA shadow, and
the fragment map lane -> (row lane & 15, chunk lane >> 4): ONE ds_read_b128 per K = 32 fragment of 16 rows.  Together they must
deliver, for GEMM row m and k = (tap, ci), the element x[b, oy+ky, ox+kx, ci] of the zero-bordered NHWC input -- including tiles
that cross image rows and images, and the clamped rows of the last tile.  The weight side: the LDS image of the 32x32x16 loop (and of
fp_pack_conv3x3_tiles_f16) read with the tile's channel quads in the order sigma = (0, 2, 3, 1), which the epilogue undoes.
Bank conflicts: ds_read_b128 serves a wave in four NON-contiguous groups of 16 lanes; every group must hit 16 distinct 16-byte
slots of the 256-byte bank row for 16 consecutive patch rows at any offset, at most two lanes per slot across one image-row crossing.
(The kernel itself is tested on the GPU: tests/test_gpu_conv_sw16.py.)"""
import numpy as np
import pytest

SIGMA = (0, 2, 3, 1)
# the lanes ds_read_b128 serves together (one 256-byte bank row per group)
GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
GROUPS = GROUPS + [[l + 32 for l in g] for g in GROUPS]


def swzp(row): return (row >> 1) & 2          # patch rows of the 16x16x32 loop
def swzw(row): return (row >> 2) & 3          # weight rows (unchanged)


def tap_address(abase, shift):
    """the kernel's form: abase = (row at tap (0,0)) << 6 | chunk << 4; add the tap's shift, flip bit 5 by bit 2 of the row"""
    x = abase + (shift << 6)
    return x ^ ((x >> 3) & 32)


def run(B, Ho, Wo, Cin, m0, seed=0, BM=512):
    TM = 4
    Hp, Wp = Ho + 2, Wo + 2
    HoWo = Ho * Wo
    M = B * HoWo
    rng = np.random.default_rng(seed)
    cstride = Cin
    x = rng.integers(1, 2**30, size=(B * Hp * Wp * cstride,), dtype=np.int64)   # unique-ish element ids

    def q_of(m):
        b = m // HoWo; r = m - b * HoWo; oy = r // Wo; ox = r - oy * Wo
        return (b * Hp + oy) * Wp + ox
    q0 = q_of(m0); qmax = B * Hp * Wp - 1
    PROWS = 512 if BM == 256 else 768
    PI = PROWS // 16 // 8
    for cc in range(Cin // 32):
        # ---- patch image in LDS: the destination is lane-linear, the swizzle sits on the source address
        lds = np.zeros((PROWS * 32,), dtype=np.int64)
        for wid in range(8):
            for j in range(PI):
                for lane in range(64):
                    row = (wid * PI + j) * 16 + (lane >> 2)
                    c = (lane & 3) ^ swzp(row)
                    q = min(q0 + row, qmax)
                    src = q * cstride + c * 8 + cc * 32
                    dst_byte = (wid * PI + j) * 1024 + lane * 16
                    lds[dst_byte // 2: dst_byte // 2 + 8] = x[src:src + 8]
        # ---- fragment reads: 8 pixel fragments of 16 rows per wave row block of 128 pixels
        for wm in range(BM // (32 * TM)):
            for t in range(2 * TM):
                for lane in range(64):
                    frow, fch = lane & 15, lane >> 4
                    m = m0 + wm * (32 * TM) + t * 16 + frow
                    mc = min(m, M - 1)
                    abase = ((q_of(mc) - q0) << 6) + (fch << 4)
                    for tap in range(9):
                        ky, kx = tap // 3, tap % 3
                        addr = tap_address(abase, ky * Wp + kx)
                        assert 0 <= addr < PROWS * 64 and addr % 16 == 0, (addr, m0, m)
                        got = lds[addr // 2: addr // 2 + 8]
                        b = mc // HoWo; r = mc - b * HoWo; oy = r // Wo; ox = r - oy * Wo
                        # lane l of a 16x16x32 operand holds k elements 8 * (l >> 4) .. + 7 of its row
                        src = ((b * Hp + oy + ky) * Wp + ox + kx) * cstride + cc * 32 + 8 * fch
                        assert np.array_equal(got, x[src:src + 8]), (m, tap, lane)
    return True


# the tile cases of tests/test_conv_sw_model.py: tiles crossing image rows and images, the clamped rows of the last tile, the 40- and
# 20-pixel widths (and 24), the 512-row tile with 768 patch rows and the 256-row tile with 512
@pytest.mark.parametrize("B,Ho,Cin,m0,BM", [(3, 40, 64, 0, 256), (3, 40, 64, 1536, 256), (3, 40, 64, 4608, 256),
                                            (5, 20, 64, 256, 256), (5, 20, 64, 1792, 256),
                                            (3, 40, 64, 0, 512), (3, 40, 64, 1536, 512), (3, 40, 64, 4608, 512),
                                            (3, 24, 64, 1536, 512), (6, 20, 64, 1024, 512)])
def test_conv_sw16_patch_and_fragment_addressing(B, Ho, Cin, m0, BM):
    assert run(B, Ho, Ho, Cin, m0, BM=BM)


def test_conv_sw16_tap_address_is_the_swizzled_row_address():
    for row0 in range(0, 700, 7):
        for fch in range(4):
            for shift in (0, 1, 2, 22, 23, 24, 42, 43, 44, 45, 46, 84, 85, 86):
                pr = row0 + shift
                assert tap_address((row0 << 6) + (fch << 4), shift) == (pr << 6) + ((fch ^ swzp(pr)) << 4)


def ways(rows, swizzle):
    """the worst number of lanes of one ds_read_b128 lane group on one 16-byte slot; rows[j] = the LDS row of fragment row j"""
    worst = 1
    for g in GROUPS:
        slots = {}
        for l in g:
            r, c = rows[l & 15], l >> 4
            slot = (((r << 6) + ((c ^ swizzle(r)) << 4)) % 256) // 16
            slots[slot] = slots.get(slot, 0) + 1
        worst = max(worst, max(slots.values()))
    return worst


def test_conv_sw16_fragment_reads_are_bank_conflict_free():
    # tap shifts of the 40- and 20-pixel widths (Wp = 42, 22) and of 24 (Wp = 26)
    shifts = (0, 1, 2, 42, 43, 44, 84, 85, 86, 22, 23, 24, 45, 46, 26, 27, 28, 52, 53, 54)
    # 16 consecutive patch rows at every row offset 0..63 and every tap shift: conflict-free
    assert max(ways([off + s + j for j in range(16)], swzp) for off in range(64) for s in shifts) == 1
    # one image-row crossing (a gap of 2 patch rows) at every position inside the fragment: at most 2-way
    assert max(ways([off + s + (j if j < c else j + 2) for j in range(16)], swzp)
               for off in range(64) for s in shifts for c in range(1, 16)) <= 2
    # why the swizzle had to change: the one of the 32x32x16 loop is 2-way under this lane map, already without a crossing
    assert max(ways([off + j for j in range(16)], swzw) for off in range(64)) == 2


def test_conv_sw16_weight_fragments_read_the_old_image_conflict_free():
    """weight fragment t of wave column wn: A row r of the MFMA = LDS row wn * 64 + t * 16 + 4 * sigma(r >> 2) + (r & 3) of the image
    chunk c at c ^ ((row >> 2) & 3) -- the 32x32x16 loop's, and fp_pack_conv3x3_tiles_f16's.  Every channel of the 128 is read once, a
    lane's accumulator quad (lane >> 4) is the channel quad sigma(lane >> 4), and the aligned reads are conflict-free."""
    seen = []
    for wn in range(2):
        for t in range(4):
            rows = [wn * 64 + t * 16 + 4 * SIGMA[r >> 2] + (r & 3) for r in range(16)]
            assert ways(rows, swzw) == 1
            assert ways([wn * 64 + t * 16 + r for r in range(16)], swzw) == 2      # the plain row order is not
            for g in range(4):                                                     # D rows 4 g + e <-> channels 4 sigma(g) + e
                assert rows[4 * g: 4 * g + 4] == [wn * 64 + t * 16 + 4 * SIGMA[g] + e for e in range(4)]
            seen += rows
    assert sorted(seen) == list(range(128))
    assert [(0x1320 >> (4 * q)) & 3 for q in range(4)] == list(SIGMA)              # the kernel's packed table
