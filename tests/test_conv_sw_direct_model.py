"""CPU: numpy model of the lane map of k_conv_sw_direct (foundationpose_amd/csrc/conv_sw.hip, csrc/igemm_epilogue.h ig_epilogue_direct), the
512 x 128 tile of the shifted-window 3x3 convolution stored straight from its accumulators.

The kernel issues v_mfma_f32_16x16x32_f16 with pixels as A and weights as B.  A and B fragments have one layout (lane l: row or column
l & 15, k chunk l >> 4), D is [A row][B column] with lane l holding column l & 15 of rows 4 (l >> 4) + e, e = 0..3.  The fragment read of
the weights is the one of k_conv_sw (w_off: fragment t of wave column wn, lane row frow -> LDS row
64 wn + 16 t + 4 sigma(frow >> 2) + (frow & 3), what makes it conflict-free), so the IMAGE is permuted: LDS row r holds weight row rho(r)
(sw_direct_row; fp_pack_conv3x3_tiles_direct_f16 and the plain path's DMA source rows), the chunks of a row where they were.  Then
column c of fragment t is channel 64 wn + 4 c + t: a lane owns four consecutive channels of a pixel, 16 lanes a pixel's 64.
(The kernel itself is tested on the GPU: tests/test_gpu_conv_sw_direct.py.)"""
import numpy as np

from test_conv_sw16_model import SIGMA, swzw, ways

TAU = (0, 3, 1, 2)                                  # sigma's inverse
BM, BN, TM = 512, 128, 4


def rho(r):
    """weight row (of the 128-channel tile) that LDS row r holds; the kernel's packed table is 0x2130"""
    return (r & 64) + 4 * (4 * ((0x2130 >> (4 * ((r >> 2) & 3))) & 3) + (r & 3)) + ((r >> 4) & 3)


def w_row(wn, t, frow):
    """LDS row that lane row frow of weight fragment t reads (w_off of conv_sw.hip, unchanged)"""
    return wn * 64 + t * 16 + 4 * SIGMA[frow >> 2] + (frow & 3)


def test_rho_is_a_permutation_built_on_sigmas_inverse():
    assert [SIGMA[TAU[q]] for q in range(4)] == [0, 1, 2, 3]
    assert [(0x2130 >> (4 * q)) & 3 for q in range(4)] == list(TAU)
    assert sorted(rho(r) for r in range(128)) == list(range(128))
    assert all((rho(r) >> 6) == (r >> 6) for r in range(128))          # a wave column keeps its 64 channels


def test_column_c_of_fragment_t_is_channel_4c_plus_t():
    for wn in range(2):
        for t in range(4):
            for c in range(16):
                assert rho(w_row(wn, t, c)) == 64 * wn + 4 * c + t


def test_pack_layout_puts_the_chunks_where_the_fragment_read_looks():
    """the image of one k-step as fp_pack_conv3x3_tiles_direct_f16 writes it (row r: weight row rho(r), chunk lc at lc ^ swz(r)), read as the
    kernel reads it (w_off: row, chunk (l >> 4) ^ swz(row)): lane l of fragment t gets k chunk l >> 4 of channel 64 wn + 4 (l & 15) + t"""
    w = np.arange(128 * 4).reshape(128, 4)           # id of (weight row, k chunk)
    img = np.zeros((128, 4), dtype=np.int64)
    for r in range(128):
        for pc in range(4):
            img[r, pc] = w[rho(r), pc ^ swzw(r)]
    for wn in range(2):
        for t in range(4):
            for lane in range(64):
                rw = w_row(wn, t, lane & 15)
                assert img[rw, (lane >> 4) ^ swzw(rw)] == w[64 * wn + 4 * (lane & 15) + t, lane >> 4]


def test_fragment_read_has_the_bank_pattern_of_the_present_image():
    """the rows and chunk positions a fragment read touches do not depend on what the rows hold: the same conflict-free reads"""
    for wn in range(2):
        for t in range(4):
            rows = [w_row(wn, t, r) for r in range(16)]
            assert ways(rows, swzw) == 1
    # and the permutation cannot be had in the read instead: the rows a lane group would then read, 4 apart, share their banks
    assert max(ways([wn * 64 + 4 * c + t for c in range(16)], swzw) for wn in range(2) for t in range(4)) > 1


def test_every_element_of_the_tile_is_stored_once_in_whole_lines():
    """acc[t][j][e] of lane l of wave (wm, wn): pixel row wm * 128 + 16 j + 4 (l >> 4) + e, channel wn * 64 + 4 (l & 15) + t; a store is the
    lane's four channels of one pixel (8 bytes at byte 2 * channel of the row)"""
    count = np.zeros((BM, BN), dtype=np.int64)
    for wid in range(8):
        wm, wn = wid // 2, wid % 2
        for j in range(2 * TM):
            for e in range(4):
                lines = {}
                for lane in range(64):
                    row = wm * 32 * TM + 16 * j + 4 * (lane >> 4) + e
                    ch = [wn * 64 + 4 * (lane & 15) + t for t in range(4)]
                    assert ch == list(range(ch[0], ch[0] + 4)) and ch[0] % 4 == 0          # one aligned 8-byte store
                    count[row, ch] += 1
                    lines.setdefault(row, []).append(2 * ch[0])
                # one store instruction: four pixels, each one aligned 128-byte line from 16 consecutive lanes
                assert len(lines) == 4
                for row, offs in lines.items():
                    assert offs == list(range(offs[0], offs[0] + 128, 8)) and offs[0] % 128 == 0
                # the four row offsets a lane needs for (j, e = 0..3) are one aligned 16-byte read of the row table
                assert (wm * 32 * TM + 16 * j) % 4 == 0
    assert (count == 1).all()
