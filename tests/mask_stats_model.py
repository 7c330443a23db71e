"""What fp_mask_depth_stats returns, restated in plain numpy (no GPU, no import of the product): per mask the box of its nonzero
bytes, the count n of its depths d >= min_depth, and elements (n-1)//2 and n//2 of np.sort over those depths as float32 bits.
The three special rows are the ones include/fp_amd.h states: an empty mask has a box of -1 and n = 0, a mask without a valid depth
keeps its box and has n = 0, a view index outside 0..V-1 reads nothing and reports an empty mask; lo / hi are the quiet NaN
0x7fc00000 whenever n == 0.  `variant` names one deliberately wrong reading of that definition: tests/test_mask_stats_cases_host.py
shows that the cases of tests/mask_stats_cases.py tell each of them from the right one.  Test infrastructure only."""
import numpy as np

F = np.float32
NAN_BITS = 0x7FC00000
VARIANTS = ("gt_min_depth", "nan_counted", "box_over_valid", "upper_median_only", "ranks_over_box")


def _row(box, n, lo_bits, hi_bits):
    return np.array(list(box) + [n, lo_bits, hi_bits, 0], np.int64).astype(np.uint32).view(np.int32)


def mask_row(depth, mask, min_depth=0.001, variant=None):
    """depth (H,W) f32, mask (H,W) uint8 -> the (8,) int32 row {v0, v1, u0, u1, n, bits(lo), bits(hi), 0}"""
    assert variant is None or variant in VARIANTS, variant
    d = np.ascontiguousarray(depth, F)
    inside = np.asarray(mask) != 0
    md = F(min_depth)
    with np.errstate(invalid="ignore"):
        if variant == "gt_min_depth":
            ok = d > md
        elif variant == "nan_counted":
            ok = ~(d < md)
        else:
            ok = d >= md
    boxed = inside & ok if variant == "box_over_valid" else inside
    rows, cols = np.flatnonzero(boxed.any(axis=1)), np.flatnonzero(boxed.any(axis=0))
    box = [-1, -1, -1, -1] if rows.size == 0 else [rows[0], rows[-1], cols[0], cols[-1]]
    pick = inside
    if variant == "ranks_over_box" and rows.size:
        pick = np.zeros_like(inside)
        pick[box[0]:box[1] + 1, box[2]:box[3] + 1] = True
    z = np.sort(d[pick & ok])
    n = int(z.size)
    if n == 0:
        return _row(box, 0, NAN_BITS, NAN_BITS)
    lo, hi = z[n // 2 if variant == "upper_median_only" else (n - 1) // 2], z[n // 2]
    return _row(box, n, int(lo.view(np.uint32)), int(hi.view(np.uint32)))


def mask_stats(depth, masks, view=None, min_depth=0.001, variant=None):
    """depth (V,H,W) f32, masks (M,H,W) uint8, view (M,) or None (all 0) -> (M,8) int32"""
    depth = np.ascontiguousarray(depth, F)
    V = depth.shape[0]
    out = np.zeros((len(masks), 8), np.int32)
    for m in range(len(masks)):
        v = 0 if view is None else int(view[m])
        out[m] = _row([-1] * 4, 0, NAN_BITS, NAN_BITS) if not 0 <= v < V else mask_row(depth[v], masks[m], min_depth, variant)
    return out


def host(stats):
    """-> (box (M,4) int64, n (M,) int64, lo (M,) f32, hi (M,) f32), as ops.mask_depth_stats_host splits the table"""
    a = np.ascontiguousarray(stats, np.int32)
    return a[:, :4].astype(np.int64), a[:, 4].astype(np.int64), a[:, 5].view(F).copy(), a[:, 6].view(F).copy()
