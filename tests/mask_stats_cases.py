"""Generated inputs for fp_mask_depth_stats (k_mask_depth_stats of csrc/frame_ops.hip): frames, depth sets built from bit patterns
so that every digit of the radix select decides, and masks at the frame's and the loads' edges.  Seeded, numpy only.  cases() returns
a list of named records (plain dicts): depth (V,H,W) f32, masks (M,H,W) uint8, view (M,) int32 or None, min_depth, targets (what the
case is there for) and reach, a predicate over the rows of tests/mask_stats_model.py that says whether the case got where it aims.
tests/test_mask_stats_cases_host.py (CPU) and tests/test_gpu_mask_stats_edges.py (GPU) use the same records.  Test infrastructure
only; not a conftest."""
import functools

import numpy as np

F = np.float32
U = np.uint32
FRAMES = ((1, 1), (1, 7), (5, 1), (2, 2), (6, 10), (33, 65), (64, 64), (481, 643))      # (H, W)
MIN_DEPTH = F(0.001)
INVALID = np.array([0x00000001, 0x007FFFFF, 0x80000000, 0x80000001, 0xBF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800000, 0],
                   U).view(F)        # two subnormals, -0.0, a negative subnormal, -1, NaN of both signs, a signalling NaN, -inf, 0


def _b(x):
    return int(F(x).view(U))


def _f(b):
    return np.asarray(b, U).view(F)


def _frame_of(values, H, W, seed, fill=0.0):
    """the values scattered over an (H, W) frame in a seeded order (cycled when there are fewer than H * W), `fill` nowhere"""
    v = np.asarray(values, F).reshape(-1)
    idx = np.random.default_rng(seed).permutation(H * W)
    out = np.full(H * W, fill, F)
    out[idx] = v[np.arange(H * W) % len(v)]
    return out.reshape(H, W)


def _mask_of(sel, value=1):
    return np.where(sel, np.uint8(value), np.uint8(0)).astype(np.uint8)


def digit_values(byte):
    """positive floats >= 0.001 that differ from each other only in byte `byte` (3 = most significant) of their bit pattern"""
    if byte == 3:
        return _f((np.arange(0x3B, 0x7F, dtype=np.int64) << 24 | 0x00123456).astype(U))
    base = {2: 0x3F001234, 1: 0x3F800012, 0: 0x3F800000}[byte]
    return _f((base | (np.arange(256, dtype=np.int64) << (8 * byte))).astype(U))


def _lohi(rows):
    return rows[:, 5].view(U), rows[:, 6].view(U)


def _first_diff_byte(a, b):
    x = int(a) ^ int(b)
    return -1 if x == 0 else (x.bit_length() - 1) // 8


def _fdb(rows):
    """the most significant byte in which lo and hi of row 0 differ (-1: equal)"""
    lo, hi = _lohi(rows)
    return _first_diff_byte(lo[0], hi[0])


def _frame_masks(H, W, depth3, rng):
    """the masks every frame size gets -> list of (name, view, mask)"""
    yy, xx = np.mgrid[0:H, 0:W]
    flat = (yy * W + xx)
    out = [("empty", 0, np.zeros((H, W), np.uint8)),
           ("full_255", 1, np.full((H, W), 255, np.uint8)),
           ("full_1", 2, np.ones((H, W), np.uint8)),
           ("random_128", 0, _mask_of(rng.random((H, W)) < 0.5, 128)),
           ("four_corners", 1, _mask_of(((yy == 0) | (yy == H - 1)) & ((xx == 0) | (xx == W - 1)), 255)),
           ("last_pixel", 2, _mask_of((yy == H - 1) & (xx == W - 1), 1)),
           ("last_byte_of_words", 0, _mask_of(flat % 4 == 3, 128)),
           ("one_last_byte", 1, _mask_of(flat == (H * W - 1 if H * W < 4 else 4 * ((H * W) // 8) + 3), 255))]
    bh, bw = max(1, H // 3), max(1, W // 3)
    for nm, (r0, c0) in dict(tl=(0, 0), tr=(0, W - bw), bl=(H - bh, 0), br=(H - bh, W - bw)).items():
        out.append(("box_" + nm, len(out) % 3, _mask_of((yy >= r0) & (yy < r0 + bh) & (xx >= c0) & (xx < c0 + bw), 1 + len(out))))
    with np.errstate(invalid="ignore"):
        out.append(("only_invalid_depths", 0, _mask_of(~(depth3[0] >= MIN_DEPTH), 77)))
    out.append(("view_minus_1", -1, np.full((H, W), 255, np.uint8)))
    out.append(("view_V", 3, np.full((H, W), 255, np.uint8)))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, depth, masks, view, targets, reach, min_depth=MIN_DEPTH):
        depth = np.ascontiguousarray(depth, F)
        depth = depth[None] if depth.ndim == 2 else depth
        masks = np.ascontiguousarray(masks, np.uint8)
        masks = masks[None] if masks.ndim == 2 else masks
        out.append(dict(name=name, depth=depth, masks=masks, view=None if view is None else np.asarray(view, np.int32),
                        min_depth=F(min_depth), targets=targets, reach=reach))

    # ---- every frame size: three frames (views in any order, -1 and V among them) and the masks of _frame_masks
    for (H, W) in FRAMES:
        rng = np.random.default_rng(1000 * H + W)
        spread = (10.0 ** rng.uniform(-3, 6, H * W)).astype(F)
        f0 = _frame_of(spread, H, W, 1)
        if H * W > 1:
            bad = rng.random((H, W)) < 0.25
            bad[0, 0] = True
            bad[-1, -1] = False
            f0[bad] = INVALID[rng.integers(0, len(INVALID), int(bad.sum()))]
        f1 = _frame_of(np.concatenate([digit_values(b) for b in (3, 2, 1, 0)]), H, W, 2)
        f2 = _frame_of([MIN_DEPTH, np.nextafter(MIN_DEPTH, F(0)), np.nextafter(MIN_DEPTH, F(1)), F(np.inf), F(0.75)], H, W, 3)
        d3 = np.stack([f0, f1, f2])
        ms = _frame_masks(H, W, d3, rng)
        nm = "frame_%dx%d" % (H, W)

        def reach(rows, ms=ms, H=H, W=W):
            names = [m[0] for m in ms]
            full = rows[names.index("full_255")]
            ok = rows[names.index("empty")][4] == 0 and tuple(full[:4]) == (0, H - 1, 0, W - 1)
            ok = ok and tuple(rows[names.index("last_pixel")][:4]) == (H - 1, H - 1, W - 1, W - 1)
            ok = ok and rows[names.index("only_invalid_depths")][4] == 0
            ok = ok and (H * W == 1) == (rows[names.index("only_invalid_depths")][0] < 0)     # a box without a valid depth
            return bool(ok and (rows[[names.index("view_minus_1"), names.index("view_V")], :5] == [-1, -1, -1, -1, 0]).all())
        add(nm, d3, np.stack([m[2] for m in ms]), [m[1] for m in ms],
            "%d x %d%s: %s" % (H, W, " (HW %% 4 == 0, W %% 4 != 0)" if (H * W) % 4 == 0 and W % 4 else "", ", ".join(m[0] for m in ms)),
            reach)

    # ---- depth sets on one 64 x 64 frame without a view index (M = 1): each digit of the select decides
    H, W = 64, 64
    full = np.full((H, W), 255, np.uint8)

    def one(name, values, targets, reach, min_depth=MIN_DEPTH):
        """a full mask over a frame that holds a list of values scattered and cycled, or over a ready (H, W) frame"""
        add(name, _frame_of(values, H, W, 5) if np.ndim(values) < 2 else values, full, None, targets, reach, min_depth)

    def sparse(values):
        """a frame with exactly these depths, every other pixel 0"""
        d = np.zeros(H * W, F)
        idx = np.random.default_rng(len(values)).choice(H * W, len(values), replace=False)
        d[idx] = np.asarray(values, F)
        return d.reshape(H, W)

    one("all_equal", [0.75], "every valid depth equal: one bin per digit holds both ranks",
        lambda r: r[0, 4] == H * W and r[0, 5] == r[0, 6] == _b(F(0.75)))
    one("two_values_even", [0.5, 2.0], "two values, even n: the median straddles them",
        lambda r: r[0, 4] % 2 == 0 and (r[0, 5], r[0, 6]) == (_b(F(0.5)), _b(F(2.0))))
    for b in (3, 2, 1, 0):
        one("differ_in_byte%d" % b, sparse(digit_values(b)), "an even number of depths that differ only in byte %d of their bits" % b,
            lambda r, b=b: _fdb(r) == b and r[0, 4] == len(digit_values(b)))
    one("spread_1e-3_1e6", (10.0 ** np.random.default_rng(9).uniform(-3, 6, H * W)).astype(F), "a spread from 1e-3 to 1e6",
        lambda r: r[0, 4] == H * W and _fdb(r) >= 0)
    one("ranks_part_at_first_digit", np.concatenate([_f(np.full(2048, 0x3E123456, U)), _f(np.full(2048, 0x40123456, U))]),
        "lo and hi differ in the most significant digit", lambda r: _fdb(r) == 3 and r[0, 4] == 4096)
    one("ranks_part_at_last_digit", np.concatenate([_f(np.full(2048, 0x3F800001, U)), _f(np.full(2048, 0x3F800002, U))]),
        "lo and hi share three digits and differ in the last", lambda r: _fdb(r) == 0 and r[0, 4] == 4096)
    md_lo, md_hi = np.nextafter(MIN_DEPTH, F(0)), np.nextafter(MIN_DEPTH, F(1))
    one("at_min_depth", sparse([MIN_DEPTH, md_lo, md_lo, md_lo]), "a depth exactly at min_depth is valid, one ulp below is not",
        lambda r: r[0, 4] == 1 and r[0, 5] == r[0, 6] == _b(MIN_DEPTH))
    one("around_min_depth", sparse([MIN_DEPTH, md_lo, md_hi, md_hi]), "min_depth, nextafter below and above it",
        lambda r: r[0, 4] == 3 and r[0, 5] == r[0, 6] == _b(md_hi))
    for md in (0.5, 1e-6):
        md = F(md)
        vals = np.concatenate([[md, np.nextafter(md, F(0)), np.nextafter(md, F(1))] * 5, 10.0 ** np.random.default_rng(3).uniform(-8, 1, 500)])
        one("min_depth_%g" % md, vals.astype(F), "min_depth = %g: depths on both sides of it and at it" % md,
            lambda r, md=md, vals=vals.astype(F): 0 < r[0, 4] < H * W and r[0, 4] == int((_frame_of(vals, H, W, 5) >= md).sum()),
            min_depth=md)
    one("invalid_only", INVALID, "subnormals, -0.0, negatives, NaN of both signs, -inf, 0: none is valid",
        lambda r: r[0, 4] == 0 and r[0, 0] == 0 and r[0, 5] == 0x7FC00000)
    one("invalid_and_three_valid", np.where(sparse([1.5, 0.25, 3.0]) != 0, sparse([1.5, 0.25, 3.0]), _frame_of(INVALID, H, W, 4)),
        "three valid depths among invalid ones of every kind", lambda r: r[0, 4] == 3 and r[0, 5] == r[0, 6] == _b(F(1.5)))
    one("inf_is_hi_alone", sparse([1.0, np.inf]), "+inf is valid and sorts last: hi = +inf, lo = 1",
        lambda r: (r[0, 4], r[0, 5], r[0, 6]) == (2, 0x3F800000, 0x7F800000))
    one("inf_is_lo_and_hi", sparse([1.0, np.inf, np.inf, np.inf]), "+inf is both middle elements",
        lambda r: (r[0, 4], r[0, 5], r[0, 6]) == (4, 0x7F800000, 0x7F800000))
    rng = np.random.default_rng(12)
    for n in (1, 2, 3, 4, 1025):
        one("n_%d" % n, sparse(rng.uniform(0.3, 2.0, n).astype(F)), "exactly %d valid depths%s" % (n, " (more than one per thread)" if n > 1024 else ""),
            lambda r, n=n: r[0, 4] == n and (n % 2 == 1) == (r[0, 5] == r[0, 6]))
    Hb, Wb = FRAMES[-1]
    add("whole_481x643_valid", (10.0 ** np.random.default_rng(13).uniform(-2.9, 3, (Hb, Wb))).astype(F), np.ones((Hb, Wb), np.uint8), None,
        "every pixel of a 481 x 643 frame inside and valid: the box is the frame",
        lambda r: tuple(r[0, :5]) == (0, Hb - 1, 0, Wb - 1, Hb * Wb))

    # ---- M = 70 and M = 12 random masks over three 33 x 65 frames
    Hm, Wm = 33, 65
    rng = np.random.default_rng(14)
    d3 = np.round(rng.uniform(0.3, 2.0, (3, Hm, Wm)), 2).astype(F)
    d3[rng.random((3, Hm, Wm)) < 0.2] = 0.0
    d3[1] = _frame_of(np.concatenate([digit_values(b) for b in (3, 2, 1, 0)]), Hm, Wm, 15)
    masks = np.stack([_mask_of(rng.random((Hm, Wm)) < p, 1 + k) for k, p in enumerate(rng.uniform(0.0, 0.6, 70) ** 2)])
    add("m_70", d3, masks, rng.integers(0, 3, 70), "70 masks in one launch, views in any order",
        lambda r: len(r) == 70 and len(set(r[:, 4] % 2)) == 2 and (r[:, 4] > 0).sum() > 50)
    add("m_12", d3, masks[40:52], rng.integers(0, 3, 12), "12 masks in one launch", lambda r: len(r) == 12 and (r[:, 4] > 0).sum() >= 6)
    return out
