"""A second implementation of the coverage half of the rasteriser (DESIGN.md / SURVEY.md App. A.8; oracle/fp_oracle.c
fpo_render_crops, csrc/raster.hip): vectorised numpy, integers for coverage, float32 for the vertex pass and the depth key.
Stages: snap -> cull -> orientation -> edge ownership -> bounding-box rounding -> depth key -> per-pixel minimum.

`variant` switches ONE stage to a neighbouring, wrong definition (tests/test_geometry_cases_host.py shows that the generated cases
tell each of them from the right one):
  tie_high_id   equal depth keys: the higher triangle id wins
  owner_mirror  the edge ownership rule mirrored (an edge owns its points if it runs upwards / towards -x)
  draw_culled   a triangle with a culled vertex is still drawn if another of its vertices is valid
  bbox_outward  the clipped bounding box grown by one cell on every side; a cell outside the crop is addressed with the flat index
                j * ow + i like every other (growing the box BEFORE the clip cannot change a pixel: the edge functions reject every
                centre outside the box of the vertices)
  snap_away     the 1/16 px snap rounds halves away from zero instead of to even
Test infrastructure only."""
import numpy as np

F = np.float32
SUBPIX = F(16.0)
GUARD_LO, GUARD_HI = F(-8192.0), F(24575.0)
ZNEAR, ZMAX, ZSCALE = F(0.001), F(4095.0), F(1048576.0)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
BIG_CELLS, BIG_MAX, STRIP_ROWS = 24, 96, 16      # csrc/raster.hip FP_BIG_CELLS / FP_BIG_MAX / FP_STRIP_ROWS
VARIANTS = ("tie_high_id", "owner_mirror", "draw_culled", "bbox_outward", "snap_away")


def fmaf(a, b, c):
    """float32 fma(a, b, c) with ONE rounding.  a * b is exact in float64; the float64 sum p + c is rounded once, and rounding
    that to float32 is a second rounding that can only go wrong when the float64 sum sits exactly on a float32 midpoint while the
    exact sum does not: there the sign of TwoSum's exact residual decides."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)           # TwoSum: s + err == p + c exactly
        r = s.astype(np.float32)
        bits = s.view(np.int64) if s.ndim else np.asarray(s).reshape(1).view(np.int64).reshape(())
        mid = ((bits & 0x1FFFFFFF) == 0x10000000) & np.isfinite(s) & (err != 0) & np.isfinite(err)
        if np.any(mid):
            lo = (s - np.abs(s) * 2.0 ** -30).astype(np.float32)      # the float32 neighbours of the midpoint
            hi = (s + np.abs(s) * 2.0 ** -30).astype(np.float32)
            lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
            r = np.where(mid, np.where(err > 0, hi, lo), r)
    return r.astype(np.float32)


def project(pos, P, bbox, K9, H, W, oh, ow, variant=None):
    """vertex pass -> (xi, yi int64 snapped crop position, iw float32, valid bool)"""
    pos = np.asarray(pos, F)
    P = np.asarray(P, F).reshape(16)
    K9 = np.asarray(K9, np.float64).astype(F).reshape(9)
    fx, sk, cx, fy, cy = K9[0], K9[1], K9[2], K9[4], K9[5]
    umin, vmin, umax, vmax = (F(0), F(0), F(W), F(H)) if bbox is None else (F(b) for b in np.asarray(bbox, F))
    vx, vy, vz = pos[:, 0], pos[:, 1], pos[:, 2]
    with np.errstate(all="ignore"):
        ax, ay = F(ow) / (umax - umin), F(oh) / (vmax - vmin)
        xc = fmaf(P[0], vx, fmaf(P[1], vy, fmaf(P[2], vz, P[3])))
        yc = fmaf(P[4], vx, fmaf(P[5], vy, fmaf(P[6], vz, P[7])))
        zc = fmaf(P[8], vx, fmaf(P[9], vy, fmaf(P[10], vz, P[11])))
        ok = zc > ZNEAR
        iw = F(1.0) / zc
        pu = fmaf(fx, xc, sk * yc)
        pv = fy * yc
        u = fmaf(pu, iw, cx)
        v = fmaf(pv, iw, cy)
        X = (u - umin) * ax
        Y = (v - vmin) * ay
        xs16, ys16 = X * SUBPIX, Y * SUBPIX
        if variant == "snap_away":
            xs = (np.sign(xs16) * np.floor(np.abs(xs16) + F(0.5))).astype(F)
            ys = (np.sign(ys16) * np.floor(np.abs(ys16) + F(0.5))).astype(F)
        else:
            xs, ys = np.rint(xs16), np.rint(ys16)
        ok = ok & (xs >= GUARD_LO) & (xs <= GUARD_HI) & (ys >= GUARD_LO) & (ys <= GUARD_HI)
        lim = float(1 << 20)
        if variant == "draw_culled":    # the culled vertex keeps a position (held to a range the integers can carry)
            xi = np.clip(np.nan_to_num(xs.astype(np.float64), nan=0.0), -lim, lim).astype(np.int64)
            yi = np.clip(np.nan_to_num(ys.astype(np.float64), nan=0.0), -lim, lim).astype(np.int64)
        else:
            xi = np.where(ok, xs, 0).astype(np.int64)
            yi = np.where(ok, ys, 0).astype(np.int64)
    return xi, yi, iw.astype(F), ok


def _owner(dx, dy, mirror):
    if mirror:
        return (dy < 0) | ((dy == 0) & (dx < 0))
    return (dy > 0) | ((dy == 0) & (dx > 0))


def render(mesh, P, bbox, K, H, W, out_hw, variant=None, chunk_cells=1 << 22):
    """One hypothesis.  -> dict(tri_id (oh,ow) int32, zbuf (oh,ow) uint32, valid (V,) bool, drawn (T,) bool = valid and non-zero
    area, zero_area (T,) bool = all vertices valid but no area after the snap, big_per_strip (strips,) = triangles per 16-row
    strip whose clipped box has more than BIG_CELLS cells)."""
    assert variant is None or variant in VARIANTS, variant
    oh, ow = out_hw
    faces = np.asarray(mesh["faces"], np.int64)
    T = faces.shape[0]
    xi, yi, iw, ok = project(mesh["pos"], P, bbox, K, H, W, oh, ow, variant)
    fok = ok[faces]
    tri_ok = fok.any(1) if variant == "draw_culled" else fok.all(1)
    x0, y0 = xi[faces[:, 0]], yi[faces[:, 0]]
    x1, y1 = xi[faces[:, 1]], yi[faces[:, 1]]
    x2, y2 = xi[faces[:, 2]], yi[faces[:, 2]]
    w0i, w1i, w2i = iw[faces[:, 0]], iw[faces[:, 1]], iw[faces[:, 2]]
    area2 = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    zero_area = fok.all(1) & (area2 == 0)
    drawn = tri_ok & (area2 != 0)
    swap = area2 < 0                                   # orientation: positive area in the y-down crop space
    x1, x2 = np.where(swap, x2, x1), np.where(swap, x1, x2)
    y1, y2 = np.where(swap, y2, y1), np.where(swap, y1, y2)
    w1i, w2i = np.where(swap, w2i, w1i), np.where(swap, w1i, w2i)
    area2 = np.abs(area2)
    mirror = variant == "owner_mirror"
    b0 = np.where(_owner(x2 - x1, y2 - y1, mirror), 0, -1)
    b1 = np.where(_owner(x0 - x2, y0 - y2, mirror), 0, -1)
    b2 = np.where(_owner(x1 - x0, y1 - y0, mirror), 0, -1)
    minx, maxx = np.minimum(np.minimum(x0, x1), x2), np.maximum(np.maximum(x0, x1), x2)
    miny, maxy = np.minimum(np.minimum(y0, y1), y2), np.maximum(np.maximum(y0, y1), y2)
    i0, i1 = np.maximum((minx - 8 + 15) >> 4, 0), np.minimum((maxx - 8) >> 4, ow - 1)
    j0, j1 = np.maximum((miny - 8 + 15) >> 4, 0), np.minimum((maxy - 8) >> 4, oh - 1)
    nonempty = drawn & (i0 <= i1) & (j0 <= j1)
    # the strips' cooperative queue: triangles whose box clipped to the strip exceeds BIG_CELLS cells
    nstrips = (oh + STRIP_ROWS - 1) // STRIP_ROWS
    big = np.zeros(nstrips, np.int64)
    for s in range(nstrips):
        r0, r1 = s * STRIP_ROWS, min(oh, (s + 1) * STRIP_ROWS) - 1
        a, b = np.maximum(j0, r0), np.minimum(j1, r1)
        big[s] = int((nonempty & (a <= b) & ((i1 - i0 + 1) * (b - a + 1) > BIG_CELLS)).sum())
    if variant == "bbox_outward":
        i0, i1, j0, j1 = i0 - 1, i1 + 1, j0 - 1, j1 + 1
    bw, bh = i1 - i0 + 1, j1 - j0 + 1
    cells = np.where(nonempty, bw * bh, 0)
    zb = np.full(oh * ow, EMPTY, np.uint64)
    ids = np.nonzero(cells > 0)[0]
    start = 0
    while start < len(ids):
        csum = np.cumsum(cells[ids[start:]])
        n = max(1, int(np.searchsorted(csum, chunk_cells, side="right")))
        sel = ids[start:start + n]
        start += n
        cnt = cells[sel]
        tri = np.repeat(sel, cnt)
        k = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        i = i0[tri] + k % bw[tri]
        j = j0[tri] + k // bw[tri]
        px, py = 16 * i + 8, 16 * j + 8
        e0 = (x2[tri] - x1[tri]) * (py - y1[tri]) - (y2[tri] - y1[tri]) * (px - x1[tri])
        e1 = (x0[tri] - x2[tri]) * (py - y2[tri]) - (y0[tri] - y2[tri]) * (px - x2[tri])
        e2 = (x1[tri] - x0[tri]) * (py - y0[tri]) - (y1[tri] - y0[tri]) * (px - x0[tri])
        inside = ((e0 + b0[tri]) >= 0) & ((e1 + b1[tri]) >= 0) & ((e2 + b2[tri]) >= 0)
        flat = j * ow + i
        inside &= (flat >= 0) & (flat < oh * ow)
        tri, e0, e1, e2, flat = tri[inside], e0[inside], e1[inside], e2[inside], flat[inside]
        assert variant is not None or max(np.abs(e0).max(initial=0), np.abs(e1).max(initial=0), np.abs(e2).max(initial=0)) < 2 ** 31, "edge function leaves int32"
        with np.errstate(all="ignore"):
            S = fmaf(e2.astype(F), w2i[tri], fmaf(e1.astype(F), w1i[tri], e0.astype(F) * w0i[tri]))
            z = area2[tri].astype(F) / S
            zq = np.rint(np.fmin(z, ZMAX) * ZSCALE)
        zq = np.where(np.isfinite(zq) & (zq >= 0), zq, 0).astype(np.uint64)   # a NaN / negative z converts to 0 on every side
        low = (np.uint64(0xFFFFFFFF) - tri.astype(np.uint64)) if variant == "tie_high_id" else tri.astype(np.uint64)
        np.minimum.at(zb, flat, (zq << np.uint64(32)) | low)
    covered = zb != EMPTY
    low = (zb & np.uint64(0xFFFFFFFF)).astype(np.int64)
    if variant == "tie_high_id":
        low = 0xFFFFFFFF - low
    tri_id = np.where(covered, low, -1).astype(np.int32).reshape(oh, ow)
    zbuf = np.where(covered, zb >> np.uint64(32), np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(oh, ow)
    assert variant is not None or int(area2.max(initial=0)) < 2 ** 31
    return dict(tri_id=tri_id, zbuf=zbuf, valid=ok, drawn=drawn, zero_area=zero_area, big_per_strip=big)
