// A uniform grid over a mesh's triangles and the walk that answers a closest-point query from it: the one copy that mesh_grid.hip (the
// build: fp_mesh_grid_count, fp_mesh_grid_fill) and mesh_scan.hip (the scan of fp_mesh_grid_point_distance,
// fp_mesh_grid_signed_distance, fp_mesh_grid_transform_residuals, fp_mesh_grid_icp_step and fp_mesh_grid_penetration) share.  The
// definition -- the cell of a coordinate, the three classes of a triangle, the shells, the stop rule and why a skipped triangle can
// neither win nor tie -- is in include/fp_amd.h.  Every pair test is mesh_closest.h's
// closest_point on a, b, c, b - a, c - a, the operations the brute-force staging performs, so a (query, triangle) pair has the same dd
// here as there; the files are compiled with -ffp-contract=off (SRCS_EXACT), which also keeps lo + (float)i * h two roundings.
#pragma once
#include <float.h>
#include <math.h>
#include "fp_common.h"
#include "mesh_closest.h"

namespace mesh_grid {

using namespace mesh_closest;

constexpr int kMaxCells = 1 << 21;             // cells of a grid
constexpr int kMaxCellsPerTriangle = 4096;     // a stored triangle's padded box covers at most so many; a larger one goes to the overflow list
constexpr float kMinPadOverM = 0x1p-20f;       // pad >= 2^-20 * M (include/fp_amd.h: the error terms of the stop rule stay under pad / 2)
constexpr float kMinCell = 0x1p-100f, kMaxCell = 0x1p100f;   // h within these: 1 / h is a normal float32

enum Class { kDropped = 0, kOverflow = 1, kStored = 2 };
// header[]: what fp_mesh_grid_count and fp_mesh_grid_fill leave on the device
enum Header { kEntries = 0, kOverflowCount = 1, kStatus = 2, kHeaderInts = 4 };
enum Status { kEntriesTooSmall = 1, kOverflowTooSmall = 2, kTooManyEntries = 4 };

// the grid as the kernels take it (by value)
struct Grid {
  float lo[3];
  float h, inv_h, pad;
  int n[3];
};

__host__ __device__ __forceinline__ bool finite(float x) { return fabsf(x) <= FLT_MAX; }
__host__ __device__ __forceinline__ bool finite3(const v3& a) { return finite(a.x) && finite(a.y) && finite(a.z); }

// cell of x on axis k: clamp(floorf((x - lo_k) * inv_h), 0, n_k - 1), clamped in float before the conversion (x = 1e30 must not overflow it)
__device__ __forceinline__ int cell_of(const Grid& g, int k, float x) {
  float t = floorf((x - g.lo[k]) * g.inv_h);
  const float top = (float)(g.n[k] - 1);
  t = t > 0.f ? t : 0.f;           // a NaN lands in cell 0 (no caller passes one)
  t = t < top ? t : top;
  return (int)t;
}

__device__ __forceinline__ float min3(float a, float b, float c) { const float m = a < b ? a : b; return m < c ? m : c; }
__device__ __forceinline__ float max3(float a, float b, float c) { const float m = a > b ? a : b; return m > c ? m : c; }

// The class of triangle f and, for a stored one, its cells i0[k]..i1[k]: the one decision that count and fill both make.
__device__ __forceinline__ int classify(const Grid& g, const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int f,
                                        int i0[3], int i1[3]) {
  const int v0 = faces[(size_t)f * 3], v1 = faces[(size_t)f * 3 + 1], v2 = faces[(size_t)f * 3 + 2];
  if (!((unsigned)v0 < (unsigned)Nv && (unsigned)v1 < (unsigned)Nv && (unsigned)v2 < (unsigned)Nv)) return kDropped;
  const v3 a = load3(pos + (size_t)v0 * 3), b = load3(pos + (size_t)v1 * 3), c = load3(pos + (size_t)v2 * 3);
  if (!(finite3(a) && finite3(b) && finite3(c))) return kOverflow;
  const float tmin[3] = {min3(a.x, b.x, c.x), min3(a.y, b.y, c.y), min3(a.z, b.z, c.z)};
  const float tmax[3] = {max3(a.x, b.x, c.x), max3(a.y, b.y, c.y), max3(a.z, b.z, c.z)};
  int cells = 1;                                    // <= n0 * n1 * n2 <= kMaxCells: no overflow
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    i0[k] = cell_of(g, k, tmin[k] - g.pad);
    i1[k] = cell_of(g, k, tmax[k] + g.pad);
    cells *= i1[k] - i0[k] + 1;
  }
  return cells > kMaxCellsPerTriangle ? kOverflow : kStored;
}

// one pair test: the smaller (dd, face) is kept by an explicit comparison -- entries do not ascend and a triangle can be met several
// times.  dd < best holds for no NaN and no +inf (best starts at +inf, best_f at -1): exactly the candidates with dd <= FLT_MAX.
__device__ __forceinline__ void test_face(const v3& p, const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int F, int f,
                                          float& best, int& best_f) {
  if ((unsigned)f >= (unsigned)F) return;          // a table that is not this mesh's reads nothing out of bounds
  v3 a, b, c, q;
  face_vertices(pos, Nv, faces, f, a, b, c);
  const float dd = closest_point(p, a, b, c, sub(b, a), sub(c, a), q);
  const bool better = dd < best || (dd == best && f < best_f);
  best = better ? dd : best;
  best_f = better ? f : best_f;
}

// the tables of a built grid as a query kernel takes them
struct Tables {
  const int32_t* cell_start;   // [ncells + 1]
  const int32_t* entries;      // [n_entries]
  const int32_t* overflow;     // [n_overflow]
  int n_entries, n_overflow;
};

// The walk of one lane for its query p (include/fp_amd.h): the shells r = 0, 1, 2, ... of Chebyshev distance r around p's cell, clipped
// to the grid, until the nearest plane of the visited block that is not the grid's end is farther than the best found (strictly), then
// the overflow list.  A non-finite p answers nothing and walks nothing.  best / best_f come in as +inf / -1.
__device__ __forceinline__ void walk(const Grid& g, const Tables& t, const float* __restrict__ pos, int Nv,
                                     const int32_t* __restrict__ faces, int F, const v3& p, float& best, int& best_f) {
  if (!finite3(p)) return;
  const float pk[3] = {p.x, p.y, p.z};
  int c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = cell_of(g, k, pk[k]);
  // a grid without a stored triangle has nothing to walk (every triangle is in the overflow list, or there is none)
  for (int r = 0; t.n_entries > 0; ++r) {
    const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.n[0] - 1);
    const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.n[1] - 1);
    const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.n[2] - 1);
    for (int z = z0; z <= z1; ++z) {
      const bool zface = z - c[2] == r || c[2] - z == r;
      for (int y = y0; y <= y1; ++y) {
        // a row on the shell's z or y face is visited whole, x0..x1: consecutive cells, so their entries are one run of the list and
        // two reads of cell_start serve the row.  Any other row only at x = c0 - r and x = c0 + r, where they are in the grid.
        const bool whole = zface || y - c[1] == r || c[1] - y == r;
        const int row = (z * g.n[1] + y) * g.n[0];
        for (int side = 0; side < (whole ? 1 : 2); ++side) {
          const int xa = whole ? x0 : side == 0 ? c[0] - r : c[0] + r;
          const int xb = whole ? x1 : xa;
          if (xa < x0 || xb > x1) continue;
          const int j0 = max(t.cell_start[row + xa], 0), j1 = min(t.cell_start[row + xb + 1], t.n_entries);
          for (int j = j0; j < j1; ++j) test_face(p, pos, Nv, faces, F, t.entries[j], best, best_f);
        }
      }
    }
    // the planes of the block that are not the grid's end: m = the distance from p to the nearest of them
    bool side = false;
    float m = __builtin_inff();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (c[k] + r < g.n[k] - 1) {
        const float X = g.lo[k] + (float)(c[k] + r + 1) * g.h;
        const float d = X - pk[k];
        side = true;
        m = d < m ? d : m;
      }
      if (c[k] - r > 0) {
        const float X = g.lo[k] + (float)(c[k] - r) * g.h;
        const float d = pk[k] - X;
        side = true;
        m = d < m ? d : m;
      }
    }
    if (!side || (m > 0.f && best < m * m)) break;
  }
  for (int j = 0; j < t.n_overflow; ++j) test_face(p, pos, Nv, faces, F, t.overflow[j], best, best_f);
}

// ---- the host side: one check of a caller's fp_mesh_grid for every entry point that takes one
inline long long cells_of(const fp_mesh_grid* g) { return (long long)g->n[0] * (long long)g->n[1] * (long long)g->n[2]; }

inline int check_grid(const char* name, const fp_mesh_grid* g) {
  FP_REQUIRE(g, "%s: NULL grid", name);
  FP_REQUIRE(finite(g->lo[0]) && finite(g->lo[1]) && finite(g->lo[2]) && finite(g->h) && finite(g->pad),
             "%s: the grid has a non-finite value (lo=(%g, %g, %g), h=%g, pad=%g)", name, g->lo[0], g->lo[1], g->lo[2], g->h, g->pad);
  FP_REQUIRE(g->h >= kMinCell && g->h <= kMaxCell, "%s: cell edge h=%g outside 2^-100..2^100 (it must be positive)", name, g->h);
  FP_REQUIRE(g->n[0] >= 1 && g->n[1] >= 1 && g->n[2] >= 1, "%s: grid of n=(%d, %d, %d) cells: each must be at least 1", name, g->n[0],
             g->n[1], g->n[2]);
  FP_REQUIRE(g->n[0] <= kMaxCells && g->n[1] <= kMaxCells && g->n[2] <= kMaxCells && cells_of(g) <= kMaxCells,
             "%s: grid of n=(%d, %d, %d) has more than 2^21 cells", name, g->n[0], g->n[1], g->n[2]);
  float M = 0.f;
  for (int k = 0; k < 3; ++k) {
    const float hi = g->lo[k] + (float)g->n[k] * g->h;
    M = fmaxf(M, fmaxf(fabsf(g->lo[k]), fabsf(hi)));
  }
  FP_REQUIRE(finite(M), "%s: the grid's far corner is not finite", name);
  FP_REQUIRE(g->pad >= kMinPadOverM * M, "%s: pad=%g is below 2^-20 of the grid's largest coordinate M=%g", name, g->pad, M);
  FP_REQUIRE(g->n_entries >= 0 && g->n_overflow >= 0, "%s: n_entries=%d or n_overflow=%d is negative", name, g->n_entries, g->n_overflow);
  FP_REQUIRE(g->cell_start, "%s: NULL cell_start", name);
  FP_REQUIRE(g->n_entries == 0 || g->entries, "%s: entries is NULL but n_entries=%d", name, g->n_entries);
  FP_REQUIRE(g->n_overflow == 0 || g->overflow, "%s: overflow is NULL but n_overflow=%d", name, g->n_overflow);
  return FP_OK;
}

inline Grid device_grid(const fp_mesh_grid* g) {
  return Grid{{g->lo[0], g->lo[1], g->lo[2]}, g->h, 1.f / g->h, g->pad, {g->n[0], g->n[1], g->n[2]}};
}

inline Tables device_tables(const fp_mesh_grid* g) { return Tables{g->cell_start, g->entries, g->overflow, g->n_entries, g->n_overflow}; }

}  // namespace mesh_grid
