// What the mesh-query entry points (mesh_distance.hip, mesh_signed.hip, mesh_icp.hip, mesh_symmetry.hip) share on the host: the
// checks of the arguments they have in common, and mesh_scan.hip's "nearest face of every query" launches.
#pragma once
#include "fp_common.h"
#include "mesh_grid.h"

namespace mesh_scan {

// the two sizes of mesh_scan.hip's tiling that show outside it: mesh_distance.hip states them for the tests, which put their cases
// on these boundaries
constexpr int kTile = 256;        // triangles per LDS tile: 4 float4 each, 16 KiB: 8 workgroups of 4 waves a CU
constexpr int kChunkMin = 1024;   // the fewest faces a workgroup scans (unless the mesh has fewer)
constexpr int kFillWorkgroups = 2048;  // workgroups wanted in flight (256 CUs x 8 of 4 waves)
static_assert(kChunkMin % kTile == 0, "a chunk is whole tiles");

// faces per chunk for a grid of `tiles` lane tiles (mesh_scan.hip's scans and mesh_ray.hip's): a multiple of kTile, at least
// kChunkMin, and no smaller than what gives about kFillWorkgroups workgroups
inline int chunk_faces(int tiles, int F) {
  const int want = tiles >= kFillWorkgroups ? 1 : fp_cdiv(kFillWorkgroups, tiles);   // chunks wanted
  int chunk = fp_cdiv(F > 0 ? F : 1, want);
  if (chunk < kChunkMin) chunk = kChunkMin;
  return fp_cdiv(chunk, kTile) * kTile;
}

// ---- mesh_scan.hip.  Each issues the init launch and, if F > 0, the scan launch on `st`, and reports a failure as "<name> (init)" or
// "<name> (scan)".  n = Q queries (points) or T * Q pairs numbered t * Q + i (pairs: p = transformed(tfs + 16 t, points[i])), n > 0.
// keys[n] is left as (bits(dd) << 32) | face of the nearest face, the smaller face on a tie, or all ones (mesh_closest.h: nearest_of);
// grid: NULL scans every face, a checked grid (mesh_grid::check_grid) walks its shells instead: the same keys.
int nearest_face_of_points(const char* name, const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid,
                           const float* points, int Q, unsigned long long* keys, hipStream_t st);
int nearest_face_of_pairs(const char* name, const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid,
                          const float* points, int Q, const float* tfs, int T, unsigned long long* keys, hipStream_t st);
// cell[n] is left as bits(dd) of the nearest face, or the bits of +inf
int nearest_dist2_of_pairs(const char* name, const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid,
                           const float* points, int Q, const float* tfs, int T, unsigned* cell, hipStream_t st);

// FP_CHECK_LAUNCH with the entry point's name at run time: a failed launch is reported as "<name> (<step>) launch failed: ..."
static inline int launched(const char* name, const char* step) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return FP_OK;
  fp_set_error("%s (%s) launch failed: %s", name, step, hipGetErrorString(e));
  return FP_ERR_LAUNCH;
}

// ---- The arguments the entry points have in common, checked once.  `name` is the entry point's; the caller does
// `if (int st = check_...(name, ...)) return st;` and puts the checks of its own arguments where they have always been.

// the mesh of a call with something to scan (live: Q > 0)
static inline int check_mesh(const char* name, bool live, const float* pos, int Nv, const int32_t* faces, int F) {
  FP_REQUIRE(!live || F == 0 || faces, "%s: faces is NULL but F=%d", name, F);
  FP_REQUIRE(!live || F == 0 || Nv == 0 || pos, "%s: pos is NULL but Nv=%d", name, Nv);
  return FP_OK;
}

// A "points" call, up to its workspace: the sizes, the grid of a call that takes one (gridded), and for Q > 0 the pointers.  Q == 0
// passes whatever the pointers are: the caller returns FP_OK then.
static inline int check_points(const char* name, const float* pos, int Nv, const int32_t* faces, int F, bool gridded,
                               const fp_mesh_grid* grid, const float* points, int Q, const float* dist2) {
  FP_REQUIRE(Q >= 0 && Q <= (1 << 30), "%s: Q=%d outside 0..2^30", name, Q);
  FP_REQUIRE(F >= 0 && F <= (1 << 30), "%s: F=%d outside 0..2^30", name, F);
  FP_REQUIRE(Nv >= 0, "%s: Nv=%d is negative", name, Nv);
  if (gridded)
    if (int st = mesh_grid::check_grid(name, grid)) return st;
  if (Q == 0) return FP_OK;
  FP_REQUIRE(points && dist2, "%s: NULL points or dist2", name);
  return check_mesh(name, true, pos, Nv, faces, F);
}

// the sizes of a "pairs" call and the grid of one that takes one (gridded); the caller returns FP_OK at T == 0 once its own values
// are checked, then checks its pointers and check_mesh
static inline int check_pairs(const char* name, int T, int Q, int F, int Nv, bool gridded, const fp_mesh_grid* grid) {
  FP_REQUIRE(T >= 0 && Q >= 0, "%s: T=%d or Q=%d is negative", name, T, Q);
  FP_REQUIRE((long long)T * (long long)Q <= (1ll << 30) && T <= (1 << 30), "%s: T=%d times Q=%d is above 2^30", name, T, Q);
  FP_REQUIRE(F >= 0 && F <= (1 << 30), "%s: F=%d outside 0..2^30", name, F);
  FP_REQUIRE(Nv >= 0, "%s: Nv=%d is negative", name, Nv);
  if (gridded)
    if (int st = mesh_grid::check_grid(name, grid)) return st;
  return FP_OK;
}

// the workspace of either: `need` bytes (0: none is read) aligned to `align`, as `bytes_fn` tells the caller
static inline int check_workspace(const char* name, const void* workspace, size_t workspace_bytes, size_t need, unsigned align,
                                  const char* bytes_fn) {
  FP_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & (align - 1)) == 0),
             "%s: workspace too small or not %u-byte aligned (%zu < %zu bytes, see %s)", name, align, workspace_bytes, need, bytes_fn);
  return FP_OK;
}

}  // namespace mesh_scan
