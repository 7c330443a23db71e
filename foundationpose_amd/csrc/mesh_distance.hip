// The exact distance from Q points to the surface of a triangle mesh (fp_mesh_point_distance; the definition, down to the float32
// operation, is in include/fp_amd.h): brute force over every (query, triangle) pair.  Three launches on the caller's stream, no
// allocation, no synchronisation, integer atomics only:
//   k_md_init    keys[i] = all ones ("no triangle answered yet")
//   k_md_scan    grid (tile of kThreads queries, chunk of faces): a lane owns one query in registers.  The chunk's triangles pass
//                through LDS in tiles of kTile (mesh_closest.h: staging and the closest-point walk, shared with
//                mesh_symmetry.hip): the lane that stages a triangle reads its three indices, checks them against Nv (a
//                triangle with an index outside the table is staged as NaN and so never counts: nothing of pos is read for it) and
//                writes a, b, c, b - a and c - a, the two differences being the definition's own float32 operations done once per
//                triangle instead of once per pair.  Every lane then reads the same triangle (one address: an LDS broadcast, no bank
//                conflict) and walks the regions: the source evaluates the seven region tests in the book's order on selects, and
//                the one quotient the chosen region needs is the only division executed (the compiler turns some of the selects
//                into short exec-masked regions, skipped when no lane of the wave needs them; the values are the same).  The lane
//                keeps the smallest (dd, face) of its chunk -- faces ascend, so `<` keeps the smaller index on a tie -- and merges
//                it into keys[i] with one 64-bit atomic minimum on (bits(dd) << 32) | face: floats >= 0 order as their bits do.
//   k_md_finish  one lane per query: dist2 and face from the key, closest recomputed for the winning face with the same function
//                (the same operations on the same operands: the same bits).
// A minimum commutes exactly, so the outputs have one value whatever the chunking and the arrival order: how the faces are cut into
// chunks depends on Q and F only to fill the chip and never shows in a result.  Compiled with -ffp-contract=off (SRCS_EXACT): the
// numpy restatement (tests/mesh_distance_model.py) computes the same bits.
// fp_mesh_grid_point_distance is the same init and finish around k_md_grid_scan, where a lane walks the shells of a uniform grid around
// its query instead (mesh_grid.h: the walk and why it skips no triangle that could win or tie); the keys are the interface, so every
// output is made by k_md_finish as above.
#include <float.h>
#include "fp_common.h"
#include "mesh_closest.h"
#include "mesh_grid.h"

namespace {

using namespace mesh_closest;   // v3, closest_point, face_vertices and the tile staging: shared with mesh_symmetry.hip

constexpr int kThreads = 256;          // queries per workgroup, one per lane
constexpr int kTile = 256;             // triangles per LDS tile: 4 float4 each, 16 KiB
constexpr int kChunkMin = 1024;        // the fewest faces a workgroup scans (unless the mesh has fewer)
constexpr int kFillWorkgroups = 2048;  // workgroups wanted in flight (256 CUs x 8 of 4 waves)

static_assert(kChunkMin % kTile == 0, "a chunk is whole tiles");
static_assert(kTile == kThreads, "a tile is staged by one pass of the workgroup");

// faces per chunk: a multiple of kTile, at least kChunkMin, and no smaller than what gives about kFillWorkgroups workgroups
inline int chunk_faces(int Q, int F) { return mesh_closest::chunk_faces(fp_cdiv(Q, kThreads), F, kTile, kChunkMin, kFillWorkgroups); }

__global__ __launch_bounds__(kThreads) void k_md_init(unsigned long long* __restrict__ keys, int Q) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < Q) keys[i] = kNoAnswer;
}

__global__ __launch_bounds__(kThreads) void k_md_scan(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int F,
                                                      const float* __restrict__ points, int Q, int chunk,
                                                      unsigned long long* __restrict__ keys) {
  __shared__ float4 tile[kTile * kTileFloat4];   // per triangle: (a, b.x) (b.yz, c.xy) (c.z, ab) (ac, -)
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kThreads + tid;
  const bool live = i < Q;
  const v3 p = load3(points + (size_t)(live ? i : Q - 1) * 3);
  const int f0 = blockIdx.y * chunk;                  // < F <= 2^30: no overflow in f0 + chunk
  const int f1 = min(F, f0 + chunk);
  float best = __builtin_inff();
  int best_f = -1;
  scan_chunk<kTile>(p, tile, pos, Nv, faces, f0, f1, tid, best, best_f);   // mesh_closest.h: the one copy
  if (live && best_f >= 0) merge_answer(keys + i, best, best_f);
}

// fp_mesh_grid_point_distance's scan in place of k_md_scan: a lane owns one query and walks the grid's shells around it (mesh_grid.h)
__global__ __launch_bounds__(kThreads) void k_md_grid_scan(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int F,
                                                           mesh_grid::Grid g, mesh_grid::Tables t, const float* __restrict__ points,
                                                           int Q, unsigned long long* __restrict__ keys) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= Q) return;
  float best = __builtin_inff();
  int best_f = -1;
  mesh_grid::walk(g, t, pos, Nv, faces, F, load3(points + (size_t)i * 3), best, best_f);
  if (best_f >= 0) merge_answer(keys + i, best, best_f);
}

__global__ __launch_bounds__(kThreads) void k_md_finish(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces,
                                                        const float* __restrict__ points, int Q,
                                                        const unsigned long long* __restrict__ keys, float* __restrict__ dist2,
                                                        int32_t* __restrict__ face, float* __restrict__ closest) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= Q) return;
  const unsigned long long key = keys[i];
  const bool none = key == kNoAnswer;
  const int f = none ? -1 : (int)(unsigned)(key & 0xffffffffull);
  dist2[i] = none ? __builtin_inff() : __uint_as_float((unsigned)(key >> 32));
  if (face) face[i] = f;
  if (closest) {
    v3 q{0.f, 0.f, 0.f};
    if (!none) {
      v3 a, b, c;
      face_vertices(pos, Nv, faces, f, a, b, c);
      closest_point(load3(points + (size_t)i * 3), a, b, c, sub(b, a), sub(c, a), q);
    }
    closest[(size_t)i * 3] = q.x;
    closest[(size_t)i * 3 + 1] = q.y;
    closest[(size_t)i * 3 + 2] = q.z;
  }
}

}  // namespace

extern "C" size_t fp_mesh_point_distance_workspace_bytes(int Q) { return Q > 0 ? (size_t)Q * sizeof(unsigned long long) : 0; }

extern "C" int fp_mesh_point_distance(const float* pos, int Nv, const int32_t* faces, int F, const float* points, int Q, float* dist2,
                                      int32_t* face, float* closest, void* workspace, size_t workspace_bytes, void* stream) {
  FP_REQUIRE(Q >= 0 && Q <= (1 << 30), "fp_mesh_point_distance: Q=%d outside 0..2^30", Q);
  FP_REQUIRE(F >= 0 && F <= (1 << 30), "fp_mesh_point_distance: F=%d outside 0..2^30", F);
  FP_REQUIRE(Nv >= 0, "fp_mesh_point_distance: Nv=%d is negative", Nv);
  if (Q == 0) return FP_OK;
  FP_REQUIRE(points && dist2, "fp_mesh_point_distance: NULL points or dist2");
  FP_REQUIRE(F == 0 || faces, "fp_mesh_point_distance: faces is NULL but F=%d", F);
  FP_REQUIRE(F == 0 || Nv == 0 || pos, "fp_mesh_point_distance: pos is NULL but Nv=%d", Nv);
  const size_t need = fp_mesh_point_distance_workspace_bytes(Q);
  FP_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0,
             "fp_mesh_point_distance: workspace too small or not 8-byte aligned (%zu < %zu bytes, see "
             "fp_mesh_point_distance_workspace_bytes)", workspace_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  const int qtiles = fp_cdiv(Q, kThreads);
  hipLaunchKernelGGL(k_md_init, dim3(qtiles), dim3(kThreads), 0, st, keys, Q);
  FP_CHECK_LAUNCH("fp_mesh_point_distance (init)");
  if (F > 0) {
    const int chunk = chunk_faces(Q, F);
    hipLaunchKernelGGL(k_md_scan, dim3(qtiles, fp_cdiv(F, chunk)), dim3(kThreads), 0, st, pos, Nv, faces, F, points, Q, chunk, keys);
    FP_CHECK_LAUNCH("fp_mesh_point_distance (scan)");
  }
  hipLaunchKernelGGL(k_md_finish, dim3(qtiles), dim3(kThreads), 0, st, pos, Nv, faces, points, Q, keys, dist2, face, closest);
  FP_CHECK_LAUNCH("fp_mesh_point_distance (finish)");
  return FP_OK;
}

extern "C" int fp_mesh_grid_point_distance(const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid,
                                           const float* points, int Q, float* dist2, int32_t* face, float* closest, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  const char* name = "fp_mesh_grid_point_distance";
  FP_REQUIRE(Q >= 0 && Q <= (1 << 30), "%s: Q=%d outside 0..2^30", name, Q);
  FP_REQUIRE(F >= 0 && F <= (1 << 30), "%s: F=%d outside 0..2^30", name, F);
  FP_REQUIRE(Nv >= 0, "%s: Nv=%d is negative", name, Nv);
  if (int st = mesh_grid::check_grid(name, grid)) return st;
  if (Q == 0) return FP_OK;
  FP_REQUIRE(points && dist2, "%s: NULL points or dist2", name);
  FP_REQUIRE(F == 0 || faces, "%s: faces is NULL but F=%d", name, F);
  FP_REQUIRE(F == 0 || Nv == 0 || pos, "%s: pos is NULL but Nv=%d", name, Nv);
  const size_t need = fp_mesh_point_distance_workspace_bytes(Q);
  FP_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0,
             "%s: workspace too small or not 8-byte aligned (%zu < %zu bytes, see fp_mesh_point_distance_workspace_bytes)", name,
             workspace_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  const int qtiles = fp_cdiv(Q, kThreads);
  hipLaunchKernelGGL(k_md_init, dim3(qtiles), dim3(kThreads), 0, st, keys, Q);
  FP_CHECK_LAUNCH("fp_mesh_grid_point_distance (init)");
  if (F > 0) {
    hipLaunchKernelGGL(k_md_grid_scan, dim3(qtiles), dim3(kThreads), 0, st, pos, Nv, faces, F, mesh_grid::device_grid(grid),
                       mesh_grid::device_tables(grid), points, Q, keys);
    FP_CHECK_LAUNCH("fp_mesh_grid_point_distance (scan)");
  }
  hipLaunchKernelGGL(k_md_finish, dim3(qtiles), dim3(kThreads), 0, st, pos, Nv, faces, points, Q, keys, dist2, face, closest);
  FP_CHECK_LAUNCH("fp_mesh_grid_point_distance (finish)");
  return FP_OK;
}
