// The exact distance from Q points to the surface of a triangle mesh (fp_mesh_point_distance; the definition, down to the float32
// operation, is in include/fp_amd.h): brute force over every (query, triangle) pair.  Three launches on the caller's stream, no
// allocation, no synchronisation, integer atomics only:
//   init, scan   mesh_scan.hip's nearest_face_of_points: keys[i] = the smallest (bits(dd) << 32) | face over the mesh's triangles, or
//                all ones when no triangle answers query i
//   k_md_finish  one lane per query: dist2 and face from the key, closest recomputed for the winning face with the same function
//                (the same operations on the same operands: the same bits).
// A minimum commutes exactly, so the outputs have one value whatever the chunking and the arrival order.  Compiled with
// -ffp-contract=off (SRCS_EXACT): the numpy restatement (tests/mesh_distance_model.py) computes the same bits.
// fp_mesh_grid_point_distance is the same call with a grid: the scan then walks the shells of a uniform grid around each query instead
// (mesh_grid.h: the walk and why it skips no triangle that could win or tie); the keys are the interface, so every output is made by
// k_md_finish as above.
#include "mesh_scan.h"

namespace {

using namespace mesh_closest;

constexpr int kThreads = 256;   // queries per workgroup of the finish, one per lane

// The scan's tile and smallest chunk, stated here as literals because tests/mesh_distance_model.py reads them from this file to put
// its cases on the tile and chunk boundaries; mesh_scan.h has the values the scan is built with.
constexpr int kTile = 256;
constexpr int kChunkMin = 1024;
static_assert(kTile == mesh_scan::kTile && kChunkMin == mesh_scan::kChunkMin, "the sizes the tests read are the scan's");

__global__ __launch_bounds__(kThreads) void k_md_finish(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces,
                                                        const float* __restrict__ points, int Q,
                                                        const unsigned long long* __restrict__ keys, float* __restrict__ dist2,
                                                        int32_t* __restrict__ face, float* __restrict__ closest) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= Q) return;
  const Nearest r = nearest_of(keys[i]);
  dist2[i] = r.dd;
  if (face) face[i] = r.f;
  if (closest) {
    v3 q{0.f, 0.f, 0.f};
    if (!r.none) {
      v3 a, b, c;
      face_vertices(pos, Nv, faces, r.f, a, b, c);
      closest_point(load3(points + (size_t)i * 3), a, b, c, sub(b, a), sub(c, a), q);
    }
    closest[(size_t)i * 3] = q.x;
    closest[(size_t)i * 3 + 1] = q.y;
    closest[(size_t)i * 3 + 2] = q.z;
  }
}

// fp_mesh_point_distance (gridded: no) and fp_mesh_grid_point_distance (gridded: yes) are one call, the scan exchanged
int point_distance(const char* name, bool gridded, const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid,
                   const float* points, int Q, float* dist2, int32_t* face, float* closest, void* workspace, size_t workspace_bytes,
                   void* stream) {
  if (int st = mesh_scan::check_points(name, pos, Nv, faces, F, gridded, grid, points, Q, dist2)) return st;
  if (Q == 0) return FP_OK;
  if (int st = mesh_scan::check_workspace(name, workspace, workspace_bytes, fp_mesh_point_distance_workspace_bytes(Q), 8,
                                          "fp_mesh_point_distance_workspace_bytes"))
    return st;
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  if (int e = mesh_scan::nearest_face_of_points(name, pos, Nv, faces, F, gridded ? grid : nullptr, points, Q, keys, st)) return e;
  hipLaunchKernelGGL(k_md_finish, dim3(fp_cdiv(Q, kThreads)), dim3(kThreads), 0, st, pos, Nv, faces, points, Q, keys, dist2, face, closest);
  return mesh_scan::launched(name, "finish");
}

}  // namespace

extern "C" size_t fp_mesh_point_distance_workspace_bytes(int Q) { return Q > 0 ? (size_t)Q * sizeof(unsigned long long) : 0; }

extern "C" int fp_mesh_point_distance(const float* pos, int Nv, const int32_t* faces, int F, const float* points, int Q, float* dist2,
                                      int32_t* face, float* closest, void* workspace, size_t workspace_bytes, void* stream) {
  return point_distance("fp_mesh_point_distance", false, pos, Nv, faces, F, nullptr, points, Q, dist2, face, closest, workspace,
                        workspace_bytes, stream);
}

extern "C" int fp_mesh_grid_point_distance(const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid,
                                           const float* points, int Q, float* dist2, int32_t* face, float* closest, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  return point_distance("fp_mesh_grid_point_distance", true, pos, Nv, faces, F, grid, points, Q, dist2, face, closest, workspace,
                        workspace_bytes, stream);
}
