// What a ray hits first on a triangle mesh (fp_mesh_ray_cast; the definition, down to the float32 operation, is in include/fp_amd.h):
// brute force over every (ray, triangle) pair, Moeller-Trumbore on the operands mesh_closest.h's LDS tile already holds (a, b - a,
// c - a).  Three launches on the caller's stream, no allocation, no synchronisation, integer atomics only:
//   k_ray_init    every key = "no triangle answered yet"
//   k_ray_scan    grid (tile of kThreads rays, chunk of faces, mesh_scan.h: chunk_faces): a lane holds its ray (o, d) in registers and
//                 the chunk's triangles pass through LDS by mesh_closest.h's scan_chunk -- the one tiling loop of the mesh queries,
//                 here with a ray for its query: the candidate of a triangle is its t, or NaN when the ray does not hit it.  The lane
//                 keeps the smallest (t, face) of its chunk and merges it into its key with one 64-bit atomic minimum (t >= +0: floats
//                 >= 0 order as their bits do).
//   k_ray_finish  one lane per ray: t and face from the key, bary and hit recomputed for the winning face with the same function (the
//                 same operations on the same operands: the same bits).
// A minimum commutes exactly, so the outputs have one value whatever the chunking and the arrival order.  Compiled with
// -ffp-contract=off (SRCS_EXACT): the numpy restatement (tests/mesh_ray_model.py) computes the same bits.
#include "mesh_scan.h"

namespace {

using namespace mesh_closest;

constexpr int kThreads = 256;   // rays per workgroup, one per lane
using mesh_scan::kTile;
static_assert(kTile == kThreads, "a tile is staged by one pass of the workgroup");

// which sides of a face answer, and the range of t that does: uniform over a launch
struct RayRange {
  float t_min, t_max;
  int cull;   // 0 both sides, 1 det > 0 only, 2 det < 0 only
};

// Moeller-Trumbore for the ray o + t d and the triangle (a, a + ab, a + ac): t, or NaN when the ray does not hit.  U, V, D are left
// for the finish (bary = (U / D, V / D)); the scan drops them.  Every comparison is false for a NaN, so nothing non-finite answers.
__device__ __forceinline__ float ray_triangle(const v3& o, const v3& d, const v3& a, const v3& ab, const v3& ac, const RayRange& r,
                                              float& U, float& V, float& D) {
  const v3 pvec = cross(d, ac);
  const float det = dot(ab, pvec);
  const v3 tvec = sub(o, a);
  const float un = dot(tvec, pvec);
  const v3 qvec = cross(tvec, ab);
  const float vn = dot(d, qvec);
  const float tn = dot(ac, qvec);
  const bool neg = det < 0.f;   // s = -1: the sign changes are exact
  D = __builtin_fabsf(det);
  U = neg ? -un : un;
  V = neg ? -vn : vn;
  const float T = neg ? -tn : tn;
  const float q = T / D;
  const float t = q == 0.f ? 0.f : q;   // a hit at -0 is recorded as +0: the key needs non-negative bits
  const bool side = r.cull == 0 || (r.cull == 1 ? det > 0.f : neg);
  const bool hit = D > 0.f && U >= 0.f && V >= 0.f && (U + V) <= D && t >= r.t_min && t <= r.t_max && t <= 3.402823466e+38f && side;
  return hit ? t : __builtin_nanf("");
}

// the ray a lane of the scan holds: scan_chunk's query type
struct RayQuery {
  v3 o, d;
  RayRange r;
  __device__ __forceinline__ float candidate(const float4* __restrict__ tile, int k) const {
    const float4 t0 = tile[k * kTileFloat4 + 0], t2 = tile[k * kTileFloat4 + 2], t3 = tile[k * kTileFloat4 + 3];
    float U, V, D;
    return ray_triangle(o, d, v3{t0.x, t0.y, t0.z}, v3{t2.y, t2.z, t2.w}, v3{t3.x, t3.y, t3.z}, r, U, V, D);
  }
};

__global__ __launch_bounds__(kThreads) void k_ray_init(unsigned long long* __restrict__ keys, int R) {
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n < R) keys[n] = kNoAnswer;
}

__global__ __launch_bounds__(kThreads) void k_ray_scan(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int F,
                                                       const float* __restrict__ origins, const float* __restrict__ dirs, int R,
                                                       RayRange range, int chunk, unsigned long long* __restrict__ keys) {
  __shared__ float4 tile[kTile * kTileFloat4];
  const int tid = threadIdx.x;
  const int n = blockIdx.x * kThreads + tid;
  const bool live = n < R;
  const size_t at = (size_t)(live ? n : R - 1) * 3;   // a lane past the end scans too: it takes part in the barriers
  const RayQuery q{load3(origins + at), load3(dirs + at), range};
  const int f0 = blockIdx.y * chunk;                  // < F <= 2^30: no overflow in f0 + chunk
  const int f1 = min(F, f0 + chunk);
  float best = __builtin_inff();
  int best_f = -1;
  scan_chunk<kTile>(q, tile, pos, Nv, faces, f0, f1, tid, best, best_f);
  if (live && best_f >= 0) merge_answer(keys + n, best, best_f);
}

__global__ __launch_bounds__(kThreads) void k_ray_finish(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces,
                                                         const float* __restrict__ origins, const float* __restrict__ dirs, int R,
                                                         RayRange range, const unsigned long long* __restrict__ keys,
                                                         float* __restrict__ t, int32_t* __restrict__ face, float* __restrict__ bary,
                                                         float* __restrict__ hit) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= R) return;
  const Nearest r = nearest_of(keys[i]);
  t[i] = r.dd;
  if (face) face[i] = r.f;
  if (!bary && !hit) return;
  const float nan = __builtin_nanf("");
  float u = nan, v = nan;
  v3 h{nan, nan, nan};
  if (!r.none) {
    const v3 o = load3(origins + (size_t)i * 3), d = load3(dirs + (size_t)i * 3);
    v3 a, b, c;
    face_vertices(pos, Nv, faces, r.f, a, b, c);
    float U, V, D;
    const float tt = ray_triangle(o, d, a, sub(b, a), sub(c, a), range, U, V, D);   // = r.dd: the same operations
    u = U / D;
    v = V / D;
    h = v3{o.x + tt * d.x, o.y + tt * d.y, o.z + tt * d.z};
  }
  if (bary) {
    bary[(size_t)i * 2] = u;
    bary[(size_t)i * 2 + 1] = v;
  }
  if (hit) {
    hit[(size_t)i * 3] = h.x;
    hit[(size_t)i * 3 + 1] = h.y;
    hit[(size_t)i * 3 + 2] = h.z;
  }
}

}  // namespace

extern "C" size_t fp_mesh_ray_cast_workspace_bytes(int R) { return R > 0 ? (size_t)R * sizeof(unsigned long long) : 0; }

extern "C" int fp_mesh_ray_cast(const float* pos, int Nv, const int32_t* faces, int F, const float* origins, const float* dirs, int R,
                                float t_min, float t_max, int cull, float* t, int32_t* face, float* bary, float* hit, void* workspace,
                                size_t workspace_bytes, void* stream) {
  const char* name = "fp_mesh_ray_cast";
  FP_REQUIRE(R >= 0 && R <= (1 << 30), "%s: R=%d outside 0..2^30", name, R);
  FP_REQUIRE(F >= 0 && F <= (1 << 30), "%s: F=%d outside 0..2^30", name, F);
  FP_REQUIRE(Nv >= 0, "%s: Nv=%d is negative", name, Nv);
  FP_REQUIRE(t_min >= 0.f && t_min <= t_max, "%s: t_min=%g, t_max=%g: 0 <= t_min <= t_max is required", name, (double)t_min,
             (double)t_max);
  FP_REQUIRE(cull >= 0 && cull <= 2, "%s: cull=%d outside 0..2", name, cull);
  if (R == 0) return FP_OK;
  FP_REQUIRE(origins && dirs && t, "%s: NULL origins, dirs or t", name);
  if (int st = mesh_scan::check_mesh(name, true, pos, Nv, faces, F)) return st;
  if (int st = mesh_scan::check_workspace(name, workspace, workspace_bytes, fp_mesh_ray_cast_workspace_bytes(R), 8,
                                          "fp_mesh_ray_cast_workspace_bytes"))
    return st;
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  const RayRange range{t_min, t_max, cull};
  const int tiles = fp_cdiv(R, kThreads);
  hipLaunchKernelGGL(k_ray_init, dim3(tiles), dim3(kThreads), 0, st, keys, R);
  if (int e = mesh_scan::launched(name, "init")) return e;
  if (F > 0) {
    const int chunk = mesh_scan::chunk_faces(tiles, F);
    hipLaunchKernelGGL(k_ray_scan, dim3(tiles, fp_cdiv(F, chunk)), dim3(kThreads), 0, st, pos, Nv, faces, F, origins, dirs, R, range,
                       chunk, keys);
    if (int e = mesh_scan::launched(name, "scan")) return e;
  }
  hipLaunchKernelGGL(k_ray_finish, dim3(fp_cdiv(R, kThreads)), dim3(kThreads), 0, st, pos, Nv, faces, origins, dirs, R, range, keys, t,
                     face, bary, hit);
  return mesh_scan::launched(name, "finish");
}
