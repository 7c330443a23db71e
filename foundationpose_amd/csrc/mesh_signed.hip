// Which side of a closed triangle mesh a point is on (fp_mesh_signed_distance), and how far T placements of Q points reach into it
// (fp_mesh_penetration); the definitions, down to the float32 operation, are in include/fp_amd.h.  The distance is the unsigned
// siblings' own: the (query, chunk of faces) scan and the closest-point walk of mesh_closest.h (one copy; the same bits as
// fp_mesh_point_distance).  The sign needs no second scan and no transcendental: the finish re-walks the winning face, learns which
// feature of it the closest point q lies on (a vertex, an edge, the interior) and takes the sign of (p - q) . n for that feature's
// angle-weighted pseudonormal n (Baerentzen and Aanaes 2005), read from the tables fp_mesh_pseudonormals made on the host (vn per
// vertex, en per face edge) or, in the interior, formed as ab x ac.
//   fp_mesh_signed_distance, three launches:
//     k_sg_init    keys[i] = all ones ("no triangle answered yet")
//     k_sd_scan    k_md_scan's grid and body: (tile of kThreads queries, chunk of faces), a lane owns one query, the triangles pass
//                  through LDS in tiles and are read by broadcast; one 64-bit atomic minimum on (bits(dd) << 32) | face per lane
//     k_sd_finish  one lane per query: dist2 and face from the key, q and the feature from the re-walk, n, the sign
//   fp_mesh_penetration, three launches:
//     k_sg_init    keys[t * Q + i] = all ones
//     k_pn_scan    k_mi_scan's pair tiling: the pairs are numbered n = t * Q + i and a lane owns one; p = ((r0*x + r1*y) + r2*z) + t
//     k_pn_finish  one workgroup per transform: each lane re-walks its pairs as k_sd_finish does, then the workgroup reduces in LDS
//                  with integer atomics only: an add for the number of points inside, a 64-bit maximum on (bits(dd) << 32) | ~i for
//                  the deepest of them (the larger dd, then the smaller i)
//   fp_mesh_grid_signed_distance: k_sg_init, k_sd_grid_scan (a lane walks the shells of a uniform grid around its query: mesh_grid.h),
//     and k_sd_finish unchanged
// A minimum, a maximum and an integer count commute exactly: every output has one value whatever the chunking and the arrival order.
// No allocation, no memset, no synchronisation.  Compiled with -ffp-contract=off (SRCS_EXACT): the numpy restatement
// (tests/mesh_signed_model.py) computes the same bits.
#include "fp_common.h"
#include "mesh_closest.h"
#include "mesh_grid.h"

namespace {

using namespace mesh_closest;

constexpr int kThreads = 256;          // queries, or (transform, point) pairs, per workgroup: one per lane
constexpr int kTile = 256;             // triangles per LDS tile: 4 float4 each, 16 KiB -- as k_md_scan: 8 workgroups of 4 waves a CU
constexpr int kChunkMin = 1024;        // the fewest faces a workgroup scans (unless the mesh has fewer)
constexpr int kFillWorkgroups = 2048;  // workgroups wanted in flight (256 CUs x 8 of 4 waves)

static_assert(kChunkMin % kTile == 0, "a chunk is whole tiles");
static_assert(kTile == kThreads, "a tile is staged by one pass of the workgroup");

// rows 0..2 of the matrix as given; ((r0*x + r1*y) + r2*z) + t, one float32 operation each, in this order (as k_ms_scan, k_mi_scan)
__device__ __forceinline__ v3 transformed(const float* __restrict__ m, const v3& x) {
  return v3{((m[0] * x.x + m[1] * x.y) + m[2] * x.z) + m[3], ((m[4] * x.x + m[5] * x.y) + m[6] * x.z) + m[7],
            ((m[8] * x.x + m[9] * x.y) + m[10] * x.z) + m[11]};
}

// What the finish knows of one query: the key's dist2 and face, and for an answered query the closest point, its feature and the sign.
struct Answer {
  float dd;
  int f, feature, sign;
  v3 q;
};

// The winning face f is walked again (the same operations on the same operands: the same q), the walk says which feature q lies on,
// and the sign is that of s = dot(p - q, n): n = vn[the vertex's index] | en[f][the edge] | ab x ac.  s < 0 is inside (-1); zero, a
// NaN and every other s are outside (+1).  A face that won has its three indices inside the table, so the read of vn is in bounds.
__device__ __forceinline__ Answer answer_of(unsigned long long key, const v3& p, const float* __restrict__ pos, int Nv,
                                            const int32_t* __restrict__ faces, const float* __restrict__ vn,
                                            const float* __restrict__ en) {
  Answer r{__builtin_inff(), -1, -1, 0, v3{0.f, 0.f, 0.f}};
  if (key == kNoAnswer) return r;
  r.f = (int)(unsigned)(key & 0xffffffffull);
  r.dd = __uint_as_float((unsigned)(key >> 32));
  v3 a, b, c;
  face_vertices(pos, Nv, faces, r.f, a, b, c);
  const v3 ab = sub(b, a), ac = sub(c, a);
  closest_point_feature(p, a, b, c, ab, ac, r.q, r.feature);
  v3 n;
  if (r.feature < 3) n = load3(vn + (size_t)faces[(size_t)r.f * 3 + r.feature] * 3);
  else if (r.feature < kFeatureInterior) n = load3(en + ((size_t)r.f * 3 + (r.feature - 3)) * 3);
  else n = cross(ab, ac);
  const float s = dot(sub(p, r.q), n);
  r.sign = s < 0.f ? -1 : 1;
  return r;
}

__global__ __launch_bounds__(kThreads) void k_sg_init(unsigned long long* __restrict__ keys, int n) {
  const int i = blockIdx.x * kThreads + threadIdx.x;   // n <= 2^30
  if (i < n) keys[i] = kNoAnswer;
}

__global__ __launch_bounds__(kThreads) void k_sd_scan(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int F,
                                                      const float* __restrict__ points, int Q, int chunk,
                                                      unsigned long long* __restrict__ keys) {
  __shared__ float4 tile[kTile * kTileFloat4];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kThreads + tid;
  const bool live = i < Q;
  const v3 p = load3(points + (size_t)(live ? i : Q - 1) * 3);
  const int f0 = blockIdx.y * chunk;                  // < F <= 2^30: no overflow in f0 + chunk
  const int f1 = min(F, f0 + chunk);
  float best = __builtin_inff();
  int best_f = -1;
  scan_chunk<kTile>(p, tile, pos, Nv, faces, f0, f1, tid, best, best_f);
  if (live && best_f >= 0) merge_answer(keys + i, best, best_f);
}

// fp_mesh_grid_signed_distance's scan in place of k_sd_scan: a lane owns one query and walks the grid's shells around it (mesh_grid.h)
__global__ __launch_bounds__(kThreads) void k_sd_grid_scan(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int F,
                                                           mesh_grid::Grid g, mesh_grid::Tables t, const float* __restrict__ points,
                                                           int Q, unsigned long long* __restrict__ keys) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= Q) return;
  float best = __builtin_inff();
  int best_f = -1;
  mesh_grid::walk(g, t, pos, Nv, faces, F, load3(points + (size_t)i * 3), best, best_f);
  if (best_f >= 0) merge_answer(keys + i, best, best_f);
}

__global__ __launch_bounds__(kThreads) void k_sd_finish(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces,
                                                        const float* __restrict__ vn, const float* __restrict__ en,
                                                        const float* __restrict__ points, int Q,
                                                        const unsigned long long* __restrict__ keys, float* __restrict__ dist2,
                                                        int32_t* __restrict__ face, float* __restrict__ closest,
                                                        int32_t* __restrict__ feature, int32_t* __restrict__ sign) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= Q) return;
  const Answer r = answer_of(keys[i], load3(points + (size_t)i * 3), pos, Nv, faces, vn, en);
  dist2[i] = r.dd;
  if (face) face[i] = r.f;
  if (closest) {
    closest[(size_t)i * 3] = r.q.x;
    closest[(size_t)i * 3 + 1] = r.q.y;
    closest[(size_t)i * 3 + 2] = r.q.z;
  }
  if (feature) feature[i] = r.feature;
  if (sign) sign[i] = r.sign;
}

__global__ __launch_bounds__(kThreads) void k_pn_scan(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int F,
                                                      const float* __restrict__ points, int Q, const float* __restrict__ tfs,
                                                      int n_pairs, int chunk, unsigned long long* __restrict__ keys) {
  __shared__ float4 tile[kTile * kTileFloat4];
  const int tid = threadIdx.x;
  const int n = blockIdx.x * kThreads + tid;          // n_pairs <= 2^30: no overflow
  const bool live = n < n_pairs;
  const int nn = live ? n : n_pairs - 1;
  const int t = nn / Q, i = nn - t * Q;
  const v3 p = transformed(tfs + (size_t)t * 16, load3(points + (size_t)i * 3));
  const int f0 = blockIdx.y * chunk;                  // < F <= 2^30: no overflow in f0 + chunk
  const int f1 = min(F, f0 + chunk);
  float best = __builtin_inff();
  int best_f = -1;
  scan_chunk<kTile>(p, tile, pos, Nv, faces, f0, f1, tid, best, best_f);
  if (live && best_f >= 0) merge_answer(keys + n, best, best_f);
}

__global__ __launch_bounds__(kThreads) void k_pn_finish(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces,
                                                        const float* __restrict__ vn, const float* __restrict__ en,
                                                        const float* __restrict__ points, int Q, const float* __restrict__ tfs,
                                                        const unsigned long long* __restrict__ keys, int32_t* __restrict__ inside,
                                                        float* __restrict__ depth2, int32_t* __restrict__ deepest,
                                                        int32_t* __restrict__ sign, float* __restrict__ dist2) {
  __shared__ int s_inside;
  __shared__ unsigned long long s_deep;
  const int tid = threadIdx.x;
  const int t = blockIdx.x;
  if (tid == 0) {
    s_inside = 0;
    s_deep = 0ull;                                     // no point inside: every key of one is above it (~i != 0 for i < 2^30)
  }
  __syncthreads();
  const float* __restrict__ m = tfs + (size_t)t * 16;
  int cnt = 0;
  unsigned long long deep = 0ull;
  for (int i = tid; i < Q; i += kThreads) {
    const size_t n = (size_t)t * Q + i;
    const Answer r = answer_of(keys[n], transformed(m, load3(points + (size_t)i * 3)), pos, Nv, faces, vn, en);
    if (r.sign < 0) {
      const unsigned long long k = ((unsigned long long)__float_as_uint(r.dd) << 32) | (unsigned)~i;
      ++cnt;
      deep = k > deep ? k : deep;
    }
    if (sign) sign[n] = r.sign;
    if (dist2) dist2[n] = r.dd;
  }
  if (cnt) {
    atomicAdd(&s_inside, cnt);
    atomicMax(&s_deep, deep);
  }
  __syncthreads();
  if (tid == 0) {
    const unsigned long long k = s_deep;
    inside[t] = s_inside;
    if (depth2) depth2[t] = k ? __uint_as_float((unsigned)(k >> 32)) : 0.f;
    if (deepest) deepest[t] = k ? (int)~(unsigned)(k & 0xffffffffull) : -1;
  }
}

}  // namespace

extern "C" size_t fp_mesh_signed_distance_workspace_bytes(int Q) { return Q > 0 ? (size_t)Q * sizeof(unsigned long long) : 0; }

extern "C" int fp_mesh_signed_distance(const float* pos, int Nv, const int32_t* faces, int F, const float* vn, const float* en,
                                       const float* points, int Q, float* dist2, int32_t* face, float* closest, int32_t* feature,
                                       int32_t* sign, void* workspace, size_t workspace_bytes, void* stream) {
  const char* name = "fp_mesh_signed_distance";
  FP_REQUIRE(Q >= 0 && Q <= (1 << 30), "%s: Q=%d outside 0..2^30", name, Q);
  FP_REQUIRE(F >= 0 && F <= (1 << 30), "%s: F=%d outside 0..2^30", name, F);
  FP_REQUIRE(Nv >= 0, "%s: Nv=%d is negative", name, Nv);
  if (Q == 0) return FP_OK;
  FP_REQUIRE(points && dist2, "%s: NULL points or dist2", name);
  FP_REQUIRE(F == 0 || faces, "%s: faces is NULL but F=%d", name, F);
  FP_REQUIRE(F == 0 || Nv == 0 || pos, "%s: pos is NULL but Nv=%d", name, Nv);
  FP_REQUIRE(F == 0 || Nv == 0 || vn, "%s: vn is NULL but Nv=%d", name, Nv);
  FP_REQUIRE(F == 0 || en, "%s: en is NULL but F=%d", name, F);
  const size_t need = fp_mesh_signed_distance_workspace_bytes(Q);
  FP_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0,
             "%s: workspace too small or not 8-byte aligned (%zu < %zu bytes, see fp_mesh_signed_distance_workspace_bytes)", name,
             workspace_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  const int qtiles = fp_cdiv(Q, kThreads);
  hipLaunchKernelGGL(k_sg_init, dim3(qtiles), dim3(kThreads), 0, st, keys, Q);
  FP_CHECK_LAUNCH("fp_mesh_signed_distance (init)");
  if (F > 0) {
    const int chunk = chunk_faces(qtiles, F, kTile, kChunkMin, kFillWorkgroups);
    hipLaunchKernelGGL(k_sd_scan, dim3(qtiles, fp_cdiv(F, chunk)), dim3(kThreads), 0, st, pos, Nv, faces, F, points, Q, chunk, keys);
    FP_CHECK_LAUNCH("fp_mesh_signed_distance (scan)");
  }
  hipLaunchKernelGGL(k_sd_finish, dim3(qtiles), dim3(kThreads), 0, st, pos, Nv, faces, vn, en, points, Q,
                     (const unsigned long long*)keys, dist2, face, closest, feature, sign);
  FP_CHECK_LAUNCH("fp_mesh_signed_distance (finish)");
  return FP_OK;
}

extern "C" int fp_mesh_grid_signed_distance(const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid, const float* vn,
                                            const float* en, const float* points, int Q, float* dist2, int32_t* face, float* closest,
                                            int32_t* feature, int32_t* sign, void* workspace, size_t workspace_bytes, void* stream) {
  const char* name = "fp_mesh_grid_signed_distance";
  FP_REQUIRE(Q >= 0 && Q <= (1 << 30), "%s: Q=%d outside 0..2^30", name, Q);
  FP_REQUIRE(F >= 0 && F <= (1 << 30), "%s: F=%d outside 0..2^30", name, F);
  FP_REQUIRE(Nv >= 0, "%s: Nv=%d is negative", name, Nv);
  if (int st = mesh_grid::check_grid(name, grid)) return st;
  if (Q == 0) return FP_OK;
  FP_REQUIRE(points && dist2, "%s: NULL points or dist2", name);
  FP_REQUIRE(F == 0 || faces, "%s: faces is NULL but F=%d", name, F);
  FP_REQUIRE(F == 0 || Nv == 0 || pos, "%s: pos is NULL but Nv=%d", name, Nv);
  FP_REQUIRE(F == 0 || Nv == 0 || vn, "%s: vn is NULL but Nv=%d", name, Nv);
  FP_REQUIRE(F == 0 || en, "%s: en is NULL but F=%d", name, F);
  const size_t need = fp_mesh_signed_distance_workspace_bytes(Q);
  FP_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0,
             "%s: workspace too small or not 8-byte aligned (%zu < %zu bytes, see fp_mesh_signed_distance_workspace_bytes)", name,
             workspace_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  const int qtiles = fp_cdiv(Q, kThreads);
  hipLaunchKernelGGL(k_sg_init, dim3(qtiles), dim3(kThreads), 0, st, keys, Q);
  FP_CHECK_LAUNCH("fp_mesh_grid_signed_distance (init)");
  if (F > 0) {
    hipLaunchKernelGGL(k_sd_grid_scan, dim3(qtiles), dim3(kThreads), 0, st, pos, Nv, faces, F, mesh_grid::device_grid(grid),
                       mesh_grid::device_tables(grid), points, Q, keys);
    FP_CHECK_LAUNCH("fp_mesh_grid_signed_distance (scan)");
  }
  hipLaunchKernelGGL(k_sd_finish, dim3(qtiles), dim3(kThreads), 0, st, pos, Nv, faces, vn, en, points, Q,
                     (const unsigned long long*)keys, dist2, face, closest, feature, sign);
  FP_CHECK_LAUNCH("fp_mesh_grid_signed_distance (finish)");
  return FP_OK;
}

extern "C" size_t fp_mesh_penetration_workspace_bytes(int T, int Q) {
  if (T <= 0 || Q <= 0 || (long long)T * (long long)Q > (1ll << 30)) return 0;
  return (size_t)T * (size_t)Q * sizeof(unsigned long long);
}

extern "C" int fp_mesh_penetration(const float* pos, int Nv, const int32_t* faces, int F, const float* vn, const float* en,
                                   const float* points, int Q, const float* tfs, int T, int32_t* inside, float* depth2,
                                   int32_t* deepest, int32_t* sign, float* dist2, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  const char* name = "fp_mesh_penetration";
  FP_REQUIRE(T >= 0 && Q >= 0, "%s: T=%d or Q=%d is negative", name, T, Q);
  FP_REQUIRE((long long)T * (long long)Q <= (1ll << 30) && T <= (1 << 30), "%s: T=%d times Q=%d is above 2^30", name, T, Q);
  FP_REQUIRE(F >= 0 && F <= (1 << 30), "%s: F=%d outside 0..2^30", name, F);
  FP_REQUIRE(Nv >= 0, "%s: Nv=%d is negative", name, Nv);
  if (T == 0) return FP_OK;
  FP_REQUIRE(inside, "%s: NULL inside", name);
  FP_REQUIRE(Q == 0 || (points && tfs), "%s: NULL points or tfs", name);
  FP_REQUIRE(Q == 0 || F == 0 || faces, "%s: faces is NULL but F=%d", name, F);
  FP_REQUIRE(Q == 0 || F == 0 || Nv == 0 || pos, "%s: pos is NULL but Nv=%d", name, Nv);
  FP_REQUIRE(Q == 0 || F == 0 || Nv == 0 || vn, "%s: vn is NULL but Nv=%d", name, Nv);
  FP_REQUIRE(Q == 0 || F == 0 || en, "%s: en is NULL but F=%d", name, F);
  const size_t need = fp_mesh_penetration_workspace_bytes(T, Q);
  FP_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0),
             "%s: workspace too small or not 8-byte aligned (%zu < %zu bytes, see fp_mesh_penetration_workspace_bytes)", name,
             workspace_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  const int n_pairs = T * Q;
  if (n_pairs > 0) {
    const int tiles = fp_cdiv(n_pairs, kThreads);
    hipLaunchKernelGGL(k_sg_init, dim3(tiles), dim3(kThreads), 0, st, keys, n_pairs);
    FP_CHECK_LAUNCH("fp_mesh_penetration (init)");
    if (F > 0) {
      const int chunk = chunk_faces(tiles, F, kTile, kChunkMin, kFillWorkgroups);
      hipLaunchKernelGGL(k_pn_scan, dim3(tiles, fp_cdiv(F, chunk)), dim3(kThreads), 0, st, pos, Nv, faces, F, points, Q, tfs, n_pairs,
                         chunk, keys);
      FP_CHECK_LAUNCH("fp_mesh_penetration (scan)");
    }
  }
  hipLaunchKernelGGL(k_pn_finish, dim3(T), dim3(kThreads), 0, st, pos, Nv, faces, vn, en, points, Q, tfs,
                     (const unsigned long long*)keys, inside, depth2, deepest, sign, dist2);
  FP_CHECK_LAUNCH("fp_mesh_penetration (finish)");
  return FP_OK;
}
