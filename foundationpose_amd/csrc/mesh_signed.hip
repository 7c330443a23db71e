// Which side of a closed triangle mesh a point is on (fp_mesh_signed_distance), and how far T placements of Q points reach into it
// (fp_mesh_penetration); the definitions, down to the float32 operation, are in include/fp_amd.h.  The distance is the unsigned
// siblings' own: mesh_scan.hip's nearest face of every query (one copy; the same bits as fp_mesh_point_distance).  The sign needs no
// second scan and no transcendental: the finish re-walks the winning face, learns which feature of it the closest point q lies on (a
// vertex, an edge, the interior) and takes the sign of (p - q) . n for that feature's angle-weighted pseudonormal n (Baerentzen and
// Aanaes 2005), read from the tables fp_mesh_pseudonormals made on the host (vn per vertex, en per face edge) or, in the interior,
// formed as ab x ac.
//   fp_mesh_signed_distance, three launches:
//     init, scan   nearest_face_of_points: keys[i] = the smallest (bits(dd) << 32) | face, or all ones
//     k_sd_finish  one lane per query: dist2 and face from the key, q and the feature from the re-walk, n, the sign
//   fp_mesh_penetration, three launches:
//     init, scan   nearest_face_of_pairs: the pairs are numbered n = t * Q + i and a lane owns one; p = ((r0*x + r1*y) + r2*z) + t
//     k_pn_finish  one workgroup per transform: each lane re-walks its pairs as k_sd_finish does, then the workgroup reduces in LDS
//                  with integer atomics only: an add for the number of points inside, a 64-bit maximum on (bits(dd) << 32) | ~i for
//                  the deepest of them (the larger dd, then the smaller i)
//   fp_mesh_grid_signed_distance: fp_mesh_signed_distance with a grid: the scan walks the shells of a uniform grid around each query
//     (mesh_grid.h), and k_sd_finish is unchanged
//   fp_mesh_grid_penetration: fp_mesh_penetration with a grid: the same walk around each transformed point, and k_pn_finish unchanged
// A minimum, a maximum and an integer count commute exactly: every output has one value whatever the chunking and the arrival order.
// No allocation, no memset, no synchronisation.  Compiled with -ffp-contract=off (SRCS_EXACT): the numpy restatement
// (tests/mesh_signed_model.py) computes the same bits.
#include "mesh_scan.h"

namespace {

using namespace mesh_closest;

constexpr int kThreads = 256;   // lanes of a finish workgroup: one per query, or striding over a transform's points

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
  const Nearest k = nearest_of(key);
  Answer r{k.dd, k.f, -1, 0, v3{0.f, 0.f, 0.f}};
  if (k.none) return r;
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

// the pseudonormal tables of a call with something to scan (live: Q > 0)
inline int check_tables(const char* name, bool live, const float* vn, int Nv, const float* en, int F) {
  FP_REQUIRE(!live || F == 0 || Nv == 0 || vn, "%s: vn is NULL but Nv=%d", name, Nv);
  FP_REQUIRE(!live || F == 0 || en, "%s: en is NULL but F=%d", name, F);
  return FP_OK;
}

// fp_mesh_signed_distance (gridded: no) and fp_mesh_grid_signed_distance (gridded: yes) are one call, the scan exchanged
int signed_distance(const char* name, bool gridded, const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid,
                    const float* vn, const float* en, const float* points, int Q, float* dist2, int32_t* face, float* closest,
                    int32_t* feature, int32_t* sign, void* workspace, size_t workspace_bytes, void* stream) {
  if (int st = mesh_scan::check_points(name, pos, Nv, faces, F, gridded, grid, points, Q, dist2)) return st;
  if (Q == 0) return FP_OK;
  if (int st = check_tables(name, true, vn, Nv, en, F)) return st;
  if (int st = mesh_scan::check_workspace(name, workspace, workspace_bytes, fp_mesh_signed_distance_workspace_bytes(Q), 8,
                                          "fp_mesh_signed_distance_workspace_bytes"))
    return st;
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  if (int e = mesh_scan::nearest_face_of_points(name, pos, Nv, faces, F, gridded ? grid : nullptr, points, Q, keys, st)) return e;
  hipLaunchKernelGGL(k_sd_finish, dim3(fp_cdiv(Q, kThreads)), dim3(kThreads), 0, st, pos, Nv, faces, vn, en, points, Q,
                     (const unsigned long long*)keys, dist2, face, closest, feature, sign);
  return mesh_scan::launched(name, "finish");
}

// fp_mesh_penetration (gridded: no) and fp_mesh_grid_penetration (gridded: yes) are one call, the scan exchanged
int penetration(const char* name, bool gridded, const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid,
                const float* vn, const float* en, const float* points, int Q, const float* tfs, int T, int32_t* inside, float* depth2,
                int32_t* deepest, int32_t* sign, float* dist2, void* workspace, size_t workspace_bytes, void* stream) {
  if (int st = mesh_scan::check_pairs(name, T, Q, F, Nv, gridded, grid)) return st;
  if (T == 0) return FP_OK;
  FP_REQUIRE(inside, "%s: NULL inside", name);
  FP_REQUIRE(Q == 0 || (points && tfs), "%s: NULL points or tfs", name);
  if (int st = mesh_scan::check_mesh(name, Q > 0, pos, Nv, faces, F)) return st;
  if (int st = check_tables(name, Q > 0, vn, Nv, en, F)) return st;
  if (int st = mesh_scan::check_workspace(name, workspace, workspace_bytes, fp_mesh_penetration_workspace_bytes(T, Q), 8,
                                          "fp_mesh_penetration_workspace_bytes"))
    return st;
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  if (Q > 0)
    if (int e = mesh_scan::nearest_face_of_pairs(name, pos, Nv, faces, F, gridded ? grid : nullptr, points, Q, tfs, T, keys, st)) return e;
  hipLaunchKernelGGL(k_pn_finish, dim3(T), dim3(kThreads), 0, st, pos, Nv, faces, vn, en, points, Q, tfs,
                     (const unsigned long long*)keys, inside, depth2, deepest, sign, dist2);
  return mesh_scan::launched(name, "finish");
}

}  // namespace

extern "C" size_t fp_mesh_signed_distance_workspace_bytes(int Q) { return Q > 0 ? (size_t)Q * sizeof(unsigned long long) : 0; }

extern "C" int fp_mesh_signed_distance(const float* pos, int Nv, const int32_t* faces, int F, const float* vn, const float* en,
                                       const float* points, int Q, float* dist2, int32_t* face, float* closest, int32_t* feature,
                                       int32_t* sign, void* workspace, size_t workspace_bytes, void* stream) {
  return signed_distance("fp_mesh_signed_distance", false, pos, Nv, faces, F, nullptr, vn, en, points, Q, dist2, face, closest, feature,
                         sign, workspace, workspace_bytes, stream);
}

extern "C" int fp_mesh_grid_signed_distance(const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid, const float* vn,
                                            const float* en, const float* points, int Q, float* dist2, int32_t* face, float* closest,
                                            int32_t* feature, int32_t* sign, void* workspace, size_t workspace_bytes, void* stream) {
  return signed_distance("fp_mesh_grid_signed_distance", true, pos, Nv, faces, F, grid, vn, en, points, Q, dist2, face, closest, feature,
                         sign, workspace, workspace_bytes, stream);
}

extern "C" size_t fp_mesh_penetration_workspace_bytes(int T, int Q) {
  if (T <= 0 || Q <= 0 || (long long)T * (long long)Q > (1ll << 30)) return 0;
  return (size_t)T * (size_t)Q * sizeof(unsigned long long);
}

extern "C" int fp_mesh_penetration(const float* pos, int Nv, const int32_t* faces, int F, const float* vn, const float* en,
                                   const float* points, int Q, const float* tfs, int T, int32_t* inside, float* depth2,
                                   int32_t* deepest, int32_t* sign, float* dist2, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  return penetration("fp_mesh_penetration", false, pos, Nv, faces, F, nullptr, vn, en, points, Q, tfs, T, inside, depth2, deepest, sign,
                     dist2, workspace, workspace_bytes, stream);
}

extern "C" int fp_mesh_grid_penetration(const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid, const float* vn,
                                        const float* en, const float* points, int Q, const float* tfs, int T, int32_t* inside,
                                        float* depth2, int32_t* deepest, int32_t* sign, float* dist2, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  return penetration("fp_mesh_grid_penetration", true, pos, Nv, faces, F, grid, vn, en, points, Q, tfs, T, inside, depth2, deepest, sign,
                     dist2, workspace, workspace_bytes, stream);
}
