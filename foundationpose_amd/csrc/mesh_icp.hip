// One Gauss-Newton step of point-to-plane ICP for each of T candidate transforms of Q surface samples against a triangle mesh
// (fp_mesh_icp_step; the definition, down to the operation, is in include/fp_amd.h): the hot path of a multi-start registration of
// one mesh onto another.  Four launches on the caller's stream, no allocation, no memset, no synchronisation, integer atomics only:
//   init, scan   mesh_scan.hip's nearest_face_of_pairs: the (transform, sample) pairs are numbered n = t * Q + i and a lane owns one,
//                so T transforms of a few samples still fill the chip.  The lane forms p = ((r0*x + r1*y) + r2*z) + t per row in
//                registers and leaves keys[n] = the smallest (bits(dd) << 32) | face over the mesh's triangles (the smaller index on
//                a tie), or all ones when no triangle answers
//   k_mi_terms   one workgroup per (transform, chunk of 256 consecutive samples), one lane per sample: p again (the same operations:
//                the same bits), the closest point q of the winning face recomputed as k_md_finish does, the face's unit normal, the
//                float32 residual r and Jacobian row J of the pair (or nothing), then icp.hip's own sums (icp_solve.h): the 28
//                float64 products and the widened dd over the wave by the xor tree, the four waves in index order; one row per
//                workgroup goes to partial[t][chunk].  dist2 and face, where asked for, are written here.
//   k_mi_finish  one wave per transform: lane c < 30 adds column c of the transform's partial rows in chunk order; lane 0 then damps,
//                factors, solves and updates the transform in float64 (icp_solve.h) and writes system[t] and tfs_out[t].
// The minimum commutes exactly, a chunk is 256 consecutive samples summed in one fixed order and the chunks are added in index order:
// the order of every sum depends on Q alone, so row t has the same bits alone, in any batch, under any chunking of the faces and on
// every replay.  Compiled with -ffp-contract=off (SRCS_EXACT): the float32 per-pair values are the ones the numpy restatement
// (tests/mesh_icp_model.py) computes, bit for bit.
// fp_mesh_grid_icp_step is the same call with a grid: the scan then walks the shells of a uniform grid around each p (mesh_grid.h);
// the keys are the interface, so the terms, the sums and the solve are the kernels above.
#include "icp_solve.h"
#include "mesh_scan.h"

namespace {

using namespace mesh_closest;
using icp_solve::kRow;
using icp_solve::kTerms;
using icp_solve::kWaves;

constexpr int kThreads = 256;          // samples per workgroup of the terms, one per lane
constexpr int kStore = kTerms + 1;     // the 28 terms and the sum of dd
constexpr int kCols = kStore + 1;      // + the pair count

static_assert(kThreads == icp_solve::kThreads, "a chunk of samples is one workgroup of the shared sums");
static_assert(kCols <= kRow, "a partial row holds the sums and the count");

__global__ __launch_bounds__(kThreads) void k_mi_terms(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces,
                                                       const float* __restrict__ points, int Q, const float* __restrict__ tfs, int C,
                                                       float max_dist, const unsigned long long* __restrict__ keys,
                                                       double* __restrict__ partial, float* __restrict__ dist2,
                                                       int32_t* __restrict__ face) {
  __shared__ double red[kWaves][kStore];
  __shared__ int cnt[kWaves];
  const int t = blockIdx.x / C, c = blockIdx.x - t * C;   // gridDim.x = T * C <= T * Q <= 2^30
  const int i = c * kThreads + threadIdx.x;
  const float md2 = max_dist * max_dist;
  float J[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, r = 0.f;
  double dd64 = 0.0;
  bool pair = false;
  if (i < Q) {   // no early return: every lane takes part in the shuffles, the ballot and the barrier below
    const float* __restrict__ m = tfs + (size_t)t * 16;
    const v3 p = transformed(m, load3(points + (size_t)i * 3));
    const size_t n = (size_t)t * Q + i;
    const Nearest k = nearest_of(keys[n]);
    const float dd = k.dd;
    if (dist2) dist2[n] = dd;
    if (face) face[n] = k.f;
    if (!k.none) {
      v3 a, b, cc, q;
      face_vertices(pos, Nv, faces, k.f, a, b, cc);
      const v3 ab = sub(b, a), ac = sub(cc, a);
      closest_point(p, a, b, cc, ab, ac, q);
      // the face normal, n = ab x ac in float32, made a unit vector through float64 (division and square root correctly rounded)
      const v3 nf = cross(ab, ac);
      const double nn = icp_solve::dot3d((double)nf.x, (double)nf.x, (double)nf.y, (double)nf.y, (double)nf.z, (double)nf.z);
      const double len = sqrt(nn);
      const float m0 = (float)((double)nf.x / len), m1 = (float)((double)nf.y / len), m2 = (float)((double)nf.z / len);
      pair = nn > 0.0 && __builtin_isfinite(m0) && __builtin_isfinite(m1) && __builtin_isfinite(m2) && dd <= md2;
      if (pair) {
        const v3 e = sub(q, p);
        const float a0 = p.x - m[3], a1 = p.y - m[7], a2 = p.z - m[11];
        r = icp_solve::dot3f(m0, e.x, m1, e.y, m2, e.z);
        J[0] = a1 * m2 - a2 * m1;
        J[1] = a2 * m0 - a0 * m2;
        J[2] = a0 * m1 - a1 * m0;
        J[3] = m0; J[4] = m1; J[5] = m2;
        dd64 = (double)dd;
      }
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long bp = __ballot(pair);
  if (lane == 0) cnt[wave] = __popcll(bp);
  icp_solve::wave_sums<kStore>(J, r, dd64, bp, lane, red[wave]);
  __syncthreads();
  icp_solve::chunk_sums<kStore>(red, cnt, partial + (size_t)blockIdx.x * kRow);
}

__global__ __launch_bounds__(64) void k_mi_finish(const double* __restrict__ partial, int C, const float* __restrict__ tfs_in,
                                                  double damping, int min_pairs, double* __restrict__ system,
                                                  float* __restrict__ tfs_out) {
  __shared__ double sum[kCols];
  const int t = blockIdx.x, lane = threadIdx.x;
  if (lane < kCols) {
    const double* p = partial + (size_t)t * C * kRow + lane;
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += p[(size_t)c * kRow];
    sum[lane] = s;
  }
  __syncthreads();
  if (lane != 0) return;
  double* o = system + (size_t)t * 40;
  icp_solve::solve_and_update(sum, sum[kStore], tfs_in + (size_t)t * 16, damping, min_pairs, o,
                              tfs_out ? tfs_out + (size_t)t * 16 : nullptr);
  o[36] = sum[kTerms];   // the sum of dd over the pairs
}

inline size_t keys_bytes(int T, int Q) { return (size_t)T * (size_t)Q * sizeof(unsigned long long); }
inline size_t workspace_of(int T, int Q) { return keys_bytes(T, Q) + (size_t)T * (size_t)fp_cdiv(Q, kThreads) * kRow * sizeof(double); }

// fp_mesh_icp_step (gridded: no) and fp_mesh_grid_icp_step (gridded: yes) are one call, the scan exchanged
int icp_step(const char* name, bool gridded, const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid,
             const float* points, int Q, const float* tfs_in, int T, float max_dist, double damping, int min_pairs, double* system,
             float* tfs_out, float* dist2, int32_t* face, void* workspace, size_t workspace_bytes, void* stream) {
  if (int st = mesh_scan::check_pairs(name, T, Q, F, Nv, gridded, grid)) return st;
  FP_REQUIRE(max_dist >= 0.f && __builtin_isfinite(max_dist), "%s: max_dist=%g must be finite and >= 0", name, (double)max_dist);
  FP_REQUIRE(damping >= 0.0 && __builtin_isfinite(damping), "%s: damping=%g must be finite and >= 0", name, damping);
  FP_REQUIRE(min_pairs >= 6, "%s: min_pairs=%d must be >= 6 (the unknowns of a step)", name, min_pairs);
  if (T == 0) return FP_OK;
  FP_REQUIRE(tfs_in && system, "%s: NULL tfs_in or system", name);
  FP_REQUIRE(Q == 0 || points, "%s: NULL points", name);
  if (int st = mesh_scan::check_mesh(name, Q > 0, pos, Nv, faces, F)) return st;
  if (int st = mesh_scan::check_workspace(name, workspace, workspace_bytes, fp_mesh_icp_workspace_bytes(T, Q), 8,
                                          "fp_mesh_icp_workspace_bytes"))
    return st;
  if (tfs_out) {   // the finish of one transform writes tfs_out while the terms of another still read tfs_in: no shared bytes
    const uintptr_t a = (uintptr_t)tfs_in, b = (uintptr_t)tfs_out, len = (uintptr_t)T * 16 * sizeof(float);
    FP_REQUIRE(a + len <= b || b + len <= a, "%s: tfs_in and tfs_out overlap", name);
  }
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  double* partial = (double*)((char*)workspace + keys_bytes(T, Q));   // 8 * T * Q bytes on: still 8-byte aligned
  const int C = fp_cdiv(Q, kThreads);
  if (Q > 0) {
    if (int e = mesh_scan::nearest_face_of_pairs(name, pos, Nv, faces, F, gridded ? grid : nullptr, points, Q, tfs_in, T, keys, st)) return e;
    hipLaunchKernelGGL(k_mi_terms, dim3(T * C), dim3(kThreads), 0, st, pos, Nv, faces, points, Q, tfs_in, C, max_dist,
                       (const unsigned long long*)keys, partial, dist2, face);
    if (int e = mesh_scan::launched(name, "terms")) return e;
  }
  hipLaunchKernelGGL(k_mi_finish, dim3(T), dim3(64), 0, st, (const double*)partial, C, tfs_in, damping, min_pairs, system, tfs_out);
  return mesh_scan::launched(name, "finish");
}

}  // namespace

extern "C" size_t fp_mesh_icp_workspace_bytes(int T, int Q) {
  if (T <= 0 || Q <= 0 || (long long)T * (long long)Q > (1ll << 30)) return 0;
  return workspace_of(T, Q);
}

extern "C" int fp_mesh_icp_step(const float* pos, int Nv, const int32_t* faces, int F, const float* points, int Q, const float* tfs_in,
                                int T, float max_dist, double damping, int min_pairs, double* system, float* tfs_out, float* dist2,
                                int32_t* face, void* workspace, size_t workspace_bytes, void* stream) {
  return icp_step("fp_mesh_icp_step", false, pos, Nv, faces, F, nullptr, points, Q, tfs_in, T, max_dist, damping, min_pairs, system,
                  tfs_out, dist2, face, workspace, workspace_bytes, stream);
}

extern "C" int fp_mesh_grid_icp_step(const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid, const float* points,
                                     int Q, const float* tfs_in, int T, float max_dist, double damping, int min_pairs, double* system,
                                     float* tfs_out, float* dist2, int32_t* face, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  return icp_step("fp_mesh_grid_icp_step", true, pos, Nv, faces, F, grid, points, Q, tfs_in, T, max_dist, damping, min_pairs, system,
                  tfs_out, dist2, face, workspace, workspace_bytes, stream);
}
