// The exact distance from Q points to the surface of a triangle mesh (fp_mesh_point_distance; the definition, down to the float32
// operation, is in include/fp_amd.h): brute force over every (query, triangle) pair.  Three launches on the caller's stream, no
// allocation, no synchronisation, integer atomics only:
//   k_md_init    keys[i] = all ones ("no triangle answered yet")
//   k_md_scan    grid (tile of kThreads queries, chunk of faces): a lane owns one query in registers.  The chunk's triangles pass
//                through LDS in tiles of kTile: the lane that stages a triangle reads its three indices, checks them against Nv (a
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
#include <float.h>
#include "fp_common.h"

namespace {

constexpr int kThreads = 256;          // queries per workgroup, one per lane
constexpr int kTile = 256;             // triangles per LDS tile: 4 float4 each, 16 KiB
constexpr int kChunkMin = 1024;        // the fewest faces a workgroup scans (unless the mesh has fewer)
constexpr int kFillWorkgroups = 2048;  // workgroups wanted in flight (256 CUs x 8 of 4 waves)
constexpr unsigned long long kNoAnswer = ~0ull;

static_assert(kChunkMin % kTile == 0, "a chunk is whole tiles");
static_assert(kTile == kThreads, "a tile is staged by one pass of the workgroup");

// faces per chunk: a multiple of kTile, at least kChunkMin, and no smaller than what gives about kFillWorkgroups workgroups
inline int chunk_faces(int Q, int F) {
  const int qtiles = fp_cdiv(Q, kThreads);
  const int want = qtiles >= kFillWorkgroups ? 1 : fp_cdiv(kFillWorkgroups, qtiles);   // chunks wanted
  int chunk = fp_cdiv(F > 0 ? F : 1, want);
  if (chunk < kChunkMin) chunk = kChunkMin;
  return fp_cdiv(chunk, kTile) * kTile;
}

struct v3 { float x, y, z; };

__device__ __forceinline__ v3 sub(const v3& a, const v3& b) { return v3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(const v3& a, const v3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// The closest point of triangle (a, b, c) to p and its squared distance: include/fp_amd.h, Ericson 5.1.5.  The region tests r1..r6
// are the book's, each taken only when none before it held; one division serves whichever region was chosen (numerator and
// denominator selected first), so every value that reaches the result is made by the operations the definition names.
__device__ __forceinline__ float closest_point(const v3& p, const v3& a, const v3& b, const v3& c, const v3& ab, const v3& ac, v3& q) {
  const v3 ap = sub(p, a);
  const float d1 = dot(ab, ap), d2 = dot(ac, ap);
  const v3 bp = sub(p, b);
  const float d3 = dot(ab, bp), d4 = dot(ac, bp);
  const v3 cp = sub(p, c);
  const float d5 = dot(ab, cp), d6 = dot(ac, cp);
  const float vc = d1 * d4 - d3 * d2;
  const float vb = d5 * d2 - d1 * d6;
  const float va = d3 * d6 - d5 * d4;
  const float e = d4 - d3, g = d5 - d6;
  const bool r1 = d1 <= 0.f && d2 <= 0.f;
  const bool r2 = !r1 && (d3 >= 0.f && d4 <= d3);
  const bool r12 = r1 || r2;
  const bool r3 = !r12 && (vc <= 0.f && d1 >= 0.f && d3 <= 0.f);
  const bool r123 = r12 || r3;
  const bool r4 = !r123 && (d6 >= 0.f && d5 <= d6);
  const bool r1234 = r123 || r4;
  const bool r5 = !r1234 && (vb <= 0.f && d2 >= 0.f && d6 <= 0.f);
  const bool r12345 = r1234 || r5;
  const bool r6 = !r12345 && (va <= 0.f && e >= 0.f && g >= 0.f);
  const bool r7 = !(r12345 || r6);
  // the one quotient: d1 / (d1 - d3) | d2 / (d2 - d6) | e / (e + g) | 1 / ((va + vb) + vc)
  const float num = r3 ? d1 : r5 ? d2 : r6 ? e : 1.f;
  const float den = r3 ? d1 - d3 : r5 ? d2 - d6 : r6 ? e + g : (va + vb) + vc;
  const float t = num / den;
  // q = base + s * dir (+ w * ac in the interior); a vertex region returns the vertex itself
  const v3 base = r6 ? b : a;
  const v3 dir = r5 ? ac : r6 ? sub(c, b) : ab;
  const float s = r7 ? vb * t : t;
  v3 e1{base.x + s * dir.x, base.y + s * dir.y, base.z + s * dir.z};
  const float w = vc * t;
  const v3 in{e1.x + w * ac.x, e1.y + w * ac.y, e1.z + w * ac.z};
  q = r1 ? a : r2 ? b : r4 ? c : r7 ? in : e1;
  const v3 d = sub(p, q);
  return dot(d, d);
}

__device__ __forceinline__ v3 load3(const float* p) { return v3{p[0], p[1], p[2]}; }

// the vertices of face f, NaN when an index is outside 0..Nv-1
__device__ __forceinline__ void face_vertices(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int f, v3& a,
                                              v3& b, v3& c) {
  const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
  const bool ok = (unsigned)i0 < (unsigned)Nv && (unsigned)i1 < (unsigned)Nv && (unsigned)i2 < (unsigned)Nv;
  const float nan = __builtin_nanf("");
  a = b = c = v3{nan, nan, nan};
  if (ok) {
    a = load3(pos + (size_t)i0 * 3);
    b = load3(pos + (size_t)i1 * 3);
    c = load3(pos + (size_t)i2 * 3);
  }
}

__global__ __launch_bounds__(kThreads) void k_md_init(unsigned long long* __restrict__ keys, int Q) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < Q) keys[i] = kNoAnswer;
}

__global__ __launch_bounds__(kThreads) void k_md_scan(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int F,
                                                      const float* __restrict__ points, int Q, int chunk,
                                                      unsigned long long* __restrict__ keys) {
  __shared__ float4 tile[kTile * 4];   // per triangle: (a, b.x) (b.yz, c.xy) (c.z, ab) (ac, -)
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kThreads + tid;
  const bool live = i < Q;
  const v3 p = load3(points + (size_t)(live ? i : Q - 1) * 3);
  const int f0 = blockIdx.y * chunk;                  // < F <= 2^30: no overflow in f0 + chunk
  const int f1 = min(F, f0 + chunk);
  float best = __builtin_inff();
  int best_f = -1;
  for (int base = f0; base < f1; base += kTile) {
    const int cnt = min(kTile, f1 - base);
    __syncthreads();                                  // the previous tile has been read by every wave
    if (tid < cnt) {
      v3 a, b, c;
      face_vertices(pos, Nv, faces, base + tid, a, b, c);
      const v3 ab = sub(b, a), ac = sub(c, a);
      tile[tid * 4 + 0] = make_float4(a.x, a.y, a.z, b.x);
      tile[tid * 4 + 1] = make_float4(b.y, b.z, c.x, c.y);
      tile[tid * 4 + 2] = make_float4(c.z, ab.x, ab.y, ab.z);
      tile[tid * 4 + 3] = make_float4(ac.x, ac.y, ac.z, 0.f);
    }
    __syncthreads();
    // (the loop vectoriser would pair two triangles into packed-fp32 instructions, which this library is built without: Makefile)
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(2)
    for (int k = 0; k < cnt; ++k) {
      const float4 t0 = tile[k * 4 + 0], t1 = tile[k * 4 + 1], t2 = tile[k * 4 + 2], t3 = tile[k * 4 + 3];
      v3 q;
      const float dd = closest_point(p, v3{t0.x, t0.y, t0.z}, v3{t0.w, t1.x, t1.y}, v3{t1.z, t1.w, t2.x}, v3{t2.y, t2.z, t2.w},
                                     v3{t3.x, t3.y, t3.z}, q);
      // dd < best holds for no NaN and no +inf (best starts at +inf): exactly the candidates with dd <= FLT_MAX that improve
      const bool better = dd < best;
      best = better ? dd : best;
      best_f = better ? base + k : best_f;
    }
  }
  if (live && best_f >= 0) {
    const unsigned long long key = ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)best_f;
    __hip_atomic_fetch_min(keys + i, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
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
