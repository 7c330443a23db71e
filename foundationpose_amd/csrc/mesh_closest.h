// The device arithmetic of the mesh queries, one copy: the closest point of a triangle to a point, how a workgroup passes a mesh's
// triangles through LDS, the transformed point of a (transform, point) pair, and the (dd, face) key a scan leaves for a finish.
// mesh_scan.hip (the nearest face of every query, for all the entry points) and mesh_grid.h (the grid's walk) scan with it;
// mesh_distance.hip (fp_mesh_point_distance), mesh_symmetry.hip (fp_mesh_transform_residuals), mesh_icp.hip (fp_mesh_icp_step) and
// mesh_signed.hip (fp_mesh_signed_distance, fp_mesh_penetration) finish with it; mesh_ray.hip (fp_mesh_ray_cast) passes its rays
// through the same tiles and keys with an intersection test of its own.  The definition, down to the float32 operation, is
// in include/fp_amd.h; the files are compiled with -ffp-contract=off (SRCS_EXACT), so the operations written here are the ones
// executed and the entry points give the same bits for the same (point, triangle) pair.
#pragma once
#include "fp_common.h"

namespace mesh_closest {

struct v3 { float x, y, z; };

__device__ __forceinline__ v3 sub(const v3& a, const v3& b) { return v3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(const v3& a, const v3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// The closest point of triangle (a, b, c) to p and its squared distance: include/fp_amd.h, Ericson 5.1.5.  The region tests r1..r6
// are the book's, each taken only when none before it held; one division serves whichever region was chosen (numerator and
// denominator selected first), so every value that reaches the result is made by the operations the definition names.
// `feature` is the part of the triangle q lies on: 0, 1, 2 vertex a, b, c (r1, r2, r4); 3, 4, 5 edge ab, bc, ca (r3, r6, r5); 6 the
// interior (r7).  It is selected from the region flags alone and takes part in no float operation: closest_point, which drops it,
// and closest_point_feature give the same q and the same dd.
constexpr int kFeatureInterior = 6;

__device__ __forceinline__ float closest_point_feature(const v3& p, const v3& a, const v3& b, const v3& c, const v3& ab, const v3& ac,
                                                       v3& q, int& feature) {
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
  feature = r1 ? 0 : r2 ? 1 : r4 ? 2 : r3 ? 3 : r6 ? 4 : r5 ? 5 : kFeatureInterior;
  const v3 d = sub(p, q);
  return dot(d, d);
}

__device__ __forceinline__ float closest_point(const v3& p, const v3& a, const v3& b, const v3& c, const v3& ab, const v3& ac, v3& q) {
  int feature;
  return closest_point_feature(p, a, b, c, ab, ac, q, feature);
}

// ab x ac in float32, each component one difference of two products: (ab1*ac2 - ab2*ac1, ab2*ac0 - ab0*ac2, ab0*ac1 - ab1*ac0)
__device__ __forceinline__ v3 cross(const v3& ab, const v3& ac) {
  return v3{ab.y * ac.z - ab.z * ac.y, ab.z * ac.x - ab.x * ac.z, ab.x * ac.y - ab.y * ac.x};
}

__device__ __forceinline__ v3 load3(const float* p) { return v3{p[0], p[1], p[2]}; }

// the point of a (transform, point) pair: rows 0..2 of the matrix as given; ((r0*x + r1*y) + r2*z) + t, one float32 operation each, in
// this order
__device__ __forceinline__ v3 transformed(const float* __restrict__ m, const v3& x) {
  return v3{((m[0] * x.x + m[1] * x.y) + m[2] * x.z) + m[3], ((m[4] * x.x + m[5] * x.y) + m[6] * x.z) + m[7],
            ((m[8] * x.x + m[9] * x.y) + m[10] * x.z) + m[11]};
}

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

// An LDS tile holds kTileFloat4 float4 per triangle: (a, b.x) (b.yz, c.xy) (c.z, ab) (ac, -).  The lane that stages face f into
// `slot` reads its three indices, checks them against Nv (a triangle with an index outside the table is staged as NaN and so never
// counts: nothing of pos is read for it) and writes a, b, c, b - a and c - a, the two differences being the definition's own float32
// operations done once per triangle instead of once per pair.
constexpr int kTileFloat4 = 4;

__device__ __forceinline__ void stage_triangle(float4* __restrict__ tile, int slot, const float* __restrict__ pos, int Nv,
                                               const int32_t* __restrict__ faces, int f) {
  v3 a, b, c;
  face_vertices(pos, Nv, faces, f, a, b, c);
  const v3 ab = sub(b, a), ac = sub(c, a);
  tile[slot * kTileFloat4 + 0] = make_float4(a.x, a.y, a.z, b.x);
  tile[slot * kTileFloat4 + 1] = make_float4(b.y, b.z, c.x, c.y);
  tile[slot * kTileFloat4 + 2] = make_float4(c.z, ab.x, ab.y, ab.z);
  tile[slot * kTileFloat4 + 3] = make_float4(ac.x, ac.y, ac.z, 0.f);
}

// the squared distance from p to the triangle staged in slot k: every lane reads the same address (an LDS broadcast, no bank conflict)
__device__ __forceinline__ float staged_distance2(const v3& p, const float4* __restrict__ tile, int k) {
  const float4 t0 = tile[k * kTileFloat4 + 0], t1 = tile[k * kTileFloat4 + 1], t2 = tile[k * kTileFloat4 + 2],
               t3 = tile[k * kTileFloat4 + 3];
  v3 q;
  return closest_point(p, v3{t0.x, t0.y, t0.z}, v3{t0.w, t1.x, t1.y}, v3{t1.z, t1.w, t2.x}, v3{t2.y, t2.z, t2.w},
                       v3{t3.x, t3.y, t3.z}, q);
}

// What a lane of the scan holds in registers: a query type with `candidate(tile, k)`, the value the triangle staged in slot k offers
// it (smaller wins), or NaN / +inf when that triangle does not answer.  A point offers its squared distance; mesh_ray.hip's ray offers
// the t of its intersection.
struct PointQuery {
  v3 p;
  __device__ __forceinline__ float candidate(const float4* __restrict__ tile, int k) const { return staged_distance2(p, tile, k); }
};

// The scan of one (lane tile, chunk of faces) workgroup, each lane holding its own query: faces f0..f1-1 pass through LDS in tiles
// of kTile (= the workgroup's size: one staging pass) and every lane keeps the smallest (value, face) -- faces ascend, so `<` keeps
// the smaller index on a tie.  best / best_f come in as +inf / -1.  Every thread of the workgroup calls it (barriers inside).
template <int kTile, class Query>
__device__ __forceinline__ void scan_chunk(const Query& q, float4* __restrict__ tile, const float* __restrict__ pos, int Nv,
                                           const int32_t* __restrict__ faces, int f0, int f1, int tid, float& best, int& best_f) {
  for (int base = f0; base < f1; base += kTile) {
    const int cnt = min(kTile, f1 - base);
    __syncthreads();                                  // the previous tile has been read by every wave
    if (tid < cnt) stage_triangle(tile, tid, pos, Nv, faces, base + tid);
    __syncthreads();
    // (the loop vectoriser would pair two triangles into packed-fp32 instructions, which this library is built without: Makefile)
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(2)
    for (int k = 0; k < cnt; ++k) {
      const float dd = q.candidate(tile, k);
      // dd < best holds for no NaN and no +inf (best starts at +inf): exactly the candidates with dd <= FLT_MAX that improve
      const bool better = dd < best;
      best = better ? dd : best;
      best_f = better ? base + k : best_f;
    }
  }
}

// the key of a lane's (dd, face): non-negative floats order as their bits do, so a 64-bit integer minimum picks the smallest (dd, face)
constexpr unsigned long long kNoAnswer = ~0ull;
__device__ __forceinline__ void merge_answer(unsigned long long* __restrict__ key, float best, int best_f) {
  const unsigned long long k = ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)best_f;
  __hip_atomic_fetch_min(key, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what a finish reads from a key: +inf and face -1 for a query that no triangle answered
struct Nearest {
  bool none;
  int f;
  float dd;
};
__device__ __forceinline__ Nearest nearest_of(unsigned long long key) {
  const bool none = key == kNoAnswer;
  return Nearest{none, none ? -1 : (int)(unsigned)(key & 0xffffffffull), none ? __builtin_inff() : __uint_as_float((unsigned)(key >> 32))};
}

}  // namespace mesh_closest
