// An object's mesh from posed RGB-D reference views (fp_tsdf_integrate / fp_tsdf_count_triangles / fp_tsdf_emit_triangles; the
// definition is in include/fp_amd.h): truncated-signed-distance fusion into a voxel volume, then marching tetrahedra.
//   k_tsdf_integrate   one voxel per lane (x fastest: a wave reads and writes 64 consecutive voxels of each array).  The V views are
//                      visited inside the kernel in index order: the running means have one summation order, there are no atomics and
//                      nothing to clear.  A view's pose and intrinsics are wave-uniform loads; its depth / mask / rgb are gathers at
//                      the voxel's pixel, which neighbouring voxels share or neighbour (L2 hits after the first wave of a row).
//   k_tsdf_cubes<false>  one cube per lane: the 8 corner values once, then the case of each of the six Kuhn tetrahedra from the
//                      corner bits -> the cube's triangle count.
//   k_tsdf_cubes<true>   the same walk again, writing the triangles at the cube's offset (the exclusive prefix sum of the counts, made
//                      by the caller), so the order of the output is cube, tetrahedron, table order, whatever the scheduling.
// A triangle corner depends only on the grid edge it lies on (interpolated from the end with the smaller linear index), so every
// tetrahedron around an edge writes the same bits and the caller welds by the edge key.
// recon_common.h holds what is shared with texture_bake.hip, tsdf_raycast.hip and tsdf_components.hip: the walk over the posed views
// (load_view, to_camera, pixel_of), Grid, axis_gradient, lerp_from_a and the checks of the grid, the origin, the view stack, min_depth
// and min_weight.  Here: the three kernels, the corner, and the entry points with the checks of their own arguments.
// Compiled with -ffp-contract=off (SRCS_EXACT): every float32 value is the one the numpy restatement (tests/tsdf_model.py) computes.
// Not a tuned path: reconstruction is a setup call.  Fusion costs several times the volume's own traffic (three IEEE divisions and
// three dependent gathers per voxel and view).  The emit kernel runs one lane per cube, writes 3 x 44 bytes per triangle scattered,
// and recomputes a shared edge's interpolation, gradients and normalisation in every tetrahedron around the edge (about six times per
// welded vertex); a pass per unique edge would do that work once.  Times: scripts/bench_reconstruct.py, DESIGN.md section 5.
#include "fp_common.h"

#include <math.h>

#include "recon_common.h"
#include "tsdf_tables.h"

namespace {

using recon::Grid;
using recon::axis_gradient;
using recon::lerp_from_a;

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void k_tsdf_integrate(recon::ViewStack in, Grid g, size_t nvox, float trunc, float min_depth,
                                                             float* __restrict__ tsdf, float* __restrict__ weight,
                                                             float* __restrict__ color, float* __restrict__ color_weight) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= nvox) return;
  const int ix = (int)(i % (size_t)g.nx);
  const size_t r = i / (size_t)g.nx;
  const int iy = (int)(r % (size_t)g.ny), iz = (int)(r / (size_t)g.ny);
  const float px = g.ox + (float)ix * g.s, py = g.oy + (float)iy * g.s, pz = g.oz + (float)iz * g.s;
  float f = tsdf[i], w = weight[i], cw = color_weight[i];
  float c0 = color[3 * i], c1 = color[3 * i + 1], c2 = color[3 * i + 2];
  for (int v = 0; v < in.V; ++v) {
    const float* T;
    recon::Pinhole cam;
    if (!recon::load_view(in, v, T, cam)) continue;   // wave-uniform
    float X, Y, Z;
    recon::to_camera(T, px, py, pz, X, Y, Z);
    if (!(Z > 0.f)) continue;
    size_t p;
    if (!recon::pixel_of(in, v, cam, X, Y, Z, p)) continue;
    const bool object = in.masks ? in.masks[p] != 0 : true;
    float obs = 1.f, sdf = 0.f;
    if (object) {
      const float d = in.depth[p];
      if (!(d >= min_depth)) continue;
      sdf = d - Z;
      if (sdf < -trunc) continue;
      const float q = sdf / trunc;
      obs = q < 1.f ? q : 1.f;
    }
    f = (f * w + obs) / (w + 1.f);
    w = w + 1.f;
    if (object && fabsf(sdf) <= trunc) {
      const float* c = in.rgb + 3 * p;
      const float d1 = cw + 1.f;
      c0 = (c0 * cw + c[0]) / d1;
      c1 = (c1 * cw + c[1]) / d1;
      c2 = (c2 * cw + c[2]) / d1;
      cw = d1;
    }
  }
  tsdf[i] = f;
  weight[i] = w;
  color_weight[i] = cw;
  color[3 * i] = c0;
  color[3 * i + 1] = c1;
  color[3 * i + 2] = c2;
}

struct Fields {
  const float* tsdf;
  const float* color;
  const float* color_weight;
};

struct Outputs {
  int64_t* keys;
  float* pos;
  float* col;
  float* nrm;
};

// one triangle corner: on the grid edge between voxel (ax, ay, az) and voxel (bx, by, bz), the first with the smaller linear index
__device__ __forceinline__ void emit_corner(const Grid& g, const Fields& in, const Outputs& out, size_t row, int ax, int ay, int az, int bx,
                                            int by, int bz) {
  const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * g.ny;
  const size_t a = (size_t)az * sz + (size_t)ay * sy + ax, b = (size_t)bz * sz + (size_t)by * sy + bx;
  const float* f = in.tsdf;
  const float fa = f[a], fb = f[b];
  const float t = fa / (fa - fb);
  out.keys[row] = (int64_t)(((uint64_t)a << 32) | (uint64_t)b);
  float* P = out.pos + 3 * row;
  P[0] = lerp_from_a(g.ox + (float)ax * g.s, g.ox + (float)bx * g.s, t);
  P[1] = lerp_from_a(g.oy + (float)ay * g.s, g.oy + (float)by * g.s, t);
  P[2] = lerp_from_a(g.oz + (float)az * g.s, g.oz + (float)bz * g.s, t);
  const bool ha = in.color_weight[a] > 0.f, hb = in.color_weight[b] > 0.f;
  float* Cc = out.col + 3 * row;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float ca = ha ? in.color[3 * a + k] : 128.f, cb = hb ? in.color[3 * b + k] : 128.f;
    Cc[k] = ha && hb ? lerp_from_a(ca, cb, t) : (ha ? ca : cb);
  }
  const float gx = lerp_from_a(axis_gradient(f, a, 1, ax, g.nx), axis_gradient(f, b, 1, bx, g.nx), t);
  const float gy = lerp_from_a(axis_gradient(f, a, sy, ay, g.ny), axis_gradient(f, b, sy, by, g.ny), t);
  const float gz = lerp_from_a(axis_gradient(f, a, sz, az, g.nz), axis_gradient(f, b, sz, bz, g.nz), t);
  const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
  float* Nn = out.nrm + 3 * row;
  const bool has = len > 0.f;
  Nn[0] = has ? gx / len : 0.f;
  Nn[1] = has ? gy / len : 0.f;
  Nn[2] = has ? gz / len : 1.f;
}

// kEmit = false: counts[cube]; kEmit = true: the triangles of the cube at offsets[cube]
template <bool kEmit>
__global__ __launch_bounds__(kThreads) void k_tsdf_cubes(const float* __restrict__ tsdf, const float* __restrict__ weight, Grid g,
                                                         size_t ncubes, float min_weight, int32_t* __restrict__ counts,
                                                         const int64_t* __restrict__ offsets, long long total, Fields in, Outputs out) {
  const size_t c = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (c >= ncubes) return;
  const int mx = g.nx - 1, my = g.ny - 1;
  const int cx = (int)(c % (size_t)mx);
  const size_t r = c / (size_t)mx;
  const int cy = (int)(r % (size_t)my), cz = (int)(r / (size_t)my);
  const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * g.ny;
  const size_t base = (size_t)cz * sz + (size_t)cy * sy + cx;
  unsigned inside = 0, seen = 0;   // bit dx + 2 dy + 4 dz
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const size_t at = base + (k & 1) + (k >> 1 & 1) * sy + (k >> 2) * sz;
    inside |= (unsigned)(tsdf[at] < 0.f) << k;
    seen |= (unsigned)(weight[at] >= min_weight) << k;
  }
  int n = 0;
  long long tri = kEmit ? offsets[c] : 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    const TsdfTet& tet = kTsdfTets[t];
    int cs = 0;
    bool all = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int bit = tet.c[k][0] + 2 * tet.c[k][1] + 4 * tet.c[k][2];
      cs |= (int)(inside >> bit & 1u) << k;
      all = all && (seen >> bit & 1u);
    }
    if (!all) continue;
    const TsdfCase& tc = kTsdfCases[cs];
    if (!kEmit) {
      n += tc.n;
      continue;
    }
    for (int j = 0; j < tc.n; ++j, ++tri) {
      if (tri < 0 || tri >= total) return;   // a prefix sum that is not this volume's: never outside the outputs
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int e = tc.e[3 * j + (tet.odd && k ? 3 - k : k)];
        const int* A = tet.c[e >> 2];
        const int* B = tet.c[e & 3];
        emit_corner(g, in, out, (size_t)tri * 3 + k, cx + A[0], cy + A[1], cz + A[2], cx + B[0], cy + B[1], cz + B[2]);
      }
    }
  }
  if (!kEmit) counts[c] = n;
}

}  // namespace

extern "C" int fp_tsdf_integrate(const float* depth, const float* rgb, const uint8_t* masks, const float* ob_in_cams, const double* Ks, int V,
                                 int H, int W, int nz, int ny, int nx, const float* origin, float voxel, float trunc, float min_depth,
                                 float* tsdf, float* weight, float* color, float* color_weight, void* stream) {
  const char* who = "fp_tsdf_integrate";
  if (int st = recon::check_view_stack(who, V, H, W, " (fuse the views in several calls)")) return st;
  if (int st = recon::check_grid(who, nz, ny, nx)) return st;
  if (int st = recon::check_origin(who, origin, voxel)) return st;
  FP_REQUIRE(isfinite(trunc) && trunc > 0.f, "%s: trunc=%g must be finite and > 0", who, (double)trunc);
  if (int st = recon::check_min_depth(who, min_depth)) return st;
  FP_REQUIRE(tsdf && weight && color && color_weight, "%s: NULL volume array", who);
  if (V == 0) return FP_OK;
  FP_REQUIRE(depth && rgb && ob_in_cams && Ks, "%s: NULL depth / rgb / ob_in_cams / Ks", who);
  const size_t nvox = (size_t)nz * ny * nx;
  const Grid g{nz, ny, nx, origin[0], origin[1], origin[2], voxel};
  const recon::ViewStack in{depth, rgb, masks, ob_in_cams, Ks, V, H, W};
  hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)((nvox + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, in, g, nvox,
                     trunc, min_depth, tsdf, weight, color, color_weight);
  FP_CHECK_LAUNCH(who);
  return FP_OK;
}

extern "C" int fp_tsdf_count_triangles(const float* tsdf, const float* weight, int nz, int ny, int nx, float min_weight, int32_t* counts,
                                       void* stream) {
  const char* who = "fp_tsdf_count_triangles";
  if (int st = recon::check_grid(who, nz, ny, nx)) return st;
  if (int st = recon::check_min_weight(who, min_weight)) return st;
  const size_t ncubes = (size_t)(nz - 1) * (ny - 1) * (nx - 1);
  if (ncubes == 0) return FP_OK;
  FP_REQUIRE(tsdf && weight && counts, "%s: NULL tsdf / weight / counts", who);
  const Grid g{nz, ny, nx, 0.f, 0.f, 0.f, 1.f};
  hipLaunchKernelGGL(k_tsdf_cubes<false>, dim3((unsigned)((ncubes + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, tsdf,
                     weight, g, ncubes, min_weight, counts, (const int64_t*)nullptr, 0ll, Fields{nullptr, nullptr, nullptr},
                     Outputs{nullptr, nullptr, nullptr, nullptr});
  FP_CHECK_LAUNCH(who);
  return FP_OK;
}

extern "C" int fp_tsdf_emit_triangles(const float* tsdf, const float* weight, const float* color, const float* color_weight, int nz, int ny,
                                      int nx, const float* origin, float voxel, float min_weight, const int64_t* offsets, long long total,
                                      int64_t* keys, float* pos, float* col, float* nrm, void* stream) {
  const char* who = "fp_tsdf_emit_triangles";
  if (int st = recon::check_grid(who, nz, ny, nx)) return st;
  if (int st = recon::check_origin(who, origin, voxel)) return st;
  if (int st = recon::check_min_weight(who, min_weight)) return st;
  FP_REQUIRE(total >= 0 && total <= (1ll << 29), "%s: total=%lld outside 0..2^29 triangles", who, total);
  const size_t ncubes = (size_t)(nz - 1) * (ny - 1) * (nx - 1);
  if (ncubes == 0 || total == 0) return FP_OK;
  FP_REQUIRE(tsdf && weight && color && color_weight, "%s: NULL volume array", who);
  FP_REQUIRE(offsets && keys && pos && col && nrm, "%s: NULL offsets / keys / pos / col / nrm", who);
  const Grid g{nz, ny, nx, origin[0], origin[1], origin[2], voxel};
  hipLaunchKernelGGL(k_tsdf_cubes<true>, dim3((unsigned)((ncubes + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, tsdf,
                     weight, g, ncubes, min_weight, (int32_t*)nullptr, offsets, total, Fields{tsdf, color, color_weight},
                     Outputs{keys, pos, col, nrm});
  FP_CHECK_LAUNCH(who);
  return FP_OK;
}
