// A texture atlas for a mesh from the posed RGB-D reference views it was fused from (fp_texture_bake; the definition is in
// include/fp_amd.h).  Face f owns the T x T texel block (f % Bx, f / Bx) of the atlas; a texel is a point of its face, projected into
// every view, kept where the view faces it and the view's depth agrees, and the kept colours are blended by cos^2 of the viewing angle.
//   k_texture_bake   one texel per lane, texels ordered block-major (lane g: face g / T^2, texel g % T^2 of its block), so a wave
//                    covers 64 / T^2 faces (T = 8: one) and the loads of the face's indices and vertices are (nearly) wave-uniform
//                    L1 hits.  The V views are visited inside the kernel in index order: one summation order, no atomics, nothing to
//                    clear.  A view's pose and intrinsics are wave-uniform (scalar) loads; depth / mask / rgb are gathers at the
//                    texel's pixel, which the texels of a block share or neighbour.
// The views are recon_common.h's ViewStack and the walk over them its load_view, to_camera and pixel_of, the ones k_tsdf_integrate
// calls: which views are skipped and which pixel a point falls on is decided there, the facing test between them here.
// Compiled with -ffp-contract=off (SRCS_EXACT): every float32 value is the one the numpy restatement (tests/texture_bake_model.py)
// computes.  Not a tuned path: baking is a setup call (three IEEE divisions and three dependent gathers per texel and view, as the
// fusion has per voxel and view).  Times: scripts/bench_reconstruct.py.
#include "fp_common.h"

#include <math.h>

#include "recon_common.h"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void k_texture_bake(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int F,
                                                           const float* __restrict__ vcol, recon::ViewStack in, int T, int Bx, size_t ntexels,
                                                           float tol, float min_cos2, float min_depth, float* __restrict__ tex,
                                                           uint8_t* __restrict__ coverage) {
  const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= ntexels) return;
  const int TT = T * T;
  const int f = (int)(g / (size_t)TT);
  const int r = (int)(g - (size_t)f * TT);
  const int j = r / T, i = r - j * T;
  const int bx = f % Bx, by = f / Bx;
  const size_t o = ((size_t)by * T + j) * ((size_t)Bx * T) + ((size_t)bx * T + i);
  float* out = tex + 3 * o;
  if (f >= F) {   // the rest of the last block row
    out[0] = out[1] = out[2] = 0.f;
    coverage[o] = 0;
    return;
  }
  const float den = (float)(T - 1);
  float a = (float)i / den, b = (float)j / den;
  const float s = a + b;
  if (s > 1.f) {   // beyond the hypotenuse: onto it
    a = a / s;
    b = b / s;
  }
  const float c = (1.f - a) - b;
  const int32_t* fi = faces + (size_t)f * 3;
  const int i0 = fi[0], i1 = fi[1], i2 = fi[2];
  const bool in0 = (unsigned)i0 < (unsigned)Nv, in1 = (unsigned)i1 < (unsigned)Nv, in2 = (unsigned)i2 < (unsigned)Nv;
  float fb0 = 128.f, fb1 = 128.f, fb2 = 128.f;
  if (vcol) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float c0 = in0 ? vcol[(size_t)i0 * 3 + k] : 128.f;
      const float c1 = in1 ? vcol[(size_t)i1 * 3 + k] : 128.f;
      const float c2 = in2 ? vcol[(size_t)i2 * 3 + k] : 128.f;
      const float m = (c * c0 + a * c1) + b * c2;
      if (k == 0) fb0 = m;
      if (k == 1) fb1 = m;
      if (k == 2) fb2 = m;
    }
  }
  float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, accw = 0.f;
  int cnt = 0;
  if (in0 && in1 && in2) {
    const float* P0 = pos + (size_t)i0 * 3;
    const float* P1 = pos + (size_t)i1 * 3;
    const float* P2 = pos + (size_t)i2 * 3;
    const float p0x = P0[0], p0y = P0[1], p0z = P0[2];
    const float p1x = P1[0], p1y = P1[1], p1z = P1[2];
    const float p2x = P2[0], p2y = P2[1], p2z = P2[2];
    const float px = (c * p0x + a * p1x) + b * p2x;
    const float py = (c * p0y + a * p1y) + b * p2y;
    const float pz = (c * p0z + a * p1z) + b * p2z;
    const float e1x = p1x - p0x, e1y = p1y - p0y, e1z = p1z - p0z;
    const float e2x = p2x - p0x, e2y = p2y - p0y, e2z = p2z - p0z;
    const float nx = e1y * e2z - e1z * e2y;
    const float ny = e1z * e2x - e1x * e2z;
    const float nz = e1x * e2y - e1y * e2x;
    const float nn = (nx * nx + ny * ny) + nz * nz;
    if (nn > 0.f && nn < INFINITY) {
      for (int v = 0; v < in.V; ++v) {
        const float* M;
        recon::Pinhole cam;
        if (!recon::load_view(in, v, M, cam)) continue;   // wave-uniform
        float X, Y, Z;
        recon::to_camera(M, px, py, pz, X, Y, Z);
        if (!(Z > 0.f)) continue;
        const float Nx = (M[0] * nx + M[1] * ny) + M[2] * nz;
        const float Ny = (M[4] * nx + M[5] * ny) + M[6] * nz;
        const float Nz = (M[8] * nx + M[9] * ny) + M[10] * nz;
        const float d = (Nx * X + Ny * Y) + Nz * Z;
        const float NN = (Nx * Nx + Ny * Ny) + Nz * Nz;
        const float rr = (X * X + Y * Y) + Z * Z;
        const float w = (d * d) / (NN * rr);   // cos^2 of the angle between the face's normal and the ray
        if (!(d < 0.f && w >= min_cos2)) continue;
        size_t p;
        if (!recon::pixel_of(in, v, cam, X, Y, Z, p)) continue;
        if (in.masks && in.masks[p] == 0) continue;
        const float dz = in.depth[p];
        if (!(dz >= min_depth)) continue;
        if (!(fabsf(dz - Z) <= tol)) continue;   // another surface is in front of the texel in this view (or behind it)
        const float* q = in.rgb + 3 * p;
        acc0 = acc0 + w * q[0];
        acc1 = acc1 + w * q[1];
        acc2 = acc2 + w * q[2];
        accw = accw + w;
        cnt = cnt + 1;
      }
    }
  }
  out[0] = cnt > 0 ? acc0 / accw : fb0;
  out[1] = cnt > 0 ? acc1 / accw : fb1;
  out[2] = cnt > 0 ? acc2 / accw : fb2;
  coverage[o] = (uint8_t)(cnt < 255 ? cnt : 255);
}

}  // namespace

extern "C" int fp_texture_bake(const float* pos, int Nv, const int32_t* faces, int F, const float* vertex_color, const float* depth,
                               const float* rgb, const uint8_t* masks, const float* ob_in_cams, const double* Ks, int V, int H, int W, int T,
                               int Bx, float tol, float min_cos, float min_depth, float* tex, uint8_t* coverage, void* stream) {
  const char* who = "fp_texture_bake";
  FP_REQUIRE(F >= 0 && F <= (1 << 24), "%s: F=%d outside 0..2^24 faces", who, F);
  FP_REQUIRE(Nv >= 0, "%s: Nv=%d must be >= 0", who, Nv);
  if (int st = recon::check_view_stack(who, V, H, W, "")) return st;
  FP_REQUIRE(T >= 2 && T <= FP_TEXTURE_BAKE_MAX_TEXELS, "%s: T=%d outside 2..%d texels a block side", who, T, FP_TEXTURE_BAKE_MAX_TEXELS);
  FP_REQUIRE(Bx >= 1, "%s: Bx=%d must be >= 1", who, Bx);
  const long long Wt = (long long)Bx * T, rows = ((long long)F + Bx - 1) / Bx, Ht = rows * T;
  FP_REQUIRE(Wt <= FP_TEXTURE_BAKE_MAX_SIDE && Ht <= FP_TEXTURE_BAKE_MAX_SIDE, "%s: an atlas of %lld x %lld texels (Ht x Wt), at most %d a side",
             who, Ht, Wt, FP_TEXTURE_BAKE_MAX_SIDE);
  FP_REQUIRE(isfinite(tol) && tol >= 0.f, "%s: tol=%g must be finite and >= 0", who, (double)tol);
  if (int st = recon::check_min_depth(who, min_depth)) return st;
  FP_REQUIRE(min_cos > 0.f && min_cos <= 1.f, "%s: min_cos=%g must be in (0, 1]", who, (double)min_cos);
  if (F == 0) return FP_OK;
  FP_REQUIRE(pos && faces && tex && coverage, "%s: NULL pos / faces / tex / coverage", who);
  FP_REQUIRE(V == 0 || (depth && rgb && ob_in_cams && Ks), "%s: NULL depth / rgb / ob_in_cams / Ks", who);
  const size_t ntexels = (size_t)(rows * Bx) * (size_t)(T * T);
  const recon::ViewStack in{depth, rgb, masks, ob_in_cams, Ks, V, H, W};
  hipLaunchKernelGGL(k_texture_bake, dim3((unsigned)((ntexels + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, pos, Nv,
                     faces, F, vertex_color, in, T, Bx, ntexels, tol, min_cos * min_cos, min_depth, tex, coverage);
  FP_CHECK_LAUNCH(who);
  return FP_OK;
}
