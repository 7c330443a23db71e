// The zero surface of a TSDF volume seen from N poses (fp_tsdf_raycast; the definition is in include/fp_amd.h): depth, camera-frame points,
// camera-frame unit normals and colours per crop pixel, in the layout fp_icp_point_plane and fp_depth_agreement read beside the same crop
// windows -- what render_crops gives for the extracted mesh, without extracting one.
//   k_tsdf_raycast   grid (16 x 16 pixel blocks of the crop, n), one lane per crop pixel.  A wave is an 8 x 8 pixel tile (lane l at
//                    (l & 7, l >> 3) of it, the four waves 2 x 2 tiles), so the 64 rays of a wave walk through neighbouring cells and
//                    share their corners in cache; the volumes fused here (8 .. 32 MB) stay in L2 / MALL.  The row's constants (the ray
//                    origin o = -R^T t, R, the window, the intrinsics, whether the row is usable) are computed by lane 0 into LDS.  Each
//                    ray is clipped to the volume's box (and z_near .. z_far), then sampled at z_0 + k * step: a trilinear sample of tsdf
//                    over the cell that holds the point, known only where all eight corners were observed.  The first known sample
//                    below 0 after a known one at or above 0 is the hit; the surface is the zero of the chord between the two.
// No atomics, no workspace, no allocation, no synchronisation; every output element is written exactly once (0 on a miss).  The march
// is divergent by nature: a wave runs as long as its longest ray, which the box clip bounds by the box's diagonal over step.
// The volume's Grid, the extraction's axis_gradient and lerp_from_a, and the checks of the grid, the origin and min_weight are
// recon_common.h's; trilinear and dot3f, which only the rays use, are here.
// Compiled with -ffp-contract=off (SRCS_EXACT): every float32 value is the one the numpy restatement (tests/tsdf_raycast_model.py)
// computes, bit for bit.  Times: scripts/bench_tsdf_raycast.py, DESIGN.md section 1.
#include "fp_common.h"

#include <math.h>

#include "recon_common.h"

namespace {

using recon::axis_gradient;
using recon::lerp_from_a;

constexpr int kThreads = 256;
constexpr int kBlockSide = 16;    // pixels a workgroup covers per axis: 2 x 2 wave tiles of 8 x 8

struct Volume {
  const float* tsdf;
  const float* weight;
  const float* color;
  const float* color_weight;
  recon::Grid g;
};

struct Camera {      // one host K9 (view == NULL, Ks == NULL) or the fp_views table
  fp_k9 K1;
  fp_views vt;
};

struct RayOut {
  float* depth;
  float* xyz;
  float* normal;
  float* color;
};

// the row's constants in LDS
enum { kO = 0, kR = 3, kUmin = 12, kVmin, kAx, kAy, kFx, kFy, kCx, kCy, kRowFloats };

__device__ __forceinline__ float dot3f(float a0, float b0, float a1, float b1, float a2, float b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

// the value at (fx, fy, fz) inside a cell from its corners v[dx + 2 dy + 4 dz]: along x, then y, then z
__device__ __forceinline__ float trilinear(const float v[8], float fx, float fy, float fz) {
  const float c00 = lerp_from_a(v[0], v[1], fx), c10 = lerp_from_a(v[2], v[3], fx);
  const float c01 = lerp_from_a(v[4], v[5], fx), c11 = lerp_from_a(v[6], v[7], fx);
  return lerp_from_a(lerp_from_a(c00, c10, fy), lerp_from_a(c01, c11, fy), fz);
}

__global__ __launch_bounds__(kThreads) void k_tsdf_raycast(Volume vol, float min_weight, const float* __restrict__ poses, Camera cam,
                                                           const float* __restrict__ bbox2d, int H, int W, int oh, int ow, float step,
                                                           float z_near, float z_far, int tiles_x, RayOut out) {
  __shared__ float row[kRowFloats];
  __shared__ int row_ok;
  const recon::Grid& g = vol.g;
  const int n = blockIdx.y;
  if (threadIdx.x == 0) {
    const float* T = poses + (size_t)n * 16;
    bool ok = g.nz >= 2 && g.ny >= 2 && g.nx >= 2;
#pragma unroll
    for (int k = 0; k < 16; ++k) ok = ok && isfinite(T[k]);
    fp_k9 K = cam.K1;
    if (cam.vt.Ks) {
      const int v = fp_view_of(cam.vt, n);
      ok = ok && v >= 0;
      K = fp_view_K<fp_k9, float>(cam.vt, v);
    }
    const float fx = K.v[0], skew = K.v[1], cx = K.v[2], fy = K.v[4], cy = K.v[5];
    ok = ok && isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy) && skew == 0.f;
    float umin = 0.f, vmin = 0.f, umax = (float)W, vmax = (float)H;
    if (bbox2d) {
      umin = bbox2d[(size_t)n * 4 + 0]; vmin = bbox2d[(size_t)n * 4 + 1]; umax = bbox2d[(size_t)n * 4 + 2]; vmax = bbox2d[(size_t)n * 4 + 3];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) row[kO + k] = -dot3f(T[k], T[3], T[4 + k], T[7], T[8 + k], T[11]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      row[kR + 3 * k] = T[4 * k]; row[kR + 3 * k + 1] = T[4 * k + 1]; row[kR + 3 * k + 2] = T[4 * k + 2];
    }
    row[kUmin] = umin; row[kVmin] = vmin;
    row[kAx] = (float)ow / (umax - umin);
    row[kAy] = (float)oh / (vmax - vmin);
    row[kFx] = fx; row[kFy] = fy; row[kCx] = cx; row[kCy] = cy;
    row_ok = ok ? 1 : 0;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
  const int i = bx * kBlockSide + (wave & 1) * 8 + (lane & 7);
  const int j = by * kBlockSide + (wave >> 1) * 8 + (lane >> 3);
  if (i >= ow || j >= oh) return;   // no barrier and no cross-lane operation below

  const float* R = row + kR;
  const float u = row[kUmin] + ((float)i + 0.5f) / row[kAx];
  const float v = row[kVmin] + ((float)j + 0.5f) / row[kAy];
  const float dcx = (u - row[kCx]) / row[kFx], dcy = (v - row[kCy]) / row[kFy];
  const float o[3] = {row[kO], row[kO + 1], row[kO + 2]};
  const float d[3] = {(R[0] * dcx + R[3] * dcy) + R[6], (R[1] * dcx + R[4] * dcy) + R[7], (R[2] * dcx + R[5] * dcy) + R[8]};
  const float lo[3] = {g.ox, g.oy, g.oz};
  const int dims[3] = {g.nx, g.ny, g.nz};
  const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * g.ny;

  // the ray's stretch inside the box and z_near .. z_far
  bool live = row_ok != 0;
  float z0 = z_near, z1 = z_far;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float hi = lo[a] + (float)(dims[a] - 1) * g.s;
    if (d[a] == 0.f) {
      live = live && o[a] >= lo[a] && o[a] <= hi;
    } else {
      const float t1 = (lo[a] - o[a]) / d[a], t2 = (hi - o[a]) / d[a];
      const float tmin = t1 < t2 ? t1 : t2, tmax = t1 < t2 ? t2 : t1;
      z0 = tmin > z0 ? tmin : z0;
      z1 = tmax < z1 ? tmax : z1;
    }
  }
  live = live && z0 <= z1;

  bool hit = false, have_prev = false;
  float f_prev = 0.f, z_prev = 0.f, zs = 0.f;
  if (live) {
    const float cmax[3] = {(float)(g.nx - 2), (float)(g.ny - 2), (float)(g.nz - 2)};
    for (int k = 0; k < FP_TSDF_RAYCAST_MAX_SAMPLES; ++k) {
      const float z = z0 + (float)k * step;
      if (!(z <= z1)) break;
      float c[3], fr[3];
      bool inside = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float q = ((o[a] + z * d[a]) - lo[a]) / g.s;
        c[a] = floorf(q);
        fr[a] = q - c[a];
        inside = inside && c[a] >= 0.f && c[a] <= cmax[a];
      }
      bool known = inside;
      float f = 0.f;
      if (inside) {
        const size_t base = (size_t)(int)c[2] * sz + (size_t)(int)c[1] * sy + (size_t)(int)c[0];
        float val[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const size_t at = base + (q & 1) + (q >> 1 & 1) * sy + (q >> 2) * sz;
          known = known && vol.weight[at] >= min_weight;
          val[q] = vol.tsdf[at];
        }
        f = trilinear(val, fr[0], fr[1], fr[2]);
      }
      if (!known) {
        have_prev = false;
        continue;
      }
      if (f < 0.f) {
        if (have_prev) {   // f_prev >= 0 (or NaN): a known sample below 0 ends the ray
          hit = true;
          zs = z_prev + step * (f_prev / (f_prev - f));
        }
        break;             // without a known sample before it the surface is met from behind: a miss
      }
      have_prev = true;
      f_prev = f;
      z_prev = z;
    }
  }

  const size_t px = ((size_t)n * oh + j) * ow + i;
  if (out.depth) out.depth[px] = hit ? zs : 0.f;
  if (out.xyz) {
    out.xyz[3 * px] = hit ? zs * dcx : 0.f;
    out.xyz[3 * px + 1] = hit ? zs * dcy : 0.f;
    out.xyz[3 * px + 2] = hit ? zs : 0.f;
  }
  if (!out.normal && !out.color) return;
  float nrm[3] = {0.f, 0.f, 0.f}, col[3] = {0.f, 0.f, 0.f};
  if (hit) {
    // the cell of the hit point, its index clamped to the volume's cells (a NaN goes to cell 0)
    int ci[3];
    float fr[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float q = ((o[a] + zs * d[a]) - lo[a]) / g.s;
      float cf = floorf(q);
      cf = cf >= 0.f ? cf : 0.f;
      cf = cf <= (float)(dims[a] - 2) ? cf : (float)(dims[a] - 2);
      ci[a] = (int)cf;
      fr[a] = q - cf;
    }
    const size_t base = (size_t)ci[2] * sz + (size_t)ci[1] * sy + (size_t)ci[0];
    if (out.normal) {
      float gx[8], gy[8], gz[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int dx = q & 1, dy = q >> 1 & 1, dz = q >> 2;
        const size_t at = base + dx + dy * sy + dz * sz;
        gx[q] = axis_gradient(vol.tsdf, at, 1, ci[0] + dx, g.nx);
        gy[q] = axis_gradient(vol.tsdf, at, sy, ci[1] + dy, g.ny);
        gz[q] = axis_gradient(vol.tsdf, at, sz, ci[2] + dz, g.nz);
      }
      const float n0 = trilinear(gx, fr[0], fr[1], fr[2]), n1 = trilinear(gy, fr[0], fr[1], fr[2]), n2 = trilinear(gz, fr[0], fr[1], fr[2]);
      const float len = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
      if (len > 0.f) {
        const float m0 = n0 / len, m1 = n1 / len, m2 = n2 / len;
#pragma unroll
        for (int k = 0; k < 3; ++k) nrm[k] = dot3f(R[3 * k], m0, R[3 * k + 1], m1, R[3 * k + 2], m2);
      }
    }
    if (out.color) {
      float acc[3] = {0.f, 0.f, 0.f}, accw = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int dx = q & 1, dy = q >> 1 & 1, dz = q >> 2;
        const size_t at = base + dx + dy * sy + dz * sz;
        if (vol.color_weight[at] > 0.f) {
          const float w = ((dx ? fr[0] : 1.f - fr[0]) * (dy ? fr[1] : 1.f - fr[1])) * (dz ? fr[2] : 1.f - fr[2]);
#pragma unroll
          for (int k = 0; k < 3; ++k) acc[k] = acc[k] + w * vol.color[3 * at + k];
          accw = accw + w;
        }
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) col[k] = accw > 0.f ? acc[k] / accw : 128.f;
    }
  }
  if (out.normal) {
    out.normal[3 * px] = nrm[0]; out.normal[3 * px + 1] = nrm[1]; out.normal[3 * px + 2] = nrm[2];
  }
  if (out.color) {
    out.color[3 * px] = col[0]; out.color[3 * px + 1] = col[1]; out.color[3 * px + 2] = col[2];
  }
}

}  // namespace

extern "C" int fp_tsdf_raycast(const float* tsdf, const float* weight, const float* color, const float* color_weight, int nz, int ny, int nx,
                               const float* origin, float voxel, float min_weight, const float* poses, const float* K, const float* Ks,
                               const int32_t* view, int V, const float* bbox2d, int H, int W, int N, int oh, int ow, float step, float z_near,
                               float z_far, float* depth, float* xyz, float* normal, float* out_color, void* stream) {
  const char* who = "fp_tsdf_raycast";
  FP_REQUIRE(N >= 0 && N <= 65535, "%s: N=%d outside 0..65535 (the grid limit; chunk the batch)", who, N);
  FP_REQUIRE(oh >= 1 && ow >= 1 && H >= 1 && W >= 1, "%s: sizes must be >= 1 (oh=%d, ow=%d, H=%d, W=%d)", who, oh, ow, H, W);
  FP_REQUIRE((long long)oh * ow <= (1 << 20), "%s: crop %dx%d has more than 2^20 pixels", who, oh, ow);
  FP_REQUIRE(bbox2d || (oh == H && ow == W), "%s: without bbox2d the crop is the frame: oh x ow = %d x %d but H x W = %d x %d", who, oh, ow,
             H, W);
  if (int st = recon::check_grid(who, nz, ny, nx)) return st;
  if (int st = recon::check_origin(who, origin, voxel)) return st;
  FP_REQUIRE(isfinite(step) && step > 0.f, "%s: step=%g must be finite and > 0", who, (double)step);
  FP_REQUIRE(isfinite(z_near) && z_near >= 0.f, "%s: z_near=%g must be finite and >= 0", who, (double)z_near);
  FP_REQUIRE(isfinite(z_far) && z_far >= z_near, "%s: z_far=%g must be finite and >= z_near=%g", who, (double)z_far, (double)z_near);
  if (int st = recon::check_min_weight(who, min_weight)) return st;
  {
    const double ex = nx - 1, ey = ny - 1, ez = nz - 1;
    const double samples = sqrt(ex * ex + ey * ey + ez * ez) * (double)voxel / (double)step;
    FP_REQUIRE(samples <= (double)(FP_TSDF_RAYCAST_MAX_SAMPLES - 2),
               "%s: step=%g gives up to %.0f samples along the volume's diagonal, more than %d: use a longer step", who, (double)step, samples,
               FP_TSDF_RAYCAST_MAX_SAMPLES - 2);
  }
  FP_REQUIRE(tsdf && weight && color && color_weight, "%s: NULL volume array", who);
  FP_REQUIRE(depth || xyz || normal || out_color, "%s: every output is NULL", who);
  FP_REQUIRE((K != nullptr) != (Ks != nullptr), "%s: exactly one of K (one camera, on the host) and Ks (the view table) must be given", who);
  Camera cam{};
  if (K) {
    FP_REQUIRE(view == nullptr, "%s: a view index needs the Ks table", who);
    FP_REQUIRE(K[1] == 0.f, "%s: K has a skew of %g; the rays are defined without one", who, (double)K[1]);
#pragma unroll
    for (int k = 0; k < 9; ++k) cam.K1.v[k] = K[k];
    cam.vt = fp_views{nullptr, nullptr, 0};
  } else {
    FP_REQUIRE(V >= 1, "%s: V=%d views in the table (need >= 1)", who, V);
    FP_REQUIRE(view || V == 1, "%s: view is NULL but there are %d views", who, V);
    cam.vt = fp_views{Ks, view, V};
  }
  if (N == 0) return FP_OK;
  FP_REQUIRE(poses, "%s: NULL poses", who);
  const Volume vol{tsdf, weight, color, color_weight, recon::Grid{nz, ny, nx, origin[0], origin[1], origin[2], voxel}};
  const int tiles_x = fp_cdiv(ow, kBlockSide), tiles_y = fp_cdiv(oh, kBlockSide);
  hipLaunchKernelGGL(k_tsdf_raycast, dim3((unsigned)(tiles_x * tiles_y), (unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, vol, min_weight,
                     poses, cam, bbox2d, H, W, oh, ow, step, z_near, z_far, tiles_x, RayOut{depth, xyz, normal, out_color});
  FP_CHECK_LAUNCH(who);
  return FP_OK;
}
