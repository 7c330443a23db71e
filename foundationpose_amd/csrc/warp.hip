// Observed-frame crop kernel (B side): replaces the kornia warp_perspective call sites
// (predict_pose_refine.py:63,72 ; predict_score.py:89-90), the dataset normalisation
// (h5_dataset.py:79-114 refine, :137-170 score incl. the depth -> frame -> xyz -> crop chain) and the
// channel concat (predict_pose_refine.py:188).  The warp is always scale+translate, so the source
// coordinates are affine in (i, j); one lane per output pixel, consecutive lanes = consecutive i, which makes
// both the frame reads (a few adjacent texels per wave, L2 resident: the frame is 3.7 MB) and the planar
// NCHW stores coalesced.  Compiled with -ffp-contract=off (definition shared with oracle/fp_oracle.c).
#include <hip/hip_fp16.h>
#include "fp_common.h"
#include "crop_map.h"

struct __attribute__((aligned(4))) f3 { float x, y, z; };   // 12-byte texel, dword aligned: one global_load_dwordx3

// One output pixel: returns the 6 network channels (rgb/255 bilinear, xyz nearest + normalisation).
template <int MODE>
__device__ __forceinline__ void warp_pixel(const float* __restrict__ rgb, const float* __restrict__ xyz_map,
                                           const float* __restrict__ depthf, float sx, float tx, float sy, float ty,
                                           float i00, float i02, float i11, float i12, float cW, float cH, const fp_k9& K,
                                           float t0, float t1, float t2, float inv_r, bool normalize, int H, int W, int oh,
                                           int ow, int i, int j, float a[6]) {
  float ix, iy;
  crop_to_frame(i, j, i00, i02, i11, i12, cW, cH, ix, iy);
  // ---- rgb, bilinear with zero padding (tap order nw, ne, sw, se as torch grid_sample)
  {
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    // A window with an infinite (or, beyond 2^31 px, merely huge) offset saturates the conversion at INT_MAX.  x0 + 1 in int is then
    // signed overflow, undefined: the compiler tested x1 >= 0 as x0 > -2 and x1 < W on the wrapped sum, found the tap inside the frame
    // and loaded from 2^31 texels past it (an illegal address).  The unsigned sum wraps by definition, so x1 = INT_MIN fails x1 >= 0.
    const int x0 = (int)fx0, y0 = (int)fy0, x1 = (int)((unsigned)x0 + 1u), y1 = (int)((unsigned)y0 + 1u);
    const float wnw = ((float)x1 - ix) * ((float)y1 - iy);
    const float wne = (ix - (float)x0) * ((float)y1 - iy);
    const float wsw = ((float)x1 - ix) * (iy - (float)y0);
    const float wse = (ix - (float)x0) * (iy - (float)y0);
    const bool vx0 = x0 >= 0 && x0 < W, vx1 = x1 >= 0 && x1 < W;
    const bool vy0 = y0 >= 0 && y0 < H, vy1 = y1 >= 0 && y1 < H;
    // one 12-byte load per tap (the frame is AoS rgb): the kernel is bound by the number of gather instructions the
    // texture addresser has to walk, not by bytes -- 5 wide loads per pixel instead of 15 dword loads
    f3 tnw = {0.f, 0.f, 0.f}, tne = tnw, tsw = tnw, tse = tnw;
    if (vx0 && vy0) tnw = *reinterpret_cast<const f3*>(rgb + ((size_t)y0 * W + x0) * 3);
    if (vx1 && vy0) tne = *reinterpret_cast<const f3*>(rgb + ((size_t)y0 * W + x1) * 3);
    if (vx0 && vy1) tsw = *reinterpret_cast<const f3*>(rgb + ((size_t)y1 * W + x0) * 3);
    if (vx1 && vy1) tse = *reinterpret_cast<const f3*>(rgb + ((size_t)y1 * W + x1) * 3);
    const float nw3[3] = {tnw.x, tnw.y, tnw.z}, ne3[3] = {tne.x, tne.y, tne.z}, sw3[3] = {tsw.x, tsw.y, tsw.z}, se3[3] = {tse.x, tse.y, tse.z};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float acc = 0.f;                             // same order and the same skipped taps as before: an absent tap adds nothing
      if (vx0 && vy0) acc += nw3[c] * wnw;
      if (vx1 && vy0) acc += ne3[c] * wne;
      if (vx0 && vy1) acc += sw3[c] * wsw;
      if (vx1 && vy1) acc += se3[c] * wse;
      a[c] = acc * (1.0f / 255.0f);  // torch GPU `/255.0` = mul by f32 reciprocal
    }
  }
  // ---- xyz, nearest
  float pt[3] = {0.f, 0.f, 0.f};
  const int qx = nn_index(ix), qy = nn_index(iy);
  const bool q_in = qx >= 0 && qx < W && qy >= 0 && qy < H;
  if (MODE == FP_MODE_REFINE) {
    if (q_in) {
      const f3 s = *reinterpret_cast<const f3*>(xyz_map + ((size_t)qy * W + qx) * 3);
      pt[0] = s.x; pt[1] = s.y; pt[2] = s.z;
    }
  } else if (q_in) {
    const float cSw = (float)ow / (float)(ow - 1), cSh = (float)oh / (float)(oh - 1);
    // integer window edge => s*(q - left): exactly 0 on the edge, so the -0.5 tie of hop 2 is deterministic
    const float lfx = rintf(i02), lfy = rintf(i12);
    const float ccx = (fabsf(i02 - lfx) <= 1e-3f) ? sx * ((float)qx - lfx) : fmaf(sx, (float)qx, tx);
    const float ccy = (fabsf(i12 - lfy) <= 1e-3f) ? sy * ((float)qy - lfy) : fmaf(sy, (float)qy, ty);
    const int px = nn_index(fmaf(ccx, cSw, -0.5f)), py = nn_index(fmaf(ccy, cSh, -0.5f));
    float z = 0.f;
    if (px >= 0 && px < ow && py >= 0 && py < oh) {
      const float xs2 = fmaf((float)px, i00, i02), ys2 = fmaf((float)py, i11, i12);
      const int rx = nn_index(fmaf(xs2, cW, -0.5f)), ry = nn_index(fmaf(ys2, cH, -0.5f));
      if (rx >= 0 && rx < W && ry >= 0 && ry < H) z = depthf[(size_t)ry * W + rx];
    }
    if (!(z < 0.001f)) {
      pt[0] = (((float)qx - K.v[2]) * z) / K.v[0];
      pt[1] = (((float)qy - K.v[5]) * z) / K.v[4];
      pt[2] = z;
    }
  }
  const float thr = (MODE == FP_MODE_SCORE) ? 0.1f : 0.001f;
  const bool invalid = pt[2] < thr;
  const float d[3] = {pt[0] - t0, pt[1] - t1, pt[2] - t2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float val = d[c];
    if (normalize) {
      val = val * inv_r;
      if (invalid || fabsf(val) >= 2.0f) val = 0.f;
    }
    a[3 + c] = val;
  }
}

// One lane per output pixel, consecutive lanes = consecutive pixels of a row (coalesced plane stores).  Measured on
// MI355X: giving a lane 8 pixels (16-byte stores) is 4x SLOWER (0.34 ms vs 0.08 ms at N=252) -- the kernel is bound by
// the gather of the 12-byte AoS frame texels through the vector L1 (about 23 cache lines per wave-load), not by its
// stores, and fewer, fatter lanes only remove the parallelism that hides that latency.
// Per-hypothesis constants of the warp (the inverse of the scale + translate crop transform): four IEEE divisions that
// every lane of a workgroup used to repeat (~45 of its 319 VALU instructions per wave, profiles/r03_stage_counters_sq.json:
// the kernel is VALU-issue-bound, 57 % of its wave cycles are issue stalls); now one lane computes them -- the same
// instructions, so the same bits -- and the workgroup reads them from LDS.  The frame constants W/(W-1), H/(H-1) and the
// row / column of a pixel (an emulated integer division) come from the host: float division there is the same IEEE
// operation, the integer division a multiply-shift.
// (WarpConst and warp_const: crop_map.h)

// Per-object diameters (fp_warp_crops with a diameter table, MULTI = true): the same lane also computes 1 / (d / 2) of the
// hypothesis' object, d = diam[obj[n]] rounded to float -- the host expression of the scalar form (IEEE division, no contraction:
// the same bits).
struct WarpObjects { const double* diam; const int32_t* obj; int M; };

// Several views (fp_warp_crops with a view table, VIEWS = true, always with MULTI): hypothesis n reads frame view[n] of the
// (V, H, W, C) stacks and K = Ks[view[n]].  n = blockIdx.y, so the index and the 9 floats come in with uniform scalar loads, once per wave.  An index
// outside 0..V-1 reads nothing: the bounds of the frame become 0 x 0, so every pixel gets what a pixel outside the frame gets.
template <int MODE, bool MULTI, typename... VT>
__global__ __launch_bounds__(256) void k_warp(const float* __restrict__ rgb, const float* __restrict__ xyz_map,
                                              const float* __restrict__ depthf, const float* __restrict__ tfs,
                                              fp_k9 K1, const float* __restrict__ poses, float inv_r1, int flags,
                                              int H, int W, int oh, int ow, void* __restrict__ Bout, WarpConst wc,
                                              WarpObjects objs, VT... vts) {
  constexpr bool VIEWS = sizeof...(VT) > 0;
  const fp_views vt = fp_views_of(vts...);
  __shared__ float inv_tf[5];   // [4]: 1 / radius (MULTI)
  const int n = blockIdx.y;
  const float* tf = tfs + (size_t)n * 9;
  const float sx = tf[0], tx = tf[2], sy = tf[4], ty = tf[5];
  if (threadIdx.x == 0) {
    crop_inverse(sx, tx, sy, ty, inv_tf);
    if (MULTI) {
      const int o = objs.obj ? objs.obj[n] : 0;
      const float d = (unsigned)o < (unsigned)objs.M ? (float)objs.diam[o] : __builtin_nanf("");
      inv_tf[4] = 1.0f / (d * 0.5f);
    }
  }
  __syncthreads();
  const float inv_r = MULTI ? inv_tf[4] : inv_r1;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int npx = oh * ow;
  if (p >= npx) return;
  const int j = wc.mul_ow ? (int)(__umulhi((unsigned)p, wc.mul_ow) >> wc.shr_ow) : p;
  const int i = p - j * ow;
  const float i00 = inv_tf[0], i11 = inv_tf[1], i02 = inv_tf[2], i12 = inv_tf[3];
  const float cW = wc.cW, cH = wc.cH;
  const float* P = poses + (size_t)n * 16;
  fp_k9 Kv;
  int Hv = H, Wv = W;
  if (VIEWS) {
    const int v = fp_view_of(vt, n);
    Kv = fp_view_K<fp_k9, float>(vt, v);
    if (v < 0) {
      Hv = 0; Wv = 0;
    } else {
      const size_t px = (size_t)v * H * W;
      rgb += px * 3;
      if (MODE == FP_MODE_REFINE) xyz_map += px * 3;
      else depthf += px;
    }
  }
  const fp_k9& K = VIEWS ? Kv : K1;   // single view: the kernel argument itself, as before
  float a[6];
  warp_pixel<MODE>(rgb, xyz_map, depthf, sx, tx, sy, ty, i00, i02, i11, i12, cW, cH, K, P[3], P[7], P[11], inv_r,
                   (flags & FP_FLAG_NORMALIZE_XYZ) != 0, Hv, Wv, oh, ow, i, j, a);
  const size_t o = (size_t)n * 6 * npx + p;
  if (flags & FP_FLAG_OUT_F16) {
    __half* B = reinterpret_cast<__half*>(Bout);
#pragma unroll
    for (int c = 0; c < 6; ++c) B[o + (size_t)c * npx] = __float2half_rn(a[c]);
  } else {
    float* B = reinterpret_cast<float*>(Bout);
#pragma unroll
    for (int c = 0; c < 6; ++c) B[o + (size_t)c * npx] = a[c];
  }
}

template <bool MULTI, bool VIEWS = false>
static int warp_launch(const char* name, const float* rgb, const float* xyz_map, const float* depth, const float* tf_to_crops,
                       const float* K9, const float* poses, float inv_r, const WarpObjects& objs, int flags, int mode, int H,
                       int W, int N, int oh, int ow, void* B, void* stream, const fp_views& vt) {
  FP_REQUIRE(rgb && tf_to_crops && (K9 || VIEWS) && poses && B, "%s: NULL tensor", name);
  FP_REQUIRE(H > 1 && W > 1 && oh > 1 && ow > 1, "%s: degenerate sizes", name);
  FP_REQUIRE(N <= 65535, "%s: N=%d exceeds the grid limit; chunk the batch", name, N);
  FP_REQUIRE(mode == FP_MODE_REFINE || mode == FP_MODE_SCORE, "%s: unknown mode %d", name, mode);
  FP_REQUIRE(mode != FP_MODE_REFINE || xyz_map, "%s: REFINE mode needs xyz_map", name);
  FP_REQUIRE(mode != FP_MODE_SCORE || depth, "%s: SCORE mode needs depth", name);
  fp_k9 K = {};
  if (!VIEWS)
    for (int i = 0; i < 9; ++i) K.v[i] = K9[i];
  dim3 grid(fp_cdiv(oh * ow, 256), N), block(256);
  const WarpConst wc = warp_const(H, W, ow);
  if constexpr (VIEWS) {
    if (mode == FP_MODE_REFINE)
      hipLaunchKernelGGL((k_warp<FP_MODE_REFINE, MULTI, fp_views>), grid, block, 0, (hipStream_t)stream, rgb, xyz_map, depth,
                         tf_to_crops, K, poses, inv_r, flags, H, W, oh, ow, B, wc, objs, vt);
    else
      hipLaunchKernelGGL((k_warp<FP_MODE_SCORE, MULTI, fp_views>), grid, block, 0, (hipStream_t)stream, rgb, xyz_map, depth,
                         tf_to_crops, K, poses, inv_r, flags, H, W, oh, ow, B, wc, objs, vt);
  } else if (mode == FP_MODE_REFINE) {
    hipLaunchKernelGGL((k_warp<FP_MODE_REFINE, MULTI>), grid, block, 0, (hipStream_t)stream, rgb, xyz_map, depth, tf_to_crops,
                       K, poses, inv_r, flags, H, W, oh, ow, B, wc, objs);
  } else {
    hipLaunchKernelGGL((k_warp<FP_MODE_SCORE, MULTI>), grid, block, 0, (hipStream_t)stream, rgb, xyz_map, depth, tf_to_crops,
                       K, poses, inv_r, flags, H, W, oh, ow, B, wc, objs);
  }
  FP_CHECK_LAUNCH(name);
  return FP_OK;
}

extern "C" int fp_warp_crops(const float* rgb, const float* xyz_map, const float* depth, const float* tf_to_crops,
                             const float* K, const float* Ks, const int32_t* view, int V, const float* poses,
                             float mesh_diameter, const double* diameters, const int32_t* obj, int M, int flags, int mode, int H,
                             int W, int N, int oh, int ow, void* B, void* stream) {
  const char* name = "fp_warp_crops";
  const bool objects = fp_has_objects(diameters, obj, M), views = fp_has_views(Ks, view, V);
  FP_REQUIRE(N >= 0, "%s: N < 0", name);
  FP_REQUIRE((flags & ~(FP_FLAG_NORMALIZE_XYZ | FP_FLAG_OUT_F16)) == 0, "%s: unknown flag bits 0x%x", name,
             flags & ~(FP_FLAG_NORMALIZE_XYZ | FP_FLAG_OUT_F16));
  if (objects) if (const int st = fp_check_objects(name, diameters, obj, M)) return st;
  if (views) if (const int st = fp_check_views(name, K, Ks, view, V, objects)) return st;
  if (N == 0) return FP_OK;
  FP_REQUIRE(K || views, "%s: neither K nor a view table (Ks) is given", name);
  const float inv_r = objects ? 0.f : 1.0f / (mesh_diameter * 0.5f);
  const WarpObjects objs = {diameters, obj, M};
  const fp_views vt = {Ks, view, V};
  return FP_LAUNCH_FORM(objects, views, warp_launch, name, rgb, xyz_map, depth, tf_to_crops, K, poses, inv_r, objs, flags, mode,
                        H, W, N, oh, ow, B, stream, vt);
}

// fp_depth_agreement: the render's depth of hypothesis n against the observed z the REFINE warp reads for the same crop pixel (the
// nearest texel of frame view[n]'s xyz map through crop_inverse / crop_to_frame / nn_index, 0 outside the frame), classified per pixel
// and counted per hypothesis: [model, valid, agree, behind] (include/fp_amd.h).  Grid and lanes as k_warp: one lane per crop pixel,
// n = blockIdx.y.  Each wave counts its pixels with a ballot, the workgroup sums its waves through LDS, and four lanes add the sums
// with one integer atomic each: integer addition is associative, so the counts are exact and the same on every replay whatever order
// the workgroups finish in.  An index outside 0..V-1 reads nothing (z_o = 0 everywhere: only `model` counts).
constexpr int kAgreeWaves = 256 / 64;

__global__ __launch_bounds__(256) void k_depth_agreement(const float* __restrict__ depth_crops, const float* __restrict__ xyz_map,
                                                         const float* __restrict__ tfs, fp_views vt, int H, int W, int oh, int ow,
                                                         float tol, WarpConst wc, int32_t* __restrict__ counts) {
  __shared__ float inv_tf[4];
  __shared__ int part[4][kAgreeWaves];   // [count][wave]
  const int n = blockIdx.y;
  if (threadIdx.x == 0) {
    const float* tf = tfs + (size_t)n * 9;
    crop_inverse(tf[0], tf[2], tf[4], tf[5], inv_tf);
  }
  __syncthreads();
  const int npx = oh * ow;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int v = fp_view_of(vt, n);
  bool model = false, valid = false, agree = false, behind = false;
  if (p < npx) {   // no early return: every lane of the workgroup takes part in the ballots and the barrier below
    const int j = wc.mul_ow ? (int)(__umulhi((unsigned)p, wc.mul_ow) >> wc.shr_ow) : p;
    const int i = p - j * ow;
    const float zr = depth_crops[(size_t)n * npx + p];
    float ix, iy;
    crop_to_frame(i, j, inv_tf[0], inv_tf[2], inv_tf[1], inv_tf[3], wc.cW, wc.cH, ix, iy);
    const int qx = nn_index(ix), qy = nn_index(iy);
    float zo = 0.f;
    if (v >= 0 && qx >= 0 && qx < W && qy >= 0 && qy < H) zo = xyz_map[(((size_t)v * H + qy) * W + qx) * 3 + 2];
    const float d = zo - zr;
    model = zr > 0.f;
    valid = model && zo >= 0.001f;
    agree = valid && fabsf(d) <= tol;
    behind = valid && d > tol;
  }
  const unsigned long long bm = __ballot(model), bv = __ballot(valid), ba = __ballot(agree), bb = __ballot(behind);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[0][wave] = __popcll(bm);
    part[1][wave] = __popcll(bv);
    part[2][wave] = __popcll(ba);
    part[3][wave] = __popcll(bb);
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < kAgreeWaves; ++w) s += part[threadIdx.x][w];
    if (s) atomicAdd(counts + (size_t)n * 4 + threadIdx.x, s);
  }
}

extern "C" int fp_depth_agreement(const float* depth_crops, const float* xyz_map, const float* tf_to_crops, const int32_t* view, int V,
                                  int H, int W, int N, int oh, int ow, float tol, int32_t* counts, void* stream) {
  FP_REQUIRE(N >= 0 && N <= 65535, "fp_depth_agreement: N=%d outside 0..65535 (the grid limit; chunk the batch)", N);
  FP_REQUIRE(oh >= 1 && ow >= 1 && H >= 1 && W >= 1 && V >= 1,
             "fp_depth_agreement: sizes must be >= 1 (oh=%d, ow=%d, H=%d, W=%d, V=%d)", oh, ow, H, W, V);
  FP_REQUIRE((long long)oh * ow <= (1 << 20), "fp_depth_agreement: crop %dx%d has more than 2^20 pixels", oh, ow);
  FP_REQUIRE(view || V == 1, "fp_depth_agreement: view is NULL but there are %d views", V);
  FP_REQUIRE(tol >= 0.f && __builtin_isfinite(tol), "fp_depth_agreement: tol=%g must be finite and >= 0", (double)tol);
  FP_REQUIRE(xyz_map && ((depth_crops && tf_to_crops && counts) || N == 0), "fp_depth_agreement: NULL tensor");
  if (N == 0) return FP_OK;
  const hipError_t e = hipMemsetAsync(counts, 0, (size_t)N * 4 * sizeof(int32_t), (hipStream_t)stream);
  if (e != hipSuccess) {
    fp_set_error("fp_depth_agreement: zeroing the counts failed: %s", hipGetErrorString(e));
    return FP_ERR_LAUNCH;
  }
  const fp_views vt = {nullptr, view, V};
  hipLaunchKernelGGL(k_depth_agreement, dim3(fp_cdiv(oh * ow, 256), N), dim3(256), 0, (hipStream_t)stream, depth_crops, xyz_map,
                     tf_to_crops, vt, H, W, oh, ow, tol, warp_const(H, W, ow), counts);
  FP_CHECK_LAUNCH("fp_depth_agreement");
  return FP_OK;
}
