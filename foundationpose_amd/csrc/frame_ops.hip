// Per-frame and per-hypothesis small ops: depth erosion / bilateral filter / back-projection,
// crop windows, pose update.  All HBM-trivial; one thread per pixel or per pose.
// Compiled with -ffp-contract=off so the operation order matches the definition in DESIGN.md.
#include <climits>

#include "fp_common.h"

// ---------------------------------------------------------------- a1 (Utils.py:359-384)
// FRAMES (the *_frames entry points): frame blockIdx.z of a (V, H, W) stack, the same arithmetic per frame
template <bool FRAMES>
__global__ void k_erode(const float* __restrict__ depth, float* __restrict__ out, int H, int W, int radius,
                        float diff_thres, float ratio_thres, float zfar) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  const int h = blockIdx.y * blockDim.y + threadIdx.y;
  if (w >= W || h >= H) return;
  if (FRAMES) {
    depth += (size_t)blockIdx.z * H * W;
    out += (size_t)blockIdx.z * H * W;
  }
  const float d0 = depth[h * W + w];
  float bad = 0.f, total = 0.f;
  for (int u = w - radius; u <= w + radius; ++u) {
    if (u < 0 || u >= W) continue;
    for (int v = h - radius; v <= h + radius; ++v) {
      if (v < 0 || v >= H) continue;
      const float cur = depth[v * W + u];
      total += 1.0f;
      if (cur < 0.001f || cur >= zfar || fabsf(cur - d0) > diff_thres) bad += 1.0f;
    }
  }
  out[h * W + w] = (bad / total > ratio_thres) ? 0.0f : d0;
}

// ---------------------------------------------------------------- a2 (Utils.py:304-343)
template <bool FRAMES>
__global__ void k_bilateral(const float* __restrict__ depth, float* __restrict__ out, int H, int W, int radius,
                            float zfar, float sigmaD, float sigmaR) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  const int h = blockIdx.y * blockDim.y + threadIdx.y;
  if (w >= W || h >= H) return;
  if (FRAMES) {
    depth += (size_t)blockIdx.z * H * W;
    out += (size_t)blockIdx.z * H * W;
  }
  float res = 0.f, mean = 0.f;
  int nvalid = 0;
  for (int u = w - radius; u <= w + radius; ++u) {
    if (u < 0 || u >= W) continue;
    for (int v = h - radius; v <= h + radius; ++v) {
      if (v < 0 || v >= H) continue;
      const float cur = depth[v * W + u];
      if (cur >= 0.001f && cur < zfar) { nvalid++; mean += cur; }
    }
  }
  if (nvalid > 0) {
    mean /= (float)nvalid;
    const float dC = depth[h * W + w];
    const float two_sd2 = 2.0f * sigmaD * sigmaD, two_sr2 = 2.0f * sigmaR * sigmaR;
    float sw = 0.f, s = 0.f;
    for (int u = w - radius; u <= w + radius; ++u) {
      if (u < 0 || u >= W) continue;
      for (int v = h - radius; v <= h + radius; ++v) {
        if (v < 0 || v >= H) continue;
        const float cur = depth[v * W + u];
        if (cur >= 0.001f && cur < zfar && fabsf(cur - mean) < 0.01f) {
          const float a = -(float)((u - w) * (u - w) + (h - v) * (h - v)) / two_sd2;
          const float b = (dC - cur) * (dC - cur) / two_sr2;
          const float wt = expf(a - b);
          sw += wt;
          s += wt * cur;
        }
      }
    }
    if (sw > 0.f) res = s / sw;
  }
  out[h * W + w] = res;
}

// ---------------------------------------------------------------- a3 (Utils.py:399-438)
// FRAMES (a view table in the pack, its Ks the dev (V, 9) f64 table): frame blockIdx.z with K = Ks[blockIdx.z] (a uniform
// address: scalar loads)
template <typename... VT>
__global__ void k_depth_to_xyz(const float* __restrict__ depth, fp_k9d K1, float zfar, int f64_internal,
                               float* __restrict__ xyz, int H, int W, VT... vts) {
  constexpr bool FRAMES = sizeof...(VT) > 0;
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  const int v = blockIdx.y * blockDim.y + threadIdx.y;
  if (u >= W || v >= H) return;
  fp_k9d K = K1;
  if (FRAMES) {
    const double* Ks = reinterpret_cast<const double*>(fp_views_of(vts...).Ks);
    depth += (size_t)blockIdx.z * H * W;
    xyz += (size_t)blockIdx.z * H * W * 3;
#pragma unroll
    for (int i = 0; i < 9; ++i) K.v[i] = Ks[(size_t)blockIdx.z * 9 + i];
  }
  const float z = depth[v * W + u];
  float x = 0.f, y = 0.f, zz = 0.f;
  if (f64_internal) {
    if (!(z < 0.001f)) {
      const double zd = (double)z;
      x = (float)(((double)u - K.v[2]) * zd / K.v[0]);
      y = (float)(((double)v - K.v[5]) * zd / K.v[4]);
      zz = z;
    }
  } else {
    if (!(z < 0.001f || z > zfar)) {
      const float fx = (float)K.v[0], fy = (float)K.v[4], cx = (float)K.v[2], cy = (float)K.v[5];
      x = (((float)u - cx) * z) / fx;
      y = (((float)v - cy) * z) / fy;
      zz = z;
    }
  }
  float* o = xyz + (size_t)(v * W + u) * 3;
  o[0] = x; o[1] = y; o[2] = zz;
}

// ---------------------------------------------------------------- a5+a6 (Utils.py:577-621, float64 internals)
// per-object diameters (a call with a diameter table): diam[obj[n]] (obj NULL: diam[0]); an index outside 0..M-1 reads as NaN
__device__ __forceinline__ double diameter_of(const double* __restrict__ diam, const int32_t* __restrict__ obj, int M, int n) {
  const int o = obj ? obj[n] : 0;
  return (unsigned)o < (unsigned)M ? diam[o] : __builtin_nan("");
}

// MULTI: the radius of hypothesis n is diam[obj[n]] * crop_ratio / 2, the expression fp_crop_windows evaluates on the host for
// its scalar form (f64, no contraction: the same bits); otherwise `radius`.  VIEWS: K of hypothesis n = the f64 table entry of
// view[n] (one lane per hypothesis: a per-lane read); an index outside 0..V-1 gives NaN K, so NaN windows
template <bool MULTI, typename... VT>
__global__ void k_crop_windows(const float* __restrict__ poses, fp_k9d K1, double radius1, const double* __restrict__ diam,
                               const int32_t* __restrict__ obj, int M, double crop_ratio, int out_w, int out_h,
                               int N, float* __restrict__ tfs, float* __restrict__ bbox, VT... vts) {
  constexpr bool VIEWS = sizeof...(VT) > 0;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const fp_views vt = fp_views_of(vts...);
  const fp_k9d K = VIEWS ? fp_view_K<fp_k9d, double>(vt, fp_view_of(vt, n)) : K1;
  const double radius = MULTI ? diameter_of(diam, obj, M, n) * crop_ratio / 2.0 : radius1;
  const float* P = poses + (size_t)n * 16;
  const double tx = (double)P[3], ty = (double)P[7], tz = (double)P[11];
  double u0 = 0.0, v0 = 0.0, rad = 0.0;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const double ox = (k == 1) ? radius : ((k == 2) ? -radius : 0.0);
    const double oy = (k == 3) ? radius : ((k == 4) ? -radius : 0.0);
    const double x = tx + ox, y = ty + oy, z = tz;
    const double px = (K.v[0] * x + K.v[1] * y) + K.v[2] * z;
    const double py = (K.v[3] * x + K.v[4] * y) + K.v[5] * z;
    const double pz = (K.v[6] * x + K.v[7] * y) + K.v[8] * z;
    const double u = px / pz, v = py / pz;
    if (k == 0) { u0 = u; v0 = v; }
    const double a = fabs(u - u0), b = fabs(v - v0);
    rad = fmax(rad, fmax(a, b));
  }
  const double left = nearbyint(u0 - rad), right = nearbyint(u0 + rad);
  const double top = nearbyint(v0 - rad), bottom = nearbyint(v0 + rad);
  const float sx = (float)((double)out_w / (right - left));
  const float sy = (float)((double)out_h / (bottom - top));
  const float ntx = (float)(-left), nty = (float)(-top);
  float* tf = tfs + (size_t)n * 9;
  const float t02 = sx * ntx, t12 = sy * nty;
  tf[0] = sx;  tf[1] = 0.f; tf[2] = t02;
  tf[3] = 0.f; tf[4] = sy;  tf[5] = t12;
  tf[6] = 0.f; tf[7] = 0.f; tf[8] = 1.f;
  const float i00 = 1.0f / sx, i11 = 1.0f / sy;
  const float i02 = (-t02) / sx, i12 = (-t12) / sy;
  float* bb = bbox + (size_t)n * 4;
  bb[0] = i02;
  bb[1] = i12;
  bb[2] = (i00 * (float)(out_w - 1)) + i02;
  bb[3] = (i11 * (float)(out_h - 1)) + i12;
}

// ---------------------------------------------------------------- a13 (predict_pose_refine.py:195-234)
struct fp_f3 { float v[3]; };

// MULTI: the diameter of hypothesis n is diam[obj[n]] rounded to float (as the scalar entry point's caller rounds it).
// VIEWS: K (deepim) of hypothesis n = the f32 table entry of view[n]; an index outside 0..V-1 writes NaN to every output row
template <bool MULTI, typename... VT>
__global__ void k_pose_update(const float* __restrict__ trans, const float* __restrict__ rot,
                              const float* __restrict__ poses_in, int rot_rep, int normalize_xyz, fp_f3 tn,
                              float rot_normalizer, float mesh_diameter1, const double* __restrict__ diam,
                              const int32_t* __restrict__ obj, int M, int N, float* __restrict__ poses_out,
                              float* __restrict__ trans_delta_out, float* __restrict__ rot_delta_out, int trans_rep, fp_k9 K1,
                              const float* __restrict__ tf_to_crops, float input_w, VT... vts) {
  constexpr bool VIEWS = sizeof...(VT) > 0;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const fp_views vt = fp_views_of(vts...);
  fp_k9 K = K1;
  if (VIEWS) {
    const int v = fp_view_of(vt, n);
    if (v < 0) {
      const float nan = __builtin_nanf("");
#pragma unroll
      for (int k = 0; k < 16; ++k) poses_out[(size_t)n * 16 + k] = nan;
      if (trans_delta_out) {
#pragma unroll
        for (int c = 0; c < 3; ++c) trans_delta_out[n * 3 + c] = nan;
      }
      if (rot_delta_out) {
#pragma unroll
        for (int c = 0; c < 9; ++c) rot_delta_out[(size_t)n * 9 + c] = nan;
      }
      return;
    }
    if (trans_rep == FP_TRANS_DEEPIM) K = fp_view_K<fp_k9, float>(vt, v);
  }
  const float mesh_diameter = MULTI ? (float)diameter_of(diam, obj, M, n) : mesh_diameter1;
  float dt[3];
  if (trans_rep == FP_TRANS_DEEPIM) {
    // predict_pose_refine.py:201-215: (trans.x, trans.y) = shift of the projected object centre in crop pixels / crop
    // width, trans.z = new depth / current depth.  tf_to_crops = [[sx,0,tx],[0,sy,ty],[0,0,1]], K upper triangular:
    // both inverses in closed form.
    const float* A = poses_in + (size_t)n * 16;
    const float* tf = tf_to_crops + (size_t)n * 9;
    const float tx = A[3], ty = A[7], tz = A[11];
    const float u = (K.v[0] * tx + K.v[1] * ty + K.v[2] * tz) / tz, v = (K.v[4] * ty + K.v[5] * tz) / tz;
    const float uc = tf[0] * u + tf[1] * v + tf[2], vc = tf[3] * u + tf[4] * v + tf[5];
    const float z_pred = trans[n * 3 + 2] * tz;
    const float ucp = uc + trans[n * 3] * input_w, vcp = vc + trans[n * 3 + 1] * input_w;
    const float vp = (vcp - tf[5]) / tf[4];
    const float up = ((ucp - tf[2]) - tf[1] * vp) / tf[0];
    const float yn = (vp - K.v[5]) / K.v[4];
    const float xn = ((up - K.v[2]) - K.v[1] * yn) / K.v[0];
    dt[0] = xn * z_pred - tx; dt[1] = yn * z_pred - ty; dt[2] = z_pred - tz;
    if (normalize_xyz) {
#pragma unroll
      for (int c = 0; c < 3; ++c) dt[c] *= (mesh_diameter / 2.0f);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = trans[n * 3 + c];
      // 'tracknet' (:195-199) squashes the raw output only when the crops are NOT normalised; any other trans_rep is the
      // plain `else` (:217-218): the raw output.  With normalize_xyz the two coincide (:232-233).
      if (!normalize_xyz) v = (trans_rep == FP_TRANS_RAW) ? v : tanhf(v) * tn.v[c];
      else v = v * (mesh_diameter / 2.0f);
      dt[c] = v;
    }
  }
  float R[9];
  if (rot_rep == FP_ROT_AXIS_ANGLE) {
    float w[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) w[c] = tanhf(rot[n * 3 + c]) * rot_normalizer;
    const float n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const float th = sqrtf(fmaxf(n2, 1e-4f));
    const float ith = 1.0f / th;
    const float f1 = ith * sinf(th);
    const float f2 = (ith * ith) * (1.0f - cosf(th));
    const float Kx[9] = {0.f, -w[2], w[1], w[2], 0.f, -w[0], -w[1], w[0], 0.f};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float k2 = (Kx[r * 3] * Kx[c] + Kx[r * 3 + 1] * Kx[3 + c]) + Kx[r * 3 + 2] * Kx[6 + c];
        R[r * 3 + c] = (f1 * Kx[r * 3 + c] + f2 * k2) + ((r == c) ? 1.0f : 0.0f);
      }
  } else {
    const float* d = rot + (size_t)n * 6;
    const float a1[3] = {d[0], d[1], d[2]}, a2[3] = {d[3], d[4], d[5]};
    const float l1 = fmaxf(sqrtf((a1[0] * a1[0] + a1[1] * a1[1]) + a1[2] * a1[2]), 1e-12f);
    const float b1[3] = {a1[0] / l1, a1[1] / l1, a1[2] / l1};
    const float dp = (b1[0] * a2[0] + b1[1] * a2[1]) + b1[2] * a2[2];
    const float u2[3] = {a2[0] - dp * b1[0], a2[1] - dp * b1[1], a2[2] - dp * b1[2]};
    const float l2 = fmaxf(sqrtf((u2[0] * u2[0] + u2[1] * u2[1]) + u2[2] * u2[2]), 1e-12f);
    const float b2[3] = {u2[0] / l2, u2[1] / l2, u2[2] / l2};
    const float b3[3] = {b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]};
#pragma unroll
    for (int c = 0; c < 3; ++c) { R[c] = b1[c]; R[3 + c] = b2[c]; R[6 + c] = b3[c]; }
  }
  const float* A = poses_in + (size_t)n * 16;
  float* O = poses_out + (size_t)n * 16;
  float o[16];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      o[r * 4 + c] = (R[0 * 3 + r] * A[0 * 4 + c] + R[1 * 3 + r] * A[1 * 4 + c]) + R[2 * 3 + r] * A[2 * 4 + c];
    o[r * 4 + 3] = A[r * 4 + 3] + dt[r];
  }
  o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) O[k] = o[k];
  // what the reference keeps as last_trans_update / last_rot_update (predict_pose_refine.py:238-239): the metric
  // translation delta and the applied rotation so3_exp_map(w)^T
  if (trans_delta_out) {
#pragma unroll
    for (int c = 0; c < 3; ++c) trans_delta_out[n * 3 + c] = dt[c];
  }
  if (rot_delta_out) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) rot_delta_out[(size_t)n * 9 + r * 3 + c] = R[c * 3 + r];
  }
}

// ---------------------------------------------------------------- a14 (estimater.py:137-156 guess_translation, :164-166)
// Per mask: the bounding box of its pixels, the count n of its valid depths (d >= min_depth) and the (n-1)//2-th and n//2-th
// smallest of them, exactly the elements torch.sort puts there.  One workgroup per mask.  Pass 1 reads the whole mask for the box
// and n; then an exact radix select (four 8-bit digits, most significant first) over the box: valid depths are positive floats, so
// their bit patterns order as uint32 (+inf last), and both ranks are found in the same passes with one LDS histogram each.
// out[m] = {v0, v1, u0, u1, n, bits(lo), bits(hi), 0}: -1 for the box of an empty mask, NaN for lo / hi when n == 0.  A view index
// outside 0..V-1 reads nothing and reports an empty mask.
#define MDS_THREADS 1024
__device__ __forceinline__ void mds_visit(const uint8_t* __restrict__ mk, const float* __restrict__ dp, int i, float min_depth,
                                          int W, int& rmin, int& rmax, int& cmin, int& cmax, int& cnt) {
  if (!mk[i]) return;
  const int r = i / W, c = i - r * W;
  rmin = min(rmin, r); rmax = max(rmax, r); cmin = min(cmin, c); cmax = max(cmax, c);
  cnt += dp[i] >= min_depth;
}

__global__ __launch_bounds__(MDS_THREADS) void k_mask_depth_stats(const float* __restrict__ depth, const uint8_t* __restrict__ masks,
                                                                  const int32_t* __restrict__ view, int V, int H, int W,
                                                                  float min_depth, int32_t* __restrict__ out) {
  __shared__ int red[MDS_THREADS / 64][5];
  __shared__ unsigned hist[2][256];
  __shared__ unsigned sel[2][2];            // per rank: the digits found so far (prefix) and the rank left inside them
  const int m = blockIdx.x, t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int vv = view ? view[m] : 0;
  const bool ok = (unsigned)vv < (unsigned)V;
  const size_t HW = (size_t)H * W;
  const uint8_t* mk = masks + (size_t)m * HW;
  const float* dp = depth + (size_t)(ok ? vv : 0) * HW;
  int rmin = INT_MAX, rmax = -1, cmin = INT_MAX, cmax = -1, cnt = 0;
  if (ok) {
    const int n = (int)HW;
    if ((HW & 3) == 0) {                      // four mask bytes per load; rows of the masks stay 4-byte aligned
      const uint32_t* mk4 = reinterpret_cast<const uint32_t*>(mk);
      for (int q = t; q < n / 4; q += MDS_THREADS) {
        const uint32_t w4 = mk4[q];
        if (!w4) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) mds_visit(mk, dp, 4 * q + e, min_depth, W, rmin, rmax, cmin, cmax, cnt);
      }
    } else {
      for (int i = t; i < n; i += MDS_THREADS) mds_visit(mk, dp, i, min_depth, W, rmin, rmax, cmin, cmax, cnt);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    rmin = min(rmin, __shfl_xor(rmin, o, 64)); rmax = max(rmax, __shfl_xor(rmax, o, 64));
    cmin = min(cmin, __shfl_xor(cmin, o, 64)); cmax = max(cmax, __shfl_xor(cmax, o, 64));
    cnt += __shfl_xor(cnt, o, 64);
  }
  if (lane == 0) { red[wid][0] = rmin; red[wid][1] = rmax; red[wid][2] = cmin; red[wid][3] = cmax; red[wid][4] = cnt; }
  __syncthreads();
  rmin = INT_MAX; rmax = -1; cmin = INT_MAX; cmax = -1; cnt = 0;
  for (int w = 0; w < MDS_THREADS / 64; ++w) {       // every thread, in one order: all hold the same totals
    rmin = min(rmin, red[w][0]); rmax = max(rmax, red[w][1]); cmin = min(cmin, red[w][2]); cmax = max(cmax, red[w][3]);
    cnt += red[w][4];
  }
  int32_t* o = out + (size_t)m * 8;
  if (cnt == 0) {                                     // no valid depth (or an empty mask: then no box either): lo = hi = NaN
    const bool any = rmax >= 0;
    const int32_t vals[8] = {any ? rmin : -1, any ? rmax : -1, any ? cmin : -1, any ? cmax : -1, 0, 0x7fc00000, 0x7fc00000, 0};
    if (t < 8) o[t] = vals[t];
    return;
  }
  if (t < 2) {
    sel[t][0] = 0u;
    sel[t][1] = t == 0 ? (unsigned)(cnt - 1) / 2 : (unsigned)cnt / 2;
  }
  const int bw = cmax - cmin + 1;
  const int box = (rmax - rmin + 1) * bw;
  unsigned known = 0u;                                // the bits of the digits found so far
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = t; i < 512; i += MDS_THREADS) (&hist[0][0])[i] = 0u;
    __syncthreads();                                  // also publishes sel[] of the previous digit
    const unsigned p0 = sel[0][0], p1 = sel[1][0];
    for (int i = t; i < box; i += MDS_THREADS) {
      const int r = rmin + i / bw, c = cmin + i % bw;
      const size_t px = (size_t)r * W + c;
      if (!mk[px]) continue;
      const float d = dp[px];
      if (!(d >= min_depth)) continue;
      const unsigned b = __float_as_uint(d);
      if ((b & known) == p0) atomicAdd(&hist[0][(b >> shift) & 255u], 1u);
      if ((b & known) == p1) atomicAdd(&hist[1][(b >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (wid < 2) {                                    // wave k scans histogram k: four bins per lane, then an inclusive lane scan
      unsigned h[4], sum = 0u;
#pragma unroll
      for (int e = 0; e < 4; ++e) { h[e] = hist[wid][lane * 4 + e]; sum += h[e]; }
      unsigned inc = sum;
      for (int o2 = 1; o2 < 64; o2 <<= 1) {
        const unsigned y = __shfl_up(inc, o2, 64);
        if (lane >= o2) inc += y;
      }
      const unsigned k = sel[wid][1];
      unsigned before = inc - sum;
      if (k >= before && k < inc) {                   // exactly one lane holds the rank
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (k < before + h[e]) {
            sel[wid][0] |= (unsigned)(lane * 4 + e) << shift;
            sel[wid][1] = k - before;
            break;
          }
          before += h[e];
        }
      }
    }
    known |= 255u << shift;
    __syncthreads();                                  // the scan has read the histograms before the next digit clears them
  }
  if (t < 8) {
    const int32_t vals[8] = {rmin, rmax, cmin, cmax, cnt, (int32_t)sel[0][0], (int32_t)sel[1][0], 0};
    o[t] = vals[t];
  }
}

// ---------------------------------------------------------------- C ABI
extern "C" int fp_depth_erode(const float* depth, float* out, int H, int W, int radius, float diff_thres,
                              float ratio_thres, float zfar, void* stream) {
  FP_REQUIRE(depth && out && H > 0 && W > 0 && radius >= 0, "fp_depth_erode: bad arguments");
  dim3 b(64, 4), g(fp_cdiv(W, 64), fp_cdiv(H, 4));
  hipLaunchKernelGGL(k_erode<false>, g, b, 0, (hipStream_t)stream, depth, out, H, W, radius, diff_thres, ratio_thres, zfar);
  FP_CHECK_LAUNCH("fp_depth_erode");
  return FP_OK;
}

extern "C" int fp_depth_bilateral(const float* depth, float* out, int H, int W, int radius, float zfar,
                                  float sigmaD, float sigmaR, void* stream) {
  FP_REQUIRE(depth && out && H > 0 && W > 0 && radius >= 0, "fp_depth_bilateral: bad arguments");
  dim3 b(64, 4), g(fp_cdiv(W, 64), fp_cdiv(H, 4));
  hipLaunchKernelGGL(k_bilateral<false>, g, b, 0, (hipStream_t)stream, depth, out, H, W, radius, zfar, sigmaD, sigmaR);
  FP_CHECK_LAUNCH("fp_depth_bilateral");
  return FP_OK;
}

extern "C" int fp_depth_to_xyz(const float* depth, const double* K, float zfar, int f64_internal, float* xyz,
                               int H, int W, void* stream) {
  FP_REQUIRE(depth && K && xyz && H > 0 && W > 0, "fp_depth_to_xyz: bad arguments");
  fp_k9d Kd;
  for (int i = 0; i < 9; ++i) Kd.v[i] = K[i];
  dim3 b(64, 4), g(fp_cdiv(W, 64), fp_cdiv(H, 4));
  hipLaunchKernelGGL(k_depth_to_xyz<>, g, b, 0, (hipStream_t)stream, depth, Kd, zfar, f64_internal, xyz, H, W);
  FP_CHECK_LAUNCH("fp_depth_to_xyz");
  return FP_OK;
}

// the batched ingest: one launch per stage over a (V, H, W) stack, frame f = blockIdx.z
extern "C" int fp_depth_erode_frames(const float* depth, float* out, int H, int W, int V, int radius, float diff_thres,
                                     float ratio_thres, float zfar, void* stream) {
  FP_REQUIRE(V >= 1 && V <= 65535, "fp_depth_erode_frames: V=%d outside 1..65535", V);
  FP_REQUIRE(depth && out && H > 0 && W > 0 && radius >= 0, "fp_depth_erode_frames: bad arguments");
  dim3 b(64, 4), g(fp_cdiv(W, 64), fp_cdiv(H, 4), V);
  hipLaunchKernelGGL(k_erode<true>, g, b, 0, (hipStream_t)stream, depth, out, H, W, radius, diff_thres, ratio_thres, zfar);
  FP_CHECK_LAUNCH("fp_depth_erode_frames");
  return FP_OK;
}

extern "C" int fp_depth_bilateral_frames(const float* depth, float* out, int H, int W, int V, int radius, float zfar,
                                         float sigmaD, float sigmaR, void* stream) {
  FP_REQUIRE(V >= 1 && V <= 65535, "fp_depth_bilateral_frames: V=%d outside 1..65535", V);
  FP_REQUIRE(depth && out && H > 0 && W > 0 && radius >= 0, "fp_depth_bilateral_frames: bad arguments");
  dim3 b(64, 4), g(fp_cdiv(W, 64), fp_cdiv(H, 4), V);
  hipLaunchKernelGGL(k_bilateral<true>, g, b, 0, (hipStream_t)stream, depth, out, H, W, radius, zfar, sigmaD, sigmaR);
  FP_CHECK_LAUNCH("fp_depth_bilateral_frames");
  return FP_OK;
}

extern "C" int fp_depth_to_xyz_frames(const float* depth, const double* Ks, float zfar, int f64_internal, float* xyz, int H,
                                      int W, int V, void* stream) {
  FP_REQUIRE(V >= 1 && V <= 65535, "fp_depth_to_xyz_frames: V=%d outside 1..65535", V);
  FP_REQUIRE(Ks, "fp_depth_to_xyz_frames: NULL K table");
  FP_REQUIRE(depth && xyz && H > 0 && W > 0, "fp_depth_to_xyz_frames: bad arguments");
  const fp_k9d unused = {};
  const fp_views vt = {Ks, nullptr, V};
  dim3 b(64, 4), g(fp_cdiv(W, 64), fp_cdiv(H, 4), V);
  hipLaunchKernelGGL(k_depth_to_xyz<fp_views>, g, b, 0, (hipStream_t)stream, depth, unused, zfar, f64_internal, xyz, H, W, vt);
  FP_CHECK_LAUNCH("fp_depth_to_xyz_frames");
  return FP_OK;
}

// The crop stage's scene arguments (K | Ks / view / V; mesh_diameter | diameters / obj / M) are checked by fp_check_objects and
// fp_check_views (fp_common.h); FP_LAUNCH_FORM names the instantiation each form runs.
extern "C" int fp_crop_windows(const float* poses, const double* K, const double* Ks, const int32_t* view, int V,
                               double mesh_diameter, const double* diameters, const int32_t* obj, int M, double crop_ratio,
                               int out_w, int out_h, int N, float* tf_to_crops, float* bbox2d, void* stream) {
  const char* name = "fp_crop_windows";
  const bool objects = fp_has_objects(diameters, obj, M), views = fp_has_views(Ks, view, V);
  FP_REQUIRE(N >= 0, "%s: N < 0", name);
  if (objects) if (const int st = fp_check_objects(name, diameters, obj, M)) return st;
  if (views) if (const int st = fp_check_views(name, K, Ks, view, V, objects)) return st;
  if (N == 0) return FP_OK;
  FP_REQUIRE(K || views, "%s: neither K nor a view table (Ks) is given", name);
  FP_REQUIRE(poses && tf_to_crops && bbox2d && out_w > 1 && out_h > 1, "%s: bad arguments", name);
  fp_k9d Kd = {};
  if (K) for (int i = 0; i < 9; ++i) Kd.v[i] = K[i];
  // the scalar form passes its radius and no ratio, the table forms the ratio and no radius: the arguments of the three
  // instantiations are what they always were
  const double radius = objects ? 0.0 : mesh_diameter * crop_ratio / 2.0, ratio = objects ? crop_ratio : 0.0;
  const dim3 grid(fp_cdiv(N, 64)), block(64);
  const hipStream_t st = (hipStream_t)stream;
  if (!objects) {
    hipLaunchKernelGGL(k_crop_windows<false>, grid, block, 0, st, poses, Kd, radius, diameters, obj, M, ratio, out_w, out_h, N,
                       tf_to_crops, bbox2d);
  } else if (!views) {
    hipLaunchKernelGGL(k_crop_windows<true>, grid, block, 0, st, poses, Kd, radius, diameters, obj, M, ratio, out_w, out_h, N,
                       tf_to_crops, bbox2d);
  } else {
    const fp_views vt = {Ks, view, V};
    hipLaunchKernelGGL((k_crop_windows<true, fp_views>), grid, block, 0, st, poses, Kd, radius, diameters, obj, M, ratio, out_w,
                       out_h, N, tf_to_crops, bbox2d, vt);
  }
  FP_CHECK_LAUNCH(name);
  return FP_OK;
}

template <bool MULTI, bool VIEWS = false>
static int pose_update_launch(const char* name, const float* trans, const float* rot, const float* poses_in, int rot_rep,
                              int normalize_xyz, const float* trans_normalizer, float rot_normalizer, float mesh_diameter,
                              const double* diam, const int32_t* obj, int M, int N, float* poses_out, float* trans_delta_out,
                              float* rot_delta_out, int trans_rep, const float* K9, const float* tf_to_crops, float input_w,
                              void* stream, const fp_views& vt) {
  FP_REQUIRE(trans && rot && poses_in && poses_out, "%s: NULL tensor", name);
  FP_REQUIRE(rot_rep == FP_ROT_AXIS_ANGLE || rot_rep == FP_ROT_6D, "%s: unknown rot_rep %d", name, rot_rep);
  FP_REQUIRE(trans_rep == FP_TRANS_TRACKNET || trans_rep == FP_TRANS_DEEPIM || trans_rep == FP_TRANS_RAW, "%s: unknown trans_rep %d", name, trans_rep);
  FP_REQUIRE(trans_rep != FP_TRANS_DEEPIM || ((K9 || VIEWS) && tf_to_crops && input_w > 0.f),
             "%s: trans_rep deepim needs K, tf_to_crops and the crop width", name);
  fp_k9 Kk = {{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}};
  if (K9) for (int i = 0; i < 9; ++i) Kk.v[i] = K9[i];
  fp_f3 tn = {{1.f, 1.f, 1.f}};
  if (trans_normalizer) { tn.v[0] = trans_normalizer[0]; tn.v[1] = trans_normalizer[1]; tn.v[2] = trans_normalizer[2]; }
  if constexpr (VIEWS)
    hipLaunchKernelGGL((k_pose_update<MULTI, fp_views>), dim3(fp_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, trans, rot,
                       poses_in, rot_rep, normalize_xyz, tn, rot_normalizer, mesh_diameter, diam, obj, M, N, poses_out,
                       trans_delta_out, rot_delta_out, trans_rep, Kk, tf_to_crops, input_w, vt);
  else
    hipLaunchKernelGGL(k_pose_update<MULTI>, dim3(fp_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, trans, rot, poses_in,
                       rot_rep, normalize_xyz, tn, rot_normalizer, mesh_diameter, diam, obj, M, N, poses_out, trans_delta_out,
                       rot_delta_out, trans_rep, Kk, tf_to_crops, input_w);
  FP_CHECK_LAUNCH(name);
  return FP_OK;
}

extern "C" int fp_pose_update(const float* trans, const float* rot, const float* poses_in, int rot_rep, int normalize_xyz,
                              const float* trans_normalizer, float rot_normalizer, float mesh_diameter, const double* diameters,
                              const int32_t* obj, int M, int N, float* poses_out, float* trans_delta_out, float* rot_delta_out,
                              int trans_rep, const float* K, const float* Ks, const int32_t* view, int V,
                              const float* tf_to_crops, float input_w, void* stream) {
  const char* name = "fp_pose_update";
  const bool objects = fp_has_objects(diameters, obj, M), views = fp_has_views(Ks, view, V);
  FP_REQUIRE(N >= 0, "%s: N < 0", name);
  if (objects) if (const int st = fp_check_objects(name, diameters, obj, M)) return st;
  if (views) if (const int st = fp_check_views(name, K, Ks, view, V, objects)) return st;
  if (N == 0) return FP_OK;
  const fp_views vt = {Ks, view, V};
  return FP_LAUNCH_FORM(objects, views, pose_update_launch, name, trans, rot, poses_in, rot_rep, normalize_xyz, trans_normalizer,
                        rot_normalizer, objects ? 0.f : mesh_diameter, diameters, obj, M, N, poses_out, trans_delta_out,
                        rot_delta_out, trans_rep, K, tf_to_crops, input_w, stream, vt);
}

extern "C" int fp_mask_depth_stats(const float* depth, const uint8_t* masks, const int32_t* view, int V, int M, int H, int W,
                                   float min_depth, int32_t* out, void* stream) {
  FP_REQUIRE(M >= 0, "fp_mask_depth_stats: M < 0");
  if (M == 0) return FP_OK;
  FP_REQUIRE(depth && masks && out, "fp_mask_depth_stats: NULL tensor");
  FP_REQUIRE(V >= 1 && H > 0 && W > 0, "fp_mask_depth_stats: bad frame size (V=%d, H=%d, W=%d)", V, H, W);
  FP_REQUIRE(view || V == 1, "fp_mask_depth_stats: %d frames need a per-mask view index", V);
  FP_REQUIRE((long long)H * W < (1ll << 31), "fp_mask_depth_stats: H * W too large");
  FP_REQUIRE(min_depth > 0.f && min_depth < __builtin_inff(),
             "fp_mask_depth_stats: min_depth must be positive and finite (the select orders valid depths by their bits)");
  FP_REQUIRE(((size_t)H * W & 3) != 0 || ((size_t)masks & 3) == 0, "fp_mask_depth_stats: masks must be 4-byte aligned");
  hipLaunchKernelGGL(k_mask_depth_stats, dim3(M), dim3(MDS_THREADS), 0, (hipStream_t)stream, depth, masks, view, V, H, W, min_depth, out);
  FP_CHECK_LAUNCH("fp_mask_depth_stats");
  return FP_OK;
}
