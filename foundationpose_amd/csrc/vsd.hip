// The pixel counts of BOP's visible surface discrepancy (fp_vsd_counts; the definition is in include/fp_amd.h): N rendered depth maps
// of estimated poses against the render of their ground truth and the observed depth, pixel by pixel.  A pure stream: est is read
// once (N * h * w * 4 bytes), gt / obs / fac are re-read per pose out of L2 / Infinity Cache.
//   k_vsd_clear     clears the N rows of the table (the result never depends on what the table held).  A kernel and not
//                   hipMemsetAsync: captured in a hipGraph, a memset of 392 bytes (7 rows of 14) replayed with garbage in its first
//                   384 bytes on ROCm 7.2 (sizes that are multiples of 16 bytes, as fp_depth_agreement's, replay correctly)
//   k_vsd_counts    grid (chunks of kThreads * kIter pixel groups, n).  A lane owns kIter groups of kVec consecutive pixels, a group apart
//                   by kThreads so that a wave's load instruction covers 64 consecutive groups (1 KiB with kVec = 4: 16-byte loads);
//                   the kIter est and gt loads are issued before the first is used.  A group with no positive est or gt pixel counts
//                   nothing (most of a frame) and reads neither obs nor fac.  The 4 + T counters stay in registers (thresholds beyond T
//                   are NaN, which no distance reaches), a wave that counted anything adds its totals (xor tree) with one integer
//                   atomic instruction, lane k adding counter k.
// Integer sums have no order, so a row has the same values alone, in a batch and on every replay.  Compiled with -ffp-contract=off
// (SRCS_EXACT): every float32 value is the one the numpy restatement (tests/bop_errors_model.py) computes.
// Measured on an MI355X (scripts/bench_bop_errors.py): 252 maps of 480 x 640, T = 10, 9.9 % of the pixels rendered:
// 0.099 ms between events for the two launches = 313 MB that must move at 3.2 TB/s, half of the 0.050 ms floor at the 6.3 TB/s a
// streaming copy reaches; one map 0.037 ms; the float32 numpy restatement of the same pairs on the host 401 ms.
#include "fp_common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kIter = 4;               // pixel groups per lane, all in flight at once
constexpr int kC = 4 + FP_VSD_MAX_T;   // counters per lane

struct Thr { float v[FP_VSD_MAX_T]; };

struct Counters {
  int c[kC];
};

// one pixel of the definition
__device__ __forceinline__ void count_pixel(float e, float g, float o, float f, float delta, const Thr& thr, Counters& k) {
  const float Do = o * f, De = e * f, Dg = g * f;
  const bool seen = Do > 0.f;
  const bool vg = Dg > 0.f && (!seen || (Dg - Do) <= delta);
  const bool ve = (De > 0.f && (!seen || (De - Do) <= delta)) || (vg && De > 0.f);
  const bool inter = vg && ve;
  k.c[0] += vg;
  k.c[1] += ve;
  k.c[2] += inter;
  k.c[3] += vg || ve;
  if (inter) {
    const float dist = fabsf(Dg - De);
#pragma unroll
    for (int t = 0; t < FP_VSD_MAX_T; ++t) k.c[4 + t] += dist >= thr.v[t];
  }
}

template <int kVec>
struct Px;
template <>
struct Px<4> { using type = float4; };
template <>
struct Px<1> { using type = float; };

__device__ __forceinline__ bool any_positive(const float4& a) { return a.x > 0.f || a.y > 0.f || a.z > 0.f || a.w > 0.f; }
__device__ __forceinline__ bool any_positive(float a) { return a > 0.f; }
__device__ __forceinline__ float4 zero_of(const float4*) { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float zero_of(const float*) { return 0.f; }

__device__ __forceinline__ void count_group(const float4& e, const float4& g, const float4& o, const float4& f, float delta,
                                            const Thr& thr, Counters& k) {
  count_pixel(e.x, g.x, o.x, f.x, delta, thr, k);
  count_pixel(e.y, g.y, o.y, f.y, delta, thr, k);
  count_pixel(e.z, g.z, o.z, f.z, delta, thr, k);
  count_pixel(e.w, g.w, o.w, f.w, delta, thr, k);
}
__device__ __forceinline__ void count_group(float e, float g, float o, float f, float delta, const Thr& thr, Counters& k) {
  count_pixel(e, g, o, f, delta, thr, k);
}

// wg = groups per window row (w / kVec), ngroups = h * wg.  Group i of the window is at est + i * kVec and, in the frame, at pixel
// (y0 + i / wg, x0 + (i % wg) * kVec).
template <int kVec>
__global__ __launch_bounds__(kThreads) void k_vsd_counts(const float* __restrict__ est, const float* __restrict__ gt,
                                                         const int32_t* __restrict__ gt_index, int G, int wg, int ngroups,
                                                         const float* __restrict__ obs, const float* __restrict__ fac, int W, int x0,
                                                         int y0, float delta, Thr thr, int T, int32_t* __restrict__ counts) {
  using V = typename Px<kVec>::type;
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  int g = gt_index ? gt_index[n] : (G == 1 ? 0 : n);
  int32_t* row = counts + (size_t)n * (4 + T);
  if ((unsigned)g >= (unsigned)G) {   // uniform: the whole workgroup leaves; the first one marks the row
    if (blockIdx.x == 0 && threadIdx.x < 4 + T) row[threadIdx.x] = -1;
    return;
  }
  const size_t image = (size_t)ngroups * kVec;
  const V* E = reinterpret_cast<const V*>(est + (size_t)n * image);
  const V* Gt = reinterpret_cast<const V*>(gt + (size_t)g * image);
  const int base = blockIdx.x * (kThreads * kIter) + threadIdx.x;
  V e[kIter], q[kIter];
#pragma unroll
  for (int i = 0; i < kIter; ++i) {
    const int idx = base + i * kThreads;
    e[i] = idx < ngroups ? E[idx] : zero_of((const V*)nullptr);
    q[i] = idx < ngroups ? Gt[idx] : zero_of((const V*)nullptr);
  }
  Counters k;
#pragma unroll
  for (int j = 0; j < kC; ++j) k.c[j] = 0;
  bool any = false;
#pragma unroll
  for (int i = 0; i < kIter; ++i) {
    if (any_positive(e[i]) || any_positive(q[i])) {   // (a group beyond the window is zero and stops here)
      const int idx = base + i * kThreads;
      const int y = idx / wg, x = (idx - y * wg) * kVec;
      const size_t at = (size_t)(y0 + y) * W + (x0 + x);
      const V o = *reinterpret_cast<const V*>(obs + at), f = *reinterpret_cast<const V*>(fac + at);
      count_group(e[i], q[i], o, f, delta, thr, k);
      any = true;
    }
  }
  if (__ballot(any) == 0ull) return;   // wave-uniform
  int mine = 0;
#pragma unroll
  for (int j = 0; j < kC; ++j) {
    int v = k.c[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == j) mine = v;
  }
  if (lane < 4 + T && mine != 0) atomicAdd(row + lane, mine);
}

__global__ __launch_bounds__(kThreads) void k_vsd_clear(int32_t* __restrict__ counts, int n) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) counts[i] = 0;
}

}  // namespace

extern "C" int fp_vsd_counts(const float* est, const float* gt, const int32_t* gt_index, int G, int N, int h, int w, const float* obs,
                             const float* fac, int H, int W, int x0, int y0, float delta, const float* thr, int T, int32_t* counts,
                             void* stream) {
  FP_REQUIRE(N >= 0 && N <= 65535, "fp_vsd_counts: N=%d outside 0..65535 (the grid limit; chunk the batch)", N);
  FP_REQUIRE(G >= 1, "fp_vsd_counts: G=%d must be >= 1", G);
  FP_REQUIRE(T >= 1 && T <= FP_VSD_MAX_T, "fp_vsd_counts: T=%d outside 1..%d", T, FP_VSD_MAX_T);
  FP_REQUIRE(thr, "fp_vsd_counts: NULL thr");
  FP_REQUIRE(h >= 1 && w >= 1 && H >= 1 && W >= 1, "fp_vsd_counts: h=%d w=%d H=%d W=%d must be >= 1", h, w, H, W);
  FP_REQUIRE((long long)h * w <= (1ll << 28) && (long long)H * W <= (1ll << 28),
             "fp_vsd_counts: more than 2^28 pixels (window %d x %d, frame %d x %d)", h, w, H, W);
  FP_REQUIRE(x0 >= 0 && y0 >= 0 && x0 <= W - w && y0 <= H - h, "fp_vsd_counts: window %d x %d at (%d, %d) is not inside the %d x %d frame", h,
             w, x0, y0, H, W);
  FP_REQUIRE(isfinite(delta) && delta >= 0.f, "fp_vsd_counts: delta=%g must be finite and >= 0", (double)delta);
  Thr t;
  for (int i = 0; i < FP_VSD_MAX_T; ++i) {
    FP_REQUIRE(i >= T || (isfinite(thr[i]) && thr[i] >= 0.f), "fp_vsd_counts: thr[%d]=%g must be finite and >= 0", i, (double)thr[i]);
    t.v[i] = i < T ? thr[i] : __builtin_nanf("");
  }
  FP_REQUIRE(gt_index || G == 1 || G == N, "fp_vsd_counts: gt_index is NULL but G=%d is neither 1 nor N=%d", G, N);
  if (N == 0) return FP_OK;
  FP_REQUIRE(est && gt && obs && fac && counts, "fp_vsd_counts: NULL tensor");
  const hipStream_t st = (hipStream_t)stream;
  const int cells = N * (4 + T);
  hipLaunchKernelGGL(k_vsd_clear, dim3(fp_cdiv(cells, kThreads)), dim3(kThreads), 0, st, counts, cells);
  FP_CHECK_LAUNCH("fp_vsd_counts (clear)");
  const bool vec = w % 4 == 0 && W % 4 == 0 && x0 % 4 == 0 &&
                   (((uintptr_t)est | (uintptr_t)gt | (uintptr_t)obs | (uintptr_t)fac) & 15) == 0;
  const int kv = vec ? 4 : 1, wg = w / kv, ngroups = h * wg;
  const dim3 grid(fp_cdiv(ngroups, kThreads * kIter), N);
  if (vec)
    hipLaunchKernelGGL(k_vsd_counts<4>, grid, dim3(kThreads), 0, st, est, gt, gt_index, G, wg, ngroups, obs, fac, W, x0, y0, delta, t, T,
                       counts);
  else
    hipLaunchKernelGGL(k_vsd_counts<1>, grid, dim3(kThreads), 0, st, est, gt, gt_index, G, wg, ngroups, obs, fac, W, x0, y0, delta, t, T,
                       counts);
  FP_CHECK_LAUNCH("fp_vsd_counts");
  return FP_OK;
}
