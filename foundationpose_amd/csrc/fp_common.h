// Shared helpers for libfp_amd.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <stdio.h>
#include "../../include/fp_amd.h"

void fp_set_error(const char* fmt, ...);

#define FP_REQUIRE(cond, ...)            \
  do {                                   \
    if (!(cond)) {                       \
      fp_set_error(__VA_ARGS__);         \
      return FP_ERR_INVALID_ARG;         \
    }                                    \
  } while (0)

#define FP_CHECK_LAUNCH(name)                                             \
  do {                                                                    \
    hipError_t e_ = hipGetLastError();                                    \
    if (e_ != hipSuccess) {                                               \
      fp_set_error("%s launch failed: %s", name, hipGetErrorString(e_));  \
      return FP_ERR_LAUNCH;                                               \
    }                                                                     \
  } while (0)

struct fp_mesh {
  const float* pos;
  const float* nrm;
  const int32_t* faces;
  const float* uv;
  const int32_t* uv_idx;
  const float* tex;
  const float* vcol;
  int V, T, Ht, Wt;
};

// fp_mesh_set_create: the descriptors of M meshes in one device table (copied once, at setup) + the largest V / T, which size
// the grids and the workspace of fp_render_crops with a set
struct fp_mesh_set {
  fp_mesh* meshes;   // [dev M]
  int M, maxV, maxT;
};

struct fp_k9 { float v[9]; };
struct fp_k9d { double v[9]; };

// Several views per call (a call that gives Ks / view / V): hypothesis n reads frame view[n] of a (V, H, W, C) stack and the intrinsics
// Ks[view[n]] of a (V, 9) device table (view NULL: all 0, allowed only for V == 1).  -1 = an index outside 0..V-1: the caller
// then reads nothing from the stack or the table.
struct fp_views {
  const void* Ks;          // [dev V,9] f32 (render, warp, pose update) | f64 (crop windows, back-projection)
  const int32_t* view;     // [dev N] | NULL
  int V;
};

__device__ __forceinline__ int fp_view_of(const fp_views& vt, int n) {
  const int v = vt.view ? vt.view[n] : 0;
  return (unsigned)v < (unsigned)vt.V ? v : -1;
}

// The kernels take the table as a trailing parameter pack: empty for the single-view instantiations, whose signatures (and so their
// kernel-argument layouts and instruction sequences) stay what they were; one fp_views for a call with a view table.
__device__ __forceinline__ fp_views fp_views_of() { return fp_views{nullptr, nullptr, 0}; }
__device__ __forceinline__ fp_views fp_views_of(const fp_views& vt) { return vt; }

// K of view v (v >= 0), or all NaN (v < 0)
template <typename KT, typename T>
__device__ __forceinline__ KT fp_view_K(const fp_views& vt, int v) {
  KT K;
  const T* src = reinterpret_cast<const T*>(vt.Ks) + (size_t)(v < 0 ? 0 : v) * 9;
#pragma unroll
  for (int i = 0; i < 9; ++i) K.v[i] = v < 0 ? (T)__builtin_nan("") : src[i];
  return K;
}

static inline int fp_cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- The scene arguments of the crop stage (fp_crop_windows, fp_render_crops, fp_warp_crops, fp_pose_update; include/fp_amd.h),
// checked here once.  Each side is given either as one host value (K; mesh_diameter) or as a device table (Ks / view / V;
// diameters / obj / M); a side is in its table form when any argument of its table is set.  `name` is the entry point's.
static inline bool fp_has_objects(const double* diameters, const int32_t* obj, int M) { return diameters || obj || M != 0; }
static inline bool fp_has_views(const void* Ks, const int32_t* view, int V) { return Ks || view || V != 0; }

static inline int fp_check_objects(const char* name, const double* diameters, const int32_t* obj, int M) {
  FP_REQUIRE(M >= 1 && diameters, "%s: need the diameters of M >= 1 objects (M=%d)", name, M);
  FP_REQUIRE(obj || M == 1, "%s: obj is NULL but there are %d objects", name, M);
  return FP_OK;
}

// `objects`: the call's object side is in its table form, the only one the view-table kernels are built for
static inline int fp_check_views(const char* name, const void* K, const void* Ks, const int32_t* view, int V, bool objects) {
  FP_REQUIRE(!K, "%s: both K and a view table (Ks / view / V) are given; pass exactly one camera description", name);
  FP_REQUIRE(V >= 1 && Ks, "%s: need the K table of V >= 1 views (V=%d)", name, V);
  FP_REQUIRE(view || V == 1, "%s: view is NULL but there are %d views", name, V);
  FP_REQUIRE(objects, "%s: a view table (Ks) with a scalar diameter is not built; pass the diameter table with it", name);
  return FP_OK;
}

// The instantiation a crop-stage call runs, from its form: host K and scalar diameter <false>, host K and diameter table <true>,
// view table and diameter table <true, true> (fp_check_views has refused a view table without the diameter table).  fn is a launch
// helper template <bool MULTI, bool VIEWS = false>.
#define FP_LAUNCH_FORM(objects, views, fn, ...) \
  (!(objects) ? fn<false>(__VA_ARGS__) : !(views) ? fn<true>(__VA_ARGS__) : fn<true, true>(__VA_ARGS__))

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: set it once per (kernel, device).
// Use as FP_SET_MAX_LDS(kernel_symbol, bytes) right before the launch.  Thread-safe (one host thread per device is the
// multi-GPU use): the per-device "done" bit is published with an atomic OR only AFTER the attribute call has returned, so a
// racing thread at worst repeats the (idempotent) call; devices >= 64 are not cached.  A failing call is reported.
#define FP_SET_MAX_LDS(kernel, bytes)                                                                                 \
  do {                                                                                                                \
    static std::atomic<unsigned long long> done_{0ull};                                                               \
    int dev_ = 0;                                                                                                     \
    (void)hipGetDevice(&dev_);                                                                                        \
    if (dev_ < 0 || dev_ >= 64 || !((done_.load(std::memory_order_acquire) >> dev_) & 1ull)) {                        \
      const hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(&kernel),                               \
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (bytes));                 \
      if (e_ != hipSuccess) {                                                                                         \
        fp_set_error("hipFuncSetAttribute(%s, %d bytes of LDS) failed on device %d: %s", #kernel, (int)(bytes), dev_, \
                     hipGetErrorString(e_));                                                                          \
        return FP_ERR_LAUNCH;                                                                                         \
      }                                                                                                               \
      if (dev_ >= 0 && dev_ < 64) done_.fetch_or(1ull << dev_, std::memory_order_release);                            \
    }                                                                                                                 \
  } while (0)
