// The surface components of a TSDF volume's cubes (fp_tsdf_label_components; the definition is in include/fp_amd.h): union-find over
// the counts of fp_tsdf_count_triangles, with `labels` itself as the parent array.
//   k_tc_init     labels[c] = a parent <= c for an active cube, -1 otherwise; sizes[c] = 0.  One lane per cube, x fastest, so the
//                 active lanes of a wave that follow each other in one row of cubes are x-neighbours of each other: a ballot finds each
//                 such run and every lane of it starts with the run's first cube as its parent, before any memory is touched.
//   k_tc_merge    one lane per cube: unite it with its +x, +y and +z neighbour where that one is active too (+x only across a wave's
//                 end: inside a wave the runs are linked already).  A union finds both roots and atomicMin's the
//                 larger root's parent down to the smaller; a parent is never larger than its child, so once this launch has
//                 finished the root of a tree is the smallest cube index of its component.
//   k_tc_flatten  labels[c] = the root of c, and counts[c] added into sizes[root]: one integer atomic per lane, or one per wave
//                 when all active lanes of the wave carry one root (the common case; a large component otherwise sends thousands of adds
//                 to one address).
// Integer atomics only: min and + commute exactly, so both outputs have one value whatever the arrival order, the definition's.
// Every loop ends on its own (the reasons stand beside each); none waits for a value another wave or workgroup has to write, and the
// only ordering relied on is the one between launches of one stream.  Parents that other lanes may be lowering are read with relaxed
// agent-scope atomic loads, never with plain loads the compiler could hoist out of a loop.
// Times, also of builds without the ballot and without the wave sum (both slower, so neither was kept as an option):
// scripts/bench_tsdf_components.py, profiles/tsdf_components.json, DESIGN.md section 1.
// The volume's dimensions are checked by recon_common.h's check_grid, as in tsdf.hip and tsdf_raycast.hip.
#include "fp_common.h"
#include "recon_common.h"

namespace {

constexpr int kThreads = 256;   // four waves of 64: a wave is 64 consecutive cubes

struct Cubes {
  int mx, my, mz, n;   // cubes along x, y, z and their product (< 2^30)
};

__device__ __forceinline__ int parent_of(const int32_t* p, int x) {
  return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Ends: every step goes to a parent strictly below x (anything else, x itself included, is returned as the root), and x >= 0.
__device__ __forceinline__ int find_root(const int32_t* p, int x) {
  for (;;) {
    const int q = parent_of(p, x);
    if ((unsigned)q >= (unsigned)x) return x;
    x = q;
  }
}

// Ends: a pass either returns or goes on with a = the parent the atomic found at the root a, which is below a; b never rises.  Both
// are >= 0, so there are at most a + b passes, whatever other lanes do in between.
__device__ __forceinline__ void unite(int32_t* p, int a, int b) {
  for (;;) {
    a = find_root(p, a);
    b = find_root(p, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;   // a was still a root: linked
    // another lane had linked a to old < a in the meantime.  Whether the min replaced that link (old > b) or not, old and b
    // are in one component and may not be in one tree yet
    a = old;
  }
}

__global__ __launch_bounds__(kThreads) void k_tc_init(const int32_t* __restrict__ counts, Cubes g, int32_t* __restrict__ labels,
                                                      int32_t* __restrict__ sizes) {
  const int c = (int)(blockIdx.x * (unsigned)kThreads + threadIdx.x);
  const bool in = c < g.n;
  const bool active = in && counts[c] > 0;
  int parent = c;
  const int lane = (int)(threadIdx.x & 63u);
  const unsigned long long act = __ballot(active);
  const unsigned long long row0 = __ballot(in && c % g.mx == 0);
  // a run starts at an active lane whose predecessor in the wave is not active or lies in the row before
  const unsigned long long starts = act & (~(act << 1) | row0);
  if (active) parent = c - (lane - (63 - __clzll((long long)(starts & (~0ull >> (63 - lane))))));
  if (in) {
    labels[c] = active ? parent : -1;
    sizes[c] = 0;
  }
}

__global__ __launch_bounds__(kThreads) void k_tc_merge(const int32_t* __restrict__ counts, Cubes g, int32_t* labels) {
  const int c = (int)(blockIdx.x * (unsigned)kThreads + threadIdx.x);
  if (c >= g.n || counts[c] <= 0) return;
  const int cx = c % g.mx, r = c / g.mx;
  const int cy = r % g.my, cz = r / g.my;
  const bool last_lane = (threadIdx.x & 63u) == 63u;   // every other lane's +x neighbour is in its run already (k_tc_init)
  if (last_lane && cx + 1 < g.mx && counts[c + 1] > 0) unite(labels, c, c + 1);
  if (cy + 1 < g.my && counts[c + g.mx] > 0) unite(labels, c, c + g.mx);
  if (cz + 1 < g.mz && counts[c + g.mx * g.my] > 0) unite(labels, c, c + g.mx * g.my);
}

__global__ __launch_bounds__(kThreads) void k_tc_flatten(const int32_t* __restrict__ counts, Cubes g, int32_t* labels, int32_t* sizes) {
  const int c = (int)(blockIdx.x * (unsigned)kThreads + threadIdx.x);
  const int n = c < g.n ? counts[c] : 0;
  const bool active = n > 0;
  int root = -1;
  if (active) {
    // the trees are final; lanes that write their root below only shorten the walks of others
    root = find_root(labels, c);
    __hip_atomic_store(labels + c, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const unsigned long long act = __ballot(active);
  if (act == 0) return;   // wave-uniform, like the branch below
  const int lead = __ffsll((long long)act) - 1;
  const int root0 = __shfl(root, lead);
  if (__ballot(active && root != root0) == 0) {
    int sum = active ? n : 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if ((int)(threadIdx.x & 63u) == lead) __hip_atomic_fetch_add(sizes + root0, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if (active) __hip_atomic_fetch_add(sizes + root, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

extern "C" int fp_tsdf_label_components(const int32_t* counts, int nz, int ny, int nx, int32_t* labels, int32_t* sizes, void* stream) {
  const char* who = "fp_tsdf_label_components";
  if (int st = recon::check_grid(who, nz, ny, nx)) return st;
  const Cubes g{nx - 1, ny - 1, nz - 1, (nz - 1) * (ny - 1) * (nx - 1)};
  if (g.n == 0) return FP_OK;
  FP_REQUIRE(counts && labels && sizes, "%s: NULL counts / labels / sizes", who);
  const dim3 grid((unsigned)((g.n + kThreads - 1) / kThreads)), block(kThreads);
  hipLaunchKernelGGL(k_tc_init, grid, block, 0, (hipStream_t)stream, counts, g, labels, sizes);
  hipLaunchKernelGGL(k_tc_merge, grid, block, 0, (hipStream_t)stream, counts, g, labels);
  hipLaunchKernelGGL(k_tc_flatten, grid, block, 0, (hipStream_t)stream, counts, g, labels, sizes);
  FP_CHECK_LAUNCH(who);
  return FP_OK;
}
