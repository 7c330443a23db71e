// The nearest face of every query: the scan that fp_mesh_point_distance, fp_mesh_signed_distance, fp_mesh_transform_residuals,
// fp_mesh_icp_step, fp_mesh_penetration and the grid form of each all begin with (mesh_scan.h has the host functions; the
// definition, down to the float32 operation, is in include/fp_amd.h).  Two launches on the caller's stream, no allocation, no
// synchronisation, integer atomics only:
//   k_init       every cell of the workspace = "no triangle answered yet"
//   k_scan       grid (tile of kThreads queries, chunk of faces): a lane owns one query in registers.  The chunk's triangles pass
//                through LDS in tiles of kTile (mesh_closest.h: scan_chunk): the lane that stages a triangle reads its three indices,
//                checks them against Nv (a triangle with an index outside the table is staged as NaN and so never counts: nothing of
//                pos is read for it) and writes a, b, c, b - a and c - a, the two differences being the definition's own float32
//                operations done once per triangle instead of once per pair.  Every lane then reads the same triangle (one address: an
//                LDS broadcast, no bank conflict) and walks the regions: the source evaluates the seven region tests in the book's
//                order on selects, and the one quotient the chosen region needs is the only division executed (the compiler turns some
//                of the selects into short exec-masked regions, skipped when no lane of the wave needs them; the values are the same).
//                The lane keeps the smallest (dd, face) of its chunk -- faces ascend, so `<` keeps the smaller index on a tie -- and
//                merges it into its cell with one atomic minimum.
//   k_grid_scan  in place of k_scan: a lane owns one query (a point, or a pair's p' formed as in k_scan) and walks the shells of a
//                uniform grid around it (mesh_grid.h: the walk and why it skips no triangle that could win or tie; the proof is per
//                query point, so p' needs nothing new)
// The scans are templates over two things.  Where a lane's query comes from (kPairs): point n of `points`, or the pair n = t * Q + i,
// p = ((r0*x + r1*y) + r2*z) + t per row of transform t, so that T transforms of a few samples still fill a workgroup.  And what the
// lane leaves (Cells): a 64-bit minimum on (bits(dd) << 32) | face (FaceKeys: floats >= 0 order as their bits do), or, for the
// residuals, which ask for no face, a 32-bit minimum on bits(dd) alone (Dist2Cells: best_f is dead there and the compiler drops it).
// A minimum commutes exactly, so a cell has one value whatever the chunking and the arrival order: how the faces are cut into chunks
// depends on the sizes only to fill the chip and never shows in a result.  Compiled with -ffp-contract=off (SRCS_EXACT).
#include "mesh_scan.h"

namespace {

using namespace mesh_closest;

constexpr int kThreads = 256;          // queries, or (transform, point) pairs, per workgroup: one per lane
using mesh_scan::kTile;                // triangles per LDS tile, and
using mesh_scan::kChunkMin;            // the fewest faces a workgroup scans: mesh_scan.h
using mesh_scan::chunk_faces;

static_assert(kTile == kThreads, "a tile is staged by one pass of the workgroup");

// ---- where query n comes from (n < count <= 2^30: no overflow): point n, or with kPairs the pair n = t * Q + i (count = T * Q)
template <bool kPairs>
__device__ __forceinline__ v3 query(const float* __restrict__ points, int Q, const float* __restrict__ tfs, int n) {
  if constexpr (kPairs) {
    const int t = n / Q, i = n - t * Q;
    return transformed(tfs + (size_t)t * 16, load3(points + (size_t)i * 3));
  } else {
    return load3(points + (size_t)n * 3);
  }
}

// ---- what query n leaves in its cell
struct FaceKeys {
  typedef unsigned long long Cell;
  static __device__ __forceinline__ void init(Cell* cell) { *cell = kNoAnswer; }
  static __device__ __forceinline__ void merge(Cell* cell, float best, int best_f) {
    if (best_f >= 0) merge_answer(cell, best, best_f);
  }
};

struct Dist2Cells {
  typedef unsigned Cell;
  static __device__ __forceinline__ void init(Cell* cell) { *cell = 0x7f800000u; }   // the bits of +inf
  // best >= 0 (a sum of squares), never NaN; -0 cannot arise from (x*x + y*y) + z*z
  static __device__ __forceinline__ void merge(Cell* cell, float best, int) {
    if (best < __builtin_inff()) __hip_atomic_fetch_min(cell, __float_as_uint(best), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// The kernels take plain arguments; Q and tfs are dead without kPairs.
template <class Cells>
__global__ __launch_bounds__(kThreads) void k_init(typename Cells::Cell* __restrict__ cells, int count) {
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n < count) Cells::init(cells + n);
}

template <bool kPairs, class Cells>
__global__ __launch_bounds__(kThreads) void k_scan(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int F,
                                                   const float* __restrict__ points, int Q, const float* __restrict__ tfs, int count,
                                                   int chunk, typename Cells::Cell* __restrict__ cells) {
  __shared__ float4 tile[kTile * kTileFloat4];   // per triangle: (a, b.x) (b.yz, c.xy) (c.z, ab) (ac, -)
  const int tid = threadIdx.x;
  const int n = blockIdx.x * kThreads + tid;
  const bool live = n < count;
  const v3 p = query<kPairs>(points, Q, tfs, live ? n : count - 1);   // a lane past the end scans too: it takes part in the barriers
  const int f0 = blockIdx.y * chunk;                  // < F <= 2^30: no overflow in f0 + chunk
  const int f1 = min(F, f0 + chunk);
  float best = __builtin_inff();
  int best_f = -1;
  scan_chunk<kTile>(PointQuery{p}, tile, pos, Nv, faces, f0, f1, tid, best, best_f);
  if (live) Cells::merge(cells + n, best, best_f);
}

template <bool kPairs, class Cells>
__global__ __launch_bounds__(kThreads) void k_grid_scan(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int F,
                                                        mesh_grid::Grid g, mesh_grid::Tables t, const float* __restrict__ points, int Q,
                                                        const float* __restrict__ tfs, int count,
                                                        typename Cells::Cell* __restrict__ cells) {
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n >= count) return;
  float best = __builtin_inff();
  int best_f = -1;
  mesh_grid::walk(g, t, pos, Nv, faces, F, query<kPairs>(points, Q, tfs, n), best, best_f);
  Cells::merge(cells + n, best, best_f);
}

using mesh_scan::launched;

// init, then if F > 0 the scan: over every face, or through the grid
template <bool kPairs, class Cells>
int scan(const char* name, const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid, const float* points, int Q,
         const float* tfs, int count, typename Cells::Cell* cells, hipStream_t st) {
  const int tiles = fp_cdiv(count, kThreads);
  hipLaunchKernelGGL(k_init<Cells>, dim3(tiles), dim3(kThreads), 0, st, cells, count);
  if (int e = launched(name, "init")) return e;
  if (F == 0) return FP_OK;
  if (grid) {
    hipLaunchKernelGGL((k_grid_scan<kPairs, Cells>), dim3(tiles), dim3(kThreads), 0, st, pos, Nv, faces, F, mesh_grid::device_grid(grid),
                       mesh_grid::device_tables(grid), points, Q, tfs, count, cells);
    return launched(name, "scan");
  }
  const int chunk = chunk_faces(tiles, F);
  hipLaunchKernelGGL((k_scan<kPairs, Cells>), dim3(tiles, fp_cdiv(F, chunk)), dim3(kThreads), 0, st, pos, Nv, faces, F, points, Q, tfs,
                     count, chunk, cells);
  return launched(name, "scan");
}

}  // namespace

namespace mesh_scan {

int nearest_face_of_points(const char* name, const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid,
                           const float* points, int Q, unsigned long long* keys, hipStream_t st) {
  return scan<false, FaceKeys>(name, pos, Nv, faces, F, grid, points, Q, nullptr, Q, keys, st);
}

int nearest_face_of_pairs(const char* name, const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid,
                          const float* points, int Q, const float* tfs, int T, unsigned long long* keys, hipStream_t st) {
  return scan<true, FaceKeys>(name, pos, Nv, faces, F, grid, points, Q, tfs, T * Q, keys, st);
}

int nearest_dist2_of_pairs(const char* name, const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid,
                           const float* points, int Q, const float* tfs, int T, unsigned* cell, hipStream_t st) {
  return scan<true, Dist2Cells>(name, pos, Nv, faces, F, grid, points, Q, tfs, T * Q, cell, st);
}

}  // namespace mesh_scan
