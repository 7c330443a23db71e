// The build of a uniform grid over a mesh's triangles (fp_mesh_grid_count, fp_mesh_grid_fill; the definition is in include/fp_amd.h,
// the per-triangle decision and the walk that reads the tables in mesh_grid.h).  On the caller's stream, integer atomics only, no
// allocation, no synchronisation:
//   fp_mesh_grid_count, three launches:
//     k_mg_zero    cell_start[0..ncells] = 0, header = 0
//     k_mg_count   one lane per triangle: classify (mesh_grid.h); a stored triangle adds 1 to every cell of its range, an overflow one
//                  adds 1 to header[1]
//     k_mg_scan    one workgroup: the exclusive scan of the counts in place (a lane sums a contiguous run in 64 bits, the 1024 sums are
//                  scanned in LDS, the lane writes its run's prefixes); header[0] = the total, which is also cell_start[ncells]
//   fp_mesh_grid_fill, two launches:
//     k_mg_zero    cursor[0..ncells] = 0
//     k_mg_fill    one lane per triangle, the same classify: a stored triangle takes slot cell_start[cell] + cursor[cell]++ in each of
//                  its cells, an overflow one slot cursor[ncells]++ of the overflow list.  A slot past the capacity or past the cell's
//                  own slots is not written: the status word header[2] says so.
// Sums and ORs of integers commute, so cell_start, the header and each cell's set of entries have one value whatever the arrival order;
// the order inside a cell is arbitrary, and the walk compares (dd, face) explicitly so that it shows in no result.
#include <limits.h>
#include "fp_common.h"
#include "mesh_grid.h"

namespace {

using namespace mesh_grid;

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;

__global__ __launch_bounds__(kThreads) void k_mg_zero(int32_t* __restrict__ a, int n, int32_t* __restrict__ header) {
  const int i = blockIdx.x * kThreads + threadIdx.x;   // n <= 2^21 + 1
  if (i < n) a[i] = 0;
  if (header && i < kHeaderInts) header[i] = 0;
}

__global__ __launch_bounds__(kThreads) void k_mg_count(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int F,
                                                       Grid g, int32_t* __restrict__ counts, int32_t* __restrict__ header) {
  const int f = blockIdx.x * kThreads + threadIdx.x;   // F <= 2^30
  if (f >= F) return;
  int i0[3], i1[3];
  const int cls = classify(g, pos, Nv, faces, f, i0, i1);
  if (cls == kOverflow) __hip_atomic_fetch_add(header + kOverflowCount, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (cls != kStored) return;
  for (int z = i0[2]; z <= i1[2]; ++z)
    for (int y = i0[1]; y <= i1[1]; ++y)
      for (int x = i0[0]; x <= i1[0]; ++x)
        __hip_atomic_fetch_add(counts + ((z * g.n[1] + y) * g.n[0] + x), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// in place over a[0..n-1] (n = ncells + 1, a[n-1] = 0 coming in): a[i] = the sum of what a[0..i-1] held, capped at INT_MAX
__global__ __launch_bounds__(kScanThreads) void k_mg_scan(int32_t* __restrict__ a, int n, int32_t* __restrict__ header) {
  __shared__ long long s[kScanThreads];
  const int tid = threadIdx.x;
  const int per = (n + kScanThreads - 1) / kScanThreads;   // <= 2049: tid * per does not overflow
  const int b = min(n, tid * per), e = min(n, b + per);
  long long sum = 0;
  for (int i = b; i < e; ++i) sum += a[i];
  s[tid] = sum;
  __syncthreads();
  for (int off = 1; off < kScanThreads; off <<= 1) {
    const long long v = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  long long run = s[tid] - sum;
  for (int i = b; i < e; ++i) {
    const int cnt = a[i];
    a[i] = (int32_t)(run < (long long)INT_MAX ? run : (long long)INT_MAX);
    run += cnt;
  }
  if (tid == kScanThreads - 1) {
    const long long total = s[tid];
    header[kEntries] = (int32_t)(total < (long long)INT_MAX ? total : (long long)INT_MAX);
    header[kStatus] = total > (long long)INT_MAX ? kTooManyEntries : 0;
  }
}

__global__ __launch_bounds__(kThreads) void k_mg_fill(const float* __restrict__ pos, int Nv, const int32_t* __restrict__ faces, int F,
                                                      Grid g, const int32_t* __restrict__ cell_start, int32_t* __restrict__ cursor,
                                                      int ncells, int32_t* __restrict__ entries, int cap_entries,
                                                      int32_t* __restrict__ overflow, int cap_overflow, int32_t* __restrict__ header) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  int i0[3], i1[3];
  const int cls = classify(g, pos, Nv, faces, f, i0, i1);
  if (cls == kOverflow) {
    const int k = __hip_atomic_fetch_add(cursor + ncells, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((unsigned)k < (unsigned)cap_overflow) overflow[k] = f;
    else __hip_atomic_fetch_or(header + kStatus, (int)kOverflowTooSmall, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (cls != kStored) return;
  bool full = false;
  for (int z = i0[2]; z <= i1[2]; ++z)
    for (int y = i0[1]; y <= i1[1]; ++y)
      for (int x = i0[0]; x <= i1[0]; ++x) {
        const int cell = (z * g.n[1] + y) * g.n[0] + x;
        const int k = __hip_atomic_fetch_add(cursor + cell, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long slot = (long long)cell_start[cell] + k;
        // inside the list and inside the cell's own slots (a cell_start that is not this mesh's writes nothing out of place)
        if (slot >= 0 && slot < (long long)cap_entries && slot < (long long)cell_start[cell + 1]) entries[slot] = f;
        else full = true;
      }
  if (full) __hip_atomic_fetch_or(header + kStatus, (int)kEntriesTooSmall, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int check_mesh(const char* name, const float* pos, int Nv, const int32_t* faces, int F, const int32_t* header) {
  FP_REQUIRE(F >= 0 && F <= (1 << 30), "%s: F=%d outside 0..2^30", name, F);
  FP_REQUIRE(Nv >= 0, "%s: Nv=%d is negative", name, Nv);
  FP_REQUIRE(F == 0 || faces, "%s: faces is NULL but F=%d", name, F);
  FP_REQUIRE(F == 0 || Nv == 0 || pos, "%s: pos is NULL but Nv=%d", name, Nv);
  FP_REQUIRE(header, "%s: NULL header", name);
  return FP_OK;
}

}  // namespace

extern "C" int fp_mesh_grid_count(const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid, int32_t* header,
                                  void* stream) {
  const char* name = "fp_mesh_grid_count";
  if (int st = check_mesh(name, pos, Nv, faces, F, header)) return st;
  FP_REQUIRE(grid, "%s: NULL grid", name);
  fp_mesh_grid shape = *grid;                  // the lists are not read here: only the shape and cell_start are checked
  shape.entries = shape.overflow = nullptr;
  shape.n_entries = shape.n_overflow = 0;
  if (int st = check_grid(name, &shape)) return st;
  const hipStream_t st = (hipStream_t)stream;
  const Grid g = device_grid(grid);
  const int ncells = (int)cells_of(grid);
  hipLaunchKernelGGL(k_mg_zero, dim3(fp_cdiv(ncells + 1, kThreads)), dim3(kThreads), 0, st, grid->cell_start, ncells + 1, header);
  FP_CHECK_LAUNCH("fp_mesh_grid_count (zero)");
  if (F > 0) {
    hipLaunchKernelGGL(k_mg_count, dim3(fp_cdiv(F, kThreads)), dim3(kThreads), 0, st, pos, Nv, faces, F, g, grid->cell_start, header);
    FP_CHECK_LAUNCH("fp_mesh_grid_count (count)");
  }
  hipLaunchKernelGGL(k_mg_scan, dim3(1), dim3(kScanThreads), 0, st, grid->cell_start, ncells + 1, header);
  FP_CHECK_LAUNCH("fp_mesh_grid_count (scan)");
  return FP_OK;
}

extern "C" size_t fp_mesh_grid_fill_workspace_bytes(const fp_mesh_grid* grid) {
  if (!grid || grid->n[0] < 1 || grid->n[1] < 1 || grid->n[2] < 1 || grid->n[0] > kMaxCells || grid->n[1] > kMaxCells ||
      grid->n[2] > kMaxCells || cells_of(grid) > kMaxCells)
    return 0;
  return (size_t)(cells_of(grid) + 1) * sizeof(int32_t);
}

extern "C" int fp_mesh_grid_fill(const float* pos, int Nv, const int32_t* faces, int F, const fp_mesh_grid* grid, int32_t* header,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  const char* name = "fp_mesh_grid_fill";
  if (int st = check_mesh(name, pos, Nv, faces, F, header)) return st;
  if (int st = check_grid(name, grid)) return st;
  const size_t need = fp_mesh_grid_fill_workspace_bytes(grid);
  FP_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0,
             "%s: workspace too small or not 4-byte aligned (%zu < %zu bytes, see fp_mesh_grid_fill_workspace_bytes)", name,
             workspace_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  const Grid g = device_grid(grid);
  const int ncells = (int)cells_of(grid);
  int32_t* cursor = (int32_t*)workspace;
  hipLaunchKernelGGL(k_mg_zero, dim3(fp_cdiv(ncells + 1, kThreads)), dim3(kThreads), 0, st, cursor, ncells + 1, (int32_t*)nullptr);
  FP_CHECK_LAUNCH("fp_mesh_grid_fill (zero)");
  if (F > 0) {
    hipLaunchKernelGGL(k_mg_fill, dim3(fp_cdiv(F, kThreads)), dim3(kThreads), 0, st, pos, Nv, faces, F, g,
                       (const int32_t*)grid->cell_start, cursor, ncells, grid->entries, grid->n_entries, grid->overflow,
                       grid->n_overflow, header);
    FP_CHECK_LAUNCH("fp_mesh_grid_fill (fill)");
  }
  return FP_OK;
}
