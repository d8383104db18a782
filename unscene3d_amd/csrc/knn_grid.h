// knn_grid.h — the uniform grid of the exact neighbour searches (knn.hip: usc_knn1_grid; normals.hip:
// usc_knn_hybrid_grid).  Build: cell of every reference point -> histogram -> exclusive scan (scan.h) -> scatter -> rank
// inside the cell, so that a cell's points lie in ascending reference index.  Both searches bin points and queries with
// knn_cell, which is monotone in the coordinate: that is what their stopping rules rest on.
#pragma once
#include "common.h"
#include "scan.h"

namespace usc {

constexpr int64_t kKnnGridMaxCells = (int64_t)1 << 27;

struct KnnGrid {
  double ox, oy, oz, cell;
  int nx, ny, nz;
};

struct __align__(16) KnnPoint {
  float x, y, z;
  int32_t i;
};

// Cell coordinate along one axis, in f64, clamped into [0, n): NaN and anything outside the grid land in a boundary
// cell, so the result is always a valid address.  Build and query share this function; the stopping rule below allows
// for its rounding.
__device__ inline int knn_cell_f64(double v, double o, double cell, int n) {
  const double t = floor((v - o) / cell);
  return (int)fmin(fmax(t, 0.0), (double)(n - 1));
}
__device__ inline int knn_cell(float v, double o, double cell, int n) { return knn_cell_f64((double)v, o, cell, n); }


static __global__ __launch_bounds__(256) void knn_grid_hist_kernel(const float* __restrict__ r, int nr, KnnGrid g,
                                                           int32_t* __restrict__ count, int32_t* __restrict__ cellid,
                                                           int32_t* __restrict__ slot) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nr) return;
  const int cx = knn_cell(r[(int64_t)i * 3 + 0], g.ox, g.cell, g.nx),
            cy = knn_cell(r[(int64_t)i * 3 + 1], g.oy, g.cell, g.ny),
            cz = knn_cell(r[(int64_t)i * 3 + 2], g.oz, g.cell, g.nz);
  const int c = (cx * g.ny + cy) * g.nz + cz;
  cellid[i] = c;
  slot[i] = atomicAdd(&count[c], 1);        // arrival order inside the cell; knn_grid_rank_kernel puts it right
}

static __global__ __launch_bounds__(256) void knn_grid_scatter_kernel(int nr, const int32_t* __restrict__ start,
                                                              const int32_t* __restrict__ cellid,
                                                              const int32_t* __restrict__ slot,
                                                              int32_t* __restrict__ arrived) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nr) arrived[start[cellid[i]] + slot[i]] = i;
}

// The stable place of a point inside its cell = the number of points of that cell with a lower reference index.
static __global__ __launch_bounds__(256) void knn_grid_rank_kernel(const float* __restrict__ r, int nr,
                                                           const int32_t* __restrict__ start,
                                                           const int32_t* __restrict__ cellid,
                                                           const int32_t* __restrict__ arrived,
                                                           KnnPoint* __restrict__ pts) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nr) return;
  const int i = arrived[j];
  const int c = cellid[i];
  const int s = start[c], e = start[c + 1];
  int rank = 0;
  for (int k = s; k < e; ++k) rank += arrived[k] < i ? 1 : 0;
  KnnPoint p;
  p.x = r[(int64_t)i * 3 + 0];
  p.y = r[(int64_t)i * 3 + 1];
  p.z = r[(int64_t)i * 3 + 2];
  p.i = i;
  pts[s + rank] = p;
}

struct KnnCountVal {
  const int32_t* count;
  int64_t n;
  __device__ int operator()(int64_t i) const { return i < n ? count[i] : 0; }
};
struct KnnStartEmit {
  int32_t* start;
  __device__ void operator()(int64_t i, int64_t prefix, int) const { start[i] = (int32_t)prefix; }
};

// workspace: start i32[cells + 1] | cellid i32[nr] | slot i32[nr] | arrived i32[nr] | pts KnnPoint[nr] | scan
struct KnnGridWs {
  int64_t start, cellid, slot, arrived, pts, scan, total;
};
static bool knn_grid_layout(int64_t nr, const int32_t* dims, KnnGridWs* w) {
  if (!dims || nr < 1 || nr > 0x7fffffff || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return false;
  const int64_t cells = (int64_t)dims[0] * dims[1] * dims[2];
  if ((int64_t)dims[0] * dims[1] > kKnnGridMaxCells || cells > kKnnGridMaxCells) return false;
  int64_t o = 0;
  w->start = o;   o += align_up((cells + 1) * 4, 256);
  w->cellid = o;  o += align_up(nr * 4, 256);
  w->slot = o;    o += align_up(nr * 4, 256);
  w->arrived = o; o += align_up(nr * 4, 256);
  w->pts = o;     o += align_up(nr * (int64_t)sizeof(KnnPoint), 256);
  w->scan = o;    o += align_up(scan_ws_bytes(cells + 1), 256);
  w->total = o;
  return true;
}

// Bins the nr reference points into ws (laid out by knn_grid_layout): start[c] .. start[c + 1] is cell c's span of pts.
static inline void knn_grid_build(const float* ref, int64_t nr, const KnnGrid& g, const KnnGridWs& w, void* ws,
                                  hipStream_t st) {
  const int64_t cells = (int64_t)g.nx * g.ny * g.nz;
  char* b = (char*)ws;
  int32_t* start = (int32_t*)(b + w.start);
  int32_t* cellid = (int32_t*)(b + w.cellid);
  int32_t* slot = (int32_t*)(b + w.slot);
  int32_t* arrived = (int32_t*)(b + w.arrived);
  KnnPoint* pts = (KnnPoint*)(b + w.pts);
  const dim3 gr((unsigned)ceil_div(nr, 256));
  (void)hipMemsetAsync(start, 0, (size_t)((cells + 1) * 4), st);
  hipLaunchKernelGGL(knn_grid_hist_kernel, gr, dim3(256), 0, st, ref, (int)nr, g, start, cellid, slot);
  // counts -> first sorted position of every cell, in place (a thread reads its own items before it writes them);
  // entry `cells` = nr
  device_exclusive_scan(KnnCountVal{start, cells}, KnnStartEmit{start}, cells + 1, b + w.scan, st);
  hipLaunchKernelGGL(knn_grid_scatter_kernel, gr, dim3(256), 0, st, (int)nr, (const int32_t*)start,
                     (const int32_t*)cellid, (const int32_t*)slot, arrived);
  hipLaunchKernelGGL(knn_grid_rank_kernel, gr, dim3(256), 0, st, ref, (int)nr, (const int32_t*)start,
                     (const int32_t*)cellid, (const int32_t*)arrived, pts);
}

}  // namespace usc
