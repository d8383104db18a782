// knn.hip — exact 1-nearest-neighbour through a uniform grid (usc_knn1_grid): the answers of usc_knn1 (misc.hip) —
// f64 distances on the f32 inputs, the lowest reference index among equidistant points, dist2 as the same f32 bits —
// without visiting every (query, reference) pair.  Replaces scipy.spatial.KDTree(ref).query(query, k=1)
// (pseudo_masks/unscene3d_pseudo_main.py:339-343).
//
// Build (knn_grid.h): cell of every reference point -> histogram -> exclusive scan -> scatter -> rank inside the cell, so
// that a cell's points lie in ascending reference index.  Query: one thread per query walks cubes of cells of Chebyshev
// radius 1, 2, ... around its own cell and stops when its best distance is strictly below what any unsearched point can
// have; a query that kKnnGridMaxRing rings do not settle is answered by streaming every reference point, block-wide,
// exactly as knn1_kernel does.
#include "knn_grid.h"

namespace usc {

constexpr int kKnnGridMaxRing = 4;          // cubes of up to 9^3 cells; past that a query streams all points
constexpr int kKnnGridTile = 1024;          // reference points per LDS tile of the streaming pass

__global__ __launch_bounds__(256) void knn_grid_query_kernel(const float* __restrict__ q, int64_t nq,
                                                            const float* __restrict__ r, int nr, KnnGrid g,
                                                            const int32_t* __restrict__ start,
                                                            const KnnPoint* __restrict__ pts, int64_t* __restrict__ idx,
                                                            float* __restrict__ dist2) {
  __shared__ float tx[kKnnGridTile], ty[kKnnGridTile], tz[kKnnGridTile];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool act = i < nq;
  const float fx = act ? q[i * 3 + 0] : 0.f, fy = act ? q[i * 3 + 1] : 0.f, fz = act ? q[i * 3 + 2] : 0.f;
  const double qx = (double)fx, qy = (double)fy, qz = (double)fz;
  double best = 1e300;
  int bi = 0x7fffffff;
  bool settled = !act;

  if (act) {
    const int cx = knn_cell(fx, g.ox, g.cell, g.nx), cy = knn_cell(fy, g.oy, g.cell, g.ny),
              cz = knn_cell(fz, g.oz, g.cell, g.nz);
    // What rounding can move: a cell coordinate, a wall o + k * cell and a distance to it are each a few f64 roundings
    // of numbers no larger than |o| + n * cell + |q|.  2^-45 of that sum is 64 times the worst case and far below any
    // distance that decides a search.
    const double slack = 0x1p-45;
    const double mx = slack * (fabs(g.ox) + g.nx * g.cell + fabs(qx)), my = slack * (fabs(g.oy) + g.ny * g.cell + fabs(qy)),
                 mz = slack * (fabs(g.oz) + g.nz * g.cell + fabs(qz));
    for (int R = 1; R <= kKnnGridMaxRing && !settled; ++R) {
      for (int dx = -R; dx <= R; ++dx) {
        const int x = cx + dx;
        if (x < 0 || x >= g.nx) continue;
        for (int dy = -R; dy <= R; ++dy) {
          const int y = cy + dy;
          if (y < 0 || y >= g.ny) continue;
          const int row = (x * g.ny + y) * g.nz;
          const bool shell = R == 1 || dx == -R || dx == R || dy == -R || dy == R;
          // a row of the shell: cells cz-R .. cz+R are one span of the sorted points; an inner row: its two end cells
          for (int part = 0; part < (shell ? 1 : 2); ++part) {
            int z0, z1;
            if (shell) {
              z0 = cz - R < 0 ? 0 : cz - R;
              z1 = cz + R > g.nz - 1 ? g.nz - 1 : cz + R;
            } else {
              z0 = z1 = part == 0 ? cz - R : cz + R;
              if (z0 < 0 || z0 >= g.nz) continue;
            }
            const int s = start[row + z0], e = start[row + z1 + 1];
            for (int j = s; j < e; ++j) {
              const KnnPoint p = pts[j];
              const double ddx = qx - (double)p.x, ddy = qy - (double)p.y, ddz = qz - (double)p.z;
              const double d = ddx * ddx + ddy * ddy + ddz * ddz;
              if (d < best || (d == best && p.i < bi)) { best = d; bi = p.i; }
            }
          }
        }
      }
      // A point outside the cube lies, along some axis, in a cell beyond cq + R or before cq - R, so past the wall
      // o + (cq + R + 1) * cell or o + (cq - R) * cell.  That holds for clamped points (they only move inwards) and
      // wherever the query itself lies, clamped or not.  A side on which the cube reaches the grid's edge hides nothing.
      double bound = 1e300;
      if (cx + R < g.nx - 1) bound = fmin(bound, (g.ox + (double)(cx + R + 1) * g.cell) - qx - mx);
      if (cx - R > 0) bound = fmin(bound, qx - (g.ox + (double)(cx - R) * g.cell) - mx);
      if (cy + R < g.ny - 1) bound = fmin(bound, (g.oy + (double)(cy + R + 1) * g.cell) - qy - my);
      if (cy - R > 0) bound = fmin(bound, qy - (g.oy + (double)(cy - R) * g.cell) - my);
      if (cz + R < g.nz - 1) bound = fmin(bound, (g.oz + (double)(cz + R + 1) * g.cell) - qz - mz);
      if (cz - R > 0) bound = fmin(bound, qz - (g.oz + (double)(cz - R) * g.cell) - mz);
      // strictly below: a point at exactly the bound with a lower index, not searched yet, must still win
      settled = bi != 0x7fffffff && bound > 0.0 && best < bound * bound;
    }
  }

  // the queries no ring settled: all reference points, in index order, through LDS (knn1_kernel's loop)
  if (__syncthreads_or(settled ? 0 : 1)) {
    const bool need = !settled;
    if (need) { best = 1e300; bi = 0x7fffffff; }
    for (int t0 = 0; t0 < nr; t0 += kKnnGridTile) {
      const int cnt = nr - t0 < kKnnGridTile ? nr - t0 : kKnnGridTile;
      for (int j = threadIdx.x; j < cnt; j += 256) {
        tx[j] = r[(int64_t)(t0 + j) * 3 + 0];
        ty[j] = r[(int64_t)(t0 + j) * 3 + 1];
        tz[j] = r[(int64_t)(t0 + j) * 3 + 2];
      }
      __syncthreads();
      if (need) {
        for (int j = 0; j < cnt; ++j) {
          const double dx = qx - (double)tx[j], dy = qy - (double)ty[j], dz = qz - (double)tz[j];
          const double d = dx * dx + dy * dy + dz * dz;
          if (d < best) { best = d; bi = t0 + j; }
        }
      }
      __syncthreads();
    }
  }
  if (act) {
    idx[i] = (int64_t)bi;
    if (dist2) dist2[i] = (float)best;
  }
}

}  // namespace usc

using namespace usc;

extern "C" {

int64_t usc_knn1_grid_ws_bytes(int64_t nr, const int32_t* dims) {
  KnnGridWs w;
  if (!knn_grid_layout(nr, dims, &w)) {
    set_error("usc_knn1_grid_ws_bytes: needs 1 <= nr < 2^31 and dims >= 1 with at most 2^27 cells");
    return -1;
  }
  return w.total;
}

int usc_knn1_grid(const float* query, int64_t nq, const float* ref, int64_t nr, const double* origin, double cell,
                  const int32_t* dims, int64_t* idx, float* dist2, void* ws, int64_t ws_bytes, usc_stream_t s) {
  KnnGridWs w;
  USC_REQUIRE(nq >= 0 && origin && cell > 0.0 && cell < 1e300 && knn_grid_layout(nr, dims, &w),
              "usc_knn1_grid: needs nq >= 0, 1 <= nr < 2^31, a finite cell > 0 and dims >= 1 with at most 2^27 cells");
  USC_REQUIRE(origin[0] == origin[0] && origin[1] == origin[1] && origin[2] == origin[2], "usc_knn1_grid: origin is NaN");
  USC_REQUIRE(ref && ws && (nq == 0 || (query && idx)), "usc_knn1_grid: null pointer");
  USC_REQUIRE(ws_bytes >= w.total, "usc_knn1_grid: workspace too small (%lld bytes, needs %lld)", (long long)ws_bytes,
              (long long)w.total);
  hipStream_t st = as_stream(s);
  const KnnGrid g{origin[0], origin[1], origin[2], cell, dims[0], dims[1], dims[2]};
  char* b = (char*)ws;
  knn_grid_build(ref, nr, g, w, ws, st);
  if (nq > 0)
    hipLaunchKernelGGL(knn_grid_query_kernel, dim3((unsigned)ceil_div(nq, 256)), dim3(256), 0, st, query, nq, ref, (int)nr,
                       g, (const int32_t*)(b + w.start), (const KnnPoint*)(b + w.pts), idx, dist2);
  USC_CHECK_LAUNCH("usc_knn1_grid");
  return USC_OK;
}

}  // extern "C"
