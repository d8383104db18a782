// dbscan.hip — sklearn.cluster.DBSCAN(eps, min_samples) for all Q query masks of one scene in one pass
// (reference trainer/trainer.py:517-533).  All masks live on the same points, so the geometry is binned once:
//   cell side h = eps / 2  =>  two points of one cell are at most sqrt(3) h = 0.87 eps apart (always neighbours),
//                              two points within eps differ by at most 2 cells per axis (125-cell stencil).
// Points are sorted by cell (the caller's torch.sort), a mask is a bit row over the sorted points, and DBSCAN over
// points becomes connected components over the (query, cell) nodes that hold a core point:
//   bits -> on-counts -> core bits (min_samples > 1) -> edges between nodes -> components, one workgroup per query
//   -> point labels.
// Every distance test is the one of cc_step_kernel (misc.hip): f32 coordinates, differences and squares in f64,
// against (double)eps * (double)eps.  No kernel waits for another workgroup and no result depends on the order in
// which atomics arrive (the only atomics are minima and a slot counter whose slots are ranked afterwards).
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"

namespace usc {

constexpr int kDbStencil = 125;   // 5 x 5 x 5 cells, index k = (dx+2)*25 + (dy+2)*5 + (dz+2); k and 124-k are opposite
constexpr int kDbSelf = 62;
constexpr int kDbCcThreads = 256;

// bits [s, e) of word w of a bit row, the rest cleared (s < e)
__device__ inline uint64_t db_range_word(const uint64_t* __restrict__ row, int w, int s, int e) {
  uint64_t v = row[w];
  const int lo = w << 6;
  if (s > lo) v &= ~0ull << (s - lo);
  if (e < lo + 64) v &= ~0ull >> (lo + 64 - e);
  return v;
}
__device__ inline int db_ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---------------------------------------------------------------------------
// 1. cell key of every point: key = (cx * ny + cy) * nz + cz, c = floor((x - min) / h) in f64, clamped to the grid
__global__ __launch_bounds__(256) void dbscan_cellkey_kernel(const float* __restrict__ xyz, int64_t n, double mx, double my,
                                                            double mz, double h, int nx, int ny, int nz,
                                                            int64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int cx = (int)floor(((double)xyz[i * 3 + 0] - mx) / h), cy = (int)floor(((double)xyz[i * 3 + 1] - my) / h),
      cz = (int)floor(((double)xyz[i * 3 + 2] - mz) / h);
  cx = cx < 0 ? 0 : (cx >= nx ? nx - 1 : cx);
  cy = cy < 0 ? 0 : (cy >= ny ? ny - 1 : cy);
  cz = cz < 0 ? 0 : (cz >= nz ? nz - 1 : cz);
  key[i] = ((int64_t)cx * ny + cy) * nz + cz;
}

// neighbour table: nbr[c][k] = compact id of the occupied cell at offset k from cell c, or -1 (binary search in the
// ascending keys of the occupied cells)
__global__ __launch_bounds__(256) void dbscan_nbr_kernel(const int64_t* __restrict__ keys, int64_t M, int nx, int ny, int nz,
                                                        int32_t* __restrict__ nbr) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= M * kDbStencil) return;
  const int64_t c = t / kDbStencil;
  const int k = (int)(t - c * kDbStencil);
  const int64_t key = keys[c];
  const int cz = (int)(key % nz), cy = (int)((key / nz) % ny), cx = (int)(key / ((int64_t)nz * ny));
  const int x = cx + k / 25 - 2, y = cy + (k / 5) % 5 - 2, z = cz + k % 5 - 2;
  int32_t found = -1;
  if (x >= 0 && x < nx && y >= 0 && y < ny && z >= 0 && z < nz) {
    const int64_t want = ((int64_t)x * ny + y) * nz + z;
    int64_t lo = 0, hi = M;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    if (lo < M && keys[lo] == want) found = (int32_t)lo;
  }
  nbr[t] = found;
}

// ---------------------------------------------------------------------------
// 2. mask bits over the sorted points: onbits[q][p / 64] bit p % 64 = masks[order[p], q] > 0.  A 64 x 64 tile is read
// along q (whole mask rows) and transposed as bits through two rounds of ballots.
__global__ __launch_bounds__(256) void dbscan_bits_kernel(const float* __restrict__ masks, const int64_t* __restrict__ order,
                                                         int64_t N, int Q, int64_t W, uint64_t* __restrict__ onbits) {
  __shared__ uint64_t rowbits[64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p0 = (int64_t)blockIdx.x * 64;
  const int q0 = blockIdx.y * 64;
  for (int i = 0; i < 16; ++i) {
    const int row = i * 4 + wave;
    const int64_t p = p0 + row;
    const int q = q0 + lane;
    bool on = false;
    if (p < N && q < Q) on = masks[order[p] * Q + q] > 0.f;
    const uint64_t b = __ballot(on);
    if (lane == 0) rowbits[row] = b;
  }
  __syncthreads();
  const uint64_t mine = rowbits[lane];
  for (int i = 0; i < 16; ++i) {
    const int qq = wave * 16 + i;
    const uint64_t w = __ballot((int)((mine >> qq) & 1));
    if (lane == 0 && q0 + qq < Q) onbits[(int64_t)(q0 + qq) * W + blockIdx.x] = w;
  }
}

// set bits per (query, cell)
__global__ __launch_bounds__(256) void dbscan_count_kernel(const uint64_t* __restrict__ bits, const int32_t* __restrict__ start,
                                                          int64_t M, int64_t W, int32_t* __restrict__ cnt) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= M) return;
  const int q = blockIdx.y;
  const uint64_t* row = bits + (int64_t)q * W;
  const int s = start[c], e = start[c + 1];
  int n = 0;
  for (int w = s >> 6; w <= (e - 1) >> 6; ++w) n += __popcll(db_range_word(row, w, s, e));
  cnt[(int64_t)q * M + c] = n;
}

// ---------------------------------------------------------------------------
// 3. core bits (min_samples > 1): a point of a (query, cell) with >= min_samples on-points is core at once; otherwise
// its on-neighbours in the stencil are counted (itself included), stopping at min_samples.  One lane per point.
__global__ __launch_bounds__(256) void dbscan_core_kernel(const float* __restrict__ xs, const int32_t* __restrict__ cell_of,
                                                         const int32_t* __restrict__ start, const int32_t* __restrict__ nbr,
                                                         const uint64_t* __restrict__ onbits, const int32_t* __restrict__ cnt,
                                                         int64_t M, int64_t W, double eps2, int ms,
                                                         uint64_t* __restrict__ corebits) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= W) return;
  const int q = blockIdx.y;
  const uint64_t* row = onbits + (int64_t)q * W;
  const uint64_t word = row[w];
  if (word == 0) {
    if (lane == 0) corebits[(int64_t)q * W + w] = 0;
    return;
  }
  bool core = false;
  if ((word >> lane) & 1) {
    const int64_t p = w * 64 + lane;
    const int c = cell_of[p];
    const int32_t* cq = cnt + (int64_t)q * M;
    if (cq[c] >= ms) {
      core = true;
    } else {
      const double x = (double)xs[p * 3 + 0], y = (double)xs[p * 3 + 1], z = (double)xs[p * 3 + 2];
      int k = 0;
      for (int t = 0; t < kDbStencil && k < ms; ++t) {
        const int b = nbr[(int64_t)c * kDbStencil + t];
        if (b < 0 || cq[b] == 0) continue;
        const int s = start[b], e = start[b + 1];
        for (int wj = s >> 6; wj <= (e - 1) >> 6 && k < ms; ++wj) {
          uint64_t v = db_range_word(row, wj, s, e);
          while (v && k < ms) {
            const int64_t j = ((int64_t)wj << 6) + __builtin_ctzll(v);
            v &= v - 1;
            const double dx = x - (double)xs[j * 3 + 0], dy = y - (double)xs[j * 3 + 1], dz = z - (double)xs[j * 3 + 2];
            if (dx * dx + dy * dy + dz * dz <= eps2) ++k;
          }
        }
      }
      core = k >= ms;
    }
  }
  const uint64_t cb = __ballot(core);
  if (lane == 0) corebits[(int64_t)q * W + w] = cb;
}

// ---------------------------------------------------------------------------
// 4. edges: nodes (q, A) and (q, B) are joined iff a core point of A and a core point of B are within eps.  One wave
// per (q, A) tests the 62 stencil cells of the upper half (k > 62); the lower half is the upper half of the other
// side.  Lanes hold core points of A, the core points of B pass by one at a time, the first hit ends the pair.
__global__ __launch_bounds__(256) void dbscan_edge_kernel(const float* __restrict__ xs, const int32_t* __restrict__ start,
                                                         const int32_t* __restrict__ nbr, const uint64_t* __restrict__ corebits,
                                                         const int32_t* __restrict__ ccnt, int64_t M, int64_t W, double eps2,
                                                         uint64_t* __restrict__ ehalf) {
  const int lane = threadIdx.x & 63;
  const int64_t A = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (A >= M) return;
  const int q = blockIdx.y;
  const int32_t* cq = ccnt + (int64_t)q * M;
  if (cq[A] == 0) {
    if (lane == 0) ehalf[(int64_t)q * M + A] = 0;
    return;
  }
  const uint64_t* row = corebits + (int64_t)q * W;
  const int sA = start[A], eA = start[A + 1];
  uint64_t bits = 0;
  for (int k = kDbSelf + 1; k < kDbStencil; ++k) {
    const int B = nbr[A * kDbStencil + k];
    if (B < 0 || cq[B] == 0) continue;
    const int sB = start[B], eB = start[B + 1];
    bool hit = false;
    for (int wa = sA >> 6; wa <= (eA - 1) >> 6 && !hit; ++wa) {
      const uint64_t va = db_range_word(row, wa, sA, eA);
      if (va == 0) continue;
      const bool mine = (va >> lane) & 1;
      const int64_t pa = mine ? ((int64_t)wa << 6) + lane : sA;
      const double x = (double)xs[pa * 3 + 0], y = (double)xs[pa * 3 + 1], z = (double)xs[pa * 3 + 2];
      for (int wb = sB >> 6; wb <= (eB - 1) >> 6 && !hit; ++wb) {
        uint64_t vb = db_range_word(row, wb, sB, eB);
        while (vb) {
          const int64_t j = ((int64_t)wb << 6) + __builtin_ctzll(vb);
          vb &= vb - 1;
          const double dx = x - (double)xs[j * 3 + 0], dy = y - (double)xs[j * 3 + 1], dz = z - (double)xs[j * 3 + 2];
          if (__any(mine && dx * dx + dy * dy + dz * dz <= eps2)) { hit = true; break; }
        }
      }
    }
    if (hit) bits |= 1ull << (k - kDbSelf - 1);
  }
  if (lane == 0) ehalf[(int64_t)q * M + A] = bits;
}

// ---------------------------------------------------------------------------
// 5. components of one query's nodes, one workgroup per query: label[c] <- min over joined nodes, then down the label
// chain to its root, repeated until a whole sweep changes nothing (workgroup barriers only).  label[c] <= c always, a
// label is a node of the same component, so the fixed point is the component's lowest node whatever the order of the
// updates.  Then the lowest original index among the core points of every component, and its rank among the
// components of the query: sklearn's cluster number.
__global__ __launch_bounds__(kDbCcThreads) void dbscan_components_kernel(
    const int64_t* __restrict__ order, const int32_t* __restrict__ start, const int32_t* __restrict__ nbr,
    const uint64_t* __restrict__ corebits, const int32_t* __restrict__ ccnt, const uint64_t* __restrict__ ehalf, int64_t M,
    int64_t W, int32_t* __restrict__ label, int32_t* __restrict__ compmin, int32_t* __restrict__ roots,
    int32_t* __restrict__ nodecl, int32_t* __restrict__ n_clusters) {
  __shared__ int n_roots;
  const int q = blockIdx.x;
  const int32_t* cq = ccnt + (int64_t)q * M;
  const uint64_t* eh = ehalf + (int64_t)q * M;
  const uint64_t* row = corebits + (int64_t)q * W;
  label += (int64_t)q * M;
  compmin += (int64_t)q * M;
  roots += (int64_t)q * M;
  nodecl += (int64_t)q * M;
  const int m = (int)M;
  for (int c = threadIdx.x; c < m; c += kDbCcThreads) {
    label[c] = cq[c] > 0 ? c : -1;
    compmin[c] = INT_MAX;
    nodecl[c] = -1;
  }
  if (threadIdx.x == 0) n_roots = 0;
  __syncthreads();
  for (;;) {
    int changed = 0;
    for (int c = threadIdx.x; c < m; c += kDbCcThreads) {
      if (cq[c] == 0) continue;
      const int cur = db_ld(label + c);
      int best = cur;
      const int32_t* nb = nbr + (int64_t)c * kDbStencil;
      for (uint64_t e = eh[c]; e; e &= e - 1) {
        const int l = db_ld(label + nb[kDbSelf + 1 + __builtin_ctzll(e)]);
        best = l < best ? l : best;
      }
      for (int k = 0; k < kDbSelf; ++k) {
        const int b = nb[k];
        if (b < 0 || cq[b] == 0 || !((eh[b] >> (kDbSelf - 1 - k)) & 1)) continue;
        const int l = db_ld(label + b);
        best = l < best ? l : best;
      }
      for (;;) {   // strictly descending, ends at a node that is its own label
        const int up = db_ld(label + best);
        if (up == best) break;
        best = up;
      }
      if (best < cur) {
        atomicMin(label + c, best);
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  for (int c = threadIdx.x; c < m; c += kDbCcThreads) {
    if (cq[c] == 0) continue;
    const int s = start[c], e = start[c + 1];
    int lowest = INT_MAX;
    for (int w = s >> 6; w <= (e - 1) >> 6; ++w)
      for (uint64_t v = db_range_word(row, w, s, e); v; v &= v - 1) {
        const int o = (int)order[((int64_t)w << 6) + __builtin_ctzll(v)];
        lowest = o < lowest ? o : lowest;
      }
    atomicMin(compmin + db_ld(label + c), lowest);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < m; c += kDbCcThreads)
    if (cq[c] > 0 && db_ld(label + c) == c) roots[atomicAdd(&n_roots, 1)] = c;   // slot order is free: ranked below
  __syncthreads();
  const int R = n_roots;
  for (int i = threadIdx.x; i < R; i += kDbCcThreads) {
    const int r = roots[i];
    const int mine = db_ld(compmin + r);
    int rank = 0;
    for (int j = 0; j < R; ++j) rank += db_ld(compmin + roots[j]) < mine;
    nodecl[r] = rank;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < m; c += kDbCcThreads) {
    if (cq[c] == 0) continue;
    const int r = db_ld(label + c);
    if (r != c) nodecl[c] = nodecl[r];
  }
  if (threadIdx.x == 0) n_clusters[q] = R;
}

// ---------------------------------------------------------------------------
// 6. point labels, 64 sorted points x 64 queries per workgroup: a core point takes the number of its node, another
// on-point the lowest number among the core points within eps (-1: noise), an off-point -2.  The tile goes through
// LDS so that labels[order[p], :] is written along q.
__global__ __launch_bounds__(256) void dbscan_point_labels_kernel(
    const float* __restrict__ xs, const int64_t* __restrict__ order, const int32_t* __restrict__ cell_of,
    const int32_t* __restrict__ start, const int32_t* __restrict__ nbr, const uint64_t* __restrict__ onbits,
    const uint64_t* __restrict__ corebits, const int32_t* __restrict__ nodecl, int64_t N, int Q, int64_t M, int64_t W,
    double eps2, int32_t* __restrict__ labels) {
  __shared__ int32_t tile[64][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p = (int64_t)blockIdx.x * 64 + lane;
  const int q0 = blockIdx.y * 64;
  const int c = p < N ? cell_of[p] : 0;
  for (int i = 0; i < 16; ++i) {
    const int qq = wave * 16 + i, q = q0 + qq;
    int lab = -2;
    if (q < Q) {
      const uint64_t on = onbits[(int64_t)q * W + blockIdx.x], core = corebits[(int64_t)q * W + blockIdx.x];
      const int32_t* ncl = nodecl + (int64_t)q * M;
      if ((core >> lane) & 1) {
        lab = ncl[c];
      } else if ((on >> lane) & 1) {
        const uint64_t* row = corebits + (int64_t)q * W;
        const double x = (double)xs[p * 3 + 0], y = (double)xs[p * 3 + 1], z = (double)xs[p * 3 + 2];
        int best = INT_MAX;
        for (int t = 0; t < kDbStencil; ++t) {
          const int b = nbr[(int64_t)c * kDbStencil + t];
          if (b < 0) continue;
          const int cl = ncl[b];
          if (cl < 0 || cl >= best) continue;   // no core point there, or nothing to gain
          const int s = start[b], e = start[b + 1];
          bool hit = false;
          for (int wj = s >> 6; wj <= (e - 1) >> 6 && !hit; ++wj)
            for (uint64_t v = db_range_word(row, wj, s, e); v; v &= v - 1) {
              const int64_t j = ((int64_t)wj << 6) + __builtin_ctzll(v);
              const double dx = x - (double)xs[j * 3 + 0], dy = y - (double)xs[j * 3 + 1], dz = z - (double)xs[j * 3 + 2];
              if (dx * dx + dy * dy + dz * dz <= eps2) { hit = true; break; }
            }
          if (hit) best = cl;
        }
        lab = best == INT_MAX ? -1 : best;
      }
    }
    tile[lane][qq] = lab;
  }
  __syncthreads();
  for (int i = 0; i < 16; ++i) {
    const int r = i * 4 + wave;
    const int64_t pp = (int64_t)blockIdx.x * 64 + r;
    const int q = q0 + lane;
    if (pp < N && q < Q) labels[order[pp] * Q + q] = tile[r][lane];
  }
}

// 7. one column per (query, cluster): out[n, col0[q] + label] = masks[n, q]; out is zeroed by the caller
__global__ __launch_bounds__(256) void dbscan_expand_kernel(const float* __restrict__ masks, const int32_t* __restrict__ labels,
                                                           const int64_t* __restrict__ col0, int64_t total, int Q,
                                                           int64_t Qp, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int l = labels[i];
  if (l < 0) return;
  const int64_t n = i / Q;
  const int q = (int)(i - n * Q);
  out[n * Qp + col0[q] + l] = masks[i];
}

static inline int64_t db_words(int64_t N) { return ceil_div(N, 64); }

}  // namespace usc

using namespace usc;

extern "C" {

int usc_dbscan_cell_keys(const float* xyz, int64_t n, float eps, double min_x, double min_y, double min_z, int32_t nx,
                         int32_t ny, int32_t nz, int64_t* keys, usc_stream_t s) {
  USC_REQUIRE(n >= 0, "usc_dbscan_cell_keys: bad n");
  USC_REQUIRE(eps > 0.f && eps <= FLT_MAX, "usc_dbscan_cell_keys: eps must be positive and finite");
  USC_REQUIRE(fabs(min_x) <= DBL_MAX && fabs(min_y) <= DBL_MAX && fabs(min_z) <= DBL_MAX, "usc_dbscan_cell_keys: non-finite grid origin");
  USC_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && nx <= USC_DBSCAN_MAX_CELLS_PER_AXIS && ny <= USC_DBSCAN_MAX_CELLS_PER_AXIS &&
                  nz <= USC_DBSCAN_MAX_CELLS_PER_AXIS,
              "usc_dbscan_cell_keys: an axis needs 1 to 2^20 cells, got %d x %d x %d", nx, ny, nz);
  if (n == 0) return USC_OK;
  USC_REQUIRE(xyz && keys, "usc_dbscan_cell_keys: null pointer");
  hipLaunchKernelGGL(dbscan_cellkey_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, as_stream(s), xyz, n, min_x,
                     min_y, min_z, (double)eps * 0.5, (int)nx, (int)ny, (int)nz, keys);
  USC_CHECK_LAUNCH("usc_dbscan_cell_keys");
  return USC_OK;
}

int usc_dbscan_neighbor_table(const int64_t* cell_keys, int64_t n_cells, int32_t nx, int32_t ny, int32_t nz, int32_t* nbr,
                              usc_stream_t s) {
  USC_REQUIRE(n_cells >= 0 && n_cells < (1ll << 31) / kDbStencil, "usc_dbscan_neighbor_table: bad n_cells");
  USC_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && nx <= USC_DBSCAN_MAX_CELLS_PER_AXIS && ny <= USC_DBSCAN_MAX_CELLS_PER_AXIS &&
                  nz <= USC_DBSCAN_MAX_CELLS_PER_AXIS,
              "usc_dbscan_neighbor_table: an axis needs 1 to 2^20 cells, got %d x %d x %d", nx, ny, nz);
  if (n_cells == 0) return USC_OK;
  USC_REQUIRE(cell_keys && nbr, "usc_dbscan_neighbor_table: null pointer");
  hipLaunchKernelGGL(dbscan_nbr_kernel, dim3((unsigned)ceil_div(n_cells * kDbStencil, 256)), dim3(256), 0, as_stream(s),
                     cell_keys, n_cells, (int)nx, (int)ny, (int)nz, nbr);
  USC_CHECK_LAUNCH("usc_dbscan_neighbor_table");
  return USC_OK;
}

int64_t usc_dbscan_ws_bytes(int64_t n, int32_t q, int64_t n_cells, int32_t min_samples) {
  if (n < 0 || q < 0 || n_cells < 0) return -1;
  const int64_t nodes = (int64_t)q * n_cells, words = (int64_t)q * db_words(n);
  // on bits (+ core bits), on counts (+ core counts), half edge masks, label / lowest index / root list / cluster id
  return 8 * words * (min_samples > 1 ? 2 : 1) + 4 * nodes * (min_samples > 1 ? 2 : 1) + 8 * nodes + 16 * nodes;
}

int usc_dbscan_labels(const float* xyz_sorted, const int64_t* order, const int32_t* cell_of, const int32_t* cell_start,
                      const int32_t* nbr, const float* masks, int64_t n, int32_t q, int64_t n_cells, float eps,
                      int32_t min_samples, void* ws, int64_t ws_bytes, int32_t* labels, int32_t* n_clusters,
                      usc_stream_t s) {
  USC_REQUIRE(n >= 1 && n <= (1ll << 31) - 64, "usc_dbscan_labels: n must be in [1, 2^31 - 64]");
  USC_REQUIRE(q >= 1 && q <= 65535, "usc_dbscan_labels: the number of queries must be in [1, 65535], got %d", q);
  USC_REQUIRE(n_cells >= 1 && n_cells <= n && n_cells < (1ll << 31) / kDbStencil, "usc_dbscan_labels: bad n_cells");
  USC_REQUIRE(eps > 0.f && eps <= FLT_MAX, "usc_dbscan_labels: eps must be positive and finite");
  USC_REQUIRE(min_samples >= 1, "usc_dbscan_labels: min_samples must be >= 1, got %d", min_samples);
  USC_REQUIRE(xyz_sorted && order && cell_of && cell_start && nbr && masks && ws && labels && n_clusters,
              "usc_dbscan_labels: null pointer");
  USC_REQUIRE(ws_bytes >= usc_dbscan_ws_bytes(n, q, n_cells, min_samples), "usc_dbscan_labels: workspace too small");
  hipStream_t st = as_stream(s);
  const int64_t M = n_cells, W = db_words(n), nodes = (int64_t)q * M, words = (int64_t)q * W;
  const bool cores = min_samples > 1;
  const double eps2 = (double)eps * (double)eps;
  char* w = (char*)ws;
  uint64_t* onbits = (uint64_t*)w;   w += 8 * words;
  uint64_t* corebits = onbits;
  if (cores) { corebits = (uint64_t*)w; w += 8 * words; }
  uint64_t* ehalf = (uint64_t*)w;    w += 8 * nodes;
  int32_t* cnt = (int32_t*)w;        w += 4 * nodes;
  int32_t* ccnt = cnt;
  if (cores) { ccnt = (int32_t*)w;   w += 4 * nodes; }
  int32_t* label = (int32_t*)w;      w += 4 * nodes;
  int32_t* compmin = (int32_t*)w;    w += 4 * nodes;
  int32_t* roots = (int32_t*)w;      w += 4 * nodes;
  int32_t* nodecl = (int32_t*)w;
  const dim3 tiles((unsigned)W, (unsigned)ceil_div(q, 64));
  const dim3 percell((unsigned)ceil_div(M, 256), (unsigned)q);
  hipLaunchKernelGGL(dbscan_bits_kernel, tiles, dim3(256), 0, st, masks, order, n, (int)q, W, onbits);
  hipLaunchKernelGGL(dbscan_count_kernel, percell, dim3(256), 0, st, (const uint64_t*)onbits, cell_start, M, W, cnt);
  if (cores) {
    hipLaunchKernelGGL(dbscan_core_kernel, dim3((unsigned)ceil_div(W, 4), (unsigned)q), dim3(256), 0, st, xyz_sorted, cell_of,
                       cell_start, nbr, (const uint64_t*)onbits, (const int32_t*)cnt, M, W, eps2, (int)min_samples, corebits);
    hipLaunchKernelGGL(dbscan_count_kernel, percell, dim3(256), 0, st, (const uint64_t*)corebits, cell_start, M, W, ccnt);
  }
  hipLaunchKernelGGL(dbscan_edge_kernel, dim3((unsigned)ceil_div(M, 4), (unsigned)q), dim3(256), 0, st, xyz_sorted, cell_start,
                     nbr, (const uint64_t*)corebits, (const int32_t*)ccnt, M, W, eps2, ehalf);
  hipLaunchKernelGGL(dbscan_components_kernel, dim3((unsigned)q), dim3(kDbCcThreads), 0, st, order, cell_start, nbr,
                     (const uint64_t*)corebits, (const int32_t*)ccnt, (const uint64_t*)ehalf, M, W, label, compmin, roots,
                     nodecl, n_clusters);
  hipLaunchKernelGGL(dbscan_point_labels_kernel, tiles, dim3(256), 0, st, xyz_sorted, order, cell_of, cell_start, nbr,
                     (const uint64_t*)onbits, (const uint64_t*)corebits, (const int32_t*)nodecl, n, (int)q, M, W, eps2,
                     labels);
  USC_CHECK_LAUNCH("usc_dbscan_labels");
  return USC_OK;
}

int usc_dbscan_expand(const float* masks, const int32_t* labels, const int64_t* col_start, int64_t n, int32_t q,
                      int64_t n_cols, float* out, usc_stream_t s) {
  USC_REQUIRE(n >= 0 && q >= 1 && n_cols >= 0 && n <= (1ll << 39) / q, "usc_dbscan_expand: bad sizes");
  if (n == 0 || n_cols == 0) return USC_OK;
  USC_REQUIRE(masks && labels && col_start && out, "usc_dbscan_expand: null pointer");
  const int64_t total = n * q;
  hipLaunchKernelGGL(dbscan_expand_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, as_stream(s), masks, labels,
                     col_start, total, (int)q, n_cols, out);
  USC_CHECK_LAUNCH("usc_dbscan_expand");
  return USC_OK;
}

}  // extern "C"
