// normals.hip — normals estimated from a point cloud: open3d's
// pcd.estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) (datasets/preprocessing/arkit_preprocessing.py:98-101)
// as two calls.
//
// usc_knn_hybrid_grid: the k nearest reference points strictly inside a radius, ordered by (d2, index), through the
// uniform grid of knn_grid.h.  d2 is usc_knn1's expression in f64 on the f32 inputs.  One thread per query keeps its
// sorted list in LDS (entry e of thread t at [e * 64 + t]: no bank conflicts, no per-thread array, no scratch).
// Which cells a query reads follows from knn_cell being monotone: a point with |p - q| < r along an axis has its cell
// between the cells of q - r and q + r, wherever the grid's walls are and whether or not anything was clamped.  A query
// whose cell range reaches further than kHybridMaxRing cells from its own cell reads every reference point instead.
//
// usc_normals_pca: mean and centred second moments of the listed neighbours in f64, then the eigenvector of the
// smallest eigenvalue by cyclic Jacobi with a fixed number of sweeps (backward stable; the closed form loses the vector
// when the two smallest eigenvalues are close).
#include "knn_grid.h"

namespace usc {

constexpr int kHybridThreads = 64;          // one wave per block: the block's lists are k * 64 * 12 bytes of LDS
constexpr int kHybridMaxK = 64;             // 48 KB of LDS at the most
constexpr int kHybridMaxRing = 4;           // as kKnnGridMaxRing of knn.hip: past 9 cells along an axis, all points
constexpr int kJacobiSweeps = 8;            // 3x3 cyclic Jacobi converges quadratically; 5 sweeps reach f64 rounding

// Offers candidate (d, id) to thread t's list of m <= k entries sorted by (d, id) ascending.  wd / wi cache the last
// entry of a full list, so that a full list rejects most candidates without touching LDS.
__device__ inline void hybrid_offer(double d, int id, int k, int& m, double& wd, int& wi, double* __restrict__ ld,
                                    int* __restrict__ li, int t) {
  if (m == k && !(d < wd || (d == wd && id < wi))) return;
  int e = m < k ? m : k - 1;                // the slot that opens: one past the end, or the entry that drops out
  while (e > 0) {
    const double pd = ld[(e - 1) * kHybridThreads + t];
    const int pi = li[(e - 1) * kHybridThreads + t];
    if (pd < d || (pd == d && pi < id)) break;
    ld[e * kHybridThreads + t] = pd;
    li[e * kHybridThreads + t] = pi;
    --e;
  }
  ld[e * kHybridThreads + t] = d;
  li[e * kHybridThreads + t] = id;
  if (m < k) ++m;
  if (m == k) {
    wd = ld[(k - 1) * kHybridThreads + t];
    wi = li[(k - 1) * kHybridThreads + t];
  }
}

static __global__ __launch_bounds__(kHybridThreads) void knn_hybrid_query_kernel(
    const float* __restrict__ q, int64_t nq, const float* __restrict__ r, int nr, KnnGrid g,
    const int32_t* __restrict__ start, const KnnPoint* __restrict__ pts, double rad, double r2, int k,
    int32_t* __restrict__ idx, int32_t* __restrict__ count) {
  extern __shared__ double hybrid_lds[];
  __shared__ int cnt[kHybridThreads];
  double* ld = hybrid_lds;                                   // f64[k][64]
  int* li = (int*)(hybrid_lds + k * kHybridThreads);         // i32[k][64]
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kHybridThreads;
  const int64_t i = base + t;
  int m = 0, wi = 0;
  double wd = 0.0;

  if (i < nq) {
    const float fx = q[i * 3 + 0], fy = q[i * 3 + 1], fz = q[i * 3 + 2];
    const double qx = (double)fx, qy = (double)fy, qz = (double)fz;
    // d2 < r2 bounds |p - q| along an axis by rad * (1 + a few 2^-53); q -+ rr is rounded once more.  2^-40 of the
    // radius and 2^-45 of the coordinate are thousands of times those roundings and far below one cell.
    const double rr = rad * (1.0 + 0x1p-40);
    const double mx = 0x1p-45 * (fabs(qx) + rad), my = 0x1p-45 * (fabs(qy) + rad), mz = 0x1p-45 * (fabs(qz) + rad);
    const int cx = knn_cell(fx, g.ox, g.cell, g.nx), cy = knn_cell(fy, g.oy, g.cell, g.ny),
              cz = knn_cell(fz, g.oz, g.cell, g.nz);
    const int lx = knn_cell_f64(qx - rr - mx, g.ox, g.cell, g.nx), hx = knn_cell_f64(qx + rr + mx, g.ox, g.cell, g.nx),
              ly = knn_cell_f64(qy - rr - my, g.oy, g.cell, g.ny), hy = knn_cell_f64(qy + rr + my, g.oy, g.cell, g.ny),
              lz = knn_cell_f64(qz - rr - mz, g.oz, g.cell, g.nz), hz = knn_cell_f64(qz + rr + mz, g.oz, g.cell, g.nz);
    const bool covered = cx - lx <= kHybridMaxRing && hx - cx <= kHybridMaxRing && cy - ly <= kHybridMaxRing &&
                         hy - cy <= kHybridMaxRing && cz - lz <= kHybridMaxRing && hz - cz <= kHybridMaxRing;
    if (covered) {
      for (int x = lx; x <= hx; ++x) {
        for (int y = ly; y <= hy; ++y) {
          const int row = (x * g.ny + y) * g.nz;
          const int s = start[row + lz], e = start[row + hz + 1];   // cells lz .. hz are one span of the sorted points
          for (int j = s; j < e; ++j) {
            const KnnPoint p = pts[j];
            const double ddx = qx - (double)p.x, ddy = qy - (double)p.y, ddz = qz - (double)p.z;
            const double d = ddx * ddx + ddy * ddy + ddz * ddz;
            if (d < r2) hybrid_offer(d, p.i, k, m, wd, wi, ld, li, t);
          }
        }
      }
    } else {
      for (int j = 0; j < nr; ++j) {
        const double ddx = qx - (double)r[(int64_t)j * 3 + 0], ddy = qy - (double)r[(int64_t)j * 3 + 1],
                     ddz = qz - (double)r[(int64_t)j * 3 + 2];
        const double d = ddx * ddx + ddy * ddy + ddz * ddz;
        if (d < r2) hybrid_offer(d, j, k, m, wd, wi, ld, li, t);
      }
    }
    count[i] = m;
  }
  cnt[t] = m;
  __syncthreads();
  // the block's rows are one contiguous piece of idx: written in order by all lanes
  const int rows = nq - base < kHybridThreads ? (int)(nq - base) : kHybridThreads;
  for (int f = t; f < rows * k; f += kHybridThreads) {
    const int row = f / k, col = f - row * k;
    idx[base * k + f] = col < cnt[row] ? li[col * kHybridThreads + row] : -1;
  }
}

// One Jacobi rotation of the symmetric 3x3 matrix in the (p, q) plane; r is the third index.  app, aqq, apq and the
// two off-diagonal entries arp, arq that the rotation mixes; vp, vq the matching columns of the eigenvector matrix.
__host__ __device__ inline void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq,
                                              double* vp, double* vq) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double tt = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));   // theta^2 = inf gives 0: no rotation needed
  const double tn = theta < 0.0 ? -tt : tt;
  const double c = 1.0 / sqrt(tn * tn + 1.0), s = tn * c;
  app -= tn * apq;
  aqq += tn * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  for (int i = 0; i < 3; ++i) {
    const double a = vp[i], b = vq[i];
    vp[i] = c * a - s * b;
    vq[i] = s * a + c * b;
  }
}

// Unit eigenvector of the smallest eigenvalue of the symmetric matrix (c00 c01 c02; . c11 c12; . . c22) as f32, with
// the sign rule of usc_normals_pca; false for a zero or non-finite matrix or vector.
__host__ __device__ inline bool normal_from_cov(double c00, double c01, double c02, double c11, double c12, double c22,
                                                float* out) {
  const double scale = fmax(fmax(fmax(fabs(c00), fabs(c11)), fabs(c22)), fmax(fmax(fabs(c01), fabs(c02)), fabs(c12)));
  if (!(scale > 0.0) || !(scale < 1e300) || c00 != c00 || c01 != c01 || c02 != c02 || c11 != c11 || c12 != c12 ||
      c22 != c22)
    return false;
  double a00 = c00 / scale, a01 = c01 / scale, a02 = c02 / scale, a11 = c11 / scale, a12 = c12 / scale,
         a22 = c22 / scale;
  double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    jacobi_rotate(a00, a11, a01, a02, a12, v0, v1);
    jacobi_rotate(a00, a22, a02, a01, a12, v0, v2);
    jacobi_rotate(a11, a22, a12, a01, a02, v1, v2);
  }
  double nx = v0[0], ny = v0[1], nz = v0[2], lam = a00;
  if (a11 < lam) { nx = v1[0]; ny = v1[1]; nz = v1[2]; lam = a11; }
  if (a22 < lam) { nx = v2[0]; ny = v2[1]; nz = v2[2]; lam = a22; }
  const double len = sqrt(nx * nx + ny * ny + nz * nz);
  if (!(len > 0.0) || !(len < 1e300)) return false;
  float fx = (float)(nx / len), fy = (float)(ny / len), fz = (float)(nz / len);
  // sign: the stored component of largest magnitude, the lowest axis among equals, is >= 0
  const float ax = fabsf(fx), ay = fabsf(fy), az = fabsf(fz);
  const float lead = (ax >= ay && ax >= az) ? fx : (ay >= az ? fy : fz);
  if (lead < 0.f) { fx = -fx; fy = -fy; fz = -fz; }
  if (!(ax + ay + az > 0.f)) return false;
  out[0] = fx;
  out[1] = fy;
  out[2] = fz;
  return true;
}

static __global__ __launch_bounds__(256) void normals_pca_kernel(const float* __restrict__ q, int64_t nq,
                                                                const float* __restrict__ r, int nr,
                                                                const int32_t* __restrict__ idx,
                                                                const int32_t* __restrict__ count, int k,
                                                                float* __restrict__ normals) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq) return;
  float out[3] = {0.f, 0.f, 1.f};
  int m = count[i];
  m = m < 0 ? 0 : (m > k ? k : m);
  const int32_t* row = idx + i * k;
  const double qx = (double)q[i * 3 + 0], qy = (double)q[i * 3 + 1], qz = (double)q[i * 3 + 2];
  bool ok = m >= 3;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int j = 0; ok && j < m; ++j) {
    const int p = row[j];
    if (p < 0 || p >= nr) { ok = false; break; }           // not a list of usc_knn_hybrid_grid: the degenerate answer
    sx += (double)r[(int64_t)p * 3 + 0] - qx;
    sy += (double)r[(int64_t)p * 3 + 1] - qy;
    sz += (double)r[(int64_t)p * 3 + 2] - qz;
  }
  if (ok) {
    const double mm = (double)m;
    const double ux = sx / mm, uy = sy / mm, uz = sz / mm;
    double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
    for (int j = 0; j < m; ++j) {
      const int p = row[j];
      const double x = ((double)r[(int64_t)p * 3 + 0] - qx) - ux, y = ((double)r[(int64_t)p * 3 + 1] - qy) - uy,
                   z = ((double)r[(int64_t)p * 3 + 2] - qz) - uz;
      c00 += x * x; c01 += x * y; c02 += x * z;
      c11 += y * y; c12 += y * z; c22 += z * z;
    }
    float n[3];
    if (normal_from_cov(c00 / mm, c01 / mm, c02 / mm, c11 / mm, c12 / mm, c22 / mm, n)) {
      out[0] = n[0];
      out[1] = n[1];
      out[2] = n[2];
    }
  }
  normals[i * 3 + 0] = out[0];
  normals[i * 3 + 1] = out[1];
  normals[i * 3 + 2] = out[2];
}

}  // namespace usc

using namespace usc;

extern "C" {

int64_t usc_knn_hybrid_grid_ws_bytes(int64_t nr, const int32_t* dims) {
  KnnGridWs w;
  if (!knn_grid_layout(nr, dims, &w)) {
    set_error("usc_knn_hybrid_grid_ws_bytes: needs 1 <= nr < 2^31 and dims >= 1 with at most 2^27 cells");
    return -1;
  }
  return w.total;
}

int usc_knn_hybrid_grid(const float* query, int64_t nq, const float* ref, int64_t nr, float radius, int32_t k,
                        const double* origin, double cell, const int32_t* dims, int32_t* idx, int32_t* count, void* ws,
                        int64_t ws_bytes, usc_stream_t s) {
  KnnGridWs w;
  USC_REQUIRE(k >= 1 && k <= kHybridMaxK, "usc_knn_hybrid_grid: k must be 1 .. %d, got %d", kHybridMaxK, (int)k);
  USC_REQUIRE(radius > 0.f && radius <= 3.4028234e38f, "usc_knn_hybrid_grid: radius must be finite and > 0");
  USC_REQUIRE(nq >= 0 && nq <= ((int64_t)0x7fffffff * kHybridThreads) / 2 && origin && cell > 0.0 && cell < 1e300 &&
                  knn_grid_layout(nr, dims, &w),
              "usc_knn_hybrid_grid: needs 0 <= nq < 2^36, 1 <= nr < 2^31, a finite cell > 0 and dims >= 1 with at most "
              "2^27 cells");
  USC_REQUIRE(origin[0] == origin[0] && origin[1] == origin[1] && origin[2] == origin[2],
              "usc_knn_hybrid_grid: origin is NaN");
  USC_REQUIRE(ref && ws && (nq == 0 || (query && idx && count)), "usc_knn_hybrid_grid: null pointer");
  USC_REQUIRE(ws_bytes >= w.total, "usc_knn_hybrid_grid: workspace too small (%lld bytes, needs %lld)",
              (long long)ws_bytes, (long long)w.total);
  hipStream_t st = as_stream(s);
  const KnnGrid g{origin[0], origin[1], origin[2], cell, dims[0], dims[1], dims[2]};
  char* b = (char*)ws;
  knn_grid_build(ref, nr, g, w, ws, st);
  if (nq > 0) {
    const double rad = (double)radius;
    const size_t lds = (size_t)k * kHybridThreads * (sizeof(double) + sizeof(int));
    hipLaunchKernelGGL(knn_hybrid_query_kernel, dim3((unsigned)ceil_div(nq, kHybridThreads)), dim3(kHybridThreads), lds,
                       st, query, nq, ref, (int)nr, g, (const int32_t*)(b + w.start), (const KnnPoint*)(b + w.pts), rad,
                       rad * rad, (int)k, idx, count);
  }
  USC_CHECK_LAUNCH("usc_knn_hybrid_grid");
  return USC_OK;
}

int usc_normals_pca(const float* query, int64_t nq, const float* ref, int64_t nr, const int32_t* idx,
                    const int32_t* count, int32_t k, float* normals, usc_stream_t s) {
  USC_REQUIRE(nq >= 0 && nr >= 1 && nr <= 0x7fffffff && k >= 1 && k <= kHybridMaxK,
              "usc_normals_pca: needs nq >= 0, 1 <= nr < 2^31 and k in 1 .. %d", kHybridMaxK);
  USC_REQUIRE(ref && (nq == 0 || (query && idx && count && normals)), "usc_normals_pca: null pointer");
  if (nq > 0)
    hipLaunchKernelGGL(normals_pca_kernel, dim3((unsigned)ceil_div(nq, 256)), dim3(256), 0, as_stream(s), query, nq, ref,
                       (int)nr, idx, count, (int)k, normals);
  USC_CHECK_LAUNCH("usc_normals_pca");
  return USC_OK;
}

}  // extern "C"
