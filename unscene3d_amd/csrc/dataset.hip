// dataset.hip — the per-scene tables of the FreeMask reader and the vertex normals of the dataset builder.
//
// usc_softmask_stats / usc_softmask_table replace the reader's host passes over the [N,K] soft-mask table
// (datasets/freemask.py): per-column count and XY extent of `soft > thr`, then the int32 table the collate takes.
// usc_mesh_vertex_normals is open3d's compute_vertex_normals (area-weighted sum of the face normals, normalised).
// Explicit stream, no allocation, no synchronisation, no float atomics.
#include <float.h>

#include "common.h"

namespace usc {

constexpr int kSmBlock = 256;              // 4 waves; lane = column of a 64-column tile, waves interleave the rows
constexpr int kSmWaves = kSmBlock / kWave;
constexpr int kSmRows = 256;               // rows of one partial (more for N > kSmRows * kSmMaxBlocks)
constexpr int kSmMaxBlocks = 2048;
constexpr int kSmFinish = 1024;            // finish pass: 16 waves share the row blocks of a column tile

static int64_t sm_rows_per_block(int64_t n) {
  return n <= (int64_t)kSmRows * kSmMaxBlocks ? kSmRows : align_up(ceil_div(n, kSmMaxBlocks), kSmWaves);
}

struct SmAcc {
  int32_t n;
  float lx, ly, hx, hy;
};

__device__ inline void sm_merge(SmAcc& a, const SmAcc& b) {
  a.n += b.n;
  a.lx = fminf(a.lx, b.lx); a.ly = fminf(a.ly, b.ly);
  a.hx = fmaxf(a.hx, b.hx); a.hy = fmaxf(a.hy, b.hy);
}

// the waves' accumulators of one column tile -> wave 0, in wave order (LDS: NW x 64 per field)
template <int NW>
__device__ inline bool sm_block_combine(SmAcc& a, int32_t (*sn)[kWave], float (*sf)[NW][kWave]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  sn[wave][lane] = a.n;
  sf[0][wave][lane] = a.lx; sf[1][wave][lane] = a.ly; sf[2][wave][lane] = a.hx; sf[3][wave][lane] = a.hy;
  __syncthreads();
  if (wave != 0) return false;
  for (int w = 1; w < NW; ++w)
    sm_merge(a, SmAcc{sn[w][lane], sf[0][w][lane], sf[1][w][lane], sf[2][w][lane], sf[3][w][lane]});
  return true;
}

// grid (column tiles, row blocks).  A wave reads 64 consecutive columns of one row: the row-major table is read
// coalesced, x / y of the row are the same address for the whole wave.
__global__ __launch_bounds__(kSmBlock) void softmask_stats_kernel(const float* __restrict__ soft,
                                                                  const float* __restrict__ xyz, int64_t N, int32_t K,
                                                                  float thr, int64_t rows_per_block,
                                                                  int32_t* __restrict__ pcount, float* __restrict__ plo,
                                                                  float* __restrict__ phi) {
  __shared__ int32_t sn[kSmWaves][kWave];
  __shared__ float sf[4][kSmWaves][kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t col = (int32_t)blockIdx.x * kWave + lane;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
  SmAcc a{0, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX};
  if (col < K) {                                              // the tail tile: lanes past K read nothing
#pragma unroll 4
    for (int64_t r = r0 + wave; r < r1; r += kSmWaves) {
      const float v = soft[r * K + col];
      const float x = xyz[3 * r], y = xyz[3 * r + 1];
      if (v > thr) {
        ++a.n;
        a.lx = fminf(a.lx, x); a.ly = fminf(a.ly, y);
        a.hx = fmaxf(a.hx, x); a.hy = fmaxf(a.hy, y);
      }
    }
  }
  if (!sm_block_combine<kSmWaves>(a, sn, sf) || col >= K) return;
  const int64_t o = (int64_t)blockIdx.y * K + col;
  pcount[o] = a.n;
  plo[2 * o] = a.lx; plo[2 * o + 1] = a.ly;
  phi[2 * o] = a.hx; phi[2 * o + 1] = a.hy;
}

// partials [row blocks][K] -> [K]: wave w takes row blocks w, w + 16, ..., the waves are joined in wave order
__global__ __launch_bounds__(kSmFinish) void softmask_stats_finish_kernel(const int32_t* __restrict__ pcount,
                                                                          const float* __restrict__ plo,
                                                                          const float* __restrict__ phi, int32_t K,
                                                                          int32_t blocks, int32_t* __restrict__ count,
                                                                          float* __restrict__ lo, float* __restrict__ hi) {
  constexpr int NW = kSmFinish / kWave;
  __shared__ int32_t sn[NW][kWave];
  __shared__ float sf[4][NW][kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t col = (int32_t)blockIdx.x * kWave + lane;
  SmAcc a{0, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX};
  if (col < K)
    for (int32_t b = wave; b < blocks; b += NW) {
      const int64_t o = (int64_t)b * K + col;
      sm_merge(a, SmAcc{pcount[o], plo[2 * o], plo[2 * o + 1], phi[2 * o], phi[2 * o + 1]});
    }
  if (!sm_block_combine<NW>(a, sn, sf) || col >= K) return;
  count[col] = a.n;
  lo[2 * col] = a.lx; lo[2 * col + 1] = a.ly;
  hi[2 * col] = a.hx; hi[2 * col + 1] = a.hy;
}

// one wave per row, lanes over the kept columns (tiles of 64): the row of `out` is written as one contiguous run
__global__ __launch_bounds__(kSmBlock) void softmask_table_kernel(const float* __restrict__ soft, int64_t N, int32_t K,
                                                                  float thr, const int32_t* __restrict__ keep,
                                                                  int32_t Kk, const float* __restrict__ segments,
                                                                  int32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * kSmWaves + (threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * kSmWaves;
  const int64_t W = (int64_t)Kk + 2;
  const int32_t k0 = lane < Kk ? keep[lane] : 0;              // the first tile's columns stay in registers
  for (int64_t r = wave; r < N; r += waves) {
    const float* __restrict__ row = soft + r * K;
    int32_t* __restrict__ o = out + r * W;
    int any = 0;
    for (int32_t j0 = 0; j0 < Kk; j0 += kWave) {
      const int32_t j = j0 + lane;
      int bit = 0;
      if (j < Kk) {
        bit = row[j0 == 0 ? k0 : keep[j]] > thr;
        o[1 + j] = bit;
      }
      any |= __any(bit);
    }
    if (lane == 0) {
      o[0] = any != 0;
      o[Kk + 1] = (int32_t)segments[r];
    }
  }
}

// One thread per vertex: the unnormalised normals (v1 - v0) x (v2 - v0) of its faces, summed in the order of the
// corner list (ascending face index), in f64 from the f32 vertices, every operation rounded on its own.
__global__ __launch_bounds__(256) void mesh_vertex_normals_kernel(const float* __restrict__ P,
                                                                  const int32_t* __restrict__ faces,
                                                                  const int64_t* __restrict__ order,
                                                                  const int64_t* __restrict__ off, int64_t nv,
                                                                  float* __restrict__ normals) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int64_t q = off[v]; q < off[v + 1]; ++q) {
    const int64_t f = order[q] / 3;
    const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    const double ax = (double)P[3 * i1] - (double)P[3 * i0], ay = (double)P[3 * i1 + 1] - (double)P[3 * i0 + 1],
                 az = (double)P[3 * i1 + 2] - (double)P[3 * i0 + 2];
    const double bx = (double)P[3 * i2] - (double)P[3 * i0], by = (double)P[3 * i2 + 1] - (double)P[3 * i0 + 1],
                 bz = (double)P[3 * i2 + 2] - (double)P[3 * i0 + 2];
    sx += ay * bz - az * by;
    sy += az * bx - ax * bz;
    sz += ax * by - ay * bx;
  }
  const double n2 = sx * sx + sy * sy + sz * sz;
  float x = 0.f, y = 0.f, z = 1.f;
  if (n2 > 0.0 && n2 <= DBL_MAX) {                            // a zero or non-finite sum keeps (0, 0, 1)
    const double n = sqrt(n2);
    x = (float)(sx / n); y = (float)(sy / n); z = (float)(sz / n);
  }
  normals[3 * v] = x; normals[3 * v + 1] = y; normals[3 * v + 2] = z;
}

}  // namespace usc

using namespace usc;

extern "C" {

int64_t usc_softmask_stats_ws_bytes(int64_t n, int32_t k) {
  if (n < 1 || k < 1) return 0;
  return ceil_div(n, sm_rows_per_block(n)) * k * 5 * 4;
}

int usc_softmask_stats(const float* soft, const float* xyz, int64_t n, int32_t k, float thr, int32_t* count, float* lo,
                       float* hi, void* ws, int64_t ws_bytes, usc_stream_t s) {
  USC_REQUIRE(n >= 1 && n <= INT32_MAX, "usc_softmask_stats: n out of range [1, 2^31-1]");
  USC_REQUIRE(k >= 1 && k <= 65535 * kWave, "usc_softmask_stats: k out of range [1, %d]", 65535 * kWave);
  USC_REQUIRE(soft && xyz && count && lo && hi && ws, "usc_softmask_stats: null pointer");
  USC_REQUIRE(ws_bytes >= usc_softmask_stats_ws_bytes(n, k), "usc_softmask_stats: workspace too small");
  const int64_t rpb = sm_rows_per_block(n);
  const int64_t blocks = ceil_div(n, rpb);
  int32_t* pcount = (int32_t*)ws;
  float* plo = (float*)ws + blocks * k;
  float* phi = plo + 2 * blocks * k;
  hipStream_t st = as_stream(s);
  const unsigned tiles = (unsigned)ceil_div(k, kWave);
  hipLaunchKernelGGL(softmask_stats_kernel, dim3(tiles, (unsigned)blocks), dim3(kSmBlock), 0, st, soft, xyz, n, k, thr,
                     rpb, pcount, plo, phi);
  USC_CHECK_LAUNCH("usc_softmask_stats");
  hipLaunchKernelGGL(softmask_stats_finish_kernel, dim3(tiles), dim3(kSmFinish), 0, st, pcount, plo, phi, k,
                     (int32_t)blocks, count, lo, hi);
  USC_CHECK_LAUNCH("usc_softmask_stats");
  return USC_OK;
}

int usc_softmask_table(const float* soft, int64_t n, int32_t k, float thr, const int32_t* keep, int32_t kk,
                       const float* segments, int32_t* out, usc_stream_t s) {
  USC_REQUIRE(n >= 0 && n <= INT32_MAX, "usc_softmask_table: n out of range [0, 2^31-1]");
  USC_REQUIRE(k >= 1 && kk >= 1 && kk <= k, "usc_softmask_table: needs 1 <= kk <= k (every keep entry in [0, k))");
  if (n == 0) return USC_OK;
  USC_REQUIRE(soft && keep && segments && out, "usc_softmask_table: null pointer");
  hipLaunchKernelGGL(softmask_table_kernel, dim3((unsigned)stream_grid(n, kSmWaves)), dim3(kSmBlock), 0, as_stream(s),
                     soft, n, k, thr, keep, kk, segments, out);
  USC_CHECK_LAUNCH("usc_softmask_table");
  return USC_OK;
}

int usc_mesh_vertex_normals(const float* vertices, const int32_t* faces, const int64_t* corner_order,
                            const int64_t* vertex_off, int64_t n_vertices, int64_t n_faces, float* normals,
                            usc_stream_t s) {
  USC_REQUIRE(n_vertices >= 0 && n_vertices <= INT32_MAX && n_faces >= 0, "usc_mesh_vertex_normals: bad size");
  if (n_vertices == 0) return USC_OK;
  USC_REQUIRE(vertices && vertex_off && normals && (n_faces == 0 || (faces && corner_order)),
              "usc_mesh_vertex_normals: null pointer");
  hipLaunchKernelGGL(mesh_vertex_normals_kernel, dim3((unsigned)ceil_div(n_vertices, 256)), dim3(256), 0, as_stream(s),
                     vertices, faces, corner_order, vertex_off, n_vertices, normals);
  USC_CHECK_LAUNCH("usc_mesh_vertex_normals");
  return USC_OK;
}

}  // extern "C"
