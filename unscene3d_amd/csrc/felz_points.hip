// felz_points.hip — the graph of the Felzenszwalb over-segmentation for a point cloud that has no mesh: the edge set
// is the symmetrised k-NN table of usc_knn_hybrid_grid, the weights are the mesh kernel's (felz_weight.h).  The
// reference invents a mesh for such clouds (Poisson reconstruction, pseudo_masks/datasets/preprocess/stanford.py:80-135)
// only to obtain an edge set; sort and merge (usc_felz_merge_host) are shared with the mesh path.
//
// Edge rule (include/usc3d.h, F2b): row i ascending, position p < count[i] ascending, j = idx[i,p] != i; the edge
// (a=i, b=j) is emitted iff i < j, or i > j and i is not among idx[j, :count[j]].  Every undirected pair of either
// list comes out once, in (i, p) order.
//
// Three steps, no atomics: a per-row bit mask of the emitting positions (k <= 64 -> one u64 per row), the device
// exclusive scan of the masks' popcounts (scan.h), and in the scan's final pass each row writes its edges at its offset.
#include "common.h"
#include "felz_weight.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace usc {
namespace {

__global__ __launch_bounds__(256) void felz_knn_edge_mask_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ count,
                                                                 int64_t n, int k, unsigned long long* __restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int ci = min(max(count[i], 0), k);
  const int32_t* row = idx + i * k;
  unsigned long long m = 0;
  for (int p = 0; p < ci; ++p) {
    const int64_t j = row[p];
    if (j == i || j < 0 || j >= n) continue;          // an index outside [0, n) breaks the precondition: nothing is read
    bool emit = i < j;
    if (!emit) {                                      // i > j: row j (an earlier row) emits the pair when it lists i
      const int cj = min(max(count[j], 0), k);
      const int32_t* other = idx + j * k;
      bool mutual = false;
      for (int q = 0; q < cj; ++q) mutual |= other[q] == (int32_t)i;
      emit = !mutual;
    }
    if (emit) m |= 1ull << p;
  }
  mask[i] = m;
}

struct EdgeCountVal {
  const unsigned long long* mask;
  __device__ int operator()(int64_t i) const { return __popcll(mask[i]); }
};
struct EdgeEmit {
  const unsigned long long* mask;
  const int32_t* idx;
  int32_t* ea;
  int32_t* eb;
  int64_t* total;
  int64_t n;
  int k;
  __device__ void operator()(int64_t i, int64_t prefix, int v) const {
    unsigned long long m = mask[i];
    int64_t e = prefix;
    while (m) {
      const int p = __ffsll(m) - 1;
      m &= m - 1;
      ea[e] = (int32_t)i;
      eb[e] = idx[i * k + p];
      ++e;
    }
    if (i == n - 1) *total = prefix + v;
  }
};

template <bool kOriented>
__global__ __launch_bounds__(256) void felz_point_edge_weights_kernel(const float* __restrict__ P, const float* __restrict__ C,
                                                                      const float* __restrict__ N, const int32_t* __restrict__ ea,
                                                                      const int32_t* __restrict__ eb, int64_t ne, int64_t np,
                                                                      float* __restrict__ w) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  const int64_t a = ea[e], b = eb[e];
  if (a < 0 || a >= np || b < 0 || b >= np) { w[e] = INFINITY; return; }   // nothing is read through a bad endpoint
  w[e] = felz_edge_weight<kOriented>(ld3(P, a), ld3(P, b), ld3(C, a), ld3(C, b), ld3(N, a), ld3(N, b));
}

constexpr int64_t kMaxPoints = (int64_t)1 << 31;

}  // namespace
}  // namespace usc

using namespace usc;

extern "C" {

int64_t usc_felz_knn_edges_ws_bytes(int64_t n_points) {
  if (n_points < 0 || n_points >= kMaxPoints) {
    set_error("usc_felz_knn_edges_ws_bytes: n_points %lld outside [0, 2^31)", (long long)n_points);
    return -1;
  }
  return align_up(n_points * (int64_t)sizeof(unsigned long long), 16) + scan_ws_bytes(n_points);
}

int usc_felz_knn_edges(const int32_t* idx, const int32_t* count, int64_t n_points, int32_t k, int32_t* edge_a,
                       int32_t* edge_b, int64_t* n_edges, void* ws, int64_t ws_bytes, usc_stream_t s) {
  USC_REQUIRE(n_points >= 0 && n_points < kMaxPoints, "usc_felz_knn_edges: n_points %lld outside [0, 2^31)", (long long)n_points);
  USC_REQUIRE(k >= 1 && k <= 64, "usc_felz_knn_edges: k must be 1 .. 64, got %d", k);
  USC_REQUIRE(n_edges, "usc_felz_knn_edges: null pointer");
  hipStream_t st = as_stream(s);
  if (n_points == 0) {
    (void)hipMemsetAsync(n_edges, 0, sizeof(int64_t), st);
    USC_CHECK_LAUNCH("usc_felz_knn_edges");
    return USC_OK;
  }
  USC_REQUIRE(idx && count && edge_a && edge_b && ws, "usc_felz_knn_edges: null pointer");
  const int64_t mask_bytes = align_up(n_points * (int64_t)sizeof(unsigned long long), 16);
  USC_REQUIRE(ws_bytes >= mask_bytes + scan_ws_bytes(n_points), "usc_felz_knn_edges: workspace of %lld bytes, needs %lld",
              (long long)ws_bytes, (long long)(mask_bytes + scan_ws_bytes(n_points)));
  unsigned long long* mask = (unsigned long long*)ws;
  hipLaunchKernelGGL(felz_knn_edge_mask_kernel, dim3((unsigned)ceil_div(n_points, 256)), dim3(256), 0, st, idx, count, n_points,
                     (int)k, mask);
  device_exclusive_scan(EdgeCountVal{mask}, EdgeEmit{mask, idx, edge_a, edge_b, n_edges, n_points, (int)k}, n_points,
                        (char*)ws + mask_bytes, st);
  USC_CHECK_LAUNCH("usc_felz_knn_edges");
  return USC_OK;
}

int usc_felz_point_edge_weights(const float* points, const float* colors, const float* normals, int64_t n_points,
                                const int32_t* edge_a, const int32_t* edge_b, int64_t n_edges, int32_t oriented,
                                float* weights, usc_stream_t s) {
  USC_REQUIRE(n_points >= 0 && n_points < kMaxPoints && n_edges >= 0 && n_edges < ((int64_t)1 << 38),
              "usc_felz_point_edge_weights: bad sizes");
  USC_REQUIRE(oriented == 0 || oriented == 1, "usc_felz_point_edge_weights: oriented must be 0 or 1, got %d", oriented);
  if (n_edges == 0) return USC_OK;
  USC_REQUIRE(points && colors && normals && edge_a && edge_b && weights, "usc_felz_point_edge_weights: null pointer");
  const dim3 grid((unsigned)ceil_div(n_edges, 256)), block(256);
  if (oriented)
    hipLaunchKernelGGL(felz_point_edge_weights_kernel<true>, grid, block, 0, as_stream(s), points, colors, normals, edge_a,
                       edge_b, n_edges, n_points, weights);
  else
    hipLaunchKernelGGL(felz_point_edge_weights_kernel<false>, grid, block, 0, as_stream(s), points, colors, normals, edge_a,
                       edge_b, n_edges, n_points, weights);
  USC_CHECK_LAUNCH("usc_felz_point_edge_weights");
  return USC_OK;
}

}  // extern "C"
