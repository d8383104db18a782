// separate.hip — `general.separate_instances` of the export step (reference trainer/trainer.py:609-650): every kept
// instance is cut into its connected parts on the adjacency of the mesh over-segmentation.
//
// The reference loops over the instances in Python (np.unique of the masked ids, a scan over sets, one np.isin over all
// points per part).  Here an instance is an S-bit row of segments between two passes over the [N, K] table:
//
//   usc_mask_columns_to_segment_bits  bool[N, K] columns -> u64[K, ceil(S/64)]: bit s of row j = any point of segment s
//                                     has column j set (:626-629); points walked in the CSR order of their segments
//   usc_mask_bits_components_wide     usc_mask_bits_components (freemask_segments.hip) with the labels of a row in
//                                     global memory instead of LDS: S up to 65 536
//   usc_segment_parts_to_columns      one u8 column per (instance, part): the points whose segment carries the part's
//                                     label (:639)
//
// Explicit stream, no allocation, no float, no read-modify-write atomics, no workgroup waits for another; every output
// element has one writer, so two runs give the same bytes.
#include "common.h"

namespace usc {
namespace {

constexpr int kSepBlock = 1024;                       // 16 waves
constexpr int kSepWaves = kSepBlock / kWave;
constexpr int kSepSegPerWave = 64 / kSepWaves;        // a workgroup owns 64 segments (one output word per column)
constexpr int kWideBlock = 1024;
constexpr int kWideWaves = kWideBlock / kWave;
constexpr int kColBlock = 256;

// grid (ceil(S / 64), ceil(K / 64)).  Lane = column.  Wave v takes segments 64 g + 4 v .. + 3: the point indices of a
// segment are read 64 at a time (coalesced) and broadcast, every lane reads its byte of the point's row (64 consecutive
// bytes per wave) and keeps one "any" flag; the 16 partial words of a column meet in LDS.
__global__ __launch_bounds__(kSepBlock) void mask_columns_to_segment_bits_kernel(
    const uint8_t* __restrict__ masks, int64_t n, int32_t k, const int64_t* __restrict__ order,
    const int64_t* __restrict__ seg_off, int32_t S, int64_t W, uint64_t* __restrict__ bits) {
  __shared__ uint64_t part[kSepWaves][kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g = blockIdx.x;
  const int32_t c = (int32_t)blockIdx.y * 64 + lane;
  const bool col_ok = c < k;
  const uint8_t* __restrict__ col = masks + (col_ok ? c : 0);
  uint64_t word = 0;
#pragma unroll 1
  for (int b = wave * kSepSegPerWave; b < (wave + 1) * kSepSegPerWave; ++b) {
    const int64_t s = g * 64 + b;
    if (s >= S) break;
    const int64_t e1 = min(seg_off[s + 1], n);                    // a broken CSR never indexes order[] outside [0, n)
    uint32_t any = 0;
    for (int64_t e0 = max(seg_off[s], (int64_t)0); e0 < e1; e0 += 64) {
      const int cnt = (int)(e1 - e0 < 64 ? e1 - e0 : 64);
      int64_t mine = order[e0 + (lane < cnt ? lane : 0)];          // lanes past the end repeat the first point: OR
      if ((uint64_t)mine >= (uint64_t)n) mine = 0;                // never read outside the table
      for (int i0 = 0; i0 < cnt; i0 += 8) {                       // 8 independent row reads in flight per lane
        uint32_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = col[__shfl(mine, i0 + j, 64) * k];
#pragma unroll
        for (int j = 0; j < 8; ++j) any |= v[j];
      }
    }
    word |= (uint64_t)(any != 0 && col_ok) << b;
  }
  part[wave][lane] = word;
  __syncthreads();
  if (wave == 0 && col_ok) {
#pragma unroll
    for (int v = 1; v < kSepWaves; ++v) word |= part[v][lane];
    bits[(int64_t)c * W + g] = word;
  }
}

__device__ inline bool sep_row_bit(const uint64_t* __restrict__ row, int s) { return (row[s >> 6] >> (s & 63)) & 1; }

// plain loads and stores of a label another thread of the workgroup may rewrite: kept out of registers across rounds
__device__ inline int32_t label_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ inline void label_store(int32_t* p, int32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// One workgroup per row; the row of label_out is the work array.  Same invariants as mask_bits_components_kernel:
// label[s] <= s, only the owner of s writes label[s], every value written is the label of a vertex of the same part.
// A round reads at least what the round before wrote (the barrier publishes the workgroup's stores), so the labels are
// never above those of the synchronous propagation, which is quiet after at most S rounds: the bound S + 1 is reached
// only by a broken run, which sets *status and leaves.
__global__ __launch_bounds__(kWideBlock) void mask_bits_components_wide_kernel(
    const uint64_t* __restrict__ bits, int64_t W, const int32_t* __restrict__ rows, int32_t S,
    const int64_t* __restrict__ adj_off, const int32_t* __restrict__ adj, int32_t* label_out,
    int32_t* __restrict__ n_comp, int32_t* __restrict__ status) {
  __shared__ int32_t s_count[kWideWaves];
  const uint64_t* __restrict__ row = bits + (int64_t)rows[blockIdx.x] * W;
  int32_t* label = label_out + (int64_t)blockIdx.x * S;
  for (int s = threadIdx.x; s < S; s += kWideBlock) label_store(label + s, sep_row_bit(row, s) ? s : -1);
  __syncthreads();
  int changed = 1;
  for (int64_t round = 0; round <= S; ++round) {
    changed = 0;
    for (int s = threadIdx.x; s < S; s += kWideBlock) {
      const int32_t cur = label_load(label + s);
      if (cur < 0) continue;
      int32_t m = cur;
      const int64_t e1 = adj_off[s + 1];
      for (int64_t e = adj_off[s]; e < e1; ++e) {
        const int32_t l = label_load(label + adj[e]);
        if (l >= 0) m = min(m, l);
      }
      m = min(m, label_load(label + m));                   // one pointer jump: label[m] >= 0 (m is in the mask)
      if (m < cur) {
        label_store(label + s, m);
        changed = 1;
      }
    }
    changed = __syncthreads_or(changed);
    if (!changed) break;
  }
  if (changed && threadIdx.x == 0) *status = 1;            // a plain vector store; every writer writes the same value
  int mine = 0;
  for (int s = threadIdx.x; s < S; s += kWideBlock) mine += label_load(label + s) == s;
  mine = wave_reduce_add(mine);
  if ((threadIdx.x & 63) == 0) s_count[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t total = 0;
#pragma unroll
    for (int v = 0; v < kWideWaves; ++v) total += s_count[v];
    n_comp[blockIdx.x] = total;
  }
}

// thread per output byte, parts fastest: consecutive threads write consecutive bytes of a point's row and read the
// labels of one segment (one address per input row)
__global__ __launch_bounds__(kColBlock) void segment_parts_to_columns_kernel(
    const int32_t* __restrict__ label, int32_t S, const int32_t* __restrict__ src, const int32_t* __restrict__ root,
    int32_t R, const int32_t* __restrict__ idx, int64_t n, uint8_t* __restrict__ out) {
  const int64_t total = n * R;
  for (int64_t e = (int64_t)blockIdx.x * kColBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kColBlock) {
    const int64_t r = e / R;
    const int32_t p = (int32_t)(e - r * R);
    out[e] = label[(int64_t)src[p] * S + idx[r]] == root[p];
  }
}

}  // namespace
}  // namespace usc

using namespace usc;

extern "C" {

int32_t usc_mask_bits_max_segments_wide(void) { return USC_MASK_BITS_MAX_SEGMENTS_WIDE; }

int usc_mask_columns_to_segment_bits(const uint8_t* masks, int64_t n, int32_t k, const int64_t* order,
                                     const int64_t* seg_off, int32_t n_segments, uint64_t* bits, usc_stream_t s) {
  USC_REQUIRE(n >= 1 && n <= (int64_t)INT32_MAX, "usc_mask_columns_to_segment_bits: n out of range [1, 2^31-1]");
  USC_REQUIRE(k >= 0 && k <= (1 << 20), "usc_mask_columns_to_segment_bits: k out of range [0, 2^20]");
  USC_REQUIRE(n_segments >= 1 && n_segments <= USC_MASK_BITS_MAX_SEGMENTS_WIDE,
              "usc_mask_columns_to_segment_bits: %d segments outside [1, %d]", n_segments,
              USC_MASK_BITS_MAX_SEGMENTS_WIDE);
  if (k == 0) return USC_OK;
  USC_REQUIRE(masks && order && seg_off && bits, "usc_mask_columns_to_segment_bits: null pointer");
  const int64_t W = ceil_div(n_segments, 64);
  hipLaunchKernelGGL(mask_columns_to_segment_bits_kernel, dim3((unsigned)W, (unsigned)ceil_div(k, 64)), dim3(kSepBlock),
                     0, as_stream(s), masks, n, k, order, seg_off, n_segments, W, bits);
  USC_CHECK_LAUNCH("usc_mask_columns_to_segment_bits");
  return USC_OK;
}

int usc_mask_bits_components_wide(const uint64_t* bits, int64_t n_bits_rows, int32_t n_segments, const int32_t* rows,
                                  int32_t n_rows, const int64_t* adj_off, const int32_t* adj, int32_t* label,
                                  int32_t* n_comp, int32_t* status, usc_stream_t s) {
  USC_REQUIRE(n_segments >= 1 && n_segments <= USC_MASK_BITS_MAX_SEGMENTS_WIDE,
              "usc_mask_bits_components_wide: %d segments outside [1, %d] (one workgroup walks a row's labels; above "
              "this count a round is too long for one workgroup)",
              n_segments, USC_MASK_BITS_MAX_SEGMENTS_WIDE);
  USC_REQUIRE(n_rows >= 0 && n_bits_rows >= 0, "usc_mask_bits_components_wide: bad sizes");
  if (n_rows == 0) return USC_OK;
  USC_REQUIRE(bits && rows && adj_off && label && n_comp && status, "usc_mask_bits_components_wide: null pointer");
  hipStream_t st = as_stream(s);
  int32_t host_status = 0;
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(mask_bits_components_wide_kernel, dim3((unsigned)n_rows), dim3(kWideBlock), 0, st, bits,
                       ceil_div(n_segments, 64), rows, n_segments, adj_off, adj, label, n_comp, status);
    USC_CHECK_LAUNCH("usc_mask_bits_components_wide");
    e = hipMemcpyAsync(&host_status, status, sizeof(int32_t), hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    set_error("usc_mask_bits_components_wide: HIP runtime error: %s", hipGetErrorString(e));
    return USC_ERR_LAUNCH;
  }
  if (host_status != 0) {
    set_error("usc_mask_bits_components_wide: the labels of a row were not quiet after %d + 1 rounds (the adjacency "
              "is not the symmetric CSR the contract asks for, or the labels were written from outside)", n_segments);
    return USC_ERR_RANGE;
  }
  return USC_OK;
}

int usc_segment_parts_to_columns(const int32_t* label, int32_t n_rows, int32_t n_segments, const int32_t* src,
                                 const int32_t* root, int32_t n_parts, const int32_t* idx, int64_t n, uint8_t* out,
                                 usc_stream_t s) {
  USC_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, "usc_segment_parts_to_columns: n out of range [0, 2^31-1]");
  USC_REQUIRE(n_rows >= 0 && n_segments >= 1 && n_parts >= 0 && n_parts <= (1 << 20),
              "usc_segment_parts_to_columns: bad sizes");
  if (n == 0 || n_parts == 0) return USC_OK;
  USC_REQUIRE(label && src && root && idx && out, "usc_segment_parts_to_columns: null pointer");
  hipLaunchKernelGGL(segment_parts_to_columns_kernel, dim3(stream_grid(n * n_parts, kColBlock)), dim3(kColBlock), 0,
                     as_stream(s), label, n_segments, src, root, n_parts, idx, n, out);
  USC_CHECK_LAUNCH("usc_segment_parts_to_columns");
  return USC_OK;
}

}  // extern "C"
