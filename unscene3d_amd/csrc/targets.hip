// targets.hip — instance targets of the supervised collate (reference datasets/utils.py:529-613, get_instance_masks).
//
// The reference loops over the instance ids of a label table [semantic label, instance id, segment id]: per instance
// several full-length passes and a branch on a tensor value.  Here one table is three launches and no per-instance
// work on the host:
//
//   index   every row finds the rank of its instance id among the U distinct ids (binary search in the sorted list);
//           a workgroup counts rows and takes the minimum row index per id in LDS, then adds / mins its non-empty
//           entries into count[U] / first[U].  Integers: the result does not depend on the order of the atomics.
//           An LDS window holds kTgtWindow ids; more ids -> grid.y windows, each counting only its own ranks.
//   select  one workgroup walks the ids in ascending order: id -1, ids without rows and ids whose label (column 0 of
//           the id's FIRST row) is filtered are dropped, the others take slots 0..T-1 by a block-wide prefix sum;
//           labels_out[t] = max(label - label_offset, 0), *n_kept = T.
//   masks   masks u8[T, N], masks[t, r] = (slot[rank[r]] == t).  A wave owns 256 consecutive rows r and keeps their
//           slots in registers (lane l: rows base + l + 64 k).  Per target row t it takes four 64-bit ballots — 256
//           result bits in row order — and lane j stores the aligned 4-byte word j of that stretch, its four bits
//           cut from the ballots at the row's byte misalignment (N need not be a multiple of 4, so every row of the
//           output starts at another alignment).  One 256-byte contiguous store per wave and row; the <= 3 bytes in
//           front of the first and behind the last aligned word are byte stores.  Every output byte is written
//           exactly once, zeros included: no memset pass.  grid.y splits T into groups of kTgtRowsPerBlock rows.
//           With segments, the y = 0 workgroups also set segment_mask[slot, segment id of the row] = 1 with plain
//           byte stores into the caller's zeroed table (all writers write the same value).
#include "common.h"

namespace usc {

constexpr int kTgtBlock = 256;
constexpr int kTgtWindow = 2048;          // ids of one LDS window (16 KiB: count + first)
constexpr int kTgtWaveRows = 256;         // rows of one wave in the mask kernel (4 per lane)
constexpr int kTgtRowsPerBlock = 8;       // target rows of one workgroup in the mask kernel

__global__ void instance_index_init_kernel(int32_t u, int32_t* __restrict__ count, int32_t* __restrict__ first) {
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < u; i += gridDim.x * blockDim.x) {
    count[i] = 0;
    first[i] = INT32_MAX;
  }
}

// index of v in the ascending list ids[u], or -1
__device__ inline int32_t find_rank(const int64_t* __restrict__ ids, int32_t u, int64_t v) {
  int32_t lo = 0, hi = u;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (ids[mid] < v) lo = mid + 1; else hi = mid;
  }
  return (lo < u && ids[lo] == v) ? lo : -1;
}

__global__ __launch_bounds__(kTgtBlock) void instance_index_kernel(const int64_t* __restrict__ labels, int64_t n,
                                                                   int32_t ld, const int64_t* __restrict__ ids,
                                                                   int32_t u, int32_t* __restrict__ rank,
                                                                   int32_t* __restrict__ count,
                                                                   int32_t* __restrict__ first) {
  __shared__ int32_t cnt[kTgtWindow], fst[kTgtWindow];
  const int32_t u0 = blockIdx.y * kTgtWindow;
  const int32_t w = min(kTgtWindow, u - u0);
  for (int i = threadIdx.x; i < w; i += kTgtBlock) {
    cnt[i] = 0;
    fst[i] = INT32_MAX;
  }
  __syncthreads();
  for (int64_t r = (int64_t)blockIdx.x * kTgtBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kTgtBlock) {
    const int32_t k = find_rank(ids, u, labels[r * ld + 1]);
    if (blockIdx.y == 0) rank[r] = k;
    const uint32_t j = (uint32_t)(k - u0);
    if (k >= 0 && j < (uint32_t)w) {
      atomicAdd(&cnt[j], 1);
      atomicMin(&fst[j], (int32_t)r);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < w; i += kTgtBlock) {
    if (cnt[i]) {
      atomicAdd(&count[u0 + i], cnt[i]);
      atomicMin(&first[u0 + i], fst[i]);
    }
  }
}

__global__ __launch_bounds__(kTgtBlock) void instance_select_kernel(const int64_t* __restrict__ labels, int32_t ld,
                                                                    const int64_t* __restrict__ ids, int32_t u,
                                                                    const int32_t* __restrict__ count,
                                                                    const int32_t* __restrict__ first,
                                                                    const int64_t* __restrict__ filter, int32_t nf,
                                                                    int64_t label_offset, int32_t* __restrict__ slot,
                                                                    int64_t* __restrict__ labels_out,
                                                                    int32_t* __restrict__ n_kept) {
  __shared__ int32_t wsum[kTgtBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t base = 0;                                  // slots taken by the ids in front of this chunk
  for (int32_t c0 = 0; c0 < u; c0 += kTgtBlock) {
    const int32_t i = c0 + threadIdx.x;
    bool keep = false;
    int64_t lab = 0;
    if (i < u && ids[i] != -1 && count[i] > 0) {
      lab = labels[(int64_t)first[i] * ld];          // the label of the instance's first row decides
      keep = true;
      for (int32_t f = 0; f < nf; ++f) keep = keep && filter[f] != lab;
    }
    const int inc = wave_inclusive_scan(keep ? 1 : 0);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int32_t off = base, total = 0;
#pragma unroll
    for (int wv = 0; wv < kTgtBlock / 64; ++wv) {
      if (wv < wave) off += wsum[wv];
      total += wsum[wv];
    }
    if (i < u) {
      const int32_t t = off + inc - 1;
      slot[i] = keep ? t : -1;
      if (keep) {
        const int64_t v = lab - label_offset;
        labels_out[t] = v > 0 ? v : 0;
      }
    }
    base += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_kept = base;
}

__device__ inline uint32_t ballot_bit(uint64_t b0, uint64_t b1, uint64_t b2, uint64_t b3, int i) {
  const int q = i >> 6;
  const uint64_t b = q == 0 ? b0 : q == 1 ? b1 : q == 2 ? b2 : b3;
  return (uint32_t)(b >> (i & 63)) & 1u;
}

__global__ __launch_bounds__(kTgtBlock) void instance_masks_kernel(const int32_t* __restrict__ rank, int64_t n,
                                                                   const int32_t* __restrict__ slot, int32_t u,
                                                                   int32_t t_total, uint8_t* __restrict__ masks,
                                                                   const int64_t* __restrict__ seg, int32_t seg_ld,
                                                                   int64_t s, uint8_t* __restrict__ segment_mask) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t base = ((int64_t)blockIdx.x * (kTgtBlock / 64) + wave) * kTgtWaveRows;
  if (base >= n) return;                             // wave-uniform; the kernel has no workgroup barrier
  const int len = (int)min((int64_t)kTgtWaveRows, n - base);

  int32_t sl[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t r = base + 64 * k + lane;
    sl[k] = -1;
    if (r < n) {
      const int32_t q = rank[r];
      if ((uint32_t)q < (uint32_t)u) {
        const int32_t t = slot[q];
        if ((uint32_t)t < (uint32_t)t_total) sl[k] = t;
      }
    }
  }
  if (segment_mask != nullptr && blockIdx.y == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (sl[k] >= 0) {
        const int64_t sg = seg[(base + 64 * k + lane) * seg_ld];
        if ((uint64_t)sg < (uint64_t)s) segment_mask[(int64_t)sl[k] * s + sg] = 1;
      }
    }
  }

  const int t0 = blockIdx.y * kTgtRowsPerBlock;
  const int t1 = min(t_total, t0 + kTgtRowsPerBlock);
  for (int t = t0; t < t1; ++t) {
    // bit i of (b0, b1, b2, b3) = masks[t, base + i]
    const uint64_t b0 = __ballot(sl[0] == t), b1 = __ballot(sl[1] == t);
    const uint64_t b2 = __ballot(sl[2] == t), b3 = __ballot(sl[3] == t);
    uint8_t* row = masks + (int64_t)t * n + base;
    const int m = (int)((uintptr_t)row & 3);         // bytes of this stretch in front of the first aligned word
    const int j_lo = m ? 1 : 0;                      // aligned word j covers the bytes 4 j - m .. 4 j - m + 3
    const int j_hi = (len + m) >> 2;                 // first word that does not end inside the stretch (<= 64)
    if (lane >= j_lo && lane < j_hi) {
      const int i0 = 4 * lane - m;
      const int q = i0 >> 6, o = i0 & 63;
      const uint64_t cur = q == 0 ? b0 : q == 1 ? b1 : q == 2 ? b2 : b3;
      const uint64_t nxt = q == 0 ? b1 : q == 1 ? b2 : q == 2 ? b3 : 0;
      uint32_t bits = (uint32_t)(cur >> o);
      if (o > 60) bits |= (uint32_t)(nxt << (64 - o));
      const uint32_t word = (bits & 1u) | ((bits & 2u) << 7) | ((bits & 4u) << 14) | ((bits & 8u) << 21);
      *reinterpret_cast<uint32_t*>(row + i0) = word;
    }
    const int head_n = min(max(4 * j_lo - m, 0), len);           // bytes in front of the first full word (<= 3)
    if (lane < head_n) row[lane] = (uint8_t)ballot_bit(b0, b1, b2, b3, lane);
    const int tail = max(4 * j_hi - m, head_n) + lane;           // bytes behind the last full word (<= 3)
    if (tail < len) row[tail] = (uint8_t)ballot_bit(b0, b1, b2, b3, tail);
  }
}

}  // namespace usc

using namespace usc;

extern "C" {

int usc_instance_index(const int64_t* labels, int64_t n, int32_t ld, const int64_t* ids, int32_t u, int32_t* rank,
                       int32_t* count, int32_t* first, usc_stream_t s) {
  USC_REQUIRE(n >= 0 && n < INT32_MAX, "usc_instance_index: n out of range [0, 2^31-2]");
  USC_REQUIRE(ld >= 2, "usc_instance_index: ld < 2 (the instance id is column 1)");
  USC_REQUIRE(u >= 0 && u <= 65535 * kTgtWindow, "usc_instance_index: u out of range");
  USC_REQUIRE(u == 0 || (ids && count && first), "usc_instance_index: null pointer");
  USC_REQUIRE(n == 0 || (labels && rank), "usc_instance_index: null pointer");
  USC_REQUIRE(n == 0 || u > 0, "usc_instance_index: rows without ids");
  hipStream_t st = as_stream(s);
  if (u == 0) return USC_OK;
  hipLaunchKernelGGL(instance_index_init_kernel, dim3(stream_grid(u, kTgtBlock)), dim3(kTgtBlock), 0, st, u, count,
                     first);
  USC_CHECK_LAUNCH("usc_instance_index");
  if (n == 0) return USC_OK;
  const dim3 grid(stream_grid(n, kTgtBlock), (unsigned)ceil_div(u, kTgtWindow));
  hipLaunchKernelGGL(instance_index_kernel, grid, dim3(kTgtBlock), 0, st, labels, n, ld, ids, u, rank, count, first);
  USC_CHECK_LAUNCH("usc_instance_index");
  return USC_OK;
}

int usc_instance_select(const int64_t* labels, int64_t n, int32_t ld, const int64_t* ids, int32_t u,
                        const int32_t* count, const int32_t* first, const int64_t* filter, int32_t nf,
                        int64_t label_offset, int32_t* slot, int64_t* labels_out, int32_t* n_kept, usc_stream_t s) {
  USC_REQUIRE(n >= 0 && n < INT32_MAX, "usc_instance_select: n out of range [0, 2^31-2]");
  USC_REQUIRE(ld >= 1, "usc_instance_select: ld < 1");
  USC_REQUIRE(u >= 0, "usc_instance_select: u < 0");
  USC_REQUIRE(nf >= 0 && (nf == 0 || filter), "usc_instance_select: bad filter list");
  USC_REQUIRE(n_kept, "usc_instance_select: null n_kept");
  USC_REQUIRE(u == 0 || (labels && ids && count && first && slot && labels_out), "usc_instance_select: null pointer");
  hipLaunchKernelGGL(instance_select_kernel, dim3(1), dim3(kTgtBlock), 0, as_stream(s), labels, ld, ids, u, count,
                     first, filter, nf, label_offset, slot, labels_out, n_kept);
  USC_CHECK_LAUNCH("usc_instance_select");
  return USC_OK;
}

int usc_instance_masks(const int32_t* rank, int64_t n, const int32_t* slot, int32_t u, int32_t t, uint8_t* masks,
                       const int64_t* seg, int32_t seg_ld, int64_t n_segments, uint8_t* segment_mask,
                       usc_stream_t s) {
  USC_REQUIRE(n >= 0 && n < INT32_MAX, "usc_instance_masks: n out of range [0, 2^31-2]");
  USC_REQUIRE(u >= 0, "usc_instance_masks: u < 0");
  USC_REQUIRE(t >= 0 && t <= u && t <= 65535 * kTgtRowsPerBlock, "usc_instance_masks: t out of range [0, u]");
  USC_REQUIRE(n_segments >= 0, "usc_instance_masks: n_segments < 0");
  if (t == 0 || n == 0) return USC_OK;
  USC_REQUIRE(rank && slot && masks, "usc_instance_masks: null pointer");
  if (n_segments == 0) segment_mask = nullptr;
  USC_REQUIRE(segment_mask == nullptr || (seg && seg_ld >= 1), "usc_instance_masks: segment_mask without segment ids");
  const dim3 grid((unsigned)ceil_div(n, (kTgtBlock / 64) * kTgtWaveRows), (unsigned)ceil_div(t, kTgtRowsPerBlock));
  hipLaunchKernelGGL(instance_masks_kernel, grid, dim3(kTgtBlock), 0, as_stream(s), rank, n, slot, u, t, masks, seg,
                     seg_ld, n_segments, segment_mask);
  USC_CHECK_LAUNCH("usc_instance_masks");
  return USC_OK;
}

}  // extern "C"
