// evaluate.hip — validation metric support (reference benchmark/evaluate_semantic_instance.py:311-361,
// `assign_instances_for_scan_with_gt`): the point overlap of every predicted mask with every GT instance.
//
// The reference computes it as an O(K·G·N) loop of np.logical_and / count_nonzero over [N] boolean vectors.  Here it is
// one integer histogram: every point p has a GT slot slot[p] (an instance, or the void slot), and
//   counts[j][s] = #{p : masks[p][j] != 0 and slot[p] == s}        (j < k)
//   counts[k][s] = #{p : slot[p] == s}                             (the GT sizes: a virtual all-true column k)
// from which the host derives every intersection, mask size, void intersection and GT vert_count.
//
// Shape.  A workgroup owns one tile of (k + 1) virtual columns x slots and one contiguous range of points.  Its table
// [slot][column] lives in LDS (row stride = tile width + 1).  Lane l of a wave owns the columns l, l + 64, ... of the
// tile and the wave walks its points one by one: the slot of a point is wave-uniform (read 64 at a time with one
// coalesced load, then broadcast with readlane), the mask bytes of a point are one coalesced row segment, and each lane
// keeps its running counts in registers for as long as consecutive points share a slot.  When the slot changes the
// wave adds its registers to LDS: 64 distinct, consecutive words per add.  At the end the workgroup adds its non-zero
// LDS entries to `counts` with integer atomics, 64 consecutive slots of one column per wave instruction.
//
// Fast case: points grouped by slot (runs of equal slot), where a wave touches LDS once per run.  Any slot order is
// correct; in random order the wave adds to LDS once per point.  When (k + 1) x nslots does not fit the table, the
// grid tiles over columns and slots; a slot tile reads every point's slot but only the mask rows of its own points.
// Counts are integers, so the result is the same whatever order the atomics land in.
#include "common.h"

namespace usc {

constexpr int kOvBlock = 512;                  // 8 waves share one LDS table
constexpr int kOvTableWords = 16384;           // 64 KiB of LDS per workgroup at most (2+ workgroups per CU)
constexpr int kOvPointsPerBlock = 1024;        // points of one workgroup before the grid is capped

template <int CPL>
__global__ __launch_bounds__(kOvBlock) void mask_gt_overlap_kernel(const uint8_t* __restrict__ masks, int64_t n,
                                                                   int32_t k, int64_t ld,
                                                                   const int32_t* __restrict__ slot, int32_t nslots,
                                                                   int32_t st, int32_t col_tiles, int64_t chunk,
                                                                   int32_t* __restrict__ counts) {
  constexpr int CT = 64 * CPL;                 // columns of one tile
  constexpr int CTP = CT + 1;                  // LDS row stride: conflict-free in both walk orders
  constexpr int U = 8;                         // points in flight per wave (divides 64; more spills SGPRs)
  extern __shared__ int32_t tab[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ct_i = blockIdx.x % col_tiles;
  const int st_i = blockIdx.x / col_tiles;
  const int c0 = ct_i * CT;
  const int s0 = st_i * st;
  const int s_cnt = min(st, nslots - s0);      // slots of this tile
  const int c_cnt = min(CT, k + 1 - c0);       // virtual columns of this tile (column k = all true)

  for (int i = threadIdx.x; i < s_cnt * CTP; i += kOvBlock) tab[i] = 0;
  __syncthreads();

  // this workgroup's points, split into one contiguous range per wave
  const int64_t p_beg = (int64_t)blockIdx.y * chunk;
  const int64_t p_end = min(n, p_beg + chunk);
  const int64_t per_wave = (p_end - p_beg + kOvBlock / 64 - 1) / (kOvBlock / 64);
  const int64_t w_beg = min(p_end, p_beg + wave * per_wave);
  const int64_t w_end = min(p_end, w_beg + per_wave);

  int col[CPL];
  bool is_mask[CPL], is_size[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    col[j] = c0 + j * 64 + lane;
    is_mask[j] = j * 64 + lane < c_cnt && col[j] < k;
    is_size[j] = j * 64 + lane < c_cnt && col[j] == k;
  }

  int cur = -1;                                // tile-local slot the registers count for (-1: none)
  int acc[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) acc[j] = 0;

  for (int64_t g = w_beg; g < w_end; g += 64) {
    const int cnt = (int)min((int64_t)64, w_end - g);
    const int sv = lane < cnt ? slot[g + lane] - s0 : -1;
    // U points at a time: all their mask bytes are requested before the first is counted
    for (int i0 = 0; i0 < cnt; i0 += U) {
      int ss[U];
      uint8_t mv[U][CPL];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int s = __builtin_amdgcn_readlane(sv, i0 + u);   // lanes >= cnt hold -1
        ss[u] = s;
        const bool in = (unsigned)s < (unsigned)s_cnt;           // else another slot tile's point
        const uint8_t* row = masks + (g + i0 + u) * ld;
#pragma unroll
        for (int j = 0; j < CPL; ++j) mv[u][j] = (in && is_mask[j]) ? row[col[j]] : (uint8_t)0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int s = ss[u];
        if ((unsigned)s >= (unsigned)s_cnt) continue;
        if (s != cur) {
          if (cur >= 0) {
#pragma unroll
            for (int j = 0; j < CPL; ++j)
              if (acc[j]) atomicAdd(&tab[cur * CTP + j * 64 + lane], acc[j]);
          }
#pragma unroll
          for (int j = 0; j < CPL; ++j) acc[j] = 0;
          cur = s;
        }
#pragma unroll
        for (int j = 0; j < CPL; ++j) acc[j] += (is_size[j] || mv[u][j] != 0) ? 1 : 0;
      }
    }
  }
  if (cur >= 0) {
#pragma unroll
    for (int j = 0; j < CPL; ++j)
      if (acc[j]) atomicAdd(&tab[cur * CTP + j * 64 + lane], acc[j]);
  }
  __syncthreads();

  // flush: consecutive lanes take consecutive slots of one column (contiguous global words)
  for (int i = threadIdx.x; i < c_cnt * s_cnt; i += kOvBlock) {
    const int c = i / s_cnt, r = i - c * s_cnt;
    const int v = tab[r * CTP + c];
    if (v) atomicAdd(&counts[(int64_t)(c0 + c) * nslots + s0 + r], v);
  }
}

template <int CPL>
static int launch_overlap(const uint8_t* masks, int64_t n, int32_t k, int64_t ld, const int32_t* slot,
                          int32_t nslots, int32_t* counts, hipStream_t st) {
  constexpr int CT = 64 * CPL;
  const int32_t slots_per_tile = (int32_t)(nslots < kOvTableWords / (CT + 1) ? nslots : kOvTableWords / (CT + 1));
  const int32_t col_tiles = (int32_t)ceil_div(k + 1, CT);
  const int64_t tiles = (int64_t)col_tiles * ceil_div(nslots, slots_per_tile);
  // enough workgroups to fill the chip, not so many that the flush atomics dominate
  int64_t chunks = ceil_div(n, kOvPointsPerBlock);
  const int64_t max_chunks = tiles >= 2048 ? 1 : 2048 / tiles;
  if (chunks > max_chunks) chunks = max_chunks;
  const int64_t chunk = ceil_div(n, chunks);
  const size_t lds = (size_t)slots_per_tile * (CT + 1) * sizeof(int32_t);
  hipLaunchKernelGGL(mask_gt_overlap_kernel<CPL>, dim3((unsigned)tiles, (unsigned)chunks), dim3(kOvBlock), lds, st,
                     masks, n, k, ld, slot, nslots, slots_per_tile, col_tiles, chunk, counts);
  USC_CHECK_LAUNCH("usc_mask_gt_overlap");
  return USC_OK;
}

}  // namespace usc

using namespace usc;

extern "C" {

int usc_mask_gt_overlap(const uint8_t* masks, int64_t n, int32_t k, int64_t ld, const int32_t* slot, int32_t nslots,
                        int32_t* counts, usc_stream_t s) {
  USC_REQUIRE(n >= 0 && n <= INT32_MAX, "usc_mask_gt_overlap: n out of range [0, 2^31-1]");
  USC_REQUIRE(k >= 1 && k <= 4096, "usc_mask_gt_overlap: k out of range [1, 4096]");
  USC_REQUIRE(ld >= k, "usc_mask_gt_overlap: ld < k");
  USC_REQUIRE(nslots >= 1 && nslots <= 65536, "usc_mask_gt_overlap: nslots out of range [1, 65536]");
  USC_REQUIRE(counts, "usc_mask_gt_overlap: null counts");
  USC_REQUIRE(n == 0 || (masks && slot), "usc_mask_gt_overlap: null pointer");
  hipStream_t st = as_stream(s);
  if (hipMemsetAsync(counts, 0, (size_t)(k + 1) * nslots * sizeof(int32_t), st) != hipSuccess) {
    set_error("usc_mask_gt_overlap: hipMemsetAsync failed");
    return USC_ERR_LAUNCH;
  }
  if (n == 0) return USC_OK;
  if (k + 1 <= 64) return launch_overlap<1>(masks, n, k, ld, slot, nslots, counts, st);
  if (k + 1 <= 128) return launch_overlap<2>(masks, n, k, ld, slot, nslots, counts, st);
  return launch_overlap<4>(masks, n, k, ld, slot, nslots, counts, st);
}

}  // extern "C"
