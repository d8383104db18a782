// freemask_segments.hip — the FreeMask pseudo-mask generator's segment mode (reference pseudo_masks/freemask_main.py
// :186-233, :282-350, :359-370) on the packed rows of freemask.hip.
//
// In segment mode keys and queries are the S segment features, a mask is a set of whole segments, and every voxel-level
// quantity of the pipeline (mask size, extent, pairwise intersection) is a function of the S-bit row and the
// per-segment tables w[s] (key voxels of segment s) and lo[s] / hi[s] (their box).  Nothing of size rows x K_voxels
// exists before the survivors' rows are formed.
//
//   usc_maxpool_down2_i32        segment ids to the key resolution: max over the present children of the k2/s2 child
//                                table (the reference pools the ids as floats through MinkowskiMaxPooling, :189-199)
//   usc_mask_bits_components     connected parts of every row's mask on the segment adjacency (CSR): one workgroup per
//                                row, labels in LDS, min-label propagation with one pointer jump per visit, until a round
//                                changes nothing (replaces the Python scan over sets of :288-327)
//   usc_mask_bits_split          one packed row per (input row, part) in (row, root) order, with its segment count,
//                                its voxel count sum w and its sum of soft values in ascending segment order
//                                (:329-348 without the f32 [parts, S] matrix; the numerators of :353)
//   usc_mask_bits_nms_weighted   lives in freemask.hip (the fill kernel's WEIGHTED instantiation)
//
// Labels: label[s] <= s always, only the thread that owns s writes label[s], and every value written is the label of a
// vertex of the same component, so the rounds converge to the one fixed point "smallest index of the component"
// whatever the interleaving: two runs give the same bits although the number of rounds may differ.
#include "common.h"

namespace usc {
namespace {

constexpr int kSegBlock = 256;
constexpr int kSegMaxS = USC_MASK_BITS_MAX_SEGMENTS;      // labels i32[S] (32 KB) + roots u16[S] (16 KB) of LDS
constexpr int kSegMaxW = kSegMaxS / 64;

__global__ __launch_bounds__(256) void maxpool_down2_i32_kernel(const int32_t* __restrict__ in, int64_t n_fine,
                                                                const int32_t* __restrict__ nbr2, int64_t n_coarse,
                                                                int32_t* __restrict__ out) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_coarse; p += (int64_t)gridDim.x * blockDim.x) {
    int32_t m = -1;                                        // a parent without a present child (no map builds one)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int ch = nbr2[(int64_t)k * n_coarse + p];
      if (ch >= 0 && ch < n_fine) m = max(m, in[ch]);
    }
    out[p] = m;
  }
}

__device__ inline bool row_bit(const uint64_t* __restrict__ row, int s) { return (row[s >> 6] >> (s & 63)) & 1; }

__global__ __launch_bounds__(kSegBlock) void mask_bits_components_kernel(const uint64_t* __restrict__ bits, int64_t W,
                                                                         const int32_t* __restrict__ rows, int32_t S,
                                                                         const int64_t* __restrict__ adj_off,
                                                                         const int32_t* __restrict__ adj,
                                                                         int32_t* __restrict__ label_out,
                                                                         int32_t* __restrict__ n_comp) {
  extern __shared__ int32_t label[];                       // [S]
  __shared__ int32_t s_count;
  const uint64_t* row = bits + (int64_t)rows[blockIdx.x] * W;
  for (int s = threadIdx.x; s < S; s += kSegBlock) label[s] = row_bit(row, s) ? s : -1;
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  int changed;
  do {
    changed = 0;
    for (int s = threadIdx.x; s < S; s += kSegBlock) {
      const int32_t cur = label[s];
      if (cur < 0) continue;
      int32_t m = cur;
      const int64_t e1 = adj_off[s + 1];
      for (int64_t e = adj_off[s]; e < e1; ++e) {
        const int32_t l = label[adj[e]];
        if (l >= 0) m = min(m, l);
      }
      m = min(m, label[m]);                                // one pointer jump: label[m] >= 0 (m is in the mask)
      if (m < cur) {
        label[s] = m;
        changed = 1;
      }
    }
  } while (__syncthreads_or(changed));
  int mine = 0;
  int32_t* out = label_out + (int64_t)blockIdx.x * S;
  for (int s = threadIdx.x; s < S; s += kSegBlock) {
    const int32_t l = label[s];
    out[s] = l;
    mine += l == s;
  }
  mine = wave_reduce_add(mine);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_count, mine);   // integers: order-free
  __syncthreads();
  if (threadIdx.x == 0) n_comp[blockIdx.x] = s_count;
}

// one workgroup per input row; output row row_off[r] + (rank of the part's root among the row's roots)
__global__ __launch_bounds__(kSegBlock) void mask_bits_split_kernel(const int32_t* __restrict__ label_in, int32_t S,
                                                                    int64_t W, const int64_t* __restrict__ row_off,
                                                                    const int32_t* __restrict__ n_comp,
                                                                    const int32_t* __restrict__ weight,
                                                                    const float* __restrict__ soft, int64_t soft_ld,
                                                                    const int32_t* __restrict__ soft_row,
                                                                    uint64_t* __restrict__ out_bits,
                                                                    int32_t* __restrict__ out_src,
                                                                    int32_t* __restrict__ out_root,
                                                                    int32_t* __restrict__ seg_count,
                                                                    int32_t* __restrict__ vox_count,
                                                                    float* __restrict__ soft_sum) {
  extern __shared__ int32_t lds[];
  int32_t* label = lds;                                    // [S]
  uint16_t* roots = reinterpret_cast<uint16_t*>(lds + S);  // [S] roots in ascending order (S <= 8192 fits 16 bits)
  __shared__ uint64_t rootmask[kSegMaxW];
  __shared__ int32_t prefix[kSegMaxW];
  const int r = blockIdx.x;
  const int nc = n_comp[r];
  if (nc == 0) return;
  const int32_t* lab = label_in + (int64_t)r * S;
  for (int s = threadIdx.x; s < S; s += kSegBlock) label[s] = lab[s];
  __syncthreads();
  for (int w = threadIdx.x; w < W; w += kSegBlock) {
    uint64_t m = 0;
    const int s1 = min(64, S - w * 64);
    for (int b = 0; b < s1; ++b) m |= (uint64_t)(label[w * 64 + b] == w * 64 + b) << b;
    rootmask[w] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t acc = 0;
    for (int w = 0; w < W; ++w) {
      prefix[w] = acc;
      acc += __popcll(rootmask[w]);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < S; s += kSegBlock)
    if (label[s] == s) {
      const int rank = prefix[s >> 6] + __popcll(rootmask[s >> 6] & ((1ull << (s & 63)) - 1));
      if (rank < nc) roots[rank] = (uint16_t)s;
    }
  __syncthreads();
  const int64_t o0 = row_off[r];
  // the packed rows: thread per (part, word)
  for (int64_t e = threadIdx.x; e < (int64_t)nc * W; e += kSegBlock) {
    const int c = (int)(e / W), w = (int)(e - (int64_t)c * W);
    const int32_t root = roots[c];
    uint64_t m = 0;
    const int s1 = min(64, S - w * 64);
    for (int b = 0; b < s1; ++b) m |= (uint64_t)(label[w * 64 + b] == root) << b;
    out_bits[(o0 + c) * W + w] = m;
  }
  // the sums: thread per part, segments in ascending order (every thread reads the same label: an LDS broadcast)
  const float* srow = soft + (int64_t)soft_row[r] * soft_ld;
  for (int c = threadIdx.x; c < nc; c += kSegBlock) {
    const int32_t root = roots[c];
    int32_t ns = 0, nv = 0;
    float sum = 0.f;
    for (int s = root; s < S; ++s)
      if (label[s] == root) {
        ++ns;
        nv += weight[s];
        sum += srow[s];
      }
    out_src[o0 + c] = r;
    out_root[o0 + c] = root;
    seg_count[o0 + c] = ns;
    vox_count[o0 + c] = nv;
    soft_sum[o0 + c] = sum;
  }
}

}  // namespace
}  // namespace usc

using namespace usc;

extern "C" {

int32_t usc_mask_bits_max_segments(void) { return kSegMaxS; }

int usc_maxpool_down2_i32(const int32_t* in, int64_t n_fine, const int32_t* nbr2, int64_t n_coarse, int32_t* out,
                          usc_stream_t s) {
  USC_REQUIRE(n_fine >= 0 && n_fine <= INT32_MAX && n_coarse >= 0 && n_coarse <= INT32_MAX,
              "usc_maxpool_down2_i32: sizes out of range [0, 2^31-1]");
  if (n_coarse == 0) return USC_OK;
  USC_REQUIRE(in && nbr2 && out, "usc_maxpool_down2_i32: null pointer");
  hipLaunchKernelGGL(maxpool_down2_i32_kernel, dim3(stream_grid(n_coarse, 256)), dim3(256), 0, as_stream(s), in, n_fine,
                     nbr2, n_coarse, out);
  USC_CHECK_LAUNCH("usc_maxpool_down2_i32");
  return USC_OK;
}

int usc_mask_bits_components(const uint64_t* bits, int64_t n_bits_rows, int32_t n_segments, const int32_t* rows,
                             int32_t n_rows, const int64_t* adj_off, const int32_t* adj, int32_t* label,
                             int32_t* n_comp, usc_stream_t s) {
  USC_REQUIRE(n_segments >= 1 && n_segments <= kSegMaxS,
              "usc_mask_bits_components: %d segments outside [1, %d] (the labels of a row live in LDS)", n_segments,
              kSegMaxS);
  USC_REQUIRE(n_rows >= 0 && n_bits_rows >= 0, "usc_mask_bits_components: bad sizes");
  if (n_rows == 0) return USC_OK;
  USC_REQUIRE(bits && rows && adj_off && label && n_comp, "usc_mask_bits_components: null pointer");
  hipLaunchKernelGGL(mask_bits_components_kernel, dim3((unsigned)n_rows), dim3(kSegBlock),
                     (size_t)n_segments * sizeof(int32_t), as_stream(s), bits, ceil_div(n_segments, 64), rows,
                     n_segments, adj_off, adj, label, n_comp);
  USC_CHECK_LAUNCH("usc_mask_bits_components");
  return USC_OK;
}

int usc_mask_bits_split(const int32_t* label, int32_t n_rows, int32_t n_segments, const int64_t* row_off,
                        const int32_t* n_comp, const int32_t* weight, const float* soft, int64_t soft_ld,
                        const int32_t* soft_row, uint64_t* out_bits, int32_t* out_src, int32_t* out_root,
                        int32_t* seg_count, int32_t* vox_count, float* soft_sum, usc_stream_t s) {
  USC_REQUIRE(n_segments >= 1 && n_segments <= kSegMaxS,
              "usc_mask_bits_split: %d segments outside [1, %d] (the labels of a row live in LDS)", n_segments, kSegMaxS);
  USC_REQUIRE(n_rows >= 0 && soft_ld >= n_segments, "usc_mask_bits_split: bad sizes");
  if (n_rows == 0) return USC_OK;
  USC_REQUIRE(label && row_off && n_comp && weight && soft && soft_row && out_bits && out_src && out_root && seg_count &&
                  vox_count && soft_sum,
              "usc_mask_bits_split: null pointer");
  const size_t lds = (size_t)n_segments * sizeof(int32_t) + (size_t)align_up(n_segments, 2) * sizeof(uint16_t);
  hipLaunchKernelGGL(mask_bits_split_kernel, dim3((unsigned)n_rows), dim3(kSegBlock), lds, as_stream(s), label,
                     n_segments, ceil_div(n_segments, 64), row_off, n_comp, weight, soft, soft_ld, soft_row, out_bits,
                     out_src, out_root, seg_count, vox_count, soft_sum);
  USC_CHECK_LAUNCH("usc_mask_bits_split");
  return USC_OK;
}

}  // extern "C"
