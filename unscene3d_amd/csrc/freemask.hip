// freemask.hip — the FreeMask pseudo-mask generator's voxel mode (reference pseudo_masks/freemask_main.py:242-279,
// :352-417) without the [Q,K] similarity matrix.
//
// A FreeMask mask is a threshold on one min-max-normalised cosine row: a[q][k] = q^ . k^, a -= rowmin,
// a /= rowmax_after + 1e-9, columns of all-zero keys := 0, mask = a >= thr (utils/freemask_utils.py:8-18,
// freemask_main.py:266-268).  The reference stores a as f32[Q,K] (1.6 GB at Q = 10 k, K = 40 k) plus a bool and a float
// copy of the masks, and runs its mask NMS as a Python double loop with one device product per pair.  Here:
//
//   usc_freemask_normalize   1 / (|row| + 1e-9) per feature row and the all-zero flag of every key
//   usc_freemask_rowstats    pass 1: q^ k^T tile by tile on v_mfma_f32_32x32x2_f32, min / max per query in registers
//   usc_freemask_bits        pass 2: the same tiles again, normalised, thresholded, written as packed bits (Q*K/8 bytes)
//                            with the mask sizes and the sums of the soft values inside the mask (maskness numerators)
//   usc_mask_bits_extent     bounding box of every mask over the key coordinates of its set bits
//   usc_mask_bits_nms        greedy mask NMS over packed rows: AND + popcount "i would kill j" bit matrix, then a
//                            one-workgroup sequential scan (a dead mask suppresses nothing)
//   usc_mask_bits_nms_weighted  the same with a weight per bit (segment mode, freemask_segments.hip: a bit is a segment,
//                            its weight the segment's key voxels)
//   usc_freemask_soft_rows   the f32 rows of the few surviving queries, from the same tile code (bit-consistent with
//                            pass 2: every a[q][k] is one fixed chain of fused multiply-adds over the channels)
//
// Tile shape of the three GEMM-like kernels: a workgroup of 8 waves owns 64 queries, scaled and zero-padded in LDS
// (64 x (C8 + 4) floats: 25 KB at C = 96, 132 KB at C = 512), and a contiguous range of 32-key tiles; a wave takes every
// eighth tile, loads its 32 keys' channels once (one float4 per lane per 8 channels) and issues two MFMA chains, one per
// 32-query half.  Lane (i, h) of the accumulator holds key i of the tile and the query rows (r & 3) + 8 (r >> 2) + 4 h,
// so one wave-wide ballot per register is the 32-bit mask word of two query rows.  Traffic per pass: the keys once per
// 64 queries (Q/64 * K * C * 4 bytes, from L2 / MALL), 2 Q K C flop.  No atomics; every sum has a fixed order.
#include "common.h"

namespace usc {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

constexpr int kFmWaves = 8;
constexpr int kFmBlock = 64 * kFmWaves;
constexpr int kFmQTile = 64;
constexpr int kFmMaxSplits = 64;
constexpr float kFmEps = 1e-9f;                 // the reference's `eps = 10e-10`

enum { kFmStats = 0, kFmBits = 1, kFmSoft = 2 };

__device__ inline int fm_acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

struct FmArgs {
  const float* fq; const float* sq; const float* fk; const float* sk;
  const uint8_t* zk;                 // all-zero flag per key (bits, soft)
  const float* rmin; const float* rmax;
  const int32_t* qidx;               // soft: the query of every output row
  int64_t Q, K;                      // Q: rows of this launch (soft: M)
  int32_t C, Cp, ld;                 // channels, rounded up to 8, LDS row stride
  int32_t tiles, chunk;              // 32-key tiles in all, tiles per split (grid.y)
  float thr;
  float* pa; float* pb;              // stats: partial min / max [splits][Q]; bits: pb = partial soft sums
  int32_t* pcount;                   // bits: partial counts [splits][Q]
  uint32_t* bits; int64_t w32;       // bits: u32 words per row (2 * ceil(K / 64))
  float* soft;                       // soft: out [M][K]
};

template <int MODE, bool VEC>
__global__ __launch_bounds__(kFmBlock) void freemask_tile_kernel(FmArgs p) {
  extern __shared__ float qs[];                       // [64][ld] scaled query rows, zero beyond C and beyond Q
  __shared__ float s_lo[kFmQTile], s_den[kFmQTile];   // bits / soft: rowmin, rowmax - rowmin + eps of the tile's queries
  __shared__ float red_a[kFmWaves][kFmQTile], red_b[kFmWaves][kFmQTile];
  __shared__ int32_t red_c[kFmWaves][kFmQTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
  const int64_t q0 = (int64_t)blockIdx.x * kFmQTile;

  for (int e = threadIdx.x; e < kFmQTile * p.Cp; e += kFmBlock) {
    const int row = e / p.Cp, c = e - row * p.Cp;
    float v = 0.f;
    if (q0 + row < p.Q && c < p.C) {
      const int64_t q = MODE == kFmSoft ? (int64_t)p.qidx[q0 + row] : q0 + row;
      v = p.fq[q * p.C + c] * p.sq[q];
    }
    qs[row * p.ld + c] = v;
  }
  if (MODE != kFmStats && threadIdx.x < kFmQTile) {
    float lo = 0.f, den = 1.f;
    if (q0 + threadIdx.x < p.Q) {
      const int64_t q = MODE == kFmSoft ? (int64_t)p.qidx[q0 + threadIdx.x] : q0 + threadIdx.x;
      lo = p.rmin[q];
      den = (p.rmax[q] - lo) + kFmEps;                // max of (a - min) is fl(max - min): fl(. - min) is monotone
    }
    s_lo[threadIdx.x] = lo;
    s_den[threadIdx.x] = den;
  }
  __syncthreads();

  float va[2][16], vb[2][16];                         // stats: min, max; bits: soft sums (va)
  int32_t vc[2][16];                                  // bits: counts
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      va[f][r] = MODE == kFmStats ? INFINITY : 0.f;
      vb[f][r] = -INFINITY;
      vc[f][r] = 0;
    }

  const int t_beg = blockIdx.y * p.chunk;
  const int t_end = min(p.tiles, t_beg + p.chunk);
  const float* qa0 = qs + i * p.ld + 4 * h;
  const float* qa1 = qs + (32 + i) * p.ld + 4 * h;
  for (int t = t_beg + wave; t < t_end; t += kFmWaves) {
    const int64_t k = (int64_t)t * 32 + i;
    const bool kvalid = k < p.K;
    const float* kp = p.fk + (kvalid ? k : 0) * p.C;
    const float ks = kvalid ? p.sk[k] : 0.f;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    for (int c0 = 0; c0 < p.Cp; c0 += 8) {
      const int c = c0 + 4 * h;
      float b[4];
      if (VEC) {
        const float4 v = *reinterpret_cast<const float4*>(kp + c);
        b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = c + j < p.C ? kp[c + j] : 0.f;
      }
      const float4 a0 = *reinterpret_cast<const float4*>(qa0 + c0);
      const float4 a1 = *reinterpret_cast<const float4*>(qa1 + c0);
      const float a0v[4] = {a0.x, a0.y, a0.z, a0.w}, a1v[4] = {a1.x, a1.y, a1.z, a1.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float bj = b[j] * ks;
        acc0 = MFMA32(a0v[j], bj, acc0);
        acc1 = MFMA32(a1v[j], bj, acc1);
      }
    }
    if (MODE == kFmStats) {
      if (kvalid) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          va[0][r] = fminf(va[0][r], acc0[r]); vb[0][r] = fmaxf(vb[0][r], acc0[r]);
          va[1][r] = fminf(va[1][r], acc1[r]); vb[1][r] = fmaxf(vb[1][r], acc1[r]);
        }
      }
    } else {
      const bool kzero = kvalid && p.zk[k] != 0;
#pragma unroll
      for (int f = 0; f < 2; ++f) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 32 * f + fm_acc_row(r, h);
          const float a = f == 0 ? acc0[r] : acc1[r];
          // (the fence keeps the scheduler from interleaving all 32 unrolled divisions: that took 256 VGPRs and spilled)
          __builtin_amdgcn_sched_barrier(0);
          float v = (a - s_lo[row]) / s_den[row];
          if (kzero) v = 0.f;
          if (MODE == kFmSoft) {
            if (kvalid && q0 + row < p.Q) p.soft[(q0 + row) * p.K + k] = v;
          } else {
            const bool bit = kvalid && v >= p.thr;
            const uint64_t m = __ballot(bit);
            const uint32_t word = h ? (uint32_t)(m >> 32) : (uint32_t)m;
            if (i == 0 && q0 + row < p.Q) p.bits[(q0 + row) * p.w32 + t] = word;
            vc[f][r] += __popc(word);
            va[f][r] += bit ? v : 0.f;
          }
        }
      }
    }
  }
  if (MODE == kFmSoft) return;

  // lanes of one half -> lane i == 0 (fixed butterfly order), waves -> LDS -> one partial per split
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float x = va[f][r], y = vb[f][r];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {
        const float xo = __shfl_xor(x, o, 64);
        if (MODE == kFmStats) {
          x = fminf(x, xo);
          y = fmaxf(y, __shfl_xor(y, o, 64));
        } else {
          x += xo;
        }
      }
      if (i == 0) {
        const int row = 32 * f + fm_acc_row(r, h);
        red_a[wave][row] = x;
        if (MODE == kFmStats) red_b[wave][row] = y;
        else red_c[wave][row] = vc[f][r];
      }
    }
  __syncthreads();
  if (threadIdx.x < kFmQTile && q0 + threadIdx.x < p.Q) {
    const int row = threadIdx.x;
    const int64_t o = (int64_t)blockIdx.y * p.Q + q0 + row;
    if (MODE == kFmStats) {
      float x = red_a[0][row], y = red_b[0][row];
      for (int w = 1; w < kFmWaves; ++w) { x = fminf(x, red_a[w][row]); y = fmaxf(y, red_b[w][row]); }
      p.pa[o] = x;
      p.pb[o] = y;
    } else {
      float x = red_a[0][row];
      int32_t n = red_c[0][row];
      for (int w = 1; w < kFmWaves; ++w) { x += red_a[w][row]; n += red_c[w][row]; }
      p.pb[o] = x;
      p.pcount[o] = n;
    }
  }
}

// partials [splits][Q] -> [Q], in split order
__global__ void freemask_stats_finish_kernel(const float* __restrict__ pa, const float* __restrict__ pb, int64_t Q,
                                             int splits, float* __restrict__ rmin, float* __restrict__ rmax) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Q) return;
  float x = pa[q], y = pb[q];
  for (int s = 1; s < splits; ++s) { x = fminf(x, pa[s * Q + q]); y = fmaxf(y, pb[s * Q + q]); }
  rmin[q] = x;
  rmax[q] = y;
}

__global__ void freemask_bits_finish_kernel(const float* __restrict__ psum, const int32_t* __restrict__ pcount, int64_t Q,
                                            int splits, float* __restrict__ soft_sum, int32_t* __restrict__ count) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Q) return;
  float x = psum[q];
  int32_t n = pcount[q];
  for (int s = 1; s < splits; ++s) { x += psum[s * Q + q]; n += pcount[s * Q + q]; }
  soft_sum[q] = x;
  count[q] = n;
}

// one wave per feature row
__global__ __launch_bounds__(256) void freemask_normalize_kernel(const float* __restrict__ f, int64_t n, int32_t C,
                                                                 float* __restrict__ scale, uint8_t* __restrict__ zero) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int lane = threadIdx.x & 63;
  float ss = 0.f;
  int nz = 0;
  for (int c = lane; c < C; c += 64) {
    const float v = f[row * C + c];
    ss = fmaf(v, v, ss);
    nz |= v != 0.f;
  }
  ss = wave_reduce_addf(ss);
  nz = wave_reduce_add(nz);
  if (lane == 0) {
    scale[row] = 1.f / (sqrtf(ss) + kFmEps);
    if (zero) zero[row] = nz == 0;
  }
}

// tiles per split and number of splits of the key range: ~2048 workgroups in all, at least one tile per wave
static void fm_splits(int64_t rows, int64_t tiles, int32_t* chunk, int32_t* splits) {
  const int64_t qt = ceil_div(rows, kFmQTile);
  int64_t s = qt >= 2048 ? 1 : 2048 / qt;
  const int64_t by_tiles = ceil_div(tiles, kFmWaves);
  if (s > by_tiles) s = by_tiles;
  if (s > kFmMaxSplits) s = kFmMaxSplits;
  if (s < 1) s = 1;
  *chunk = (int32_t)ceil_div(tiles, s);
  *splits = (int32_t)ceil_div(tiles, *chunk);
}

static bool fm_vec_ok(const float* fk, int32_t C) { return C % 8 == 0 && ((uintptr_t)fk & 15) == 0; }

template <int MODE>
static int fm_launch(FmArgs& p, int64_t rows, int splits, hipStream_t st, const char* name) {
  p.Cp = (int32_t)align_up(p.C, 8);
  p.ld = p.Cp + 4;
  const size_t lds = (size_t)kFmQTile * p.ld * sizeof(float);
  const dim3 grid((unsigned)ceil_div(rows, kFmQTile), (unsigned)splits);
#define USC_FM(V)                                                                                              \
  {                                                                                                            \
    static bool attr_set = false;                                                                              \
    auto kfn = freemask_tile_kernel<MODE, V>;                                                                  \
    if (!attr_set) { /* the largest tile (C = 512); with the static arrays below the 160 KB of a workgroup */  \
      if (hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize,                    \
                              kFmQTile * (512 + 4) * (int)sizeof(float)) != hipSuccess) {                      \
        (void)hipGetLastError();                                                                               \
        set_error("%s: cannot reserve %d bytes of LDS", name, kFmQTile * (512 + 4) * (int)sizeof(float));      \
        return USC_ERR_LAUNCH;                                                                                 \
      }                                                                                                        \
      attr_set = true;                                                                                         \
    }                                                                                                          \
    hipLaunchKernelGGL(kfn, grid, dim3(kFmBlock), lds, st, p);                                                 \
  }
  if (fm_vec_ok(p.fk, p.C)) USC_FM(true) else USC_FM(false)
#undef USC_FM
  USC_CHECK_LAUNCH(name);
  return USC_OK;
}

// ---------------------------------------------------------------------------------------------- packed-mask kernels
__global__ __launch_bounds__(256) void mask_bits_extent_kernel(const uint64_t* __restrict__ bits, int64_t W, int64_t K,
                                                               const int32_t* __restrict__ coords,
                                                               int32_t* __restrict__ lo, int32_t* __restrict__ hi) {
  __shared__ int32_t red[4][6];
  const uint64_t* row = bits + (int64_t)blockIdx.x * W;
  int32_t mn[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, mx[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  for (int64_t w = threadIdx.x; w < W; w += 256) {
    uint64_t m = row[w];
    while (m) {
      const int64_t k = w * 64 + __builtin_ctzll(m);
      m &= m - 1;
      if (k < K) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const int32_t c = coords[k * 3 + d];
          mn[d] = min(mn[d], c);
          mx[d] = max(mx[d], c);
        }
      }
    }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[d] = min(mn[d], __shfl_xor(mn[d], o, 64));
      mx[d] = max(mx[d], __shfl_xor(mx[d], o, 64));
    }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { red[wave][d] = mn[d]; red[wave][3 + d] = mx[d]; }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int d = threadIdx.x;
    lo[(int64_t)blockIdx.x * 3 + d] = min(min(red[0][d], red[1][d]), min(red[2][d], red[3][d]));
    hi[(int64_t)blockIdx.x * 3 + d] = max(max(red[0][3 + d], red[1][3 + d]), max(red[2][3 + d], red[3][3 + d]));
  }
}

constexpr int kNmsChunk = 16;       // 64-bit words of every row per LDS round

// kill[a][b / 64] bit b % 64 = "mask at position a suppresses the mask at position b" for the 64 x 64 block (ta, tb),
// tb >= ta (the scan reads nothing below the diagonal block).  Thread (ty, tx) counts the 4 x 4 pairs
// (4 ty + u, 4 tx + v).  WEIGHTED (segment mode: a bit is a whole segment): the intersection is the sum of weight[s]
// over the set bits of the AND instead of their number, and `count` holds the rows' weighted sizes.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void mask_bits_nms_fill_kernel(const uint64_t* __restrict__ bits, int64_t W,
                                                                 const int32_t* __restrict__ count,
                                                                 const int32_t* __restrict__ order, int32_t n,
                                                                 float thr, uint64_t* __restrict__ kill, int32_t nW,
                                                                 const int32_t* __restrict__ weight, int64_t K) {
  const int ta = blockIdx.y, tb = blockIdx.x;
  if (tb < ta) return;
  __shared__ uint64_t sa[64][kNmsChunk + 1], sb[64][kNmsChunk + 1];
  __shared__ int32_t inter_s[64][65];
  __shared__ int32_t row_a[64], row_b[64], cnt_a[64], cnt_b[64];
  __shared__ int32_t sw[WEIGHTED ? kNmsChunk * 64 : 1];
  if (threadIdx.x < 64) {
    const int pa = ta * 64 + threadIdx.x, pb = tb * 64 + threadIdx.x;
    const int ra = pa < n ? order[pa] : -1, rb = pb < n ? order[pb] : -1;
    row_a[threadIdx.x] = ra; row_b[threadIdx.x] = rb;
    cnt_a[threadIdx.x] = ra >= 0 ? count[ra] : 0;
    cnt_b[threadIdx.x] = rb >= 0 ? count[rb] : 0;
  }
  __syncthreads();
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  int32_t inter[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) inter[u][v] = 0;
  for (int64_t w0 = 0; w0 < W; w0 += kNmsChunk) {
    for (int e = threadIdx.x; e < 64 * kNmsChunk; e += 256) {
      const int r = e / kNmsChunk, wc = e - r * kNmsChunk;
      const bool in = w0 + wc < W;
      sa[r][wc] = (in && row_a[r] >= 0) ? bits[(int64_t)row_a[r] * W + w0 + wc] : 0ull;
      sb[r][wc] = (in && row_b[r] >= 0) ? bits[(int64_t)row_b[r] * W + w0 + wc] : 0ull;
    }
    if (WEIGHTED)
      for (int e = threadIdx.x; e < 64 * kNmsChunk; e += 256) {
        const int64_t k = w0 * 64 + e;
        sw[e] = k < K ? weight[k] : 0;
      }
    __syncthreads();
#pragma unroll 4
    for (int wc = 0; wc < kNmsChunk; ++wc) {
      uint64_t xa[4], xb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { xa[u] = sa[4 * ty + u][wc]; xb[u] = sb[4 * tx + u][wc]; }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          if (WEIGHTED) {
            uint64_t m = xa[u] & xb[v];
            while (m) {
              inter[u][v] += sw[wc * 64 + __builtin_ctzll(m)];
              m &= m - 1;
            }
          } else {
            inter[u][v] += __popcll(xa[u] & xb[v]);
          }
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) inter_s[4 * ty + u][4 * tx + v] = inter[u][v];
  __syncthreads();
  if (threadIdx.x < 64 && row_a[threadIdx.x] >= 0) {
    const int a = threadIdx.x;
    uint64_t word = 0;
    for (int b = 0; b < 64; ++b) {
      if (row_b[b] < 0) continue;
      const int32_t in = inter_s[a][b];
      const int32_t uni = cnt_a[a] + cnt_b[b] - in;
      const bool k = uni > 0 ? (float)in / (float)uni > thr : true;   // reference matrix_nms, kernel='mask'
      word |= (uint64_t)k << b;
    }
    kill[(int64_t)(ta * 64 + a) * nW + tb] = word;
  }
}

// the greedy rule, sequential over positions, one workgroup: dead[] lives in LDS; per 64-position block wave 0 settles
// the block itself (64 dependent steps on one register), then every thread ORs the kill rows of the block's live
// positions into its own later words
__global__ __launch_bounds__(1024) void mask_bits_nms_scan_kernel(const uint64_t* __restrict__ kill, int32_t n,
                                                                  int32_t nW, uint8_t* __restrict__ keep) {
  extern __shared__ uint64_t dead[];
  __shared__ uint64_t s_live;
  for (int w = threadIdx.x; w < nW; w += blockDim.x) dead[w] = 0;
  __syncthreads();
  for (int B = 0; B < nW; ++B) {
    if (threadIdx.x < 64) {
      const int t = threadIdx.x;
      const int pos = B * 64 + t;
      const uint64_t kw = pos < n ? kill[(int64_t)pos * nW + B] : 0ull;
      uint64_t cur = dead[B];
      for (int s = 0; s < 64; ++s) {
        const uint64_t ks = __shfl(kw, s, 64);
        if (!((cur >> s) & 1)) cur |= ks & ~((2ull << s) - 1);     // only later positions
      }
      const int in_block = min(64, n - B * 64);
      const uint64_t valid = in_block == 64 ? ~0ull : ((1ull << in_block) - 1);
      if (t == 0) {
        dead[B] = cur;
        s_live = ~cur & valid;
      }
    }
    __syncthreads();
    const uint64_t live = s_live;
    for (int w = B + 1 + threadIdx.x; w < nW; w += blockDim.x) {
      uint64_t acc = dead[w];
      uint64_t m = live;
      while (m) {
        const int t = __builtin_ctzll(m);
        m &= m - 1;
        acc |= kill[(int64_t)(B * 64 + t) * nW + w];
      }
      dead[w] = acc;
    }
    __syncthreads();
  }
  for (int pos = threadIdx.x; pos < n; pos += blockDim.x) keep[pos] = !((dead[pos >> 6] >> (pos & 63)) & 1);
}

}  // namespace
}  // namespace usc

using namespace usc;

extern "C" {

int usc_freemask_normalize(const float* feats, int64_t n, int32_t c, float* scale, uint8_t* zero, usc_stream_t s) {
  USC_REQUIRE(n >= 0 && n <= INT32_MAX, "usc_freemask_normalize: n out of range [0, 2^31-1]");
  USC_REQUIRE(c >= 1 && c <= 512, "usc_freemask_normalize: c out of range [1, 512]");
  if (n == 0) return USC_OK;
  USC_REQUIRE(feats && scale, "usc_freemask_normalize: null pointer");
  hipLaunchKernelGGL(freemask_normalize_kernel, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, as_stream(s), feats, n, c,
                     scale, zero);
  USC_CHECK_LAUNCH("usc_freemask_normalize");
  return USC_OK;
}

int64_t usc_freemask_ws_bytes(int64_t q, int64_t k) {
  if (q < 1 || k < 1) return 0;
  int32_t chunk, splits;
  fm_splits(q, 2 * ceil_div(k, 64), &chunk, &splits);
  return (int64_t)2 * splits * q * 4;
}

#define USC_FM_COMMON(name)                                                                          \
  USC_REQUIRE(q >= 1 && q <= INT32_MAX - 64, name ": q out of range");                               \
  USC_REQUIRE(k >= 1 && k <= INT32_MAX - 64, name ": k out of range");                               \
  USC_REQUIRE(c >= 1 && c <= 512, name ": c out of range [1, 512]");                                 \
  USC_REQUIRE(fq && sq && fk && sk, name ": null pointer")

int usc_freemask_rowstats(const float* fq, const float* sq, int64_t q, const float* fk, const float* sk, int64_t k,
                          int32_t c, float* rowmin, float* rowmax, void* ws, int64_t ws_bytes, usc_stream_t s) {
  USC_FM_COMMON("usc_freemask_rowstats");
  USC_REQUIRE(rowmin && rowmax && ws, "usc_freemask_rowstats: null pointer");
  USC_REQUIRE(ws_bytes >= usc_freemask_ws_bytes(q, k), "usc_freemask_rowstats: workspace too small");
  FmArgs p = {};
  p.fq = fq; p.sq = sq; p.fk = fk; p.sk = sk; p.Q = q; p.K = k; p.C = c;
  p.tiles = (int32_t)(2 * ceil_div(k, 64));
  int32_t splits;
  fm_splits(q, p.tiles, &p.chunk, &splits);
  p.pa = (float*)ws;
  p.pb = p.pa + (int64_t)splits * q;
  hipStream_t st = as_stream(s);
  if (int rc = fm_launch<kFmStats>(p, q, splits, st, "usc_freemask_rowstats")) return rc;
  hipLaunchKernelGGL(freemask_stats_finish_kernel, dim3((unsigned)ceil_div(q, 256)), dim3(256), 0, st, p.pa, p.pb, q,
                     splits, rowmin, rowmax);
  USC_CHECK_LAUNCH("usc_freemask_rowstats");
  return USC_OK;
}

int usc_freemask_bits(const float* fq, const float* sq, int64_t q, const float* fk, const float* sk,
                      const uint8_t* zero_k, int64_t k, int32_t c, const float* rowmin, const float* rowmax,
                      float threshold, uint64_t* bits, int32_t* count, float* soft_sum, void* ws, int64_t ws_bytes,
                      usc_stream_t s) {
  USC_FM_COMMON("usc_freemask_bits");
  USC_REQUIRE(zero_k && rowmin && rowmax && bits && count && soft_sum && ws, "usc_freemask_bits: null pointer");
  USC_REQUIRE(ws_bytes >= usc_freemask_ws_bytes(q, k), "usc_freemask_bits: workspace too small");
  FmArgs p = {};
  p.fq = fq; p.sq = sq; p.fk = fk; p.sk = sk; p.zk = zero_k; p.rmin = rowmin; p.rmax = rowmax;
  p.Q = q; p.K = k; p.C = c; p.thr = threshold;
  p.w32 = 2 * ceil_div(k, 64);
  p.tiles = (int32_t)p.w32;
  int32_t splits;
  fm_splits(q, p.tiles, &p.chunk, &splits);
  p.pb = (float*)ws;
  p.pcount = (int32_t*)ws + (int64_t)splits * q;
  p.bits = (uint32_t*)bits;
  hipStream_t st = as_stream(s);
  if (int rc = fm_launch<kFmBits>(p, q, splits, st, "usc_freemask_bits")) return rc;
  hipLaunchKernelGGL(freemask_bits_finish_kernel, dim3((unsigned)ceil_div(q, 256)), dim3(256), 0, st, p.pb, p.pcount, q,
                     splits, soft_sum, count);
  USC_CHECK_LAUNCH("usc_freemask_bits");
  return USC_OK;
}

int usc_freemask_soft_rows(const float* fq, const float* sq, int64_t q, const float* fk, const float* sk,
                           const uint8_t* zero_k, int64_t k, int32_t c, const float* rowmin, const float* rowmax,
                           const int32_t* qidx, int32_t m, float* out, usc_stream_t s) {
  USC_FM_COMMON("usc_freemask_soft_rows");
  USC_REQUIRE(m >= 0 && m <= 4096, "usc_freemask_soft_rows: m out of range [0, 4096]");
  if (m == 0) return USC_OK;
  USC_REQUIRE(zero_k && rowmin && rowmax && qidx && out, "usc_freemask_soft_rows: null pointer");
  FmArgs p = {};
  p.fq = fq; p.sq = sq; p.fk = fk; p.sk = sk; p.zk = zero_k; p.rmin = rowmin; p.rmax = rowmax; p.qidx = qidx;
  p.Q = m; p.K = k; p.C = c;
  p.tiles = (int32_t)(2 * ceil_div(k, 64));
  int32_t splits;
  fm_splits(m, p.tiles, &p.chunk, &splits);
  p.soft = out;
  return fm_launch<kFmSoft>(p, m, splits, as_stream(s), "usc_freemask_soft_rows");
}

int usc_mask_bits_extent(const uint64_t* bits, int64_t n, int64_t k, const int32_t* coords, int32_t* lo, int32_t* hi,
                         usc_stream_t s) {
  USC_REQUIRE(n >= 0 && n <= INT32_MAX, "usc_mask_bits_extent: n out of range");
  USC_REQUIRE(k >= 1 && k <= INT32_MAX - 64, "usc_mask_bits_extent: k out of range");
  if (n == 0) return USC_OK;
  USC_REQUIRE(bits && coords && lo && hi, "usc_mask_bits_extent: null pointer");
  hipLaunchKernelGGL(mask_bits_extent_kernel, dim3((unsigned)n), dim3(256), 0, as_stream(s), bits, ceil_div(k, 64), k,
                     coords, lo, hi);
  USC_CHECK_LAUNCH("usc_mask_bits_extent");
  return USC_OK;
}

int64_t usc_mask_bits_nms_ws_bytes(int64_t n) { return n < 1 ? 0 : n * ceil_div(n, 64) * 8; }

static int mask_bits_nms_run(const char* name, const uint64_t* bits, const int32_t* count, const int32_t* weight,
                             int64_t k, const int32_t* order, int32_t n, float nms_thr, uint8_t* keep, void* ws,
                             int64_t ws_bytes, usc_stream_t s) {
  USC_REQUIRE(n >= 0 && n <= 524288, "%s: n out of range [0, 524288]", name);
  USC_REQUIRE(k >= 1 && k <= INT32_MAX - 64, "%s: k out of range", name);
  if (n == 0) return USC_OK;
  USC_REQUIRE(bits && count && order && keep && ws, "%s: null pointer", name);
  USC_REQUIRE(ws_bytes >= usc_mask_bits_nms_ws_bytes(n), "%s: workspace too small", name);
  const int32_t nW = (int32_t)ceil_div(n, 64);      // <= 8192: dead[] fits 64 KB of LDS
  hipStream_t st = as_stream(s);
  if (weight)
    hipLaunchKernelGGL(mask_bits_nms_fill_kernel<true>, dim3(nW, nW), dim3(256), 0, st, bits, ceil_div(k, 64), count,
                       order, n, nms_thr, (uint64_t*)ws, nW, weight, k);
  else
    hipLaunchKernelGGL(mask_bits_nms_fill_kernel<false>, dim3(nW, nW), dim3(256), 0, st, bits, ceil_div(k, 64), count,
                       order, n, nms_thr, (uint64_t*)ws, nW, weight, k);
  USC_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(mask_bits_nms_scan_kernel, dim3(1), dim3(1024), (size_t)nW * 8, st, (const uint64_t*)ws, n, nW,
                     keep);
  USC_CHECK_LAUNCH(name);
  return USC_OK;
}

int usc_mask_bits_nms(const uint64_t* bits, const int32_t* count, int64_t k, const int32_t* order, int32_t n,
                      float nms_thr, uint8_t* keep, void* ws, int64_t ws_bytes, usc_stream_t s) {
  return mask_bits_nms_run("usc_mask_bits_nms", bits, count, nullptr, k, order, n, nms_thr, keep, ws, ws_bytes, s);
}

int usc_mask_bits_nms_weighted(const uint64_t* bits, const int32_t* count, const int32_t* weight, int64_t k,
                               const int32_t* order, int32_t n, float nms_thr, uint8_t* keep, void* ws,
                               int64_t ws_bytes, usc_stream_t s) {
  USC_REQUIRE(weight || n == 0, "usc_mask_bits_nms_weighted: null pointer");
  return mask_bits_nms_run("usc_mask_bits_nms_weighted", bits, count, weight, k, order, n, nms_thr, keep, ws, ws_bytes,
                           s);
}

}  // extern "C"
