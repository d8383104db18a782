// spconv_bf16.hip — bf16 matrix-core forward convolution (inference precision "bf16", unscene3d_amd/precision.py).
//
//   out[o, :] (=|+=) sum_k bf16(in[nbr[k][o], :]) @ bf16(W[k]) (+ bias)       f32 accumulate, f32 output
//
// The f32 kernels (spconv.hip, spconv_sorted.hip) run on v_mfma_f32_32x32x2_f32, 1/16 of the bf16 matrix-core rate.
// Here the operands are bf16 (v_mfma_f32_32x32x16_bf16): the activations as one bf16 copy per conv input
// (usc_cast_bf16, round to nearest even) and the weights packed once into the B-fragment order
// (usc_spconv_pack_w_bf16).  Every product of two bf16 values is exact in f32, so the result differs from a float64
// conv of the ROUNDED operands only by the f32 accumulation.
//
// Layout of one workgroup (256 threads = 4 waves): 4 x kRowTiles x 32 output rows by 32 * CT output columns
// (grid.y walks the column groups).  Per kernel offset k the block stages the packed weights of up to kChunk 16-channel
// steps in LDS (shared by the 4 waves), and each wave gathers its rows' bf16 activations straight into A fragments
// (16 bytes per lane and step: lane l holds A[row l&31][k = 8 (l>>5) + j], j = 0..7).  Offsets none of the block's rows
// has are skipped by the whole block, offsets none of a wave's rows has by that wave.  Each output element is summed
// by one lane over k ascending, channel ascending: no atomics, no split-K, two launches give the same bits.
//
// Reference: MinkowskiEngine 0.5.4 MinkowskiConvolution / MinkowskiConvolutionTranspose forward
// (src/convolution_kernel.cu, models/res16unet.py:224-297) — under the opt-in inference precision only.
#include "common.h"
#include "bf16_frag.h"

namespace usc {
namespace {

constexpr int kChunk = 4;               // 16-channel steps of weights staged in LDS at a time

__global__ __launch_bounds__(256) void cast_bf16_kernel(const float4* __restrict__ in, uint2* __restrict__ out, int64_t n4) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n4; e += (int64_t)gridDim.x * 256) {
    const float4 v = in[e];
    out[e] = make_uint2((uint32_t)f32_to_bf16_rne(v.x) | ((uint32_t)f32_to_bf16_rne(v.y) << 16),
                        (uint32_t)f32_to_bf16_rne(v.z) | ((uint32_t)f32_to_bf16_rne(v.w) << 16));
  }
}
__global__ void cast_bf16_tail_kernel(const float* __restrict__ in, uint16_t* __restrict__ out, int64_t from, int64_t n) {
  const int64_t e = from + threadIdx.x;
  if (e < n) out[e] = f32_to_bf16_rne(in[e]);
}

// Wp[k][s][t][lane][j] = bf16(W[k][16 s + 8 (lane >> 5) + j][32 t + (lane & 31)])   (one 16-byte B fragment per lane)
__global__ __launch_bounds__(256) void pack_w_kernel(const float* __restrict__ W, int K, int cin, int cout,
                                                     uint16_t* __restrict__ Wp) {
  const int S = cin / 16, T = cout / 32;
  const int64_t total = (int64_t)K * S * T * 64;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int lane = (int)(e & 63);
    int64_t q = e >> 6;
    const int t = (int)(q % T); q /= T;
    const int s = (int)(q % S);
    const int k = (int)(q / S);
    const float* src = W + ((int64_t)k * cin + 16 * s + 8 * (lane >> 5)) * cout + 32 * t + (lane & 31);
    uint16_t* dst = Wp + e * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[j] = f32_to_bf16_rne(src[(int64_t)j * cout]);
  }
}

// inv[k][f] = c where nbr2[k][c] = f (the child table of a stride-2 map read backwards), else -1: the gather table of
// the transposed conv, whose output rows are the fine rows
__global__ __launch_bounds__(256) void fill_i32_kernel(int32_t* __restrict__ p, int64_t n, int32_t v) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) p[e] = v;
}
__global__ __launch_bounds__(256) void invert_table_kernel(const int32_t* __restrict__ nbr2, int K, int64_t n_coarse,
                                                           int64_t n_fine, int32_t* __restrict__ inv) {
  const int64_t total = (int64_t)K * n_coarse;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int32_t f = nbr2[e];
    if (f >= 0 && f < n_fine) {
      const int64_t k = e / n_coarse;
      inv[k * n_fine + f] = (int32_t)(e - k * n_coarse);
    }
  }
}

template <int CT>
__global__ __launch_bounds__(256) void gather_gemm_bf16_kernel(const uint16_t* __restrict__ in, int cin,
                                                               const uint16_t* __restrict__ Wp, int K, int cout,
                                                               const int32_t* __restrict__ nbr, int64_t n_out,
                                                               const float* __restrict__ bias, float* __restrict__ out,
                                                               int accumulate) {
  __shared__ bf16x8 sB[kChunk * CT * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int S = cin >> 4, T = cout >> 5;
  const int t0 = blockIdx.y * CT;
  const int64_t row0 = (int64_t)blockIdx.x * kBlockRows + wave * 32 * kRowTiles;

  f32x16 acc[kRowTiles][CT];
#pragma unroll
  for (int a = 0; a < kRowTiles; ++a)
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][c][i] = 0.f;

  for (int k = 0; k < K; ++k) {
    int64_t src[kRowTiles];
    bool mine = false;
#pragma unroll
    for (int a = 0; a < kRowTiles; ++a) {
      const int64_t row = row0 + a * 32 + r;
      int64_t i = -1;
      if (row < n_out) i = nbr ? (int64_t)nbr[(int64_t)k * n_out + row] : row;
      src[a] = i;
      mine |= i >= 0;
    }
    const bool wave_has = __any(mine);
    if (!__syncthreads_or(wave_has ? 1 : 0)) continue;          // no row of the block has offset k
    for (int s0 = 0; s0 < S; s0 += kChunk) {
      const int ns = S - s0 < kChunk ? S - s0 : kChunk;
      // A fragments of the chunk first (their latency overlaps the weight staging)
      bf16x8 afr[kChunk][kRowTiles];
#pragma unroll
      for (int s = 0; s < kChunk; ++s)
#pragma unroll
        for (int a = 0; a < kRowTiles; ++a) {
          bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
          if (wave_has && s < ns && src[a] >= 0)
            v = *reinterpret_cast<const bf16x8*>(in + src[a] * cin + 16 * (s0 + s) + 8 * h);
          afr[s][a] = v;
        }
      __syncthreads();                                           // the previous chunk's readers are done with sB
      const bf16x8* gB = reinterpret_cast<const bf16x8*>(Wp);
      for (int e = tid; e < ns * CT * 64; e += 256) {
        const int s = e / (CT * 64), rem = e - s * CT * 64;
        const int c = rem >> 6, l = rem & 63;
        sB[e] = gB[(((int64_t)k * S + s0 + s) * T + t0 + c) * 64 + l];
      }
      __syncthreads();
      if (!wave_has) continue;
#pragma unroll
      for (int s = 0; s < kChunk; ++s) {
        if (s < ns) {
#pragma unroll
          for (int c = 0; c < CT; ++c) {
            const bf16x8 b = sB[(s * CT + c) * 64 + lane];
#pragma unroll
            for (int a = 0; a < kRowTiles; ++a)
              acc[a][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr[s][a], b, acc[a][c], 0, 0, 0);
          }
        }
      }
    }
  }
  // C/D map: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int a = 0; a < kRowTiles; ++a)
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int col = (t0 + c) * 32 + r;
      const float b = bias ? bias[col] : 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int64_t row = row0 + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (row < n_out) {
          float* o = out + row * cout + col;
          const float v = acc[a][c][i] + b;
          *o = accumulate ? *o + v : v;
        }
      }
    }
}

}  // namespace

int spconv_up_table(const int32_t* nbr2, int32_t K, int64_t n_coarse, int64_t n_fine, int32_t* inv, hipStream_t st) {
  const int64_t n = (int64_t)K * n_fine;
  if (n > 0) hipLaunchKernelGGL(fill_i32_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, st, inv, n, -1);
  if ((int64_t)K * n_coarse > 0)
    hipLaunchKernelGGL(invert_table_kernel, dim3(stream_grid((int64_t)K * n_coarse, 256)), dim3(256), 0, st, nbr2, K,
                       n_coarse, n_fine, inv);
  USC_CHECK_LAUNCH("usc bf16 transposed-conv table");
  return USC_OK;
}

}  // namespace usc

using namespace usc;

extern "C" {

int usc_cast_bf16(const float* in, int64_t n, uint16_t* out, usc_stream_t s) {
  USC_REQUIRE(n >= 0, "usc_cast_bf16: bad size");
  if (n == 0) return USC_OK;
  USC_REQUIRE(in && out, "usc_cast_bf16: null pointer");
  USC_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 7) == 0, "usc_cast_bf16: misaligned pointer");
  hipStream_t st = as_stream(s);
  const int64_t n4 = n >> 2;
  if (n4 > 0)
    hipLaunchKernelGGL(cast_bf16_kernel, dim3(stream_grid(n4, 256)), dim3(256), 0, st, (const float4*)in, (uint2*)out, n4);
  if (n & 3) hipLaunchKernelGGL(cast_bf16_tail_kernel, dim3(1), dim3(4), 0, st, in, out, n4 << 2, n);
  USC_CHECK_LAUNCH("usc_cast_bf16");
  return USC_OK;
}

int usc_spconv_pack_w_bf16(const float* W, int32_t K, int32_t cin, int32_t cout, uint16_t* Wp, usc_stream_t s) {
  USC_REQUIRE(K >= 1 && cin >= 16 && cin % 16 == 0 && cout >= 32 && cout % 32 == 0,
              "usc_spconv_pack_w_bf16: needs K >= 1, cin a multiple of 16, cout a multiple of 32 (got K=%d %d -> %d)", K,
              cin, cout);
  USC_REQUIRE(W && Wp, "usc_spconv_pack_w_bf16: null pointer");
  const int64_t total = (int64_t)K * (cin / 16) * (cout / 32) * 64;
  hipLaunchKernelGGL(pack_w_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, as_stream(s), W, (int)K, (int)cin,
                     (int)cout, Wp);
  USC_CHECK_LAUNCH("usc_spconv_pack_w_bf16");
  return USC_OK;
}

int64_t usc_spconv_gather_gemm_bf16_ws_bytes(int64_t n_out, int32_t cin, int32_t cout, int32_t K) {
  if (n_out < 0 || K < 1 || K > 64 || cin < 16 || cin % 16 || cin > 4096 || cout < 32 || cout % 32 || cout > 4096) return -1;
  return 0;
}

int usc_spconv_gather_gemm_bf16(const uint16_t* in, int64_t n_in, int32_t cin, const uint16_t* Wp, int32_t K,
                                int32_t cout, const int32_t* nbr, int64_t n_out, const float* bias, float* out,
                                int32_t accumulate, void* ws, int64_t ws_bytes, usc_stream_t s) {
  (void)ws;
  (void)ws_bytes;
  USC_REQUIRE(usc_spconv_gather_gemm_bf16_ws_bytes(n_out, cin, cout, K) >= 0 && n_in >= 0,
              "usc_spconv_gather_gemm_bf16: shape not covered (K=%d, %d -> %d channels; needs cin %% 16 == 0, cout %% 32 == 0)",
              K, cin, cout);
  USC_REQUIRE(nbr || K == 1, "usc_spconv_gather_gemm_bf16: K>1 needs a neighbour table");
  USC_REQUIRE(nbr || n_in == n_out, "usc_spconv_gather_gemm_bf16: identity map needs n_in == n_out");
  if (n_out == 0) return USC_OK;
  USC_REQUIRE(in && Wp && out, "usc_spconv_gather_gemm_bf16: null pointer");
  USC_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)Wp & 15) == 0, "usc_spconv_gather_gemm_bf16: operands must be 16-byte aligned");
  const int CT = col_tiles(cout);
  dim3 grid((unsigned)ceil_div(n_out, kBlockRows), (unsigned)(cout / 32 / CT));
  hipStream_t st = as_stream(s);
#define USC_BF16_LAUNCH(CTv)                                                                                          \
  hipLaunchKernelGGL(gather_gemm_bf16_kernel<CTv>, grid, dim3(256), 0, st, in, (int)cin, Wp, (int)K, (int)cout, nbr, \
                     n_out, bias, out, (int)accumulate)
  switch (CT) {
    case 3: USC_BF16_LAUNCH(3); break;
    case 2: USC_BF16_LAUNCH(2); break;
    default: USC_BF16_LAUNCH(1); break;
  }
#undef USC_BF16_LAUNCH
  USC_CHECK_LAUNCH("usc_spconv_gather_gemm_bf16");
  return USC_OK;
}

}  // extern "C"
