// spconv_bf16.hip — the bf16 matrix-core convolutions (unscene3d_amd/precision.py): one gather-GEMM over P operand planes.
//
//   out[o, :] (=|+=) sum_k sum_{i + j < P} x_i[nbr[k][o], :] @ W_j[k] (+ bias)           f32 accumulate, f32 output
//
// P = 1, inference precision "bf16": x_0 = bf16(x), W_0 = bf16(W) (round to nearest even; usc_cast_bf16,
// usc_spconv_pack_w_bf16).  Every product of two bf16 values is exact in f32, so the result differs from a float64 conv
// of the ROUNDED operands only by the f32 accumulation.
// P = 2, 3, training precisions "bf16x2" / "bf16x3" (forward and input gradient of the stride-1 convolutions): an f32
// value is split into P planes, x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1) (subtractions in f32): three
// planes reproduce x exactly.  The kept plane products are 6 for P = 3 (dropped terms <= 2^-23 |x||w|, below f32's own
// rounding) and 3 for P = 2 (<= 3 * 2^-16 |x||w|).
//
// The f32 kernels (spconv.hip, spconv_sorted.hip) run on v_mfma_f32_32x32x2_f32, 1/16 of the rate of the
// v_mfma_f32_32x32x16_bf16 used here.  Nothing is converted or subtracted inside the MFMA loop: the activation planes
// come from memory, interleaved per row (bf16[rows][P][c], usc_split_bf16_rows: the planes of one gathered row are
// contiguous), the weight planes packed once into the B-fragment order, one plane after the other
// (usc_spconv_pack_w_split).
//
// Layout of one workgroup (256 threads = 4 waves): 4 x kRowTiles x 32 output rows by 32 * CT output columns
// (grid.y walks the column groups).  Per kernel offset k the block stages the packed weights of up to kChunk 16-channel
// steps in LDS (shared by the 4 waves), and each wave gathers its rows' bf16 activations straight into A fragments
// (16 bytes per lane, step and plane: lane l holds A[row l&31][k = 8 (l>>5) + j], j = 0..7).  Offsets none of the
// block's rows has are skipped by the whole block, offsets none of a wave's rows has by that wave.  Each output element
// is summed by one lane over k ascending, channel step ascending; with P >= 2 the products of a step smallest first
// (pair_x / pair_w read backwards) into a partial sum that starts at zero: no atomics, no split-K, two launches give
// the same bits.
//
// Reference: MinkowskiEngine 0.5.4 MinkowskiConvolution / MinkowskiConvolutionTranspose forward and backward (input
// gradient) (src/convolution_kernel.cu; models/modules/common.py:125-188, models/res16unet.py:224-297) — under the
// opt-in precisions only.
#include "common.h"

namespace usc {
namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int kRowTiles = 2;            // 32-row tiles per wave
constexpr int kBlockRows = 4 * 32 * kRowTiles;

// 16-channel steps of weights staged in LDS at a time (the A fragments of a chunk are chunk * kRowTiles * P * 4 registers
// beside 32 * CT accumulators), and the kept products (activation plane i, weight plane j), i + j < P, largest first:
// P = 1: x0w0;  P = 2: x0w0 x0w1 x1w0;  P = 3: x0w0 x0w1 x1w0 x0w2 x1w1 x2w0
template <int P> struct Planes { static constexpr int chunk = P == 3 ? 2 : 4, pairs = P * (P + 1) / 2; };
__host__ __device__ constexpr int pair_x(int q) { return q == 2 || q == 4 ? 1 : q == 5 ? 2 : 0; }
__host__ __device__ constexpr int pair_w(int q) { return q == 1 || q == 4 ? 1 : q == 3 ? 2 : 0; }

// 32-column tiles per workgroup column group: the widest of 3, 2, 1 that divides cout / 32 (four tiles, 128 accumulator
// registers, leave one wave per SIMD)
inline int col_tiles(int cout) {
  const int T = cout / 32;
  return T % 3 == 0 ? 3 : T % 2 == 0 ? 2 : 1;
}

// round to nearest even; NaN stays a (quiet) NaN
__device__ inline uint16_t f32_to_bf16_rne(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ inline float bf16_to_f32(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

// x -> its P planes.  A value whose first plane is not finite (inf, NaN, or a finite value that rounds to inf) keeps
// that plane and gets zero in the others: inf stays inf and does not turn into NaN (inf - inf).
template <int P>
__device__ inline void split_value(float x, uint16_t (&pl)[P]) {
  pl[0] = f32_to_bf16_rne(x);
  if constexpr (P > 1) {
#pragma unroll
    for (int p = 1; p < P; ++p) pl[p] = 0;
    if ((pl[0] & 0x7f80u) == 0x7f80u) return;
    float r = x - bf16_to_f32(pl[0]);
    pl[1] = f32_to_bf16_rne(r);
    if constexpr (P > 2) {
      r = r - bf16_to_f32(pl[1]);
      pl[2] = f32_to_bf16_rne(r);
    }
  }
}

// in f32[rows][c] -> out bf16[rows][P][c]; the body walks groups of four consecutive elements.  VEC: a group stays inside
// one row (c % 4 == 0, or P = 1, where the output is as flat as the input) and each plane takes one 8-byte store.
template <int P, bool VEC>
__global__ __launch_bounds__(256) void split_kernel(const float4* __restrict__ in, int64_t n4, int64_t c,
                                                    uint16_t* __restrict__ out) {
  for (int64_t e4 = (int64_t)blockIdx.x * 256 + threadIdx.x; e4 < n4; e4 += (int64_t)gridDim.x * 256) {
    const float4 v = in[e4];
    const float x[4] = {v.x, v.y, v.z, v.w};
    uint16_t pl[4][P];
#pragma unroll
    for (int i = 0; i < 4; ++i) split_value<P>(x[i], pl[i]);
    const int64_t e = e4 << 2;
    if (VEC) {
      const int64_t row = P == 1 ? 0 : e / c, ch = e - row * c;
#pragma unroll
      for (int p = 0; p < P; ++p)
        *reinterpret_cast<uint2*>(out + (row * P + p) * c + ch) =
            make_uint2((uint32_t)pl[0][p] | ((uint32_t)pl[1][p] << 16), (uint32_t)pl[2][p] | ((uint32_t)pl[3][p] << 16));
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = (e + i) / c, ch = (e + i) - row * c;
#pragma unroll
        for (int p = 0; p < P; ++p) out[(row * P + p) * c + ch] = pl[i][p];
      }
    }
  }
}
template <int P>
__global__ void split_tail_kernel(const float* __restrict__ in, int64_t from, int64_t n, int64_t c, uint16_t* __restrict__ out) {
  const int64_t e = from + threadIdx.x;
  if (e >= n) return;
  uint16_t pl[P];
  split_value<P>(in[e], pl);
  const int64_t row = P == 1 ? 0 : e / c, ch = e - row * c;
#pragma unroll
  for (int p = 0; p < P; ++p) out[(row * P + p) * c + ch] = pl[p];
}

// Wp[p][k][s][t][lane][j] = plane p of Wsrc(k)[16 s + 8 (lane >> 5) + j][32 t + (lane & 31)]   (one 16-byte B fragment
// per lane; S = cin_op / 16 steps, T = cout_op / 32 tiles of the OPERAND shape).  Plain: Wsrc(k) = W[k], operand shape
// cin -> cout.  Transposed: Wsrc(k)[n][c] = W[mirror ? K - 1 - k : k][c][n], operand shape cout -> cin (W is
// [K][cin][cout] either way).
template <int P>
__global__ __launch_bounds__(256) void pack_w_split_kernel(const float* __restrict__ W, int K, int cin, int cout,
                                                           int transposed, uint16_t* __restrict__ Wp) {
  const int ci = transposed ? cout : cin, co = transposed ? cin : cout;       // operand widths
  const int S = ci / 16, T = co / 32;
  const int64_t total = (int64_t)K * S * T * 64;
  const int64_t plane = total * 8;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int lane = (int)(e & 63);
    int64_t q = e >> 6;
    const int t = (int)(q % T); q /= T;
    const int s = (int)(q % S);
    const int k = (int)(q / S);
    const int row = 16 * s + 8 * (lane >> 5), col = 32 * t + (lane & 31);     // of the operand matrix, rows row .. row + 7
    const float* src;
    int64_t step;
    if (transposed) {
      const int ks = K > 1 ? K - 1 - k : k;
      src = W + ((int64_t)ks * cin + col) * cout + row;
      step = 1;
    } else {
      src = W + ((int64_t)k * cin + row) * cout + col;
      step = cout;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      uint16_t pl[P];
      split_value<P>(src[j * step], pl);
#pragma unroll
      for (int p = 0; p < P; ++p) Wp[p * plane + e * 8 + j] = pl[p];
    }
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

template <int P, int CT>
__global__ __launch_bounds__(256) void gather_gemm_planes_kernel(const uint16_t* __restrict__ in, int cin,
                                                                 const uint16_t* __restrict__ Wp, int K, int cout,
                                                                 const int32_t* __restrict__ nbr, int64_t n_out,
                                                                 const float* __restrict__ bias, float* __restrict__ out,
                                                                 int accumulate) {
  constexpr int kChunk = Planes<P>::chunk;
  __shared__ bf16x8 sB[P * kChunk * CT * 64];              // [plane][step][column tile][lane]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int S = cin >> 4, T = cout >> 5;
  const int t0 = blockIdx.y * CT;
  const int64_t row0 = (int64_t)blockIdx.x * kBlockRows + wave * 32 * kRowTiles;
  const int64_t wplane = (int64_t)K * S * T * 64;          // B fragments per weight plane
  const int64_t xrow = (int64_t)P * cin;                   // bf16 values per activation row (P planes)

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
      bf16x8 afr[kChunk][kRowTiles][P];
#pragma unroll
      for (int s = 0; s < kChunk; ++s)
#pragma unroll
        for (int a = 0; a < kRowTiles; ++a)
#pragma unroll
          for (int p = 0; p < P; ++p) {
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (wave_has && s < ns && src[a] >= 0)
              v = *reinterpret_cast<const bf16x8*>(in + src[a] * xrow + p * cin + 16 * (s0 + s) + 8 * h);
            afr[s][a][p] = v;
          }
      __syncthreads();                                           // the previous chunk's readers are done with sB
      const bf16x8* gB = reinterpret_cast<const bf16x8*>(Wp);
      if constexpr (P == 1) {                                    // one plane: the staged steps are contiguous in sB
        for (int e = tid; e < ns * CT * 64; e += 256) {
          const int s = e / (CT * 64), rem = e - s * CT * 64;
          const int c = rem >> 6, l = rem & 63;
          sB[e] = gB[(((int64_t)k * S + s0 + s) * T + t0 + c) * 64 + l];
        }
      } else {
        for (int e = tid; e < P * ns * CT * 64; e += 256) {
          const int p = e / (ns * CT * 64), rp = e - p * ns * CT * 64;
          const int s = rp / (CT * 64), rem = rp - s * CT * 64;
          const int c = rem >> 6, l = rem & 63;
          sB[((p * kChunk + s) * CT + c) * 64 + l] = gB[p * wplane + (((int64_t)k * S + s0 + s) * T + t0 + c) * 64 + l];
        }
      }
      __syncthreads();
      if (!wave_has) continue;
#pragma unroll
      for (int s = 0; s < kChunk; ++s) {
        if (s < ns) {
#pragma unroll
          for (int c = 0; c < CT; ++c) {
            bf16x8 b[P];
#pragma unroll
            for (int p = 0; p < P; ++p) b[p] = sB[((p * kChunk + s) * CT + c) * 64 + lane];
#pragma unroll
            for (int a = 0; a < kRowTiles; ++a) {
              if constexpr (P == 1) {
                acc[a][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr[s][a][0], b[0], acc[a][c], 0, 0, 0);
              } else {
                // the kept products of this step are summed from zero, smallest first, and that partial sum is added to
                // the accumulator by the vector unit (round to nearest): a long accumulation chain through this MFMA's C
                // operand does not round to nearest (measured: 1 + 0.75 ulp gives 1), which biased sums over many rows.
                // (One plane keeps that chain: its operands are rounded to bf16 to begin with.)
                f32x16 part;
#pragma unroll
                for (int i = 0; i < 16; ++i) part[i] = 0.f;
#pragma unroll
                for (int q = Planes<P>::pairs - 1; q >= 0; --q)
                  part = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr[s][a][pair_x(q)], b[pair_w(q)], part, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[a][c][i] += part[i];
              }
            }
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

template <int P>
void launch_split(const float* in, int64_t n, int64_t c, uint16_t* out, hipStream_t st) {
  const int64_t n4 = n >> 2;
  if (n4 > 0) {
    if (P == 1 || c % 4 == 0)
      hipLaunchKernelGGL((split_kernel<P, true>), dim3(stream_grid(n4, 256)), dim3(256), 0, st, (const float4*)in, n4, c, out);
    else if constexpr (P > 1)
      hipLaunchKernelGGL((split_kernel<P, false>), dim3(stream_grid(n4, 256)), dim3(256), 0, st, (const float4*)in, n4, c, out);
  }
  if (n & 3) hipLaunchKernelGGL(split_tail_kernel<P>, dim3(1), dim3(4), 0, st, in, n4 << 2, n, c, out);
}

template <int P>
void launch_pack_w(const float* W, int K, int cin, int cout, int transposed, uint16_t* Wp, hipStream_t st) {
  const int ci = transposed ? cout : cin, co = transposed ? cin : cout;
  const int64_t total = (int64_t)K * (ci / 16) * (co / 32) * 64;
  hipLaunchKernelGGL(pack_w_split_kernel<P>, dim3(stream_grid(total, 256)), dim3(256), 0, st, W, K, cin, cout, transposed, Wp);
}

template <int P>
void launch_gemm(int CT, dim3 grid, hipStream_t st, const uint16_t* in, int cin, const uint16_t* Wp, int K, int cout,
                 const int32_t* nbr, int64_t n_out, const float* bias, float* out, int accumulate) {
#define USC_PLANES_LAUNCH(CTv)                                                                                        \
  hipLaunchKernelGGL((gather_gemm_planes_kernel<P, CTv>), grid, dim3(256), 0, st, in, cin, Wp, K, cout, nbr, n_out, \
                     bias, out, accumulate)
  switch (CT) {
    case 3: USC_PLANES_LAUNCH(3); break;
    case 2: USC_PLANES_LAUNCH(2); break;
    default: USC_PLANES_LAUNCH(1); break;
  }
#undef USC_PLANES_LAUNCH
}

// what usc_spconv_gather_gemm_bf16 (P = 1) and usc_spconv_gather_gemm_split (P = 2, 3) check once the shape is known to
// be covered, and the launch
int gemm_planes(const char* who, int P, const uint16_t* in, int64_t n_in, int cin, const uint16_t* Wp, int K, int cout,
                const int32_t* nbr, int64_t n_out, const float* bias, float* out, int accumulate, hipStream_t st) {
  USC_REQUIRE(nbr || K == 1, "%s: K>1 needs a neighbour table", who);
  USC_REQUIRE(nbr || n_in == n_out, "%s: identity map needs n_in == n_out", who);
  if (n_out == 0) return USC_OK;
  USC_REQUIRE(in && Wp && out, "%s: null pointer", who);
  USC_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)Wp & 15) == 0, "%s: operands must be 16-byte aligned", who);
  const int CT = col_tiles(cout);
  dim3 grid((unsigned)ceil_div(n_out, kBlockRows), (unsigned)(cout / 32 / CT));
  if (P == 1) launch_gemm<1>(CT, grid, st, in, cin, Wp, K, cout, nbr, n_out, bias, out, accumulate);
  else if (P == 2) launch_gemm<2>(CT, grid, st, in, cin, Wp, K, cout, nbr, n_out, bias, out, accumulate);
  else launch_gemm<3>(CT, grid, st, in, cin, Wp, K, cout, nbr, n_out, bias, out, accumulate);
  USC_CHECK_LAUNCH(who);
  return USC_OK;
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
  launch_split<1>(in, n, n, out, as_stream(s));
  USC_CHECK_LAUNCH("usc_cast_bf16");
  return USC_OK;
}

int usc_split_bf16_rows(const float* in, int64_t rows, int32_t c, int32_t P, uint16_t* out, usc_stream_t s) {
  USC_REQUIRE(rows >= 0 && c >= 1, "usc_split_bf16_rows: bad size");
  USC_REQUIRE(P == 2 || P == 3, "usc_split_bf16_rows: P must be 2 or 3 (got %d)", P);
  const int64_t n = rows * c;
  if (n == 0) return USC_OK;
  USC_REQUIRE(in && out, "usc_split_bf16_rows: null pointer");
  USC_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 7) == 0, "usc_split_bf16_rows: misaligned pointer");
  if (P == 2) launch_split<2>(in, n, c, out, as_stream(s));
  else launch_split<3>(in, n, c, out, as_stream(s));
  USC_CHECK_LAUNCH("usc_split_bf16_rows");
  return USC_OK;
}

int usc_split_bf16(const float* in, int64_t n, int32_t P, uint16_t* out, usc_stream_t s) {
  USC_REQUIRE(n >= 0 && n <= 0x7fffffff, "usc_split_bf16: bad size");
  if (n == 0) {
    USC_REQUIRE(P == 2 || P == 3, "usc_split_bf16: P must be 2 or 3 (got %d)", P);
    return USC_OK;
  }
  return usc_split_bf16_rows(in, 1, (int32_t)n, P, out, s);
}

int usc_spconv_pack_w_bf16(const float* W, int32_t K, int32_t cin, int32_t cout, uint16_t* Wp, usc_stream_t s) {
  USC_REQUIRE(K >= 1 && cin >= 16 && cin % 16 == 0 && cout >= 32 && cout % 32 == 0,
              "usc_spconv_pack_w_bf16: needs K >= 1, cin a multiple of 16, cout a multiple of 32 (got K=%d %d -> %d)", K,
              cin, cout);
  USC_REQUIRE(W && Wp, "usc_spconv_pack_w_bf16: null pointer");
  launch_pack_w<1>(W, (int)K, (int)cin, (int)cout, 0, Wp, as_stream(s));
  USC_CHECK_LAUNCH("usc_spconv_pack_w_bf16");
  return USC_OK;
}

int usc_spconv_pack_w_split(const float* W, int32_t K, int32_t cin, int32_t cout, int32_t P, int32_t transposed,
                            uint16_t* Wp, usc_stream_t s) {
  USC_REQUIRE(P == 2 || P == 3, "usc_spconv_pack_w_split: P must be 2 or 3 (got %d)", P);
  const int ci = transposed ? cout : cin, co = transposed ? cin : cout;
  USC_REQUIRE(K >= 1 && ci >= 16 && ci % 16 == 0 && co >= 32 && co % 32 == 0,
              "usc_spconv_pack_w_split: needs K >= 1 and an operand shape with the input width a multiple of 16 and the "
              "output width a multiple of 32 (got K=%d, operand %d -> %d)", K, ci, co);
  USC_REQUIRE(W && Wp, "usc_spconv_pack_w_split: null pointer");
  if (P == 2) launch_pack_w<2>(W, (int)K, (int)cin, (int)cout, (int)(transposed != 0), Wp, as_stream(s));
  else launch_pack_w<3>(W, (int)K, (int)cin, (int)cout, (int)(transposed != 0), Wp, as_stream(s));
  USC_CHECK_LAUNCH("usc_spconv_pack_w_split");
  return USC_OK;
}

int64_t usc_spconv_gather_gemm_bf16_ws_bytes(int64_t n_out, int32_t cin, int32_t cout, int32_t K) {
  if (n_out < 0 || K < 1 || K > 64 || cin < 16 || cin % 16 || cin > 4096 || cout < 32 || cout % 32 || cout > 4096) return -1;
  return 0;
}

int64_t usc_spconv_gather_gemm_split_ws_bytes(int64_t n_out, int32_t cin, int32_t cout, int32_t K, int32_t P) {
  if (P != 2 && P != 3) return -1;
  return usc_spconv_gather_gemm_bf16_ws_bytes(n_out, cin, cout, K);
}

int usc_spconv_gather_gemm_bf16(const uint16_t* in, int64_t n_in, int32_t cin, const uint16_t* Wp, int32_t K,
                                int32_t cout, const int32_t* nbr, int64_t n_out, const float* bias, float* out,
                                int32_t accumulate, void* ws, int64_t ws_bytes, usc_stream_t s) {
  (void)ws;
  (void)ws_bytes;
  USC_REQUIRE(usc_spconv_gather_gemm_bf16_ws_bytes(n_out, cin, cout, K) >= 0 && n_in >= 0,
              "usc_spconv_gather_gemm_bf16: shape not covered (K=%d, %d -> %d channels; needs cin %% 16 == 0, cout %% 32 == 0)",
              K, cin, cout);
  return gemm_planes("usc_spconv_gather_gemm_bf16", 1, in, n_in, (int)cin, Wp, (int)K, (int)cout, nbr, n_out, bias, out,
                     (int)accumulate, as_stream(s));
}

int usc_spconv_gather_gemm_split(const uint16_t* in, int64_t n_in, int32_t cin, const uint16_t* Wp, int32_t K,
                                 int32_t cout, int32_t P, const int32_t* nbr, int64_t n_out, const float* bias,
                                 float* out, int32_t accumulate, void* ws, int64_t ws_bytes, usc_stream_t s) {
  (void)ws;
  (void)ws_bytes;
  USC_REQUIRE(usc_spconv_gather_gemm_split_ws_bytes(n_out, cin, cout, K, P) >= 0 && n_in >= 0,
              "usc_spconv_gather_gemm_split: shape not covered (P=%d, K=%d, %d -> %d channels; needs P 2 or 3, cin %% 16 == 0, "
              "cout %% 32 == 0, K <= 64)", P, K, cin, cout);
  return gemm_planes("usc_spconv_gather_gemm_split", P, in, n_in, (int)cin, Wp, (int)K, (int)cout, nbr, n_out, bias, out,
                     (int)accumulate, as_stream(s));
}

}  // extern "C"
