// vit_attention.hip — fused, unmasked, forward-only attention for the ViT image encoder (head dim 64, any token count).
//
// The DINO ViT-S/8 encoder of the pseudo-mask generator runs 2 962 tokens per 192x256 frame (patch 8 at stride 4).  In
// plain operators every block writes and re-reads a [6, 2962, 2962] f32 score tensor (210 MB); here the scores never
// leave the registers (flash style, online softmax).
//
//   qkv f32[B, T, 3, H, 64]   the rows nn.Linear(384, 1152) writes: no permute copy in front of the kernel
//   o   f32[B, T, H*64]       head-major columns, what attn.proj reads
//   o = softmax(scale * q k^T) v per (batch, head)
//
// One workgroup = 4 waves = 128 queries of one (batch, head); a wave owns 32 query rows and keeps their Q in registers.
// K and V are streamed through LDS in tiles of 64 keys (the next tile's global loads are in flight during the MFMAs of
// the current one).  Both products run with the QUERY on the MFMA lane:
//   S   = K   . Q^T   [key][query]     a lane holds 16 of the 32 keys of its own query: the row max and the row sum are
//                                      in-lane but for one exchange with lane ^ 32
//   O^T = V^T . P^T   [d][query]       sums over S's row index, so the S accumulator IS the B operand (no LDS round
//                                      trip), and the online-softmax rescale of O is one per-lane factor
// precision 0: f32 operands on v_mfma_f32_32x32x2_f32; precision 1: q, k, v and P rounded to bf16 (nearest even) on
// v_mfma_f32_32x32x16_bf16; accumulators and softmax statistics are f32 in both.  No atomics, every sum in a fixed
// order: two calls on the same input give the same bits.  Key rows >= T of the last tile are staged as zeros and their
// scores set to -inf (p = 0 exactly); query rows >= T are computed on a clamped row and never stored.
#include "common.h"

#include <math.h>

namespace usc {
namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

constexpr int kD = 64;                    // head dim
constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kQTile = 32 * kWaves;       // queries per workgroup
constexpr int kKTile = 64;                // keys per LDS tile

// LDS images.  f32: K [key][68] (rows padded by one 16-byte read: conflict-free ds_read_b128 down a column of keys),
// V [key][64].  bf16: K [key][72] (144-byte rows, same reason), V TRANSPOSED [d][68] (136-byte rows): the PV product
// wants, per lane, one d and four consecutive keys — one 8-byte read of the transposed image.
constexpr int kKRowF32 = 68, kVRowF32 = 64;
constexpr int kKRowBf16 = 144, kVRowBf16 = 136;            // bytes
constexpr int kVOffF32 = kKTile * kKRowF32 * 4;
constexpr int kVOffBf16 = kKTile * kKRowBf16;
constexpr int kLdsF32 = kVOffF32 + kKTile * kVRowF32 * 4;  // 33 792 B
constexpr int kLdsBf16 = kVOffBf16 + kD * kVRowBf16;       // 17 920 B

// two f32 -> packed bf16 pair, round to nearest even (v_cvt_pk_bf16_f32); a in the low half
__device__ inline uint32_t pack_bf16(float a, float b) {
  f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

// row of a 32x32 MFMA accumulator that register r of lane half h holds (the column is lane & 31)
__device__ inline constexpr int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

template <bool BF16>
__global__ __launch_bounds__(kThreads) void vit_attn_kernel(const float* __restrict__ qkv, int T, int H,
                                                            float scale_log2e, float* __restrict__ o) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[BF16 ? kLdsBf16 : kLdsF32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const int b = blockIdx.y / H, head = blockIdx.y - b * H;
  const int64_t row_stride = (int64_t)3 * H * kD;
  const float* qb = qkv + (int64_t)b * T * row_stride + head * kD;
  const float* kb = qb + (int64_t)H * kD;
  const float* vb = kb + (int64_t)H * kD;
  const int q_row = blockIdx.x * kQTile + wave * 32 + lr;

  // ---- Q fragment of this lane's query: d = 32 * lh + (0..31), the k order both QK^T operands use
  float qf[BF16 ? 1 : 32];
  bf16x8 qh[BF16 ? 4 : 1];
  {
    const float4* qp = (const float4*)(qb + (int64_t)min(q_row, T - 1) * row_stride + lh * 32);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float4 v = qp[i];
      if constexpr (BF16) {
        const uint32_t lo = pack_bf16(v.x, v.y), hi = pack_bf16(v.z, v.w);
        qh[i >> 1][(i & 1) * 4 + 0] = (short)(lo & 0xffffu);
        qh[i >> 1][(i & 1) * 4 + 1] = (short)(lo >> 16);
        qh[i >> 1][(i & 1) * 4 + 2] = (short)(hi & 0xffffu);
        qh[i >> 1][(i & 1) * 4 + 3] = (short)(hi >> 16);
      } else {
        qf[4 * i + 0] = v.x; qf[4 * i + 1] = v.y; qf[4 * i + 2] = v.z; qf[4 * i + 3] = v.w;
      }
    }
  }

  // ---- staging registers: 4 float4 of K and 4 of V per thread and tile
  float4 kreg[4], vreg[4];
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + kThreads * i;
      const int krow = kt * kKTile + (idx >> 4), c4 = idx & 15;
      float4 kv = *(const float4*)(kb + (int64_t)min(krow, T - 1) * row_stride + c4 * 4);
      if (krow >= T) kv = make_float4(0.f, 0.f, 0.f, 0.f);
      kreg[i] = kv;
      // f32: the same (row, column) piece of V.  bf16: rows 2p and 2p+1 of one column piece, written as key pairs
      int vrow, vc4;
      if constexpr (BF16) {
        const int item = tid + kThreads * (i >> 1);
        vrow = kt * kKTile + 2 * (item >> 4) + (i & 1);
        vc4 = item & 15;
      } else {
        vrow = krow;
        vc4 = c4;
      }
      float4 vv = *(const float4*)(vb + (int64_t)min(vrow, T - 1) * row_stride + vc4 * 4);
      if (vrow >= T) vv = make_float4(0.f, 0.f, 0.f, 0.f);
      vreg[i] = vv;
    }
  };
  auto write_tile = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + kThreads * i;
      const int row = idx >> 4, c4 = idx & 15;
      if constexpr (BF16) {
        *(uint2*)(lds + row * kKRowBf16 + c4 * 8) =
            make_uint2(pack_bf16(kreg[i].x, kreg[i].y), pack_bf16(kreg[i].z, kreg[i].w));
      } else {
        *(float4*)(lds + (row * kKRowF32 + c4 * 4) * 4) = kreg[i];
        *(float4*)(lds + kVOffF32 + (row * kVRowF32 + c4 * 4) * 4) = vreg[i];
      }
    }
    if constexpr (BF16) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int item = tid + kThreads * p;
        const int kp = item >> 4, dc = item & 15;
        unsigned char* dst = lds + kVOffBf16 + (dc * 4) * kVRowBf16 + kp * 4;
        const float4 a = vreg[2 * p], c = vreg[2 * p + 1];
        *(uint32_t*)(dst + 0 * kVRowBf16) = pack_bf16(a.x, c.x);
        *(uint32_t*)(dst + 1 * kVRowBf16) = pack_bf16(a.y, c.y);
        *(uint32_t*)(dst + 2 * kVRowBf16) = pack_bf16(a.z, c.z);
        *(uint32_t*)(dst + 3 * kVRowBf16) = pack_bf16(a.w, c.w);
      }
    }
  };

  f32x16 O[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) O[0][r] = O[1][r] = 0.f;
  float m = -INFINITY, l = 0.f;       // running max (log2 domain) and sum of this lane's query

  const int nt = (T + kKTile - 1) / kKTile;
  load_tile(0);
  for (int kt = 0; kt < nt; ++kt) {
    __syncthreads();                  // every wave has finished reading the previous tile
    write_tile();
    __syncthreads();
    if (kt + 1 < nt) load_tile(kt + 1);

    // ---- S = K . Q^T: two 32-key sub-tiles, columns = this wave's 32 queries
    f32x16 S[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) S[0][r] = S[1][r] = 0.f;
    if constexpr (BF16) {
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          const bf16x8 kf = *(const bf16x8*)(lds + (sub * 32 + lr) * kKRowBf16 + (lh * 32 + s * 8) * 2);
          S[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qh[s], S[sub], 0, 0, 0);
        }
    } else {
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4)
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          const float4 kv = *(const float4*)(lds + ((sub * 32 + lr) * kKRowF32 + lh * 32 + s4 * 4) * 4);
          S[sub] = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.x, qf[4 * s4 + 0], S[sub], 0, 0, 0);
          S[sub] = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.y, qf[4 * s4 + 1], S[sub], 0, 0, 0);
          S[sub] = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.z, qf[4 * s4 + 2], S[sub], 0, 0, 0);
          S[sub] = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.w, qf[4 * s4 + 3], S[sub], 0, 0, 0);
        }
    }

    // ---- online softmax of the lane's query over the tile's 64 keys (32 in this lane, 32 in lane ^ 32)
    const bool tail = kt * kKTile + kKTile > T;
    float mx = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float t = S[sub][r] * scale_log2e;
        if (tail && kt * kKTile + sub * 32 + acc_row(r, lh) >= T) t = -INFINITY;
        S[sub][r] = t;
        mx = fmaxf(mx, t);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m, mx);             // finite: every tile holds at least one key < T
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);
    m = m_new;
    float psum = 0.f;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(S[sub][r] - m_new);
        S[sub][r] = p;
        psum += p;
      }
    psum += __shfl_xor(psum, 32, 64);
    l = l * alpha + psum;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      O[0][r] *= alpha;
      O[1][r] *= alpha;
    }

    // ---- O^T += V^T . P^T: the S accumulators are the B operand as they stand
    if constexpr (BF16) {
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          // element j of lane half h is key 16 s2 + 8 (j >> 2) + 4 h + (j & 3) of the sub-tile: V is read in that order
          bf16x8 pf;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t w = pack_bf16(S[sub][8 * s2 + 2 * j], S[sub][8 * s2 + 2 * j + 1]);
            pf[2 * j] = (short)(w & 0xffffu);
            pf[2 * j + 1] = (short)(w >> 16);
          }
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            const unsigned char* vp = lds + kVOffBf16 + (db * 32 + lr) * kVRowBf16 + (sub * 32 + 16 * s2 + 4 * lh) * 2;
            const uint2 lo = *(const uint2*)vp, hi = *(const uint2*)(vp + 16);
            const uint4 w = make_uint4(lo.x, lo.y, hi.x, hi.y);
            O[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w), pf, O[db], 0, 0, 0);
          }
        }
    } else {
      const float* vl = (const float*)(lds + kVOffF32);
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = sub * 32 + acc_row(r, lh);
#pragma unroll
          for (int db = 0; db < 2; ++db)
            O[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(vl[key * kVRowF32 + db * 32 + lr], S[sub][r], O[db], 0, 0, 0);
        }
    }
  }

  // ---- o[b, q, head*64 + d] = O^T[d][q] / l; register 4g + i of block db is d = 32 db + 8 g + 4 lh + i
  if (q_row < T) {
    float* op = o + ((int64_t)b * T + q_row) * ((int64_t)H * kD) + head * kD;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *(float4*)(op + db * 32 + 8 * g + 4 * lh) = make_float4(O[db][4 * g + 0] / l, O[db][4 * g + 1] / l,
                                                                 O[db][4 * g + 2] / l, O[db][4 * g + 3] / l);
  }
}

}  // namespace
}  // namespace usc

using namespace usc;

extern "C" {

int32_t usc_vit_attn_head_dim(void) { return kD; }

int usc_vit_attn_fwd(const float* qkv, int32_t B, int32_t T, int32_t H, float scale, int32_t precision, float* o,
                     usc_stream_t s) {
  USC_REQUIRE(qkv && o, "usc_vit_attn_fwd: null pointer");
  USC_REQUIRE(B >= 1 && T >= 1 && H >= 1, "usc_vit_attn_fwd: B, T and H must be >= 1 (got %d, %d, %d)", B, T, H);
  USC_REQUIRE(T <= (1 << 30), "usc_vit_attn_fwd: T = %d exceeds 2^30", T);
  USC_REQUIRE((int64_t)B * H <= 65535, "usc_vit_attn_fwd: B * H = %lld exceeds 65535", (long long)B * H);
  USC_REQUIRE(precision == 0 || precision == 1, "usc_vit_attn_fwd: precision must be 0 (f32) or 1 (bf16), got %d",
              precision);
  USC_REQUIRE(isfinite(scale), "usc_vit_attn_fwd: scale is not finite");
  USC_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)o & 15) == 0, "usc_vit_attn_fwd: qkv and o must be 16-byte aligned");
  const dim3 grid((unsigned)ceil_div(T, kQTile), (unsigned)(B * H));
  const float scale_log2e = scale * 1.4426950408889634f;
  if (precision == 1)
    hipLaunchKernelGGL(vit_attn_kernel<true>, grid, dim3(kThreads), 0, as_stream(s), qkv, T, H, scale_log2e, o);
  else
    hipLaunchKernelGGL(vit_attn_kernel<false>, grid, dim3(kThreads), 0, as_stream(s), qkv, T, H, scale_log2e, o);
  USC_CHECK_LAUNCH("usc_vit_attn_fwd");
  return USC_OK;
}

}  // extern "C"
