// selftrain.hip — the self-training files as bit rows (trainer/postprocess.py::save_for_freemask(fmt="bits"),
// datasets/freemask.py::load_self_train_bits).
//
// A round's export is a bool[N, K] table (240 k points x 100 masks: 24 MB).  Here it lives as K rows of
// u64[ceil(N / 64)] in the layout of usc_freemask_bits (point r = bit r % 64 of word r / 64, bits at positions >= N
// are zero): 3 MB, and the reader's greedy merge is a few popcounts per column.
//
//   usc_mask_columns_to_bits      [n, k] bytes -> k bit rows + column counts (a transposing pack)
//   usc_mask_bits_gather          masks[ind] on bit rows (the 1-NN transfer to another cloud)
//   usc_selftrain_merge           the greedy "add an instance when more than half of it is new" loop, one workgroup
//   usc_mask_bits_to_columns(_u8) chosen bit rows -> 0/1 columns of a row-major table
//
// Explicit stream, no allocation, no synchronisation, no workgroup waits for another, no atomics: every output word
// has one writer and every count is a fixed tree of integer sums, so two runs give the same bytes.
#include "common.h"

namespace usc {
namespace {

constexpr int kStBlock = 256;                 // 4 waves; a wave owns one output word (64 consecutive points)
constexpr int kStWaves = kStBlock / kWave;
constexpr int kStChunk = 128;                 // columns of one LDS round of the pack
constexpr int kStLd = kStChunk + 4;           // bytes per staged row: 33 dwords, the column reads hit 64 banks
constexpr int kMergeBlock = 1024;
constexpr int kMergeWaves = kMergeBlock / kWave;
constexpr int kMergeLdsWordsDefault = 7168;   // 56 KB of foreground words: up to 458 752 points
int32_t g_merge_lds_words = kMergeLdsWordsDefault;

// lane c of a 64-column group keeps the ballot word of column c; the group is stored once it is complete
#define USC_ST_KEEP(word, c, mine) \
  if (((c) & 63) == lane) mine = (word)

// grid ceil(W / 4).  Wave -> rows [64 w, 64 w + 64): its 64 x ck byte tile goes through LDS (consecutive lanes read
// consecutive bytes of a row), then lane = row reads one column at a time and the wave votes.
__global__ __launch_bounds__(kStBlock) void mask_columns_to_bits_kernel(const uint8_t* __restrict__ masks, int64_t n,
                                                                        int32_t k, int64_t W,
                                                                        uint64_t* __restrict__ bits) {
  __shared__ uint8_t tile[kStWaves][kWave * kStLd];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * kStWaves + wave;
  const bool active = w < W;
  const int64_t r0 = w * 64;
  const int rows = active ? (int)(n - r0 < 64 ? n - r0 : 64) : 0;
  uint8_t* t = tile[wave];
  for (int32_t c0 = 0; c0 < k; c0 += kStChunk) {
    const int ck = k - c0 < kStChunk ? k - c0 : kStChunk;
    for (int e = lane; e < rows * ck; e += 64) {
      const int r = e / ck, c = e - r * ck;
      t[r * kStLd + c] = masks[(r0 + r) * k + c0 + c];
    }
    __syncthreads();
    uint64_t mine = 0;
    for (int c = 0; c < ck; ++c) {
      const uint64_t word = __ballot(lane < rows && t[lane * kStLd + c] != 0);
      USC_ST_KEEP(word, c, mine);
      if ((c & 63) == 63 || c == ck - 1) {
        const int32_t col = c0 + (c & ~63) + lane;
        if (active && lane <= (c & 63)) bits[(int64_t)col * W + w] = mine;
      }
    }
    __syncthreads();
  }
}

// grid ceil(Wn / 4).  Lane = output row: its source row is read once, then one vote per column.
__global__ __launch_bounds__(kStBlock) void mask_bits_gather_kernel(const uint64_t* __restrict__ src, int64_t Wm,
                                                                    const int64_t* __restrict__ ind, int64_t n,
                                                                    int32_t k, int64_t Wn,
                                                                    uint64_t* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * kStWaves + (threadIdx.x >> 6);
  if (w >= Wn) return;
  const int64_t r = w * 64 + lane;
  const bool valid = r < n;
  const int64_t i = valid ? ind[r] : 0;
  const uint64_t* __restrict__ p = src + (i >> 6);
  const int sh = (int)(i & 63);
  uint64_t mine = 0;
  for (int32_t c = 0; c < k; ++c) {
    const uint64_t word = __ballot(valid && ((p[(int64_t)c * Wm] >> sh) & 1));
    USC_ST_KEEP(word, c, mine);
    if ((c & 63) == 63 || c == k - 1) {
      const int32_t col = (c & ~63) + lane;
      if (lane <= (c & 63)) dst[(int64_t)col * Wn + w] = mine;
    }
  }
}

// one workgroup per bit row: count[row] = its set bits (waves joined in wave order; integer sums)
__global__ __launch_bounds__(kStBlock) void mask_bits_count_kernel(const uint64_t* __restrict__ bits, int64_t W,
                                                                   int32_t* __restrict__ count) {
  __shared__ int32_t red[kStWaves];
  const uint64_t* __restrict__ row = bits + (int64_t)blockIdx.x * W;
  int32_t c = 0;
  for (int64_t w = threadIdx.x; w < W; w += kStBlock) c += __popcll(row[w]);
  c = wave_reduce_add(c);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) count[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// One workgroup, columns in ascending order.  Word w of the foreground belongs to thread w % 1024 from the first
// read to the last write, so only the popcount of a column crosses threads: one barrier per column (the partial sums
// alternate between two LDS rows).  LDS: the foreground lives in LDS and is written back at the end; otherwise it is
// updated in place in global memory.
template <bool LDS>
__global__ __launch_bounds__(kMergeBlock) void selftrain_merge_kernel(const uint64_t* __restrict__ st,
                                                                      const int32_t* __restrict__ total, int32_t kp,
                                                                      int64_t W, uint64_t* fg_g, int32_t max_add,
                                                                      uint64_t* __restrict__ fresh,
                                                                      int32_t* __restrict__ picked,
                                                                      int32_t* __restrict__ n_added) {
  extern __shared__ uint64_t fg_s[];
  __shared__ int32_t red[2][kMergeWaves];
  uint64_t* fg = LDS ? fg_s : fg_g;
  const int tid = threadIdx.x;
  if (LDS)
    for (int64_t w = tid; w < W; w += kMergeBlock) fg_s[w] = fg_g[w];
  int32_t a = 0;
  for (int32_t j = 0; j < kp && a < max_add; ++j) {
    const uint64_t* __restrict__ row = st + (int64_t)j * W;
    int32_t f = 0;
    for (int64_t w = tid; w < W; w += kMergeBlock) f += __popcll(row[w] & ~fg[w]);
    f = wave_reduce_add(f);
    if ((tid & 63) == 0) red[j & 1][tid >> 6] = f;
    __syncthreads();
    f = 0;
#pragma unroll
    for (int v = 0; v < kMergeWaves; ++v) f += red[j & 1][v];
    const int32_t t = total[j];
    if (t > 0 && 2 * (int64_t)f > (int64_t)t) {        // the host rule in integers: a tie is refused
      uint64_t* __restrict__ out = fresh + (int64_t)a * W;
      for (int64_t w = tid; w < W; w += kMergeBlock) {
        const uint64_t x = row[w] & ~fg[w];
        out[w] = x;
        fg[w] |= x;
      }
      if (tid == 0) picked[a] = j;
      ++a;
    }
  }
  for (int64_t e = (int64_t)a * W + tid; e < (int64_t)max_add * W; e += kMergeBlock) fresh[e] = 0ull;
  for (int32_t e = a + tid; e < max_add; e += kMergeBlock) picked[e] = -1;
  if (LDS)
    for (int64_t w = tid; w < W; w += kMergeBlock) fg_g[w] = fg_s[w];
  if (tid == 0) *n_added = a;
}

// grid W.  A workgroup takes the 64 points of one word: the word of up to 256 chosen rows goes to LDS, then
// consecutive threads write consecutive columns of a point's output row.
template <typename T>
__global__ __launch_bounds__(kStBlock) void mask_bits_to_columns_kernel(const uint64_t* __restrict__ bits, int64_t W,
                                                                        const int32_t* __restrict__ rows, int32_t m,
                                                                        int64_t n, T* __restrict__ out, int64_t ld,
                                                                        int32_t col0) {
  __shared__ uint64_t sw[kStBlock];
  const int64_t w = blockIdx.x;
  const int64_t r0 = w * 64;
  const int nr = (int)(n - r0 < 64 ? n - r0 : 64);
  for (int32_t i0 = 0; i0 < m; i0 += kStBlock) {
    const int mc = m - i0 < kStBlock ? m - i0 : kStBlock;
    if ((int)threadIdx.x < mc) sw[threadIdx.x] = bits[(int64_t)rows[i0 + threadIdx.x] * W + w];
    __syncthreads();
    for (int e = threadIdx.x; e < nr * mc; e += kStBlock) {
      const int r = e / mc, i = e - r * mc;
      out[(r0 + r) * ld + col0 + i0 + i] = (T)((sw[i] >> r) & 1);
    }
    __syncthreads();
  }
}

constexpr int64_t kStMaxN = (int64_t)INT32_MAX - 64;     // counts are int32
constexpr int32_t kStMaxK = 1 << 20;

template <typename T>
int bits_to_columns_run(const char* name, const uint64_t* bits, const int32_t* rows, int32_t m, int64_t n, T* out,
                        int64_t ld, int32_t col0, usc_stream_t s) {
  USC_REQUIRE(n >= 0 && n <= kStMaxN, "%s: n out of range [0, 2^31-65]", name);
  USC_REQUIRE(m >= 0 && m <= kStMaxK, "%s: m out of range [0, %d]", name, kStMaxK);
  USC_REQUIRE(col0 >= 0 && ld >= (int64_t)col0 + m, "%s: needs 0 <= col0 and col0 + m <= ld", name);
  if (n == 0 || m == 0) return USC_OK;
  USC_REQUIRE(bits && rows && out, "%s: null pointer", name);
  const int64_t W = ceil_div(n, 64);
  hipLaunchKernelGGL(mask_bits_to_columns_kernel<T>, dim3((unsigned)W), dim3(kStBlock), 0, as_stream(s), bits, W, rows,
                     m, n, out, ld, col0);
  USC_CHECK_LAUNCH(name);
  return USC_OK;
}

}  // namespace
}  // namespace usc

using namespace usc;

extern "C" {

int usc_mask_columns_to_bits(const uint8_t* masks, int64_t n, int32_t k, uint64_t* bits, int32_t* count,
                             usc_stream_t s) {
  USC_REQUIRE(n >= 1 && n <= kStMaxN, "usc_mask_columns_to_bits: n out of range [1, 2^31-65]");
  USC_REQUIRE(k >= 1 && k <= kStMaxK, "usc_mask_columns_to_bits: k out of range [1, %d]", kStMaxK);
  USC_REQUIRE(masks && bits && count, "usc_mask_columns_to_bits: null pointer");
  const int64_t W = ceil_div(n, 64);
  hipStream_t st = as_stream(s);
  hipLaunchKernelGGL(mask_columns_to_bits_kernel, dim3((unsigned)ceil_div(W, kStWaves)), dim3(kStBlock), 0, st, masks,
                     n, k, W, bits);
  USC_CHECK_LAUNCH("usc_mask_columns_to_bits");
  hipLaunchKernelGGL(mask_bits_count_kernel, dim3((unsigned)k), dim3(kStBlock), 0, st, (const uint64_t*)bits, W, count);
  USC_CHECK_LAUNCH("usc_mask_columns_to_bits");
  return USC_OK;
}

int usc_mask_bits_gather(const uint64_t* src, int64_t m, const int64_t* ind, int64_t n, int32_t k, uint64_t* dst,
                         int32_t* count, usc_stream_t s) {
  USC_REQUIRE(m >= 1 && m <= kStMaxN, "usc_mask_bits_gather: m out of range [1, 2^31-65]");
  USC_REQUIRE(n >= 1 && n <= kStMaxN, "usc_mask_bits_gather: n out of range [1, 2^31-65]");
  USC_REQUIRE(k >= 1 && k <= kStMaxK, "usc_mask_bits_gather: k out of range [1, %d]", kStMaxK);
  USC_REQUIRE(src && ind && dst && count, "usc_mask_bits_gather: null pointer");
  const int64_t Wn = ceil_div(n, 64);
  hipStream_t st = as_stream(s);
  hipLaunchKernelGGL(mask_bits_gather_kernel, dim3((unsigned)ceil_div(Wn, kStWaves)), dim3(kStBlock), 0, st, src,
                     ceil_div(m, 64), ind, n, k, Wn, dst);
  USC_CHECK_LAUNCH("usc_mask_bits_gather");
  hipLaunchKernelGGL(mask_bits_count_kernel, dim3((unsigned)k), dim3(kStBlock), 0, st, (const uint64_t*)dst, Wn, count);
  USC_CHECK_LAUNCH("usc_mask_bits_gather");
  return USC_OK;
}

int usc_mask_bits_count(const uint64_t* bits, int32_t k, int64_t n, int32_t* count, usc_stream_t s) {
  USC_REQUIRE(n >= 1 && n <= kStMaxN, "usc_mask_bits_count: n out of range [1, 2^31-65]");
  USC_REQUIRE(k >= 0 && k <= kStMaxK, "usc_mask_bits_count: k out of range [0, %d]", kStMaxK);
  if (k == 0) return USC_OK;
  USC_REQUIRE(bits && count, "usc_mask_bits_count: null pointer");
  hipLaunchKernelGGL(mask_bits_count_kernel, dim3((unsigned)k), dim3(kStBlock), 0, as_stream(s), bits, ceil_div(n, 64),
                     count);
  USC_CHECK_LAUNCH("usc_mask_bits_count");
  return USC_OK;
}

int32_t usc_selftrain_merge_lds_words(int32_t words) {
  const int32_t before = g_merge_lds_words;
  if (words >= 0) g_merge_lds_words = words < kMergeLdsWordsDefault ? words : kMergeLdsWordsDefault;
  return before;
}

int usc_selftrain_merge(const uint64_t* st, const int32_t* total, int32_t kp, int64_t n, uint64_t* fg,
                        int32_t max_add, uint64_t* fresh, int32_t* picked, int32_t* n_added, usc_stream_t s) {
  USC_REQUIRE(n >= 1 && n <= kStMaxN, "usc_selftrain_merge: n out of range [1, 2^31-65]");
  USC_REQUIRE(kp >= 0 && kp <= kStMaxK, "usc_selftrain_merge: kp out of range [0, %d]", kStMaxK);
  USC_REQUIRE(max_add >= 0 && max_add <= kStMaxK, "usc_selftrain_merge: max_add out of range [0, %d]", kStMaxK);
  USC_REQUIRE(fg && n_added, "usc_selftrain_merge: null pointer");
  USC_REQUIRE(kp == 0 || (st && total), "usc_selftrain_merge: null pointer");
  USC_REQUIRE(max_add == 0 || (fresh && picked), "usc_selftrain_merge: null pointer");
  const int64_t W = ceil_div(n, 64);
  if (W <= g_merge_lds_words)
    hipLaunchKernelGGL(selftrain_merge_kernel<true>, dim3(1), dim3(kMergeBlock), (size_t)W * 8, as_stream(s), st, total,
                       kp, W, fg, max_add, fresh, picked, n_added);
  else
    hipLaunchKernelGGL(selftrain_merge_kernel<false>, dim3(1), dim3(kMergeBlock), 0, as_stream(s), st, total, kp, W, fg,
                       max_add, fresh, picked, n_added);
  USC_CHECK_LAUNCH("usc_selftrain_merge");
  return USC_OK;
}

int usc_mask_bits_to_columns(const uint64_t* bits, const int32_t* rows, int32_t m, int64_t n, float* out, int64_t ld,
                             int32_t col0, usc_stream_t s) {
  return bits_to_columns_run<float>("usc_mask_bits_to_columns", bits, rows, m, n, out, ld, col0, s);
}

int usc_mask_bits_to_columns_u8(const uint64_t* bits, const int32_t* rows, int32_t m, int64_t n, uint8_t* out,
                                int64_t ld, int32_t col0, usc_stream_t s) {
  return bits_to_columns_run<uint8_t>("usc_mask_bits_to_columns_u8", bits, rows, m, n, out, ld, col0, s);
}

}  // extern "C"
