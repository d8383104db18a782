// units.hip — native issue path for the backbone: one C call launches every kernel of a
// "convolution -> batch norm (+ residual) (+ ReLU)" unit, forward or backward.
//
// The kernels are the ones behind the per-operator entry points (usc_spconv_*, usc_bn_*); what moves here
// is the ISSUE LOOP.  From Python every launch cost ~10-20 us of interpreter, ctypes, allocator and autograd
// bookkeeping, ~1 000 of them per training step for the backbone alone, which put the host level with the
// device.  A unit is 3-4 launches forward and 4-6 backward behind ONE call; the kernel choice
// (mask-sorted / tile-compacted / row-order / pair-list form, weight transposes, split counts) that lived in
// unscene3d_amd/ops.py is restated here so that both paths launch identical kernels.
//
// Inside this file each such decision is written once: plan_table_gemm (which table-form GEMM, with what scratch: sized
// by table_gemm_ws, executed by table_gemm), wgrad_job / issue_wgrad (which weight-gradient kernel, on which operands:
// inline, on the lane, held, or alone out of a deferred group) and forward_unit (the frame of the three forward units).
//
// Reference: models/modules/resnet_block.py:48-64 (conv -> norm -> relu / `out += residual`),
// models/res16unet.py:231-297 (conv{0..4} / convtr{4..7} + bn + relu), models/modules/common.py:125-188.
#include <stdlib.h>

#include <vector>

#include "common.h"

// rows.hip: the unit calls take the batch norm's tile form on maps of up to usc_bn_tile_max_rows() rows (usc_bn_plan
// reports the same answer)
namespace usc { bool tile_rows_ok(int64_t n, int c); }

using namespace usc;

namespace {

struct WsCursor {
  char* base; int64_t bytes; int64_t off;
  void* take(int64_t n) {
    n = align_up(n > 0 ? n : 16, 256);
    if (off + n > bytes) return nullptr;
    void* p = base + off;
    off += n;
    return p;
  }
  int64_t left() const { return bytes - off; }
  void* rest() { return base + off; }
};

inline bool table_is_compact(int64_t n_out, int cin, int cout, int K) {
  return (usc_spconv_plan(0, n_out, cin, cout, K) >> 12) & 1;
}
inline bool sorted_ok(const usc_kmap* m, int cin, int cout) {
  return m->nbr && m->perm && m->tile_mask && m->K > 1 && m->K <= 32 && cin % 32 == 0 && cout % 32 == 0 && cin <= 4096;
}

// What one table-form GEMM over the map's table launches and takes from the cursor (out rows n_out; wt: the mirrored
// transpose of W is meant).  Sized by table_gemm_ws and executed by table_gemm, so the two cannot drift apart.
struct TableGemmPlan {
  bool sorted;          // the mask-sorted kernel; else the gather kernel (tile-compacted where usc_spconv_plan says so)
  int64_t wt_bytes;     // first take: > 0 when an explicit usc_weight_transpose into it precedes the launch
  int64_t gemm_bytes;   // second take: the kernel's own scratch (0: none taken)
};
TableGemmPlan plan_table_gemm(const usc_kmap* m, int64_t n_out, int cin, int cout, int K, bool wt) {
  const bool compact = m->nbr && table_is_compact(n_out, cin, cout, K);
  if (sorted_ok(m, cin, cout) && !compact) return {true, 0, usc_spconv_sorted_ws_bytes(n_out, cin, cout, K)};
  // the transpose is folded into the tile-compacted kernel only
  return {false, wt && !compact ? (int64_t)K * cin * cout * 4 : 0, usc_spconv_gather_gemm_ws_bytes(n_out, cin, cout, K)};
}

// bytes the table-form GEMM needs
int64_t table_gemm_ws(const usc_kmap* m, int64_t n_out, int cin, int cout, int K, bool wt) {
  const TableGemmPlan pl = plan_table_gemm(m, n_out, cin, cout, K, wt);
  return align_up(pl.wt_bytes, 256) + align_up(pl.gemm_bytes, 256);
}

// out[o] (+)= sum_k in[nbr[k][o]] W[k] over the map's table; `wt`: W is given as the forward [K, cout, cin] and the
// mirrored transpose W'[k][c][n] = W[K-1-k][n][c] is meant (mirror only when K > 1).  No table: identity rows (1x1).
// slices the split-K launch left un-reduced for whoever consumes `out` next (usc_spconv_sorted_gemm_ex)
struct Slices { const float* partial = nullptr; int G = 0; };

int table_gemm(const usc_kmap* m, const float* in, int64_t n_in, int cin, const float* W, int K, int cout, int64_t n_out,
               const float* bias, float* out, int accumulate, int wt, WsCursor ws, usc_stream_t s, Slices* left = nullptr) {
  if (left) *left = Slices{};
  if (n_out == 0) return USC_OK;
  const TableGemmPlan pl = plan_table_gemm(m, n_out, cin, cout, K, wt != 0);
  if (pl.wt_bytes > 0) {
    float* Wt = (float*)ws.take(pl.wt_bytes);
    USC_REQUIRE(Wt, "usc unit: workspace too small (weight transpose)");
    // W is [K, cout, cin] as a forward weight; the product wants [K, cin, cout]
    int rc = usc_weight_transpose(W, K, cout, cin, K > 1 ? 1 : 0, Wt, s);
    if (rc) return rc;
    W = Wt;
    wt = 0;
  }
  const int64_t b = pl.gemm_bytes;
  void* w = b > 0 ? ws.take(b) : nullptr;
  USC_REQUIRE(b == 0 || w, "usc unit: workspace too small (%s gemm)", pl.sorted ? "sorted" : "gather");
  if (!pl.sorted) return usc_spconv_gather_gemm(in, n_in, cin, W, K, cout, m->nbr, n_out, bias, out, accumulate, wt, w, b, s);
  int32_t G = 0;
  const int rc = usc_spconv_sorted_gemm_ex(in, n_in, cin, W, K, cout, m->nbr, m->perm, m->tile_mask, n_out, bias, out,
                                           accumulate, wt, w, b, left ? &G : nullptr, s);
  if (!rc && left && G > 0) { left->partial = (const float*)w; left->G = G; }
  return rc;
}

struct ConvShape { int64_t n_in, n_out; };   // rows of the convolution's input / output feature matrices
inline ConvShape conv_shape(const usc_kmap* m, int kind) {
  return kind == USC_CONV_UP ? ConvShape{m->n_out, m->n_in} : ConvShape{m->n_in, m->n_out};
}

// ---- a unit's weight gradient -------------------------------------------------------------------------------------
// dW[k] (+)= sum over the pairs of offset k of x[a]^T dy[b], described completely: built in ONE place (wgrad_job) and
// launched in ONE place (issue_wgrad), wherever it runs — at once in the caller's scratch, on the lane, noted by the
// lane's hold, or as the lone launch of a deferred group.
struct WgradJob {
  const float* x; const float* dy; float* dW;
  const int32_t* a_idx; const int32_t* b_idx; const int64_t* koff;   // the pair lists; all NULL: identity rows (K = 1)
  int64_t rows; int cin, cout, K;
  int64_t list_bytes;                                                // scratch of the pair-list kernel
  const int32_t* nbr; int64_t n_out, table_bytes;                    // nbr set: the table form may be taken, with its scratch
};
WgradJob wgrad_job(const usc_kmap* m, int kind, ConvShape sh, const float* x, const float* dy, float* dW, int cin, int cout) {
  WgradJob j{};
  j.x = x; j.dy = dy; j.dW = dW; j.cin = cin; j.cout = cout;
  if (m->nbr) {               // the pair lists, in and out swapped for the transposed conv
    const bool up = kind == USC_CONV_UP;
    j.a_idx = up ? m->pair_out : m->pair_in;
    j.b_idx = up ? m->pair_in : m->pair_out;
    j.koff = m->koff; j.K = m->K; j.rows = m->pair_capacity;
  } else {                    // no table: identity rows
    j.K = 1; j.rows = sh.n_in;
  }
  j.list_bytes = usc_spconv_wgrad_ws_bytes_rows(m->K, cin, cout, j.rows);
  // the stem (3 -> 32 channels) has a table-form kernel, on the lane too: it is the LAST weight gradient of the backward
  // pass — the lane's tail, which the step waits for — and the pair-list kernel needs 110 us for it, the table form 57
  // (round 6: the lane branch used to send everything through usc_spconv_wgrad)
  if (kind == USC_CONV_SAME && m->nbr && cin <= 4 && cout == 32 && m->K <= 32) {
    j.nbr = m->nbr; j.n_out = sh.n_out;
    j.table_bytes = usc_spconv_wgrad_table_ws_bytes(m->K, cin, cout);
  }
  return j;
}
// ws / ws_bytes: the scratch the launch may use — the lane's own on the lane, what is left of the caller's when issued
// inline (an asymmetry kept as it was: "the table form fits" is asked of whichever of the two the job runs in).  The
// caller has made sure that the pair-list form fits; the table form is taken where it fits too.
int issue_wgrad(const WgradJob& j, int accumulate, void* ws, int64_t ws_bytes, usc_stream_t s) {
  if (j.nbr && j.table_bytes <= ws_bytes)
    return usc_spconv_wgrad_table(j.x, j.cin, j.dy, j.cout, j.nbr, j.K, j.n_out, j.dW, accumulate, ws, j.table_bytes, s);
  return usc_spconv_wgrad(j.x, j.cin, j.dy, j.cout, j.K, j.a_idx, j.b_idx, j.koff, j.rows, j.dW, accumulate, ws, j.list_bytes, s);
}

// ---- the weight-gradient lane -----------------------------------------------------------------------------------
// The input-gradient and the weight-gradient kernels of one convolution are independent.  On the coarse levels of
// the U-Net (hundreds to a few thousand rows) both are latency-bound launches that occupy a fraction of the 256 CUs,
// so running them side by side costs about as much as the longer of the two.  A fork onto a side stream joined inside
// each call (measured and removed) put the caller's stream behind the side stream once per convolution, and that cost
// more than the overlap returned.  The lane never joins inside a call: the weight gradient of a small map is queued on the
// lane stream behind ONE event of the caller's stream (everything it reads is ready at that point) and the call
// returns; the input-gradient chain — the critical path of the backward pass — carries on, and the latency-bound
// weight-gradient launches of the coarse levels fill the CUs it leaves idle.  The caller joins once, when the
// gradients are needed (usc_wgrad_lane_join), keeps x / dy / dW alive until then, and gives the lane its own scratch.
struct Lane { hipStream_t st = nullptr; hipEvent_t fork = nullptr, join = nullptr, chain = nullptr; void* ws = nullptr; int64_t ws_bytes = 0;
              int64_t max_rows = 0; bool dirty = false;
              // hold: weight gradients of maps with >= hold_min_rows rows are only NOTED until the caller's chain reaches a map
              // with <= release_max_rows rows (or the hold is lifted); from then on everything goes to the lane at once
              bool hold = false; int64_t hold_min_rows = 0, release_max_rows = 0; std::vector<WgradJob> held;
              // chain: recorded on the lane behind the input-gradient chain of a range issued ON the lane
              // (usc_program_run_lane), in front of that range's weight gradients
              bool chain_set = false; };
Lane g_lane[16];
Lane* lane_for_current_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  return g_lane[dev].st ? &g_lane[dev] : nullptr;
}

// the held weight gradients go to the lane, in the order they were noted, behind one event of the caller's stream
int lane_release(Lane* lane, usc_stream_t s) {
  lane->hold = false;
  if (lane->held.empty()) return USC_OK;
  if (hipEventRecord(lane->fork, as_stream(s)) != hipSuccess || hipStreamWaitEvent(lane->st, lane->fork, 0) != hipSuccess) {
    lane->held.clear();
    set_error("usc wgrad lane: releasing the held weight gradients failed (event)");
    return USC_ERR_LAUNCH;
  }
  int rc = USC_OK;
  lane->dirty = true;
  for (size_t i = 0; i < lane->held.size() && !rc; ++i)
    rc = issue_wgrad(lane->held[i], 1, lane->ws, lane->ws_bytes, (usc_stream_t)lane->st);
  lane->held.clear();
  return rc;
}

int check_map(const usc_kmap* m, int kind, int cin, int cout, const char* who) {
  USC_REQUIRE(m, "%s: null kernel map", who);
  USC_REQUIRE(kind == USC_CONV_SAME || kind == USC_CONV_DOWN || kind == USC_CONV_UP, "%s: unknown conv kind %d", who, kind);
  USC_REQUIRE(cin >= 1 && cout >= 1 && m->K >= 1 && m->n_in >= 0 && m->n_out >= 0, "%s: bad sizes", who);
  USC_REQUIRE(m->nbr || (m->K == 1 && kind == USC_CONV_SAME), "%s: K>1 needs a neighbour table", who);
  USC_REQUIRE(kind != USC_CONV_SAME || m->n_in == m->n_out, "%s: a stride-1 map has n_in == n_out", who);
  return USC_OK;
}

// ---- element-wise steps of a step program ---------------------------------------------------------------------------
// dst[r][0:ca] = a[r][:], dst[r][ca:ca+cb] = b[r][:]   (float4 lanes; ca, cb multiples of 4)
__global__ __launch_bounds__(256) void cat_cols_kernel(const float4* __restrict__ a, int ca4, const float4* __restrict__ b,
                                                      int cb4, float4* __restrict__ dst, int64_t total4) {
  const int c4 = ca4 + cb4;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total4; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / c4;
    const int j = (int)(e - r * c4);
    dst[e] = j < ca4 ? a[r * ca4 + j] : b[r * cb4 + (j - ca4)];
  }
}
// da[r][:] = src[r][0:ca], db[r][:] (+)= src[r][ca:ca+cb]
__global__ __launch_bounds__(256) void split_cols_kernel(const float4* __restrict__ src, int ca4, int cb4, float4* __restrict__ da,
                                                        float4* __restrict__ db, int accumulate, int64_t total4) {
  const int c4 = ca4 + cb4;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total4; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / c4;
    const int j = (int)(e - r * c4);
    const float4 v = src[e];
    if (j < ca4) {
      da[r * ca4 + j] = v;
    } else {
      float4* o = db + r * cb4 + (j - ca4);
      if (accumulate) { const float4 t = *o; *o = make_float4(t.x + v.x, t.y + v.y, t.z + v.z, t.w + v.w); }
      else *o = v;
    }
  }
}
__global__ __launch_bounds__(256) void add_inplace_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
  const int64_t n4 = n >> 2;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n4; e += (int64_t)gridDim.x * 256) {
    float4 d = reinterpret_cast<float4*>(dst)[e];
    const float4 v = reinterpret_cast<const float4*>(src)[e];
    d.x += v.x; d.y += v.y; d.z += v.z; d.w += v.w;
    reinterpret_cast<float4*>(dst)[e] = d;
  }
  for (int64_t e = (n4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) dst[e] += src[e];
}
inline unsigned ew_grid(int64_t work) {
  int64_t g = ceil_div(work, (int64_t)256 * 4);
  if (g < 1) g = 1;
  if (g > 2048) g = 2048;
  return (unsigned)g;
}

// weight gradients queued during ONE usc_program_run call (same kernel map and shape -> one grouped launch)
struct DeferredWgrads {
  const usc_kmap* map = nullptr; int cin = 0, cout = 0, n = 0;
  const float* a[16]; const float* b[16]; float* dW[16];
};
int flush_deferred(DeferredWgrads& q, void* ws, int64_t ws_bytes, usc_stream_t s) {
  if (q.n == 0) return USC_OK;
  const usc_kmap* m = q.map;
  int rc = USC_OK;
  if (q.n >= 2 && usc_spconv_wgrad_group_ok(q.n, q.cin, q.cout, m->K, m->pair_capacity)) {
    rc = usc_spconv_wgrad_group(q.n, q.a, q.b, q.dW, q.cin, q.cout, m->K, m->pair_in, m->pair_out, m->koff, m->pair_capacity, 1, s);
  } else {
    // too few for the grouped grid: each its usual launch (only stride-1 table maps are deferred)
    WgradJob j = wgrad_job(m, USC_CONV_SAME, conv_shape(m, USC_CONV_SAME), nullptr, nullptr, nullptr, q.cin, q.cout);
    if (j.list_bytes > ws_bytes) { set_error("usc_program_run: workspace too small (weight gradient)"); rc = USC_ERR_ARG; }
    for (int r = 0; r < q.n && !rc; ++r) {
      j.x = q.a[r]; j.dy = q.b[r]; j.dW = q.dW[r];
      rc = issue_wgrad(j, 1, ws, ws_bytes, s);
    }
  }
  q.n = 0;
  q.map = nullptr;
  return rc;
}

// ---- the bf16 matrix-core precisions of a unit (spconv_bf16.hip): one plane for inference, 2 or 3 for training --------
// the input gradient is the same product over the mirrored transpose: operand shape cout -> cin
bool split_dgrad_ok(const usc_kmap* m, int cin, int cout, int planes) {
  return usc_spconv_gather_gemm_split_ws_bytes(m->n_in, cout, cin, m->K, planes) >= 0;
}
// scratch of one split product: the operand's planes, the packed weight planes, the kernel's own
int64_t split_gemm_ws(const usc_kmap* m, int64_t n_src, int c_src, int c_dst, int planes) {
  const int64_t g = usc_spconv_gather_gemm_split_ws_bytes(m->n_out, c_src, c_dst, m->K, planes);
  return align_up(n_src * c_src * planes * 2, 256) + align_up((int64_t)planes * m->K * c_src * c_dst * 2, 256) +
         align_up(g > 0 ? g : 16, 256);
}
// dst[o] (+)= sum_k sum_{i+j<P} src_i[nbr[k][o]] W_j[k].  src is converted on every call, on the caller's stream; so is W
// f32[K][cin][cout], unless the caller has it packed (Wp, one plane).  transposed: the product over the mirrored
// transpose of W, src has cout channels and dst cin.  up: the transposed conv of a stride-2 map, where every fine row has
// one parent: the child table read backwards is the gather table over the fine rows.
// Scratch, in this order: the operand's planes, the packed weight planes, the kernel's own, the table.
int planes_gemm(const usc_kmap* m, int P, const float* src, int64_t n_src, int c_src, const float* W,
                const uint16_t* Wp, int c_dst, int64_t n_dst, int transposed, bool up, float* dst, int accumulate,
                WsCursor cur, usc_stream_t s, const char* who) {
  const int K = m->K;
  const int64_t gb = P == 1 ? usc_spconv_gather_gemm_bf16_ws_bytes(n_dst, c_src, c_dst, K)
                            : usc_spconv_gather_gemm_split_ws_bytes(n_dst, c_src, c_dst, K, P);
  USC_REQUIRE(gb >= 0, "%s: shape not covered by the bf16 kernels (P=%d, K=%d, %d -> %d channels)", who, P, K, c_src, c_dst);
  uint16_t* xs = (uint16_t*)cur.take(n_src * c_src * P * 2);
  uint16_t* wp = Wp ? nullptr : (uint16_t*)cur.take((int64_t)P * K * c_src * c_dst * 2);
  void* gws = gb > 0 ? cur.take(gb) : nullptr;
  int32_t* table = up ? (int32_t*)cur.take((int64_t)K * n_dst * 4) : nullptr;
  USC_REQUIRE(xs && (Wp || wp) && (gb == 0 || gws) && (!up || table), "%s: workspace too small %s", who,
              P == 1 ? "(usc_unit_bf16_ws_bytes)" : "for the split precision (usc_unit_split_ws_bytes)");
  int rc = P == 1 ? usc_cast_bf16(src, n_src * c_src, xs, s) : usc_split_bf16_rows(src, n_src, c_src, P, xs, s);
  if (rc) return rc;
  if (!Wp) {
    rc = transposed ? usc_spconv_pack_w_split(W, K, c_dst, c_src, P, 1, wp, s)
                    : usc_spconv_pack_w_split(W, K, c_src, c_dst, P, 0, wp, s);
    if (rc) return rc;
    Wp = wp;
  }
  const int32_t* nbr = m->nbr;
  if (up) {
    rc = spconv_up_table(m->nbr, K, m->n_out, n_dst, table, as_stream(s));
    if (rc) return rc;
    nbr = table;
  }
  return P == 1 ? usc_spconv_gather_gemm_bf16(xs, n_src, c_src, Wp, K, c_dst, nbr, n_dst, nullptr, dst, accumulate, gws, gb, s)
                : usc_spconv_gather_gemm_split(xs, n_src, c_src, Wp, K, c_dst, P, nbr, n_dst, nullptr, dst, accumulate, gws, gb, s);
}

void conv_ws_parts(const usc_kmap* m, int kind, int cin, int cout, int64_t* fwd, int64_t* dgrad, int64_t* wg) {
  const int K = m->K;
  const ConvShape sh = conv_shape(m, kind);
  const int64_t wbytes = align_up((int64_t)K * cin * cout * 4, 256);
  *fwd = kind == USC_CONV_UP ? 0 : table_gemm_ws(m, sh.n_out, cin, cout, K, false);      // UP: pair-list form, no scratch
  if (kind == USC_CONV_SAME) *dgrad = table_gemm_ws(m, sh.n_in, cout, cin, K, true);
  else if (kind == USC_CONV_DOWN) *dgrad = wbytes;                                       // transposed weights for the pair-list form
  else *dgrad = wbytes + table_gemm_ws(m, sh.n_in, cout, cin, K, false);
  *dgrad = align_up(*dgrad + 256, 256);
  const WgradJob j = wgrad_job(m, kind, sh, nullptr, nullptr, nullptr, cin, cout);       // whichever form it takes fits
  *wg = align_up(j.nbr && j.table_bytes > j.list_bytes ? j.table_bytes : j.list_bytes, 256);
}

int conv_forward_impl(const usc_kmap* m, int32_t kind, const float* x, int32_t cin, const float* W, int32_t cout,
                      const float* bias, float* y, void* ws, int64_t ws_bytes, usc_stream_t s, Slices* left) {
  if (left) *left = Slices{};
  int rc = check_map(m, kind, cin, cout, "usc_conv_forward");
  if (rc) return rc;
  const ConvShape sh = conv_shape(m, kind);
  if (sh.n_out == 0) return USC_OK;
  USC_REQUIRE(x && W && y, "usc_conv_forward: null pointer");
  WsCursor cur{(char*)ws, ws ? ws_bytes : 0, 0};
  if (kind == USC_CONV_UP) {
    // every fine row has exactly one parent: out[fine] = in[coarse] W[k]
    USC_REQUIRE(m->pair_in && m->pair_out && m->koff, "usc_conv_forward: transposed conv needs the pair lists");
    USC_REQUIRE(!bias, "usc_conv_forward: bias is not supported on the pair-list form");
    return usc_spconv_pairs_gemm(x, cin, W, m->K, cout, m->pair_out, m->pair_in, m->koff, sh.n_out, y, s);
  }
  return table_gemm(m, x, sh.n_in, cin, W, m->K, cout, sh.n_out, bias, y, 0, 0, cur, s, left);
}

// the input gradient of a convolution whose split-K slices are still to be summed: dx = (accumulate ? dx : 0) + sum of
// the G slices; consumed by the batch norm backward of the unit whose output gradient dx is (tile form), or reduced by
// flush_pending
struct Pending { float* dx = nullptr; const float* partial = nullptr; int G = 0; int64_t n = 0; int c = 0; int accumulate = 0; };

int flush_pending(Pending& p, usc_stream_t s) {
  if (p.G <= 0) return USC_OK;
  const int rc = usc_group_reduce(p.partial, p.G, p.n, p.c, nullptr, p.accumulate, p.dx, s);
  p = Pending{};
  return rc;
}

int conv_backward_impl(const usc_kmap* m, int32_t kind, const float* x, int32_t cin, const float* W, int32_t cout,
                       const float* dy, float* dx, int32_t dx_accumulate, float* dW, int32_t dW_accumulate, void* ws,
                       int64_t ws_bytes, usc_stream_t s, Pending* out, int planes = 0) {
  if (out) *out = Pending{};
  int rc = check_map(m, kind, cin, cout, "usc_conv_backward");
  if (rc) return rc;
  const ConvShape sh = conv_shape(m, kind);
  const int K = m->K;
  USC_REQUIRE(x && W && dy, "usc_conv_backward: null pointer");
  WsCursor cur{(char*)ws, ws ? ws_bytes : 0, 0};
  WgradJob job = wgrad_job(m, kind, sh, x, dy, dW, cin, cout);
  // lane: the weight gradient queued on the lane stream, joined by the caller at the end of the backward pass
  if (dW && dW_accumulate && x && dy) {
    Lane* lane = lane_for_current_device();
    const bool lane_ok = lane && sh.n_in > 0 && sh.n_in <= lane->max_rows && sh.n_out <= lane->max_rows &&
                         job.list_bytes <= lane->ws_bytes && (!m->nbr || (m->pair_in && m->pair_out && m->koff));
    const int64_t big = sh.n_in > sh.n_out ? sh.n_in : sh.n_out;
    // the chain has reached a map too small to fill the chip: what was held runs beside it from here on
    if (lane && lane->hold && big <= lane->release_max_rows) { rc = lane_release(lane, s); if (rc) return rc; }
    if (lane_ok && lane->hold && big >= lane->hold_min_rows) {
      // an asymmetry kept as it was: what is held goes through the pair-list kernel when it is released, the stem too (the
      // shipped schedule never holds the stem, but usc_wgrad_lane_hold is public)
      job.nbr = nullptr;
      lane->held.push_back(job);
      dW = nullptr;          // noted; launched by lane_release
    } else if (lane_ok &&
        hipEventRecord(lane->fork, as_stream(s)) == hipSuccess && hipStreamWaitEvent(lane->st, lane->fork, 0) == hipSuccess) {
      lane->dirty = true;
      rc = issue_wgrad(job, 1, lane->ws, lane->ws_bytes, (usc_stream_t)lane->st);
      if (rc) return rc;
      dW = nullptr;          // done (queued); the rest of this call is the input gradient on the caller's stream
    }
  }
  int64_t dgrad_bytes = 0;
  // slices may stay behind only when the consumer can take them (tile-form batch norm on the input map) and nothing in
  // this call overwrites them: the weight gradient then takes its scratch behind the input gradient's region
  Slices left;
  // split precision: the input gradient on the bf16 matrix cores where the transposed shape (cout -> cin) is covered
  const bool split_dx = planes > 0 && kind == USC_CONV_SAME && split_dgrad_ok(m, cin, cout, planes);
  const bool may_defer = !split_dx && out && dx && tile_rows_ok(sh.n_in, cin);
  if (may_defer) {
    int64_t f_, w_;
    conv_ws_parts(m, kind, cin, cout, &f_, &dgrad_bytes, &w_);
    if (dgrad_bytes + w_ > cur.bytes) dgrad_bytes = 0;
  }
  Slices* want = (may_defer && dgrad_bytes > 0) ? &left : nullptr;
  if (dx && sh.n_in > 0) {
    if (split_dx) {
      rc = planes_gemm(m, planes, dy, sh.n_out, cout, W, nullptr, cin, sh.n_in, 1, false, dx, dx_accumulate, cur, s,
                       "usc_conv_backward");
    } else if (kind == USC_CONV_SAME) {
      // stride-1 map: the mirrored offset reaches the rows that read row i; transpose folded where the kernel can
      rc = table_gemm(m, dy, sh.n_out, cout, W, K, cin, sh.n_in, nullptr, dx, dx_accumulate, 1, cur, s, want);
    } else {
      const bool down = kind == USC_CONV_DOWN;
      USC_REQUIRE(!down || !dx_accumulate, "usc_conv_backward: accumulate is not supported on the pair-list form");
      USC_REQUIRE(!down || (m->pair_in && m->pair_out && m->koff), "usc_conv_backward: strided conv needs the pair lists");
      float* Wt = (float*)cur.take((int64_t)K * cin * cout * 4);
      USC_REQUIRE(Wt, "usc_conv_backward: workspace too small");
      rc = usc_weight_transpose(W, K, cin, cout, 0, Wt, s);
      // DOWN: the pair lists read backwards.  UP: dx[coarse] = sum_k dy[child k of coarse] W[k]^T, the child table again
      if (!rc) rc = down ? usc_spconv_pairs_gemm(dy, cout, Wt, K, cin, m->pair_out, m->pair_in, m->koff, sh.n_in, dx, s)
                         : table_gemm(m, dy, sh.n_out, cout, Wt, K, cin, sh.n_in, nullptr, dx, dx_accumulate, 0, cur, s, want);
    }
    if (!rc && left.G > 0) {
      out->dx = dx; out->partial = left.partial; out->G = left.G; out->n = sh.n_in; out->c = cin; out->accumulate = dx_accumulate;
    }
    if (rc) dW = nullptr;   // skip the weight gradient
  }
  if (dW) {
    // the weight gradient reuses the scratch from the start (stream order), or takes it behind the slices left above
    WsCursor wc{(char*)ws, ws ? ws_bytes : 0, left.G > 0 ? dgrad_bytes : 0};
    void* w = wc.take(job.list_bytes);
    if (!w) { set_error("usc_conv_backward: workspace too small (weight gradient)"); return USC_ERR_ARG; }
    rc = issue_wgrad(job, dW_accumulate, w, (char*)ws + ws_bytes - (char*)w, s);
  }
  return rc;
}

// the batch norm's tile form (coarse levels) takes a forward unit's output when the statistics are the batch's
bool bn_tile_form(const usc_bn* bn, int64_t n, int c, int64_t sb) {
  return bn->training && tile_rows_ok(n, c) && sb >= usc_bn_tile_ws_bytes(c);
}

// the end of every forward unit: statistics of y (the batch's, or the running ones in eval mode), then scale and shift
// (+ residual) (+ ReLU).  tile: the caller allows the tile form (bn_tile_form), which sums the split-K slices the
// convolution left behind on its way (none: y is finished).
int bn_act_tail(const char* who, const usc_bn* bn, bool tile, Slices left, float* y, int64_t n, int cout,
                const float* residual, int relu, float* stats, float* out, void* sws, int64_t sb, usc_stream_t s) {
  float* mean = stats, *invstd = stats + cout, *scale = stats + 2 * cout, *shift = stats + 3 * cout;
  if (tile)
    return usc_bn_tile_forward(left.partial, left.G, y, n, cout, bn->gamma, bn->beta, bn->eps, bn->momentum, bn->running_mean,
                               bn->running_var, bn->num_batches_tracked, mean, invstd, scale, shift, residual, relu, out, sws,
                               sb, s);
  int rc;
  if (bn->training) {
    rc = usc_bn_forward_stats(y, n, cout, bn->gamma, bn->beta, bn->eps, bn->momentum, bn->running_mean, bn->running_var,
                              bn->num_batches_tracked, mean, invstd, scale, shift, sws, sb, s);
  } else {
    USC_REQUIRE(bn->running_mean && bn->running_var, "%s: eval mode needs running statistics", who);
    rc = usc_bn_eval_stats(bn->gamma, bn->beta, bn->running_mean, bn->running_var, bn->eps, cout, mean, invstd, scale,
                           shift, s);
  }
  if (rc) return rc;
  return usc_bn_apply(y, scale, shift, residual, relu, out, n, cout, s);
}

// The frame of a forward unit behind the three entry points: the shared checks, the cursor, the batch norm's partials
// FIRST, the convolution, bn_act_tail.  The entry points differ in their error texts and in how y is produced:
struct FwdForm {
  const char* who;       // the entry point
  const char* map_who;   // the name the map is checked under (the f32 unit reports usc_conv_forward's checks)
  const char* ws_note;   // what follows "workspace too small"
  int P;                 // 0: f32 (conv_forward_impl); 1: packed bf16 weights Wp (inference); 2, 3: split planes of W
};
int forward_unit(const FwdForm& f, const usc_kmap* m, int32_t kind, const float* x, int32_t cin, const float* W,
                 const uint16_t* Wp, int32_t cout, const usc_bn* bn, const float* residual, int32_t relu, float* y,
                 float* stats, float* out, void* ws, int64_t ws_bytes, usc_stream_t s) {
  int rc = check_map(m, kind, cin, cout, f.map_who);
  if (rc) return rc;
  USC_REQUIRE(bn && bn->c == cout, "%s: batch-norm width must equal the conv's output width", f.who);
  USC_REQUIRE(y && stats && out && bn->gamma && bn->beta, "%s: null pointer", f.who);
  const ConvShape sh = conv_shape(m, kind);
  if (f.P) {
    const int64_t gb = f.P == 1 ? usc_spconv_gather_gemm_bf16_ws_bytes(sh.n_out, cin, cout, m->K)
                                : usc_spconv_gather_gemm_split_ws_bytes(sh.n_out, cin, cout, m->K, f.P);
    USC_REQUIRE(gb >= 0, "%s: shape not covered (K=%d, %d -> %d channels)", f.who, m->K, cin, cout);
  }
  if (sh.n_out == 0) return USC_OK;
  if (f.P) {
    USC_REQUIRE(x && (f.P == 1 ? (const void*)Wp : (const void*)W), "%s: null pointer", f.who);
    USC_REQUIRE(m->nbr || kind == USC_CONV_SAME, "%s: strided maps need the child table", f.who);
  }
  WsCursor cur{(char*)ws, ws ? ws_bytes : 0, 0};
  const int64_t sb = usc_colstats_ws_bytes(sh.n_out, cout);
  void* sws = cur.take(sb);                       // BN partials first: the conv's scratch takes the rest
  USC_REQUIRE(sws, "%s: workspace too small%s", f.who, f.ws_note);
  // tile form (coarse levels, not in inference): the f32 convolution leaves its split-K slices behind, two launches do
  // the rest; after the split precision it finds y finished (no slices)
  const bool tile = f.P != 1 && bn_tile_form(bn, sh.n_out, cout, sb);
  Slices left;
  if (f.P == 0) rc = conv_forward_impl(m, kind, x, cin, W, cout, nullptr, y, cur.rest(), cur.left(), s, tile ? &left : nullptr);
  else rc = planes_gemm(m, f.P, x, sh.n_in, cin, W, Wp, cout, sh.n_out, 0, kind == USC_CONV_UP, y, 0, cur, s, f.who);
  if (rc) return rc;
  return bn_act_tail(f.who, bn, tile, left, y, sh.n_out, cout, residual, relu, stats, out, sws, sb, s);
}

// in: slices of THIS unit's output gradient (in->dx == dout) left by the previous step, or NULL / empty;
// out: receives the slices of this unit's input gradient when they may stay un-reduced (else left empty)
int unit_backward_impl(const usc_kmap* m, int32_t kind, const float* x, int32_t cin, const float* W, int32_t cout,
                       const usc_bn* bn, const float* y, const float* stats, const float* out_relu,
                       const float* dout, float* dy, float* dres, float* dx, int32_t dx_accumulate, float* dW,
                       int32_t dW_accumulate, float* dgamma, float* dbeta, int32_t dbn_accumulate, void* ws,
                       int64_t ws_bytes, usc_stream_t s, Pending* in, Pending* out, int planes = 0) {
  if (out) *out = Pending{};
  USC_REQUIRE(bn && bn->c == cout, "usc_conv_bn_act_backward: batch-norm width must equal the conv's output width");
  USC_REQUIRE(y && stats && dout && dy && dgamma && dbeta && bn->gamma, "usc_conv_bn_act_backward: null pointer");
  const ConvShape sh = conv_shape(m, kind);
  if (sh.n_out == 0) return USC_OK;
  // split precision: the planes and packs are taken behind the batch norm backward; a short scratch is refused here,
  // before anything is launched (dy, dgamma, dbeta untouched)
  if (planes > 0)
    USC_REQUIRE(ws && ws_bytes >= usc_unit_split_ws_bytes(m, kind, cin, cout, planes),
                "usc_conv_bn_act_backward_split: workspace too small (usc_unit_split_ws_bytes)");
  WsCursor cur{(char*)ws, ws ? ws_bytes : 0, 0};
  const int64_t sb = usc_colstats_ws_bytes(sh.n_out, cout);
  void* sws = cur.take(sb);
  float* red = (float*)cur.take(2 * (int64_t)cout * 4);   // mean_g | mean_gxhat
  USC_REQUIRE(sws && red, "usc_conv_bn_act_backward: workspace too small");
  const float* mean = stats, *invstd = stats + cout;
  int rc;
  const bool has_in = in && in->G > 0;
  if (has_in) USC_REQUIRE(in->dx == dout && in->n == sh.n_out && in->c == cout, "usc unit: pending slices do not belong to this unit");
  if (tile_rows_ok(sh.n_out, cout) && sb >= usc_bn_tile_ws_bytes(cout)) {
    rc = usc_bn_tile_backward(has_in ? in->partial : nullptr, has_in ? in->G : 0, has_in ? in->accumulate : 0, (float*)dout, y,
                              out_relu, mean, invstd, bn->gamma, sh.n_out, cout, bn->training, dbn_accumulate, dgamma,
                              dbeta, dy, dres, sws, sb, s);
    if (has_in) *in = Pending{};
    if (rc) return rc;
  } else {
    if (has_in) { rc = flush_pending(*in, s); if (rc) return rc; }
    rc = usc_bn_backward_reduce(y, dout, out_relu, mean, invstd, sh.n_out, cout, bn->training, dbn_accumulate, dgamma,
                                dbeta, red, red + cout, sws, sb, s);
    if (rc) return rc;
    rc = usc_bn_backward_dx(y, dout, out_relu, mean, invstd, bn->gamma, red, red + cout, dy, dres, sh.n_out, cout, s);
    if (rc) return rc;
  }
  return conv_backward_impl(m, kind, x, cin, W, cout, dy, dx, dx_accumulate, dW, dW_accumulate, cur.rest(), cur.left(), s, out,
                            planes);
}

int check_split(const usc_kmap* m, int32_t kind, int32_t P, const char* who) {
  USC_REQUIRE(m, "%s: null kernel map", who);
  USC_REQUIRE(P == 2 || P == 3, "%s: P must be 2 or 3 (got %d)", who, P);
  USC_REQUIRE(kind == USC_CONV_SAME, "%s: the split precision covers stride-1 units only", who);
  return USC_OK;
}

int64_t program_half_bytes(const usc_step* steps, int32_t n_steps) {
  int64_t need = 256;
  if (!steps) return need;
  for (int i = 0; i < n_steps; ++i) {
    const usc_step& t = steps[i];
    if ((t.op == USC_STEP_UNIT_FWD || t.op == USC_STEP_UNIT_BWD) && t.map) {
      int64_t b = usc_unit_ws_bytes(t.map, t.kind, t.cin, t.cout);
      if (t.split_planes) {                        // (an uncovered shape is reported by the step itself)
        const int64_t sb = usc_unit_split_ws_bytes(t.map, t.kind, t.cin, t.cout, t.split_planes);
        if (sb > b) b = sb;
      }
      if (b > need) need = b;
    } else if (t.op == USC_STEP_UNIT_FWD_BF16 && t.map) {
      const int64_t b = usc_unit_bf16_ws_bytes(t.map, t.kind, t.cin, t.cout);
      if (b > need) need = b;
    }
  }
  return align_up(need, 256);
}

}  // namespace

extern "C" {

int usc_set_wgrad_lane(usc_stream_t lane, void* lane_ws, int64_t lane_ws_bytes, int64_t max_rows) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) {
    set_error("usc_set_wgrad_lane: unsupported device index");
    return USC_ERR_ARG;
  }
  Lane& e = g_lane[dev];
  if (!lane) {
    e.st = nullptr;
    e.held.clear();
    e.hold = false;
    e.chain_set = false;
    return USC_OK;
  }
  USC_REQUIRE(lane_ws && lane_ws_bytes > 0 && max_rows > 0, "usc_set_wgrad_lane: the lane needs its own scratch and a row bound");
  if (!e.fork) {
    if (hipEventCreateWithFlags(&e.fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e.join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e.chain, hipEventDisableTiming) != hipSuccess) {
      set_error("usc_set_wgrad_lane: hipEventCreate failed");
      return USC_ERR_LAUNCH;
    }
  }
  e.st = as_stream(lane);
  e.ws = lane_ws;
  e.ws_bytes = lane_ws_bytes;
  e.max_rows = max_rows;
  e.dirty = false;
  e.chain_set = false;
  return USC_OK;
}

int usc_wgrad_lane_hold(int32_t mode, int64_t hold_min_rows, int64_t release_max_rows, usc_stream_t s) {
  Lane* lane = lane_for_current_device();
  if (!lane) return USC_OK;
  if (mode > 0) {
    USC_REQUIRE(hold_min_rows > release_max_rows && release_max_rows >= 0, "usc_wgrad_lane_hold: hold_min_rows must exceed release_max_rows");
    if (!lane->held.empty()) { const int rc = lane_release(lane, s); if (rc) return rc; }
    lane->hold = true;
    lane->hold_min_rows = hold_min_rows;
    lane->release_max_rows = release_max_rows;
    return USC_OK;
  }
  if (mode < 0) {            // the caller's pass failed: what was noted points into buffers that are gone
    lane->held.clear();
    lane->hold = false;
    return USC_OK;
  }
  return lane_release(lane, s);
}

int32_t usc_wgrad_lane_holding(void) {
  Lane* lane = lane_for_current_device();
  return lane && lane->hold ? 1 : 0;
}

int usc_wgrad_lane_join(usc_stream_t s) {
  Lane* lane = lane_for_current_device();
  if (lane && !lane->held.empty()) { const int rc = lane_release(lane, s); if (rc) return rc; }
  if (!lane || !lane->dirty) return USC_OK;
  if (hipEventRecord(lane->join, lane->st) != hipSuccess || hipStreamWaitEvent(as_stream(s), lane->join, 0) != hipSuccess) {
    set_error("usc_wgrad_lane_join: joining the lane failed");
    return USC_ERR_LAUNCH;
  }
  lane->dirty = false;
  return USC_OK;
}

int64_t usc_conv_ws_bytes(const usc_kmap* m, int32_t kind, int32_t cin, int32_t cout) {
  if (!m) return 0;
  int64_t fwd, dgrad, wg;
  conv_ws_parts(m, kind, cin, cout, &fwd, &dgrad, &wg);
  const int64_t bwd = dgrad + wg;          // disjoint regions: the two may run on different streams
  return (fwd > bwd ? fwd : bwd) + 256;
}

int usc_conv_forward(const usc_kmap* m, int32_t kind, const float* x, int32_t cin, const float* W, int32_t cout,
                     const float* bias, float* y, void* ws, int64_t ws_bytes, usc_stream_t s) {
  return conv_forward_impl(m, kind, x, cin, W, cout, bias, y, ws, ws_bytes, s, nullptr);
}

int usc_conv_backward(const usc_kmap* m, int32_t kind, const float* x, int32_t cin, const float* W, int32_t cout,
                      const float* dy, float* dx, int32_t dx_accumulate, float* dW, int32_t dW_accumulate, void* ws,
                      int64_t ws_bytes, usc_stream_t s) {
  return conv_backward_impl(m, kind, x, cin, W, cout, dy, dx, dx_accumulate, dW, dW_accumulate, ws, ws_bytes, s, nullptr);
}

int64_t usc_unit_ws_bytes(const usc_kmap* m, int32_t kind, int32_t cin, int32_t cout) {
  return usc_conv_ws_bytes(m, kind, cin, cout) + align_up(usc_colstats_ws_bytes(0, cout), 256) +
         align_up(2 * (int64_t)cout * 4, 256) + 256;
}

int usc_conv_bn_act_forward(const usc_kmap* m, int32_t kind, const float* x, int32_t cin, const float* W, int32_t cout,
                            const usc_bn* bn, const float* residual, int32_t relu, float* y, float* stats, float* out,
                            void* ws, int64_t ws_bytes, usc_stream_t s) {
  return forward_unit({"usc_conv_bn_act_forward", "usc_conv_forward", "", 0}, m, kind, x, cin, W, nullptr, cout, bn, residual,
                      relu, y, stats, out, ws, ws_bytes, s);
}

int64_t usc_unit_bf16_ws_bytes(const usc_kmap* m, int32_t kind, int32_t cin, int32_t cout) {
  if (!m) return 0;
  const ConvShape sh = conv_shape(m, kind);
  const int64_t g = usc_spconv_gather_gemm_bf16_ws_bytes(sh.n_out, cin, cout, m->K);
  if (g < 0) return -1;
  int64_t b = align_up(usc_colstats_ws_bytes(sh.n_out, cout), 256) + align_up(sh.n_in * cin * 2, 256) + align_up(g, 256);
  if (kind == USC_CONV_UP) b += align_up((int64_t)m->K * sh.n_out * 4, 256);
  return b + 256;
}

int usc_conv_bn_act_forward_bf16(const usc_kmap* m, int32_t kind, const float* x, int32_t cin, const uint16_t* Wp,
                                 int32_t cout, const usc_bn* bn, const float* residual, int32_t relu, float* y,
                                 float* stats, float* out, void* ws, int64_t ws_bytes, usc_stream_t s) {
  const char* who = "usc_conv_bn_act_forward_bf16";
  return forward_unit({who, who, " (usc_unit_bf16_ws_bytes)", 1}, m, kind, x, cin, nullptr, Wp, cout, bn, residual, relu, y,
                      stats, out, ws, ws_bytes, s);
}

int usc_conv_bn_act_backward(const usc_kmap* m, int32_t kind, const float* x, int32_t cin, const float* W, int32_t cout,
                             const usc_bn* bn, const float* y, const float* stats, const float* out_relu,
                             const float* dout, float* dy, float* dres, float* dx, int32_t dx_accumulate, float* dW,
                             int32_t dW_accumulate, float* dgamma, float* dbeta, int32_t dbn_accumulate, void* ws,
                             int64_t ws_bytes, usc_stream_t s) {
  return unit_backward_impl(m, kind, x, cin, W, cout, bn, y, stats, out_relu, dout, dy, dres, dx, dx_accumulate, dW,
                            dW_accumulate, dgamma, dbeta, dbn_accumulate, ws, ws_bytes, s, nullptr, nullptr);
}

int64_t usc_unit_split_ws_bytes(const usc_kmap* m, int32_t kind, int32_t cin, int32_t cout, int32_t P) {
  if (!m) return 0;
  if ((P != 2 && P != 3) || kind != USC_CONV_SAME) return -1;
  if (usc_spconv_gather_gemm_split_ws_bytes(m->n_out, cin, cout, m->K, P) < 0) return -1;
  // the f32 unit's need (batch-norm partials, weight gradient, an input gradient that stays f32) plus the larger of the
  // forward's and the input gradient's planes and packs
  const int64_t f = split_gemm_ws(m, m->n_in, cin, cout, P);
  const int64_t b = split_dgrad_ok(m, cin, cout, P) ? split_gemm_ws(m, m->n_out, cout, cin, P) : 0;
  return usc_unit_ws_bytes(m, kind, cin, cout) + (f > b ? f : b) + 256;
}

int usc_conv_bn_act_forward_split(const usc_kmap* m, int32_t kind, const float* x, int32_t cin, const float* W, int32_t cout,
                                  int32_t P, const usc_bn* bn, const float* residual, int32_t relu, float* y, float* stats,
                                  float* out, void* ws, int64_t ws_bytes, usc_stream_t s) {
  const char* who = "usc_conv_bn_act_forward_split";
  const int rc = check_split(m, kind, P, who);
  if (rc) return rc;
  return forward_unit({who, who, " (usc_unit_split_ws_bytes)", P}, m, kind, x, cin, W, nullptr, cout, bn, residual, relu, y,
                      stats, out, ws, ws_bytes, s);
}

int usc_conv_bn_act_backward_split(const usc_kmap* m, int32_t kind, const float* x, int32_t cin, const float* W, int32_t cout,
                                   int32_t P, const usc_bn* bn, const float* y, const float* stats, const float* out_relu,
                                   const float* dout, float* dy, float* dres, float* dx, int32_t dx_accumulate, float* dW,
                                   int32_t dW_accumulate, float* dgamma, float* dbeta, int32_t dbn_accumulate, void* ws,
                                   int64_t ws_bytes, usc_stream_t s) {
  const int rc = check_split(m, kind, P, "usc_conv_bn_act_backward_split");
  if (rc) return rc;
  return unit_backward_impl(m, kind, x, cin, W, cout, bn, y, stats, out_relu, dout, dy, dres, dx, dx_accumulate, dW,
                            dW_accumulate, dgamma, dbeta, dbn_accumulate, ws, ws_bytes, s, nullptr, nullptr, P);
}

int32_t usc_step_size(void) { return (int32_t)sizeof(usc_step); }

// two halves: step i works in half i & 1, so the input-gradient slices a backward step leaves for the next one survive it
int64_t usc_program_ws_bytes(const usc_step* steps, int32_t n_steps) { return 2 * program_half_bytes(steps, n_steps) + 256; }

namespace {
// chain_done (optional): recorded on `s` behind the last kernel of the units' chain, in front of the weight gradients the
// call itself deferred
int program_run_impl(const usc_step* steps, int32_t begin, int32_t end, void* ws_all, int64_t ws_all_bytes, usc_stream_t s,
                     hipEvent_t chain_done) {
  USC_REQUIRE(steps && begin >= 0 && end >= begin, "usc_program_run: bad step range");
  hipStream_t st = as_stream(s);
  DeferredWgrads q;
  Pending pend;
  int rc = USC_OK;
  // the scratch in two halves (see usc_program_ws_bytes); a caller that sized it for one step only gets the old behaviour
  const int64_t half = ws_all_bytes > 256 ? (((ws_all_bytes - 256) / 2) & ~(int64_t)255) : 0;
  const bool two = ws_all && half >= program_half_bytes(steps + begin, end - begin);
  void* ws = ws_all;
  int64_t ws_bytes = two ? half : ws_all_bytes;
  for (int i = begin; i < end && !rc; ++i) {
    const usc_step& t = steps[i];
    if (two) ws = (char*)ws_all + (i & 1) * half;
    // slices left by the previous step: only the backward of the unit whose output gradient they are can take them
    if (pend.G > 0 && !(t.op == USC_STEP_UNIT_BWD && t.dout == pend.dx)) {
      rc = flush_pending(pend, s);
      if (rc) break;
    }
    switch (t.op) {
      case USC_STEP_UNIT_FWD:
        rc = t.split_planes ? usc_conv_bn_act_forward_split(t.map, t.kind, t.x, t.cin, t.W, t.cout, t.split_planes, t.bn,
                                                            t.residual, t.relu, t.y, t.stats, t.out, ws, ws_bytes, s)
                            : usc_conv_bn_act_forward(t.map, t.kind, t.x, t.cin, t.W, t.cout, t.bn, t.residual, t.relu, t.y,
                                                      t.stats, t.out, ws, ws_bytes, s);
        break;
      case USC_STEP_UNIT_FWD_BF16:
        rc = usc_conv_bn_act_forward_bf16(t.map, t.kind, t.x, t.cin, (const uint16_t*)t.W, t.cout, t.bn, t.residual, t.relu,
                                          t.y, t.stats, t.out, ws, ws_bytes, s);
        break;
      case USC_STEP_UNIT_BWD: {
        USC_REQUIRE(t.map, "usc_program_run: step %d has no kernel map", i);
        // the same rule as units.py::_defer_wgrad: only shapes the grouped launch can take are postponed (the 3-channel
        // stem keeps its table-form kernel, fine-level convolutions that can never group run at once)
        const bool defer = t.defer_wgrad && t.dW && t.dW_accumulate && t.kind == USC_CONV_SAME && t.map->K > 1 && t.map->pair_in &&
                           t.cin % 32 == 0 && t.cout % 32 == 0 &&
                           (usc_spconv_wgrad_group_ok(2, t.cin, t.cout, t.map->K, t.map->pair_capacity) ||
                            usc_spconv_wgrad_group_ok(usc_spconv_wgrad_group_max(), t.cin, t.cout, t.map->K, t.map->pair_capacity));
        if (defer && q.n > 0 && (q.map != t.map || q.cin != t.cin || q.cout != t.cout || q.n == 16)) {
          rc = flush_deferred(q, ws, ws_bytes, s);       // (this step's half: the previous step's slices are in the other)
          if (rc) break;
        }
        Pending next;
        if (t.split_planes) rc = check_split(t.map, t.kind, t.split_planes, "usc_program_run");
        if (rc) break;
        rc = unit_backward_impl(t.map, t.kind, t.x, t.cin, t.W, t.cout, t.bn, t.y, t.stats, t.out, t.dout, t.dy, t.dres,
                                t.dx, t.dx_accumulate, defer ? nullptr : t.dW, t.dW_accumulate, t.dgamma, t.dbeta,
                                t.dbn_accumulate, ws, ws_bytes, s, &pend, two ? &next : nullptr, t.split_planes);
        if (!rc && pend.G > 0) rc = flush_pending(pend, s);       // (not consumed: cannot happen, kept for safety)
        pend = next;
        if (!rc && defer) {          // x and this step's own dy stay valid until the end of the call (caller's arenas)
          q.map = t.map; q.cin = t.cin; q.cout = t.cout;
          q.a[q.n] = t.x; q.b[q.n] = t.dy; q.dW[q.n] = t.dW;
          ++q.n;
        }
        break;
      }
      case USC_STEP_CAT: {
        USC_REQUIRE(t.a && t.b && t.dst && t.ca % 4 == 0 && t.cb % 4 == 0 && t.n >= 0, "usc_program_run: bad cat step %d", i);
        const int64_t total4 = t.n * ((t.ca + t.cb) / 4);
        if (total4 > 0)
          hipLaunchKernelGGL(cat_cols_kernel, dim3(ew_grid(total4)), dim3(256), 0, st, (const float4*)t.a, t.ca / 4,
                             (const float4*)t.b, t.cb / 4, (float4*)t.dst, total4);
        break;
      }
      case USC_STEP_SPLIT: {
        USC_REQUIRE(t.a && t.dst && t.dst2 && t.ca % 4 == 0 && t.cb % 4 == 0 && t.n >= 0, "usc_program_run: bad split step %d", i);
        const int64_t total4 = t.n * ((t.ca + t.cb) / 4);
        if (total4 > 0)
          hipLaunchKernelGGL(split_cols_kernel, dim3(ew_grid(total4)), dim3(256), 0, st, (const float4*)t.a, t.ca / 4, t.cb / 4,
                             (float4*)t.dst, (float4*)t.dst2, (int)t.accumulate, total4);
        break;
      }
      case USC_STEP_ADD:
        USC_REQUIRE(t.a && t.dst && t.n >= 0, "usc_program_run: bad add step %d", i);
        if (t.n > 0) hipLaunchKernelGGL(add_inplace_kernel, dim3(ew_grid(t.n / 4 + 1)), dim3(256), 0, st, t.dst, t.a, t.n);
        break;
      default:
        set_error("usc_program_run: unknown step op");
        rc = USC_ERR_ARG;
    }
  }
  int rc3 = flush_pending(pend, s);
  if (chain_done && !rc && !rc3 && hipEventRecord(chain_done, st) != hipSuccess) {
    set_error("usc_program_run_lane: recording the chain's event failed");
    rc3 = USC_ERR_LAUNCH;
  }
  // the queued weight gradients last: with two halves, the one the pending slices (just reduced, in stream order) were not in
  const int rc2 = flush_deferred(q, ws, ws_bytes, s);
  if (rc) return rc;
  if (rc3) return rc3;
  if (rc2) return rc2;
  USC_CHECK_LAUNCH("usc_program_run");
  return USC_OK;
}
}  // namespace

int usc_program_run(const usc_step* steps, int32_t begin, int32_t end, void* ws_all, int64_t ws_all_bytes, usc_stream_t s) {
  return program_run_impl(steps, begin, end, ws_all, ws_all_bytes, s, nullptr);
}

int usc_program_run_lane(const usc_step* steps, int32_t begin, int32_t end, void* ws, int64_t ws_bytes, usc_stream_t s) {
  Lane* lane = lane_for_current_device();
  USC_REQUIRE(lane, "usc_program_run_lane: no weight-gradient lane on this device (usc_set_wgrad_lane)");
  USC_REQUIRE(ws != lane->ws, "usc_program_run_lane: the range needs scratch of its own, not the lane's");
  const usc_stream_t ls = (usc_stream_t)lane->st;
  // what an earlier hold noted goes first, behind the caller's stream as usual
  if (!lane->held.empty() || lane->hold) { const int rc = lane_release(lane, s); if (rc) return rc; }
  if (as_stream(s) != lane->st &&
      (hipEventRecord(lane->fork, as_stream(s)) != hipSuccess || hipStreamWaitEvent(lane->st, lane->fork, 0) != hipSuccess)) {
    set_error("usc_program_run_lane: putting the lane behind the caller's stream failed (event)");
    return USC_ERR_LAUNCH;
  }
  // the chain first: every weight gradient the lane would take is noted and goes behind the chain's event
  lane->hold = true;
  lane->hold_min_rows = 0;
  lane->release_max_rows = -1;
  lane->dirty = true;
  lane->chain_set = false;
  int rc = program_run_impl(steps, begin, end, ws, ws_bytes, ls, lane->chain);
  if (rc) {                                   // nothing stays noted after a failed range
    lane->held.clear();
    lane->hold = false;
    return rc;
  }
  lane->chain_set = true;
  return lane_release(lane, ls);
}

int usc_wgrad_lane_wait_chain(usc_stream_t s) {
  Lane* lane = lane_for_current_device();
  USC_REQUIRE(lane && lane->chain_set, "usc_wgrad_lane_wait_chain: no range has been issued on the lane (usc_program_run_lane)");
  if (as_stream(s) != lane->st && hipStreamWaitEvent(as_stream(s), lane->chain, 0) != hipSuccess) {
    set_error("usc_wgrad_lane_wait_chain: waiting for the chain's event failed");
    return USC_ERR_LAUNCH;
  }
  return USC_OK;
}

}  // extern "C"
