/*
 * usc3d.h — flat C ABI of libusc3d_hip.so: the MI355X (gfx950) hot path of
 * UnScene3D's self-training step and pseudo-mask generator.
 *
 * Every entry point takes raw DEVICE pointers (caller-owned, contiguous,
 * row-major), plain sizes and an explicit stream (hipStream_t passed as
 * void*).  No entry point allocates, frees, synchronises or keeps a pointer
 * beyond the call; scratch memory is passed in by the caller (sizes via the
 * *_ws_bytes helpers).  Every function returns 0 on success or a negative
 * usc_status; usc_last_error() gives the message (the Python wrapper raises
 * RuntimeError — never exit()/abort(), cf. reference cuda_utils.cpp:4-6 vs
 * pointnet2 cuda_utils.h:32-41).
 *
 * Each declaration cites the reference interface it replaces
 * (paths relative to RozDavid/UnScene3D @ 2024_10_08).
 * [ME] = MinkowskiEngine 0.5.4, an un-vendored dependency of the reference
 * (conf/unscene3d_requirements.txt:50); semantics restated in oracle/.
 */
#ifndef USC3D_H
#define USC3D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* usc_stream_t; /* hipStream_t */

enum usc_status {
  USC_OK = 0,
  USC_ERR_ARG = -1,     /* bad argument (null pointer, unsupported shape) */
  USC_ERR_LAUNCH = -2,  /* HIP launch/runtime error */
  USC_ERR_RANGE = -3    /* coordinate outside the packable range */
};

/* Message for the last failing call on this thread ("" if none). */
const char* usc_last_error(void);
/* Library/ABI version (bumped on any signature change). */
int usc_abi_version(void);
/* What the loaded library was built from: "arch=gfx950; HIP version: ...; built <UTC time>; sources sha256 <16 hex>" (the
 * hash covers every .hip / .cpp / .h the objects were compiled from).  __graft_entry__.build() and smoke() print it. */
const char* usc_build_info(void);
/* Number of visible HIP devices, or a negative usc_status. */
int usc_device_count(void);

/* ------------------------------------------------------------------------
 * V1/V3/R1  coordinate maps  — replaces [ME] ME.utils.sparse_quantize
 * (datasets/utils.py:403-408, pseudo_masks/datasets/voxelizer.py:142) and the
 * coordinate-manager insert behind ME.SparseTensor(...) (trainer/trainer.py:115)
 * and the stride-2 maps implied by MinkowskiConvolution(k=2,s=2)
 * (models/res16unet.py:51-116).
 * ---------------------------------------------------------------------- */

/* coords_out[i,:] = floor(xyz[i,:] / voxel_size) in float64 (== np.floor(x/v),
 * datasets/utils.py:403), cast to int32.  xyz: f64[n,3]. */
int usc_voxel_floor_f64(const double* xyz, int64_t n, double voxel_size,
                        int32_t* coords_out, usc_stream_t s);

/* HIP-FREE, fork-safe host forms (plain C++ over HOST pointers; no HIP call, no global state): the reference voxelises
 * in forked DataLoader workers on the CPU (datasets/utils.py:403-414, conf/data/indoor.yaml:24), where the parent's HIP
 * runtime must not be touched.  usc_voxel_floor_f64_host = usc_voxel_floor_f64; usc_unique_coords_host = the unique_idx /
 * inverse pair of usc_coordmap_build(quant = 1) on coords i32[n,d], d = 3 (x,y,z) or 4 (b,x,y,z): first-occurrence rows
 * in ascending order — ME.utils.sparse_quantize(return_index=True, return_inverse=True).  Bit-equal to the device path. */
int usc_voxel_floor_f64_host(const double* xyz, int64_t n, double voxel_size,
                             int32_t* coords_out);
int usc_unique_coords_host(const int32_t* coords, int64_t n, int32_t d,
                           int64_t* unique_idx, int64_t* inverse,
                           int64_t* n_out);

/* Hash-table capacity (slots, power of two) required for n coordinates. */
int64_t usc_coordmap_capacity(int64_t n);
/* Scratch bytes for usc_coordmap_build on n rows. */
int64_t usc_coordmap_ws_bytes(int64_t n);

/* Build a coordinate map (open-addressing hash on the packed 64-bit key of
 * (b, x, y, z)) over coords i32[n,4], optionally quantising x,y,z to
 * multiples of `quant` first (quant<=1: none; quant = 2*tensor_stride builds
 * the next-coarser map: c -> floor(c/quant)*quant).
 * Outputs, all caller-allocated:
 *   table_keys u64[cap], table_vals i32[cap]  — persistent map: key -> row
 *   unique_idx i64[n]   first n_out entries valid: the FIRST-OCCURRENCE input
 *                       row of each distinct coordinate, ascending
 *                       (== unique_map of sparse_quantize)
 *   inverse    i64[n]   row of the distinct coordinate each input row maps to
 *                       (== inverse_map)
 *   out_coords i32[n,4] first n_out rows valid: the distinct (quantised)
 *                       coordinates in map-row order (may be NULL)
 *   n_out      i64[1]   device scalar
 */
int usc_coordmap_build(const int32_t* coords, int64_t n, int32_t quant,
                       uint64_t* table_keys, int32_t* table_vals, int64_t cap,
                       int64_t* unique_idx, int64_t* inverse,
                       int32_t* out_coords, int64_t* n_out,
                       void* ws, int64_t ws_bytes, usc_stream_t s);

/* Spatial (z-order) cell id of every row: Morton code of ((c - lo) >> shift) with
 * bits_per_axis bits per axis, batch index above it.  Feeding these ids to
 * usc_segment_csr gives a stable, cache-friendly row permutation (rows of one
 * 2^shift-voxel cell become contiguous) — an MI355X-side optimisation of the
 * collate step (datasets/utils.py:412-417 gathers by unique_map; any consistent
 * row order is valid downstream); it keeps gathers of neighbouring rows inside
 * one XCD's L2. */
int usc_morton_cell_ids(const int32_t* coords, int64_t n, int32_t shift,
                        int32_t lo_x, int32_t lo_y, int32_t lo_z,
                        int32_t bits_per_axis, int64_t* ids, usc_stream_t s);

/* ------------------------------------------------------------------------
 * R2  kernel maps ("rulebooks") — replaces [ME] the kernel-map construction
 * cached by the CoordinateManager for MinkowskiConvolution /
 * MinkowskiConvolutionTranspose / MinkowskiAvgPooling
 * (models/modules/common.py:125-188, models/mask3d.py:131).
 * ---------------------------------------------------------------------- */

/* Dense neighbour table for a stride-1 k^3 HYPER_CUBE kernel on one map:
 *   nbr[k*n + o] = row i with coord_i == coord_o + off_k*tensor_stride, else -1
 * offsets: ksize=3 -> {-1,0,1}^3, x fastest (k = dx+1 + 3(dy+1) + 9(dz+1)).
 * coords i32[n,4] are the map's coordinates; table_* its hash table. */
int usc_kernel_map_cube(const int32_t* coords, int64_t n, int32_t tensor_stride,
                        int32_t ksize, const uint64_t* table_keys,
                        const int32_t* table_vals, int64_t cap, int32_t* nbr,
                        usc_stream_t s);

/* Child table of a k=2,s=2 kernel between a fine map (n_fine rows, tensor
 * stride ts) and its coarse parent (n_coarse rows):
 *   nbr2[k*n_coarse + p] = fine row whose parent is p and whose offset index is
 *       k = ox + 2*oy + 4*oz, o = (c_fine - c_parent)/ts in {0,1}^3, else -1
 *   kidx[i] = k of fine row i (u8)
 * parent i64[n_fine] is the `inverse` returned by usc_coordmap_build(quant=2ts).
 * nbr2 must be pre-filled with -1 by the caller. */
int usc_kernel_map_down2(const int32_t* fine_coords, int64_t n_fine,
                         int32_t tensor_stride, const int64_t* parent,
                         const int32_t* coarse_coords, int64_t n_coarse,
                         int32_t* nbr2, uint8_t* kidx, usc_stream_t s);

/* Scratch bytes for usc_rulebook_compact on a [K, n_out] table. */
int64_t usc_rulebook_ws_bytes(int64_t K, int64_t n_out);
/* Compact a dense neighbour table into per-offset pair lists, ordered by
 * (k, out row):  for p in [koff[k], koff[k+1]): (in_idx[p], out_idx[p]).
 * in_idx/out_idx i32[K*n_out] capacity, koff i64[K+1] (device). */
int usc_rulebook_compact(const int32_t* nbr, int64_t K, int64_t n_out,
                         int32_t* in_idx, int32_t* out_idx, int64_t* koff,
                         void* ws, int64_t ws_bytes, usc_stream_t s);

/* ------------------------------------------------------------------------
 * C  sparse convolution — replaces [ME] MinkowskiConvolution /
 * MinkowskiConvolutionTranspose forward + backward
 * (models/modules/common.py:146,179; instances models/res16unet.py:39-221,
 * models/modules/resnet_block.py:24-43, models/mask3d.py:60-62).
 * fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32.
 * ---------------------------------------------------------------------- */

/* out[k][co][ci] = W[mirror ? K-1-k : k][ci][co]  — weights for the dgrad
 * kernels (mirror=1 for a stride-1 odd kernel whose map is its own transpose). */
int usc_weight_transpose(const float* W, int32_t K, int32_t cin, int32_t cout,
                         int32_t mirror, float* out, usc_stream_t s);

/* Output-stationary implicit GEMM over a dense neighbour table:
 *   out[o,:] = sum_k  in[nbr[k*n_out+o], :] @ W[k]  (+ bias)
 * in f32[n_in,cin], W f32[K,cin,cout].  nbr==NULL means K==1 identity
 * (1x1 conv / linear).  bias f32[cout] or NULL.  accumulate=1 adds into out.
 * Small maps (coarse U-Net levels) split the K offsets over extra workgroups and
 * reduce the partial sums in a fixed order through `ws`
 * (usc_spconv_gather_gemm_ws_bytes; 0 bytes when no split is planned).
 * w_transposed=1 (tile-compacted plan, usc_spconv_plan bit 12; also K = 1 on identity rows with cin, cout multiples of
 * 32 — a linear layer's [cout][cin] weight read in place): W is the forward
 * conv's f32[K,cout,cin] and W'[k][c][n] = W[K-1-k][n][c] is used (stride-1 dgrad).
 * Covers: k3/s1 conv fwd and dgrad (W = usc_weight_transpose(mirror=1), or w_transposed),
 * k2/s2 conv fwd (nbr = child table), conv-transpose dgrad. */
/* Launch plan chosen for a shape (for profiling labels): returns
 * NB | aligned<<8 | G<<16 where NB = 32-column blocks per wave, aligned = fast
 * path, G = offset groups.  kind 0: gather_gemm (n = n_out), 1: pairs_gemm
 * (n = P_capacity), 2: wgrad (bit 13 set: the all-input-tiles kernel, CT = code>>16). */
int usc_spconv_plan(int32_t kind, int64_t n, int32_t cin, int32_t cout,
                    int32_t K);
/* Mask-sorted form of the same convolution (all map sizes, cin and cout multiples
 * of 32).  usc_rowsort_build groups the OUTPUT rows of a neighbour table by their
 * neighbour bitmask (one bucket pass on up to 12 informative offset bits):
 *   perm      i32[n_out]            output rows, similar masks adjacent
 *   tile_mask u32[ceil(n_out/32)]   OR of the masks of each run of 32 rows of perm
 * so that a 32-row matrix-core tile skips every offset none of its rows has.
 * usc_spconv_sorted_gemm computes usc_spconv_gather_gemm's result; its output
 * bits do not depend on perm (each output element is reduced by one lane over
 * k ascending, channel ascending); weights are staged through LDS per workgroup.
 * One perm serves the forward conv and, for a stride-1 map, its input gradient:
 * w_transposed=1 takes the FORWARD weights f32[K, cout, cin] and uses
 * W'[k][c][n] = W[K-1-k][n][c] while staging them (no usc_weight_transpose pass).
 * Replaces the same MinkowskiEngine calls as usc_spconv_gather_gemm
 * (models/res16unet.py:224-297; ME 0.5.4 src/convolution_kernel.cu, un-vendored). */
int64_t usc_rowsort_ws_bytes(int32_t K, int64_t n_out);
int usc_rowsort_build(const int32_t* nbr, int32_t K, int64_t n_out,
                      int32_t* perm, uint32_t* tile_mask, void* ws,
                      int64_t ws_bytes, usc_stream_t s);
int64_t usc_spconv_sorted_ws_bytes(int64_t n_out, int32_t cin, int32_t cout,
                                   int32_t K);
int usc_spconv_sorted_gemm(const float* in, int64_t n_in, int32_t cin,
                           const float* W, int32_t K, int32_t cout,
                           const int32_t* nbr, const int32_t* perm,
                           const uint32_t* tile_mask, int64_t n_out,
                           const float* bias, float* out, int32_t accumulate,
                           int32_t w_transposed, void* ws, int64_t ws_bytes,
                           usc_stream_t s);
/* The same with the slice reduction left to the caller: when the launch plan splits the K offsets over G > 1 partial-sum
 * slices and `slices_left` is not NULL (and there is no bias), *slices_left = G, the slices f32[G][n_out][cout] stay at
 * the start of `ws`, and `out` / `accumulate` are NOT applied — the caller sums the slices in slice order, usually fused
 * with what follows the convolution (usc_bn_tile_forward / usc_bn_tile_backward below; usc_group_reduce is the plain
 * form).  *slices_left = 0: the call did everything, as usc_spconv_sorted_gemm.  Replaces the same MinkowskiEngine
 * calls (models/modules/common.py:125-188). */
int usc_spconv_sorted_gemm_ex(const float* in, int64_t n_in, int32_t cin,
                              const float* W, int32_t K, int32_t cout,
                              const int32_t* nbr, const int32_t* perm,
                              const uint32_t* tile_mask, int64_t n_out,
                              const float* bias, float* out, int32_t accumulate,
                              int32_t w_transposed, void* ws, int64_t ws_bytes,
                              int32_t* slices_left, usc_stream_t s);
/* out[n,c] = (accumulate ? out : 0) + bias + sum_g partial[g][n][c], g ascending (the reduction the split-K launches
 * end with; c a multiple of 4). */
int usc_group_reduce(const float* partial, int32_t G, int64_t n, int32_t c,
                     const float* bias, int32_t accumulate, float* out,
                     usc_stream_t s);

int64_t usc_spconv_gather_gemm_ws_bytes(int64_t n_out, int32_t cin,
                                        int32_t cout, int32_t K);
int usc_spconv_gather_gemm(const float* in, int64_t n_in, int32_t cin,
                           const float* W, int32_t K, int32_t cout,
                           const int32_t* nbr, int64_t n_out,
                           const float* bias, float* out, int32_t accumulate, int32_t w_transposed,
                           void* ws, int64_t ws_bytes, usc_stream_t s);

/* One-parent form (transposed-conv forward, strided-conv dgrad):
 *   out[rows_out[p],:] = in[rows_in[p],:] @ W[k]   for p in [koff[k], koff[k+1])
 * driven by the per-offset pair lists of usc_rulebook_compact on the child
 * table (every output row appears in exactly one pair).  koff i64[K+1] device,
 * P_capacity = upper bound of koff[K] known to the host. */
int usc_spconv_pairs_gemm(const float* in, int32_t cin, const float* W,
                          int32_t K, int32_t cout, const int32_t* rows_in,
                          const int32_t* rows_out, const int64_t* koff,
                          int64_t P_capacity, float* out, usc_stream_t s);

/* ------------------------------------------------------------------------
 * bf16 matrix-core forward convolution (opt-in inference precision,
 * unscene3d_amd.inference_precision("bf16")): bf16 operands on
 * v_mfma_f32_32x32x16_bf16, f32 accumulation, f32 output.  Replaces the
 * forward of MinkowskiConvolution / MinkowskiConvolutionTranspose
 * (ME 0.5.4 src/convolution_kernel.cu; models/res16unet.py:224-297) only
 * under that opt-in; training always runs the f32 kernels above.
 * ---------------------------------------------------------------------- */
/* out[i] = bf16(in[i]), round to nearest even (NaN stays NaN); in 16-byte,
 * out 8-byte aligned.  The activation copy the bf16 conv gathers from
 * (replaces the input read of the ME forward conv). */
int usc_cast_bf16(const float* in, int64_t n, uint16_t* out, usc_stream_t s);
/* Weights f32[K,cin,cout] -> bf16 in B-fragment order,
 * Wp[k][cin/16][cout/32][64][8] with Wp[k][s][t][l][j] = W[k][16s + 8(l>>5) + j][32t + (l&31)]
 * (K*cin*cout bf16 values; cin a multiple of 16, cout of 32).  Replaces ME's
 * kernel parameter as the forward conv reads it. */
int usc_spconv_pack_w_bf16(const float* W, int32_t K, int32_t cin, int32_t cout,
                           uint16_t* Wp, usc_stream_t s);
/* Scratch bytes usc_spconv_gather_gemm_bf16 needs for a shape (0: none), or
 * -1 when the shape is not covered (cin % 16, cout % 32, K > 64, ...): the
 * caller then takes the f32 path. */
int64_t usc_spconv_gather_gemm_bf16_ws_bytes(int64_t n_out, int32_t cin,
                                             int32_t cout, int32_t K);
/* out[o,:] (= or += when accumulate) sum_k in[nbr[k*n_out+o],:] @ W[k] (+ bias)
 * with in bf16[n_in,cin] (usc_cast_bf16), Wp packed (usc_spconv_pack_w_bf16);
 * nbr -1 = no neighbour (contributes zero), nbr NULL = K==1 identity rows.
 * Each output element is summed by one lane over k and channel ascending: no
 * atomics, no split-K, bit-identical from run to run.  Covers the forward of
 * k3/s1 (K=27), k2/s2 (K=8, nbr = child table) and, on the inverted child
 * table, the k2 transposed conv.  Replaces the same ME calls as
 * usc_spconv_gather_gemm, forward only. */
int usc_spconv_gather_gemm_bf16(const uint16_t* in, int64_t n_in, int32_t cin,
                                const uint16_t* Wp, int32_t K, int32_t cout,
                                const int32_t* nbr, int64_t n_out,
                                const float* bias, float* out, int32_t accumulate,
                                void* ws, int64_t ws_bytes, usc_stream_t s);

/* ------------------------------------------------------------------------
 * Split-bf16 matrix-core convolution at f32-grade accuracy (opt-in training
 * precision, unscene3d_amd.training_precision("bf16x2" | "bf16x3")): each f32
 * operand is P bf16 planes x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1)
 * (round to nearest even, f32 subtractions), and the plane products (i, j) with
 * i + j < P are summed in f32 on v_mfma_f32_32x32x16_bf16.  Dropped terms:
 * <= 2^-23 |x||w| per product for P = 3, <= 3 * 2^-16 |x||w| for P = 2.
 * Stands for the forward and the input gradient of MinkowskiConvolution
 * (ME 0.5.4 src/convolution_kernel.cu; models/modules/common.py:125-188,
 * models/res16unet.py:224-297) under that opt-in; the weight gradient stays on
 * the f32 kernels.
 * ---------------------------------------------------------------------- */
/* in f32[rows,c] -> out bf16[rows][P][c] (the planes of one row are contiguous:
 * what the split conv gathers).  P is 2 or 3.  A value whose first plane is
 * not finite keeps it and gets zero in the other planes (inf stays inf).  in
 * 16-byte, out 8-byte aligned.  Replaces the input read of the ME conv
 * forward / backward (models/modules/common.py:125-188). */
int usc_split_bf16_rows(const float* in, int64_t rows, int32_t c, int32_t P,
                        uint16_t* out, usc_stream_t s);
/* The same for a flat array, any n: out bf16[P][n] (one row of n values). */
int usc_split_bf16(const float* in, int64_t n, int32_t P, uint16_t* out,
                   usc_stream_t s);
/* Weights f32[K,cin,cout] -> P bf16 planes, each in the B-fragment order of
 * usc_spconv_pack_w_bf16, one plane after the other (P*K*cin*cout values).
 * transposed = 1 packs the mirrored transpose the input gradient needs,
 * W'[k][n][c] = W[K-1-k][c][n] (K == 1: the plain transpose), the convention of
 * usc_weight_transpose(mirror); the operand shape is then cout -> cin.  The
 * operand's input width must be a multiple of 16, its output width of 32.
 * Replaces ME's kernel parameter as the conv forward / backward reads it
 * (models/modules/common.py:125-188). */
int usc_spconv_pack_w_split(const float* W, int32_t K, int32_t cin, int32_t cout,
                            int32_t P, int32_t transposed, uint16_t* Wp,
                            usc_stream_t s);
/* Scratch bytes usc_spconv_gather_gemm_split needs (0: none), or -1 when the
 * shape is not covered (P not 2 or 3, cin % 16, cout % 32, K > 64, ...). */
int64_t usc_spconv_gather_gemm_split_ws_bytes(int64_t n_out, int32_t cin,
                                              int32_t cout, int32_t K, int32_t P);
/* out[o,:] (= or += when accumulate) sum_k sum_{i+j<P} x_i[nbr[k*n_out+o],:] @ W_j[k] (+ bias)
 * with in bf16[n_in][P][cin] (usc_split_bf16_rows), Wp from
 * usc_spconv_pack_w_split; nbr -1 = no neighbour, nbr NULL = K==1 identity
 * rows.  One lane sums each output element over k, channel step and product
 * in a fixed order: no atomics, no split-K, bit-identical from run to run.
 * Replaces the same ME calls as usc_spconv_gather_gemm for the stride-1 conv
 * forward and, on the transposed pack, its input gradient
 * (MinkowskiConvolution forward / backward, models/modules/common.py:125-188). */
int usc_spconv_gather_gemm_split(const uint16_t* in, int64_t n_in, int32_t cin,
                                 const uint16_t* Wp, int32_t K, int32_t cout,
                                 int32_t P, const int32_t* nbr, int64_t n_out,
                                 const float* bias, float* out,
                                 int32_t accumulate, void* ws, int64_t ws_bytes,
                                 usc_stream_t s);

/* Scratch bytes for usc_spconv_wgrad. */
int64_t usc_spconv_wgrad_ws_bytes(int32_t K, int32_t cin, int32_t cout);
/* Weight gradient:  dW[k] = sum_{p in list k}  a[a_idx[p],:]^T  b[b_idx[p],:]
 * a f32[*,cin], b f32[*,cout], dW f32[K,cin,cout]; pair lists as produced by
 * usc_rulebook_compact (a_idx/b_idx i32, koff i64[K+1] device).
 * a_idx==NULL && K==1: identity pairs over n_rows (1x1 conv). Deterministic
 * (fixed split + ordered reduction, no float atomics).  accumulate=1 adds into
 * dW (a parameter's existing gradient buffer) instead of overwriting it. */
int usc_spconv_wgrad(const float* a, int32_t cin, const float* b, int32_t cout,
                     int32_t K, const int32_t* a_idx, const int32_t* b_idx,
                     const int64_t* koff, int64_t n_rows, float* dW, int32_t accumulate, void* ws,
                     int64_t ws_bytes, usc_stream_t s);
/* Exact scratch need of usc_spconv_wgrad for pair lists of capacity n_rows (the bound
 * above assumes the maximum split count). */
int64_t usc_spconv_wgrad_ws_bytes_rows(int32_t K, int32_t cin, int32_t cout,
                                       int64_t n_rows);
/* Weight gradient in TABLE form for few input channels (cin <= 4, cout = 32: the 3 -> 32 stem, reference
 * models/res16unet.py conv0p1s1):  dW[k][c][n] = sum_o in[nbr[k][o]][c] dy[o][n]  with the forward conv's neighbour
 * table nbr i32[K, n_out].  32 / cin offsets share one MFMA tile (row m = offset, channel), 3 groups instead of 27
 * per-offset passes with 3 useful tile rows each. */
int64_t usc_spconv_wgrad_table_ws_bytes(int32_t K, int32_t cin, int32_t cout);
int usc_spconv_wgrad_table(const float* in, int32_t cin, const float* dy, int32_t cout, const int32_t* nbr, int32_t K,
                           int64_t n_out, float* dW, int32_t accumulate, void* ws, int64_t ws_bytes, usc_stream_t s);

/* GROUPED weight gradient: R problems of one shape on one kernel map — the conv1 / conv2 weight gradients of a level's
 * residual blocks (reference models/modules/resnet_block.py:48-64 builds them, autograd differentiates them one by
 * one; models/res16unet.py LAYERS = 2..6 same-shape blocks per level) — in ONE grid: dW[r][k] (+)= sum_p a[r][a_idx[p]]^T
 * b[r][b_idx[p]].  a / b / dW: HOST arrays of R device pointers (copied into the launch; R <= usc_spconv_wgrad_group_max()).
 * No pair split and no reduction launch: every (problem, offset, channel tile) workgroup walks its whole pair list and
 * writes (accumulate = 1: adds into) dW[r][k] itself, in a fixed order.  usc_spconv_wgrad_group_ok: whether the grouped
 * form applies (channel pair covered, >= 256 workgroups, <= 2 048 pairs per offset: the coarse levels). */
/* > 0: usc_spconv_wgrad launches its all-input-tiles kernel with at most that many workgroups along x, each walking
 * several (offset, split) work items ("background form": the launch leaves wave slots and matrix-core time on every CU
 * to the kernels of another stream).  0 restores the plain launches.  Process-wide; set by the weight-gradient lane
 * around its own launches.  Same arithmetic, same results. */
void usc_spconv_wgrad_grid_limit(int32_t max_workgroups);
int32_t usc_spconv_wgrad_group_max(void);
int usc_spconv_wgrad_group_ok(int32_t R, int32_t cin, int32_t cout, int32_t K, int64_t n_rows);
int usc_spconv_wgrad_group(int32_t R, const float* const* a, const float* const* b, float* const* dW, int32_t cin,
                           int32_t cout, int32_t K, const int32_t* a_idx, const int32_t* b_idx, const int64_t* koff,
                           int64_t n_rows, int32_t accumulate, usc_stream_t s);

/* ------------------------------------------------------------------------
 * Native issue path: whole convolutions and "conv -> batch norm (+ residual)
 * (+ ReLU)" units behind ONE call each way — the operator granularity of
 * models/modules/resnet_block.py:48-64 (conv1/norm1/relu, conv2/norm2,
 * `out += residual`, relu) and of the stem / strided / transposed stages of
 * models/res16unet.py:231-297.  Same kernels and kernel choice as the
 * per-operator entry points above; the point is that the host issues 3-6
 * launches per call instead of one per call from the interpreter.
 *
 * usc_kmap describes one kernel map of the batch (built by usc_kernel_map_cube /
 * usc_kernel_map_down2, usc_rowsort_build, usc_rulebook_compact); all pointers
 * are device pointers owned by the caller's coordinate manager.
 *   kind USC_CONV_SAME : k^3 stride-1 conv on one map (n_in == n_out), or a 1x1
 *                        conv when nbr == NULL and K == 1
 *        USC_CONV_DOWN : k=2,s=2 conv, fine map (n_in rows) -> coarse map
 *                        (n_out rows); nbr = child table [8][n_out]
 *        USC_CONV_UP   : the transposed conv on the SAME map description:
 *                        input = coarse rows (n_out), output = fine rows (n_in)
 * ---------------------------------------------------------------------- */
typedef struct usc_kmap {
  const int32_t* nbr;        /* i32[K][n_out]; NULL: identity (1x1 conv) */
  const int32_t* perm;       /* usc_rowsort_build of nbr, or NULL */
  const uint32_t* tile_mask; /* usc_rowsort_build of nbr, or NULL */
  const int32_t* pair_in;    /* usc_rulebook_compact of nbr: rows of the n_in side */
  const int32_t* pair_out;   /*                              rows of the n_out side */
  const int64_t* koff;       /* i64[K+1] (device) */
  int64_t n_in, n_out;
  int64_t pair_capacity;     /* allocated length of pair_in / pair_out */
  int32_t K;
  int32_t reserved;
} usc_kmap;

enum usc_conv_kind { USC_CONV_SAME = 0, USC_CONV_DOWN = 1, USC_CONV_UP = 2 };

/* MinkowskiBatchNorm == BatchNorm1d over rows (models/modules/common.py:22).
 * training != 0: batch statistics (+ running-stat update when running_* != NULL,
 * num_batches_tracked incremented when != NULL); else running statistics. */
typedef struct usc_bn {
  const float* gamma;
  const float* beta;
  float* running_mean;
  float* running_var;
  int64_t* num_batches_tracked;
  float eps, momentum;
  int32_t c;
  int32_t training;
} usc_bn;

/* Optional: the weight-gradient LANE, a second stream of the caller with its own scratch (NULL lane: off; per device).
 * usc_conv_backward / usc_conv_bn_act_backward then queue the weight gradient of a map with <= max_rows rows (only
 * the accumulate-into-a-gradient-buffer form) on the lane behind one event of the caller's stream and return WITHOUT
 * waiting for it; the input-gradient chain of the backward pass is not held up, the latency-bound weight-gradient
 * launches of the coarse U-Net levels run beside it.  The caller keeps x, dy and dW alive and untouched until it has
 * called usc_wgrad_lane_join(s) — `s` then waits for everything queued on the lane so far (end of the backward pass,
 * and before a gradient bucket is handed to a collective).  Results are unchanged (same kernels, same order per
 * gradient buffer). */
int usc_set_wgrad_lane(usc_stream_t lane, void* lane_ws, int64_t lane_ws_bytes, int64_t max_rows);
int usc_wgrad_lane_join(usc_stream_t s);
/* Scheduling of the lane against the caller's chain (step program of the backbone's backward pass, which visits the
 * U-Net stages fine -> coarse -> fine, models/res16unet.py:224-297 in reverse).  mode 1: from now on the weight gradient
 * of a map with >= hold_min_rows rows is only NOTED; the first backward call on a map with <= release_max_rows rows —
 * a stage whose launches cannot fill 256 CUs — puts everything noted on the lane behind one event of `s` and ends the
 * hold (later calls queue at once, as without a hold).  The throughput-bound fine-level weight gradients then run
 * beside the latency-bound coarse-level chain instead of beside the fine-level input gradients they compete with for
 * matrix-core issue slots.  mode 0: release what is still noted and end the hold (also done by usc_wgrad_lane_join).
 * mode -1: forget what was noted (the caller's pass failed; the noted pointers are stale).  The caller keeps every
 * noted x / dy / dW alive until the join, as for a queued one.  Results are unchanged. */
int usc_wgrad_lane_hold(int32_t mode, int64_t hold_min_rows, int64_t release_max_rows, usc_stream_t s);
/* 1 while a hold is in force on the current device (nothing released yet), else 0. */
int32_t usc_wgrad_lane_holding(void);
/* Launch statistics of the tile-compacted kernel (the dominant kernel of the step, models/modules/common.py:125-188),
 * taken by the kernel itself while a real step runs — every stream, graph and lane as they are — so that the bench can
 * report the kernel's rate inside the step it times (`roofline.frac_in_step`) next to its rate alone.  Between begin and
 * end every such launch gets the next slot of `ring_dev` (device memory, slots x 4 x u64, initialised on `s` by begin):
 * {earliest workgroup start, latest workgroup end (wall-clock ticks, usc_wall_clock_khz), real (in, out) pairs of the
 * launch, 0}; launches beyond `slots` are not recorded.  usc_launch_stats_end stops the recording and copies the shapes
 * of the recorded launches, in launch order, into host_out (<= max_out entries); it returns their number.  The caller
 * synchronises before reading the ring.  Cost while recording: two atomics per workgroup. */
typedef struct usc_launch_stat { int64_t n_out; int32_t cin, cout, K, nb; } usc_launch_stat;
int usc_launch_stats_begin(void* ring_dev, int64_t slots, usc_stream_t s);
int64_t usc_launch_stats_end(usc_launch_stat* host_out, int64_t max_out);
int64_t usc_wall_clock_khz(void);
/* Scratch bytes covering forward AND backward of one convolution / one unit. */
int64_t usc_conv_ws_bytes(const usc_kmap* m, int32_t kind, int32_t cin,
                          int32_t cout);
int64_t usc_unit_ws_bytes(const usc_kmap* m, int32_t kind, int32_t cin,
                          int32_t cout);
/* y = conv(x; W) (+ bias; bias only for SAME/DOWN).  W f32[K,cin,cout]. */
int usc_conv_forward(const usc_kmap* m, int32_t kind, const float* x,
                     int32_t cin, const float* W, int32_t cout,
                     const float* bias, float* y, void* ws, int64_t ws_bytes,
                     usc_stream_t s);
/* dx (skipped when NULL; dx_accumulate adds into dx — gather forms only) and
 * dW (skipped when NULL; dW_accumulate adds into a gradient buffer). */
int usc_conv_backward(const usc_kmap* m, int32_t kind, const float* x,
                      int32_t cin, const float* W, int32_t cout,
                      const float* dy, float* dx, int32_t dx_accumulate,
                      float* dW, int32_t dW_accumulate, void* ws,
                      int64_t ws_bytes, usc_stream_t s);
/* mean/invstd/scale/shift of an eval-mode batch norm from its running statistics. */
int usc_bn_eval_stats(const float* gamma, const float* beta,
                      const float* running_mean, const float* running_var,
                      float eps, int32_t c, float* mean, float* invstd,
                      float* scale, float* shift, usc_stream_t s);
/* out = [relu]( BN(conv(x; W)) (+ residual) ).  Saved for the backward pass:
 * y = conv output f32[n,cout], stats f32[4][cout] = mean | invstd | scale | shift,
 * out (its sign is the ReLU mask). */
int usc_conv_bn_act_forward(const usc_kmap* m, int32_t kind, const float* x,
                            int32_t cin, const float* W, int32_t cout,
                            const usc_bn* bn, const float* residual,
                            int32_t relu, float* y, float* stats, float* out,
                            void* ws, int64_t ws_bytes, usc_stream_t s);
/* Backward of the unit.  out_relu = the forward output when relu was applied, else
 * NULL.  dy f32[n,cout] receives d(conv output) (scratch the caller may drop);
 * dres (or NULL) receives the residual branch's gradient (= masked dout).
 * dgamma/dbeta: written, or added into when dbn_accumulate. */
int usc_conv_bn_act_backward(const usc_kmap* m, int32_t kind, const float* x,
                             int32_t cin, const float* W, int32_t cout,
                             const usc_bn* bn, const float* y,
                             const float* stats, const float* out_relu,
                             const float* dout, float* dy, float* dres,
                             float* dx, int32_t dx_accumulate, float* dW,
                             int32_t dW_accumulate, float* dgamma,
                             float* dbeta, int32_t dbn_accumulate, void* ws,
                             int64_t ws_bytes, usc_stream_t s);
/* usc_conv_bn_act_forward with the convolution in bf16 (usc_spconv_gather_gemm_bf16):
 * Wp = the conv's weights packed by usc_spconv_pack_w_bf16; x is f32 and is
 * cast to bf16 in the scratch; batch norm, residual and ReLU are the f32 ones of
 * usc_conv_bn_act_forward (no tile form).  Inference only: y / stats / out are
 * as there, but nothing here is meant for a backward pass.  Returns an error
 * for shapes usc_spconv_gather_gemm_bf16_ws_bytes does not cover.  Replaces ME's
 * conv forward + MinkowskiBatchNorm under the bf16 inference precision. */
int64_t usc_unit_bf16_ws_bytes(const usc_kmap* m, int32_t kind, int32_t cin,
                               int32_t cout);
int usc_conv_bn_act_forward_bf16(const usc_kmap* m, int32_t kind,
                                 const float* x, int32_t cin,
                                 const uint16_t* Wp, int32_t cout,
                                 const usc_bn* bn, const float* residual,
                                 int32_t relu, float* y, float* stats,
                                 float* out, void* ws, int64_t ws_bytes,
                                 usc_stream_t s);

/* usc_conv_bn_act_forward / _backward of a stride-1 (USC_CONV_SAME) unit with the
 * convolution's forward and input gradient in split bf16 (P = 2 or 3 planes,
 * usc_spconv_gather_gemm_split).  Forward: x is split and W packed into the
 * scratch on the caller's stream on EVERY call (no cache: an optimizer may write
 * W in place between, or inside, passes), then the unit's f32 batch norm,
 * residual and ReLU run as in usc_conv_bn_act_forward (tile form included; the
 * convolution leaves no slices).  Backward: batch norm backward as in
 * usc_conv_bn_act_backward, then dy is split, W packed transposed and dx
 * computed over the map's table (dx_accumulate honoured); where the transposed
 * shape is not covered (cin % 32 != 0) the input gradient runs on the f32
 * kernels.  The weight gradient is exactly usc_conv_bn_act_backward's: f32
 * kernels, lane, hold / release.  The forward returns an error for shapes
 * usc_spconv_gather_gemm_split_ws_bytes does not cover, and both return one,
 * before anything is launched, when the scratch is too short (the backward:
 * shorter than usc_unit_split_ws_bytes).  Replaces ME's
 * MinkowskiConvolution forward / backward + MinkowskiBatchNorm
 * (models/modules/common.py:125-188, models/modules/resnet_block.py:48-64) under
 * the split training precision. */
int64_t usc_unit_split_ws_bytes(const usc_kmap* m, int32_t kind, int32_t cin,
                                int32_t cout, int32_t P);
int usc_conv_bn_act_forward_split(const usc_kmap* m, int32_t kind,
                                  const float* x, int32_t cin, const float* W,
                                  int32_t cout, int32_t P, const usc_bn* bn,
                                  const float* residual, int32_t relu, float* y,
                                  float* stats, float* out, void* ws,
                                  int64_t ws_bytes, usc_stream_t s);
int usc_conv_bn_act_backward_split(const usc_kmap* m, int32_t kind,
                                   const float* x, int32_t cin, const float* W,
                                   int32_t cout, int32_t P, const usc_bn* bn,
                                   const float* y, const float* stats,
                                   const float* out_relu, const float* dout,
                                   float* dy, float* dres, float* dx,
                                   int32_t dx_accumulate, float* dW,
                                   int32_t dW_accumulate, float* dgamma,
                                   float* dbeta, int32_t dbn_accumulate,
                                   void* ws, int64_t ws_bytes, usc_stream_t s);

/* ------------------------------------------------------------------------
 * Step programs: the issue loop of a whole network stage behind ONE call.
 * The reference walks Res16UNetBase.forward (models/res16unet.py:224-297) module by module from the interpreter, and
 * autograd walks it back; here the caller describes the same walk once as an array of steps — conv+BN units, the
 * channel concatenation of a skip connection (`me.cat`, :259-289), and for the way back the units' backward calls, the
 * column split of a concatenation's gradient and the fan-in adds of tensors with several consumers — and
 * usc_program_run launches steps [begin, end) in order on the stream.  Every pointer is a device pointer owned by the
 * caller (activations, gradients and scratch live in the caller's arenas for as long as the steps need them); the
 * library allocates nothing and keeps nothing: deferred weight gradients (defer_wgrad != 0, see
 * usc_spconv_wgrad_group) are queued inside one call only and flushed before it returns.
 *   USC_STEP_UNIT_FWD : usc_conv_bn_act_forward(map, kind, x, cin, W, cout, bn, residual, relu, y, stats, out)
 *   USC_STEP_UNIT_BWD : usc_conv_bn_act_backward(map, kind, x, cin, W, cout, bn, y, stats, out (NULL: no ReLU),
 *                       dout, dy, dres, dx, dx_accumulate, dW, dW_accumulate, dgamma, dbeta, dbn_accumulate)
 *   USC_STEP_CAT      : dst[n, ca + cb] = [a[n, ca] | b[n, cb]]
 *   USC_STEP_SPLIT    : dst[n, ca] = a[:, :ca];  dst2[n, cb] (+= when accumulate) a[:, ca:ca + cb]   (a is [n, ca + cb])
 *   USC_STEP_ADD      : dst[0 .. n) += a[0 .. n)   (n counts floats)
 *   USC_STEP_UNIT_FWD_BF16 : usc_conv_bn_act_forward_bf16(map, kind, x, cin, W (read as the packed bf16 weights),
 *                       cout, bn, residual, relu, y, stats, out)
 * A USC_STEP_UNIT_FWD / USC_STEP_UNIT_BWD step with split_planes = 2 or 3 calls usc_conv_bn_act_forward_split /
 * usc_conv_bn_act_backward_split with P = split_planes instead (0: the f32 unit).
 * ---------------------------------------------------------------------- */
enum usc_step_op { USC_STEP_UNIT_FWD = 0, USC_STEP_UNIT_BWD = 1, USC_STEP_CAT = 2, USC_STEP_SPLIT = 3, USC_STEP_ADD = 4,
                   USC_STEP_UNIT_FWD_BF16 = 5 };
typedef struct usc_step {
  int32_t op, kind, cin, cout, relu;
  int32_t dx_accumulate, dW_accumulate, dbn_accumulate, defer_wgrad, accumulate;
  const usc_kmap* map;
  const usc_bn* bn;
  const float* x;
  const float* W;
  const float* residual;
  float* y;
  float* stats;
  float* out;
  const float* dout;
  float* dy;
  float* dres;
  float* dx;
  float* dW;
  float* dgamma;
  float* dbeta;
  const float* a;
  const float* b;
  float* dst;
  float* dst2;
  int64_t n;
  int32_t ca, cb;
  int32_t split_planes, reserved;
} usc_step;
/* sizeof(usc_step) as the library was compiled: a binding checks its own mirror of the structure against it. */
int32_t usc_step_size(void);
/* Scratch bytes that cover every step of the program (the steps run one after the other on one stream). */
int64_t usc_program_ws_bytes(const usc_step* steps, int32_t n_steps);
int usc_program_run(const usc_step* steps, int32_t begin, int32_t end, void* ws, int64_t ws_bytes, usc_stream_t s);
/* Steps [begin, end) of a backward program issued ON the weight-gradient lane (usc_set_wgrad_lane; an error without one):
 * the lane waits behind one event of `s`, then runs the units' input-gradient chain, then — behind an event of its own,
 * "the chain is done" — every weight gradient of the range (those the lane takes are noted while the chain is issued,
 * as under usc_wgrad_lane_hold, and released behind it).  `s` does not wait for anything: a later
 * usc_wgrad_lane_wait_chain(s) puts `s` behind the chain only (whoever continues the program from the range's input
 * gradients), usc_wgrad_lane_join(s) behind everything.  For a range whose gradients do not depend on what `s` is about
 * to run: the finest U-Net stage beside the mask decoder's backward.  ws: scratch of the range's own
 * (usc_program_ws_bytes), neither the lane's nor one that other streams use meanwhile.  A hold in force is released
 * first.  Same kernels and the same results as usc_program_run on `s`. */
int usc_program_run_lane(const usc_step* steps, int32_t begin, int32_t end, void* ws, int64_t ws_bytes, usc_stream_t s);
int usc_wgrad_lane_wait_chain(usc_stream_t s);

/* ------------------------------------------------------------------------
 * B  row-wise batch norm / ReLU / residual — replaces [ME] MinkowskiBatchNorm
 * (= BatchNorm1d over feature rows), MinkowskiReLU and `out += residual`
 * (models/modules/common.py:22, models/modules/resnet_block.py:48-64).
 * ---------------------------------------------------------------------- */

int64_t usc_colstats_ws_bytes(int64_t n, int32_t c);
/* Per-channel sums over rows: sum1[c] = sum_i x[i,c], sum2[c] = sum_i x[i,c]*y[i,c]
 * (y==NULL -> x*x).  Deterministic two-stage reduction.  f32 in, f64 partials. */
int usc_colstats(const float* x, const float* y, int64_t n, int32_t c,
                 double* sum1, double* sum2, void* ws, int64_t ws_bytes,
                 usc_stream_t s);
/* BatchNorm1d training statistics in one pass (f64 accumulation) + finalisation:
 * mean, invstd = 1/sqrt(var_biased+eps), scale = gamma*invstd, shift = beta-mean*scale,
 * and the running-stat update running = (1-m)*running + m*{mean, var_unbiased}
 * (running_* may both be NULL).  ws: usc_colstats_ws_bytes(n, c).  num_batches_tracked (i64[1]
 * or NULL) is incremented by the same launch. */
int usc_bn_forward_stats(const float* x, int64_t n, int32_t c, const float* gamma,
                         const float* beta, float eps, float momentum,
                         float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean,
                         float* invstd, float* scale, float* shift, void* ws,
                         int64_t ws_bytes, usc_stream_t s);
/* y = [relu]( x*scale[c] + shift[c] (+ residual) ); mask-free (backward uses y>0). */
int usc_bn_apply(const float* x, const float* scale, const float* shift,
                 const float* residual, int32_t relu, float* y, int64_t n,
                 int32_t c, usc_stream_t s);
/* BatchNorm backward given saved mean/invstd and channel sums of (dy) and (dy*xhat):
 *   g = relu_mask ? (y_out>0 ? dy : 0) : dy      (applied on the fly when y_out!=NULL)
 *   dx = gamma*invstd*( g - mean_g - xhat*mean_gxhat ),  xhat=(x-mean)*invstd
 * Also writes dres = g when dres != NULL (residual branch gradient). */
int usc_bn_backward_dx(const float* x, const float* dy, const float* y_out,
                       const float* mean, const float* invstd,
                       const float* gamma, const float* mean_g,
                       const float* mean_gxhat, float* dx, float* dres,
                       int64_t n, int32_t c, usc_stream_t s);
/* Reductions needed by the above in one pass: dbeta[c] = sum g, dgamma[c] = sum g*xhat,
 * mean_g = dbeta/n, mean_gxhat = dgamma/n (both 0 when training==0: eval-mode BN
 * treats the statistics as constants).  g applies the ReLU mask of y_out when given.  accumulate=1 adds dgamma / dbeta into the given
 * buffers (the parameters' gradient tensors) instead of overwriting them. */
/* TILE FORM of the training-mode batch norm around a split-K convolution, for maps of up to usc_bn_tile_max_rows() rows
 * (the U-Net's coarse levels, where every launch sits on its latency floor): conv -> BN (+ residual) (+ ReLU) of
 * models/modules/resnet_block.py:48-64 / models/modules/common.py:22 in TWO launches after the convolution instead of
 * four (slice reduction, statistics, finalisation, apply):
 *   forward   y = sum of the G slices `partial` f32[G][n][c] in slice order (G == 0: y already holds the conv output),
 *             per-tile f64 column sums, then every workgroup of the apply launch adds the <= 64 tile sums in tile order,
 *             finalises (mean / invstd / scale / shift and the running statistics written once) and applies
 *             out = [relu](y * scale + shift [+ residual]).  Same statistics as usc_bn_forward_stats up to the order of
 *             the f64 additions.
 *   backward  dout' = (accumulate ? dout : 0) + sum of the G input-gradient slices (G == 0: dout is finished),
 *             g = ReLU-masked dout' (y_out != NULL), tile sums of g and g * xhat; then dgamma / dbeta (added into when
 *             dbn_accumulate), and dy = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)) (training == 0: the two
 *             means are 0).  g is written to dres when given (the residual branch's gradient), else in place into dout
 *             when it was formed from slices; a finished dout without dres is not written.
 * ws: usc_bn_tile_ws_bytes(c) bytes.  usc_bn_tile_ok(n, c): do the kernels cover this map (c a multiple of 32, <= 1024)?
 * usc_bn_tile_max_rows(): the map size up to which usc_conv_bn_act_forward / _backward and usc_program_run TAKE this form
 * (4 096 rows). */
int64_t usc_bn_tile_max_rows(void);
/* Host only, launches nothing: the forms a [n, c] map takes (n, c >= 1; else -1).  Computed by the helpers the launch
 * code itself calls.
 *   bits 0-1   statistics form of usc_bn_forward_stats (backward = 0) / usc_bn_backward_reduce (backward = 1):
 *              0 refused, 1 one launch (bn_small_kernel), 2 two launches (colstats_kernel + finalisation)
 *   bit 2      one launch: the XCD column remap is on
 *   bits 3-5   two launches: channels per lane (4 or 1);  bits 8-19: their number of workgroups
 *   bit 20     usc_bn_tile_ok(n, c);  then bits 24-31: row tiles of usc_bn_tile_*, bits 32 up: rows per tile
 *   bit 21     usc_conv_bn_act_forward (training mode) / _backward (both modes) and usc_program_run take the tile form on
 *              this map */
int64_t usc_bn_plan(int64_t n, int32_t c, int32_t backward);
int usc_bn_tile_ok(int64_t n, int32_t c);
int64_t usc_bn_tile_ws_bytes(int32_t c);
int usc_bn_tile_forward(const float* partial, int32_t G, float* y, int64_t n,
                        int32_t c, const float* gamma, const float* beta,
                        float eps, float momentum, float* running_mean,
                        float* running_var, int64_t* num_batches_tracked,
                        float* mean, float* invstd, float* scale, float* shift,
                        const float* residual, int32_t relu, float* out,
                        void* ws, int64_t ws_bytes, usc_stream_t s);
int usc_bn_tile_backward(const float* partial, int32_t G, int32_t accumulate,
                         float* dout, const float* y, const float* y_out,
                         const float* mean, const float* invstd,
                         const float* gamma, int64_t n, int32_t c,
                         int32_t training, int32_t dbn_accumulate,
                         float* dgamma, float* dbeta, float* dy, float* dres,
                         void* ws, int64_t ws_bytes, usc_stream_t s);
int usc_bn_backward_reduce(const float* x, const float* dy, const float* y_out,
                           const float* mean, const float* invstd, int64_t n,
                           int32_t c, int32_t training, int32_t accumulate, float* dgamma,
                           float* dbeta, float* mean_g, float* mean_gxhat,
                           void* ws, int64_t ws_bytes, usc_stream_t s);
/* y = max(x,0);  dx = (y>0) ? dy : 0 */
int usc_relu_fwd(const float* x, float* y, int64_t numel, usc_stream_t s);
int usc_relu_bwd(const float* y, const float* dy, float* dx, int64_t numel,
                 usc_stream_t s);

/* ------------------------------------------------------------------------
 * P  average pooling — replaces [ME] MinkowskiAvgPooling(kernel_size=2,
 * stride=2, dimension=3) forward (models/mask3d.py:131,213,432).
 *   out[p,:] = mean over present children nbr2[k*n_coarse+p]
 * ---------------------------------------------------------------------- */
int usc_avgpool_down2(const float* in, int32_t c, const int32_t* nbr2,
                      int64_t n_coarse, float* out, usc_stream_t s);
/* The attention-mask chain of the mask module (models/mask3d.py:418-439: per-voxel
 * logits = segment logits gathered through point2segment, pooled
 * num_pooling_steps times, then sigmoid < 0.5) without the [voxels, Q] table:
 *   row_of (optional, i64[n_fine]): child ch reads row row_of[ch] of `in`
 *          (leading dimension ld >= c) — first step, `in` = the [segments, Q] logits;
 *   mask_out (optional, u8[n_coarse, c]): last step writes
 *          sigmoid(mean) < 0.5 instead of the means (`out` may then be NULL). */
int usc_avgpool_down2_ex(const float* in, int32_t c, int32_t ld,
                         const int64_t* row_of, const int32_t* nbr2,
                         int64_t n_coarse, float* out, uint8_t* mask_out,
                         usc_stream_t s);

/* ------------------------------------------------------------------------
 * gather / scatter rows (D1 mask-module row gather mask3d.py:418-419, feature
 * gathers by unique_map datasets/utils.py:412-417)
 * ---------------------------------------------------------------------- */
/* out[i,:] = src[idx[i],:]   idx i64[n] */
int usc_gather_rows(const float* src, int32_t c, const int64_t* idx, int64_t n,
                    float* out, usc_stream_t s);

/* dst[idx[i],:] += src[i,:]  (dst caller-zeroed) — backward of usc_gather_rows for sampled
 * index sets (float atomics; exact and order-independent when idx has no duplicates). */
int usc_scatter_add_rows(const float* src, int32_t c, const int64_t* idx,
                         int64_t n, float* dst, usc_stream_t s);

/* dst[idx[i],:] = src[i,:] for an index set the CALLER knows to be free of duplicates (a permutation,
 * torch.randperm(n)[:k] — the decoder's sampled keys, models/mask3d.py:325): plain 16-byte stores, no atomics;
 * with a zeroed dst this is the backward of usc_gather_rows at gather bandwidth.  Duplicates would race. */
int usc_scatter_rows_unique(const float* src, int32_t c, const int64_t* idx,
                            int64_t n, float* dst, usc_stream_t s);
/* dst[idx[i],:] += src[i,:] for a duplicate-free index set: plain read-modify-write.  Several sampled subsets of one
 * table (the three decoders' key samples of a level, models/mask3d.py:306-349: autograd sums their three scattered
 * gradients) are accumulated launch after launch into ONE buffer instead of three zero-filled tensors and two adds. */
int usc_scatter_rows_unique_add(const float* src, int32_t c, const int64_t* idx,
                                int64_t n, float* dst, usc_stream_t s);

/* The decoder's key sampling of one pass (reference models/mask3d.py:306-346: three row gathers by the sampled
 * indices, `attn[attn.sum(1) == K] = False`, `attn |= padding`), two launches:
 *   out_feats[b,k,:] = feats[idx[b*K+k],:]   out_pos likewise (pos may be NULL)   f32, c and p multiples of 4
 *   out_mask[b,k,:]  = mask[idx[b*K+k],:] (bool bytes [n,q], q <= 256), then
 *     - a query column that is masked in ALL K gathered rows of its scene is cleared in the scene's real rows,
 *     - rows k >= n_valid[b] (padding; their idx repeats a real row) are fully masked.
 * n_valid: HOST array i32[n_scenes] (n_scenes <= 16).  ws: usc_sample_keys_ws_bytes().
 * Partial calls: feats == NULL with c == 0 gathers the mask rows only (the part of a pass's keys that depends on the
 * queries, :337-346); mask == NULL with q == 0 the feature / positional rows only (query-independent: a caller may
 * issue it ahead of the decoder loop on another stream; one launch, no ws). */
int64_t usc_sample_keys_ws_bytes(int32_t n_scenes, int32_t K, int32_t q);
int usc_sample_keys(const float* feats, int32_t c, const uint8_t* mask, int32_t q, const float* pos, int32_t p,
                    const int64_t* idx, int32_t n_scenes, int32_t K, const int32_t* n_valid, float* out_feats,
                    uint8_t* out_mask, float* out_pos, void* ws, int64_t ws_bytes, usc_stream_t s);

/* The attention-mask rows of one decoder pass for the SAMPLED keys only, straight from the [segments, q] logits: the
 * bytes that d calls of usc_avgpool_down2_ex (the last one with mask_out) followed by the mask-only usc_sample_keys
 * give, in one launch plus the all-masked-column launch of usc_sample_keys (skip_fix != 0: left out; the rows are
 * then the gathered bits with the padding rows masked).
 *   in      f32 logits, leading dimension ld (a multiple of 4, >= q; `in` 16-byte aligned); q % 4 == 0, q <= 128
 *   tabs    HOST array of d (1..4) device child tables i32[8, n_rows[j]], -1 where a child is absent: tabs[0] holds
 *           rows of `in` (point2segment folded into the finest map's k2/s2 child table), tabs[j] rows of table j-1
 *   idx     i64[n_scenes*K], batch-wide rows of table d-1; n_valid: HOST i32[n_scenes] (n_scenes <= 16), as for
 *           usc_sample_keys; ws: usc_attn_mask_rows_ws_bytes() (-1: sizes out of range), 4-byte aligned
 * Every mean is summed in child-slot order and rounded to f32 before its parent adds it, like the separate launches. */
int64_t usc_attn_mask_rows_ws_bytes(int32_t n_scenes, int32_t K, int32_t q, int32_t d);
int usc_attn_mask_rows(const float* in, int32_t ld, int32_t q, int32_t d, const int32_t* const* tabs,
                       const int64_t* n_rows, const int64_t* idx, int32_t n_scenes, int32_t K,
                       const int32_t* n_valid, uint8_t* out_mask, void* ws, int64_t ws_bytes, int32_t skip_fix,
                       usc_stream_t s);

/* ------------------------------------------------------------------------
 * Q3  segment mean — replaces torch_scatter.scatter_mean(src, index, dim=0)
 * (models/mask3d.py:12,223; trainer/trainer.py:449) forward + backward.
 * CSR built once per scene: order i64[n] rows sorted by segment (stable),
 * seg_off i64[S+1].
 * ---------------------------------------------------------------------- */
int64_t usc_segment_csr_ws_bytes(int64_t n, int64_t S);
int usc_segment_csr(const int64_t* seg, int64_t n, int64_t S, int64_t* order,
                    int64_t* seg_off, void* ws, int64_t ws_bytes,
                    usc_stream_t s);
int usc_segment_mean_fwd(const float* src, int32_t c, const int64_t* order,
                         const int64_t* seg_off, int64_t S, float* out,
                         usc_stream_t s);
/* dsrc[i,:] = dout[seg[i],:] / count[seg[i]] */
int usc_segment_mean_bwd(const float* dout, int32_t c, const int64_t* seg,
                         const int64_t* seg_off, int64_t n, float* dsrc,
                         usc_stream_t s);

/* Per-segment mean over the NON-ZERO feature rows of each segment (N1:
 * aggregate_features mode 'mean', pseudo_masks/unscene3d_pseudo_main.py:350-402):
 * out f32[S,d], nonzero_cnt i64[S] (may be NULL).  Uses the segment CSR. */
int usc_segment_mean_nonzero(const float* feats, int32_t d,
                             const int64_t* order, const int64_t* seg_off,
                             int64_t S, float* out, int64_t* nonzero_cnt,
                             usc_stream_t s);
/* Same with the per-channel MAX over the non-zero rows (aggregation_mode 'max',
 * unscene3d_pseudo_main.py:366: valid_segment_feats.max(0)[0]); segments without
 * a non-zero row give 0. */
int usc_segment_max_nonzero(const float* feats, int32_t d,
                            const int64_t* order, const int64_t* seg_off,
                            int64_t S, float* out, int64_t* nonzero_cnt,
                            usc_stream_t s);

/* Masked cross attention of the mask decoder, all heads at once:
 *   o = softmax(q k^T / sqrt(16) + mask) v   per (batch, head), head dim 16, L <= usc_attn_max_queries() = 256,
 * q, o f32[L,B,E], k, v f32[S,B,E] (sequence-first, E = 16*H), mask u8[B,S,L] (non-zero =
 * masked, shared by the heads).  No [heads, L, S] tensor is materialised: the forward is split
 * over keys (partial (o, max, sum) per split + a combine pass) and saves lse f32[B*H, usc_attn_lse_stride(L)]; the
 * backward recomputes the probabilities and reduces dq partials in a fixed order (no float atomics: two calls on
 * the same inputs give the same bits).
 * Queries come in groups of 128: L <= 128 runs the one-group kernels (4 mask words per key, lse stride 128);
 * 129 <= L <= 256 the two-group instantiations (8 mask words per key, lse stride 256, a query-group grid dimension
 * in the forward, all 8 query tiles walked per key chunk in the backward).  usc_attn_ws_bytes depends on L only
 * through the group count.
 * Replaces nn.MultiheadAttention's attention core in CrossAttentionLayer
 * (models/mask3d.py:547-605; memory_mask built at :341-348). */
int32_t usc_attn_max_queries(void);
/* row stride of lse for L queries (cross and self attention): 128 for L <= 128, 256 above */
int32_t usc_attn_lse_stride(int32_t L);
int64_t usc_attn_ws_bytes(int32_t L, int32_t S, int32_t B, int32_t H);
int usc_attn_fwd(const float* q, const float* k, const float* v,
                 const uint8_t* mask, int32_t L, int32_t S, int32_t B, int32_t H,
                 int32_t E, float* o, float* lse, void* ws, int64_t ws_bytes,
                 usc_stream_t s);
int usc_attn_bwd(const float* q, const float* k, const float* v,
                 const uint8_t* mask, const float* o, const float* lse,
                 const float* dO, int32_t L, int32_t S, int32_t B, int32_t H,
                 int32_t E, float* dq, float* dk, float* dv,
                 int32_t mask_bits_in_ws /* ws = the forward call's workspace, packed mask still at its start */,
                 void* ws, int64_t ws_bytes, usc_stream_t s);

/* Self attention of the decoder queries (S = L <= 256 keys, no mask, head dim 16): q, k, v, o, dO, dq, dk, dv
 * f32[L,B,E] sequence-first, lse f32[B*H, usc_attn_lse_stride(L)].  ONE launch each way (forward: one workgroup per
 * (batch, head), two above 128 queries; backward: per (batch, head) one workgroup per query tile for dq and one per
 * key chunk for dk / dv); no partial sum leaves a workgroup and every sum has a fixed order (bit-reproducible under
 * any load, no atomics).
 * Replaces nn.MultiheadAttention's attention core in SelfAttentionLayer (models/mask3d.py:491-545). */
int usc_self_attn_fwd(const float* q, const float* k, const float* v, int32_t L,
                      int32_t B, int32_t H, int32_t E, float* o, float* lse,
                      usc_stream_t s);
int usc_self_attn_bwd(const float* q, const float* k, const float* v, const float* o,
                      const float* lse, const float* dO, int32_t L, int32_t B,
                      int32_t H, int32_t E, float* dq, float* dk, float* dv,
                      usc_stream_t s);

/* Rectangular linear sum assignment (minimise) of n_prob independent cost matrices f32[n_prob, nr, nc], one wave per
 * problem, entirely on the device: row_ind / col_ind i64[n_prob, min(nr,nc)] (rows ascending, like scipy), status
 * i32[n_prob] (0 = solved; 1 = infeasible, i.e. infinite / NaN costs — the indices are then the identity).
 * The algorithm, its f64 dual updates and its tie-breaking are those of scipy.optimize.linear_sum_assignment
 * (rectangular_lsap: shortest augmenting paths), so equal costs give scipy's assignment.
 * Replaces `linear_sum_assignment(C.cpu())` of HungarianMatcher.memory_efficient_forward (models/matcher.py:150-168):
 * no device->host copy and no host solve in the middle of the training step. */
int usc_lsap_batch(const float* cost, int32_t n_prob, int32_t nr, int32_t nc,
                   int64_t* row_ind, int64_t* col_ind, int32_t* status, usc_stream_t s);

/* The set criterion on the device, per scene and for all L <= 16 prediction levels at once (reference
 * models/matcher.py:98-168 cost matrices; models/criterion.py:22-73, :138-216 losses, :194-200 DropLoss).  masks[l] /
 * dmasks[l]: the level's mask logits f32[S, ld] (Q <= ld <= 256 columns, any value; Q <= 256 queries: above 128 queries
 * or columns the launches take a second group of 128 columns, up to 128 they are what they always were) and their
 * gradient; logits: class
 * logits addressed as logits[l*ls_level + q*ls_q + c], c < C; labels i64[T] (253 = ignore).
 * max_targets, 32 .. 128 (anything else is an error), is the caller's bound on T: T outside 1 .. max_targets is
 * refused before anything is launched (SetCriterion passes its device_max_targets, 32 unless opted in).  The target
 * bits are W = ceil(T / 32) words per row, word-major: bits u32[W, S], word w = the targets 32w .. 32w+31; up to 32
 * targets that is u32[S].  usc_criterion_drop_counts and _losses need T <= Q for every T; _costs and _backward need it
 * only above 32 targets; _losses alone has no bound on L (its kernel takes no per-level pointer table).
 *   usc_criterion_target_bits  tm u8[T,S] -> bits (bit t of word w = row s belongs to target 32w + t), cnt i32[T] =
 *                              |tm[t]|
 *   usc_criterion_costs        cost = w_mask*BCE + w_class*(-p[label]) + w_dice*dice  f32[L,Q,T] (the LSAP input), its
 *                              parts cmask / cdice [L,Q,T], nmat [L,Q,T] = sum_s sigmoid(x) tm, ssum [L,Q] =
 *                              sum_s sigmoid(x), logp [L,Q,C] = log softmax (kept for the losses and the backward).
 *                              Once per word, one word after the other on the stream: word w fills the columns 32w ..
 *                              (2 W launches); the workspace of usc_criterion_ws_bytes_q(L, S, T, Q) is reused per word,
 *                              so above 32 targets it is the 32-target size.  It is strided by the column count: 128 up
 *                              to 128 queries (usc_criterion_ws_bytes(L, S, T), the same number), 256 above; ws_bytes
 *                              below the size for this call's Q is refused.  A pair's entries do not depend on the
 *                              scene's other targets or queries
 *   usc_criterion_drop_counts  DropLoss only, after usc_lsap_batch: counts i32[2,L,T] = per matched pair (row order of
 *                              src / tid) I = |pred & target| and F = |pred|, pred = (x > 0); integer sums, exact.
 *                              counts is zeroed here
 *   usc_criterion_losses       src/tid i64[L,T] (usc_lsap_batch) -> part f32[L,4] = (sum w*nll, sum w, mask loss, dice
 *                              loss) of this scene, tcls i32[L,Q] = target class per query (noobj = C-1 unmatched).
 *                              DropLoss (a matched pair whose prediction overlaps its target with IoU below thresh gets
 *                              weight 0 in the mask and dice loss; the divisor stays T): given counts, cnt and thresh it
 *                              writes wts f32[L,T] = 1 if U > 0 and f32(I) / f32(U) >= thresh else 0, U = F + cnt - I,
 *                              and applies them inside the same fixed-order sums.  counts = cnt = wts = NULL: no DropLoss
 *   usc_criterion_table        parts [B,L,4] of the batch's scenes -> table [L,4] = (loss_ce, loss_mask, loss_dice, 0),
 *                              den_tot [L]
 *   usc_criterion_backward     gtable = d total / d table [L,4] -> dmasks (full padded width, zero outside the matched
 *                              columns) and dlogits (same addressing as logits).  wts (usc_criterion_losses): the
 *                              column of a pair with weight 0 is exactly 0.  wts = NULL: no DropLoss
 * Fixed summation order everywhere.  Replaces the torch op chains of HungarianMatcher.memory_efficient_forward and
 * SetCriterion.loss_labels / loss_masks, with DropLoss `(fg * tm).sum(1) / (fg + tm).sum(1) >= thresh` on the gathered
 * [T, S] masks, and above 32 targets the operator path's device->host copy and scipy solve per level and scene. */
int64_t usc_criterion_ws_bytes(int32_t L, int32_t S, int32_t T);
int64_t usc_criterion_ws_bytes_q(int32_t L, int32_t S, int32_t T, int32_t Q);
int usc_criterion_target_bits(const uint8_t* tm, int32_t T, int32_t max_targets, int32_t S,
                              uint32_t* bits, int32_t* cnt, usc_stream_t s);
int usc_criterion_costs(const float* const* masks, int32_t L, int32_t ld, int32_t S,
                        int32_t Q, int32_t T, int32_t max_targets, const uint32_t* bits,
                        const int32_t* cnt, const float* logits, int64_t ls_level, int64_t ls_q,
                        int32_t C, const int64_t* labels, float w_mask, float w_class,
                        float w_dice, float* cost, float* cmask, float* cdice, float* nmat,
                        float* ssum, float* logp, void* ws, int64_t ws_bytes, usc_stream_t s);
int usc_criterion_drop_counts(const float* const* masks, int32_t L, int32_t ld, int32_t S,
                              int32_t Q, int32_t T, int32_t max_targets, const uint32_t* bits,
                              const int64_t* src, const int64_t* tid, int32_t* counts,
                              usc_stream_t s);
int usc_criterion_losses(const float* cmask, const float* cdice, const float* logp,
                         const int64_t* src, const int64_t* tid, const int64_t* labels,
                         const float* class_w, int32_t L, int32_t Q, int32_t T,
                         int32_t max_targets, int32_t C, int32_t noobj, int32_t* tcls, float* part,
                         const int32_t* counts, const int32_t* cnt, float thresh, float* wts,
                         usc_stream_t s);
int usc_criterion_table(const float* parts, int32_t B, int32_t L, float* table,
                        float* den_tot, usc_stream_t s);
int usc_criterion_backward(const float* const* masks, float* const* dmasks, int32_t L,
                           int32_t ld, int32_t S, int32_t Q, int32_t T, int32_t max_targets,
                           const uint32_t* bits, const int32_t* cnt, const int64_t* src,
                           const int64_t* tid, const float* nmat, const float* ssum,
                           const float* logp, const int32_t* tcls, const float* class_w,
                           const float* gtable, const float* den_tot, int32_t C, int64_t ls_level,
                           int64_t ls_q, float* dlogits, const float* wts, usc_stream_t s);

/* Linear layer on a handful of rows (the 100 decoder queries):
 *   y[M,N] = x[M,K] W[N,K]^T + b[N]   (b may be NULL);  N, K multiples of 32.
 * usc_linear_bwd: dx[M,K] = dy W, dW[N,K] = dy^T x, db[N] = column sums of dy; each
 * of dx / dW may be NULL to skip it (db is produced inside the dW tiles: db
 * without dW is refused); accumulate=1 adds dW / db into the given buffers
 * (parameter gradients).  One workgroup per 32x32 output tile on the f32 matrix
 * cores; the forward is one launch, both gradients together are one launch.
 * Replaces nn.Linear / the nn.MultiheadAttention projections of the mask decoder
 * (models/mask3d.py:491-651 attention layers and FFN, :70-72 mask_embed_head). */
int usc_linear_fwd(const float* x, const float* W, const float* b, int32_t M,
                   int32_t N, int32_t K, float* y, usc_stream_t s);
int usc_linear_bwd(const float* dy, const float* x, const float* W, int32_t M,
                   int32_t N, int32_t K, float* dx, float* dW, float* db,
                   int32_t accumulate, usc_stream_t s);
/* The same two launches with what surrounds the layer in the decoder folded in
 * (every extra pointer optional):
 *   x2      the layer's input is x + x2 (query / key positional encodings,
 *           models/mask3d.py:485,517) — forward and weight gradient;
 *   relu    y = max(y, 0) (FFN activation, :542); y_relu = that output: the
 *           gradients count dy only where it is > 0;
 *   dx_add  [M,K] added to dx (a second gradient path into the same input). */
int usc_linear_fwd_ex(const float* x, const float* x2, const float* W,
                      const float* b, int32_t M, int32_t N, int32_t K,
                      int32_t relu, float* y, usc_stream_t s);
/* ... writing y as an [M_pad, N] table whose rows M..M_pad-1 are zero: the 100 query embeddings of the mask module
 * (models/mask3d.py:425) zero-extended to the 128 rows the following product's kernels want, in the producing launch
 * (was: a fill and a copy per call, and a slice copy on the way back). */
int usc_linear_fwd_pad(const float* x, const float* x2, const float* W, const float* b, int32_t M, int32_t N, int32_t K,
                       int32_t relu, float* y, int32_t M_pad, usc_stream_t s);
/* ... several projections of ONE input in one launch: W [N,K] is a stack of N/split_cols weight matrices (the packed
 * in_proj_weight of nn.MultiheadAttention), y comes back as [N/split_cols][M][split_cols] (each projection its own
 * contiguous matrix) and the positional term x2 enters the output columns < x2_cols only — the q, k, v of a
 * self-attention block (models/mask3d.py:507-517: q = k = tgt + query_pos, v = tgt), three launches before. */
int usc_linear_fwd_split(const float* x, const float* x2, const float* W, const float* b, int32_t M, int32_t N, int32_t K,
                         int32_t x2_cols, int32_t split_cols, float* y, usc_stream_t s);
int usc_linear_bwd_ex(const float* dy, const float* y_relu, const float* x,
                      const float* x2, const float* W, int32_t M, int32_t N,
                      int32_t K, float* dx, const float* dx_add, float* dW,
                      float* db, int32_t accumulate, usc_stream_t s);
/* ... and with a second addend and a second output: dx = dy W + dx_add + dx_add2, dx_b = dy W + dx_add (each optional).
 * One product feeding two gradients — the layer input's, which also collects a residual path (dx_add2), and the
 * positional term's, which does not (models/mask3d.py:485-494: `tgt + pos` into the projection, `tgt` into the
 * residual) — without an extra add launch. */
int usc_linear_bwd_ex2(const float* dy, const float* y_relu, const float* x, const float* x2, const float* W, int32_t M,
                       int32_t N, int32_t K, float* dx, const float* dx_add, const float* dx_add2, float* dx_b, float* dW,
                       float* db, int32_t accumulate, usc_stream_t s);
/* The input gradient of L <= usc_linear_heads_max() linear heads over ONE input in one launch:
 *   dx[M,K] = P_0 + (P_1 + ( ... + P_{L-1})),  P_l = dy[l] [M,N] W[l] [N,K]   (dy, W: host arrays of L device pointers)
 * — the 13 mask-logit products of a training step over the segment table (models/mask3d.py:425,430).  The bits of the
 * chain usc_linear_bwd_ex(dy[l], ..., dx_add = the sum so far), last head first. */
int32_t usc_linear_heads_max(void);
int usc_linear_heads_dx(const float* const* dy, const float* const* W, int32_t L, int32_t M, int32_t N, int32_t K, float* dx,
                        usc_stream_t s);
/* Backward of usc_linear_fwd_split for the self-attention projections (split_cols = E, N = 3E, x2_cols = 2E), one launch:
 * dy3 [3][M][E] = dq | dk | dv;  dx = dq Wq + dk Wk + dv Wv (+ dres: the block's residual path);  dx_b (optional) =
 * dq Wq + dk Wk, the positional term's gradient;  dW [3E][E] and db [3E] written or (accumulate) added to, with the
 * positional term in the q and k rows only. */
int usc_qkv_proj_bwd(const float* dy3, const float* x, const float* pos, const float* W, int32_t M, int32_t E, float* dx,
                     float* dx_b, const float* dres, float* dW, float* db, int32_t accumulate, usc_stream_t s);
/* out[c] (+)= sum over the n rows of x f32[n, c]: the bias gradient of a linear
 * layer over many rows (the 3 200 / 12 800 sampled voxels of a decoder pass,
 * models/mask3d.py:351-352 lin_squeeze and the key / value projections of
 * :547-605).  Fixed summation order (64-row partials, then 16 interleaved ascending chains): the same
 * bits on every launch, also when replayed from a captured graph.
 * ws: usc_col_sum_ws_bytes(n, c). */
int64_t usc_col_sum_ws_bytes(int64_t n, int32_t c);
int usc_col_sum(const float* x, int64_t n, int32_t c, float* out,
                int32_t accumulate, void* ws, int64_t ws_bytes, usc_stream_t s);

/* LayerNorm over the last dimension of x f32[rows, d] (d in 64*{1,2,3,4,6,8}):
 *   y = (x - mean) * rstd * gamma + beta,  rstd = 1/sqrt(var + eps)  (biased var);
 * mean/rstd f32[rows] are saved for the backward, which is ONE launch for
 * rows <= 1024 (dx, dgamma, dbeta; column sums reduced in a fixed wave order;
 * accumulate=1 adds dgamma / dbeta into the given buffers).
 * Replaces nn.LayerNorm of the mask decoder (models/mask3d.py:174 decoder_norm,
 * :515/:572/:627 post-norms of SelfAttentionLayer / CrossAttentionLayer / FFNLayer). */
int usc_layernorm_fwd(const float* x, const float* gamma, const float* beta,
                      int64_t rows, int32_t d, float eps, float* y, float* mean,
                      float* rstd, usc_stream_t s);
/* y = LayerNorm(x + res): the post-norm residual of the decoder layers
 * (models/mask3d.py:523-524, 493-494, 543-544) in the same launch; the sum is
 * written to sum_out f32[rows, d], which the backward takes as its `x`. */
int usc_add_layernorm_fwd(const float* x, const float* res, const float* gamma,
                          const float* beta, int64_t rows, int32_t d, float eps,
                          float* y, float* sum_out, float* mean, float* rstd,
                          usc_stream_t s);
int64_t usc_layernorm_bwd_ws_bytes(int64_t rows, int32_t d);
int usc_layernorm_bwd(const float* dy, const float* x, const float* mean,
                      const float* rstd, const float* gamma, int64_t rows,
                      int32_t d, float* dx, float* dgamma, float* dbeta,
                      int32_t accumulate, void* ws, int64_t ws_bytes,
                      usc_stream_t s);
/* The same with dx = (LayerNorm's input gradient) + dx_add (f32[rows, d] or NULL): the gradient that reaches x AROUND
 * the norm — `queries` feed `decoder_norm` inside mask_module AND the next decoder layer (models/mask3d.py:356-373,
 * :410) — summed in this launch instead of by an autograd add. */
int usc_layernorm_bwd_ex(const float* dy, const float* x, const float* mean,
                         const float* rstd, const float* gamma, int64_t rows,
                         int32_t d, const float* dx_add, float* dx, float* dgamma,
                         float* dbeta, int32_t accumulate, void* ws,
                         int64_t ws_bytes, usc_stream_t s);

/* ------------------------------------------------------------------------
 * Q1  furthest point sampling — replaces pointnet2._ext.furthest_point_sampling
 * (third_party/pointnet2/_ext_src/src/sampling.cpp:67-88,
 *  sampling_gpu.cu:73-232; called from models/mask3d.py:228).
 * xyz f32[b,n,3], tmp f32[b,n] pre-filled with 1e10, idx i32[b,m].
 * Bit-exact with the reference kernel's result incl. its tie-break
 * (winner = tied k with smallest (k mod 512), then smallest k, for n>=512)
 * and its |p|^2 <= 1e-3 skip.
 * ---------------------------------------------------------------------- */
int usc_furthest_point_sampling(const float* xyz, int32_t b, int32_t n,
                                int32_t m, float* tmp, int32_t* idx,
                                usc_stream_t s);

/* ------------------------------------------------------------------------
 * Q2  Fourier positional encoding — replaces
 * PositionEmbeddingCoordsSine.get_fourier_embeddings
 * (models/position_embedding.py:128-157) with normalize=True
 * (shift_scale_points :12-40, dst_range [0,1]):
 *   out[i, :] = [sin(2*pi*xn@B) | cos(2*pi*xn@B)],  xn=(x-lo)/(hi-lo)
 * xyz f32[n,3], lo/hi f32[3], gauss_B f32[3,d/2], out f32[n,d] (row-major).
 * ---------------------------------------------------------------------- */
int usc_fourier_posenc(const float* xyz, int64_t n, const float* lo,
                       const float* hi, const float* gauss_B, int32_t d,
                       float* out, usc_stream_t s);

/* ------------------------------------------------------------------------
 * N2-N4  normalized-cut pseudo masks — replaces the numpy/scipy functions of
 * pseudo_masks/unscene3d_pseudo_main.py:82-153 (normalize_mat,
 * get_affinity_matrix, second_smallest_eigenvector) and cosine_sim
 * (utils/freemask_utils.py:8-18).
 * ---------------------------------------------------------------------- */
/* normed f32[S,d] = F.normalize(F) (cosine_mode=1: divided once more by ||.||+1e-9);
 * sim f32[S,S] = normed normed^T; cosine_mode=1 also applies cosine_sim's per-row
 * min-max (attn -= rowmin; attn /= rowmax + 1e-9). */
int usc_ncut_similarity(const float* F, int64_t S, int32_t d,
                        int32_t cosine_mode, float* normed, float* sim,
                        usc_stream_t s);
/* The same over F with the rows flagged in zero_rows (u8[S] or NULL) multiplied by 0 first: the features
 * get_masked_affinity_matrix (unscene3d_pseudo_main.py:122-135) hands to the next iteration are
 * `(1 - painting) * feats`, painting only grows, so iteration i sees the ORIGINAL features with the rows painted so
 * far zeroed — formed inside the row normalisation instead of by four element-wise passes per iteration. */
int usc_ncut_similarity_masked(const float* F, const uint8_t* zero_rows, int64_t S,
                               int32_t d, int32_t cosine_mode, float* normed,
                               float* sim, usc_stream_t s);
/* In-place normalize_mat: A -= min(A[A != 0]) if any(A > 0); A[A < 0] = 0;
 * A /= max(A) + 1e-5.  ws >= 12288 bytes. */
int usc_ncut_normalize_mat(float* A, int64_t S, void* ws, int64_t ws_bytes,
                           usc_stream_t s);
/* Abin u8[S,S] = ((simA [+ simB]) / (1|2)) > tau with painted rows/columns forced
 * off (unscene3d_pseudo_main.py:426-427); deg f64[S] = column sums of
 * (A ? 1 : eps) BEFORE the painting overwrite (:111-118).  simB, painted may be NULL. */
int usc_ncut_binarize(const float* simA, const float* simB, int64_t S, float tau,
                      double eps, const uint8_t* painted, uint8_t* Abin,
                      double* deg, usc_stream_t s);
/* Eigenvector #2 (second smallest eigenvalue) of (D - A) v = lambda D v, i.e.
 * scipy.linalg.eigh(D - A, D, subset_by_index=[1, 2])[1][:, 0], fp64, with LAPACK's
 * sign (dsygvx sequence restated: lower triangle, dsytrd 'L' reflectors, dstein
 * normalisation).  A = Abin ? 1 : eps.  evec f64[S], eval f64[2] = (lambda_1, lambda_2). */
int64_t usc_ncut_fiedler_ws_bytes(int64_t S);
int usc_ncut_fiedler(const uint8_t* Abin, const double* deg, int64_t S, double eps,
                     double* evec, double* eval, void* ws, int64_t ws_bytes,
                     usc_stream_t s);
/* The same; flags bit 0 forces the stepwise tridiagonalisation (as USC3D_TRI_STEPWISE=1 does). */
int usc_ncut_fiedler_ex(const uint8_t* Abin, const double* deg, int64_t S, double eps,
                        double* evec, double* eval, void* ws, int64_t ws_bytes,
                        usc_stream_t s, int32_t flags);
/* The kernels usc_ncut_fiedler_ex launches for S segments on a device with `cus`
 * compute units (host only, no HIP call; -1 unless 3 <= S <= 8000):
 *   bits 0-3   tridiagonalisation: 0 stepwise (tri_reflect_symv + tri_update per
 *              step), one launch with the rows in 1 registers <10,3>, 2 registers
 *              <16,4>, 3 LDS, 4 global memory
 *   bit  4     tri_eig_kernel works in LDS (else in global memory)
 *   bits 8-11  back-transformation: 0 tri_backtransform_kernel (1024 threads),
 *              1-3 tri_backtransform_quad_kernel<2,3,4>, 4-7 the one-wave
 *              tri_backtransform_wave_kernel<4,8,11,16> (USC3D_BACKTRANSFORM_QUAD=0)
 * USC3D_TRI_STEPWISE and USC3D_BACKTRANSFORM_{QUAD,WAVE} are honoured as in the launch.
 * The launch still falls back to stepwise if the kernel cannot get its LDS. */
int32_t usc_ncut_fiedler_plan(int64_t S, int32_t cus, int32_t flags);

/* ------------------------------------------------------------------------
 * N6  exact 1-nearest-neighbour — replaces scipy.spatial.KDTree.query(k=1)
 * (pseudo_masks/unscene3d_pseudo_main.py:341-343, :651-652).  f64 distances on
 * f32 inputs; ties resolve to the lowest reference index.
 * query f32[nq,3], ref f32[nr,3] -> idx i64[nq], dist2 f32[nq] (may be NULL).
 * ---------------------------------------------------------------------- */
int usc_knn1(const float* query, int64_t nq, const float* ref, int64_t nr,
             int64_t* idx, float* dist2, usc_stream_t s);

/* ------------------------------------------------------------------------
 * N6b the same search through a uniform grid — scipy.spatial.KDTree(ref)
 * .query(query, k=1) of pseudo_masks/unscene3d_pseudo_main.py:339-343 in O(N)
 * (csrc/knn.hip).  Returns exactly what usc_knn1 returns: f64 distances on the
 * f32 inputs, the lowest reference index among equidistant points, dist2 the
 * same f32 bits.  Inputs are finite.
 * The grid is the caller's: origin f64[3], cell > 0 and dims i32[3] are HOST
 * values (cell (i,j,k) covers origin + (i..i+1, j..j+1, k..k+1) * cell; at most
 * 2^27 cells, 1 <= nr < 2^31).  Any grid gives the right answer — points and
 * queries outside it are clamped into its boundary cells — a grid that fits
 * the reference points with a few points per occupied cell gives it fast.
 * Reference points are binned (histogram, scan, scatter in ascending index per
 * cell); a query searches cubes of cells of Chebyshev radius 1, 2, .. 4 around
 * its cell until its best distance is strictly below the distance of the
 * nearest wall of the cube (less a rounding allowance), else streams all
 * reference points like usc_knn1.  ws holds usc_knn1_grid_ws_bytes(nr, dims)
 * bytes (-1 for sizes out of range); nq = 0 bins the points and searches
 * nothing.  No allocation, no host synchronisation.
 * ---------------------------------------------------------------------- */
int64_t usc_knn1_grid_ws_bytes(int64_t nr, const int32_t* dims);
int usc_knn1_grid(const float* query, int64_t nq, const float* ref, int64_t nr,
                  const double* origin, double cell, const int32_t* dims,
                  int64_t* idx, float* dist2, void* ws, int64_t ws_bytes,
                  usc_stream_t s);

/* ------------------------------------------------------------------------
 * N6c normals estimated from a point cloud — replaces open3d's
 * pcd.estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))
 * (datasets/preprocessing/arkit_preprocessing.py:98-101) (csrc/normals.hip).
 *
 * usc_knn_hybrid_grid: the k nearest reference points inside a radius.
 * query f32[nq,3], ref f32[nr,3] -> idx i32[nq,k], count i32[nq].  The
 * candidates of a query are the reference points with d2 < r2, STRICTLY, where
 * d2 is usc_knn1's expression (f64 on the f32 inputs, x, y, z in that order)
 * and r2 = (double)radius * radius.  They are ordered by (d2, index) ascending;
 * the first count = min(k, candidates) indices are written, the rest of the
 * row is -1.  1 <= k <= 64; radius is finite and > 0; anything else, or a
 * workspace shorter than usc_knn_hybrid_grid_ws_bytes(nr, dims), is refused
 * before any launch with nothing written.  origin, cell, dims: the caller's
 * grid, with usc_knn1_grid's rules — any grid gives the right answer, points
 * and queries are clamped into it; cell = radius makes a query read at most
 * 27 cells; a query whose ball reaches more than 4 cells from its own cell
 * along an axis reads every reference point.  nq = 0 bins the points only.
 * UNPINNED: the strict `<` is this library's reading of open3d's SearchHybrid.
 *
 * usc_normals_pca: per query, with m = count and x_j = ref[idx_j] - query
 * (exact in f64): mean and centred second moments of the x_j summed in f64 in
 * list order and divided by m; normals f32[nq,3] = the unit eigenvector of the
 * smallest eigenvalue (cyclic Jacobi in f64, fixed sweeps), rounded to f32.
 * m < 3, a zero or non-finite covariance or vector, or an index outside
 * [0, nr) gives (0, 0, 1).  Sign: of the stored f32 components the one of
 * largest magnitude (the lowest axis among equals) is >= 0.  UNPINNED:
 * open3d's sign is a by-product of its eigen routine.
 * Both: explicit stream, no allocation, no host synchronisation, no float
 * atomics; two calls write the same bytes.
 * ---------------------------------------------------------------------- */
int64_t usc_knn_hybrid_grid_ws_bytes(int64_t nr, const int32_t* dims);
int usc_knn_hybrid_grid(const float* query, int64_t nq, const float* ref,
                        int64_t nr, float radius, int32_t k,
                        const double* origin, double cell, const int32_t* dims,
                        int32_t* idx, int32_t* count, void* ws,
                        int64_t ws_bytes, usc_stream_t s);
int usc_normals_pca(const float* query, int64_t nq, const float* ref,
                    int64_t nr, const int32_t* idx, const int32_t* count,
                    int32_t k, float* normals, usc_stream_t s);

/* ------------------------------------------------------------------------
 * E1  eps-ball connected components — replaces
 * sklearn.cluster.DBSCAN(eps, min_samples=1).fit(xyz).labels_
 * (trainer/trainer.py:521-523): min-label propagation with pointer jumping; the
 * caller iterates usc_cc_eps_step (ping-pong label buffers) until `changed`
 * (i32[1], device) reads 0, then usc_cc_eps_finish numbers the components in
 * first-seen order (labels i64[n]).  xyz f32[n,3].
 * ---------------------------------------------------------------------- */
int usc_cc_eps_init(int32_t* label, int64_t n, usc_stream_t s);
int usc_cc_eps_step(const float* xyz, int64_t n, float eps,
                    const int32_t* label_in, int32_t* label_out,
                    int32_t* changed, usc_stream_t s);
int usc_cc_eps_finish(const int32_t* label, int64_t n, int32_t* rank_ws,
                      int64_t* labels, usc_stream_t s);

/* ------------------------------------------------------------------------
 * E1b DBSCAN of all query masks of one scene in one pass — replaces the loop
 * over queries around sklearn.cluster.DBSCAN(eps, min_samples).fit(xyz[on])
 * of trainer/trainer.py:517-533, for any min_samples >= 1 (csrc/dbscan.hip).
 * Points are binned into cells of side eps / 2; the caller sorts them by cell
 * key between the calls (ops.dbscan_masks):
 *   usc_dbscan_cell_keys      replaces nothing in the reference (binning):
 *       xyz f32[n,3] -> keys i64[n] = (cx*ny + cy)*nz + cz,
 *       c = floor((x - min) / (eps/2)) in f64; nx, ny, nz <= 2^20.
 *   usc_dbscan_neighbor_table cell_keys i64[n_cells] ascending and distinct ->
 *       nbr i32[n_cells,125]: the occupied cell at offset (k/25-2, k/5%5-2,
 *       k%5-2), or -1.
 *   usc_dbscan_labels         replaces sklearn.cluster.DBSCAN(...).labels_ per
 *       query (trainer.py:521-523): xyz_sorted f32[n,3] and order i64[n] (sorted
 *       position -> original row, ascending inside a cell), cell_of i32[n],
 *       cell_start i32[n_cells+1], masks f32[n,q] in ORIGINAL row order (on:
 *       > 0) -> labels i32[n,q] in original row order (sklearn's label on an
 *       on-point, -1 noise, -2 off) and n_clusters i32[q].  Distances as in
 *       usc_cc_eps_step: f64 on the f32 coordinates against
 *       (double)eps*(double)eps.  ws: usc_dbscan_ws_bytes bytes.
 *   usc_dbscan_expand         replaces the per-cluster mask products of
 *       trainer.py:525-533: out f32[n,n_cols] (zeroed by the caller),
 *       out[i, col_start[q] + labels[i,q]] = masks[i,q] where the label >= 0.
 * ---------------------------------------------------------------------- */
#define USC_DBSCAN_MAX_CELLS_PER_AXIS (1 << 20)
int usc_dbscan_cell_keys(const float* xyz, int64_t n, float eps, double min_x,
                         double min_y, double min_z, int32_t nx, int32_t ny,
                         int32_t nz, int64_t* keys, usc_stream_t s);
int usc_dbscan_neighbor_table(const int64_t* cell_keys, int64_t n_cells,
                              int32_t nx, int32_t ny, int32_t nz, int32_t* nbr,
                              usc_stream_t s);
int64_t usc_dbscan_ws_bytes(int64_t n, int32_t q, int64_t n_cells,
                            int32_t min_samples);
int usc_dbscan_labels(const float* xyz_sorted, const int64_t* order,
                      const int32_t* cell_of, const int32_t* cell_start,
                      const int32_t* nbr, const float* masks, int64_t n,
                      int32_t q, int64_t n_cells, float eps,
                      int32_t min_samples, void* ws, int64_t ws_bytes,
                      int32_t* labels, int32_t* n_clusters, usc_stream_t s);
int usc_dbscan_expand(const float* masks, const int32_t* labels,
                      const int64_t* col_start, int64_t n, int32_t q,
                      int64_t n_cols, float* out, usc_stream_t s);

/* ------------------------------------------------------------------------
 * L3  tri-plane projection — replaces
 * custom_cuda_utils.project_sparse_voxels_to_planes{,_backward}
 * (utils/cuda_utils/cuda_utils.cpp:26-46, cuda_utils_kernel.cu:371-603; wrapper
 * models/noise_robust_loss.py:16-71).  In-place accumulation into caller-zeroed
 * outputs, like the reference; voxels outside [0,dim) are dropped like there.
 * coords i32[V,4] (b,x,y,z) shifted to >= 0, pred/target f32[V,inst];
 * planes f32[dim_a,dim_b,inst], counts i32[dim_a,dim_b].
 * Backward: grad_pred[v,p] = mean of the non-zero among the three plane grads.
 * ---------------------------------------------------------------------- */
int usc_project_planes_fwd(const int32_t* coords, const float* pred,
                           const float* target, int64_t V, int32_t inst,
                           int32_t dim_x, int32_t dim_y, int32_t dim_z,
                           float* pred_xy, float* pred_xz, float* pred_yz,
                           float* tgt_xy, float* tgt_xz, float* tgt_yz,
                           int32_t* cnt_xy, int32_t* cnt_xz, int32_t* cnt_yz,
                           usc_stream_t s);
int usc_project_planes_bwd(const int32_t* coords, int64_t V, int32_t inst,
                           int32_t dim_x, int32_t dim_y, int32_t dim_z,
                           const float* g_xy, const float* g_xz,
                           const float* g_yz, float* grad_pred,
                           usc_stream_t s);

/* ------------------------------------------------------------------------
 * F1  2D -> 3D feature projection — replaces [CUDA ext] project_features_cuda.project_features_cuda
 * and project_features_cuda.unproject_depth_images (utils/cuda_utils/project_image_cuda.cpp:10-31,
 * project_image_cuda_kernel.cu:24-146,190-290; wrapper utils/cuda_utils/raycast_image.py:18-77; caller
 * pseudo_masks/unscene3d_pseudo_main.py:287-330).
 * views f32[B,V,4,4] row-major camera-to-grid matrices in voxel units (already shifted by the per-batch
 * minimum like the wrapper does), intrinsics f32[B,4] = fx, fy, mx, my.
 * Every pixel (b,v,y,x) marches  t = t0, t0+inc, ...  (sequential fp32 accumulation, like the reference)
 * and reports the row of the first occupied voxel at round-half-away(cam + t*dir):
 *   hit i32[B,V,H,W]   row, -1 = none.  Row 0 never hits (the reference's grid stores 0 for "empty").
 *   seg i64[B,V,H,W]   optional: row, or n_rows for a miss — the segment ids usc_segment_csr takes.
 * _map: the occupancy is the coordinate hash of usc_coordmap_build (tensor stride 1); shift i32[B,3] is
 *       the per-batch minimum coordinate (grid voxel + shift = map coordinate).
 * _dense: occupancy i64[B,dim_z,dim_y,dim_x] exactly as the reference builds it (0 = empty).
 * ---------------------------------------------------------------------- */
/* Optional free-space filter of the _map ray cast: one bit per 8x8x8-voxel brick of the (shifted) grid,
 * set where a voxel row > 0 lives; mask u32[B, ceil(bricks_x*bricks_y*bricks_z / 32)] (zeroed here),
 * brick index = (gz*bricks_y + gy)*bricks_x + gx.  coords i32[n,4] are the map's coordinates. */
int usc_brick_mask_build(const int32_t* coords, int64_t n, const int32_t* shift, int32_t B,
                         int32_t bricks_x, int32_t bricks_y, int32_t bricks_z,
                         uint32_t* mask, usc_stream_t s);
int usc_raycast_first_hit_map(const uint64_t* table_keys, const int32_t* table_vals,
                              int64_t cap, int64_t n_rows, const int32_t* shift,
                              const uint32_t* brick_mask /* may be NULL */, int32_t bricks_x,
                              int32_t bricks_y, int32_t bricks_z,
                              const float* views, const float* intrinsics,
                              int32_t B, int32_t V, int32_t H, int32_t W,
                              float depth_min, float depth_max, float ray_increment,
                              int32_t* hit, int64_t* seg, usc_stream_t s);
int usc_raycast_first_hit_dense(const int64_t* occupancy, int32_t dim_z, int32_t dim_y,
                                int32_t dim_x, int64_t n_rows, const float* views,
                                const float* intrinsics, int32_t B, int32_t V,
                                int32_t H, int32_t W, float depth_min, float depth_max,
                                float ray_increment, int32_t* hit, int64_t* seg,
                                usc_stream_t s);
/* Per-voxel reduction of the hit pixels' features over the CSR (order, seg_off) that
 * usc_segment_csr built from `seg` with n_rows+1 segments; feats f32[n_pix,c]; sums run in
 * ascending pixel order (deterministic; the reference's float atomics are unordered).
 *   mode 0: out f32[n_rows,c] = sum / (count + 10e-5) on every row (0 where nothing hit);
 *           num i32[n_rows] = count                                  (raycast_image.py:66-68)
 *   mode 1: out is the scene feature table: out[r] = (out[r] + sum/(count+10e-5)) / 2 on the rows
 *           that were hit only; num = count     (unscene3d_pseudo_main.py:311-313, :327-328)
 *   mode 2: out[r] += sum, num[r] += count — the operator's own in-place accumulation
 *           (project_image_cuda_kernel.cu:49,61-64)
 *   num may be NULL. */
int usc_project_reduce(const float* feats, int32_t c, const int64_t* order,
                       const int64_t* seg_off, int64_t n_rows, int32_t mode,
                       float* out, int32_t* num, usc_stream_t s);
/* Mode 1 of usc_project_reduce for V frames in one launch, reading the image encoder's token grids instead
 * of their resized maps (models/encoders_2d/dino.py:53-60 resizes every grid to [H,W,c] with
 * F.interpolate(size=(H,W), mode='bilinear'); pseudo_masks/unscene3d_pseudo_main.py:303-313 then folds one
 * frame at a time).  tokens f32[V,gh,gw,c], 1 <= c <= 512; (order, seg_off) is the CSR usc_segment_csr
 * built over n_rows+1 segments from the `seg` of ONE ray cast over the same V views (B = 1), so the pixel
 * index is (v*H + y)*W + x and every row's list is grouped by frame, in frame order.  Per row r and per
 * frame f that hits it, in ascending f:
 *   m_f = (sum over the frame's pixels, in list order, of bilinear(tokens[f], y, x)) / (count_f + 10e-5)
 *   scene[r] = (scene[r] + m_f) / 2
 * bilinear, in f32 with separately rounded operations (half-pixel centres, as torch computes it):
 *   src = (gh / H) * (y + 0.5) - 0.5, clamped at 0 from below; y0 = (int)src; lambda = src - y0;
 *   second tap y0 + (y0 < gh - 1); the same in x;
 *   val = (1-ly) * ((1-lx)*t00 + lx*t01) + ly * ((1-lx)*t10 + lx*t11).
 * Rows no frame hits are not written.  frames_hit i32[n_rows] (may be NULL) = number of frames of this call
 * that hit the row.  No atomics: the result does not depend on how frames are grouped into calls. */
int usc_project_fuse_tokens(const float* tokens, int32_t V, int32_t gh, int32_t gw,
                            int32_t c, int32_t H, int32_t W, const int64_t* order,
                            const int64_t* seg_off, int64_t n_rows, float* scene,
                            int32_t* frames_hit, usc_stream_t s);
/* Prediction mode (project_image_cuda_kernel.cu:68-109): out i32[n_rows,c] (caller-initialised to the
 * ignore label) = max(out, preds of the pixels that hit the row); preds i32[n_pix,c]. */
int usc_project_predictions(const int32_t* preds, int32_t c, const int32_t* hit,
                            int64_t n_pix, int32_t* out, usc_stream_t s);
/* depth f32[V,H,W], views f32[V,4,4], intrinsics f32[V,4] -> cloud f32[V*H*W,5] = (view, pixel index,
 * x, y, z) for depth > 0; other rows are left as the caller initialised them
 * (project_image_cuda_kernel.cu:249-290). */
int usc_unproject_depth(const float* depth, const float* views, const float* intrinsics,
                        int32_t V, int32_t H, int32_t W, float* cloud, usc_stream_t s);

/* ------------------------------------------------------------------------
 * T  optimizer step — torch.optim.AdamW(lr, betas, eps, weight_decay) of
 * `configure_optimizers` (trainer/trainer.py:953-966) over FLAT f32 buffers of n elements
 * (16-byte aligned): p *= 1 - lr*wd; m = lerp(m, g, 1-b1); v = b2 v + (1-b2) g^2;
 * p -= (lr / (1 - b1^step)) * m / (sqrt(v) / sqrt(1 - b2^step) + eps).  step counts from 1.
 * ---------------------------------------------------------------------- */
/* Diagnostic, no reference counterpart: `wgs` workgroups that spin for `microseconds` on stream s.  HIP multiplexes its
 * streams onto a few hardware queues (4 per priority by default), and two streams that share one do not overlap however
 * independent their work is: unscene3d_amd/streams.py times pairs of these launches to pick streams that really run
 * beside the compute stream. */
int usc_spin(int64_t microseconds, int wgs, usc_stream_t s);

int usc_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                   int64_t n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int64_t step, usc_stream_t s);

/* The same step on the data-parallel SUM of the gradients: g = grad[i] * grad_scale, then usc_adamw_step's
 * arithmetic.  grad_scale = 1.0f / (float)world (the division done once, in f32) reproduces torch's
 * `flat.div_(world)` bit for bit: for a host scalar divisor torch multiplies by the f32 reciprocal — exact for a
 * power of two, one rounding of 1/world otherwise (world 3: grad * 0x1.555556p-2f, not grad / 3.0f).
 * write_back_grad != 0 stores g back (grad holds the mean afterwards; 32 B per parameter), 0 leaves the sum
 * (28 B per parameter, and no averaging pass over the buffer before it). */
int usc_adamw_step_scaled(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                          float grad_scale, int32_t write_back_grad,
                          float lr, float beta1, float beta2, float eps, float weight_decay,
                          int64_t step, usc_stream_t s);

/* ------------------------------------------------------------------------
 * A1  elastic distortion of the training augmentation — the per-point half of
 * datasets/semseg.py:651-688 `elastic_distortion` (called from freemask_semseg.py:356-361):
 * xyz_out[i,0:3] = xyz_in[i,0:3] + magnitude * trilinear(noise)(xyz_in[i,0:3]), evaluated in f64 like
 * scipy's RegularGridInterpolator(bounds_error=0, fill_value=0).  xyz f32 or f64 [n,row_stride] (only the
 * first three columns are read/written; in place allowed), noise f32[dim_x,dim_y,dim_z,3] (already
 * smoothed), axis_* f64[dim_*] the grid coordinates (np.linspace of the reference).
 * ---------------------------------------------------------------------- */
int usc_elastic_displace(const void* xyz_in, int32_t is_f64, int64_t n, int32_t row_stride,
                         const float* noise, int32_t dim_x, int32_t dim_y, int32_t dim_z,
                         const double* axis_x, const double* axis_y, const double* axis_z,
                         double magnitude, void* xyz_out, usc_stream_t s);

/* ------------------------------------------------------------------------
 * F4  training-time augmentations of the scene reader — replaces the numpy /
 * volumentations / albumentations steps of datasets/freemask_semseg.py:334-406.
 * ---------------------------------------------------------------------- */
/* x[:, 0:3] <- x[:, 0:3] M^T + t in place (f64 arithmetic, one rounding to the
 * table's type): centring + random shift (:335-342), axis flips (:348-351),
 * Scale3d and RotateAroundAxis3d of conf/augmentation/volumentations_aug.yaml.
 * M (9, row-major) and t (3) are HOST doubles; x is f32 or f64 [n, row_stride]. */
int usc_affine_rows(void* x, int32_t is_f64, int64_t n, int32_t row_stride,
                    const double* M, const double* t, usc_stream_t s);
/* out[c] = ((x[0,c] + x[1,c]) + x[2,c]) + ... in f32, c < cols <= 64: numpy's
 * summation order for a.sum(0) / a.mean(0) of a C-contiguous table, so that
 * `coordinates -= coordinates.mean(0)` (:335) is reproduced bit for bit. */
int usc_colsum_sequential(const float* x, int64_t n, int32_t row_stride,
                          int32_t cols, float* out, usc_stream_t s);
/* out[i,c] = lut[c*256 + uint8(color[i,c])], c < 3: RandomBrightnessContrast /
 * RGBShift of conf/augmentation/albumentations_aug.yaml and the colour
 * normalisation (:408-409) as per-channel tables over the uint8-truncated
 * colours.  color f32[n,row_stride], lut f32[3][256] (device), out f32. */
int usc_color_lut(const float* color, int64_t n, int32_t row_stride,
                  const float* lut, float* out, int32_t out_stride,
                  usc_stream_t s);

/* ------------------------------------------------------------------------
 * F2  Felzenszwalb mesh over-segmentation — replaces the reference's
 * felzenszwalb_cpp extension (utils/cpp_utils/segmentator.cpp:17-154
 * segment_graph / segment_mesh; caller pseudo_masks/datasets/scannet.py:156-197).
 * Device: face normals, vertex normals (the running blend of face normals in
 * face order, :62-82), edge weights (:85-121) — bit-equal to the reference
 * (separately rounded operations).  The caller sorts the 3F edges by weight on
 * the device (stable) and hands the sorted lists to usc_felz_merge_host for the
 * two sequential merge loops (:17-44, :127-139).
 * ---------------------------------------------------------------------- */
/* face_normals f32[F,3] = normalised cross(p2-p1, p3-p1). */
int usc_felz_face_normals(const float* vertices, const int32_t* faces,
                          int64_t n_faces, float* face_normals, usc_stream_t s);
/* corner_order i64[3F]: the (face, corner) entries 3f+j sorted by their vertex,
 * stable (usc_segment_csr over faces.reshape(-1)); vertex_off i64[V+1]. */
int usc_felz_vertex_normals(const float* face_normals, const int64_t* corner_order,
                            const int64_t* vertex_off, int64_t n_vertices,
                            float* normals, usc_stream_t s);
/* Edge 3f+0 = (i1,i2), 3f+1 = (i1,i3), 3f+2 = (i3,i2): endpoints and weight. */
int usc_felz_edge_weights(const float* vertices, const float* colors,
                          const float* normals, const int32_t* faces,
                          int64_t n_faces, int32_t* edge_a, int32_t* edge_b,
                          float* weights, usc_stream_t s);
/* HOST pointers (the one exception in this ABI): edges sorted by weight ->
 * comps i32[V] = union-find representative of every vertex. */
int usc_felz_merge_host(const int32_t* edge_a, const int32_t* edge_b,
                        const float* weights, int64_t n_edges, int32_t n_vertices,
                        float kthr, int32_t seg_min_verts, int32_t* comps);

/* ------------------------------------------------------------------------
 * F2b the same over-segmentation for a point cloud without a mesh
 * (csrc/felz_points.hip): the edge set is a symmetrised k-NN table instead of
 * the triangles' sides.  The reference reconstructs a mesh for such clouds
 * (pseudo_masks/datasets/preprocess/stanford.py:80-135, open3d Poisson) only
 * to have edges; sort and merge are F2's.
 *
 * usc_felz_knn_edges: idx i32[n,k], count i32[n] as usc_knn_hybrid_grid writes
 * them for query == ref (1 <= k <= 64, 0 <= n < 2^31).  PRECONDITION: the
 * first count[i] entries of row i are distinct and lie in [0, n); an entry
 * outside [0, n) is skipped, never dereferenced, and a count is clamped to
 * [0, k].  For row i ascending and position p < count[i] ascending, with
 * j = idx[i,p] != i, the edge (edge_a = i, edge_b = j) is emitted iff i < j,
 * or i > j and i does not occur in idx[j, :count[j]].  So every undirected
 * pair that appears in either list is emitted exactly once, oriented from the
 * emitting row, in (i, p) order.  (A point need not be first in its own row:
 * coincident points sort by index.)
 * ONE call into WORST-CASE buffers, not a count/fill pair: edge_a and edge_b
 * hold n * k entries each (a point that is missing from its own full row, as
 * among more than k coincident points, emits k edges), the first *n_edges of
 * them are written and the rest is left alone; n_edges i64[1] is DEVICE
 * memory, written on the stream.  The caller reads it back when it needs the
 * number on the host (the pipeline ends in the host merge anyway).  Steps: a
 * per-row bit mask of the emitting positions, the device exclusive scan of
 * their popcounts, and the write pass.  ws holds
 * usc_felz_knn_edges_ws_bytes(n) bytes (-1 for n out of range).
 *
 * usc_felz_point_edge_weights: weights f32[n_edges] of an explicit edge list
 * over points, colors, normals f32[n_points,3].
 *   oriented = 1  usc_felz_edge_weights' arithmetic, operation for operation
 *                 (one shared device function): for the same endpoints,
 *                 normals and colours the bits are equal.
 *   oriented = 0  for estimated normals, whose sign is arbitrary
 *                 (usc_normals_pca), so the convexity test means nothing:
 *                 normal_dist = 1 - |dot|, and no weight is squared.
 * A zero-length edge (coincident points) has a NaN direction; `dot2 > 0` is
 * then false and the weight is the finite normal_dist * color_dist.  An
 * endpoint outside [0, n_points) reads nothing and gives +inf.
 * Both: explicit stream, no allocation, no host synchronisation, no atomics;
 * two calls write the same bytes; bad arguments are refused before any launch
 * with nothing written.
 * ---------------------------------------------------------------------- */
int64_t usc_felz_knn_edges_ws_bytes(int64_t n_points);
int usc_felz_knn_edges(const int32_t* idx, const int32_t* count, int64_t n_points,
                       int32_t k, int32_t* edge_a, int32_t* edge_b,
                       int64_t* n_edges, void* ws, int64_t ws_bytes,
                       usc_stream_t s);
int usc_felz_point_edge_weights(const float* points, const float* colors,
                                const float* normals, int64_t n_points,
                                const int32_t* edge_a, const int32_t* edge_b,
                                int64_t n_edges, int32_t oriented,
                                float* weights, usc_stream_t s);

/* ------------------------------------------------------------------------
 * Validation AP — the mask / GT-instance overlap counts of the ScanNet instance
 * evaluator (benchmark/evaluate_semantic_instance.py, assign_instances_for_scan*).
 * masks u8[n, ld] row-major, nonzero = point in mask (np.not_equal(mask, 0));
 * slot i32[n], each in [0, nslots): the GT instance slot of every point (the
 * caller's last slot = void); counts i32[(k + 1) * nslots], written in full:
 *   counts[j * nslots + s] = #points with masks[p, j] != 0 and slot[p] == s  (j < k)
 *   counts[k * nslots + s] = #points with slot[p] == s                      (GT sizes)
 * k in 1..4096, ld >= k, nslots in 1..65536, n in 0..2^31-1.  Exact integers:
 * bit-identical from run to run.  One call per scene, no synchronisation.
 * ---------------------------------------------------------------------- */
int usc_mask_gt_overlap(const uint8_t* masks, int64_t n, int32_t k, int64_t ld,
                        const int32_t* slot, int32_t nslots, int32_t* counts,
                        usc_stream_t s);

/* ------------------------------------------------------------------------
 * ViT image-encoder attention (models/encoders_2d/dino.py through
 * third_party/dino_vit/extractor.py: DINO ViT-S/8 at stride 4, 2 962 tokens
 * per 192x256 frame).  Unmasked, non-causal, forward only, head dim 64:
 *   o = softmax(scale * q k^T) v   per (batch, head)
 * qkv f32[B, T, 3, H, 64]: the rows nn.Linear(384, 1152) writes, read in place;
 * o f32[B, T, H*64]: head-major columns, what attn.proj reads.  Both 16-byte
 * aligned.  B, T, H >= 1, B*H <= 65535; T up to 2^30 (keys are streamed,
 * the scores never reach memory: no limit from the kernel's structure).
 * precision 0: f32 operands (v_mfma_f32_32x32x2_f32); 1: q, k, v and the
 * probabilities rounded to bf16, nearest even as usc_cast_bf16
 * (v_mfma_f32_32x32x16_bf16).  Accumulators and the running max / sum are f32
 * in both.  No atomics, fixed summation order: bit-identical from run to run.
 * Replaces `attn = (q @ k.transpose(-2, -1)) * scale; softmax; attn @ v` of
 * the ViT's Attention.forward and the permutes around it.
 * ---------------------------------------------------------------------- */
int32_t usc_vit_attn_head_dim(void); /* 64 */
int usc_vit_attn_fwd(const float* qkv, int32_t B, int32_t T, int32_t H, float scale,
                     int32_t precision, float* o, usc_stream_t s);

/* ------------------------------------------------------------------------
 * Instance targets of the supervised collate (datasets/utils.py:529-613,
 * get_instance_masks) from one label table labels i64[n, ld]: column 0 the
 * semantic label, column 1 the instance id (any int64), optionally a column of
 * contiguous segment ids.  ids i64[u]: the distinct instance ids, ascending.
 * n in 0..2^31-2.  Integers only: bit-identical from run to run.
 *
 * usc_instance_index: rank i32[n] = index of the row's id in ids (-1: not in
 *   the list); count i32[u] = rows per id; first i32[u] = its first row
 *   (INT32_MAX for an id without rows).  All three written in full.
 * usc_instance_select: walks ids in ascending order; drops id -1, ids without
 *   rows and ids whose label labels[first, 0] is one of filter i64[nf]; the
 *   others take slots 0..T-1 in that order.  slot i32[u] (-1: dropped),
 *   labels_out i64[>= T]: max(label - label_offset, 0); *n_kept = T (device).
 * usc_instance_masks: masks u8[t, n], masks[j, r] = (slot[rank[r]] == j), every
 *   byte written exactly once (no memset needed), any base alignment.  With
 *   segment_mask u8[t, n_segments] (zeroed by the caller; may be NULL) it sets
 *   segment_mask[j, seg[r * seg_ld]] = 1 for every row r of target j; segment
 *   ids outside [0, n_segments) are skipped.  t = 0, n = 0 and n_segments = 0
 *   launch nothing.
 * ---------------------------------------------------------------------- */
int usc_instance_index(const int64_t* labels, int64_t n, int32_t ld, const int64_t* ids, int32_t u,
                       int32_t* rank, int32_t* count, int32_t* first, usc_stream_t s);
int usc_instance_select(const int64_t* labels, int64_t n, int32_t ld, const int64_t* ids, int32_t u,
                        const int32_t* count, const int32_t* first, const int64_t* filter, int32_t nf,
                        int64_t label_offset, int32_t* slot, int64_t* labels_out, int32_t* n_kept,
                        usc_stream_t s);
int usc_instance_masks(const int32_t* rank, int64_t n, const int32_t* slot, int32_t u, int32_t t,
                       uint8_t* masks, const int64_t* seg, int32_t seg_ld, int64_t n_segments,
                       uint8_t* segment_mask, usc_stream_t s);

/* ------------------------------------------------------------------------
 * FreeMask pseudo masks, voxel mode (pseudo_masks/freemask_main.py:242-279,
 * :352-417; utils/freemask_utils.py:8-18 cosine_sim; utils/pc_utils.py:727-757
 * matrix_nms(kernel='mask')) without the f32[Q,K] similarity matrix.
 *   a[q][k] = (fq[q] * sq[q]) . (fk[k] * sk[k]);  a -= rowmin[q];
 *   a /= (rowmax[q] - rowmin[q]) + 1e-9;  a[:, all-zero keys] = 0;  mask = a >= threshold
 * fq f32[q,c], fk f32[k,c], 1 <= c <= 512, any q, k >= 1 (tails inside the
 * kernels).  The products run on v_mfma_f32_32x32x2_f32; every a[q][k] is the
 * same chain of operations in the three kernels that form it, so the bits, the
 * sums and the soft rows agree with each other bit for bit.  No atomics, fixed
 * summation order: bit-identical from run to run.
 *
 * usc_freemask_normalize: scale[r] = 1 / (|feats[r]| + 1e-9) for every row;
 *   zero u8[n] (may be NULL) = 1 where the row is all zero.
 * usc_freemask_rowstats: rowmin / rowmax f32[q] of a over all k keys (the
 *   all-zero keys included, as the reference).
 * usc_freemask_bits: bits u64[q, ceil(k/64)], key j = bit j % 64 of word
 *   j / 64, bits at positions >= k zero, every word written; count i32[q] = the
 *   popcount of the row; soft_sum f32[q] = sum of a over the row's set bits.
 * usc_freemask_soft_rows: out f32[m, k], row j = the normalised, key-zeroed a of
 *   query qidx[j] (each in [0, q)); m <= 4096.
 * ws: usc_freemask_ws_bytes(q, k) bytes, for rowstats and bits alike.
 *
 * usc_mask_bits_extent: lo / hi i32[n,3] = min / max of coords i32[k,3] over the
 *   set bits of every row of bits u64[n, ceil(k/64)]; an empty row gives
 *   lo = INT32_MAX > hi = INT32_MIN.
 * usc_mask_bits_nms: greedy mask NMS over the rows order i32[n] of bits (each
 *   in range, in descending score order), count i32[rows] their popcounts:
 *   walking positions upward, a position i that is still alive kills every
 *   later alive j with  union > 0 ? (float)inter / (float)union > nms_thr : true,
 *   inter = popcount(row_i & row_j), union = count_i + count_j - inter.
 *   keep u8[n] by position.  ws: usc_mask_bits_nms_ws_bytes(n) =
 *   n * ceil(n/64) * 8 bytes (the "i would kill j" bit matrix); n <= 524288.
 * ---------------------------------------------------------------------- */
int usc_freemask_normalize(const float* feats, int64_t n, int32_t c, float* scale, uint8_t* zero, usc_stream_t s);
int64_t usc_freemask_ws_bytes(int64_t q, int64_t k);
int usc_freemask_rowstats(const float* fq, const float* sq, int64_t q, const float* fk, const float* sk, int64_t k,
                          int32_t c, float* rowmin, float* rowmax, void* ws, int64_t ws_bytes, usc_stream_t s);
int usc_freemask_bits(const float* fq, const float* sq, int64_t q, const float* fk, const float* sk,
                      const uint8_t* zero_k, int64_t k, int32_t c, const float* rowmin, const float* rowmax,
                      float threshold, uint64_t* bits, int32_t* count, float* soft_sum, void* ws, int64_t ws_bytes,
                      usc_stream_t s);
int usc_freemask_soft_rows(const float* fq, const float* sq, int64_t q, const float* fk, const float* sk,
                           const uint8_t* zero_k, int64_t k, int32_t c, const float* rowmin, const float* rowmax,
                           const int32_t* qidx, int32_t m, float* out, usc_stream_t s);
int usc_mask_bits_extent(const uint64_t* bits, int64_t n, int64_t k, const int32_t* coords, int32_t* lo, int32_t* hi,
                         usc_stream_t s);
int64_t usc_mask_bits_nms_ws_bytes(int64_t n);
int usc_mask_bits_nms(const uint64_t* bits, const int32_t* count, int64_t k, const int32_t* order, int32_t n,
                      float nms_thr, uint8_t* keep, void* ws, int64_t ws_bytes, usc_stream_t s);

/* ------------------------------------------------------------------------
 * FreeMask pseudo masks, segment mode (pseudo_masks/freemask_main.py:186-233,
 * :282-350, :359-370): keys = queries = the S segment features, a mask is a
 * set of whole segments, rows are S-bit rows in the layout of usc_freemask_bits.
 * Explicit stream, no allocation, no synchronisation, no float atomics; two
 * runs give identical bits.
 *
 * usc_maxpool_down2_i32 (:189-199, MinkowskiMaxPooling(kernel_size=2, stride=2)
 *   on the id column, pooled as integers): out[p] = max of in[child] over the
 *   present children nbr2[k * n_coarse + p] (k < 8, -1 = absent; the table of
 *   usc_avgpool_down2); a child index >= n_fine counts as absent; a parent
 *   without a child gives -1.
 * usc_mask_bits_components (:288-327, the per-query scan over sets): for the
 *   rows rows[i] (i < n_rows, each in [0, n_bits_rows)) of bits
 *   u64[n_bits_rows, ceil(S/64)], the connected parts of the row's mask on the
 *   undirected adjacency adj_off i64[S+1], adj i32[adj_off[S]] (symmetric, every
 *   entry in [0, S): the CALLER checks that).  label i32[n_rows, S]: -1 outside
 *   the mask, else the smallest segment index of the part; n_comp i32[n_rows].
 *   One workgroup per row, labels in LDS, min-label propagation until a round
 *   changes nothing.  S <= USC_MASK_BITS_MAX_SEGMENTS
 *   (= usc_mask_bits_max_segments()), refused above.
 * usc_mask_bits_split (:329-348, :353 numerators): row_off i64[n_rows] = the
 *   exclusive scan of n_comp.  Output row row_off[i] + j is the part of input
 *   row i with the j-th smallest root: out_bits u64[R, ceil(S/64)], out_src
 *   (= i), out_root, seg_count, vox_count = sum of weight[s] over the part
 *   (i32[R]), soft_sum f32[R] = sum of soft[soft_row[i] * soft_ld + s] over the
 *   part in ascending s.  Same cap on S.
 * usc_mask_bits_nms_weighted (utils/pc_utils.py:727-757 on the remapped masks of
 *   :361-370): usc_mask_bits_nms with inter = sum of weight[s] over the set bits
 *   of row_i & row_j (weight i32[k]) and the caller's weighted counts.  Exact
 *   while the sum of all weights is below 2^24 (the CALLER checks that).
 * ---------------------------------------------------------------------- */
#define USC_MASK_BITS_MAX_SEGMENTS 8192
int32_t usc_mask_bits_max_segments(void);
int usc_maxpool_down2_i32(const int32_t* in, int64_t n_fine, const int32_t* nbr2, int64_t n_coarse, int32_t* out,
                          usc_stream_t s);
int usc_mask_bits_components(const uint64_t* bits, int64_t n_bits_rows, int32_t n_segments, const int32_t* rows,
                             int32_t n_rows, const int64_t* adj_off, const int32_t* adj, int32_t* label,
                             int32_t* n_comp, usc_stream_t s);
int usc_mask_bits_split(const int32_t* label, int32_t n_rows, int32_t n_segments, const int64_t* row_off,
                        const int32_t* n_comp, const int32_t* weight, const float* soft, int64_t soft_ld,
                        const int32_t* soft_row, uint64_t* out_bits, int32_t* out_src, int32_t* out_root,
                        int32_t* seg_count, int32_t* vox_count, float* soft_sum, usc_stream_t s);
int usc_mask_bits_nms_weighted(const uint64_t* bits, const int32_t* count, const int32_t* weight, int64_t k,
                               const int32_t* order, int32_t n, float nms_thr, uint8_t* keep, void* ws,
                               int64_t ws_bytes, usc_stream_t s);

/* ------------------------------------------------------------------------
 * Dataset tables (datasets/freemask.py, datasets/preprocessing.py).  Explicit
 * stream, no allocation, no synchronisation, no float atomics.
 *
 * usc_softmask_stats (datasets/freemask_semseg.py:300-310 without the [N,K,2]
 *   temporaries): for every column j of soft f32[n,k], count i32[k] = the rows
 *   with soft > thr, lo / hi f32[k,2] = min / max of x and y (xyz f32[n,3]) over
 *   those rows; an empty column gives lo = +FLT_MAX, hi = -FLT_MAX.  Lanes run
 *   over columns; partials per row block, then one finish pass in block order.
 *   ws: usc_softmask_stats_ws_bytes(n, k).
 * usc_softmask_table (:311-316 and the segment column of :437): out
 *   i32[n, kk+2]; column 1 + j = soft[:, keep[j]] > thr as 0/1 (keep i32[kk],
 *   every entry in [0, k): the CALLER checks that), column 0 = the OR of those,
 *   column kk+1 = (int32_t)segments[r].
 * usc_mesh_vertex_normals (open3d TriangleMesh::ComputeVertexNormals): the
 *   unnormalised face normals (v1-v0) x (v2-v0), in f64 from the f32 vertices
 *   and uncontracted, summed per vertex over corner_order i64[3F] (the stable
 *   sort of the face corners by vertex: ascending face order) between
 *   vertex_off[v] and vertex_off[v+1], normalised, stored as f32; a zero or
 *   non-finite sum gives (0,0,1).  Face indices in [0, V): the CALLER checks.
 * ---------------------------------------------------------------------- */
int64_t usc_softmask_stats_ws_bytes(int64_t n, int32_t k);
int usc_softmask_stats(const float* soft, const float* xyz, int64_t n, int32_t k, float thr, int32_t* count, float* lo,
                       float* hi, void* ws, int64_t ws_bytes, usc_stream_t s);
int usc_softmask_table(const float* soft, int64_t n, int32_t k, float thr, const int32_t* keep, int32_t kk,
                       const float* segments, int32_t* out, usc_stream_t s);
int usc_mesh_vertex_normals(const float* vertices, const int32_t* faces, const int64_t* corner_order,
                            const int64_t* vertex_off, int64_t n_vertices, int64_t n_faces, float* normals,
                            usc_stream_t s);

/* ------------------------------------------------------------------------
 * Self-training files as bit rows (csrc/selftrain.hip; trainer/postprocess.py
 * save_for_freemask(fmt="bits"), datasets/freemask.py load_self_train_bits).
 * Layout of usc_freemask_bits: row j is u64[W], W = ceil(n / 64), point r is
 * bit r % 64 of word r / 64; bits at positions >= n are written as zero and
 * every word is written.  Explicit stream, no allocation, no synchronisation,
 * no atomics: two runs give the same bytes.
 *
 * usc_mask_columns_to_bits: masks u8[n,k] row-major (non-zero = set) -> bits
 *   u64[k,W], count i32[k] = the column popcounts (a second pass over the
 *   rows).  A wave owns 64 consecutive points; its tile is staged through LDS
 *   128 columns at a time and gives one ballot word per column.
 * usc_mask_bits_gather: dst row j = src row j (u64[k, ceil(m / 64)]) read at
 *   ind i64[n] (the 1-NN transfer masks[ind]); every entry in [0, m): the
 *   CALLER checks that.  count i32[k] = the popcounts of dst.
 * usc_mask_bits_count: count i32[k] = the popcounts of the rows of bits
 *   u64[k,W] (the sizes of a file's masks: the file holds no counts).
 * usc_selftrain_merge (datasets/freemask_semseg.py:246-265): one workgroup
 *   walks the rows of st u64[kp,W] in ascending order; with f = popcount(st[j]
 *   & ~fg), row j is taken when total[j] > 0 and 2 f > total[j] (integers; a
 *   tie is refused): fresh[a] = st[j] & ~fg, fg |= fresh[a], picked[a] = j.
 *   Stops at a == max_add or j == kp; rows a.. of fresh are zero, picked[a..]
 *   = -1, *n_added = a; fg u64[W] is updated in place.  kp = 0 and max_add = 0
 *   are valid.  fg is kept in LDS while W <= usc_selftrain_merge_lds_words
 *   (default 7168 words = 458 752 points), else in global memory.
 * usc_selftrain_merge_lds_words(words): sets that limit (clamped to the
 *   default; a negative value changes nothing) and returns the previous one.
 * usc_mask_bits_to_columns / _u8: out[r * ld + col0 + i] = bit r of row
 *   rows[i] (i32[m], rows of bits u64[*, W]: the CALLER checks the range) as
 *   0.0f / 1.0f (u8: 0 / 1), r < n; needs col0 + m <= ld.
 * ---------------------------------------------------------------------- */
int usc_mask_columns_to_bits(const uint8_t* masks, int64_t n, int32_t k, uint64_t* bits, int32_t* count,
                             usc_stream_t s);
int usc_mask_bits_gather(const uint64_t* src, int64_t m, const int64_t* ind, int64_t n, int32_t k, uint64_t* dst,
                         int32_t* count, usc_stream_t s);
int usc_mask_bits_count(const uint64_t* bits, int32_t k, int64_t n, int32_t* count, usc_stream_t s);
int32_t usc_selftrain_merge_lds_words(int32_t words);
int usc_selftrain_merge(const uint64_t* st, const int32_t* total, int32_t kp, int64_t n, uint64_t* fg,
                        int32_t max_add, uint64_t* fresh, int32_t* picked, int32_t* n_added, usc_stream_t s);
int usc_mask_bits_to_columns(const uint64_t* bits, const int32_t* rows, int32_t m, int64_t n, float* out, int64_t ld,
                             int32_t col0, usc_stream_t s);
int usc_mask_bits_to_columns_u8(const uint64_t* bits, const int32_t* rows, int32_t m, int64_t n, uint8_t* out,
                                int64_t ld, int32_t col0, usc_stream_t s);

/* ------------------------------------------------------------------------
 * general.separate_instances of the export step (csrc/separate.hip; reference
 * trainer/trainer.py:609-650, utils/point_cloud_utils.py:82-121): a kept
 * instance is cut into its connected parts on the segment adjacency.  Explicit
 * stream, no allocation, no float, no read-modify-write atomics; every output
 * element has one writer: two runs give the same bytes.
 *
 * usc_mask_columns_to_segment_bits (:626-629, np.unique of the masked ids per
 *   instance): masks u8[n,k] row-major (non-zero = set); order i64[n], seg_off
 *   i64[S+1] = the points sorted by segment index (usc_segment_csr).  bits
 *   u64[k, ceil(S/64)] in the layout of usc_freemask_bits: bit s of row j = OR
 *   of masks[p,j] over the points p of segment s; bits at positions >= S are
 *   zero, every word is written.  The CALLER checks the CSR (seg_off rises
 *   from 0 to n, order is a permutation); a broken one gives wrong bits but no
 *   read outside the arrays: offsets are clamped to [0, n] and an entry of order
 *   outside [0, n) is read as point 0.  k = 0 is valid.
 * usc_mask_bits_components_wide (:632, separate_segments): the contract and
 *   the labels of usc_mask_bits_components for S up to
 *   USC_MASK_BITS_MAX_SEGMENTS_WIDE (= usc_mask_bits_max_segments_wide()): one
 *   workgroup per row, the row of `label` is the work array (global memory).
 *   The round loop stops after S + 1 rounds; a correct run is quiet after at
 *   most S.  Reaching the bound sets *status (device i32[1], zeroed here), and
 *   the call, which waits for the stream to read it, returns USC_ERR_RANGE.
 *   Above the cap a round of one workgroup over a row is too long: refused.
 * usc_segment_parts_to_columns (:639, np.isin per part): out u8[n, n_parts],
 *   out[r * n_parts + p] = (label[src[p] * S + idx[r]] == root[p]); label
 *   i32[n_rows, S], src in [0, n_rows), idx i32[n] in [0, S): the CALLER checks
 *   both.  n = 0 and n_parts = 0 are valid.
 * ---------------------------------------------------------------------- */
#define USC_MASK_BITS_MAX_SEGMENTS_WIDE 65536
int32_t usc_mask_bits_max_segments_wide(void);
int usc_mask_columns_to_segment_bits(const uint8_t* masks, int64_t n, int32_t k, const int64_t* order,
                                     const int64_t* seg_off, int32_t n_segments, uint64_t* bits, usc_stream_t s);
int usc_mask_bits_components_wide(const uint64_t* bits, int64_t n_bits_rows, int32_t n_segments, const int32_t* rows,
                                  int32_t n_rows, const int64_t* adj_off, const int32_t* adj, int32_t* label,
                                  int32_t* n_comp, int32_t* status, usc_stream_t s);
int usc_segment_parts_to_columns(const int32_t* label, int32_t n_rows, int32_t n_segments, const int32_t* src,
                                 const int32_t* root, int32_t n_parts, const int32_t* idx, int64_t n, uint8_t* out,
                                 usc_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* USC3D_H */
