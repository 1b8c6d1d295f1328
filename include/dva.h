/*
 * dva.h — C ABI of libdva_hip.so, the MI355X (gfx950) implementation of the DeepViewAgg
 * multimodal hot path (mapping build -> multi-view gather -> view-attention pooling).
 *
 * Contract (SURVEY.md §8b "C-ABI to export"):
 *   - plain C entry points, caller-owned DEVICE buffers (HBM pointers), sizes as integers;
 *   - every function returns int: 0 = ok, <0 = DVA_ERR_*; no exceptions cross the ABI;
 *   - the HIP stream is passed explicitly (as void* == hipStream_t); nothing synchronises the
 *     device unless stated ("[syncs]"), no hidden global state, re-entrant;
 *   - no torch types. The reference is 100 % Python, so "the reference interface each entry
 *     replaces" is a Python call site, cited per function as file:line under /root/reference.
 *
 * Layouts: feature maps are channels-last x[B][H][W][C]; row matrices are row-major [rows][C];
 * CSR pointers are int64 (reference: torch.LongTensor). dtype codes below select the element type
 * of "feature" buffers (void*): fp32, bf16 or fp16; scores / mapping features / statistics are fp32.
 * DVA_F16 (torch.float16, autocast(float16)) is accepted by: dva_segment_csr_fwd / _bwd, dva_gather_csr,
 * dva_gather_nearest_fwd / _bwd, dva_gather_bilinear_fwd / _bwd, dva_gather_rows_sum,
 * dva_gather_segment_reduce_fwd / _bwd, dva_interp_segment_reduce_fwd / _bwd, dva_view_attention_*,
 * dva_view_gather_attention_*, dva_view_gather_rows_grad, dva_view_gather_rows_grad_rec16_to, dva_rowbn_*, dva_chain_attn_fwd_dt, dva_chain_attn_bwd_dt and
 * dva_plan_split_rows_grad (dtype = out_dtype = DVA_F16).  Every other entry with a dtype argument returns
 * DVA_ERR_UNSUPPORTED for it before launching anything.
 */
#ifndef DVA_H_
#define DVA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVA_OK 0
#define DVA_ERR_INVALID (-1)     /* bad argument (null pointer, negative size, bad enum) */
#define DVA_ERR_UNSUPPORTED (-2) /* valid request this build does not implement           */
#define DVA_ERR_LAUNCH (-3)      /* HIP runtime reported a launch/runtime error           */
#define DVA_ERR_OVERFLOW (-4)    /* composite key does not fit int64 (utils/multimodal.py:141) */

#define DVA_F32 0
#define DVA_BF16 1
#define DVA_F16 2

#define DVA_SUM 0
#define DVA_MEAN 1
#define DVA_MAX 2
#define DVA_MIN 3

/* camera models of core/multimodal/visibility.py:478-538 */
#define DVA_CAM_EQUIRECT 0      /* 's3dis_equirectangular' */
#define DVA_CAM_PINHOLE_SCANNET 1
#define DVA_CAM_PINHOLE_KITTI 2 /* 'kitti360_perspective' */
#define DVA_CAM_FISHEYE_KITTI 3 /* 'kitti360_fisheye' */

/* library / device introspection ------------------------------------------------------------ */
int dva_version(void);
/* number of visible HIP devices, or <0 on runtime error. Does not create a context. */
int dva_device_count(void);

/* ------------------------------------------------------------------------------------------ *
 * CSR segment primitives.  Replace torch_scatter.segment_csr / gather_csr call sites:
 *   modules/multimodal/pooling.py:63 (BimodalCSRPool), :289,:295 (weighted sum, gating max),
 *   :628 (DeepSetFeat pool), :787,:807 (softmax), :813-841 (gather_csr);
 *   core/multimodal/image.py:1767 (per-view mean of mapping features).
 * Empty groups reduce to 0 (pooling.py:870); max/min ties -> first row of the group.
 * ------------------------------------------------------------------------------------------ */

/* out[g, c] = reduce_{r in [ptr[g], ptr[g+1])} src[r, c].  arg (nullable) receives, for MAX/MIN,
 * the winning row index (int32, -1 for empty groups); required later by the backward. */
int dva_segment_csr_fwd(const void* src, const int64_t* ptr, void* out, int32_t* arg,
                        int64_t n_groups, int32_t C, int32_t dtype, int32_t reduce, void* stream);

/* grad_src[r, c] for r in every group (rows outside [ptr[0], ptr[n_groups]) are not touched).
 * SUM: grad_out[g,c]; MEAN: grad_out[g,c]/n_g; MAX/MIN: grad_out[g,c] if r == arg[g,c] else 0. */
int dva_segment_csr_bwd(const void* grad_out, const int64_t* ptr, const int32_t* arg,
                        void* grad_src, int64_t n_groups, int32_t C, int32_t dtype,
                        int32_t reduce, void* stream);

/* out[r, c] = src[g(r), c]  (pooling.py:813-841 gather_csr). Backward = dva_segment_csr_fwd(SUM). */
int dva_gather_csr(const void* src, const int64_t* ptr, void* out, int64_t n_groups, int32_t C,
                   int32_t dtype, void* stream);

/* Per-group softmax of fp32 scores src[V, G] (pooling.py:758-810 segment_softmax_csr):
 * a = exp((s - max_g)/d) / (sum_g exp(.) + eps), d = sqrt(n_g) if scaling else 1. */
int dva_segment_softmax_csr_fwd(const float* src, const int64_t* ptr, float* out,
                                int64_t n_groups, int32_t G, int32_t scaling, float eps,
                                void* stream);
/* grad_src = a * (grad_a - sum_g(a * grad_a)) / d   (the eps term's O(1e-12) leak is dropped). */
int dva_segment_softmax_csr_bwd(const float* grad_out, const float* out, const int64_t* ptr,
                                float* grad_src, int64_t n_groups, int32_t G, int32_t scaling,
                                void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Multi-view feature gather.  Replaces SameSettingImageData.get_mapped_features
 * (core/multimodal/image.py:1262-1287): nearest = x[feature_map_indexing] (:1285, indexing
 * tuple built at :1871-1885 after downscale_images :1916-1980); bilinear = sparse_interpolation
 * (:105-170).  Feature maps are channels-last [B,H,W,C] so one atom = one contiguous C-burst.
 * ------------------------------------------------------------------------------------------ */

/* Build the packed 8-byte gather index of every atom (mapped pixel):
 *   idx[p] = { int32 image, int16 x, int16 y } with x = floor(px / ratio), y = floor(py / ratio)
 * image[p] = images[view(p)] expanded through atom_ptr (image.py:1879-1880 repeat_interleave).
 * pixels: [P,2] (w,h) of pix_bytes-wide signed ints (2, 4 or 8: image.py:507-516 pixel_dtype).
 * ratio >= 1 is the mapping->feature-map downscale (image.py:1953-1954, float floor-division). */
int dva_pack_gather_index(const int64_t* images, const int64_t* atom_ptr, const void* pixels,
                          int32_t pix_bytes, double ratio, int64_t n_views, int64_t n_atoms,
                          void* packed_idx /* int64[P] */, void* stream);

/* dva_pack_gather_index followed by dva_gather_row_index (row_offset 0, no counts) in one pass: the flat row index
 * (image * H + y) * W + x of every atom straight from the mapping (image.py:1871-1885 + :1953-1954); what the lazy
 * nearest gather needs.  Same pixel rounding as dva_pack_gather_index. */
int dva_mapping_row_index(const int64_t* images, const int64_t* atom_ptr, const void* pixels, int32_t pix_bytes,
                          double ratio, int64_t n_views, int64_t n_atoms, int32_t B, int32_t H, int32_t W,
                          int32_t* row_idx, void* stream);
/* row_idx[p] = row_offset + (img*H + y)*W + x : the atom's row in the [B*H*W, C] view of the map
 * (image.py:1871-1885 flattened).  counts (nullable, caller-zeroed int32[B*H*W]) += 1 per atom. */
int dva_gather_row_index(const void* packed_idx, int64_t n_atoms, int32_t B, int32_t H, int32_t W,
                         int32_t row_offset, int32_t* row_idx, int32_t* counts, void* stream);

/* out[p, :] = x[img, y, x, :] */
int dva_gather_nearest_fwd(const void* x, const void* packed_idx, void* out, int64_t n_atoms,
                           int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream);
/* grad_x[img, y, x, :] += grad_out[p, :].  grad_x is fp32 [B,H,W,C], caller-zeroed
 * (fp32 accumulation of bf16 gradients; atomics => run-to-run order may vary in the last ulp). */
int dva_gather_nearest_bwd(const void* grad_out, const void* packed_idx, float* grad_x,
                           int64_t n_atoms, int32_t B, int32_t H, int32_t W, int32_t C,
                           int32_t dtype, void* stream);

/* The nearest gather (core/multimodal/image.py:1262-1287) fused with the MAX / MEAN / SUM / MIN pool behind it
 * (BimodalCSRPool(mode), pooling.py:14-71; at the atomic level of a non-exact mapping -- several pixels per view -- through
 * modules.py:400-407, at the view level as the view pooling of the image-only and the mean-pool baselines): out[s][c] = reduce over the items a in [seg_ptr[s], seg_ptr[s+1]) of rows[row_idx[a]][c]
 * with dva_segment_csr_fwd's arithmetic (fp32 accumulation from 0 in item order, MEAN divides once by the fp32 count, one
 * rounding to the storage type, empty segments give 0, MAX / MIN: first item on ties) -- bit for bit the materialised
 * composition, no [P, C] tensor.  Any C >= 1, dtype fp32 / bf16 / fp16: 16-byte accesses when C % (16 / s) == 0 and rows,
 * out and arg are 16-byte aligned, one thread per (segment, channel) otherwise.  arg (MAX / MIN, else nullable) uint16
 * [S][C] = offset of the winning item inside its segment (0xffff: none; segments must own <= 65534 items).
 * _bwd: grad_rows [R][C] in the rows' dtype, WRITTEN (every element once, fp32 accumulation, one rounding) =
 * sum over the items a on row r of grad_out[s][c] (SUM), grad_out[s][c] / count_s (MEAN, fp32 true division) or
 * grad_out[s][c] where arg[s][c] == a - seg_ptr[s] (MAX / MIN), s = seg_of_item[a] (int32 [P], dva_csr_expand); a segmented
 * reduction over the row plan of the items (perm int32 [P] = items sorted by map row, row_ptr int32 [R + 1], as
 * dva_row_plan gives them), one wavefront per map row, no float atomics: deterministic.
 * Sizes of 2^31 or more return DVA_ERR_UNSUPPORTED. */
int dva_gather_segment_reduce_fwd(const void* rows, const int32_t* row_idx, const int64_t* seg_ptr, void* out, void* arg,
                                  int64_t S, int64_t P, int64_t R, int32_t C, int32_t dtype, int32_t reduce,
                                  void* stream);
int dva_gather_segment_reduce_bwd(const void* grad_out, const void* arg, const int64_t* seg_ptr, const int32_t* perm,
                                  const int32_t* row_ptr, const int32_t* seg_of_item, void* grad_rows, int64_t S,
                                  int64_t P, int64_t R, int32_t C, int32_t dtype, int32_t reduce, void* stream);

/* The BILINEAR gather (sparse_interpolation, image.py:105-170) fused with the MAX / MEAN / SUM / MIN pool behind it
 * (BimodalCSRPool(mode), pooling.py:14-71): out[s][c] = reduce over the items p in [seg_ptr[s], seg_ptr[s+1]) of v(p, c),
 * v(p, c) = ((w0 x0 + w1 x1) + w2 x2) + w3 x3 with x_k = rows[tap_rows[p][k]][c] and w_k = tap_weights[p][k] -- the
 * arithmetic of dva_gather_bilinear_fwd (products and sums rounded one by one, no fma), rounded once to the storage type as
 * the [P, C] tensor would have held it -- and on those values dva_segment_csr_fwd's arithmetic (fp32 accumulation from 0
 * in item order, MEAN divides once by the fp32 count, one rounding, empty segments give 0, MAX / MIN: first item on ties,
 * NaN as that entry treats it): bit for bit the materialised composition, no [P, C] tensor.  rows [R][C] fp32 / bf16 /
 * fp16 = the stacked map rows (several settings: the numbering of the concatenation), tap_rows int32 [P][4] and
 * tap_weights fp32 [P][4] in the tap order of dva_gather_bilinear_taps_anchor, both 16-byte aligned (else
 * DVA_ERR_UNSUPPORTED).  Any C >= 1: 16-byte row accesses when C % (16 / s) == 0 and rows, out and arg are 16-byte
 * aligned, element accesses otherwise; one wavefront per segment.  arg (MAX / MIN, else nullable) uint16 [S][C] = offset
 * of the winning item inside its segment (0xffff: none; segments must own <= 65534 items).
 * _bwd: grad_rows [R][C] in the rows' dtype, WRITTEN (every element once, fp32 accumulation, one rounding; a map row
 * without taps gets 0) = sum over the taps (p, k) with tap_rows[p][k] == r of tap_weights[p][k] * g(p, c), g(p, c) =
 * grad_out[s][c] (SUM), grad_out[s][c] / count_s (MEAN, fp32 true division) or grad_out[s][c] where arg[s][c] == p -
 * seg_ptr[s], else 0 (MAX / MIN), s = seg_of_item[p] (int32 [P], dva_csr_expand); a segmented reduction over the row plan
 * of the 4 P taps (perm int32 [4 P] = taps 4 p + k sorted by map row, row_ptr int32 [R + 1], as dva_row_plan gives them for
 * the flat tap_rows), one wavefront per map row, no float atomics: deterministic.  No [P, C] gradient exists.
 * 4 P, R or S of 2^31 or more return DVA_ERR_UNSUPPORTED. */
int dva_interp_segment_reduce_fwd(const void* rows, const int32_t* tap_rows, const float* tap_weights,
                                  const int64_t* seg_ptr, void* out, void* arg, int64_t S, int64_t P, int64_t R, int32_t C,
                                  int32_t dtype, int32_t reduce, void* stream);
int dva_interp_segment_reduce_bwd(const void* grad_out, const void* arg, const int64_t* seg_ptr, const int32_t* perm,
                                  const int32_t* row_ptr, const float* tap_weights, const int32_t* seg_of_item,
                                  void* grad_rows, int64_t S, int64_t P, int64_t R, int32_t C, int32_t dtype,
                                  int32_t reduce, void* stream);

/* The same backward over the ANCHOR plan of the items (anchors of dva_gather_bilinear_taps_anchor; perm int32 [P] = items
 * sorted by anchor, row_ptr int32 [n_anchors + 1], as dva_row_plan gives them): S fp32 [n_anchors][4][C], WRITTEN, =
 * sum over the items p of anchor a of tap_weights[p][k] * g(p, c) -- dva_anchor_rows_sum with g evaluated on the fly, P keys
 * instead of 4 P and every gradient row of a segment read once per item; dva_anchor_combine turns S into the fp32 map
 * gradient.  fp32 / bf16 with C / (16 / s) a power of two <= 64 and 16-byte aligned grad_out, arg, tap_weights and S;
 * anything else (fp16 among it) returns DVA_ERR_UNSUPPORTED: the caller takes dva_interp_segment_reduce_bwd.  row_ptr may
 * point into the plan (a range of images).
 * _fixup: the items of the dummy anchor (row_ptr[dummy] .. row_ptr[dummy + 1] of the whole plan), tap by tap in plan order
 * into grad_rows fp32 [R][C] after dva_anchor_combine; one block, no atomics: deterministic. */
int dva_interp_anchor_rows_sum(const void* grad_out, const void* arg, const int64_t* seg_ptr, const int32_t* perm,
                               const int32_t* row_ptr, const float* tap_weights, const int32_t* seg_of_item, float* S,
                               int64_t n_anchors, int64_t P, int32_t C, int32_t dtype, int32_t reduce, void* stream);
int dva_interp_anchor_fixup(const void* grad_out, const void* arg, const int64_t* seg_ptr, const int32_t* perm,
                            const int32_t* row_ptr, const int32_t* tap_rows, const float* tap_weights,
                            const int32_t* seg_of_item, float* grad_rows, int64_t dummy, int64_t P, int32_t C,
                            int32_t dtype, int32_t reduce, void* stream);

/* Bilinear gather with the reference's border-replicate semantics (image.py:105-170):
 * q = coord * (H, W) + 0.5 in the 1-padded map; 4 taps floor(q), floor(q+1); weights |prod(q - opposite)|.
 * coords fp32 [P,2] = (y, x) in [0,1]; the image of atom p comes from packed_idx (its x,y unused). */
int dva_gather_bilinear_fwd(const void* x, const void* packed_idx, const float* coords, void* out,
                            int64_t n_atoms, int32_t B, int32_t H, int32_t W, int32_t C,
                            int32_t dtype, void* stream);
int dva_gather_bilinear_bwd(const void* grad_out, const void* packed_idx, const float* coords,
                            float* grad_x, int64_t n_atoms, int32_t B, int32_t H, int32_t W,
                            int32_t C, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * DeepViewAgg view attention.  Replaces the tail of GroupBimodalCSRPool.forward /
 * QKVBimodalCSRPool.forward (modules/multimodal/pooling.py:284-300, :514-530):
 *   att  = segment_softmax_csr(compat, ptr, scaling)                       [V,G]
 *   pool = segment_csr(val * expand_group_feat(att), ptr, 'sum')            [N,C]
 *   gate = tanh(relu(w * segment_csr(compat, ptr, 'max') + b))  (Gating, pooling.py:690-715)
 *   out  = pool * expand_group_feat(gate)
 * expand_group_feat (pooling.py:737-755): group g owns floor(C/G) (+1 for the first C mod G) channels.
 * gate_w / gate_b nullable together (gating=False): out = pool.
 * Saved for backward / save_last: att [V,G], gate [N,G], amax int32 [N,G] (row of the group max,
 * -1 for unseen points).  n_views = ptr[n_points] (used to size the launch geometry only).
 * algo: 0 = auto, 1 = generic kernels (any C, G), 2 = fused wavefront-team kernels (needs
 * C*s % 16 == 0 with C*s/16 a power of two <= 64, G a power of two dividing C with whole 16-byte
 * lanes per group; DVA_ERR_UNSUPPORTED otherwise).
 * ------------------------------------------------------------------------------------------ */
int dva_view_attention_fwd(const void* val, const float* compat, const int64_t* ptr,
                           const float* gate_w, const float* gate_b, void* out, float* att,
                           float* gate, int32_t* amax, int64_t n_points, int64_t n_views, int32_t C,
                           int32_t G, int32_t scaling, float eps, int32_t dtype, int32_t algo,
                           void* stream);

/* grad_val [V,C] (dtype), grad_compat [V,G] fp32, grad_gate_wb fp32[2*G] (caller-zeroed; atomically
 * accumulated: first G = d/dw, last G = d/db; nullable when gating is off). */
int dva_view_attention_bwd(const void* grad_out, const void* val, const float* compat,
                           const float* att, const float* gate, const int32_t* amax,
                           const int64_t* ptr, const float* gate_w, const float* gate_b,
                           void* grad_val, float* grad_compat, float* grad_gate_wb,
                           int64_t n_points, int64_t n_views, int32_t C, int32_t G, int32_t scaling,
                           int32_t dtype, int32_t algo, void* stream);

/* Same maths with the view gather fused in: the value of view v is rows[row_idx[v], :]
 * (rows = [R, C] value map, e.g. E_mod applied at feature-map level; DESIGN.md "E_mod hoisting").
 * Replaces image.py:1285 + pooling.py:284-300 in one pass: no [V, C] tensor is materialised.
 * Backward: grad_rows fp32 [R, C] non-NULL = scatter-add with atomics (caller-zeroed);
 * grad_rows NULL = only grad_compat / grad_gate_wb are produced and the caller obtains the rows
 * gradient from dva_view_gather_rows_grad (segmented reduction, deterministic, faster).
 * view_rec (nullable, fp32 [n_views, rec_stride], rec_stride >= G + 1, a multiple of 8 keeps one record
 * per 32-byte sector): per view, word 0 = point id (int32 bits), words 1..G = gate * attention per
 * group -- everything dva_view_gather_rows_grad needs about a view in one place. */
int dva_view_gather_attention_fwd(const void* rows, const int32_t* row_idx, const float* compat,
                                  const int64_t* ptr, const float* gate_w, const float* gate_b,
                                  void* out, float* att, float* gate, int32_t* amax,
                                  int64_t n_points, int64_t n_views, int32_t C, int32_t G,
                                  int32_t scaling, float eps, int32_t dtype, int32_t algo,
                                  void* stream);
int dva_view_gather_attention_bwd(const void* grad_out, const void* rows, const int32_t* row_idx,
                                  const float* compat, const float* att, const float* gate,
                                  const int32_t* amax, const int64_t* ptr, const float* gate_w,
                                  const float* gate_b, float* grad_rows, float* grad_compat,
                                  float* grad_gate_wb, float* view_rec, int32_t rec_stride,
                                  int64_t n_points, int64_t n_views, int32_t C, int32_t G,
                                  int32_t scaling, int32_t dtype, int32_t algo, void* stream);

/* Which kernels a view-attention call of this shape runs (host only: nothing is launched, no device is touched): the
 * answer of the geometry rule the four entries above dispatch on.  Returns 1 = the wavefront-team kernels, with *lpr =
 * lanes per view row (C / 4 for fp32, C / 8 for bf16 / fp16) and *rows = view rows in flight per team, which shrinks
 * with the average segment n_views / n_points; 0 = the generic kernels (*lpr = *rows = 0); DVA_ERR_INVALID otherwise.
 * (lpr, rows) in {(8, 8), (16, 4), (8, 4), (16, 2)} are compiled instances, every other pair takes the instance with
 * a run-time geometry.  A call whose val / rows, out, grad_out or grad_val pointer is no multiple of 16 bytes, or
 * whose algo is 1, runs the generic kernels whatever the shape. */
int dva_view_attention_geometry(int32_t C, int32_t G, int64_t n_points, int64_t n_views, int32_t dtype, int32_t* lpr,
                                int32_t* rows);

/* Transposed view of a row index (views grouped by the feature-map row they read): the backward of
 * the gather in image.py:1285 (index_select -> index_add) as a CSR over rows.
 * row_idx int32 [n_views] with values in [0, n_rows).  Outputs: perm int32 [n_views] (view ids
 * ordered by row, original order inside a row: stable radix sort), row_ptr int32 [n_rows+1],
 * counts int32 [n_rows] (nullable) = views per row.  n_views, n_rows < 2^31. */
int64_t dva_row_plan_workspace_bytes(int64_t n_views, int64_t n_rows);
int dva_row_plan(const int32_t* row_idx, int64_t n_views, int64_t n_rows, int32_t* perm,
                 int32_t* row_ptr, int32_t* counts, void* workspace, int64_t workspace_bytes,
                 void* stream);

/* The row plan SPLIT in two (round 5; 512 < n_rows <= 2^18, otherwise DVA_ERR_UNSUPPORTED and the caller keeps dva_row_plan):
 * a two-pass stable MSD radix partition (digits key >> 9 | key & 511, tiles of 4096 views) whose offset tables are built
 * from the row keys alone -- dva_plan_split_build: row_ptr int32 [n_rows + 1], counts int32 [n_rows] (nullable), identical to
 * dva_row_plan's, and `tables` (dva_plan_split_table_bytes; kept by the caller until the backward); scratch: 2 n_views bytes,
 * free afterwards -- and whose two scatter passes move the 16-BYTE VIEW RECORDS of the attention backward themselves --
 * dva_plan_split_sort_records: rec [n_views][16] in view order -> rec_sorted in plan order (record i = plan entry i, views of
 * a row in view order, word 3 of a record = its row key), through buf [n_views][16]; rec_sorted may be rec (or NULL: pass A only, see dva_plan_split_rows_grad); row_idx NULL: word 3
 * of the records already holds the row key (dva_chain_attn_bwd writes it there).  The rows gradient
 * (dva_view_gather_rows_grad_rec16_to with perm = NULL) then streams its records: no permutation exists, no random 16-byte
 * fetch per view.  Replaces the index_add of core/multimodal/image.py:1262-1287's backward like dva_row_plan. */
int64_t dva_plan_split_table_bytes(int64_t n_views, int64_t n_rows);
int dva_plan_split_build(const int32_t* row_idx, int64_t n_views, int64_t n_rows, int32_t* row_ptr, int32_t* counts,
                         void* tables, int64_t tables_bytes, void* scratch, int64_t scratch_bytes, void* stream);
/* dva_mapping_row_index + dva_plan_split_build in one call for an EXACT mapping (one atom per view, so no atom_ptr): one
 * kernel writes the row keys and counts their high digit, the rest of the build is dva_plan_split_build's.  row_idx int32
 * [n_views], row_ptr, counts (nullable), tables and scratch as there, n_rows = B * H * W; every output is byte for byte
 * what the two calls leave.  Refuses what either of them refuses, and a pixels pointer that is not aligned to one (x, y)
 * pair (DVA_ERR_UNSUPPORTED: the pair is one load). */
int dva_mapping_row_index_split(const int64_t* images, const void* pixels, int32_t pix_bytes, double ratio,
                                int64_t n_views, int32_t B, int32_t H, int32_t W, int32_t* row_idx, int32_t* row_ptr,
                                int32_t* counts, void* tables, int64_t tables_bytes, void* scratch, int64_t scratch_bytes,
                                void* stream);
int dva_plan_split_sort_records(const int32_t* row_idx, const void* rec, int64_t n_views, int64_t n_rows,
                                const int32_t* row_ptr, const void* tables, int64_t tables_bytes, void* buf,
                                void* rec_sorted, void* stream);
/* The rows gradient straight from BUCKET-ordered records, without pass B: dva_plan_split_sort_records with rec_sorted =
 * NULL runs pass A only (view order -> bucket order, into buf); then ONE workgroup per bucket of 512 map rows keeps their C
 * fp32 sums in its registers, ranks and stages the bucket's tiles in LDS like pass B and consumes the staged records where
 * they lie (the 16 bytes per view pass B writes and the rows gradient reads again never exist).  grad_rows [n_rows][C]
 * bf16, written; deterministic; a row is summed by one lane team in view order (dva_view_gather_rows_grad_rec16_to splits
 * it over 8 lane slots: the two agree to fp32 rounding).  bf16 / bf16 or fp16 / fp16 (fp32 sums, one rounding), C in
 * {32, 64}, G in {1, 2, 4}; otherwise
 * DVA_ERR_UNSUPPORTED (the caller runs pass B and dva_view_gather_rows_grad_rec16_to).
 * fp32 / fp32 (round 6; the reference's default arithmetic, models/base_model.py:244,381): bucket_rec = the 32-BYTE records
 * of dva_chain_attn_bwd_f32 in bucket order, from dva_plan_split_sort_records32 -- pass A on {point | 4 fp32 weights | 3 pad
 * words} records, row_idx required, the row key written into word 7 of every record; buf [n_views][32] -- grad_out fp32
 * [N][C], grad_rows fp32 [n_rows][C]; C in {32, 64}. */
int dva_plan_split_sort_records32(const int32_t* row_idx, const void* rec, int64_t n_views, int64_t n_rows,
                                  const void* tables, int64_t tables_bytes, void* buf, void* stream);
int dva_plan_split_rows_grad(const void* grad_out, const void* bucket_rec, int64_t n_views, int64_t n_rows,
                             const void* tables, int64_t tables_bytes, void* grad_rows, int32_t C, int32_t G, int32_t dtype,
                             int32_t out_dtype, void* stream);

/* grad_rows[r, c] = sum over the views v of row r of grad_out[p(v), c] * gate[p(v), g(c)] *
 * att[v, g(c)]  (written, not accumulated; fp32 [n_rows, C]).  view_point int32 [n_views] = point of
 * every view (dva_csr_expand); gate nullable (no gating); grad_out [n_points, C] in dtype.
 * With view_rec (from dva_view_gather_attention_bwd) att / gate / view_point are not read. */
int dva_view_gather_rows_grad(const void* grad_out, const float* att, const float* gate,
                              const int32_t* view_point, const int32_t* perm, const int32_t* row_ptr,
                              const float* view_rec, int32_t rec_stride, float* grad_rows,
                              int64_t n_rows, int64_t n_views, int32_t C, int32_t G, int32_t dtype,
                              void* stream);

/* The same reduction over packed 16-byte view records {int32 point | 4 x bf16 weight | pad} (dva_chain_attn_bwd):
 * bf16 grad_out, G in {1, 2, 4}, C / 8 a power of two <= 64, (C / G) % 8 == 0. */
/* (perm may be NULL: the records then lie in plan order -- record i belongs to plan entry i -- as
 * dva_plan_split_sort_records leaves them.) */
/* The output dtype is chosen by the caller: out_dtype = DVA_F32 (fp32 [n_rows, C] as above) or the 2-byte dtype of grad_out
 * (DVA_BF16 / DVA_F16) -- the summed row is
 * rounded once where it is summed, for maps that are bf16 anyway (the gradient autograd hands on has the map's dtype:
 * core/multimodal/image.py:1262-1287 is an index_add in the map's dtype); no fp32 [n_rows, C] tensor, no conversion pass. */
int dva_view_gather_rows_grad_rec16_to(const void* grad_out, const int32_t* perm, const int32_t* row_ptr,
                                       const void* view_rec16, void* grad_rows, int32_t out_dtype, int64_t n_rows,
                                       int64_t n_views, int32_t C, int32_t G, int32_t dtype, void* stream);

/* Backward of a gather over the row plan (dva_row_plan): grad_rows[r, :] = sum over the plan entries e of row r
 * of weights[e] * grad_out[e >> atom_shift, :]  (fp32 [n_rows, C], written, not accumulated; deterministic).
 * Nearest gather: entries = atoms (weights NULL, atom_shift 0) -- dva_gather_nearest_bwd without atomics.
 * Bilinear gather: entries = the 4 corner taps of every atom from dva_gather_bilinear_taps (atom_shift 2);
 * n_atoms = number of ENTRIES. */
int dva_gather_rows_sum(const void* grad_out, const int32_t* perm, const int32_t* row_ptr,
                        const float* weights, int32_t atom_shift, float* grad_rows, int64_t n_rows,
                        int64_t n_atoms, int32_t C, int32_t dtype, void* stream);
/* The bilinear backward over the ANCHOR plan (3 x fewer sorted keys, every gradient row read once instead of four
 * times): anchors int32 [n_atoms] from dva_gather_bilinear_taps_anchor = the cell (top, left) of the view's 2 x 2 tap
 * block on the replication-padded grid, (img (H + 1) + top) (W + 1) + left; views without that structure carry the
 * dummy anchor B (H + 1) (W + 1).  Plan = dva_row_plan(anchors, B (H + 1) (W + 1) + 1).
 *   dva_anchor_rows_sum: S fp32 [n_anchors][4][C] (written) = per anchor and tap the weighted sum of grad_out rows;
 *   dva_anchor_combine:  grad_rows fp32 [B*H*W][C] (written) from S (pass the S of the first B (H+1) (W+1) anchors);
 *   dva_anchor_fixup:    += the taps of the dummy-anchor views (fp32 atomics; none on real data). */
int dva_gather_bilinear_taps_anchor(const void* packed_idx, const float* coords, int64_t n_atoms, int32_t B,
                                    int32_t H, int32_t W, int32_t* rows, float* weights, int32_t* anchors,
                                    void* stream);
/* The taps of n_settings <= 8 SETTINGS (feature maps of different sizes; the outputs of dva_gather_bilinear_taps_anchor per
 * setting) as ONE gather over the stacked map rows, in a given view order -- the reference concatenates the materialised
 * [V_s, C] tensors of the settings and indexes the result with view_cat_sorting (core/multimodal/image.py:1549-1588,
 * modules/multimodal/modules.py:514-525); here the taps are concatenated instead and no [V, C] tensor exists.
 * tap_rows / tap_weights / anchors: HOST arrays of n_settings device pointers; n_views / n_rows / n_anchors: HOST arrays
 * (views, map rows B H W, anchors B (H + 1) (W + 1) of every setting).  order int64 [n_views_total] (device, nullable =
 * identity): view i of the result = view order[i] of the concatenation.  Tap rows are offset by the rows of the settings
 * before, anchors by their anchors; a setting's dummy anchor (= its n_anchors) becomes the common one (= sum n_anchors). */
int dva_bilinear_taps_cat(int32_t n_settings, const void* const* tap_rows, const void* const* tap_weights,
                          const void* const* anchors, const int64_t* n_views, const int64_t* n_rows,
                          const int64_t* n_anchors, const int64_t* order, int64_t n_views_total, int32_t* rows_out,
                          float* weights_out, int32_t* anchors_out, void* stream);
int dva_anchor_rows_sum(const void* grad_out, const int32_t* perm, const int32_t* row_ptr, const float* weights,
                        float* S, int64_t n_anchors, int64_t n_views, int32_t C, int32_t dtype, void* stream);
int dva_anchor_combine(const float* S, float* grad_rows, int32_t B, int32_t H, int32_t W, int32_t C, void* stream);
int dva_anchor_fixup(const void* grad, const int32_t* rows, const float* weights, const int32_t* anchors,
                     float* grad_rows, int64_t n_atoms, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype,
                     void* stream);
/* The same two steps for the fused bilinear path (csrc/chain_emod.hip): the rows are dy_a bf16 [V][C] in position order
 * and the BatchNorm_a backward dz_a = G dy_a - K1 - K2 z_a (bn_a fp32 [4][C] = mean | invstd | gamma | beta,
 * sm_a fp32 [2][C] = S1 / M | S2_hat / M of dva_bn_bwd_consts, natural channel order) is folded into the scatter,
 * replacing the in-place pass dva_emod_bwd(stage 1).  C a multiple of 32.  dva_anchor_rows_sum_bn takes z either as
 * z_a bf16 [V][C] (applied row by row; Y, tap_rows NULL) or, z_a NULL, as Y bf16 [R][C] (position order) + tap_rows
 * int32 [V][4]: all views of an anchor interpolate the same four rows of Y, so their z term is a 4 x 4 Gram matrix of
 * the tap weights (accumulated in the kernel) times those rows -- one random row per view instead of two. */
int dva_anchor_rows_sum_bn(const void* dy_a, const void* z_a, const float* bn_a, const float* sm_a, const int32_t* perm,
                           const int32_t* row_ptr, const float* weights, const int32_t* tap_rows, const void* Y,
                           float* S, int64_t n_anchors, int64_t n_views, int32_t C, void* stream);
int dva_anchor_fixup_bn(const void* dy_a, const void* z_a, const float* bn_a, const float* sm_a, const int32_t* rows,
                        const float* weights, const int32_t* anchors, float* grad_rows, int64_t n_atoms, int32_t B,
                        int32_t H, int32_t W, int32_t C, void* stream);
/* rows int32 [4 * n_atoms], weights fp32 [4 * n_atoms]: corner rows (tl, tr, bl, br) of the [B*H*W, C] map and
 * bilinear weights of every atom, exactly the taps of dva_gather_bilinear_fwd (image.py:138-165). */
int dva_gather_bilinear_taps(const void* packed_idx, const float* coords, int64_t n_atoms, int32_t B,
                             int32_t H, int32_t W, int32_t* rows, float* weights, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Fused DeepSetFeat (+ score Linear) chain over the V views, exact fp32, forward and backward.
 * Replaces, for map_encoder='DeepSetFeat' (pool='max', fusion='concatenation', nc_inner=32,
 * in_map=8), the torch composition of modules/multimodal/pooling.py:658-669 + :282 (MLP blocks =
 * Linear(no bias) -> BatchNorm1d -> LeakyReLU(0.2), core/common_modules/base_modules.py:38-48).
 * Each entry is one pass between two batch-statistics barriers; "a_k" are PRE-BatchNorm
 * activations [V,32] fp32, "bn" arrays are fp32 [4][32] = mean | invstd | gamma | beta,
 * "stats" are caller-zeroed double[64] = per-channel sum | sum of squares (forward) or
 * S1 = sum dz | S2 = sum dz*a_hat (backward), "sm" are fp32 [2][32] = S1/M | S2/M (zeros in eval).
 * The layer passes run on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, operands from registers).
 * act_dtype = STORAGE type of the [V,32] activation / gradient tensors (the `void*` arguments):
 * DVA_F32, or DVA_BF16 (what the reference keeps under torch.autocast).  Arithmetic,
 * weights, statistics, per-point tensors (addend, pooled, dpooled, dt) and the scores stay fp32.
 * ------------------------------------------------------------------------------------------ */
/* group_of_row[r] = g for ptr[g] <= r < ptr[g+1] (dense expansion of CSR pointers, int32). */
int dva_csr_expand(const int64_t* ptr, int64_t n_groups, int32_t* group_of_row, void* stream);
/* a1 = x_map.Wa^T (F = 8). stats_only: statistics of a1; else a2 = leaky(BN1(a1)).Wb^T written
 * with its statistics (mlp_elt_1, pooling.py:649-650). */
int dva_deepset_fwd_first(const float* x_map, const float* Wa, const float* bn1, const float* Wb,
                          void* a2, double* stats, int64_t V, int32_t F, int32_t stats_only,
                          int32_t act_dtype, void* stream);
/* pooled[p] = max_v leaky(BN(a[v])) over the point's views (first row on ties; 0 / arg -1 for
 * unseen points): segment_csr(x, csr, 'max') of pooling.py:660,:628.  n_views = ptr[N] (launch-geometry hint:
 * lanes per point follow the average segment length; <= 0: default). */
int dva_deepset_segmax(const void* a, const float* bn, const int64_t* ptr, float* pooled,
                       int32_t* arg, int64_t N, int64_t n_views, int32_t act_dtype, void* stream);
/* a_out[v] = leaky(BN_in(a_in[v])).W^T (+ addend[group_of_row[v]]) with statistics of a_out.
 * The addend carries the set half of the concatenation: cat(x, x_set).Wc^T = x.WcA^T + (x_set.WcB^T)[p]
 * (pooling.py:666-668).  bn_in == NULL: the input is used raw (set MLP on the pooled features). */
int dva_deepset_fwd_layer(const void* a_in, const float* bn_in, const float* W, const float* addend,
                          const int32_t* group_of_row, void* a_out, double* stats, int64_t V,
                          int32_t act_dtype, void* stream);
/* out[v, g] = leaky(BN(a[v])).Ws[g] + bs[g], G <= 32 (E_score, pooling.py:258,:282; also Q/K). */
int dva_deepset_fwd_score(const void* a, const float* bn, const float* Ws, const float* bs,
                          float* compat, int64_t V, int32_t G, int32_t act_dtype, void* stream);
int dva_deepset_bwd_score(const float* dcompat, const void* a, const float* bn, const float* Ws,
                          void* dz, float* dWs, float* dbs, double* st, int64_t V, int32_t G,
                          int32_t act_dtype, void* stream);
/* Backward of one layer: da_L = BN-backward(dz_L), dW_L += da_L^T x_L, dx = da_L.W_L;
 * out = dx (raw_out) or dz_prev = dx*leaky'(BN_prev(a_prev)) with S1/S2 of BN_prev in st_prev;
 * dt[group_of_row[v]] += da_L[v] (nullable). prev_is_xmap: a_prev is x_map [V,8] and the previous
 * activation is recomputed as x_map.Wa^T. dW / dt are caller-zeroed fp32, atomically accumulated.
 * bn_prev == NULL (with raw_out): the layer input is a_prev itself (no BatchNorm / activation).
 * first_grad (nullable; DVA_BF16 storage, prev_is_xmap, !raw_out, dt NULL): caller-zeroed fp32[520] =
 * P[32][8] | Q[32][8] | SX[8] with P = sum_v dz_prev x^T, Q = sum_v a_prev_hat x^T, SX = sum_v x, from
 * which the first layer's weight gradient follows without another pass (BN-backward is linear in the
 * statistics): dWa[n][f] = gamma invstd (P - (S1/M)[n] SX[f] - (S2/M)[n] Q)[n][f].  `out` is then not
 * written (may be NULL) and dva_deepset_bwd_first is not needed. */
int dva_deepset_bwd_layer(const void* dz_L, const void* a_L, const float* bn_L, const float* sm_L,
                          const float* W_L, const void* a_prev, const float* Wa, const float* bn_prev,
                          void* out, float* dW, double* st_prev, float* dt,
                          const int32_t* group_of_row, float* first_grad, int64_t V,
                          int32_t prev_is_xmap, int32_t raw_out, int32_t act_dtype, void* stream);
/* dz2 = (dcat + [arg[p]==v] dpooled[p]) * leaky'(BN2(a2)): joins the max-pool path (segment max
 * backward routes to the arg row only) with the direct path; S1/S2 of BN2 in st. */
int dva_deepset_bwd_max(const void* dcat, const void* a2, const float* bn2, const int32_t* arg,
                        const float* dpooled, const int32_t* group_of_row, void* dz2, double* st,
                        int64_t V, int32_t act_dtype, void* stream);
/* dWa[n][j] += sum_v BN1-backward(dz1)[v][n] * x_map[v][j]. */
int dva_deepset_bwd_first(const void* dz1, const float* x_map, const float* Wa, const float* bn1,
                          const float* sm1, float* dWa, int64_t V, int32_t F, int32_t act_dtype,
                          void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Weighted BatchNorm1d + LeakyReLU over the R rows of a feature map: one MLP block of E_mod
 * (pooling.py:245,275; core/common_modules/base_modules.py:38-48) evaluated on the map rows instead of
 * the V gathered views.  counts int32 [R] = views per row (dva_row_plan / dva_gather_row_index): the
 * batch statistics over the views are the statistics over the rows weighted by counts.  counts NULL = every
 * row counts once: plain BatchNorm1d + LeakyReLU over [R, C] (used for E_mod on materialised [V, C] views).
 * y / out / grad_* are [R, C] in dtype; sums = caller-zeroed double[2*C]; bn = fp32 [4][C] =
 * mean | invstd | gamma | beta; sm = fp32 [2][C] = S1/n | S2/n (zeros when running statistics are used).
 * ------------------------------------------------------------------------------------------ */
/* sums = sum_r counts_r y_r | sum_r counts_r y_r^2 */
int dva_rowbn_stats(const void* y, const int32_t* counts, double* sums, int64_t R, int32_t C,
                    int32_t dtype, void* stream);
/* out = leaky(gamma (y - mean) invstd + beta), negative slope `slope` */
int dva_rowbn_apply(const void* y, const float* bn, void* out, int64_t R, int32_t C, float slope,
                    int32_t dtype, void* stream);
/* sums = S1 | S2 with dz = grad_out leaky'(z): S1 = sum_r dz_r, S2 = sum_r dz_r a_r (a = normalised y);
 * also d beta = S1, d gamma = S2. */
int dva_rowbn_bwd_stats(const void* grad_out, const void* y, const float* bn, double* sums, int64_t R,
                        int32_t C, float slope, int32_t dtype, void* stream);
/* grad_y = gamma invstd (dz - counts (S1/n) - counts a (S2/n)) */
int dva_rowbn_bwd_apply(const void* grad_out, const void* y, const int32_t* counts, const float* bn,
                        const float* sm, void* grad_y, int64_t R, int32_t C, float slope, int32_t dtype,
                        void* stream);

/* ------------------------------------------------------------------------------------------ *
 * E_mod on the map rows as fused row kernels (csrc/emod_rows.hip): the two-block MLP [Linear (no bias) ->
 * weighted BatchNorm1d -> LeakyReLU] x 2 in train mode on bf16 rows, widths 32 or 64, matrix products on
 * v_mfma_f32_32x32x16_bf16.  The Linear of a block, the BatchNorm + activation of the block before it and the
 * statistics of the BatchNorm after it are one pass; dva_bn_finalize / dva_bn_bwd_consts run between the
 * passes, dva_rowbn_apply is the last forward pass and dva_rowbn_bwd_stats the first backward pass.  All
 * rows bf16, contiguous, 16-byte aligned; W fp32 [C_out][C_in] (rounded to bf16 in the kernel); bn / bn_in
 * fp32 [4][C] as above; counts int32 [R] nullable; (R + 32) * 128 bytes must stay below 2^32
 * (DVA_ERR_UNSUPPORTED otherwise, as for a width other than 32 / 64).  max_blocks > 0 caps the launch grid
 * (0 = the default grid); dva_emod_rows_grid tells the grid a call will use.
 * ------------------------------------------------------------------------------------------ */
int dva_emod_rows_grid(int64_t R, int32_t backward, int32_t max_blocks);
/* y [R, C_out] = bf16(op(in) W^T), op = identity (bn_in NULL) or bf16(leaky(BatchNorm(in))) with the
 * constants bn_in [4][C_in] and negative slope `slope`; sums (caller-zeroed double[2 * C_out]) += sum_r
 * counts_r y_r | sum_r counts_r y_r^2 of the rounded y. */
int dva_emod_rows_fwd(const void* in, const float* W, const float* bn_in, const int32_t* counts, void* y,
                      double* sums, int64_t R, int32_t C_in, int32_t C_out, float slope, int32_t max_blocks,
                      void* stream);
/* One block backwards.  dy [R, C_out] = bf16 of dva_rowbn_bwd_apply's formula from grad_in, y, bn, sm, counts
 * and `slope` (never stored); dw_ws fp32 [grid][C_out][C_in]: every block writes the partial sum of
 * dy^T op(x_in) over its rows; grad_x [R, C_in] = bf16(dy W), nullable when bn_in is NULL (then no product
 * is formed).  bn_in non-NULL: op(x_in) = bf16(leaky(BatchNorm(x_in))) with slope_in, and sums (caller-zeroed
 * double[2 * C_in]) += S1 | S2 of dz = grad_x leaky'(z_in) as dva_rowbn_bwd_stats defines them. */
int dva_emod_rows_bwd(const void* grad_in, const void* y, const float* bn, const float* sm, const int32_t* counts,
                      const void* x_in, const float* bn_in, const float* W, void* grad_x, float* dw_ws,
                      double* sums, int64_t R, int32_t C_in, int32_t C_out, float slope, float slope_in,
                      int32_t max_blocks, void* stream);
/* out_a[i] = sum_p ws_a[p][i] (i < n_a, p < parts_a), the same for b: the partials in a fixed order (two
 * calls give the same bits).  n_a is a multiple of 16. */
int dva_emod_rows_dw_reduce(const float* ws_a, int32_t n_a, int32_t parts_a, float* out_a, const float* ws_b,
                            int32_t n_b, int32_t parts_b, float* out_b, void* stream);

/* BatchNorm1d bookkeeping between two passes (one launch): sums = double[2*C] (sum | sum of squares over m
 * rows) -> bn = fp32 [4][C] = mean | invstd | gamma | beta.  training: batch statistics (biased variance),
 * running_mean / running_var (nullable pair) updated with `momentum` using the unbiased variance,
 * *num_batches_tracked += 1 (nullable); else the running statistics are used.  gamma / beta nullable
 * (no affine).  nn.BatchNorm1d as wrapped by FastBatchNorm1d (base_modules.py:131-156). */
int dva_bn_finalize(const double* sums, double m, float* running_mean, float* running_var,
                    int64_t* num_batches_tracked, const float* gamma, const float* beta, float momentum,
                    float eps, int32_t training, int32_t C, float* bn, void* stream);
/* out[i] = (float)(in[i] * scale): S1/M | S2/M tables of the BatchNorm backward. */
int dva_scale_f64(const double* in, double scale, float* out, int32_t n, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Recompute chain (bf16 matrix cores): GroupBimodalCSRPool with map_encoder = DeepSetFeat(8 -> 32, max,
 * concatenation) for a lazily gathered (nearest, exact mapping) bf16 value map -- modules/multimodal/
 * pooling.py:263-315 + :658-669 -- without any [V, .] activation tensor: every pass re-evaluates the
 * per-view chain  x_map -> L1 -> L2 -> (+ set branch of the point) -> L5 -> L6 -> scores  from the 32-byte
 * mapping features inside the kernel (v_mfma_f32_32x32x16_bf16, layers chained in registers).  Train-mode
 * BatchNorm keeps its global barriers: one statistics pass per V-level BatchNorm layer (forward) and per
 * BatchNorm-backward (backward); in eval mode the forward is dva_chain_stats2 (set pooling) +
 * dva_chain_attn_fwd.  All backward statistics ("stats" of the *_bwd entries) are S1 = sum dy | sum dy z with z the RAW
 * layer output: S2 = sum dy z_hat = invstd (sum dy z - mean S1) is the caller's one-liner.  Operands are rounded to bf16 (what torch.autocast(bfloat16) feeds the reference's
 * Linear layers), accumulation / BatchNorm / softmax / statistics are fp32 / fp64.
 * Views are processed in TILES of <= 32 consecutive views made of whole points (points with more than 32
 * views: consecutive fragment tiles); "bn" arrays are fp32 [4][32] = mean | invstd | gamma | beta
 * (dva_bn_finalize), "stats" caller-zeroed double[64].  All per-point outputs are only written for points
 * that have views: the caller zero-fills them.
 * ------------------------------------------------------------------------------------------ */
/* ops: DVA_CHAIN_OPS_BYTES (32 KiB) device buffer receiving the weight operands (18 bf16 matrix-core operand
 * blocks + an fp32 copy of the forward ones, from which the kernels build BatchNorm-folded operands
 * bf16(0.6 gamma invstd W) for the layers whose raw output a pass does not need).  W1 [32][8], W2 [32][32],
 * W5 [32][ld5] (the first 32 columns: the per-view half of the concatenation layer), W6 [32][32], Ws [G][32], G <= 4 -- or
 * G = 32: the last layer is the KEY layer of QKVBimodalCSRPool (dva_chain_keys_compat; its backward runs
 * through dva_chain_score_stats_keys / dva_chain_bwd_layer6_keys). */
#define DVA_CHAIN_OPS_BYTES (18 * 64 * 16 + 7 * 64 * 32)
int dva_chain_prep(const float* W1, const float* W2, const float* W5, int32_t ld5, const float* W6,
                   const float* Ws, int32_t G, void* ops, void* stream);
/* BatchNorm bookkeeping of one chain layer: dva_bn_finalize (C = 32) + a fifth table row, bn fp32 [5][32] =
 * mean | invstd | gamma | beta | shift, shift = the 0.6-scaled constant the layer's product starts from.  Plain layer
 * (W = NULL): 0.6 (beta - mean G).  Layer evaluated with BatchNorm folded into its operand, training: W fp32 [32][ldw]
 * (first K columns), sum_a fp64 [K] = sum over the m rows of the layer's INPUT; shift = 0.6 beta - bf16(0.6 G W) .
 * (sum_a / m): the folded product keeps the exact batch mean.  Every dva_chain_* kernel takes these 5-row tables. */
int dva_chain_bn_consts(const double* sums, double m, float* running_mean, float* running_var,
                        int64_t* num_batches_tracked, const float* gamma, const float* beta, float momentum, float eps,
                        int32_t training, const float* W, int32_t ldw, int32_t K, const double* sum_a, float* bn,
                        void* stream);
/* Tile table of ptr (int64 [n_points + 1]).  chunk_points int64 [n_chunks + 1]: ascending point indices,
 * chunk c = points [chunk_points[c], chunk_points[c + 1]) is tiled independently (first 0, last n_points).
 * count: counts int32 [n_chunks] = tiles per chunk.  build: offsets int64 [n_chunks] = exclusive prefix sum
 * of counts; tiles int32 [sum(counts)][2] = {first view, n_views | fragment << 8} (fragment 0 = whole
 * points, 1 / 2 / 3 = first / middle / last fragment of a point with more than 32 views). */
/* The two host-side steps around count / build as launches: chunk_points[c] = first point whose views start at or
 * after c * views_per_chunk (c = 1 .. n_chunks - 1; [0] = 0, [n_chunks] = n_points); offsets = exclusive prefix sum of
 * counts (n_chunks <= 2^20), n_tiles int32 [1] = the total. */
int dva_chain_tile_chunks(const int64_t* ptr, int64_t n_points, int64_t views_per_chunk, int32_t n_chunks,
                          int64_t* chunk_points, void* stream);
int dva_chain_tile_offsets(const int32_t* counts, int32_t n_chunks, int64_t* offsets, int32_t* n_tiles,
                           void* stream);
int dva_chain_tile_count(const int64_t* ptr, const int64_t* chunk_points, int32_t n_chunks, int32_t* counts,
                         void* stream);
int dva_chain_tile_build(const int64_t* ptr, const int64_t* chunk_points, int32_t n_chunks,
                         const int64_t* offsets, void* tiles, void* stream);
/* moments double[44] (caller-zeroed) += sum_v x | sum_v x_i x_j (i <= j, row-major upper triangle);
 * stats1 double[64] = sum z1 | sum z1^2 of z1 = bf16(W1) x, derived from the moments (exact_w1 != 0: of z1 = W1 x,
 * the first layer of the fp32-class chain dva_chain3_*; the same flag on dva_chain_stats1 / dva_chain_dw1). */
int dva_chain_moments(const float* x_map, int64_t n_views, const float* W1, int32_t exact_w1, double* moments,
                      double* stats1, void* stream);
/* stats double[96] (caller-zeroed) += sum z2 | sum z2^2 | sum a1 (the layer's input: what dva_chain_bn_consts needs
 * for the folded shift); zstar fp32 [N][32] / arg int32 [N][32] = value / first view of the per-point extremum of
 * sign(gamma2) z2 (the view that max-pools a2 = leaky(BN2(z2))). */
int dva_chain_stats2(const float* x_map, const int32_t* view_point, const void* tiles, const int32_t* n_tiles,
                     const void* ops, const float* bn1, const float* gamma2, double* stats, float* zstar,
                     int32_t* arg, int64_t n_views, void* stream);
/* pooled fp32 [N][32] = leaky(BN2(zstar)) for seen points, 0 for unseen ones. */
int dva_chain_pooled(const float* zstar, const float* bn2, const int64_t* ptr, float* pooled, int64_t n_points,
                     void* stream);
/* layer = 5: stats double[96] += sum | sum of squares of z5 = W5a a2 + u[point] (third row untouched); layer = 6: of z6,
 * third row += sum a5 (the layer's input).  u fp32 [N][32] = the per-point half of the concatenation layer
 * (W5b . set features). */
int dva_chain_stats(int32_t layer, const float* x_map, const int32_t* view_point, const float* u,
                    const void* tiles, const int32_t* n_tiles, const void* ops, const float* bn1,
                    const float* bn2, const float* bn5, double* stats, int64_t n_views, int64_t n_points,
                    void* stream);
/* Key layer of QKVBimodalCSRPool on the recompute chain (round 4; reference modules/multimodal/pooling.py:454-547:
 * keys = K(E_map(x_map))): ops prepared by dva_chain_prep with Ws = K.weight [32][32], G = 32.  keys bf16 [V][32] in
 * ACCUMULATOR order: position 16 h + r holds key channel (r & 3) + 8 (r >> 2) + 4 h (the layout of the rows the chain's
 * backward passes hand to each other).
 * The same pass also writes the compatibilities (pooling.py:520-531) compat fp32 [V][4] =
 * scale * sum over the 32 / G key channels of group g of the (bf16-rounded) key * queries[point(v)][.] -- queries fp32 [N][32]
 * in the keys' position order, G in {1, 2, 4} query-key groups (columns >= G are written as 0), 16-byte aligned. */
int dva_chain_keys_compat(const float* x_map, const int32_t* view_point, const float* u, const void* tiles,
                          const int32_t* n_tiles, const void* ops, const float* bn1, const float* bn2, const float* bn5,
                          const float* bn6, const float* key_bias, void* keys, const float* queries, float* compat,
                          int32_t G, float scale, int64_t n_views, int64_t n_points, void* stream);
/* compat fp32 [V][G] = scale * sum over the nc_qk = 32 / G key channels of group g of keys[v] * queries[point(v)]
 * (pooling.py:520-531), keys as dva_chain_keys_compat writes them, queries fp32 [N][32] in the same position order; G in {1, 2, 4}.
 * _bwd: grad_keys bf16 [V][32] (position order; NULL: skipped -- the chain backward builds it in registers),
 * grad_queries fp32 [N][32] (written).  dva_qkv_dquery: grad_queries alone, grad_compat with leading dimension ld >= G
 * (the [V][4] layout of dva_chain_keys_compat / dva_chain_attn_bwd: ld = 4). */
int dva_qkv_compat(const void* keys, const float* queries, const int32_t* view_point, float* compat, int64_t n_views,
                   int32_t G, float scale, void* stream);
int dva_qkv_compat_bwd(const float* grad_compat, const void* keys, const float* queries, const int32_t* view_point,
                       const int64_t* ptr, void* grad_keys, float* grad_queries, int64_t n_points, int64_t n_views,
                       int32_t G, float scale, void* stream);
int dva_qkv_dquery(const float* grad_compat, int32_t ld, const void* keys, const int64_t* ptr, float* grad_queries,
                   int64_t n_points, int64_t n_views, int32_t G, float scale, void* stream);
/* out bf16 [N][C] (caller-zeroed) = gate * sum_v softmax_v(scores) * rows[row_idx[v]]:
 * x_map + rows in -> pooled features out.  rows bf16 [n_rows][C], C in {32, 64, 128, 256, 512},
 * G in {1, 2, 4} with (C / G) % 8 == 0; gate_w / gate_b fp32 [G] nullable together.
 * scores_out (nullable; training): fp32 [V][4] receives the scores E_score(E_map(x_map)) of every view (columns < G),
 * what dva_chain_attn_bwd starts from (16 bytes per view instead of one more chain evaluation). */
int dva_chain_attn_fwd(const float* x_map, const int32_t* view_point, const float* u, const void* tiles,
                       const int32_t* n_tiles, const void* ops, const float* bn1, const float* bn2,
                       const float* bn5, const float* bn6, const float* score_bias, const void* rows,
                       const int32_t* row_idx, const int64_t* ptr, const float* gate_w, const float* gate_b,
                       void* out, float* scores_out, int64_t n_points, int64_t n_views, int64_t n_rows, int32_t C,
                       int32_t G, int32_t scaling, float eps, void* stream);
/* dva_chain_attn_fwd with the element type of rows and out as an argument: dtype DVA_BF16 (= dva_chain_attn_fwd) or
 * DVA_F16 (autocast(float16): fp16 value rows, fp16 pooled features; the scores stay bf16-operand / fp32-accumulator). */
int dva_chain_attn_fwd_dt(const float* x_map, const int32_t* view_point, const float* u, const void* tiles,
                          const int32_t* n_tiles, const void* ops, const float* bn1, const float* bn2,
                          const float* bn5, const float* bn6, const float* score_bias, const void* rows,
                          const int32_t* row_idx, const int64_t* ptr, const float* gate_w, const float* gate_b,
                          void* out, float* scores_out, int64_t n_points, int64_t n_views, int64_t n_rows, int32_t C,
                          int32_t G, int32_t scaling, float eps, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Recompute chain with a per-view E_mod: the fused path of the BILINEAR gather (interpolate=True;
 * reference core/multimodal/image.py:105-170 sparse_interpolation + modules/multimodal/pooling.py:245,275 E_mod per
 * view; csrc/chain_emod.hip).  The first Linear of E_mod commutes with the interpolation and runs on the map rows
 * (caller): Y bf16 [n_rows][C_out] = rows W_a^T in POSITION order (position 32 b + 16 h + r = channel
 * 32 b + (r & 3) + 8 (r >> 2) + 4 h: the 16 channels a lane owns are contiguous).  Per view: the 4 taps
 * tap_rows int32 [V][4] / tap_weights fp32 [V][4] (dva_gather_bilinear_taps) of Y -> z_a -> BatchNorm_a ->
 * LeakyReLU(0.2) -> Linear_b on the matrix cores -> BatchNorm_b -> LeakyReLU = the value of the view.
 * C_out in {32, 64} (dva_emod_prep and the eval form of dva_emod_attn_fwd, z_a = NULL, also 128 and, G = 4, 256), G in {1, 2, 4}.  bn_a / bn_b fp32 [4][C_out] = mean | invstd | gamma | beta (dva_bn_finalize),
 * natural channel order; statistics fp64 [2][C_out] caller-zeroed; tiles / view_point / scores / chain arguments as
 * for the dva_chain_* entries.
 * z_a bf16 [V][C_out] (position order): the interpolated Linear_a output of every view, rounded to bf16 (what the
 * layer's output is under autocast in the reference).  Train mode: written by dva_emod_stats(layer 1), read by every
 * later pass of the step instead of the four taps of Y (those passes ignore Y / tap_rows / tap_weights, which may be
 * NULL).  Eval mode: dva_emod_attn_fwd with z_a = NULL evaluates the taps itself.
 * A C_out outside {32, 64, 128, 256} or a G outside {1, 2, 4} is DVA_ERR_INVALID; a pair of valid ones without kernels
 * (C_out = 256 with G != 4) and a stage a width does not have are DVA_ERR_UNSUPPORTED.  Both return before any launch.
 * ------------------------------------------------------------------------------------------ */
/* eops: 2 * (C_out / 32)^2 * 2 KiB: Linear_b's weight W_b fp32 [C_out][C_out] as bf16 matrix-core operands
 * (forward blocks, then the transposed blocks of the input gradient). */
int dva_emod_prep(const float* Wb, int32_t C_out, void* eops, void* stream);
/* layer 1: z_a (out, nullable) <- bf16(taps of Y), stats += sum z_a | sum z_a^2 of the stored values (eops, bn_a
 * unused);  layer 2: stats += sum z_b | sum z_b^2 from z_a (in). */
int dva_emod_stats(int32_t layer, const void* Y, const int32_t* tap_rows, const float* tap_weights, const void* tiles,
                   const int32_t* n_tiles, const void* eops, const float* bn_a, double* stats, void* z_a,
                   int64_t n_views, int64_t n_rows, int32_t C_out, void* stream);
/* Layer-1 statistics pass of dva_emod_stats in ANCHOR order (round 4): perm = the permutation of the anchor plan
 * (dva_row_plan of the views' anchors, the plan the backward scatters through).  A tile is 32 consecutive plan entries, so
 * neighbouring lanes read the same four rows of Y (cache hits instead of 8 C_out gathered bytes per view); z_a rows are
 * written to their view's position, stats as dva_emod_stats(layer 1).  C_out in {32, 64, 128, 256}; z_a may be NULL. */
int dva_emod_stats1_plan(const void* Y, const int32_t* tap_rows, const float* tap_weights, const int32_t* perm,
                         double* stats, void* z_a, int64_t n_views, int64_t n_rows, int32_t C_out, void* stream);
/* The fused view kernel: x_map + z_a (or, z_a = NULL, the taps of Y) -> out bf16 [N][C_out] (caller-zeroed) =
 * gate * sum_v softmax_v(scores) E_mod(view v); scores_out as dva_chain_attn_fwd. */
int dva_emod_attn_fwd(const float* x_map, const int32_t* view_point, const float* u, const void* tiles,
                      const int32_t* n_tiles, const void* ops, const float* bn1, const float* bn2, const float* bn5,
                      const float* bn6, const float* score_bias, const void* Y, const int32_t* tap_rows,
                      const float* tap_weights, const void* eops, const float* bn_a, const float* bn_b,
                      const int64_t* ptr, const float* gate_w, const float* gate_b, void* out, float* scores_out,
                      const void* z_a, int64_t n_points, int64_t n_views, int64_t n_rows, int32_t C_out, int32_t G,
                      int32_t scaling, float eps, void* stream);
/* Attention + gate backward from the stored scores with E_mod re-evaluated: grad_scores, view_rec, grad_gate_wb as
 * dva_chain_attn_bwd; stats_b += S1 | sum dy_b z_b of the BatchNorm_b backward. */
int dva_emod_attn_bwd(const float* scores, const int32_t* view_point, const void* tiles, const int32_t* n_tiles,
                      const void* Y, const int32_t* tap_rows, const float* tap_weights, const void* eops,
                      const float* bn_a, const float* bn_b, const int64_t* ptr, const float* gate_w,
                      const float* gate_b, const void* grad_out, const void* out, float* grad_scores, void* view_rec,
                      float* grad_gate_wb, double* stats_b, const void* z_a, int64_t n_points, int64_t n_views,
                      int64_t n_rows, int32_t C_out, int32_t G, int32_t scaling, float eps, void* stream);
/* E_mod backward.  stage 2: view_rec + grad_out -> dWb fp32 [C_out][C_out] (caller-zeroed) += the gradient of W_b,
 * da bf16 [V][C_out] (position order) = leaky'(y_a) W_b^T dz_b, stats_a += S1 | sum dy_a z_a  (sm_b = S / M of
 * BatchNorm_b).  stage 1: da <- dz_a = BatchNorm_a backward of da in place (sm_a; C_out <= 64); the gradient of Y follows as
 * dva_gather_rows_sum(da, row plan of tap_rows, tap_weights, atom_shift 2).
 * C_out in {32, 64, 128}.  C_out = 128 ("wide rows", round 4) evaluates stage 2 as two kernels that can also be called
 * on their own: stage 3 = da + stats_a only (dWb may be NULL), stage 4 = dWb only (stats_a may be NULL). */
int dva_emod_bwd(int32_t stage, const void* Y, const int32_t* tap_rows, const float* tap_weights, const void* tiles,
                 const int32_t* n_tiles, const void* eops, const float* bn_a, const float* bn_b, const float* sm_a,
                 const float* sm_b, const void* view_rec, const void* grad_out, void* da, float* dWb, double* stats_a,
                 const void* z_a, int64_t n_points, int64_t n_views, int64_t n_rows, int32_t C_out, int32_t G,
                 void* stream);

/* The arithmetic between two BatchNorm-backward passes as one launch.  stats fp64 [2C] = S1 | S2, bn fp32 [4][C] =
 * mean | invstd | gamma | beta.  do_hat: S2 arrives as sum dy z (raw layer output) and becomes
 * invstd (S2 - mean S1) = sum dy z_hat, in place.  Then sm fp32 [2C] = stats * inv_m, dgamma = S2, dbeta = S1
 * (each nullable). */
int dva_bn_bwd_consts(double* stats, const float* bn, double inv_m, int32_t do_hat, float* sm, float* dgamma,
                      float* dbeta, int32_t C, void* stream);
/* Statistics of the BatchNorm-1 backward from P (stage 2 of dva_chain_bwd_layer): P fp32 [32][20] = sum_v dy1
 * [x_hi (8) | x_lo (8) | 1 | unused (3)]^T; stats fp64 [64] = sum dy1 (= P[:, 16]) | sum dy1 z1 with z1 = bf16(W1) x
 * (= sum_f bf16(W1)[:, f] (P[:, f] + P[:, 8 + f]): z1 is linear in x).  Raw-z form like every other "stats". */
int dva_chain_stats1(const float* P, const float* W1, int32_t exact_w1, double* stats, void* stream);
/* First-layer weight gradient without another view pass: BatchNorm-1 backward is linear in its statistics and
 * z1 = W1 x is linear in x, so dW1 = G1 (P - (S1/M) SX^T - (S2/M) . Q), Q = sum_v z1_hat x^T from the moments.
 * P fp32 [32][20] (dva_chain_bwd_layer stage 2: x_map as hi | lo columns), mom fp64 [44] (dva_chain_moments), sm1 = S/M of layer 1. */
int dva_chain_dw1(const float* P, const double* mom, const float* W1, int32_t exact_w1, const float* bn1,
                  const float* sm1, float* dW1, void* stream);
/* Per-point set branch of DeepSetFeat on the chain (pooling.py:660-664): pooled fp32 [N][32] (+ the set-size
 * feature sqrt(1 / (n + 1e-3)) when w33 = Wsa[:, 32] is given) -> mlp_set = MLP[32(+1), 32, 32] -> u = Wc[:, 32:] . s,
 * the per-point half of the concatenation layer.  Every pass re-evaluates the branch from pooled (three-term bf16
 * split: fp32-class accuracy); one pass per BatchNorm barrier.  ops: 24 KiB device buffer (dva_chain_set_prep:
 * Wsa [32][ld_sa], Wsb [32][32], Wc [32][ld_c] of which the columns 32..63 are used).
 *   fwd stage 1: stats += statistics of s1 | stage 2: of s2 (needs bn_s1) | stage 3: u fp32 [N][32] (bn_s1, bn_s2)
 *   bwd stage 1: dW [32][ld_dw] += du^T a2 (= d Wc[:, 32:]), stats += S of layer s2
 *       stage 2: dW += d Wsb, stats += S of layer s1                                   (sm_s2)
 *       stage 3: dW += d Wsa[:, :32], dw33[i * ld_dw] += d Wsa[i, 32] (nullable), dpooled fp32 [N][32]  (sm_s1, sm_s2)
 * Backward statistics are S1 = sum dy | sum dy z (raw layer output), like dva_chain_bwd_layer. */
int dva_chain_set_prep(const float* Wsa, int32_t ld_sa, const float* Wsb, const float* Wc, int32_t ld_c, void* ops,
                       void* stream);
int dva_chain_set_fwd(int32_t stage, const float* pooled, const int64_t* ptr, const float* w33, const void* ops,
                      const float* bn_s1, const float* bn_s2, float* u, double* stats, int64_t n_points,
                      void* stream);
int dva_chain_set_bwd(int32_t stage, const float* pooled, const int64_t* ptr, const float* w33, const void* ops,
                      const float* bn_s1, const float* bn_s2, const float* sm_s1, const float* sm_s2,
                      const float* du, float* dpooled, float* dW, int32_t ld_dw, float* dw33, double* stats,
                      int64_t n_points, void* stream);
/* Backward of the softmax / weighted sum / gate of dva_chain_attn_fwd from the scores it left (scores fp32 [V][4]):
 * no chain evaluation.  grad_out / out bf16 [N][C] (out = the forward result; only read for points with more than 32
 * views).  Outputs: grad_scores fp32 [V][4] (columns >= G zero), view_rec = V packed 16-byte records {int32 point id |
 * gate * attention of groups 0..3 as bf16 | 4 unused bytes} (what dva_view_gather_rows_grad_rec16_to consumes: the rows
 * gradient is rounded to bf16, its weights travel as bf16), grad_gate_wb fp32 [2 G] (caller-zeroed, d gate_w |
 * d gate_b; nullable with gating off). */
int dva_chain_attn_bwd(const float* scores, const int32_t* view_point, const void* tiles, const int32_t* n_tiles,
                       const void* rows, const int32_t* row_idx, const int64_t* ptr, const float* gate_w,
                       const float* gate_b, const void* grad_out, const void* out, float* grad_scores, void* view_rec,
                       float* grad_gate_wb, int64_t n_points, int64_t n_views, int64_t n_rows, int32_t C, int32_t G,
                       int32_t scaling, float eps, void* stream);
/* dva_chain_attn_bwd with the element type of rows / grad_out / out as an argument: DVA_BF16 (= dva_chain_attn_bwd) or
 * DVA_F16.  The 16-byte view records keep their bf16 weights for both. */
int dva_chain_attn_bwd_dt(const float* scores, const int32_t* view_point, const void* tiles, const int32_t* n_tiles,
                          const void* rows, const int32_t* row_idx, const int64_t* ptr, const float* gate_w,
                          const float* gate_b, const void* grad_out, const void* out, float* grad_scores, void* view_rec,
                          float* grad_gate_wb, int64_t n_points, int64_t n_views, int64_t n_rows, int32_t C, int32_t G,
                          int32_t scaling, float eps, int32_t dtype, void* stream);
/* dva_chain_attn_bwd for fp32 value rows (the no-autocast path: ops.view_gather_attention backward when the scores
 * are fp32 [V][4]): rows / grad_out / out fp32, C in {32, 64, 128, 256}, view_rec = fp32 [V][8] records
 * {point id (int bits) | gate * attention per group | pad} as dva_view_gather_rows_grad reads them (rec_stride 8). */
int dva_chain_attn_bwd_f32(const float* scores, const int32_t* view_point, const void* tiles, const int32_t* n_tiles,
                           const float* rows, const int32_t* row_idx, const int64_t* ptr, const float* gate_w,
                           const float* gate_b, const float* grad_out, const float* out, float* grad_scores,
                           float* view_rec, float* grad_gate_wb, int64_t n_points, int64_t n_views, int64_t n_rows,
                           int32_t C, int32_t G, int32_t scaling, float eps, void* stream);
/* QKVBimodalCSRPool in ONE view kernel (round 4): dva_chain_attn_fwd with the KEY layer as the chain's last layer (ops
 * prepared with Ws = K.weight, G = 32; key_bias fp32 [32]) and the compatibilities scale * <key, queries[point]> per query-key
 * group as the scores (queries fp32 [N][32] in the keys' position order, 16-byte aligned; G in {1, 2, 4} = query-key groups =
 * attention groups).  scores_out (nullable) fp32 [V][4] receives the compatibilities, keys_out (nullable) bf16 [V][32] the
 * key rows (position order) dva_qkv_dquery reads back in the backward; everything else as dva_chain_attn_fwd. */
int dva_chain_attn_fwd_keys(const float* x_map, const int32_t* view_point, const float* u, const void* tiles,
                            const int32_t* n_tiles, const void* ops, const float* bn1, const float* bn2,
                            const float* bn5, const float* bn6, const float* key_bias, const float* queries, float scale,
                            const void* rows, const int32_t* row_idx, const int64_t* ptr, const float* gate_w,
                            const float* gate_b, void* out, float* scores_out, void* keys_out, int64_t n_points,
                            int64_t n_views, int64_t n_rows, int32_t C, int32_t G, int32_t scaling, float eps,
                            void* stream);
/* Score layer backward + the statistics of the BatchNorm-6 backward (one chain evaluation per view):
 * stats6 += S1 | S2 of layer 6 with dy6 = leaky'(t6) Ws^T grad_scores (t6 = the folded layer-6 product, the
 * pre-activation the forward's activation saw), dWs fp32 [G][32] / dbs fp32 [G] (caller-zeroed) += the gradient of the
 * score layer. */
int dva_chain_score_stats(const float* x_map, const int32_t* view_point, const float* u, const void* tiles,
                          const int32_t* n_tiles, const void* ops, const float* bn1, const float* bn2,
                          const float* bn5, const float* bn6, const float* grad_scores, double* stats6, float* dWs,
                          float* dbs, int32_t G, int64_t n_views, int64_t n_points, void* stream);
/* The same pass below the KEY layer of QKVBimodalCSRPool (ops prepared with G = 32): the gradient of a view's key row is
 * built in registers, dK'[v][i] = scale grad_compat[v][g(i)] queries[point(v)][i] (grad_compat fp32 [V][4], queries fp32
 * [N][32] in position order, G in {1, 2, 4} query-key groups); dWk fp32 [32][32] / dbk fp32 [32] (caller-zeroed) += the
 * gradient of the key layer.  dva_chain_bwd_layer6_keys: stage 6 of dva_chain_bwd_layer below that layer
 * (da_out = dy5 bf16 [V][32], dW = dW6, stats += S of layer 5). */
int dva_chain_score_stats_keys(const float* x_map, const int32_t* view_point, const float* u, const void* tiles,
                               const int32_t* n_tiles, const void* ops, const float* bn1, const float* bn2,
                               const float* bn5, const float* bn6, const float* grad_compat, const float* queries,
                               double* stats6, float* dWk, float* dbk, int32_t G, float scale, int64_t n_views,
                               int64_t n_points, void* stream);
int dva_chain_bwd_layer6_keys(const float* x_map, const int32_t* view_point, const float* u, const void* tiles,
                              const int32_t* n_tiles, const void* ops, const float* bn1, const float* bn2,
                              const float* bn5, const float* bn6, const float* sm6, const float* grad_compat,
                              const float* queries, void* da_out, float* dW, double* stats, int32_t G, float scale,
                              int64_t n_views, int64_t n_points, void* stream);
/* One backward pass of the chain between two BatchNorm-backward barriers ("sm" = fp32 [2][32] = S1/M | S2/M of
 * the pass's own layer, zeros with running statistics; dW / P / stats caller-zeroed, accumulated with
 * atomics).  Each pass re-evaluates the chain from x_map up to its own layer; the gradient w.r.t. the BatchNorm
 * output of the layer below (dy = leaky'(.) da, the derivative of the activation already applied with the sign of
 * the pre-activation the forward saw) is handed from pass to pass as da_out -> da_in, bf16 [V][32] (64 bytes per
 * view, in the lane order of the kernels: opaque to the caller):
 *   stage 6: grad_scores -> dW [32][32] = dW6, stats += S of layer 5, da_out = dy5                         (sm6)
 *   stage 5: da_in = dy5 -> dW [32][64] (first 32 columns) = dW5 per-view half, du fp32 [N][32] = gradient of u
 *            (written for seen points), stats += S of layer 2 (view part), da_out = dy2                (sm5)
 *   stage 2: da_in = dy2 (+ dpooled = the dpooled_dy of dva_chain_route_stats, routed to the arg views of
 *            dva_chain_stats2) -> dW [32][32] = dW2,
 *            P fp32 [32][20] += sum_v dy1 [x_hi (8) | x_lo (8) | 1 | unused]^T; the statistics of layer 1 follow
 *            from P (dva_chain_stats1; stats may be NULL)                                                (sm2) */
int dva_chain_bwd_layer(int32_t stage, const float* x_map, const int32_t* view_point, const float* u,
                        const void* tiles, const int32_t* n_tiles, const void* ops, const float* bn1,
                        const float* bn2, const float* bn5, const float* bn6, const float* sm2, const float* sm5,
                        const float* sm6, const float* grad_scores, const int32_t* arg, const float* dpooled,
                        const void* da_in, void* da_out, float* dW, float* du, float* P,
                        double* stats, int32_t G, int64_t n_views, int64_t n_points, void* stream);
/* ---- The chain in fp32: DeepSetFeat + E_score for fp32 features OUTSIDE torch.autocast (the reference's default,
 * models/base_model.py:244), replacing the stored-activation passes dva_deepset_* (13 stored [V, 32] tensors).
 * Same tiles, statistics and hand-over rules as dva_chain_* above; every product runs on the fp32 matrix cores
 * (v_mfma_f32_32x32x2_f32: exact fp32 fma chains), BatchNorm + LeakyReLU in fp32 on the accumulators (no BatchNorm
 * folding; leaky' follows the sign of the plain pre-activation), gradient rows between the passes fp32 [V][32].
 * These passes are bound by the matrix pipe, not by HBM: the raw outputs of layers 2 and 5 (z2, z5: fp32 [V][32])
 * stay in HBM and every pass starts from them instead of re-evaluating the chain from x_map.
 * bn tables: fp32 [>= 4][32] mean | invstd | gamma | beta.  The attention (softmax, value gather, weighted sum, gate)
 * stays in dva_view_gather_attention_*; these entries produce the scores fp32 [V][4] (columns >= G zero) and consume
 * their gradient fp32 [V][4].
 *   dva_chain3_prep         ops: 26 KiB device buffer (26 operand blocks of 64 float4)
 *   dva_chain3_stats2       x_map -> z2 (stored); stats double[64] += sum z2 | sum z2^2; zstar / arg as dva_chain_stats2
 *   dva_chain3_stats        layer 5: rows_in = z2 (bn = bn2) -> z5 = W5a act(BN2(z2)) + u[point] (stored), stats of z5;
 *                           layer 6: rows_in = z5 (bn = bn5) -> stats of z6 (view_point, u, z5 unused, may be NULL)
 *   dva_chain3_scores       z5 -> scores
 *   dva_chain3_score_stats  z5, grad_scores -> dWs [G][32], dbs [G], stats6 (S of the BatchNorm-6 backward)
 *   dva_chain3_bwd_layer    bn_lo / bn_hi = tables of the lower / upper layer of the pass, sm = S / M of the upper one
 *     stage 6: z_rows = z5, grad_scores -> dW (= dW6 [32][32]), stats (S of layer 5), da_out = dy5      (bn5, bn6)
 *     stage 5: z_rows = z2, da_in = dy5, view_point, u -> dW (= dW5 [32][64], view half), du [N][32] (caller-zeroed),
 *              stats (S of layer 2, view part), da_out = dy2                                              (bn2, bn5)
 *     stage 2: x_map, z_rows = z2, da_in = dy2, view_point, arg, dpooled (dva_chain_route_stats) -> dW (= dW2),
 *              P fp32 [32][20] = sum dy1 [x (8) | 0 (8) | 1 | 0]^T (dva_chain_stats1 / dva_chain_dw1, exact_w1 = 1)
 *                                                                                                          (bn1, bn2)
 * dva_chain_moments / dva_chain_stats1 / dva_chain_dw1 (exact_w1 = 1), dva_chain_pooled and dva_chain_route_stats
 * are shared with the bf16 chain. */
int dva_chain3_prep(const float* W1, const float* W2, const float* W5, int32_t ld5, const float* W6, const float* Ws,
                    int32_t G, void* ops, void* stream);
int dva_chain3_stats2(const float* x_map, const int32_t* view_point, const void* tiles, const int32_t* n_tiles,
                      const void* ops, const float* bn1, const float* gamma2, double* stats, float* zstar,
                      int32_t* arg, float* z2, int64_t n_views, void* stream);
int dva_chain3_stats(int32_t layer, const float* rows_in, const int32_t* view_point, const float* u,
                     const void* tiles, const int32_t* n_tiles, const void* ops, const float* bn, float* z5,
                     double* stats, int64_t n_views, int64_t n_points, void* stream);
int dva_chain3_scores(const float* z5, const void* tiles, const int32_t* n_tiles, const void* ops, const float* bn5,
                      const float* bn6, const float* score_bias, int32_t G, float* scores, int64_t n_views,
                      void* stream);
int dva_chain3_score_stats(const float* z5, const void* tiles, const int32_t* n_tiles, const void* ops,
                           const float* bn5, const float* bn6, const float* grad_scores, double* stats6, float* dWs,
                           float* dbs, int32_t G, int64_t n_views, void* stream);
int dva_chain3_bwd_layer(int32_t stage, const float* x_map, const float* z_rows, const int32_t* view_point,
                         const float* u, const void* tiles, const int32_t* n_tiles, const void* ops,
                         const float* bn_lo, const float* bn_hi, const float* sm, const float* grad_scores,
                         const int32_t* arg, const float* dpooled, const float* da_in, float* da_out, float* dW,
                         float* du, float* P, double* stats, int64_t n_views, int64_t n_points, void* stream);
/* The per-point set branch of the fp32 chain: dva_chain_set_* on the fp32 matrix cores (ops: 24 KiB). */
int dva_chain3_set_prep(const float* Wsa, int32_t ld_sa, const float* Wsb, const float* Wc, int32_t ld_c, void* ops,
                        void* stream);
int dva_chain3_set_fwd(int32_t stage, const float* pooled, const int64_t* ptr, const float* w33, const void* ops,
                       const float* bn_s1, const float* bn_s2, float* u, double* stats, int64_t n_points,
                       void* stream);
int dva_chain3_set_bwd(int32_t stage, const float* pooled, const int64_t* ptr, const float* w33, const void* ops,
                       const float* bn_s1, const float* bn_s2, const float* sm_s1, const float* sm_s2,
                       const float* du, float* dpooled, float* dW, int32_t ld_dw, float* dw33, double* stats,
                       int64_t n_points, void* stream);
/* stats += S1 | S2 of layer 2, per-point part: sum over the seen points of leaky'(BN2(zstar)) dpooled (x z_hat);
 * dpooled_dy fp32 [N][32] = leaky'(BN2(zstar)) dpooled (0 for unseen points): the `dpooled` of stage 2. */
int dva_chain_route_stats(const float* zstar, const float* dpooled, const float* bn2, const int64_t* ptr,
                          double* stats, float* dpooled_dy, int64_t n_points, void* stream);

/* 'concatenation' fusion (modules/multimodal/fusion.py:7-53: torch.cat((x_main, x_mod), dim=-1)) with the dtype
 * promotion of torch.cat folded in: x_main fp32 [N][C_main], x_mod fp32 / bf16 [N][C_mod] -> out fp32
 * [N][C_main + C_mod]; bwd: grad_out -> grad_main fp32, grad_mod in mod_dtype.  C_main, C_mod multiples of 4. */
int dva_concat_cast_fwd(const float* x_main, const void* x_mod, float* out, int64_t N, int32_t C_main, int32_t C_mod,
                        int32_t mod_dtype, void* stream);
int dva_concat_cast_bwd(const float* grad_out, float* grad_main, void* grad_mod, int64_t N, int32_t C_main,
                        int32_t C_mod, int32_t mod_dtype, void* stream);
/* Measurement helper (bench.py): float4 grid-stride device copy of nbytes (multiple of 16) -- the practical HBM
 * ceiling (read + write) beside which the roofline fractions are quoted. */
int dva_copy_ceiling(const void* src, void* dst, int64_t nbytes, void* stream);
/* out[p, :] = 0 for every point p without views (ptr[p + 1] == ptr[p]); rows of the other points are not touched.
 * out: n_points rows of row_bytes bytes (multiple of 16, 16-byte aligned).  The pooled features of unseen points are exact
 * zeros (reference modules/multimodal/pooling.py:870, torch_scatter's empty segments); the view kernels write only the
 * points that have views. */
int dva_zero_unseen_rows(const int64_t* ptr, void* out, int64_t n_points, int64_t row_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Voxel parent index after a strided sparse 3D convolution.  Replaces the torchsparse (v1.1.0, not in the
 * reference tree) `sphashquery(sphash(in_coords), sphash(out_coords))` call of
 * modules/multimodal/modules.py:176-198 together with the flooring of the spatial columns:
 * idx[i] = j such that out_coords[j] == in_coords[i] with every column except batch_col floored to a
 * multiple of stride_out (floor towards -inf), or -1 when no output voxel has these coordinates.
 * in_coords int32 [n_in, 4], out_coords int32 [n_out, 4] (16-byte aligned; torchsparse layout: x, y, z,
 * batch => batch_col = 3; batch_col = -1 floors all four columns), idx int64 [n_in].  Exact (full
 * coordinate compare in an open-addressing table), deterministic; duplicate out rows -> smallest j.
 * ------------------------------------------------------------------------------------------ */
int64_t dva_voxel_parent_workspace_bytes(int64_t n_out);
int dva_voxel_parent_index(const int32_t* in_coords, int64_t n_in, const int32_t* out_coords, int64_t n_out,
                           int32_t stride_out, int32_t batch_col, int64_t* idx, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Sparse 3D convolution on voxel tensors.  Replaces torchsparse v1.1.0 `Conv3d` /
 * transposed `Conv3d` (not in the reference tree) behind modules/SparseConv3d/nn/torchsparse.py:6-40, used by
 * ResNetDown / ResNetUp / ResBlock (modules/SparseConv3d/modules.py:10-220).
 *
 * dva_voxel_kernel_map: nbr[k * n_dst + j] = i such that src_coords[i] == dst_coords[j] + offsets[k] on the
 * first three columns with equal fourth (batch) column, else -1 (torchsparse `sphashquery(sphash(dst,
 * offsets), sphash(src))`).  Coordinates int32 [n, 4], 16-byte aligned; offsets int32 [K, 3] on the device.
 * Workspace: dva_voxel_parent_workspace_bytes(n_src).
 *
 * dva_sparse_conv_apply: out[j, :] = bias + sum_k x[nbr[k][j], :] @ Wk   (missing neighbours contribute 0).
 *   mode 0: W = fp32 [K, Cin, Cout], Wk = W[k]            (forward; transposed convolution with its own map)
 *   mode 1: W = fp32 [K, Cout, Cin], Wk = W[k]^T          (input gradient, with the transposed kernel map)
 * x [n_src, Cin], out [n_dst, Cout] in `dtype` (DVA_F32: fp32 accuracy through a 3-term bf16 split on the
 * matrix cores; DVA_BF16: bf16 operands, fp32 accumulation), bias fp32 [Cout] nullable.  Cin and Cout must be
 * multiples of 16 (the host pads), n_src >= 1.  Workspace: dva_sparse_conv_workspace_bytes (re-packed weights).
 * Every output row is written exactly once: deterministic, no atomics.
 *
 * dva_sparse_conv_wgrad: grad_W[k][a][b] = sum_j x[nbr[k][j]][a] * grad_out[j][b], fp32 [K, Cin, Cout],
 * zeroed by the call, accumulated with fp32 atomics (summation order not fixed).
 *
 * Inference with constant weights (since dva_version 332):
 * dva_sparse_conv_pack_weights: the re-pack dva_sparse_conv_apply runs on every call, once, into the caller's
 * buffer `packed` (16-byte aligned, packed_bytes >= dva_sparse_conv_workspace_bytes(K, Cin, Cout, dtype); the
 * layout depends on `dtype`, the feature type of the later calls).  W and mode as above.
 * dva_sparse_conv_apply_packed: the mode 0 convolution from that buffer, no workspace and no re-pack launch,
 * with the activation and the residual sum folded into the store.  Per output element, in fp32, every step
 * rounded on its own (no fused multiply-add), then ONE rounding to `dtype`:
 *   v = acc + bias[n];   v = v >= 0 ? v : slope * v;   v = v + residual[j][n];   out[j][n] = dtype(v)
 * slope finite (1: no activation, 0: ReLU); residual [n_dst, Cout] in `dtype`, 16-byte aligned, nullable, must
 * not alias out.  A destination without any neighbour gets act(bias) + residual.  Deterministic, no atomics.
 * Both validate as dva_sparse_conv_apply does, in its order, before any HIP call.
 *
 * Features in parts (since dva_version 333): the convolution of the channel concatenation of P tensors on the
 * same voxels, without that concatenation in memory.  `parts` and `widths` are HOST arrays of P device pointers
 * and P channel counts (copied into the kernel arguments: no device table, no copy, no synchronisation); part p
 * is [n_src, widths[p]] in `dtype`, 16-byte aligned, widths[p] a multiple of 16 (the host pads a narrow part,
 * alone), 1 <= P <= 4.  Cin = sum of the widths; W, the packed buffer and grad_W are those of the single-tensor
 * entries for that Cin, the input channels in concatenation order (a padded part's zero rows in place).
 * dva_sparse_conv_apply_parts is dva_sparse_conv_apply in mode 0, dva_sparse_conv_apply_packed_parts is
 * dva_sparse_conv_apply_packed, dva_sparse_conv_wgrad_parts is dva_sparse_conv_wgrad.  The 16-channel steps run
 * in concatenation order, so apply gives the bits of the single-tensor entry on the concatenated tensor.
 * Validation, in this order: scalars (P <= 0 or widths == NULL: DVA_ERR_INVALID), DVA_F16 (DVA_ERR_UNSUPPORTED),
 * P > 4 (DVA_ERR_UNSUPPORTED), a width <= 0 (DVA_ERR_INVALID) or not a multiple of 16 (DVA_ERR_UNSUPPORTED), then
 * as the single-tensor entry: n_dst == 0 is DVA_OK before any device pointer is looked at; a null or misaligned
 * part is DVA_ERR_INVALID.
 * ------------------------------------------------------------------------------------------ */
int dva_voxel_kernel_map(const int32_t* src_coords, int64_t n_src, const int32_t* dst_coords, int64_t n_dst,
                         const int32_t* offsets, int32_t K, int32_t* nbr, void* workspace,
                         int64_t workspace_bytes, void* stream);
int64_t dva_sparse_conv_workspace_bytes(int32_t K, int32_t Cin, int32_t Cout, int32_t dtype);
int dva_sparse_conv_apply(const void* x, const int32_t* nbr, const float* W, const float* bias, void* out,
                          int64_t n_src, int64_t n_dst, int32_t K, int32_t Cin, int32_t Cout, int32_t mode,
                          int32_t dtype, void* workspace, int64_t workspace_bytes, void* stream);
int dva_sparse_conv_wgrad(const void* x, const int32_t* nbr, const void* grad_out, float* grad_W, int64_t n_src,
                          int64_t n_dst, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* stream);
int dva_sparse_conv_pack_weights(const float* W, int32_t K, int32_t Cin, int32_t Cout, int32_t mode, int32_t dtype,
                                 void* packed, int64_t packed_bytes, void* stream);
int dva_sparse_conv_apply_packed(const void* x, const int32_t* nbr, const void* packed, int64_t packed_bytes,
                                 const float* bias, const void* residual, float slope, void* out, int64_t n_src,
                                 int64_t n_dst, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* stream);
int dva_sparse_conv_apply_parts(const void* const* parts, const int32_t* widths, int32_t P, const int32_t* nbr,
                                const float* W, const float* bias, void* out, int64_t n_src, int64_t n_dst,
                                int32_t K, int32_t Cout, int32_t dtype, void* workspace, int64_t workspace_bytes,
                                void* stream);
int dva_sparse_conv_apply_packed_parts(const void* const* parts, const int32_t* widths, int32_t P,
                                       const int32_t* nbr, const void* packed, int64_t packed_bytes,
                                       const float* bias, const void* residual, float slope, void* out,
                                       int64_t n_src, int64_t n_dst, int32_t K, int32_t Cout, int32_t dtype,
                                       void* stream);
int dva_sparse_conv_wgrad_parts(const void* const* parts, const int32_t* widths, int32_t P, const int32_t* nbr,
                                const void* grad_out, float* grad_W, int64_t n_src, int64_t n_dst, int32_t K,
                                int32_t Cout, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Neighbourhood-based mapping features (core/data_transform/multimodal/image.py:431-612): exact k nearest
 * neighbours of every point among all points (replaces KeOps `((x_i - x_j)**2).sum(2).argKmin(k, dim=1)`,
 * :506-507; pykeops 1.4.2 is not in the reference tree) and the per-view occlusion counts (:560-599).
 * ------------------------------------------------------------------------------------------ */
/* neighbors int32 [n, k] (k <= 128), dist2 fp32 [n, k] (nullable): ascending by (d2, index) with
 * d2 = ((dx*dx + dy*dy) + dz*dz) in fp32; the point itself is its own first neighbour; -1 / inf when
 * n < k.  bbox = fp32[6] device array (min xyz | max xyz of the cloud); cell = grid cell size;
 * (max - min) / cell must stay below 2^20 per axis.  One call searches at most max_shell Chebyshev shells
 * of cells around each query and finishes every query whose k-th distance is provably final within them
 * (or all queries, when the shells cover the whole cloud); `done` (uint8 [n], nullable) is read to skip
 * finished queries and set for those finished here, so sparse regions are handled by calling again with
 * a coarser cell (host: deepviewagg_amd.ops.knn, cell x4 per level).  The result is exact for any cell. */
int64_t dva_knn_workspace_bytes(int64_t n);
int dva_knn(const float* xyz, int64_t n, const float* bbox, float cell, int32_t k, int32_t max_shell,
            uint8_t* done, int32_t* neighbors, float* dist2, void* workspace, int64_t workspace_bytes,
            void* stream);
/* The same search for the n_query points of a separate query cloud in the n_search points of a search cloud
 * (PCAComputePointwise with use_full_pos, reference core/data_transform/features.py:360-485: KeOps argKmin of the
 * query cloud against data.full_pos).  neighbors int32 [n_query, k] (k <= 128, n_search >= k) index the search
 * cloud, dist2 fp32 [n_query, k] (nullable): ascending by (d2, search index) with d2 = ((dx*dx + dy*dy) + dz*dz) in
 * fp32, ties to the lower index, no self-first rule.  bbox (device fp32[6]) must cover BOTH clouds (queries may lie
 * outside the search cloud's box); the grid is built on the search cloud.  cell, max_shell and done (uint8 [n_query])
 * as for dva_knn; exact for any cell.  n_query < 2^31, n_search < 2^30 (DVA_ERR_UNSUPPORTED beyond). */
int64_t dva_knn_query_workspace_bytes(int64_t n_query, int64_t n_search);
int dva_knn_query(const float* query_xyz, int64_t n_query, const float* search_xyz, int64_t n_search,
                  const float* bbox, float cell, int32_t k, int32_t max_shell, uint8_t* done, int32_t* neighbors,
                  float* dist2, void* workspace, int64_t workspace_bytes, void* stream);
/* Per-point PCA of the k-point neighbourhoods neighbors int32 [n_query, k] (indices into search_xyz fp32
 * [n_search, 3]; 1 <= k <= 128, n_search >= k): what the reference's batch_pca (core/data_transform/features.py:307-329)
 * computes per point.  Mean of the neighbour positions, covariance of the centred positions / k (not k - 1),
 * eigenvalues fp32 [n_query, 3] ascending with values below 0 set to 0, eigenvectors fp32 [n_query, 9] as three unit
 * rows [v0 | v1 | v2] (evec.transpose(2, 1).flatten(1)): the first three values are the normal.  Sign convention: the
 * fp32 component of largest magnitude of every eigenvector is positive (the first one of equal magnitudes).  A covariance
 * with a NaN entry (NaN / inf coordinates) or a neighbour index outside [0, n_search) gives eigenvalues (1, 1, 1)
 * and the identity (features.py:320-323); a zero covariance (all neighbours equal) gives 0 and the identity.
 * Covariance accumulated in fp64, eigenproblem solved by fp64 cyclic Jacobi (csrc/pca.hip). */
int dva_pointwise_pca(const float* search_xyz, int64_t n_search, const int32_t* neighbors, int64_t n_query,
                      int32_t k, float* eigenvalues, float* eigenvectors, void* stream);
/* out fp32 [n_views, n_k]: (1 + #{i < k_list[c] : neighbors[p(v), i] is seen by image(v)}) / (k_list[c] + 1)
 * (k_list ascending, last <= k).  view_point int32 [n_views] (dva_csr_expand), images int64 [n_views],
 * bits = scratch uint64 [n_points * ceil(n_images / 64)]. */
int dva_view_occlusion(const int32_t* view_point, const int64_t* images, int64_t n_views, int64_t n_points,
                       int32_t n_images, const int32_t* neighbors, int32_t k, const int32_t* k_list,
                       int32_t n_k, uint64_t* bits, float* out, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * One strided level of the voxel pyramid (since dva_version 334; csrc/voxel_level.hip): what a strided sparse
 * convolution needs before it can run -- output coordinates, the parent of every input voxel and, for
 * kernel_size 2 / stride 2 / dilation 1, both kernel maps -- from one sort instead of a torch composition and three
 * hash tables.  Coordinates int32 [n, 4] = (x, y, z, batch), 16-byte aligned; ratio = the output tensor stride,
 * in_stride = the input's.  0 <= n < 2^30 (DVA_ERR_UNSUPPORTED beyond); n == 0 is DVA_OK before any pointer is read.
 *   dva_voxel_bounds      bounds int64 [8] (device) = min x, y, z, batch, max x, y, z, batch of coords.
 *   dva_voxel_level       bounds: HOST int64 [8], lo and hi of the rows with x, y, z floored to a multiple of ratio
 *                         (floor towards -inf).  Floor is monotone, so the floored bounds of any finer tensor of the
 *                         same pyramid are exact.  out_coords int32 [capacity n, 4] = the unique floored rows, ascending
 *                         (batch, z, y, x); parent int64 [n] = the row of out_coords holding the floored input row;
 *                         record int64 [2] (device) = n_out, flags:
 *                           DVA_VOXEL_LEVEL_FLAG_STRIDE  some x, y or z is not a multiple of in_stride (the results are
 *                                                        valid; dva_voxel_level_maps does not apply)
 *                           DVA_VOXEL_LEVEL_FLAG_KEY     prod(hi - lo + 1) >= 2^62: nothing else is written
 *                           DVA_VOXEL_LEVEL_FLAG_BOUNDS  a floored row lies outside bounds: out_coords, parent and n_out
 *                                                        are unspecified (every access stays inside the buffers)
 *                         Workspace: dva_voxel_level_workspace_bytes(n) (also that of dva_voxel_bounds).
 *   dva_voxel_level_maps  after the caller has read the record, for ratio == 2 * in_stride (else DVA_ERR_INVALID):
 *                         nbr int32 [8, n_out], nbr_t int32 [8, n] as dva_voxel_kernel_map(in, out, offsets) and
 *                         (out, in, -offsets) give them for the offsets {0, in_stride}^3, z fastest: with d = (c -
 *                         floor(c)) / in_stride and k = (d_x * 2 + d_y) * 2 + d_z, nbr_t[k][i] = parent[i] and
 *                         nbr[k][parent[i]] = i (duplicate input rows: the smallest i), -1 elsewhere.  Requires input
 *                         coordinates that are multiples of in_stride (no STRIDE flag).  A parent outside [0, n_out)
 *                         writes -1.  No workspace.
 * Deterministic: integer atomics only (or of flags, min of row ids).
 * ------------------------------------------------------------------------------------------ */
#define DVA_VOXEL_LEVEL_FLAG_STRIDE 1
#define DVA_VOXEL_LEVEL_FLAG_KEY 2
#define DVA_VOXEL_LEVEL_FLAG_BOUNDS 4
int64_t dva_voxel_level_workspace_bytes(int64_t n);
int dva_voxel_bounds(const int32_t* coords, int64_t n, int64_t* bounds, void* workspace, int64_t workspace_bytes,
                     void* stream);
int dva_voxel_level(const int32_t* in_coords, int64_t n, int32_t ratio, int32_t in_stride, const int64_t* bounds,
                    int32_t* out_coords, int64_t* parent, int64_t* record, void* workspace, int64_t workspace_bytes,
                    void* stream);
int dva_voxel_level_maps(const int32_t* in_coords, const int64_t* parent, int64_t n, int64_t n_out, int32_t ratio,
                         int32_t in_stride, int32_t* nbr, int32_t* nbr_t, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Voxel-grid subsampling.  Replaces GridSampling3D (core/data_transform/grid_transform.py:24-191: torch_cluster
 * grid_cluster, torch_geometric voxel_grid + consecutive_cluster, torch_scatter scatter_add / scatter_mean).
 *   dva_grid_quantize  pos [n, 3] (DVA_GRID_F32 or _F64) -> coords int32 [n, 3] = rint(pos / size), the division
 *                      correctly rounded in the dtype of pos (fp32: by (float)size), ties to even.  stats int64 [9]
 *                      (device) = min x, y, z, batch, max x, y, z, batch, flags (bit 0: a non-finite coordinate,
 *                      bit 1: |pos / size| >= 2^24; the coords of such points are 0).  batch int64 [n] nullable
 *                      (0 for all).  The caller reads stats to size the key: end_bit = bits of prod(max - min + 1).
 *   dva_grid_cluster   key = mixed radix of (batch, z, y, x) - min, x fastest, < 2^end_bit (1 <= end_bit <= 63);
 *                      stable sort: order int64 [n] = points in ascending key, then index; voxels numbered in ascending
 *                      key: cluster int64 [n], offsets int64 [capacity n + 1] (voxel v = order[offsets[v] ..
 *                      offsets[v+1])), rep int64 [capacity n] = the member of largest rank (rank int64 [n] nullable,
 *                      read as 32-bit values; NULL: the largest index), voxel_coords int32 [capacity n, 3] nullable =
 *                      coords[rep], *n_voxels (device) = M.
 *   dva_grid_mean      out [M, C] = per voxel the sum of the rows in the dtype of src, sequential in ascending point
 *                      index, divided by the count in that dtype (fp32 counts saturate at 2^24 as a sum of ones does);
 *                      integer dtypes (DVA_GRID_I32 / _I64): wrapping sum, quotient rounded toward zero.  Workspace:
 *                      dva_grid_workspace_bytes(n, C * element size).  Bitwise reproducible (no atomics).
 *   dva_grid_majority  out int64 [M] = per voxel the most frequent label (labels int64 in [label_min, label_min +
 *                      n_labels), n_labels <= 2^32), ties to the smallest; end_bit = bits of M * n_labels.
 * 1 <= n < 2^31 (DVA_ERR_UNSUPPORTED beyond); workspace of quantize / cluster / majority:
 * dva_grid_workspace_bytes(n, 0).  Argument errors return DVA_ERR_INVALID before any HIP call. */
#define DVA_GRID_F32 0
#define DVA_GRID_F64 1
#define DVA_GRID_I32 2
#define DVA_GRID_I64 3
int64_t dva_grid_workspace_bytes(int64_t n, int64_t row_bytes);
int dva_grid_quantize(const void* pos, int32_t dtype, int64_t n, double size, const int64_t* batch, int32_t* coords,
                      int64_t* stats, void* workspace, int64_t workspace_bytes, void* stream);
int dva_grid_cluster(const int32_t* coords, const int64_t* batch, const int64_t* rank, int64_t n,
                     const int64_t* stats, int32_t end_bit, int64_t* order, int64_t* cluster, int64_t* offsets,
                     int64_t* rep, int32_t* voxel_coords, int64_t* n_voxels, void* workspace,
                     int64_t workspace_bytes, void* stream);
int dva_grid_mean(const void* src, int32_t dtype, int64_t n, int32_t C, const int64_t* order, const int64_t* offsets,
                  int64_t n_voxels, void* out, void* workspace, int64_t workspace_bytes, void* stream);
int dva_grid_majority(const int64_t* labels, int64_t n, const int64_t* cluster, int64_t n_voxels, int64_t label_min,
                      int64_t n_labels, int32_t end_bit, int64_t* out, void* workspace, int64_t workspace_bytes,
                      void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Exact radius query.  Replaces scikit-learn's KDTree.query_radius under SphereSampling / CylinderSampling and
 * GridSphereSampling / GridCylinderSampling (core/data_transform/transforms.py:99-232, :301-405), all centres in
 * one call.  pos fp32 [n, 3]; centres fp64 [n_centres, dims], dims = 3 (sphere) or 2 (cylinder: z is ignored);
 * radius fp64 >= 0, or radii fp64 [n_centres] (nullable; when given, radius is ignored and a negative or NaN entry
 * gives an empty ball).  Point p is a member of centre c iff d <= r * r with d = ((dx dx) + dy dy) + dz dz,
 * dx = (double)p.x - c.x, every product and sum rounded on its own in fp64 (no fused multiply-add), r * r computed
 * once, the boundary inclusive: scikit-learn's leaf test.  A point with a non-finite coordinate is never a member.
 *   dva_radius_count  ptr int64 [n_centres + 1] (device) = CSR offsets; ptr[n_centres] is the number of members of
 *                     all centres and may exceed 2^31.  Leaves the per-(tile, centre) offsets in the workspace.
 *   dva_radius_fill   idx int64 [ptr[n_centres]] = the members of every centre in ascending point index, from the
 *                     SAME workspace, untouched since dva_radius_count of the same arguments.  idx_capacity = the
 *                     number of elements idx holds; nothing is written beyond it.
 * Brute force over all pairs in two passes, no atomics: bitwise reproducible.  n < 2^31 (DVA_ERR_UNSUPPORTED beyond);
 * n = 0, n_centres = 0 and empty balls are valid.  The workspace grows with n * n_centres (4 bytes per centre and
 * 512 points): the caller splits the centres to its budget.  Argument errors return DVA_ERR_INVALID before any HIP
 * call. */
int64_t dva_radius_query_workspace_bytes(int64_t n, int64_t n_centres);
int dva_radius_count(const float* pos, int64_t n, const double* centres, int64_t n_centres, int32_t dims,
                     double radius, const double* radii, int64_t* ptr, void* workspace, int64_t workspace_bytes,
                     void* stream);
int dva_radius_fill(const float* pos, int64_t n, const double* centres, int64_t n_centres, int32_t dims,
                    double radius, const double* radii, const int64_t* ptr, int64_t* idx, int64_t idx_capacity,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * ElasticDistortion (core/data_transform/grid_transform.py:194-256: six scipy.ndimage.convolve calls over a noise
 * volume and a scipy RegularGridInterpolator over every point, on the host).  One distortion level is
 *   dva_minmax3_f32       out fp32 [6] (device) = the column minima, then the column maxima, of pos fp32 [n, 3];
 *                         n >= 1.  Exact and independent of the order of reduction; non-finite values are not
 *                         supported (a NaN is skipped).  Workspace: dva_minmax3_workspace_bytes().
 *                         The caller derives the volume's shape [dx, dy, dz] and the three knot axes from these six
 *                         numbers on the host (numpy's promotion rules decide their bits).
 *   dva_elastic_smooth    out fp32 [dx, dy, dz, 3] = the noise volume after two rounds of three 3-tap passes along
 *                         axes 0, 1, 2, zero padded: per pass ((0 + a w) + b w) + c w in fp64 over the neighbours in
 *                         ascending order, w = (double)(1.0f / 3.0f), every product and sum rounded on its own, the
 *                         pass stored as fp32 -- scipy.ndimage.convolve of a float32 array with the reference's blur
 *                         kernels.  noise is not modified; out may not alias it.  Workspace (two volumes the passes
 *                         alternate between): dva_elastic_workspace_bytes(dx, dy, dz).
 *   dva_elastic_displace  out fp32 [n, 3] = fp32(fp64(pos) + value * magnitude); value = the trilinear interpolant of
 *                         field fp32 [dx, dy, dz, 3] at pos over the knots axes fp64 [dx + dy + dz] (the three axes
 *                         one after the other, each ascending, at least 2 knots), in fp64: per axis the cell i = the
 *                         largest index with ax[i] <= x clipped to [0, d - 2], y = (x - ax[i]) / (ax[i + 1] - ax[i]),
 *                         the eight corners in the order of itertools.product (axis 0 slowest, lower corner first),
 *                         weight = (w0 w1) w2 with w = 1 - y | y, value += field[corner] * weight from 0; 0 for a
 *                         point outside the axes.  No fused multiply-add, correctly rounded division: scipy's
 *                         RegularGridInterpolator(method="linear", bounds_error=False, fill_value=0) bit for bit.
 *                         out may alias pos.
 * 3 n < 2^31 and 3 dx dy dz < 2^31 (DVA_ERR_UNSUPPORTED beyond).  No atomics: bitwise reproducible.  Argument errors
 * return DVA_ERR_INVALID before any HIP call. */
int64_t dva_minmax3_workspace_bytes(void);
int dva_minmax3_f32(const float* pos, int64_t n, float* out, void* workspace, int64_t workspace_bytes, void* stream);
int64_t dva_elastic_workspace_bytes(int64_t dx, int64_t dy, int64_t dz);
int dva_elastic_smooth(const float* noise, int64_t dx, int64_t dy, int64_t dz, float* out, void* workspace,
                       int64_t workspace_bytes, void* stream);
int dva_elastic_displace(const float* pos, int64_t n, const float* field, const double* axes, int64_t dx, int64_t dy,
                         int64_t dz, double magnitude, float* out, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * The image tail of the multimodal transform chains (image_tail.hip): ColorJitter -> RandomHorizontalFlip ->
 * ToFloatImage -> Normalize of core/data_transform/multimodal/image.py:1195-1282, where ColorJitter and Normalize are
 * torchvision.transforms 0.8.2 objects.  Parity with torchvision is UNPINNED (it is no dependency and no fixture of it
 * exists): the arithmetic stated here, restated from its ColorJitter.forward and functional_tensor, is the contract.
 * All of it is fp32, every operation rounded on its own, no fused multiply-add, correctly rounded division;
 * u8(v) = truncation toward zero.
 *   dva_image_tail_u8        x uint8 [B, 3, H, W].  The n_ops <= 3 ops op_codes[k] (DVA_JITTER_*, each at most once) are
 *                            applied in order with the factors factors[k] >= 0 (HOST arrays; f = f32(factors[k]), the
 *                            complement f32(1.0 - factors[k]) is taken in double here):
 *                              gray            u8((f32(0.2989) r + f32(0.587) g) + f32(0.114) b)
 *                              blend(p, q, f)  u8(clamp(f p + (1 - f) q, 0, 255))
 *                              brightness      blend(p, 0, f);  saturation  blend(p, gray(pixel), f)
 *                              contrast        blend(p, m_i, f), m_i = f32(S_i) / f32(H W), S_i = the exact int64 sum
 *                                              of gray over image i after the ops that precede contrast (per image,
 *                                              not per batch)
 *                            then, with flip, output column w takes source column W - 1 - w; with to_float the value
 *                            is f32(p) / f32(255), and with mean / std (HOST fp32 [3] each, both or neither, to_float
 *                            required, no zero in std) it is (v - mean[c]) / std[c].  out is uint8 [B, 3, H, W]
 *                            without to_float and fp32 [B, 3, H, W] with it; it may not alias x.
 *                            Launches: with contrast, a clear of the B accumulators on the stream and the gray-sum
 *                            kernel (integer partial sums, one 64-bit integer atomic add per block: order-free, the
 *                            same call gives the same bytes), then the apply kernel; one kernel otherwise.
 *                            workspace: dva_image_tail_workspace_bytes(B), needed with contrast only (nullable
 *                            otherwise); it need not be cleared by the caller.
 *   dva_image_normalize_f32  out fp32 [B, C, HW] = (x - mean[c]) / std[c] for x fp32 [B, C, HW], 1 <= C <=
 *                            DVA_IMAGE_MAX_CHANNELS (DVA_ERR_UNSUPPORTED beyond); mean / std HOST fp32 [C].  out may
 *                            alias x.
 *   dva_image_window_u8      the same tail over a window of a source image that is never materialised (the deferred
 *                            CenterRoll / CropImageGroups / image selection of the online chains).  src uint8
 *                            [N, 3, H, W] contiguous; index int64 [B], rolls int64 [B], offsets int64 [B, 2] = (x, y),
 *                            all DEVICE arrays; the window is Wc x Hc with 1 <= Wc <= W, 1 <= Hc <= H:
 *                              win[b, c, y, x] = src[index[b], c, offsets[b, 1] + y,
 *                                                    (offsets[b, 0] + x - rolls[b]) mod W]      (non-negative mod)
 *                              out             = dva_image_tail_u8(win, ...)
 *                            that is the roll of image index[b] along W by rolls[b], then the crop at offsets[b], then
 *                            the tail, with the same op list, flip, to_float, mean and std arguments.  The flip mirrors
 *                            WINDOW columns (output column x takes window column Wc - 1 - x) and the contrast mean is
 *                            m_b = f32(S_b) / f32(Hc Wc), S_b the exact int64 sum of gray over the window of output
 *                            image b alone.  out is uint8 [B, 3, Hc, Wc] without to_float and fp32 with it; it may not
 *                            alias src.  Launches and workspace (dva_image_window_workspace_bytes(B)) as for
 *                            dva_image_tail_u8: at most two kernels, integer atomics only.
 *                            index, rolls and offsets cannot be validated without a synchronisation, so the kernels
 *                            clamp for memory safety: the source image to [0, N - 1], the source row to [0, H - 1];
 *                            the column is in range after the mod.  Values outside 0 <= index[b] < N or
 *                            0 <= offsets[b, 1] <= H - Hc are the caller's error: the result is unspecified, no access
 *                            leaves src.  Wc > W, Hc > H, Wc < 1, Hc < 1 or N < 1 with B > 0 are DVA_ERR_INVALID.
 * B <= 65535 and B H ceil(W / 4) < 2^31 (DVA_ERR_UNSUPPORTED beyond; B Hc ceil(Wc / 4) for the window); B = 0 or an
 * empty image is a no-op.  Argument errors (null pointer, negative size, more than three ops, a repeated or unknown op
 * code, a negative factor, a zero in std) return DVA_ERR_INVALID before any HIP call.  Nothing synchronises. */
#define DVA_JITTER_BRIGHTNESS 0
#define DVA_JITTER_CONTRAST 1
#define DVA_JITTER_SATURATION 2
#define DVA_IMAGE_MAX_CHANNELS 64
int64_t dva_image_tail_workspace_bytes(int64_t B);
int dva_image_tail_u8(const uint8_t* x, int64_t B, int64_t H, int64_t W, const int32_t* op_codes,
                      const double* factors, int32_t n_ops, int32_t flip, int32_t to_float, const float* mean,
                      const float* std, void* out, void* workspace, int64_t workspace_bytes, void* stream);
int dva_image_normalize_f32(const float* x, int64_t B, int64_t C, int64_t HW, const float* mean, const float* std,
                            float* out, void* stream);
int64_t dva_image_window_workspace_bytes(int64_t B);
int dva_image_window_u8(const uint8_t* src, int64_t N, int64_t H, int64_t W, const int64_t* index,
                        const int64_t* rolls, const int64_t* offsets, int64_t B, int64_t Wc, int64_t Hc,
                        const int32_t* op_codes, const double* factors, int32_t n_ops, int32_t flip, int32_t to_float,
                        const float* mean, const float* std, void* out, void* workspace, int64_t workspace_bytes,
                        void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Loading images (image_load.hip): the pixel arithmetic of SameSettingImageData.read_images
 * (core/multimodal/image.py:1059-1099) and NonStaticMask (core/data_transform/multimodal/image.py:130-154) once the
 * files are decoded.  The reference resizes with PIL.Image.resize, for RGB images Pillow's 8-bit BICUBIC resample.
 * That arithmetic is the contract, bit for bit.  Per axis (input length inSize, box [in0, in1), output length out), in
 * C double, every operation rounded on its own, no fused multiply-add -- computed by the HOST (ops.image_resample_tables):
 *   scale = filterscale = (in1 - in0) / out, filterscale = max(filterscale, 1); support = 2.0 filterscale;
 *   ksize = (int)ceil(support) * 2 + 1; for output xx: center = in0 + (xx + 0.5) scale, ss = 1.0 / filterscale,
 *   xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), inSize) - xmin,
 *   w[x] = bicubic((x + xmin - center + 0.5) ss) for x < xmax, divided by their sum ww (taken in that order) if ww != 0;
 *   bicubic(x), a = -0.5, x = |x|: ((a + 2) x - (a + 3)) x x + 1 for x < 1, (((x - 5) x + 8) x - 4) a for x < 2, else 0;
 *   k[x] = (int)(w[x] < 0 ? -0.5 + w[x] 2^22 : 0.5 + w[x] 2^22), the cast truncating toward zero.
 * A pixel and channel, on the DEVICE: int32 s = 2^21 + sum_x in[xmin + x] k[x], out = clamp(s >> 22, 0, 255), the
 * shift arithmetic.  A resize is a horizontal pass into a uint8 intermediate (a rounding point), then a vertical pass; a
 * pass whose axis keeps its length with the box covering it is skipped.
 *   dva_image_resample_u8    ONE pass along x (axis 0) or y (axis 1) over B images of 3 channels.  src and dst are
 *                            described by BYTE strides (image, row, column, channel) and their (h, w): HWC bytes are
 *                            (h w 3, w 3, 3, 1), a planar [B, 3, h, w] batch is (3 h w, w, 1, h w).  coeffs int32
 *                            [n_tables, table_rows, ksize] and bounds int32 [n_tables, table_rows, 2] = (xmin, xmax),
 *                            table_index int32 [B] (nullable: table 0) and shifts int32 [B, 3] (nullable: zeros) are
 *                            DEVICE arrays.  With i the output index along the axis and j along the other axis:
 *                              r      = i + shifts[b, 0]                 (mod out_period when out_period > 0)
 *                              a(x)   = xmin[r] + x + shifts[b, 1]       (mod src_period when src_period > 0)
 *                              o      = j + shifts[b, 2]                 (mod other_period when other_period > 0)
 *                              dst[b, i, j, c] = clamp((2^21 + sum_{x < xmax[r]} src[b, a(x), o, c] k[r, x]) >> 22)
 *                            with row r of table table_index[b]; every mod is non-negative.  These shifts fold the
 *                            roll and the crop of read_images into a pass: no rolled or cropped image is written.  A
 *                            non-zero src_period / other_period must equal the source length of its axis and
 *                            out_period may not exceed table_rows (DVA_ERR_INVALID).  Any ksize is served (the tap loop
 *                            runs to xmax[r]).  The device arrays cannot be validated without a synchronisation, so
 *                            the kernel clamps the table, its row, the tap range and every source index into range:
 *                            no access leaves src or the tables, values outside are the caller's error.  dst may not
 *                            overlap src.  One kernel, no workspace, nothing synchronises.
 *   dva_image_resample_workspace_bytes   the bytes of the HWC intermediate [B, H, W, 3] between two passes, padded as
 *                            every workspace region is.
 *   dva_image_nonstatic_mask images uint8 [n, 3, H, W] contiguous, n >= 1; mask uint8 (bool) [W, H], TRANSPOSED:
 *                              mask[x, y] = OR_{1 <= i < n} AND_c (images[0, c, y, x] != images[i, c, y, x])
 *                            (all zero for n = 1).  One kernel, a tiled transpose through LDS.
 * Argument errors (null pointer, negative size, axis other than 0 / 1, no table, a stride < 1) return DVA_ERR_INVALID
 * before any HIP call; sizes beyond int32 per axis return DVA_ERR_UNSUPPORTED; B = 0 or an empty destination is a
 * no-op. */
int64_t dva_image_resample_workspace_bytes(int64_t B, int64_t H, int64_t W);
int dva_image_resample_u8(const uint8_t* src, int64_t B, int64_t src_h, int64_t src_w, int64_t src_stride_b,
                          int64_t src_stride_y, int64_t src_stride_x, int64_t src_stride_c, uint8_t* dst, int64_t dst_h,
                          int64_t dst_w, int64_t dst_stride_b, int64_t dst_stride_y, int64_t dst_stride_x,
                          int64_t dst_stride_c, int32_t axis, const int32_t* coeffs, const int32_t* bounds,
                          int64_t n_tables, int64_t table_rows, int32_t ksize, const int32_t* table_index,
                          const int32_t* shifts, int32_t out_period, int32_t src_period, int32_t other_period,
                          void* stream);
int dva_image_nonstatic_mask(const uint8_t* images, int64_t n, int64_t H, int64_t W, uint8_t* mask, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * The positional 3D augmentations of the per-sample transform chains (cloud_augment.hip): RandomNoise, RandomRotate /
 * Random3AxisRotation, RandomScaleAnisotropic, RandomSymmetry and Center (core/data_transform/transforms.py:463-563,
 * features.py:30-81; RandomRotate and Center are torch_geometric's, of which no source or fixture exists here: for
 * those two the arithmetic below is the contract, parity is UNPINNED).  The host makes every random draw; this entry
 * applies the drawn values.  All arithmetic is fp32, every operation rounded on its own, no fused multiply-add,
 * correctly rounded division and square root.
 *   dva_cloud_augment_f32    pos fp32 [n, 3], norm fp32 [n, 3] (nullable), noise fp32 [n, 3] (nullable), all DEVICE and
 *                            contiguous.  The n_steps <= DVA_CLOUD_MAX_STEPS steps codes[k] (DVA_CLOUD_*, HOST int32)
 *                            with the parameters params[k] (HOST fp32 [n_steps, DVA_CLOUD_STEP_PARAMS], passed on by
 *                            value: q = params + DVA_CLOUD_STEP_PARAMS k) are applied in order to every point p and,
 *                            where a step says so, to its normal v:
 *                              NOISE    p_c = p_c + e_c, e = the point's row of noise.  No parameters.
 *                              LINEAR   p_i = ((p_0 M_i0 + p_1 M_i1) + p_2 M_i2), M row-major in q[0..8]; with q[9]
 *                                       != 0 (with_norm) the same for v.  Random3AxisRotation passes its matrix M
 *                                       (pos @ M^T), RandomRotate the transpose of its matrix A (pos @ A).
 *                              SCALE    p_c = p_c * s_c, s = q[0..2]; with q[9] != 0 (with_norm) v_c = v_c / s_c,
 *                                       l = sqrt((v_0 v_0 + v_1 v_1) + v_2 v_2), v_c = v_c / max(l, 1e-12f)
 *                                       (F.normalize).
 *                              FLIP     on every axis c with q[c] != 0: p_c = m_c - p_c, m_c = the exact maximum of p_c
 *                                       over the n points in their state at this step.  At least one axis.
 *                              CENTER   p_c = p_c - mu_c, mu_c = f32(S_c / n), S_c = the fp64 sum of the fp32 values
 *                                       p_c of the n points in their state at this step, the division in fp64.
 *                            out fp32 [n, 3] takes p; norm_out fp32 [n, 3] takes v and is written (and required) only
 *                            when some step has with_norm.  consts fp32 [number of FLIP and CENTER steps, 3] (DEVICE)
 *                            takes the rows m / mu the entry used, in step order, 0 on the axes a FLIP leaves alone;
 *                            it is required when such a step exists.
 *                            Launches: one reduction kernel per FLIP / CENTER step, in step order (it evaluates the
 *                            steps in front of its step on every point and writes per-block partial maxima or fp64
 *                            sums), then one apply kernel.  The partials of a reduction are combined by every block of
 *                            the next launch in a fixed order; no atomics, and the grid of a reduction depends on n
 *                            alone: the same call gives the same bytes.  Every launch reads each input row once and
 *                            the apply kernel writes each output element once.  Nothing synchronises.
 *                            Aliasing: out may be pos (and norm_out norm) only in a list WITHOUT a FLIP or CENTER
 *                            step, where a point is read and written by its own lane alone; with one, the reductions
 *                            and the apply pass must read the same input and an alias is DVA_ERR_INVALID.
 *                            workspace: dva_cloud_augment_workspace_bytes(n, n_steps) (rows of partials for up to
 *                            n_steps reducing steps), needed with a FLIP / CENTER step only; it need not be cleared.
 *                            Two deviations from the reference's torch composition are inherent: LINEAR against a BLAS
 *                            matmul (both lie within 3 * 2^-24 * sum_j |p_j| |M_ij| of the exact value, so within
 *                            twice that of each other), and CENTER against torch's fp32 mean (mu here is the correctly
 *                            rounded mean up to the fp64 summation error; torch sums in fp32).  NOISE, SCALE on pos
 *                            and FLIP are the composition's results bit for bit.  NaN coordinates are not supported.
 * Argument errors return DVA_ERR_INVALID before any HIP call: a negative size, more than DVA_CLOUD_MAX_STEPS steps, a
 * null codes / params with steps, an unknown code, NOISE without noise, with_norm without norm, a FLIP of no axis; and,
 * with n > 0, a null pos / out, a missing norm_out / consts / workspace where the list needs one, a workspace that is
 * too small.  3 n >= 2^31 is DVA_ERR_UNSUPPORTED.  n = 0 is a no-op that needs no buffer. */
#define DVA_CLOUD_NOISE 0
#define DVA_CLOUD_LINEAR 1
#define DVA_CLOUD_SCALE 2
#define DVA_CLOUD_FLIP 3
#define DVA_CLOUD_CENTER 4
#define DVA_CLOUD_MAX_STEPS 16
#define DVA_CLOUD_STEP_PARAMS 10
int64_t dva_cloud_augment_workspace_bytes(int64_t n, int32_t n_steps);
int dva_cloud_augment_f32(const float* pos, const float* norm, const float* noise, int64_t n, const int32_t* codes,
                          const float* params, int32_t n_steps, float* out, float* norm_out, float* consts,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * The tail of the segmentation step (segloss.hip).  Replaces F.log_softmax + F.nll_loss and lovasz_softmax of
 * models/segmentation/sparseconv3d.py:42-55 (metrics/lovasz_loss.py:155-202) and the argmax + bincount of
 * SegmentationTracker._compute_metrics (metrics/segmentation_tracker.py:71-91).
 * Limits of every entry: 1 <= C <= 64 (C < 1: DVA_ERR_INVALID, C > 64: DVA_ERR_UNSUPPORTED) and P C < 2^31
 * (DVA_ERR_UNSUPPORTED beyond).  Argument errors are returned before any HIP call.  No float atomics: two runs
 * give the same bits.  labels int64 [P]; a label equal to ignore_index takes no part.
 *
 *   dva_seg_logsoftmax_nll_fwd  logits [P, C] of dtype DVA_F32 / DVA_BF16 / DVA_F16, upcast exactly; log_probs fp32
 *                               [P, C] = (x - max) - log(sum exp(x - max)) in fp32.  num = sum w[y] (-logp[y]) and
 *                               den = sum w[y] over the rows whose label is in [0, C) (weight fp32 [C] nullable = all
 *                               ones; another label outside [0, C) takes no part either), reduced in fp64 from
 *                               per-block partials in a fixed order; numden fp64 [2] = {num, den}, loss fp32 [1] =
 *                               num / den (NaN when no row is counted, as torch).  Workspace:
 *                               dva_seg_nll_workspace_bytes().
 *   dva_seg_logsoftmax_nll_bwd  grad_logits [P, C] of dtype `dtype`, one pass: with g = grad_log_probs (fp32 [P, C],
 *                               nullable = 0) + [j == y] (-w[y] / den) grad_loss[0] (device fp32, nullable = 0):
 *                               grad_logits = g - exp(log_probs) sum_j g.
 *   dva_confusion_counts        counts int64 [C, C] += 1 at [label, argmax(outputs row)]; argmax as numpy's: the first
 *                               maximum, a NaN is the maximum and the first NaN wins.  Rows whose label is neither
 *                               ignore_index nor in [0, C) add 1 to n_bad int64 [1] instead.  Per-block LDS histogram,
 *                               integer atomics.
 *   dva_lovasz_softmax          lovasz_softmax_flat of probas fp32 [P, C] (any values) over the points whose label is
 *                               not ignore_index (use_ignore = 0: over all points).  Class c takes part when
 *                               class_mask[c] != 0 (uint8 [C], nullable = all) and, with present_only, when some valid
 *                               point carries label c.  Per class: err = |fg - p_c| in fp32, sorted descending, ties
 *                               in ascending point order (stable); with n_k foreground points among the first k and G
 *                               in all, J_k = 1 - (G - n_k) / (G + k - n_k) from the integer counts in fp64, J_0 = 0,
 *                               grad_k = J_k - J_{k-1}, loss_c = sum err_k grad_k in fp64.  loss fp32 [1] = the mean
 *                               over the n_used classes taking part (0 when there is none); grad fp32 [P, C] =
 *                               dloss / dprobas = sign(p - fg) grad_k / n_used rounded once, 0 where p == fg, for
 *                               ignored points and for classes that take no part.  Nothing is read back to the host.
 *                               Workspace: dva_lovasz_workspace_bytes(P, C) (24 bytes per element of probas + the
 *                               sort's own).  The segmented pass works in tiles of DVA_LOVASZ_TILE sorted elements
 *                               (dva_lovasz_tile()); the carry across tiles is one exclusive prefix per class, linear in P. */
#define DVA_LOVASZ_TILE 1024
int dva_lovasz_tile(void);
int64_t dva_seg_nll_workspace_bytes(void);
int dva_seg_logsoftmax_nll_fwd(const void* logits, int32_t dtype, const int64_t* labels, const float* weight,
                               int64_t ignore_index, int64_t P, int32_t C, float* log_probs, float* loss,
                               double* numden, void* workspace, int64_t workspace_bytes, void* stream);
int dva_seg_logsoftmax_nll_bwd(const float* log_probs, const int64_t* labels, const float* weight,
                               const double* numden, const float* grad_loss, const float* grad_log_probs,
                               int64_t ignore_index, int64_t P, int32_t C, void* grad_logits, int32_t dtype,
                               void* stream);
int dva_confusion_counts(const void* outputs, int32_t dtype, const int64_t* labels, int64_t ignore_index, int64_t P,
                         int32_t C, int64_t* counts, int64_t* n_bad, void* stream);
int64_t dva_lovasz_workspace_bytes(int64_t P, int32_t C);
int dva_lovasz_softmax(const float* probas, const int64_t* labels, int64_t P, int32_t C, int64_t ignore_index,
                       int32_t use_ignore, const uint8_t* class_mask, int32_t present_only, float* loss, float* grad,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Voting on the raw cloud and K-NN interpolation of the votes (vote.hip).  Replaces the host accumulation
 * `votes[ids] += outputs; counts[ids] += 1` of metrics/s3dis_tracker.py:56-61, metrics/segmentation_helpers.py
 * (SegmentationVoter.add_vote) and metrics/kitti360_tracker.py:144-152, and torch_geometric's knn_interpolate + argmax +
 * ConfusionMatrix of s3dis_tracker.py:94-118, segmentation_helpers.py:76-83 and kitti360_tracker.py:188-222.
 * Limits: 1 <= C <= 64 (C < 1: DVA_ERR_INVALID, C > 64: DVA_ERR_UNSUPPORTED), N, P, M < 2^31, n k < 2^31, k <= 128
 * (DVA_ERR_UNSUPPORTED beyond).  Argument errors are returned before any HIP call; zero rows is a no-op.  No float
 * atomics: two runs give the same bits.  Nothing synchronises.
 *
 *   dva_vote_add          votes fp32 [N, C] and counts int32 [N], in place: for every id in ids int64 [P] that lies in
 *                         [0, N), votes[id] += outputs[p] and counts[id] += 1 with p the LAST row of this call that
 *                         carries the id (an id that occurs several times is counted once, as in the reference, where
 *                         torch leaves open which occurrence).  outputs [P, C] of dtype DVA_F32 / DVA_BF16 / DVA_F16,
 *                         widened exactly.  An id outside [0, N) writes nothing and adds 1 to n_bad int64 [1].
 *                         slots int32 [dva_vote_workspace_bytes(N) / 4]: all -1 on entry (the caller fills it once)
 *                         and all -1 again on exit.
 *   dva_knn_interpolate   x fp32 [M, C]; neighbors int32 [n, k] and dist2 fp32 [n, k] as dva_knn_query returns them
 *                         (k <= M).  Per query, in fp32, every operation rounded on its own, in neighbour rank order:
 *                         w_r = 1 / max(d2_r, 1e-16); num = ((0 + x[nbr_0] w_0) + x[nbr_1] w_1) + ...;
 *                         den = ((0 + w_0) + w_1) + ...; value = num / den: torch_geometric's knn_interpolate.
 *                         own int32 [n] (nullable): where own[i] >= 0 the value of query i is the row x[own[i]] as it
 *                         is (a point that has votes keeps them; kitti360_tracker.py:219-222).
 *                         Outputs, each nullable, at least one given: y fp32 [n, C] = the values; pred int64 [n] =
 *                         their argmax as numpy's (the first maximum, a NaN is the maximum); counts int64 [C, C] += 1
 *                         at [labels[i], pred[i]] (labels int64 [n], required with counts) for the rows whose label is
 *                         not ignore_index, a label outside [0, C) adding 1 to n_bad int64 [1] instead (required
 *                         with counts).  A neighbour or own index outside [0, M) gives a NaN row, pred -1, no count
 *                         and 1 in n_bad.  With y NULL no [n, C] buffer exists. */
int64_t dva_vote_workspace_bytes(int64_t N);
int dva_vote_add(float* votes, int32_t* counts, int64_t N, int32_t C, const int64_t* ids, const void* outputs,
                 int32_t dtype, int64_t P, int32_t* slots, int64_t slots_bytes, int64_t* n_bad, void* stream);
int dva_knn_interpolate(const float* x, int64_t M, int32_t C, const int32_t* neighbors, const float* dist2, int64_t n,
                        int32_t k, const int32_t* own, float* y, int64_t* pred, const int64_t* labels,
                        int64_t ignore_index, int64_t* counts, int64_t* n_bad, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Lexicographic integer keys. Replace utils/multimodal.py:36-94 (lexargsort / lexargunique on a
 * composite int64 key, :97-179 CompositeTensor, :253-323 lex ops).
 * ------------------------------------------------------------------------------------------ */

/* Bytes of temporary storage the two functions below need for n keys. */
int64_t dva_lex_workspace_bytes(int64_t n);
/* order[i] = index of the i-th smallest key; STABLE (ties keep input order), which is one of the
 * orders numpy's unstable argsort (multimodal.py:316) may return. keys_sorted nullable. */
int dva_argsort_i64(const int64_t* keys, int64_t n, int64_t* order, int64_t* keys_sorted,
                    void* workspace, int64_t workspace_bytes, void* stream);
/* first[j] = smallest input index carrying the j-th smallest distinct key (numpy
 * unique(return_index=True), multimodal.py:310); *n_unique written to device memory. */
int dva_argunique_i64(const int64_t* keys, int64_t n, int64_t* first, int64_t* n_unique_dev,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Mapping build (point -> pixel visibility).  Replaces SplattingVisibility.__call__
 * = camera_projection_cpu + visibility_from_splatting_cpu + postprocess_features
 * (core/multimodal/visibility.py:478-538, :1073-1195, :1548-1582, glue :1699-1757).
 * The CPU/numba path is the semantic reference (README.md:122-123).
 * ------------------------------------------------------------------------------------------ */
typedef struct dva_camera {
  int32_t model;        /* DVA_CAM_* */
  int32_t img_w, img_h; /* projection map size (proj_size) */
  int32_t crop_top, crop_bottom;
  float r_min, r_max;   /* informative copies; the range test uses r_min_d / r_max_d */
  float img_xyz[3];     /* camera centre */
  /* Row-major 3x3 / 3-vector the projection multiplies by, prepared by the host exactly like the
   * reference does per image (scalar work): equirect: rot = M_o.M_p.M_k from opk
   * (visibility.py:57-90), v = (xyz - img_xyz).rot^T; 'scannet': (rot, trans) =
   * inv(extrinsic)[:3,:3|3] (:232-236), p = rot.xyz + trans; kitti perspective / fisheye:
   * (rot, trans) = extrinsic[:3,:3|3] (:238-242, :304-308), p = rot^T.(xyz - trans). */
  float rot[9];
  float trans[3];
  float fx, fy, mx, my; /* pinhole intrinsics [0][0], [1][1], [0][2], [1][2] */
  float fisheye[7];     /* xi, k1, k2, gamma1, gamma2, u0, v0 */
  double r_min_d, r_max_d; /* float64 scalars (numba promotes the float32 distances to compare) */
  double voxel, k_swell, d_swell;
  int32_t exact;
} dva_camera;

/* Bytes of device workspace dva_visibility needs for n candidate points and this camera. */
int64_t dva_visibility_workspace_bytes(const dva_camera* cam, int64_t n);

/* One image.  xyz fp32 [n,3] candidate points IN CALLER ORDER (tie-breaks depend on it),
 * mask nullable uint8 [img_w, img_h] (indexed [x][y], visibility.py:427-432).
 * Outputs (capacity n each when cam->exact, else max(n, img_w * cropped_h) since every covered pixel is
 * emitted; *n_out_dev = q written on device), in the reference's output order
 * (x-major, then y; visibility.py:1190-1195):
 *   idx   int64[q] index into xyz          x_pix,y_pix int64[q]   depth fp32[q]
 *   x_proj,y_proj fp64[q] float projection of the surviving points (for mapping features)
 */
int dva_visibility(const float* xyz, int64_t n, const dva_camera* cam, const uint8_t* mask,
                   int64_t* idx, int64_t* x_pix, int64_t* y_pix, float* depth, double* x_proj,
                   double* y_proj, int64_t* n_out_dev, void* workspace, int64_t workspace_bytes,
                   void* stream);

/* camera_projection alone (reference core/multimodal/visibility.py:478-538: range, field-of-view / crop / mask cull,
 * float projection), survivors in candidate order: idx int64[m], depth fp32[m], x_proj / y_proj fp64[m] (capacity n),
 * *n_out_dev = m.  The start of the visibility models other than the splatting one (DepthBasedVisibility,
 * BiasuttiVisibility: visibility.py:1356-1496, :1779-1803).  Workspace: dva_visibility_workspace_bytes(cam, n). */
int dva_camera_projection(const float* xyz, int64_t n, const dva_camera* cam, const uint8_t* mask, int64_t* idx,
                          float* depth, double* x_proj, double* y_proj, int64_t* n_out_dev, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* B images of ONE setting in one set of launches (reference core/data_transform/multimodal/image.py:192-428 loops
 * over the images; core/multimodal/visibility.py:1073-1195 per image).  cam0 (host) = the camera of image 0: projection
 * size, crops, model, exact, splatting parameters must be the same for all images; cams_dev = device array of the
 * n_images cameras (poses / intrinsics per image).  Outputs as dva_visibility, rows of all images concatenated
 * image-major (capacity n_images x the single-image capacity), row_ptr int64 [n_images + 1] = first row of every
 * image (device), *n_out_dev = total.  No host synchronisation inside. */
int64_t dva_visibility_batch_workspace_bytes(const dva_camera* cam0, int64_t n, int32_t n_images);
int dva_visibility_batch(const float* xyz, int64_t n, const dva_camera* cam0, const dva_camera* cams_dev,
                         int32_t n_images, const uint8_t* mask, int64_t* idx, int64_t* x_pix, int64_t* y_pix,
                         float* depth, double* x_proj, double* y_proj, int64_t* row_ptr, int64_t* n_out_dev,
                         void* workspace, int64_t workspace_bytes, void* stream);
/* dva_mapping_features for the rows of dva_visibility_batch (the camera of a row follows from row_ptr);
 * row_image int32 [q] nullable receives the image of every row. */
int dva_mapping_features_batch(const float* xyz, const int64_t* idx, const float* depth, const double* y_proj,
                               const float* linearity, const float* planarity, const float* scattering,
                               const float* normals, const dva_camera* cams_dev, const int64_t* row_ptr,
                               int32_t n_images, int64_t q, float* features, int32_t* row_image, int32_t* n_cols,
                               void* stream);

/* Mapping features of the q surviving points (visibility.py:1548-1582); nullable inputs drop
 * their column exactly like the reference. features fp32 [q, n_cols], column order:
 * depth, linearity, planarity, scattering, orientation, pixel height. Returns n_cols via *n_cols. */
int dva_mapping_features(const float* xyz, const int64_t* idx, const float* depth,
                         const double* y_proj, const float* linearity, const float* planarity,
                         const float* scattering, const float* normals, const dva_camera* cam,
                         int64_t q, float* features, int32_t* n_cols, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Mapping merge after a strided 3D convolution.  Replaces ImageMapping.select_points(idx,
 * mode='merge') + from_dense (core/multimodal/image.py:2211-2273, :1728-1795): point i becomes voxel
 * idx[i]; the views of a voxel's points are united per image (ascending image id), duplicate pixels
 * of a merged view removed (ascending x, then y), the features of a merged view are the fp32 mean of
 * its source views, added in ascending point order and divided by their number.
 * Mapping over n_points points: pointers int64 [n_points + 1], images int64 [n_views] (< 2^31),
 * atom_ptr int64 [n_views + 1], pixels int16 [n_atoms, 2] as (x, y), non-negative (pixel_bytes = 2;
 * 1 / 4 / 8 return DVA_ERR_UNSUPPORTED), features fp32 [n_views, F] nullable; idx int64 [n_points].
 * n_points, n_views, n_atoms >= 2^31 - 1 return DVA_ERR_UNSUPPORTED.
 * dva_mapping_merge_count writes sizes[4] (device) = {M = max(idx) + 1, views of the result, atoms of
 * the result, ok}; ok = 0 when some id in [0, M) has no point or an id is outside [0, n_points): the
 * caller keeps the input mapping (image.py:2229-2233) and does not call the fill.  The caller reads
 * sizes back (the only host synchronisation of the operation), allocates the outputs and calls
 * dva_mapping_merge_fill with the SAME workspace, untouched in between: out_pointers int64 [M + 1],
 * out_images int64 [V'], out_atom_ptr int64 [V' + 1], out_pixels int16 [P', 2], out_features fp32
 * [V', F] (null iff features is null).  Every output element is written exactly once, without float
 * atomics: two calls give the same bits.  dva_mapping_merge_tile_atoms: the atoms of a voxel up to
 * which it is merged in LDS; larger voxels are sorted in the workspace.
 * ------------------------------------------------------------------------------------------ */
int dva_mapping_merge_tile_atoms(void);
int64_t dva_mapping_merge_workspace_bytes(int64_t n_points, int64_t n_views, int64_t n_atoms);
int dva_mapping_merge_count(const int64_t* pointers, const int64_t* images, const int64_t* atom_ptr,
                            const void* pixels, int32_t pixel_bytes, const int64_t* idx, int64_t n_points,
                            int64_t n_views, int64_t n_atoms, int64_t* sizes, void* workspace,
                            int64_t workspace_bytes, void* stream);
int dva_mapping_merge_fill(const int64_t* pointers, const int64_t* images, const int64_t* atom_ptr,
                           const void* pixels, int32_t pixel_bytes, const float* features, int32_t F,
                           int64_t n_points, int64_t n_views, int64_t n_atoms, int64_t n_voxels,
                           int64_t n_views_out, int64_t n_atoms_out, int64_t* out_pointers, int64_t* out_images,
                           int64_t* out_atom_ptr, void* out_pixels, float* out_features, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Mapping selection.  Replaces the torch compositions of ImageMapping.select_points(mode='pick'),
 * select_images, select_views and crop (core/multimodal/image.py:2029-2342, csr.py:235-294): one
 * filter / compact / renumber of the nested CSR point -> views -> atoms, with one readback.
 * Mapping as for the merge (pixels int16, pixel_bytes = 2; 1 / 4 / 8 return DVA_ERR_UNSUPPORTED;
 * features fp32 [n_views, F] nullable).  Output point m is source point point_idx[m] (int64 [n_out],
 * any order, duplicates allowed; null: all points in order, n_out = n_points).  A source view
 * survives if view_mask (uint8 [n_views], nullable) is set for it and
 *   image_map without image_keys: image_map[image] >= 0 (int64 [n_map]; an image >= n_map is dropped),
 *   image_map with image_keys:    image == image_keys[k] for some k and image_map[k] >= 0 (image_keys
 *                                 int64 [n_map] ASCENDING; a repeated key sets flag bit 2),
 * and it gets that new id.  compact (exclusive with image_map): the new id of a surviving view is the
 * rank of its image among the distinct surviving images, which must be < n_images.  crop_offsets (int64
 * [n_images, 2], exclusive with image_map and compact): atom pixels become pixel - offset[image] in
 * int16 arithmetic, atoms outside [0, crop_w) x [0, crop_h) and views left without atoms are dropped,
 * the surviving views of a point are ordered by ascending image, stably, and the features of a view
 * are acc = 0; acc += f (c times); acc /= (float)c for its c surviving atoms.  Two surviving views of
 * one point with the same image set flag bit 0.  n_images is 0 without compact and crop.
 * dva_mapping_select_count writes sizes (device int64 [4 + n_images]) = {views of the result, atoms of
 * the result, distinct images, flags, the distinct images ascending ...}: the distinct images are those
 * of the surviving views with compact, and of the source views that pass view_mask with a crop.
 * flags: bit 0 unsupported (see above, or 2^31 - 1 or more views or atoms in the result), bit 1 a point
 * index or image id out of range, bit 2 a repeated image key; with any of them set the fill must not
 * be called.  The caller reads sizes back (the only host synchronisation), allocates the outputs and
 * calls dva_mapping_select_fill with the SAME arguments and workspace, untouched in between:
 * out_pointers int64 [n_out + 1], out_images int64 [V'], out_atom_ptr int64 [V' + 1], out_pixels int16
 * [P', 2], out_features fp32 [V', F] (null when features is null; an empty output may be null).  Every
 * output element is written exactly once, without float atomics; features are copied as bits except
 * under a crop.
 * dva_mapping_select_tile_views: the views of a point up to which a crop orders them in LDS.
 * Sizes of 2^31 - 1 or more return DVA_ERR_UNSUPPORTED.
 * dva_mapping_image_stats: stats int64 [5, n_images] = per image id < n_images the number of atoms,
 * then min x, max x, min y, max y of its pixels (integer atomics), INT64_MAX / INT64_MIN for the minima /
 * maxima of an image without atoms; views of other image ids are skipped.
 * ------------------------------------------------------------------------------------------ */
int dva_mapping_select_tile_views(void);
int64_t dva_mapping_select_workspace_bytes(int64_t n_out, int64_t n_views, int64_t n_images, int32_t crop);
int dva_mapping_select_count(const int64_t* pointers, const int64_t* images, const int64_t* atom_ptr,
                             const void* pixels, int32_t pixel_bytes, int64_t n_points, int64_t n_views,
                             int64_t n_atoms, const int64_t* point_idx, int64_t n_out, const uint8_t* view_mask,
                             const int64_t* image_keys, const int64_t* image_map, int64_t n_map, int32_t compact,
                             int64_t n_images, int64_t crop_w, int64_t crop_h, const int64_t* crop_offsets,
                             int64_t* sizes, void* workspace, int64_t workspace_bytes, void* stream);
int dva_mapping_select_fill(const int64_t* pointers, const int64_t* images, const int64_t* atom_ptr,
                            const void* pixels, int32_t pixel_bytes, const float* features, int32_t F,
                            int64_t n_points, int64_t n_views, int64_t n_atoms, const int64_t* point_idx,
                            int64_t n_out, const uint8_t* view_mask, const int64_t* image_keys,
                            const int64_t* image_map, int64_t n_map, int32_t compact, int64_t n_images, int64_t crop_w,
                            int64_t crop_h, const int64_t* crop_offsets, int64_t n_views_out, int64_t n_atoms_out,
                            int64_t* out_pointers, int64_t* out_images, int64_t* out_atom_ptr, void* out_pixels,
                            float* out_features, void* workspace, int64_t workspace_bytes, void* stream);
int dva_mapping_image_stats(const int64_t* images, const int64_t* atom_ptr, const void* pixels, int32_t pixel_bytes,
                            int64_t n_views, int64_t n_atoms, int64_t n_images, int64_t* stats, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * The image picks (csrc/mapping_pick.hip): CenterRoll and the coverage counts of
 * PickImagesFromMemoryCredit (core/data_transform/multimodal/image.py:962-1037, :765-874).  Mapping
 * arrays as for the selection (pixels int16, pixel_bytes = 2; 1 / 4 / 8 return DVA_ERR_UNSUPPORTED).
 *
 * dva_mapping_center_rollings: rollings int64 [n_images] = per image the roll r * width >> 8 of the
 *   first candidate r in {0, step, 2 step, ... < 256}, step = 256 / angular_res (integer division,
 *   angular_res in 1..256), that minimises (hi - lo) + (|hi + lo - 256| >> 1), lo / hi the minimum /
 *   maximum of (c + r) mod 256 over the distinct c = x * 256 / width of the image's atom columns x:
 *   for 0 <= x < width <= 32767 the reference's float expressions (:999-1029) exactly.  An image
 *   without atoms gets 0.  info int32 [2] = {images without atoms, flags}; flag bit 0: a view whose image
 *   is outside [0, n_images), bit 1: an atom column outside [0, width); such views / atoms are left out
 *   and the caller decides.  Integer OR atomics into a 256-bit occupancy bitmap per image: the result
 *   does not depend on their order.  workspace: dva_mapping_center_workspace_bytes(n_images) bytes,
 *   4-byte aligned.  width > 32767 returns DVA_ERR_UNSUPPORTED.
 * dva_mapping_roll_pixels: x = (x + rollings[image]) mod width (the sign of width) IN PLACE in the
 *   column of every atom; views whose image is outside [0, n_images) are left alone.
 * dva_mapping_coverage_step: one step of the coverage counts over n_items mappings of the SAME
 *   n_points points (items is a HOST array, read before the entry returns; item b has n_points <= the
 *   total, its images are the global ids image_base .. image_base + n_images - 1, bases ascending
 *   without overlap inside n_images).  covered uint8 [n_points] is the state, zero before the first
 *   step.  With pick a global image id (or -1): covered[p] is set for every point p that pick sees;
 *   then counts[i] += 1 for every view (p, i) of a point still uncovered, so that on a counts row that
 *   was zero counts[i] = |{p : image i sees p, no picked image sees p}|, the row sums of the
 *   reference's dense matrix (:803-868).  PRECONDITION: a view is a distinct (point, image) pair, as in
 *   every mapping from_dense builds; a repeated pair counts twice.  counts int64 [n_images] must be zero
 *   on entry; clear (int64 [n_images], nullable, not counts) is zeroed by the same launch: the row of
 *   the next step.  Up to dva_mapping_coverage_hist_images() images in all a workgroup counts in an LDS
 *   histogram and flushes one integer atomic per non-zero bin; above, global integer atomics.  No float
 *   atomics.  dva_mapping_coverage_group_items() = 32 items per launch, by value.
 * ------------------------------------------------------------------------------------------ */
struct dva_coverage_item {
  const int64_t* pointers;
  const int64_t* images;
  int64_t n_points;
  int64_t n_views;
  int64_t n_images;
  int64_t image_base;
};
int64_t dva_mapping_center_workspace_bytes(int64_t n_images);
int dva_mapping_center_rollings(const int64_t* images, const int64_t* atom_ptr, const void* pixels, int32_t pixel_bytes,
                                int64_t n_views, int64_t n_atoms, int64_t n_images, int64_t width, int32_t angular_res,
                                int64_t* rollings, int32_t* info, void* workspace, int64_t workspace_bytes,
                                void* stream);
int dva_mapping_roll_pixels(const int64_t* images, const int64_t* atom_ptr, void* pixels, int32_t pixel_bytes,
                            int64_t n_views, int64_t n_atoms, const int64_t* rollings, int64_t n_images,
                            int64_t width, void* stream);
int dva_mapping_coverage_group_items(void);
int dva_mapping_coverage_hist_images(void);
int dva_mapping_coverage_step(const struct dva_coverage_item* items /* HOST array */, int64_t n_items,
                              int64_t n_points, int64_t n_images, int64_t pick, uint8_t* covered, int64_t* counts,
                              int64_t* clear, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * Mapping collation.  Replaces the torch composition of CSRBatch.from_csr_list on ImageMappings
 * followed by insert_empty_groups (core/multimodal/csr.py:352-420, :197-229): n_items mappings
 * stacked into one, without a host synchronisation.  items is a HOST array, read before the entry
 * returns and not kept: item b has pointers int64 [n_points + 1], images int64 [n_views], atom_ptr
 * int64 [n_views + 1], pixels int16 [n_atoms, 2] (pixel_bytes = 2; anything else returns
 * DVA_ERR_UNSUPPORTED), features fp32 [n_views, F] (null for every item when F = 0), all device
 * arrays, and its destination point_base: ascending, point_base[b] >= point_base[b-1] +
 * n_points[b-1], and n_points_out >= the end of the last item.  n_views_out and n_atoms_out are the
 * sums over the items.  With view_base[b] / atom_base[b] the views / atoms of the items before b:
 *   out_pointers int64 [n_points_out + 1]: entry 0 is 0, entry point_base[b] + i (1 <= i <=
 *     n_points[b]) is pointers_b[i] + view_base[b], and every entry no item covers (in front of the
 *     first item, between two items, behind the last) holds the views stacked so far;
 *   out_images int64 [n_views_out]: images_b[j] + off[b] at view_base[b] + j, off[b] the sum over
 *     c < b of max(images_c) + 1 (int64 arithmetic; 0 for an item without views), reduced and
 *     scanned on the device; out_image_offsets (device int64 [n_items], nullable) receives off;
 *   out_atom_ptr int64 [n_views_out + 1]: entry 0 is 0, entry view_base[b] + j (1 <= j <= n_views[b])
 *     is atom_ptr_b[j] + atom_base[b];
 *   out_pixels int16 [n_atoms_out, 2] and out_features fp32 [n_views_out, F]: copied as bits.
 * Every output element is written exactly once, without atomics; only the sizes bound the accesses,
 * never a value read from pointers or atom_ptr.  The item descriptors reach the kernels by value,
 * dva_mapping_collate_group_items() = 32 per launch: up to 32 items are three launches (maxima,
 * scan, fill), every further 32 add a maxima and a fill launch.  No allocation and no copy inside
 * the entry, and no host memory kept after it returns.  Bad arguments (null items or outputs, n_items < 1,
 * negative sizes, bases that descend or overlap, sums that differ from the totals) return
 * DVA_ERR_INVALID before any HIP call; totals of 2^31 - 1 or more return DVA_ERR_UNSUPPORTED.
 * workspace: dva_mapping_collate_workspace_bytes(n_items) bytes, 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
struct dva_collate_item {
  const int64_t* pointers;
  const int64_t* images;
  const int64_t* atom_ptr;
  const void* pixels;
  const float* features;
  int64_t n_points;
  int64_t n_views;
  int64_t n_atoms;
  int64_t point_base;
};
int dva_mapping_collate_group_items(void);
int64_t dva_mapping_collate_workspace_bytes(int64_t n_items);
int dva_mapping_collate(const struct dva_collate_item* items /* HOST array */, int64_t n_items, int32_t pixel_bytes,
                        int32_t F, int64_t n_points_out, int64_t n_views_out, int64_t n_atoms_out,
                        int64_t* out_pointers, int64_t* out_images, int64_t* out_atom_ptr, void* out_pixels,
                        float* out_features, int64_t* out_image_offsets /* device [n_items], nullable */,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ *
 * The tail of the image-only models (models/segmentation/multimodal/no3d.py:102-154): nearest-seen
 * fill in eval mode (csrc/nearest_seen.hip) and the view-level loss (csrc/view_loss.hip).
 *
 * dva_nearest_seen   pos fp32 [n, 3], seen uint8 [n] (non-zero = seen), bbox = device fp32[6] (min xyz |
 *   max xyz of pos).  src int32 [n]: src[i] = i for a seen point; for an unseen point the index, in
 *   the numbering of pos, of the seen point with the smallest d2 = ((dx*dx + dy*dy) + dz*dz), every
 *   operation rounded on its own in fp32 (the distance of dva_knn_query), ties to the lowest index.
 *   With no seen point src[i] = i everywhere and any_seen[0] = 0 (else 1).  The whole array is one
 *   cloud: a batch is searched across its samples, as the reference does.
 *   Levels as for dva_knn: a call with last = 0 walks at most max_shell shells of cells around each
 *   unfinished query (done uint8 [n], zeroed by the caller before the first call) and finishes those
 *   whose neighbour is provably final; the call with last != 0 walks every shell the box holds, so
 *   it finishes every query for ANY cell (the cell affects time only; a cell below extent / 2^19, in
 *   the last call below extent / 16, is raised to that on the device), and writes src of the seen points and any_seen.  With x
 *   ([n, K] of dtype, K <= 2^20; last call only) the same launch also writes filled[i] = x[src[i]],
 *   rows copied as bits; filled must not alias x.  No float atomics: two runs give the same bits.
 *   Nothing is read back to the host and the number of seen points is never needed.
 *   n < 2^30 (DVA_ERR_UNSUPPORTED beyond); n = 0 is a no-op; bad arguments return before any HIP call.
 *
 * dva_view_nll_*   the loss nll_loss(log_softmax(x_view), repeat_interleave(labels, views per point))
 *   of views that are a gather x_view[v] = rows[row_idx[v]] (row_idx int32 [n_views]; null = the
 *   identity, n_rows = n_views), without x_view and without the repeated labels.  csr_idx int64
 *   [n_points + 1] are the view pointers, labels int64 [n_points]; a view counts when its point's
 *   label is not ignore_index and lies in [0, K); 1 <= K <= 64 and n_rows K < 2^31, n_views < 2^31
 *   (DVA_ERR_UNSUPPORTED beyond).
 *     counts  cnt int32 [n_rows, K], zeroed by the call: cnt[r][c] = counted views of row r whose
 *             point has label c (int32 atomics: exact, so every run gives the same bits).
 *     fwd     rows [n_rows, K] of dtype, upcast exactly; weight fp32 [K] (nullable: ones).
 *             loss[0] = num / den, num = sum cnt w_c (-logp_r[c]), den = sum cnt w_c, reduced in fp64
 *             in a fixed order; numden fp64 [2] keeps both; NaN when no view counts.
 *     bwd     grad_rows[r][c] = grad_loss[0] / den * ((sum_c' cnt[r][c'] w_c') softmax_r[c] - cnt[r][c] w_c)
 *             in the rows' dtype; a row without counted views gets zeros.
 *   Nothing synchronises with the host.
 * ------------------------------------------------------------------------------------------ */
int64_t dva_nearest_seen_workspace_bytes(int64_t n);
int dva_nearest_seen(const float* pos, const uint8_t* seen, int64_t n, const float* bbox, float cell,
                     int32_t max_shell, int32_t last, uint8_t* done, int32_t* src, uint8_t* any_seen, const void* x,
                     int32_t K, int32_t dtype, void* filled, void* workspace, int64_t workspace_bytes, void* stream);
int64_t dva_view_nll_workspace_bytes(void);
int dva_view_nll_counts(const int32_t* row_idx, int64_t n_views, const int64_t* csr_idx, const int64_t* labels,
                        int64_t n_points, int64_t ignore_index, int64_t n_rows, int32_t K, int32_t* cnt,
                        void* stream);
int dva_view_nll_fwd(const void* rows, int32_t dtype, const int32_t* cnt, const float* weight, int64_t n_rows,
                     int32_t K, float* loss, double* numden, void* workspace, int64_t workspace_bytes, void* stream);
int dva_view_nll_bwd(const void* rows, int32_t dtype, const int32_t* cnt, const float* weight, const double* numden,
                     const float* grad_loss, int64_t n_rows, int32_t K, void* grad_rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVA_H_ */
