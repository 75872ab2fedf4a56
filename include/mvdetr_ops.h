/* mvdetr_ops.h -- C ABI of libmvdetr_ops.so: the MI355X (gfx950) kernels of MVDeTr's multiview
 * ground-plane fusion path.
 *
 * This is the drop-in boundary.  Each entry point replaces one host launcher of the reference's
 * CUDA extension (paths relative to the reference checkout), keeps that launcher's argument
 * order and meaning, and differs from it only in returning the HIP error code instead of
 * printf-ing it (ms_deform_im2col_cuda.cuh:948-952, 1321-1325 swallow launch failures).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (including spatial_shapes / level_start_index, which the
 *     reference also reads on the device: ms_deform_attn_cuda.cu:67-68); no host copies, no
 *     synchronisation, no allocation: work is enqueued on `stream` and the call returns.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - tensors are dense row-major with the shapes given below; fp32 (`_f32`) or fp64 (`_f64`),
 *     like AT_DISPATCH_FLOATING_TYPES in ms_deform_attn_cuda.cu:64,134.
 *   - return value: 0 (hipSuccess) or a hipError_t; 1 (hipErrorInvalidValue) for bad arguments.
 *   - thread-safe and re-entrant: the only global state is the forward-variant knob below
 *     (an atomic int, initialised from the environment variable MVDETR_MSDA_FWD_IMPL).
 */
#ifndef MVDETR_OPS_H
#define MVDETR_OPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVDETR_OPS_ABI_VERSION 18   /* 12: + mvdetr_warp_perspective_backward_tagged_*; 13: + mvdetr_msda_set_backward_deterministic; the fused training pair takes every encoder shape; 14: + mvdetr_msda_get_backward_deterministic; 15: + mvdetr_deform_conv2d_*; 16: + mvdetr_attention_*; still 16 with mvdetr_bn_act_f32, mvdetr_bn_relu_maxpool_f32, mvdetr_trunk_* and with mvdetr_focal_loss_*, mvdetr_reg_l1_loss_*, mvdetr_loss_* (purely additive: nothing existing changed, and the loader looks every symbol up by name, so a stale build still fails to load); 17: + mvdetr_msda_last_backward_route; still 17 with mvdetr_bn_act_f16 / _bf16 and mvdetr_bn_relu_maxpool_f16 / _bf16, and with mvdetr_winograd_*, mvdetr_conv3x3_winograd_f32 (purely additive again); 18: + mvdetr_add_layernorm_last_kernel; still 18 with mvdetr_attn_forward_f16 / _bf16 and mvdetr_deform_conv2d_forward_f16 / _bf16 (purely additive), and with the mvdetr_frame_targets_* entries (additive too), and with mvdetr_deform_conv2d_route_kind, mvdetr_attention_route_kind (additive) */

/* ABI version of the loaded library (checked by the Python loader). */
int mvdetr_ops_abi_version(void);

/* ---- Multi-scale deformable attention, forward ------------------------------------------------
 * Replaces ms_deformable_im2col_cuda (ms_deform_im2col_cuda.cuh:923-954) and the kernel it
 * launches (cuh:237-299, device helper cuh:33-84).
 *   value            [batch, spatial_size, num_heads, channels]
 *   spatial_shapes   [num_levels, 2]  int64 (H_l, W_l)
 *   level_start_index[num_levels]     int64, token offset of level l inside spatial_size
 *   sampling_loc     [batch, num_query, num_heads, num_levels, num_point, 2]  (x, y) in [0,1]
 *   attn_weight      [batch, num_query, num_heads, num_levels, num_point]
 *   out              [batch, num_query, num_heads*channels]   (every element is written)
 */
int mvdetr_msda_forward_f32(void *stream, const float *value, const int64_t *spatial_shapes,
                            const int64_t *level_start_index, const float *sampling_loc,
                            const float *attn_weight, int batch, int spatial_size, int num_heads,
                            int channels, int num_levels, int num_query, int num_point, float *out);
int mvdetr_msda_forward_f64(void *stream, const double *value, const int64_t *spatial_shapes,
                            const int64_t *level_start_index, const double *sampling_loc,
                            const double *attn_weight, int batch, int spatial_size, int num_heads,
                            int channels, int num_levels, int num_query, int num_point, double *out);

/* 16-bit storage variants of the forward (an extension: the reference dispatches float and double only,
 * ms_deform_attn_cuda.cu:64, so under autocast its callers cast to fp32 around the op).  Tensors as above with
 * IEEE binary16 (`_f16`) or bfloat16 (`_bf16`) elements passed as raw 16-bit words; every arithmetic step is fp32 and
 * the result is rounded once (nearest-even) when stored.  Forward only; device pointers only. */
int mvdetr_msda_forward_f16(void *stream, const uint16_t *value, const int64_t *spatial_shapes,
                            const int64_t *level_start_index, const uint16_t *sampling_loc,
                            const uint16_t *attn_weight, int batch, int spatial_size, int num_heads, int channels,
                            int num_levels, int num_query, int num_point, uint16_t *out);
int mvdetr_msda_forward_bf16(void *stream, const uint16_t *value, const int64_t *spatial_shapes,
                             const int64_t *level_start_index, const uint16_t *sampling_loc,
                             const uint16_t *attn_weight, int batch, int spatial_size, int num_heads, int channels,
                             int num_levels, int num_query, int num_point, uint16_t *out);

/* Fused forward for deformable-encoder calls: the arithmetic MSDeformAttn.forward wraps around the core
 * (multiview_detector/models/ops/modules/ms_deform_attn.py:100-107) happens inside the kernel, so the
 * sampling_locations / attention_weights tensors are never written or re-read:
 *     loc = reference_points[:, :, None] + sampling_offsets / (W_l, H_l);  aw = softmax_{L*P}(attn_logits)
 *   reference_points [*, num_query, num_levels, num_point, 2]; consecutive batch elements are
 *                    `ref_batch_stride` floats apart (0 = one set shared by the whole batch)
 *   sampling_offsets [batch, num_query, num_heads, num_levels, num_point, 2]  (the Linear's raw output)
 *   attn_logits      [batch, num_query, num_heads, num_levels, num_point]     (the Linear's raw output)
 *   level_major      bit mask.  Bit 0 (1): the two raw tensors are [batch, num_query, num_levels, num_heads,
 *                    num_point(, 2)] instead -- the caller permutes the Linear's weight rows once; keeps what one
 *                    level iteration reads in the same cache lines.  Bit 1 (2): reference_points is
 *                    [*, num_query, num_levels, 2], ONE point per (query, level) shared by the num_point sampling
 *                    points -- what MVDeTr's reference map holds P copies of (mvdetr.py:49-58 with all heights 0);
 *                    a quarter of the reference bytes.  Bit 2 (4), not together with bit 0: ONE raw tensor
 *                    [batch, num_query, num_heads / g, num_levels, (g x num_point x 2 offsets | g x num_point logits)]
 *                    with g = 32 / channels heads per 128-byte slice of the token row, again a permutation of the
 *                    Linears' weight rows: everything one workgroup reads for a (query, level) is one contiguous run
 *                    of 12 g floats (the kernel is bound by the number of cache lines a CU can miss on, and the plain
 *                    layouts fetch a 128-byte line for 32 or 64 of its bytes); `sampling_offsets` points at the tensor,
 *                    `attn_logits` must equal sampling_offsets + 8 g and the two query strides must be equal.
 *                    Bit 3 (8), only with bit 1: reference_points is [*, num_levels, num_query, 2] (neighbouring
 *                    queries of a level in the same cache lines).  Other bits: hipErrorInvalidValue.
 *   offsets_query_stride / logits_query_stride: floats from one query's block to the next (0 = dense), so
 *                    both may be column blocks of one wider GEMM output; multiples of 4
 * Only the shapes the LDS-tiled kernel takes are supported (fp32, channels 16 or 32, num_point 4,
 * num_levels <= 16, num_query == spatial_size, 16-byte aligned pointers): mvdetr_msda_fused_supported()
 * returns 1 for them, and the forward returns hipErrorNotSupported (801) otherwise. */
int mvdetr_msda_fused_supported(int batch, int spatial_size, int num_heads, int channels, int num_levels,
                                int num_query, int num_point);
int mvdetr_msda_forward_fused_f32(void *stream, const float *value, const int64_t *spatial_shapes,
                                  const int64_t *level_start_index, const float *reference_points,
                                  int64_t ref_batch_stride, const float *sampling_offsets,
                                  const float *attn_logits, int level_major, int offsets_query_stride,
                                  int logits_query_stride, int batch, int spatial_size, int num_heads,
                                  int channels, int num_levels, int num_query, int num_point, float *out);

/* 16-bit storage variant of the fused forward (inference; an addition, the ABI version above is unchanged), for the ONE form
 * MSDeformAttn calls it in (csrc/msda_forward_fused_half.hip):
 *   value  [batch, spatial_size, num_heads, channels]  16-bit words (IEEE binary16 `_f16` / bfloat16 `_bf16`)
 *   raw    [batch, Lq, >= num_heads*num_levels*12]  16-bit, the slice-interleaved tensor with the level outermost (bits 4|16
 *          above; g = 32 / channels heads per run as in the fp32 layout, so the same permuted Linear produces it);
 *          raw_query_stride elements between queries (0 = dense), a multiple of 4
 *   reference_points  [batch or 1, num_levels, Lq, 2]  FP32, one point per (query, level), level-major (bits 2|8);
 *          ref_batch_stride floats between batch elements (0 = shared)
 *   out    [batch, Lq, num_heads*channels]  16-bit
 * Softmax over the num_levels*4 logits, loc = ref + offset / (W, H) and the bilinear blend are fp32; every output element is
 * rounded once, to nearest-even.  Served: channels 16 or 32, num_point 4, num_levels <= 16 OF EQUAL SHAPE (device data: on
 * other shapes every output element is NaN), num_query == spatial_size, 16-byte aligned value / raw / out:
 * mvdetr_msda_fused_half_supported() returns 1 for such dimensions, and the forward returns hipErrorNotSupported (801) for
 * anything else.  Kernel name: "msda_fwd_fused_half". */
int mvdetr_msda_fused_half_supported(int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                     int num_point);
int mvdetr_msda_forward_fused_f16(void *stream, const uint16_t *value, const int64_t *spatial_shapes,
                                  const int64_t *level_start_index, const float *reference_points, int64_t ref_batch_stride,
                                  const uint16_t *raw, int raw_query_stride, int batch, int spatial_size, int num_heads,
                                  int channels, int num_levels, int num_point, uint16_t *out);
int mvdetr_msda_forward_fused_bf16(void *stream, const uint16_t *value, const int64_t *spatial_shapes,
                                   const int64_t *level_start_index, const float *reference_points, int64_t ref_batch_stride,
                                   const uint16_t *raw, int raw_query_stride, int batch, int spatial_size, int num_heads,
                                   int channels, int num_levels, int num_point, uint16_t *out);

/* The same with the queries restricted to the tokens of levels [query_level_begin, query_level_end): the
 * encoder call of ONE rank of a query-sharded run (cameras = levels partitioned over GPUs; SURVEY 8e option
 * B -- not in the reference, which is single-device).  `value` still holds all spatial_size tokens;
 * reference_points, sampling_offsets, attn_logits and out hold only the num_query =
 * sum_{l in range} H_l*W_l queries of the range, in token order.  (0, num_levels) is the call above. */
int mvdetr_msda_fused_levels_supported(int batch, int spatial_size, int num_heads, int channels, int num_levels,
                                       int num_query, int num_point, int query_level_begin, int query_level_end);
int mvdetr_msda_forward_fused_levels_f32(void *stream, const float *value, const int64_t *spatial_shapes,
                                         const int64_t *level_start_index, const float *reference_points,
                                         int64_t ref_batch_stride, const float *sampling_offsets,
                                         const float *attn_logits, int level_major, int offsets_query_stride,
                                         int logits_query_stride, int query_level_begin, int query_level_end,
                                         int batch, int spatial_size, int num_heads, int channels, int num_levels,
                                         int num_query, int num_point, float *out);

/* ---- Multi-scale deformable attention, backward -----------------------------------------------
 * Replaces ms_deformable_col2im_cuda (ms_deform_im2col_cuda.cuh:956-1327) and its six kernel
 * variants (cuh:301-920, device helpers cuh:87-234).
 *   grad_col          [batch, num_query, num_heads*channels]   upstream gradient
 *   grad_value        same shape as value; MUST BE ZERO on entry (accumulated with atomics,
 *                     like the reference: ms_deform_attn_cuda.cu:121)
 *   grad_sampling_loc same shape as sampling_loc; fully written
 *   grad_attn_weight  same shape as attn_weight; fully written
 */
int mvdetr_msda_backward_f32(void *stream, const float *grad_col, const float *value,
                             const int64_t *spatial_shapes, const int64_t *level_start_index,
                             const float *sampling_loc, const float *attn_weight, int batch,
                             int spatial_size, int num_heads, int channels, int num_levels,
                             int num_query, int num_point, float *grad_value,
                             float *grad_sampling_loc, float *grad_attn_weight);
int mvdetr_msda_backward_f64(void *stream, const double *grad_col, const double *value,
                             const int64_t *spatial_shapes, const int64_t *level_start_index,
                             const double *sampling_loc, const double *attn_weight, int batch,
                             int spatial_size, int num_heads, int channels, int num_levels,
                             int num_query, int num_point, double *grad_value,
                             double *grad_sampling_loc, double *grad_attn_weight);

/* ---- Fused TRAINING pair (ABI 10): MSDeformAttn.forward / backward with the module arithmetic inside the kernels --------
 * What the reference runs when gradients are needed -- softmax and location arithmetic in torch (ms_deform_attn.py:100-107),
 * the extension's forward / backward on the materialised sampling_locations (135 MB at Wildtrack size) and
 * attention_weights (68 MB) (func.py:21-38, cuh:237-299, 956-1327), and torch's backward of that arithmetic -- as two calls
 * on the module's RAW Linear outputs:
 *   raw   [batch, Lq, >= M*L*P*3]  one tensor, per query [L][M/g][g*P*2 offsets | g*P logits], g = 32 / channels heads per
 *         128-byte slice (the layout MultiScaleDeformableAttention.slice_major_rows(level_outer=True) gives the GEMM);
 *         raw_query_stride floats between queries
 *   reference_points [batch or 1, L, Lq, 2]  ONE point per (query, level), level-major (MVDeTr's map; ref_batch_stride 0 when
 *         shared by the batch)
 * Shapes: queries = tokens (Lq = spatial_size), up to 16 levels OF EQUAL SHAPE (the caller's promise: on other shapes the
 * outputs are NaN), 4 points, 16- or 32-channel heads (an even number of 16-channel heads); mvdetr_msda_fused_train_supported
 * says whether a call qualifies (1 / 0).  ABI 10 - 12 took 6 / 7 levels of 16-channel heads only (MVDeTr's own shapes: their
 * kernels are msda_fwd_group2, msda_bwd_onepass and msda_bwd_fused_sampling); since ABI 13 every other encoder shape runs the
 * inference forward of that shape + a statistics pass, and the one-pass backward (16 channels) or msda_bwd_value_tok + the
 * level-groups sampling kernel (32 channels; not in the deterministic mode).
 * forward: out [batch, Lq, M*D] as mvdetr_msda_forward_fused_f32, plus stats [batch, Lq, M, 2] = (maximum logit,
 *          1 / sum of exp(logit - maximum)) of every (query, head), which the backward needs to rebuild the weights.
 * backward: grad_value [batch, S, M, D] (ACCUMULATED: zero it first) and grad_raw [batch, Lq, raw_query_stride] (the
 *          M*L*P*3 leading columns of every query are written, in raw's layout) from grad_output, the same inputs, stats and
 *          the forward's out (softmax backward: d logit = a (d a - <grad_output, out>)).
 * Return 0, hipErrorNotSupported (801) for shapes / alignments outside the above, another hipError_t on failure. */
int mvdetr_msda_fused_train_supported(int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                      int num_point);
int mvdetr_msda_forward_fused_train_f32(void *stream, const float *value, const int64_t *spatial_shapes,
                                        const int64_t *level_start_index, const float *reference_points,
                                        int64_t ref_batch_stride, const float *raw, int raw_query_stride, int batch,
                                        int spatial_size, int num_heads, int channels, int num_levels, int num_point,
                                        float *out, float *stats);
int mvdetr_msda_backward_fused_f32(void *stream, const float *grad_output, const float *value,
                                   const int64_t *spatial_shapes, const int64_t *level_start_index,
                                   const float *reference_points, int64_t ref_batch_stride, const float *raw,
                                   int raw_query_stride, const float *stats, const float *out, int batch, int spatial_size,
                                   int num_heads, int channels, int num_levels, int num_point, float *grad_value,
                                   float *grad_raw);

/* ---- Feature -> ground-plane homography warp ---------------------------------------------------
 * Replaces the third-party call kornia.warp_perspective(src, M, dsize, mode='bilinear',
 * padding_mode='zeros', align_corners=False) at multiview_detector/models/mvdetr.py:194-195
 * (kornia: normalize_homography -> inverse -> transform_points(meshgrid) -> F.grid_sample),
 * fused into one kernel.
 *   src  [n, channels, src_h, src_w]        (NCHW, like the reference's imgs_feat)
 *   M    [n, 3, 3]  destination pixel <- source pixel homography, same dtype as src
 *   dst  [n, channels, dst_h, dst_w]        every element is written (zeros outside the view)
 * `layout_nhwc` is a bit mask (bit 2, value 4: mode='nearest' instead of bilinear -- frameDataset.py:80).  Bit 0 (value 1): dst is written as [n, dst_h, dst_w, channels] instead (the
 * token layout the shadow transformer consumes, trans_world_feat.py:92), saving the permute copy.  Bit 1
 * (value 2): src is [n, src_h, src_w, channels] -- what a channels_last trunk produces -- so every bilinear
 * corner is one contiguous channel vector; supported together with bit 0 (value 3), channels a multiple of
 * 16 bytes, 16-byte aligned pointers; hipErrorNotSupported (801) otherwise.  Other bits: hipErrorInvalidValue.
 * Which kernel every warp entry below runs, what it refuses with which code and what it accepts without a launch is ONE table,
 * warp_route() of csrc/warp_route.h (plain C++; tests/test_warp_route.py prints it on the CPU, tests/test_warp_refusals_gpu.py
 * checks the codes on the library).  The entries are in csrc/warp_perspective.hip, the kernels and their launchers in
 * csrc/warp_forward.hip and csrc/warp_backward.hip.
 */
int mvdetr_warp_perspective_forward_f32(void *stream, const float *src, const float *M, int n,
                                        int channels, int src_h, int src_w, int dst_h, int dst_w,
                                        int layout_nhwc, float *dst);
int mvdetr_warp_perspective_forward_f64(void *stream, const double *src, const double *M, int n,
                                        int channels, int src_h, int src_w, int dst_h, int dst_w,
                                        int layout_nhwc, double *dst);

/* 16-bit storage variants of the forward (inference; an addition, the ABI version above is unchanged): src and dst are IEEE
 * binary16 (`_f16`) / bfloat16 (`_bf16`) words, M stays FP32; the source position is computed in fp64 exactly as above, the
 * blend weights and the blend are fp32, and every output element is rounded once, to nearest-even.  All four layout
 * combinations and bit 2 (nearest) are taken: channel-last on both sides with channels % 8 == 0 and 16-byte aligned tensors
 * runs "warp_fwd_cl_half" (8 channels per lane), everything else "warp_fwd_half" (2-byte accesses).  No backward, no host
 * entry. */
int mvdetr_warp_perspective_forward_f16(void *stream, const uint16_t *src, const float *M, int n, int channels, int src_h,
                                        int src_w, int dst_h, int dst_w, int layout_nhwc, uint16_t *dst);
int mvdetr_warp_perspective_forward_bf16(void *stream, const uint16_t *src, const float *M, int n, int channels, int src_h,
                                         int src_w, int dst_h, int dst_w, int layout_nhwc, uint16_t *dst);

/* Gradient of the warp w.r.t. src (what autograd reaches through grid_sample in the reference).
 *   grad_dst [n, channels, dst_h, dst_w] (or NHWC if layout_nhwc bit 0)
 *   grad_src [n, channels, src_h, src_w] (or NHWC if layout_nhwc bit 1, same restrictions as the forward);
 *            OVERWRITTEN: every element is stored, it need not be zeroed (ABI 9; up to ABI 8 it had to be zero on entry)
 * With both sides channel-last (layout_nhwc & 3 == 3) the gradient is computed as a GATHER over the destination pixels
 * whose bilinear footprint touches each source texel (the homography is invertible): no atomics, the order of every
 * sum is fixed, so the result is deterministic -- unlike grid_sample's atomicAdd backward.  It uses
 * stream-ordered scratch (80 bytes per 2x2 block of source texels + 4 bytes per destination pixel, hipMallocAsync on
 * `stream`), kept per (device, stream) between calls and grown on demand.
 * The other layouts scatter with fp atomics after a hipMemsetAsync (MVDETR_WARP_BWD_IMPL=scatter forces that for
 * channel-last tensors too).
 */
int mvdetr_warp_perspective_backward_f32(void *stream, const float *grad_dst, const float *M, int n,
                                         int channels, int src_h, int src_w, int dst_h, int dst_w,
                                         int layout_nhwc, float *grad_src);
int mvdetr_warp_perspective_backward_f64(void *stream, const double *grad_dst, const double *M,
                                         int n, int channels, int src_h, int src_w, int dst_h,
                                         int dst_w, int layout_nhwc, double *grad_src);

/* The one-call gradient with a caller-supplied VERSION TAG of the matrices (ABI 12): `matrices_tag` != 0 is the caller's
 * promise that calls with the same tag -- on this device and stream, with the same shapes -- pass the same M.  The library
 * keeps the gather's geometry (see below) in its per-(device, stream) scratch together with the tag, so the second and later
 * calls of a training loop without augmentation launch the gather alone: what mvdetr_warp_perspective_backward_* would do if
 * it could compare M on the host (it cannot: M is a device pointer, and comparing it on the device would cost every call a
 * dependent launch).  Tag 0 = unknown: identical to mvdetr_warp_perspective_backward_*.  A new tag (or an untagged call on
 * the stream in between) rebuilds the geometry.  Replaces kornia.warp_perspective's backward at mvdetr.py:194-195. */
int mvdetr_warp_perspective_backward_tagged_f32(void *stream, const float *grad_dst, const float *M, int n, int channels,
                                                int src_h, int src_w, int dst_h, int dst_w, int layout_nhwc,
                                                uint64_t matrices_tag, float *grad_src);
int mvdetr_warp_perspective_backward_tagged_f64(void *stream, const double *grad_dst, const double *M, int n, int channels,
                                                int src_h, int src_w, int dst_h, int dst_w, int layout_nhwc,
                                                uint64_t matrices_tag, double *grad_src);

/* The same gradient in two steps, for callers whose matrices stay the same from call to call (training without
 * augmentation: the projection matrices are constants, mvdetr.py:82-95,155-161).  The gather's geometry -- which destination
 * pixels can touch each 2x2 block of source texels -- depends on M and the shapes only:
 *   mvdetr_warp_backward_plan_bytes   size of the plan of such a call in bytes, 0 when the gather does not take the shapes
 *                                     (channels * elem_size not a multiple of 16, more than 2^31 elements, or
 *                                     MVDETR_WARP_BWD_IMPL=scatter): use mvdetr_warp_perspective_backward_* then
 *   mvdetr_warp_backward_plan_*       fills `plan` (caller-owned device memory of that size, 16-byte aligned) for M [n,3,3]
 *   mvdetr_warp_perspective_backward_planned_*   the gradient from a plan built for the same M and shapes; the plan is only
 *                                     read (any number of calls, any streams ordered after the plan's); layouts: channel-last
 *                                     on both sides (layout_nhwc bits 0 and 1 set; bit 2 = nearest), 16-byte aligned tensors
 * One kernel per call instead of two and a stream write, no library-side scratch.  Results are bit-identical to
 * mvdetr_warp_perspective_backward_* (the same kernels). */
int64_t mvdetr_warp_backward_plan_bytes(int n, int channels, int src_h, int src_w, int dst_h, int dst_w, int elem_size);
int mvdetr_warp_backward_plan_f32(void *stream, const float *M, int n, int channels, int src_h, int src_w, int dst_h, int dst_w,
                                  void *plan);
int mvdetr_warp_backward_plan_f64(void *stream, const double *M, int n, int channels, int src_h, int src_w, int dst_h, int dst_w,
                                  void *plan);
int mvdetr_warp_perspective_backward_planned_f32(void *stream, const float *grad_dst, const float *M, const void *plan, int n,
                                                 int channels, int src_h, int src_w, int dst_h, int dst_w, int layout_nhwc,
                                                 float *grad_src);
int mvdetr_warp_perspective_backward_planned_f64(void *stream, const double *grad_dst, const double *M, const void *plan, int n,
                                                 int channels, int src_h, int src_w, int dst_h, int dst_w, int layout_nhwc,
                                                 double *grad_src);

/* ---- Residual add + LayerNorm (the tail of both halves of the shadow transformer's encoder layer) -------
 * Replaces  self.norm1(src + self.dropout1(src2))  /  self.norm2(src + self.dropout3(ffn))  in eval mode
 * (multiview_detector/models/deformable_transformer.py:96-100; torch.nn.LayerNorm over the last dimension,
 * biased variance, eps inside the square root) by one pass:
 *     out[r, :] = LayerNorm(x[r, :] + residual[r, :]) * weight + bias
 *   x, residual, out [rows, cols] fp32, contiguous (residual may be NULL; out must not overlap the inputs)
 *   weight, bias     [cols]  (both NULL: no affine)
 * cols must be 64, 128 or 256 with (cols/64)*4-byte aligned pointers: hipErrorNotSupported (801) otherwise. */
int mvdetr_add_layernorm_f32(void *stream, const float *x, const float *residual, const float *weight,
                             const float *bias, int64_t rows, int cols, float eps, float *out);
/* The same with a second output  out2[r, :] = out[r, :] + add2[r % add2_rows, :]  -- the next encoder layer's query
 * `src + pos` (deformable_transformer.py:92, with_pos_embed), so that add is not a pass of its own.  add2
 * [add2_rows, cols] (the position embedding, shared by the batch); add2 and out2 are given together. */
int mvdetr_add_layernorm_add_f32(void *stream, const float *x, const float *residual, const float *weight,
                                 const float *bias, const float *add2, int64_t add2_rows, int64_t rows, int cols,
                                 float eps, float *out, float *out2);

/* 16-bit storage variants (inference; an addition, the ABI version above is unchanged): x, residual, weight, bias, add2, out
 * and out2 are IEEE binary16 (`_f16`) / bfloat16 (`_bf16`) words.  The sum x + residual, its mean and variance and the
 * normalised row are fp32; out is rounded once, and out2 is formed from the UNROUNDED row plus add2 and rounded once.  The same
 * cols set; pointers aligned to (cols/64)*2 bytes (16-byte aligned tensors take 16-byte accesses): 801 otherwise. */
int mvdetr_add_layernorm_add_f16(void *stream, const uint16_t *x, const uint16_t *residual, const uint16_t *weight,
                                 const uint16_t *bias, const uint16_t *add2, int64_t add2_rows, int64_t rows, int cols,
                                 float eps, uint16_t *out, uint16_t *out2);
int mvdetr_add_layernorm_add_bf16(void *stream, const uint16_t *x, const uint16_t *residual, const uint16_t *weight,
                                  const uint16_t *bias, const uint16_t *add2, int64_t add2_rows, int64_t rows, int cols,
                                  float eps, uint16_t *out, uint16_t *out2);
/* Name of the kernel the last add + LayerNorm call of this process launched: the kernels' own names,
 * "add_layernorm_rows128x2" (128 columns, every pointer 16-byte aligned), "add_layernorm_rows<1>" / "<2>" / "<4>" (64 / 128 / 256
 * columns, one row per wave), "add_layernorm_rows_half<COLS,VEC>" (VEC = 8: 16-byte aligned; VEC = COLS / 64 otherwise);
 * "none" before the first launch.  A refused call (801, 1) leaves it unchanged.  Host-side static storage; never NULL. */
const char *mvdetr_add_layernorm_last_kernel(void);

/* ---- The ResNet trunk's inference epilogues (csrc/trunk_epilogue.hip) ---------------------------
 * Eval-mode BatchNorm2d with what follows it in a residual block, one pass over channel-last fp32 activations:
 *     y[r, c] = act( x[r, c]*s[c] + t[c]  [+ res[r, c]]  [+ res[r, c]*s2[c] + t2[c]] )
 *     s = gamma / sqrt(var + eps),  t = beta - mean*s     (formed in the kernel on every call; gamma / beta NULL: 1 / 0)
 *   x, res, y   [rows, channels] fp32, 16-byte aligned (NHWC memory: rows = N*H*W); y may be x (in place), res may not be y
 *   res         NULL: no residual.  With every res_* NULL it is added as is (the identity branch); with res_mean / res_var
 *               (and optionally res_gamma / res_beta) it goes through its own BatchNorm first (the downsample branch)
 *   relu        non-zero: act = ReLU with torch's NaN rule (relu(NaN) = NaN); zero: none
 * channels must be a multiple of 4.  hipErrorInvalidValue (1) for anything else that does not fit. */
int mvdetr_bn_act_f32(void *stream, const float *x, const float *mean, const float *var, const float *gamma,
                      const float *beta, float eps, const float *res, const float *res_mean, const float *res_var,
                      const float *res_gamma, const float *res_beta, float res_eps, int64_t rows, int channels, int relu,
                      float *y);
/* The stem: MaxPool2d(kernel 3, stride 2, padding 1) over relu(BatchNorm(x)) in one pass.
 *   x [n, h, w, channels], y [n, (h-1)/2+1, (w-1)/2+1, channels] fp32 NHWC, 16-byte aligned, not overlapping
 * Padding counts as -inf and a NaN in the window gives NaN, as in torch.  channels/4 must divide 256 or be a multiple of
 * it (64, 128, ..., 1024, 2048, ...): hipErrorNotSupported (801) otherwise. */
int mvdetr_bn_relu_maxpool_f32(void *stream, const float *x, const float *mean, const float *var, const float *gamma,
                               const float *beta, float eps, int n, int h, int w, int channels, float *y);
/* The same two passes over 16-bit activations (float16 / bfloat16 as raw uint16_t words, channel-last): x, res and y
 * are 16-bit, the BatchNorm vectors stay fp32 (MVDeTr.to_inference keeps them so).  Every step is fp32 -- the sum
 * bn(x) + identity is not rounded in between, the pool takes its max on fp32 values -- and the result is rounded once,
 * to nearest-even, on the way out.  A lane owns eight channels (one 16-byte access): channels must be a multiple of 8
 * (hipErrorInvalidValue otherwise), and the pool wants channels/8 to divide 256 or be a multiple of it
 * (hipErrorNotSupported otherwise).  Everything else -- arguments, aliasing (y may be x, res never y), validation --
 * as the _f32 entries above. */
int mvdetr_bn_act_f16(void *stream, const uint16_t *x, const float *mean, const float *var, const float *gamma,
                      const float *beta, float eps, const uint16_t *res, const float *res_mean, const float *res_var,
                      const float *res_gamma, const float *res_beta, float res_eps, int64_t rows, int channels, int relu,
                      uint16_t *y);
int mvdetr_bn_act_bf16(void *stream, const uint16_t *x, const float *mean, const float *var, const float *gamma,
                       const float *beta, float eps, const uint16_t *res, const float *res_mean, const float *res_var,
                       const float *res_gamma, const float *res_beta, float res_eps, int64_t rows, int channels, int relu,
                       uint16_t *y);
int mvdetr_bn_relu_maxpool_f16(void *stream, const uint16_t *x, const float *mean, const float *var, const float *gamma,
                               const float *beta, float eps, int n, int h, int w, int channels, uint16_t *y);
int mvdetr_bn_relu_maxpool_bf16(void *stream, const uint16_t *x, const float *mean, const float *var, const float *gamma,
                                const float *beta, float eps, int n, int h, int w, int channels, uint16_t *y);
/* Name of the kernel the last trunk-epilogue call of this process launched ("bn_relu", "bn_add_relu", "bn_bn_add_relu",
 * "bn_relu_maxpool", ...; the 16-bit entries: the same names with "_half" appended; "none" before the first), and how
 * many such launches there have been: tests tell the fused path from torch's ops by them.  Static storage; never NULL. */
const char *mvdetr_trunk_last_kernel(void);
int64_t mvdetr_trunk_launch_count(void);

/* ---- Winograd F(2x2, 3x3) convolution in fp32 (csrc/conv_winograd.hip; additive entries) -----------------------
 * A 3x3 convolution with stride 1, padding = dilation, groups 1 and no bias over channel-last fp32 activations, as
 *     Y = A^T [ sum_c (G g G^T) .* (B^T d B) ] A     per 2x2 output tile
 * with the sixteen products over the input channels on the fp32 MFMA (2.25x fewer multiplications than the direct
 * form; fp32 inputs, products and sums throughout).  Two steps:
 *   mvdetr_winograd_weights_f32   w [K, C, 3, 3] dense (OIHW) -> U [16, C, K]: G g G^T formed in fp64 and rounded once.
 *                                 Runs once per weight tensor (C * K threads).
 *   mvdetr_conv3x3_winograd_f32   x [N, H, W, C] -> y [N, H, W, K] (NHWC memory, y fresh: it may not be x), one launch;
 *                                 x and U are only read, every element of y is written once, nothing outside it; no
 *                                 atomics: bit-reproducible.  A dilation d runs as d * d undilated convolutions on the
 *                                 pixel sub-lattices (y mod d, x mod d), in place.
 * Contract: C % 8 == 0, K % 64 == 0, dilation 1, 2 or 4, 16-byte aligned x, U, y, (256 + 2 H W) max(C, K) < 2^30,
 * fewer than 2^31 tiles: hipErrorNotSupported (801) otherwise, hipErrorInvalidValue for null pointers / sizes <= 0.
 * Kernel names: "winograd_weights_f32", "conv3x3_winograd_f32". */
int mvdetr_winograd_weights_f32(const float *w, int C, int K, float *U, void *stream);
int mvdetr_conv3x3_winograd_f32(const float *x, const float *U, float *y, int N, int H, int W, int C, int K, int dilation,
                                void *stream);
/* The same convolution with the block's inference epilogue applied in the output store (additive entry):
 *     y = act( conv(x)*s + t  [+ res]  [+ res*s2 + t2] )
 * with s, t, s2, t2, act and the BatchNorm / residual arguments exactly as in mvdetr_bn_act_f32, in its argument order and
 * its arithmetic, element for element: the result has the bits of mvdetr_conv3x3_winograd_f32 followed by mvdetr_bn_act_f32
 * in place, without the pass over y.  The BatchNorm vectors are [K] (4-byte aligned here: a lane reads one channel);
 * res [N, H, W, K] is y's geometry, 16-byte aligned, only read, and only where y is stored.
 * Refusals: those of mvdetr_conv3x3_winograd_f32; hipErrorInvalidValue for a missing mean / var, for a residual BatchNorm
 * without a residual, and for a residual whose byte range overlaps y's. */
int mvdetr_conv3x3_winograd_bn_act_f32(const float *x, const float *U, float *y, int N, int H, int W, int C, int K,
                                       int dilation, const float *mean, const float *var, const float *gamma,
                                       const float *beta, float eps, const float *res, const float *res_mean,
                                       const float *res_var, const float *res_gamma, const float *res_beta, float res_eps,
                                       int relu, void *stream);
/* Name of the kernel the last call of the three above launched ("none" before the first) and their launch count: one per
 * call; the convolution's name is "conv3x3_winograd_f32" whatever its store applies. */
const char *mvdetr_winograd_last_kernel(void);
/* What the last convolution's store applied: "none", "bn", "bn_add" or "bn_bn_add", with "_relu" appended under ReLU
 * (mvdetr_trunk_last_kernel's names). */
const char *mvdetr_winograd_last_epilogue(void);
int64_t mvdetr_winograd_launch_count(void);
/* The convolution's grid is persistent: min(units, CUs) workgroups, each running every G-th unit of 64 tiles x 64 output
 * channels.  This caps it at n workgroups for the whole process (0: no cap, the default) and returns the previous cap
 * (additive entry).  For tests, so that small shapes run many units per workgroup; results do not depend on it. */
int mvdetr_winograd_set_max_workgroups(int n);
/* The last round's tail (additive entries, the ABI version above is unchanged).  A unit is indivisible, so with G workgroups,
 * R = units / G and rem = units % G > 0, the last round keeps rem CUs busy for a whole unit time.  Where rem <= G / 2 the
 * persistent kernel runs the units [0, R G) and a second launch, "conv3x3_winograd_w16_f32", runs the rest as 2 rem HALF
 * units of 32 tiles x 64 channels (v_mfma_f32_16x16x4_f32, the same order of channels: the same bits).  One convolution
 * call stays one count of mvdetr_winograd_launch_count and its name stays "conv3x3_winograd_f32".
 *   mvdetr_winograd_set_tail         0: never; 1: the default -- where rem <= G / 2, on the (C, K, dilation) on which it
 *                                    measured faster; 2: whenever rem > 0, on every shape (tests).  Returns the previous mode.
 *   mvdetr_winograd_last_tail_units  the units the last convolution call ran as half units (0: no second launch)
 *   mvdetr_winograd_plan             without a device: out[6] = {units, G, R, rem, half units, variant} of a call on
 *                                    `workgroups` CUs under the current cap, tail mode and variant; the refusals of
 *                                    mvdetr_conv3x3_winograd_f32's shapes
 * The persistent kernel has two forms with the same units, order of channels and bits: 1, "conv3x3_winograd_f32" proper (4 waves,
 * 32 tiles x 32 channels per wave on v_mfma_f32_32x32x2_f32, one wave per SIMD), and 2, "conv3x3_winograd_w16x2_f32" (8 waves,
 * 32 tiles x 16 channels per wave on v_mfma_f32_16x16x4_f32, two waves per SIMD).
 *   mvdetr_winograd_set_variant      0: the default -- 2 on the (C, K, dilation) on which it measured faster, 1 elsewhere;
 *                                    1 or 2: that one on every shape (tests, A/B).  Returns the previous setting.
 *   mvdetr_winograd_last_variant     the form the last convolution call ran (0 before the first) */
int mvdetr_winograd_set_variant(int variant);
int mvdetr_winograd_last_variant(void);
int mvdetr_winograd_set_tail(int mode);
int mvdetr_winograd_last_tail_units(void);
int mvdetr_winograd_plan(int N, int H, int W, int C, int K, int dilation, int workgroups, int64_t *out);
/* How form 2 deals a chunk's memory work to the two waves of a SIMD (additive entries, the ABI version above is unchanged;
 * the plan's six fields do not depend on it).  Schedule 1, lockstep: all eight waves run one program, so both waves of a SIMD
 * issue their loads in the same half k-step.  Schedule 2, de-phased: waves 4-7 run a program of their own with the same
 * arithmetic, barrier and LDS layout, whose loads and input transform sit in other half k-steps.  The same bits.
 *   mvdetr_winograd_set_schedule     0: the default -- 2 on the (C, K, dilation) on which it measured faster, 1 elsewhere;
 *                                    1 or 2: that one on every shape (tests, A/B); anything else is 0.  Returns the previous
 *                                    setting.
 *   mvdetr_winograd_last_schedule    the schedule of the last convolution call (0 before the first; 1 where it ran form 1)
 *   mvdetr_winograd_schedule_of      what a form 2 launch of this (C, K, dilation) takes under the current setting: 1 or 2 */
int mvdetr_winograd_set_schedule(int schedule);
int mvdetr_winograd_last_schedule(void);
int mvdetr_winograd_schedule_of(int C, int K, int dilation);

/* ---- The backward of that convolution (csrc/conv_winograd_backward.hip; additive entries, the ABI version above is unchanged)
 * Data gradient: for stride 1 and padding = dilation it is the same convolution of grad_y [N, H, W, K] with the weights
 * flipped in both spatial axes and transposed in (C, K), so it needs one weight transform and no kernel of its own:
 *   mvdetr_winograd_weights_dgrad_f32   w [K, C, 3, 3] dense -> Ut [16, K, C]: G g' G^T of g'[i][j] = w[k][c][2 - i][2 - j],
 *                                       formed in fp64 and rounded once as mvdetr_winograd_weights_f32 does.  Feed it to
 *                                       mvdetr_conv3x3_winograd_f32(grad_y, Ut, grad_x, N, H, W, K, C, ...), C and K
 *                                       exchanged: C % 64 == 0 and K % 8 == 0 here.  Kernel name "winograd_weights_dgrad_f32".
 * Weight gradient, in the Winograd domain: dU[p][c][k] = sum over the 2x2 tiles of (B^T d B)[p][tile][c] (A dY A^T)[p][tile][k],
 * gw = G^T dU G -- sixteen GEMMs reduced over the forward's tile grid on v_mfma_f32_32x32x2_f32, 16 multiplications per
 * (tile, c, k) against 36 of the direct form:
 *   mvdetr_conv3x3_winograd_wgrad_f32   x [N, H, W, C], gy [N, H, W, K] (NHWC memory, only read) -> gw [K, C, 3, 3] dense,
 *                                       every element written, nothing outside it.  A unit is a 64 x 64 block of (k, c); its
 *                                       tiles are split over S workgroups, each with a contiguous range of chunks of 8 tiles,
 *                                       whose partial gw go to slice s of `workspace` ([S, K, C, 3, 3] floats), and a second
 *                                       small kernel sums the S slices in index order.  No atomics: for a given S the result
 *                                       is bit-identical from call to call.  The library allocates nothing:
 *   mvdetr_winograd_wgrad_workspace_bytes  what `workspace` must hold for a call on a device of `workgroups` CUs under the
 *                                       current settings (-1 for a shape the call refuses)
 *   mvdetr_winograd_wgrad_plan          without a device: out[5] = {units, chunks, S, chunks per split, chunks of the last
 *                                       split}.  The default S is CUs / units (one workgroup per CU, which is what fits),
 *                                       at least 1 and at most the chunks; mvdetr_winograd_set_max_workgroups caps the CUs
 *                                       counted and the grid (the items (unit, split) then go round-robin).
 *   mvdetr_winograd_set_wgrad_splits    force S (0: the default; clamped to the chunks); returns the previous setting.  Tests.
 *   mvdetr_winograd_last_wgrad_splits   the S of the last weight-gradient call
 * Contract of the weight gradient: C % 64 == 0, K % 64 == 0, dilation 1, 2 or 4, 16-byte aligned x, gy, gw, workspace, the
 * forward's bounds ((256 + 2 H W) max(C, K) < 2^30, C K < 2^26, fewer than 2^31 tiles) and workspace_bytes at least what
 * mvdetr_winograd_wgrad_workspace_bytes says: hipErrorNotSupported (801) otherwise; hipErrorInvalidValue for null x, gy, gw,
 * sizes <= 0, and a gw or workspace whose bytes overlap an input's (or each other's).  N == 0 writes zeros to gw.
 * One call is one count of mvdetr_winograd_launch_count, the reduce kernel included; its name is "conv3x3_winograd_wgrad_f32". */
int mvdetr_winograd_weights_dgrad_f32(const float *w, int C, int K, float *Ut, void *stream);
int mvdetr_conv3x3_winograd_wgrad_f32(const float *x, const float *gy, float *gw, int N, int H, int W, int C, int K, int dilation,
                                      void *workspace, int64_t workspace_bytes, void *stream);
int64_t mvdetr_winograd_wgrad_workspace_bytes(int N, int H, int W, int C, int K, int dilation, int workgroups);
int mvdetr_winograd_wgrad_plan(int N, int H, int W, int C, int K, int dilation, int workgroups, int64_t *out);
int mvdetr_winograd_set_wgrad_splits(int n);
int mvdetr_winograd_last_wgrad_splits(void);

/* ---- Introspection (used by bench.py / tests, not by the model code) ---------------------------
 * Name of the kernel variant the last forward call ON THIS THREAD dispatched to
 * ("gather", "tile16", ...).  Static storage; never NULL. */
const char *mvdetr_msda_last_forward_impl(void);
/* Name of the kernel that call launched ("msda_fwd_group[LDS-DMA windows]", "msda_fwd_tile", "msda_fwd_gather", ...). */
const char *mvdetr_msda_last_forward_kernel(void);
/* Name of the route the last MSDA backward ON THIS THREAD took through either entry ("twopass", "split", "onepass", "atomic",
 * "deterministic", "fused-split", "fused-twopass", "fused-onepass", "fused-groups", "fused-deterministic"; "none" before the
 * first).  An empty or refused call leaves it as it was.  Static storage; never NULL. */
const char *mvdetr_msda_last_backward_route(void);

/* What the code object records for that kernel instantiation (hipFuncGetAttributes): registers per lane, scratch bytes per
 * lane (non-zero = the instantiation spills), static LDS bytes.  Returns 0 (and -1 in the outputs) when unknown. */
int mvdetr_msda_last_forward_resources(int *num_regs, int *scratch_bytes_per_lane, int *static_lds_bytes);

/* Name of the kernel the last warp call of this process launched (any thread: autograd runs backwards on its own) ("warp_fwd_cl", "warp_fwd<NCHW>", "warp_bwd_gather",
 * ...): one name per layout route, asserted by tests/test_warp_gpu.py.  Static storage; never NULL. */
const char *mvdetr_warp_last_kernel(void);

/* The warp gradient's one-call form keeps its geometry scratch per (device, stream) between calls (hipMallocAsync on the
 * call's stream, grown on demand).  This drops every cached buffer -- e.g. after destroying streams, or to hand the memory
 * back; call it when no warp backward is in flight.  Not usable under HIP graph capture: capture the two-step form
 * (mvdetr_warp_backward_plan_* + mvdetr_warp_perspective_backward_planned_*) with a caller-owned plan buffer instead. */
int mvdetr_warp_release_scratch(void);

/* Forward kernel variant selection: 0 = auto (default; tiled LDS kernel where it applies, else
 * the gather kernel), 1 = always gather, 2 = tile whenever the shape supports it.  Results are
 * identical up to fp32 summation order; this is a tuning/testing knob.  Returns the previous value.
 * Initial value comes from MVDETR_MSDA_FWD_IMPL = auto | gather | tile. */
int mvdetr_msda_set_forward_impl(int impl);

/* Deterministic backward (opt-in; ABI 13).  The reference's col2im adds grad_value with atomicAdd
 * (ms_deform_im2col_cuda.cuh:125-152) and is not reproducible run to run; neither are this library's default backward
 * kernels (fp32 atomics when LDS windows are flushed).  With on != 0, mvdetr_msda_backward_f32 and
 * mvdetr_msda_backward_fused_f32 sum grad_value in 64-bit fixed point with one binary point per call -- 38 bits below
 * max|grad_out| x max(1, max|attn_weight|) -- so the result is bit-identical run to run (grad_sampling_loc / grad_attn_weight have
 * one writer per element in every mode).  Costs a scratch of 8 bytes per value element, kept per (device, stream) between calls (mvdetr_msda_release_scratch), and three small launches.
 * Only deformable-encoder calls are served (fp32, 16-channel heads, equal level shapes, num_query == spatial_size,
 * spatial_size * num_levels * num_point < 2^24); every other call returns hipErrorNotSupported (801) while the mode is on, and
 * unequal level shapes (device data) fill grad_value with NaN.  Returns the previous state; the initial state comes from
 * MVDETR_MSDA_BWD_DETERMINISTIC=1. */
int mvdetr_msda_set_backward_deterministic(int on);
/* The mode's current state (1 = on), without changing it (ABI 14: a caller that only wants to KNOW -- MSDeformAttn.forward
 * refusing a training call the mode cannot serve -- must not toggle a process-wide switch other threads' backwards read). */
int mvdetr_msda_get_backward_deterministic(void);

/* The deterministic mode keeps its 64-bit accumulators (8 bytes per value element) per (device, stream) between calls
 * (hipMallocAsync on the call's stream, grown on demand).  This drops every cached buffer; call it when no backward is in flight.
 * Not usable under HIP graph capture. */
int mvdetr_msda_release_scratch(void);

/* dst[n][c][r] = src[n][r][c]: layout change between NCHW (rows = channels, cols = h*w) and the channel-last layout the
 * fast warp kernels read, and back.  Tiled through LDS, both sides move in 256-byte runs. */
int mvdetr_transpose_f32(void *stream, const float *src, int n, int rows, int cols, float *dst);
int mvdetr_transpose_f64(void *stream, const double *src, int n, int rows, int cols, double *dst);

/* ---- Deformable convolution (ABI 15) ------------------------------------------------------------------------------
 * torchvision.ops.deform_conv2d v1 (no modulation mask, weight groups 1) -- the DeformConv2d of the reference's
 * DeformConvWorldFeat (conv_world_feat.py:55-76).
 *   input  [batch, in_channels, in_h, in_w]: NCHW, or channel-last memory ([batch, in_h, in_w, in_channels]) when
 *          input_nhwc != 0; grad_input has the same layout
 *   offset [batch, 2 * offset_groups * kernel_h * kernel_w, out_h, out_w]; channel 2 (g kh kw + i kw + j) is dy of group g,
 *          tap (i, j), the next one dx; group g owns in_channels / offset_groups input channels
 *   weight [out_channels, in_channels, kernel_h, kernel_w], bias [out_channels] or NULL; out [batch, out_channels, out_h, out_w]
 *   out_h = (in_h + 2 pad_h - dil_h (kernel_h - 1) - 1) / stride_h + 1 (out_w likewise): F.conv2d's output size
 * Sample of tap (i, j): bilinear at y = h stride_h - pad_h + i dil_h + dy, x likewise, in pixel units (no -0.5 shift); 0
 * when y <= -1, y >= in_h, x <= -1 or x >= in_w; corners outside the image contribute 0.
 * Backward: grad_input is ACCUMULATED into (pass it zeroed); grad_offset and grad_weight are written.  The offset gradient
 * is the derivative of the bilinear weights with the floor held fixed.  grad_bias is grad_out summed over (batch, h, w): not
 * computed here.  Results are not bit-reproducible run to run (atomics).
 * fp32 calls with a channel-last input, offset_groups 1, in_channels % 16 == 0, out_channels % 32 == 0 and a 16-byte aligned
 * input run the MFMA implicit-GEMM kernels ("dc_fwd_mfma" / "dc_bwd_mfma"); every other call the generic kernels
 * ("dc_fwd_generic" / "dc_bwd_generic").  Which one is decided in ONE place, dc_route() of csrc/deform_conv_route.h, for these
 * and the 16-bit entries below; mvdetr_deform_conv2d_route_kind asks it.  Return 0, hipErrorInvalidValue, hipErrorNotSupported
 * (an MFMA forward of more than 65535 * 128 output channels) or the launch's HIP error. */
int mvdetr_deform_conv2d_forward_f32(void *stream, const float *input, const float *offset, const float *weight,
                                     const float *bias, int batch, int in_channels, int in_h, int in_w, int out_channels,
                                     int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                                     int dil_w, int offset_groups, int input_nhwc, float *out);
int mvdetr_deform_conv2d_forward_f64(void *stream, const double *input, const double *offset, const double *weight,
                                     const double *bias, int batch, int in_channels, int in_h, int in_w, int out_channels,
                                     int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                                     int dil_w, int offset_groups, int input_nhwc, double *out);
int mvdetr_deform_conv2d_backward_f32(void *stream, const float *grad_out, const float *input, const float *offset,
                                      const float *weight, int batch, int in_channels, int in_h, int in_w, int out_channels,
                                      int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                                      int dil_w, int offset_groups, int input_nhwc, float *grad_input, float *grad_offset,
                                      float *grad_weight);
int mvdetr_deform_conv2d_backward_f64(void *stream, const double *grad_out, const double *input, const double *offset,
                                      const double *weight, int batch, int in_channels, int in_h, int in_w, int out_channels,
                                      int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                                      int dil_w, int offset_groups, int input_nhwc, double *grad_input, double *grad_offset,
                                      double *grad_weight);
/* Name of the kernel route the last deformable-convolution call of this process took (any thread). Static; never NULL. */
const char *mvdetr_deform_conv2d_last_kernel(void);
/* The route of a call without making it (an addition, the ABI version above is unchanged): entry 0 = forward, 1 = backward (elem_size 4 or 8), 2 = the 16-bit forward
 * (elem_size 2); every pointer counts as given, `aligned` != 0 as 16-byte aligned, out_batch_stride as large enough.  Returns the
 * kind -- 0 dc_fwd_generic, 1 dc_fwd_mfma, 2 dc_fwd_mfma_half, 3 dc_bwd_generic, 4 dc_bwd_mfma, 5 a backward that only zeroes
 * its outputs -- or minus the status: -1 an empty call (returns 0, launches nothing), -2 hipErrorInvalidValue, -3
 * hipErrorNotSupported. */
int mvdetr_deform_conv2d_route_kind(int entry, int elem_size, int batch, int in_channels, int in_h, int in_w, int out_channels,
                                    int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                                    int dil_w, int offset_groups, int input_nhwc, int aligned);

/* 16-bit inference forward (float16 / bfloat16 as raw 16-bit words; 16-bit storage, fp32 arithmetic, ONE rounding on the way
 * out): "dc_fwd_mfma_half", the implicit GEMM of dc_fwd_mfma on v_mfma_f32_32x32x16_{f16,bf16} (csrc/deform_conv_half.hip).
 *   input   channel-last memory [batch, in_h, in_w, in_channels] (input_nhwc must be 1), 16-byte aligned
 *   offset  [batch, 2 * kernel_h * kernel_w, out_h, out_w] (offset_groups must be 1); positions are formed in fp32
 *   weight  PERMUTED to [kernel_h * kernel_w][out_channels][in_channels], 16-byte aligned; bias [out_channels] or NULL
 *   out     NCHW: element (b, o, h, w) at out[b * out_batch_stride + (o * out_h + h) * out_w + w]; out_batch_stride (in
 *           elements) >= out_channels * out_h * out_w, so a channel slice of a larger [batch, N * C, h, w] tensor can be
 *           written in place; relu != 0 applies max(., 0) before the rounding
 * in_channels % 16 == 0 and out_channels % 32 == 0.  The entries validate before they touch the device and launch nothing
 * they refuse: hipErrorInvalidValue for a bad shape or a null pointer, hipErrorNotSupported for offset_groups != 1,
 * input_nhwc == 0, channel counts the kernel does not take or a misaligned pointer.  Every output element is owned by one
 * lane: results are bit-reproducible run to run. */
int mvdetr_deform_conv2d_forward_f16(void *stream, const uint16_t *input, const uint16_t *offset, const uint16_t *weight,
                                     const uint16_t *bias, int batch, int in_channels, int in_h, int in_w, int out_channels,
                                     int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                                     int dil_w, int offset_groups, int input_nhwc, int relu, int64_t out_batch_stride,
                                     uint16_t *out);
int mvdetr_deform_conv2d_forward_bf16(void *stream, const uint16_t *input, const uint16_t *offset, const uint16_t *weight,
                                      const uint16_t *bias, int batch, int in_channels, int in_h, int in_w, int out_channels,
                                      int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                                      int dil_w, int offset_groups, int input_nhwc, int relu, int64_t out_batch_stride,
                                      uint16_t *out);

/* ---- Fused multi-head attention (the op inside nn.MultiheadAttention; reference call sites models/transformer.py:40,59) ---
 *   out[b, h, i, :] = sum_j softmax_j(scale * q[b, h, i, :] . k[b, h, j, :]) * v[b, h, j, :],   scale = 1 / sqrt(head_dim)
 * for `sq` queries and `sk` >= 1 keys of `batch` x `heads` independent problems; no masks.  No score or probability is
 * written to memory.  q, k, v, out and the gradients are addressed as  base + b * S[0] + h * S[1] + token * S[2] + channel
 * (ELEMENT strides; the channel is contiguous), so one [S, B, 3E] in-projection result serves as q, k and v in place.
 *   strides   HOST pointer (read during the call, an exception to the device-pointer rule): 3 int64 per tensor in the
 *             order q, k, v, out (forward: 12 values) and q, k, v, out, grad_out, grad_q, grad_k, grad_v (backward: 24).
 *   lse       [batch, heads, sq] dense: the NATURAL logarithm of sum_j exp(scale * q_i . k_j) (of the SCALED scores);
 *             written by the forward, read by the backward, which recomputes p_ij = exp(scale * q_i . k_j - lse_i).
 *   dropout   dropout_p in [0, 1); 0 = none.  Element (b, h, i, j) is KEPT iff
 *                 hash(seed, ((b * heads + h) * sq + i) * sk + j) >= (uint32_t)(dropout_p * 2^32)
 *             where hash(seed, idx) is: x = idx * 0x9E3779B97F4A7C15 + seed (mod 2^64); x ^= x >> 30;
 *             x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31; result = x >> 32
 *             (csrc/attention_hash.h, the one definition every path includes).  Kept probabilities are multiplied by
 *             1 / (1 - dropout_p) in the product with v only; lse is that of the undropped probabilities; the backward applies
 *             the same mask and factor.  Pass the forward's dropout_p and seed to the backward.
 *   workspace (backward) device buffer of mvdetr_attention_workspace_bytes(...) bytes (delta_i = grad_out_i . out_i).
 * Every element of out, lse, grad_q, grad_k, grad_v is written; inputs are never written; no atomics: results are
 * bit-reproducible run to run.  fp32 with head_dim 16 or 32, 16-byte aligned base pointers and strides that are multiples
 * of 4 take the MFMA kernels ("attn_fwd_mfma" / "attn_bwd_mfma"); everything else with head_dim <= 256 the generic
 * kernels ("attn_fwd_generic" / "attn_bwd_generic"); head_dim > 256 returns 1. */
int64_t mvdetr_attention_workspace_bytes(int batch, int heads, int sq, int sk, int head_dim, int elem_size);
int mvdetr_attention_forward_f32(void *stream, const float *q, const float *k, const float *v, const int64_t *strides,
                                 int batch, int heads, int sq, int sk, int head_dim, double dropout_p, uint64_t seed,
                                 float *out, float *lse);
int mvdetr_attention_forward_f64(void *stream, const double *q, const double *k, const double *v, const int64_t *strides,
                                 int batch, int heads, int sq, int sk, int head_dim, double dropout_p, uint64_t seed,
                                 double *out, double *lse);
int mvdetr_attention_backward_f32(void *stream, const float *grad_out, const float *q, const float *k, const float *v,
                                  const float *out, const float *lse, const int64_t *strides, int batch, int heads, int sq,
                                  int sk, int head_dim, double dropout_p, uint64_t seed, void *workspace, float *grad_q,
                                  float *grad_k, float *grad_v);
int mvdetr_attention_backward_f64(void *stream, const double *grad_out, const double *q, const double *k, const double *v,
                                  const double *out, const double *lse, const int64_t *strides, int batch, int heads, int sq,
                                  int sk, int head_dim, double dropout_p, uint64_t seed, void *workspace, double *grad_q,
                                  double *grad_k, double *grad_v);
/* 16-bit storage variants of the forward (inference; an addition, the ABI version above is unchanged): q, k, v, out are IEEE
 * binary16 (_f16) or bfloat16 (_bf16) as raw 16-bit words, addressed by the same 12 ELEMENT strides as above.  Forward only: no
 * dropout, no lse, no masks.  One kernel, "attn_fwd_mfma_half" (csrc/attention_half.hip): S = Q K^T on the 16-bit MFMA is
 * exactly the fp32 kernel's S of the upcast inputs (fp32 accumulator); softmax, running maximum and sum, rescale and 1 / l are
 * fp32; the probabilities enter the P V product as TWO 16-bit terms (hi = rn16(P), lo = rn16(P - hi)), which leaves 2^-18 (bf16)
 * / 2^-22 (f16) of P; out is rounded once, to nearest even.  No atomics: bit-reproducible run to run.
 * head_dim must be 16 or 32, sk >= 1, every base pointer 16-byte aligned and every stride a multiple of 8 elements (each row
 * starts 16-byte aligned), batch and heads <= 65535: hipErrorNotSupported (801) otherwise, and no kernel is launched (the
 * caller upcasts and takes the fp32 entry).  batch * heads * sq == 0 returns 0 without a launch. */
int mvdetr_attn_forward_f16(void *stream, const uint16_t *q, const uint16_t *k, const uint16_t *v, const int64_t *strides,
                            int batch, int heads, int sq, int sk, int head_dim, uint16_t *out);
int mvdetr_attn_forward_bf16(void *stream, const uint16_t *q, const uint16_t *k, const uint16_t *v, const int64_t *strides,
                             int batch, int heads, int sq, int sk, int head_dim, uint16_t *out);
/* Queries per workgroup of attn_fwd_mfma_half: 64, 128, or 0 = chosen by the shape (the default: 128 unless sq <= 64).  The
 * results do not depend on it.  Process-wide; returns the previous value, -1 (and changes
 * nothing) for any other argument.  For tests and tools. */
int mvdetr_attn_half_set_query_tile(int queries);
/* Name of the kernel route the last device attention call of this process took (any thread). Static; never NULL. */
const char *mvdetr_attention_last_kernel(void);
/* The route of a call without making it (an addition, the ABI version above is unchanged; the one decision is attn_route() of csrc/attention_route.h): entry 0 = forward,
 * 1 = backward (elem_size 4 or 8), 2 = the 16-bit forward (elem_size 2); every pointer counts as given, `aligned` != 0 as all of
 * them 16-byte aligned, `strides_ok` != 0 as every stride a multiple of 4 (16-bit: 8) elements.  Returns the kind -- 0
 * attn_fwd_generic, 1 attn_fwd_mfma, 2 attn_fwd_mfma_half, 3 attn_bwd_generic, 4 attn_bwd_mfma -- or minus the status: -1 an
 * empty call (returns 0, launches nothing), -2 hipErrorInvalidValue, -3 hipErrorNotSupported. */
int mvdetr_attention_route_kind(int entry, int elem_size, int batch, int heads, int sq, int sk, int head_dim, double dropout_p,
                                int strides_ok, int aligned);

/* ---- Detection objective: focal loss over heat maps, masked L1 at gathered positions ------------------------------
 * (csrc/detection_loss.hip; additive entries, the ABI version above is unchanged.)  The formulas are those of the
 * reference's loss/losses.py:17-64.  One call is ONE kernel launch over `nseg` <= MVDETR_LOSS_MAX_SEGMENTS segments;
 * `segs` is a HOST array that is copied into the kernel arguments (nothing is uploaded), every other pointer, and every
 * pointer inside a segment, is a device pointer.  `_f32` / `_f64` is the element type of logits / output, target, mask (focal)
 * and the gradients.  Results stay on the device: out[0 .. nseg-1] the segments' losses, out[nseg] = sum_s weight_s * loss_s.
 * `stats` [nseg] fp64 is written by the forward (focal: num_pos; L1: the denominator) and read by the backward, whose
 * grad_out is the [nseg + 1] gradient of `out`.  No host synchronisation, no floating-point atomics: bit-reproducible.
 *   stride / grad_stride: element strides of the [batch, channels, height, width] tensor and of its gradient (any layout).
 *   focal: target and mask (NULL: none; it multiplies the negative term) are dense NCHW of the same shape.
 *   L1: mask [batch, k] bytes, ind [batch, k] int64 = y * width + x (entries outside the map are never dereferenced and
 *       contribute nothing), target [batch, k, channels] dense; k <= 1024.
 *   grad: written entirely by the backward (NULL: that segment gets no gradient); ignored by the forward.
 *   workspace: mvdetr_focal_loss_workspace_bytes(...) bytes, 8-byte aligned, contents arbitrary.
 *   counters: MVDETR_LOSS_MAX_SEGMENTS + 1 int32, ZERO on entry; the kernel leaves them zero, so one buffer per stream
 *       can be reused call after call.
 * Kernel names: "focal_loss_fwd", "focal_loss_bwd", "reg_l1_loss_fwd", "reg_l1_loss_bwd". */
#define MVDETR_LOSS_MAX_SEGMENTS 4
typedef struct {
    const void *logits, *target, *mask;
    void *grad;
    int64_t stride[4], grad_stride[4];
    int batch, channels, height, width;
    double weight;
} mvdetr_focal_segment;
typedef struct {
    const void *output;
    const uint8_t *mask;
    const int64_t *ind;
    const void *target;
    void *grad;
    int64_t stride[4], grad_stride[4];
    int batch, channels, height, width, k;
    double weight;
} mvdetr_l1_segment;
int64_t mvdetr_focal_loss_workspace_bytes(const mvdetr_focal_segment *segs, int nseg, int elem_size);
int mvdetr_focal_loss_forward_f32(void *stream, const mvdetr_focal_segment *segs, int nseg, void *workspace, int32_t *counters,
                                  float *out, double *stats);
int mvdetr_focal_loss_forward_f64(void *stream, const mvdetr_focal_segment *segs, int nseg, void *workspace, int32_t *counters,
                                  double *out, double *stats);
int mvdetr_focal_loss_backward_f32(void *stream, const mvdetr_focal_segment *segs, int nseg, const float *grad_out,
                                   const double *stats);
int mvdetr_focal_loss_backward_f64(void *stream, const mvdetr_focal_segment *segs, int nseg, const double *grad_out,
                                   const double *stats);
int mvdetr_reg_l1_loss_forward_f32(void *stream, const mvdetr_l1_segment *segs, int nseg, float *out, double *stats);
int mvdetr_reg_l1_loss_forward_f64(void *stream, const mvdetr_l1_segment *segs, int nseg, double *out, double *stats);
int mvdetr_reg_l1_loss_backward_f32(void *stream, const mvdetr_l1_segment *segs, int nseg, const float *grad_out,
                                    const double *stats);
int mvdetr_reg_l1_loss_backward_f64(void *stream, const mvdetr_l1_segment *segs, int nseg, const double *grad_out,
                                    const double *stats);
/* Name of the kernel the last loss call of this process launched ("none" before the first), and the number of launches. */
const char *mvdetr_loss_last_kernel(void);
int64_t mvdetr_loss_launch_count(void);

/* ---- Detection extraction: world heat map -> ground-plane detections ------------------------------------------------
 * (csrc/detect.hip; additive entries, the ABI version above is unchanged.)  The last stage of the reference's test loop on
 * the device, without a host round-trip: mvdet_decode (utils/decode.py:80-93), the cls_thres test (trainer.py:130-132) and
 * the greedy distance NMS (utils/nms.py:7-44).  Per frame b of heatmap [batch, 1, height, width] (raw logits) and offset
 * [batch, 2, height, width] (NULL: every cell's centre, +0.5), both addressed through their four element strides (host
 * arrays), so channels_last maps are read in place:
 *   score  s = 1 / (1 + exp(-logit)); a cell is a candidate when s > cls_thres (rounded to the element type; NaN never is);
 *   position  x = (column + dx) * reduce, y = (row + dy) * reduce, one rounded add and one rounded multiply; swap_xy != 0
 *          exchanges them (the reference's indexing = 'ij', trainer.py:125-128);
 *   NMS    candidates are visited in descending score order, EQUAL SCORES HIGHER ROW-MAJOR CELL INDEX FIRST (the reference's
 *          order among ties is that of an unstable torch.sort; on tie-free input the two agree); only the first top_k in
 *          that order take part (top_k <= 0: all); one is kept unless an already kept one lies within
 *          sqrt(dx * dx + dy * dy) <= dist_thres (rounded to the element type; products and sum rounded separately).
 * Outputs, all device memory: det [batch, max_det, 3] = (x, y, score) rows in kept order, cell [batch, max_det] the cells'
 * row-major indices, count [batch] the TRUE number kept, also when it exceeds max_det (rows beyond max_det are dropped,
 * never written); rows at and after min(count, max_det) are zero.  Correct for any number of candidates up to
 * height * width (<= 2^30).  workspace: mvdetr_detect_workspace_bytes(batch, height, width, elem_size) bytes, 16-byte aligned,
 * contents arbitrary.  Two launches ("detect_compact+detect_nms"), no host synchronisation, no floating-point atomics:
 * bit-reproducible.  The candidate list lives in LDS up to 3072 (f32) / 1728 (f64) candidates of a frame and in the
 * workspace beyond; MVDETR_DETECT_ROUTE=global keeps it in the workspace always ("..._global").
 * mvdetr_distance_nms_*: the NMS stage alone, the contract of utils/nms.py:7-44 -- points [n, 2] and scores [n] dense ->
 * keep [n] int64 (the kept indices, then zeros) and count [1]; workspace of mvdetr_detect_workspace_bytes(1, 1, n, elem_size)
 * bytes; one launch ("distance_nms" / "distance_nms_global"); n >= 1. */
int64_t mvdetr_detect_workspace_bytes(int batch, int height, int width, int elem_size);
int mvdetr_detect_forward_f32(void *stream, const float *heatmap, const int64_t *heatmap_stride, const float *offset,
                              const int64_t *offset_stride, int batch, int height, int width, double reduce, double cls_thres,
                              double dist_thres, int top_k, int swap_xy, int max_det, void *workspace, float *det, int32_t *cell,
                              int32_t *count);
int mvdetr_detect_forward_f64(void *stream, const double *heatmap, const int64_t *heatmap_stride, const double *offset,
                              const int64_t *offset_stride, int batch, int height, int width, double reduce, double cls_thres,
                              double dist_thres, int top_k, int swap_xy, int max_det, void *workspace, double *det, int32_t *cell,
                              int32_t *count);
int mvdetr_distance_nms_f32(void *stream, const float *points, const float *scores, int n, double dist_thres, int top_k,
                            void *workspace, int64_t *keep, int32_t *count);
int mvdetr_distance_nms_f64(void *stream, const double *points, const double *scores, int n, double dist_thres, int top_k,
                            void *workspace, int64_t *keep, int32_t *count);
/* Name of the route the last device detect / NMS call of this process took ("none" before the first), and the number of
 * kernel launches these entries have made. */
const char *mvdetr_detect_last_kernel(void);
int64_t mvdetr_detect_launch_count(void);

/* ---- Peak extraction: heat map (+ offset, + wh) -> the top_k local maxima of every map ---------------------------------
 * (csrc/peak_detect.hip; additive entries, the ABI version above is unchanged.)  The reference's ctdet_decode
 * (utils/decode.py:7-77) for single-channel maps, on the device and without a host round-trip.  Per map b of heatmap
 * [batch, 1, height, width] (raw logits), offset and wh [batch, 2, height, width] (either may be NULL), all addressed through
 * their four element strides (host arrays), so channels_last maps are read in place:
 *   score      s = 1 / (1 + exp(-logit)), one expression evaluated once per cell;
 *   candidate  a cell whose score equals the maximum of the scores of its 3x3 neighbourhood inside the map (max_pool2d pads
 *              with -inf), compared on the scores, so a plateau of equal scores is kept whole; with use_thres != 0 also
 *              s > cls_thres (rounded to the element type).  A NaN score is never a candidate and is ignored in its
 *              neighbours' maxima (max_pool2d would propagate it: the library's deviation);
 *   order      score descending, EQUAL SCORES HIGHER ROW-MAJOR CELL INDEX FIRST (the library's tie rule; torch.topk's order
 *              among ties is unspecified); the first top_k candidates are written, 1 <= top_k <= 1024;
 *   row        x = column + dx, y = row + dy (one rounded add; 0.5 without an offset map), w and h as gathered, and the box
 *              x1 = (x - 0.5 w) scale, y1 = (y - h) scale, x2 = (x + 0.5 w) scale, y2 = y scale: the decoded point is the
 *              foot point, the bottom-centre of the box; every product, sum and difference rounded on its own.
 * Outputs, all device memory: xy [batch, top_k, 2], wh_out [batch, top_k, 2] and box [batch, top_k, 4] (both NULL when wh
 * is), score [batch, top_k], cell [batch, top_k] row-major indices, count [batch] the TRUE number of candidates, also when
 * it exceeds top_k; rows at and after min(count, top_k) are zero.  Correct for any number of candidates from 0 to
 * height * width (<= 2^30).  workspace: mvdetr_peak_detect_workspace_bytes(batch, height, width, elem_size) bytes, 16-byte
 * aligned, contents arbitrary.  Two launches, no host synchronisation, no floating-point and no device-scope atomics:
 * bit-reproducible.  A map's candidate list lives in LDS up to mvdetr_peak_detect_lds_capacity(elem_size) candidates and in
 * the workspace beyond; the count decides, on the device. */
int64_t mvdetr_peak_detect_workspace_bytes(int batch, int height, int width, int elem_size);
int mvdetr_peak_detect_lds_capacity(int elem_size);
int mvdetr_peak_detect_forward_f32(void *stream, const float *heatmap, const int64_t *heatmap_stride, const float *offset,
                                   const int64_t *offset_stride, const float *wh, const int64_t *wh_stride, int batch, int height,
                                   int width, int top_k, double cls_thres, int use_thres, double scale, void *workspace, float *xy,
                                   float *wh_out, float *box, float *score, int32_t *cell, int32_t *count);
int mvdetr_peak_detect_forward_f64(void *stream, const double *heatmap, const int64_t *heatmap_stride, const double *offset,
                                   const int64_t *offset_stride, const double *wh, const int64_t *wh_stride, int batch, int height,
                                   int width, int top_k, double cls_thres, int use_thres, double scale, void *workspace, double *xy,
                                   double *wh_out, double *box, double *score, int32_t *cell, int32_t *count);
/* Name of the route the last device call of this process took: "peak_compact+peak_select", with "_global" appended when any
 * map of that call kept its list in the workspace ("none" before the first call).  The route is chosen on the device, so this
 * WAITS for the device and reads one flag back: for tests and tools.  And the number of kernel launches these entries made. */
const char *mvdetr_peak_detect_last_kernel(void);
int64_t mvdetr_peak_detect_launch_count(void);

/* ---- CPU path (host pointers, no stream, synchronous) ------------------------------------------------------------
 * The reference extension raises for CPU tensors (ms_deform_attn_cpu.cpp:17-41 are stubs; ms_deform_attn.h:38,60).
 * These entry points make the same contracts work on host memory: same argument meaning and layouts as the device
 * functions above; std::thread parallel (MVDETR_HOST_THREADS, else OMP_NUM_THREADS, else all cores up to 64);
 * deterministic (no atomics).  grad_value / grad_src are ACCUMULATED into: pass them zeroed.
 * warp: `layout_nhwc` bits 0/1 as above; `mode` 0 = bilinear, 1 = nearest.  Return 0 on success. */
int mvdetr_msda_forward_host_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                 const float *sampling_loc, const float *attn_weight, int batch, int spatial_size,
                                 int num_heads, int channels, int num_levels, int num_query, int num_point, float *out);
int mvdetr_msda_forward_host_f64(const double *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                 const double *sampling_loc, const double *attn_weight, int batch, int spatial_size,
                                 int num_heads, int channels, int num_levels, int num_query, int num_point, double *out);
int mvdetr_msda_backward_host_f32(const float *grad_output, const float *value, const int64_t *spatial_shapes,
                                  const int64_t *level_start_index, const float *sampling_loc, const float *attn_weight,
                                  int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                  int num_point, float *grad_value, float *grad_sampling_loc, float *grad_attn_weight);
int mvdetr_msda_backward_host_f64(const double *grad_output, const double *value, const int64_t *spatial_shapes,
                                  const int64_t *level_start_index, const double *sampling_loc, const double *attn_weight,
                                  int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                  int num_point, double *grad_value, double *grad_sampling_loc, double *grad_attn_weight);
int mvdetr_warp_perspective_forward_host_f32(const float *src, const float *mats, int n, int channels, int src_h, int src_w,
                                             int dst_h, int dst_w, int layout_nhwc, int mode, float *dst);
int mvdetr_warp_perspective_forward_host_f64(const double *src, const double *mats, int n, int channels, int src_h, int src_w,
                                             int dst_h, int dst_w, int layout_nhwc, int mode, double *dst);
int mvdetr_warp_perspective_backward_host_f32(const float *grad_dst, const float *mats, int n, int channels, int src_h,
                                              int src_w, int dst_h, int dst_w, int layout_nhwc, int mode, float *grad_src);
int mvdetr_warp_perspective_backward_host_f64(const double *grad_dst, const double *mats, int n, int channels, int src_h,
                                              int src_w, int dst_h, int dst_w, int layout_nhwc, int mode, double *grad_src);

/* deformable convolution on host memory: same arguments as the device entries without the stream; grad_input is
 * accumulated into, grad_offset and grad_weight are written; deterministic */
int mvdetr_deform_conv2d_forward_host_f32(const float *input, const float *offset, const float *weight, const float *bias,
                                          int batch, int in_channels, int in_h, int in_w, int out_channels, int kernel_h,
                                          int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                                          int offset_groups, int input_nhwc, float *out);
int mvdetr_deform_conv2d_forward_host_f64(const double *input, const double *offset, const double *weight, const double *bias,
                                          int batch, int in_channels, int in_h, int in_w, int out_channels, int kernel_h,
                                          int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                                          int offset_groups, int input_nhwc, double *out);
int mvdetr_deform_conv2d_backward_host_f32(const float *grad_out, const float *input, const float *offset, const float *weight,
                                           int batch, int in_channels, int in_h, int in_w, int out_channels, int kernel_h,
                                           int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                                           int offset_groups, int input_nhwc, float *grad_input, float *grad_offset,
                                           float *grad_weight);
int mvdetr_deform_conv2d_backward_host_f64(const double *grad_out, const double *input, const double *offset,
                                           const double *weight, int batch, int in_channels, int in_h, int in_w, int out_channels,
                                           int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                                           int dil_h, int dil_w, int offset_groups, int input_nhwc, double *grad_input,
                                           double *grad_offset, double *grad_weight);

/* attention on host memory: same arguments as the device entries without the stream and the workspace; deterministic; never
 * more than a 64-key tile of scores per thread.  mvdetr_attention_dropout_mask_host writes the keep decision (1 = kept) of
 * every element of the [batch, heads, sq, sk] probabilities, as the kernels and the host path make it (tests). */
int mvdetr_attention_forward_host_f32(const float *q, const float *k, const float *v, const int64_t *strides, int batch,
                                      int heads, int sq, int sk, int head_dim, double dropout_p, uint64_t seed, float *out,
                                      float *lse);
int mvdetr_attention_forward_host_f64(const double *q, const double *k, const double *v, const int64_t *strides, int batch,
                                      int heads, int sq, int sk, int head_dim, double dropout_p, uint64_t seed, double *out,
                                      double *lse);
int mvdetr_attention_backward_host_f32(const float *grad_out, const float *q, const float *k, const float *v, const float *out,
                                       const float *lse, const int64_t *strides, int batch, int heads, int sq, int sk,
                                       int head_dim, double dropout_p, uint64_t seed, float *grad_q, float *grad_k,
                                       float *grad_v);
int mvdetr_attention_backward_host_f64(const double *grad_out, const double *q, const double *k, const double *v,
                                       const double *out, const double *lse, const int64_t *strides, int batch, int heads,
                                       int sq, int sk, int head_dim, double dropout_p, uint64_t seed, double *grad_q,
                                       double *grad_k, double *grad_v);
int mvdetr_attention_dropout_mask_host(uint64_t seed, double dropout_p, int batch, int heads, int sq, int sk, uint8_t *mask);

/* detection extraction on host memory: same arguments as the device entries without the stream and the workspace, the same
 * arithmetic and tie rule; one thread per frame */
int mvdetr_detect_forward_host_f32(const float *heatmap, const int64_t *heatmap_stride, const float *offset,
                                   const int64_t *offset_stride, int batch, int height, int width, double reduce, double cls_thres,
                                   double dist_thres, int top_k, int swap_xy, int max_det, float *det, int32_t *cell, int32_t *count);
int mvdetr_detect_forward_host_f64(const double *heatmap, const int64_t *heatmap_stride, const double *offset,
                                   const int64_t *offset_stride, int batch, int height, int width, double reduce, double cls_thres,
                                   double dist_thres, int top_k, int swap_xy, int max_det, double *det, int32_t *cell,
                                   int32_t *count);
int mvdetr_distance_nms_host_f32(const float *points, const float *scores, int n, double dist_thres, int top_k, int64_t *keep,
                                 int32_t *count);
int mvdetr_distance_nms_host_f64(const double *points, const double *scores, int n, double dist_thres, int top_k, int64_t *keep,
                                 int32_t *count);

/* peak extraction on host memory: same arguments as the device entries without the stream and the workspace, the same
 * candidate test, arithmetic and tie rule; one thread per map */
int mvdetr_peak_detect_forward_host_f32(const float *heatmap, const int64_t *heatmap_stride, const float *offset,
                                        const int64_t *offset_stride, const float *wh, const int64_t *wh_stride, int batch,
                                        int height, int width, int top_k, double cls_thres, int use_thres, double scale, float *xy,
                                        float *wh_out, float *box, float *score, int32_t *cell, int32_t *count);
int mvdetr_peak_detect_forward_host_f64(const double *heatmap, const int64_t *heatmap_stride, const double *offset,
                                        const int64_t *offset_stride, const double *wh, const int64_t *wh_stride, int batch,
                                        int height, int width, int top_k, double cls_thres, int use_thres, double scale, double *xy,
                                        double *wh_out, double *box, double *score, int32_t *cell, int32_t *count);

/* Frame ingest: uint8 camera frames [k, src_h, src_w, 3] (pixels dense: 3 bytes each, src_w of them per row; frame_stride and
 * row_stride in BYTES are free, so a cropped view is read in place) -> out [k, 3, dst_h, dst_w] in NCHW memory, or
 * [k, dst_h, dst_w, 3] (channels-last) with layout_nhwc != 0.  One pass does the reference dataset's augmentation warp, ToTensor,
 * Normalize and Resize:
 *   out[k, c, y, x] = sum over the 4 taps of the bilinear resize (F.interpolate, align_corners=False, no antialias; positions
 *   ((2x + 1) src_w - dst_w) / (2 dst_w), formed from integers, clamped below at 0, second tap min(x0 + 1, src_w - 1)) of
 *   A[k, c, yy, xx] * a_c + b_c, with a_c = 1 / (255 std_c) and b_c = -mean_c / std_c supplied by the caller.
 * A is the frame itself when mats is null.  Otherwise mats [k, 9] (row-major 3x3, fp64, destination pixel <- source pixel,
 * integer pixel centres: cv2.warpPerspective's convention) and A[yy, xx] is the bilinear blend of the four frame pixels
 * around (u / w, v / w), (u, v, w) = mats^-1 (xx, yy, 1) in fp64, every tap outside the frame = `border` (a grey level), and
 * = border where w <= 0 or the position or the inverse is not finite.  A is not rounded to uint8.  The blend is fp32; the
 * 16-bit outputs round once on the store.  Sizes up to 16384, k up to 65535.  No allocation, no synchronisation.
 * mvdetr_ingest_last_kernel: the kernel the last call of this process launched ("ingest_identity_wide" -- aligned 16-byte
 * loads, frames / strides multiples of 16; "ingest_identity_narrow"; "ingest_identity_direct" -- no LDS, large downscales;
 * "ingest_warp"; "none"). */
int mvdetr_ingest_frames_f32(void *stream, const uint8_t *frames, int64_t frame_stride, int64_t row_stride, const double *mats,
                             float a0, float a1, float a2, float b0, float b1, float b2, int k, int src_h, int src_w, int dst_h,
                             int dst_w, int layout_nhwc, float border, float *out);
int mvdetr_ingest_frames_f16(void *stream, const uint8_t *frames, int64_t frame_stride, int64_t row_stride, const double *mats,
                             float a0, float a1, float a2, float b0, float b1, float b2, int k, int src_h, int src_w, int dst_h,
                             int dst_w, int layout_nhwc, float border, uint16_t *out);
int mvdetr_ingest_frames_bf16(void *stream, const uint8_t *frames, int64_t frame_stride, int64_t row_stride, const double *mats,
                              float a0, float a1, float a2, float b0, float b1, float b2, int k, int src_h, int src_w, int dst_h,
                              int dst_w, int layout_nhwc, float border, uint16_t *out);
const char *mvdetr_ingest_last_kernel(void);

/* frame ingest on host memory: the same contract without the stream, scale / bias / border as doubles (the f32 entry rounds
 * them to float and blends in float, the f64 entry blends in double); threads own output rows */
int mvdetr_ingest_frames_host_f32(const uint8_t *frames, int64_t frame_stride, int64_t row_stride, const double *mats, double a0,
                                  double a1, double a2, double b0, double b1, double b2, int k, int src_h, int src_w, int dst_h,
                                  int dst_w, int layout_nhwc, double border, float *out);
int mvdetr_ingest_frames_host_f64(const uint8_t *frames, int64_t frame_stride, int64_t row_stride, const double *mats, double a0,
                                  double a1, double a2, double b0, double b1, double b2, int k, int src_h, int src_w, int dst_h,
                                  int dst_w, int layout_nhwc, double border, double *out);

/* Training targets: the CenterNet-style ground truth of one SEGMENT of `maps` equally shaped [height, width] maps (the
 * reference's get_gt, datasets/frameDataset.py:19-46, with the box half of its random_affine, utils/image_utils.py:46-83) from
 * padded annotations, in one launch; no count is read back, nothing allocates or synchronises.
 *   coords   [maps, cap, 4] boxes (x1, y1, x2, y2) with is_boxes != 0, else [maps, cap, 2] points (x, y); fp64, at `reduce`
 *            times the map's resolution
 *   count    [maps] int32, the valid objects of a map (clamped to [0, cap]); pids [maps, cap] int64 or null (zeros)
 *   mats     [maps, 9] row-major 3x3 or null, boxes only: the augmentation (source pixel -> destination pixel; its first two
 *            rows are used); shrink [maps] or null (= 1), with mats only: sqrt(max(|sin a|, |cos a|)) of the rotation angle,
 *            made by the caller (the kernel has no sin / cos / sqrt); img_h, img_w: the image the boxes are clipped to
 *   keep     [maps] bytes or null: a map with keep == 0 gets all-zero outputs, heat map included (camera dropout)
 *   patch    [2 radius + 1, 2 radius + 1] fp32, the gaussian made by the caller (no device exp); radius <= max_radius()
 *   cap <= 1024, cap <= top_k, height and width <= 16384, maps <= 65535
 * Arithmetic, fp64 and WITHOUT FMA contraction until the stated roundings, per object in order:
 *   with mats  each corner (x1,y1) (x2,y2) (x1,y2) (x2,y1) -> X = (M00 x + M01 y) + M02, Y = (M10 x + M11 y) + M12; hull = min /
 *              max of the four; per axis c = (hi + lo) / 2, s = (hi - lo) shrink, lo' = min(max(c - s / 2, 0), lim), hi' =
 *              min(max(c + s / 2, 0), lim), lim = img_w - 1 / img_h - 1; with w = hi'x - lo'x, h = hi'y - lo'y, area =
 *              (x2 - x1)(y2 - y1) the box is kept when w > 4 && h > 4, w h / (area + 1e-16) > 0.1 and
 *              max(w / (h + 1e-16), h / (w + 1e-16)) < 10.  Kept boxes are compacted in order: slot = rank among the kept.
 *   without    slot = object index.
 *   a box's point is x = (x1 + x2) / 2, y = y2, its size w = x2 - x1, h = y2 - y1; centre ct = fp32(x / reduce), fp32(y / reduce)
 *   (one rounding each); inside when 0 <= ct.x < width && 0 <= ct.y < height on the fp32 values, else the slot stays empty;
 *   cell = trunc(ct), idx = cell.y width + cell.x, offset = ct - fp32(cell) in fp32, wh = fp32(w / reduce), fp32(h / reduce).
 * Outputs (EVERY element is written; empty slots and untouched cells are zero): heatmap [maps, height, width] fp32, cell (y, x)
 * = max of patch[y - cy + radius, x - cx + radius] over the inside objects with |x - cx|, |y - cy| <= radius; reg_mask
 * [maps, top_k] bytes 0 / 1; idx, pid [maps, top_k] int64; offset [maps, top_k, 2] fp32; wh [maps, top_k, 2] fp32 (boxes:
 * required; points: null).  The result is bit-reproducible (a gather: no atomics).
 * mvdetr_frame_targets_launch_count: kernel launches of this process so far (one per call with maps > 0). */
int mvdetr_frame_targets_f64(void *stream, const double *coords, int is_boxes, const int32_t *count, const int64_t *pids,
                             const double *mats, const double *shrink, const uint8_t *keep, const float *patch, int maps, int cap,
                             int height, int width, int img_h, int img_w, int radius, int top_k, double reduce, float *heatmap,
                             uint8_t *reg_mask, int64_t *idx, int64_t *pid, float *offset, float *wh);
int mvdetr_frame_targets_max_radius(void);
int64_t mvdetr_frame_targets_launch_count(void);

/* the same on host memory, synchronous: the same arithmetic operation for operation (threads own maps, then heat-map rows) */
int mvdetr_frame_targets_host_f64(const double *coords, int is_boxes, const int32_t *count, const int64_t *pids,
                                  const double *mats, const double *shrink, const uint8_t *keep, const float *patch, int maps,
                                  int cap, int height, int width, int img_h, int img_w, int radius, int top_k, double reduce,
                                  float *heatmap, uint8_t *reg_mask, int64_t *idx, int64_t *pid, float *offset, float *wh);

#ifdef __cplusplus
}
#endif
#endif /* MVDETR_OPS_H */
