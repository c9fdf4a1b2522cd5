/* C-ABI of the MI355X (gfx950) kernels behind SimPB's hybrid 2D/3D decoder hot path.
 *
 * Plain pointers and sizes only: every pointer is a DEVICE pointer owned by the caller, the
 * callee never allocates or frees, every output buffer is fully overwritten, and `stream` is a
 * hipStream_t (NULL = the legacy default stream). Each function returns 0 on success or one of
 * the SIMPB_E* codes; nothing is thrown, nothing is printed.
 *
 * Citations are file:line under /root/reference/projects/mmdet3d_plugin/.
 */
#ifndef SIMPB_HIP_H
#define SIMPB_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define SIMPB_OK 0
#define SIMPB_EINVAL 1   /* null pointer, non-positive size, or a layout the kernels cannot take */
#define SIMPB_ELAUNCH 2  /* hipGetLastError() after the launch was not hipSuccess */

#define SIMPB_RECORD3D_WIDTH 15 /* columns of the 3D detection record (simpb_decode3d_record) */

/* Library/ABI version (bumped when a signature changes). */
int simpb_abi_version(void);

/* Text of the HIP error behind the last SIMPB_ELAUNCH on the calling thread ("" if none). */
const char* simpb_last_error(void);

/* Optional per-launch timing for measurement (bench.py): while enabled, the sampler entry points
 * record a HIP event pair on their launch stream directly around the kernel launch.
 *   simpb_timing_enable(n)  allocate n event pairs (0 = disable and free); not thread-safe
 *   simpb_timing_read(id, ms_out, max_n)  waits for the recorded pairs of kernel `id`, writes their
 *                           elapsed milliseconds, returns how many (or -1)
 *   simpb_timing_reset()    forget the recorded pairs, keep the allocation */
#define SIMPB_KERNEL_DAF 1
#define SIMPB_KERNEL_MSDA 2
int simpb_timing_enable(int capacity);
int simpb_timing_read(int kernel_id, float* ms_out, int max_n);
void simpb_timing_reset(void);

/* Replaces `deformable_aggregation(...)` (ops/src/deformable_aggregation.cpp:4-19, launcher
 * ops/src/deformable_aggregation_cuda.cu:265-288, kernel :129-187); same argument order plus the
 * stream. Layouts (deformable_aggregation.cpp:22-28):
 *   mc_ms_feat        f32 [batch_size, num_feat, num_embeds]      channel innermost
 *   spatial_shape     i32 [num_cams, num_scale, 2] = (H, W)
 *   scale_start_index i32 [num_cams, num_scale]                  token offset inside num_feat
 *   sample_location   f32 [batch_size, num_anchors, num_pts, num_cams, 2] = (x/W_img, y/H_img)
 *   weights           f32 [batch_size, num_anchors, num_pts, num_cams, num_scale, num_groups]
 *   output            f32 [batch_size, num_anchors, num_embeds]  overwritten (no pre-zero needed)
 * num_embeds % num_groups must be 0. Results are deterministic (no atomics). */
int simpb_deformable_aggregation_forward(
    float* output, const float* mc_ms_feat, const int* spatial_shape, const int* scale_start_index,
    const float* sample_location, const float* weights,
    int batch_size, int num_cams, int num_feat, int num_embeds, int num_scale,
    int num_anchors, int num_pts, int num_groups, void* stream);

/* DeformableFeatureAggregation.forward between its Linear layers in ONE launch (models/blocks.py:110-162): key points
 * (models/detection3d/blocks.py:181-222) -> project_points (blocks.py:198-213) -> softmax of _get_weights (:177-187) ->
 * the aggregation above. The workgroup that aggregates an anchor computes its num_pts x num_cams sampling locations and
 * its softmax weights on chip, so neither tensor exists in memory (simpb_dfa_points + simpb_dfa_weights +
 * simpb_deformable_aggregation_forward are the same arithmetic in three launches; tests compare the two).
 *   mc_ms_feat   f32 (feat_is_f16 = 0) or f16 (1) [batch_size, num_feat, num_embeds]; the f16 form is for tokens that are
 *                f16 numbers anyway (the fp16 backbone's output, simpb.py:63): same results, half the gather bytes
 *   anchor f32 [bs, A, 11]; learnable f32 [bs, A, num_learn * 3] (raw learnable_fc output); fix_scale f32 [num_fix, 3]
 *   projection_mat f32 [bs, cams, 4, 4]; image_wh f32 [bs, cams, 2]
 *   feat_logits f32 [bs, A, num_scale * num_pts * num_groups] = weights_fc(feature + anchor_embed)
 *   cam_logits  f32 [bs, cams, num_scale * num_pts * num_groups] = camera_embed . weights_fc.weight^T
 *   loc_out / weights_out: optional (NULL) copies of the two on-chip tensors in the layouts of the operator above
 * Supported layout: num_embeds <= 256, (num_embeds / num_groups) % 4 == 0, num_groups a power of two <= 64,
 * num_pts * num_cams <= 128, cams * num_scale * num_pts * num_groups <= 4096; anything else returns SIMPB_EINVAL. */
int simpb_dfa_fused_forward(
    float* output, const void* mc_ms_feat, int feat_is_f16, const int* spatial_shape, const int* scale_start_index,
    const float* anchor, const float* learnable, const float* fix_scale, const float* projection_mat, const float* image_wh,
    const float* feat_logits, const float* cam_logits, float* loc_out, float* weights_out, int batch_size, int num_cams,
    int num_feat, int num_embeds, int num_scale, int num_anchors, int num_fix, int num_learn, int num_groups, void* stream);
/* The same with `cam_valid` u8 [batch_size, num_cams] (device; NULL = every camera, identical to simpb_dfa_fused_forward): a
 * camera with 0 delivered no frame, and stream b is aggregated exactly as the reference aggregates it when given the
 * remaining cameras only. The softmax over (cam, level, point) runs over the valid cameras: a masked camera's logits count
 * as -inf by substitution, so its weights are exactly 0.0 (weights_out too) and its locations are (-1, -1) (loc_out too).
 * Nothing of a masked camera is read -- not its tokens (no tap is issued), its projection_mat / image_wh rows or its
 * cam_logits row: they may hold anything, NaN included. A stream with no valid camera gives zeros (callers refuse it). */
int simpb_dfa_fused_forward_cams(
    float* output, const void* mc_ms_feat, int feat_is_f16, const int* spatial_shape, const int* scale_start_index,
    const float* anchor, const float* learnable, const float* fix_scale, const float* projection_mat, const float* image_wh,
    const float* feat_logits, const float* cam_logits, float* loc_out, float* weights_out, int batch_size, int num_cams,
    int num_feat, int num_embeds, int num_scale, int num_anchors, int num_fix, int num_learn, int num_groups,
    const unsigned char* cam_valid, void* stream);
/* The same for a rig of num_cams = 1..8 cameras (cam_valid may be NULL). The rest of the layout stays the shipped one
 * (num_scale 4, num_fix 7, num_learn 6, num_groups 8, num_embeds 256): there is one compiled kernel per camera count, and
 * anything else returns SIMPB_EINVAL before any HIP call. Six cameras launch the kernels the two entries above launch. */
int simpb_dfa_fused_forward_rig(
    float* output, const void* mc_ms_feat, int feat_is_f16, const int* spatial_shape, const int* scale_start_index,
    const float* anchor, const float* learnable, const float* fix_scale, const float* projection_mat, const float* image_wh,
    const float* feat_logits, const float* cam_logits, float* loc_out, float* weights_out, int batch_size, int num_cams,
    int num_feat, int num_embeds, int num_scale, int num_anchors, int num_fix, int num_learn, int num_groups,
    const unsigned char* cam_valid, void* stream);


/* Replaces `deformable_aggregation_grad(...)` (ops/src/deformable_aggregation.cpp:64-84, launcher
 * ops/src/deformable_aggregation_cuda.cu:291-318, kernels :62-126,190-262), the backward of the
 * operator (ops/deformable_aggregation.py:39-75). Layouts as the forward; grad_output f32
 * [batch_size, num_anchors, num_embeds]. All three gradients are fully written (the callee clears
 * grad_mc_ms_feat itself; the caller need not pre-zero anything). grad_weights and
 * grad_sampling_location are deterministic; grad_mc_ms_feat is accumulated with float atomics.
 * Supported layout: num_embeds % 64 == 0, num_embeds <= 256, (num_embeds / num_groups) % 32 == 0,
 * num_pts * num_cams <= 128 (the shipped 256 / 8 / 13 x 6); anything else returns SIMPB_EINVAL. */
int simpb_deformable_aggregation_backward(
    float* grad_mc_ms_feat, float* grad_sampling_location, float* grad_weights, const float* mc_ms_feat,
    const int* spatial_shape, const int* scale_start_index, const float* sample_location, const float* weights,
    const float* grad_output, int batch_size, int num_cams, int num_feat, int num_embeds, int num_scale,
    int num_anchors, int num_pts, int num_groups, void* stream);

/* Replaces the per-camera loop over mmcv's `ms_deform_attn_forward` in
 * QueryGroupMultiScaleDeformableAttention.forward (models/group_attn.py:222-235): ONE launch for
 * all camera groups. Sampling rule = mmcv's CUDA op = grid_sample(bilinear, zeros,
 * align_corners=False).
 *   value          f32 [batch_size, num_cams, num_value, num_heads, channels]
 *   spatial_shapes i64 [num_levels, 2] = (H, W)      (group_attn.py passes torch.long)
 *   level_start    i64 [num_levels]
 *   sampling_loc   f32 [batch_size, num_query, num_heads, num_levels, num_points, 2] = (x, y) in [0,1]
 *   attn_weight    f32 [batch_size, num_query, num_heads, num_levels, num_points]
 *   query_cam      i32 [num_query]   camera group of each query slot (what query_groups encodes)
 *   output         f32 [batch_size, num_query, num_heads * channels]  overwritten */
int simpb_ms_deform_attn_grouped_forward(
    float* output, const float* value, const long long* spatial_shapes, const long long* level_start,
    const float* sampling_loc, const float* attn_weight, const int* query_cam,
    int batch_size, int num_cams, int num_value, int num_heads, int channels,
    int num_levels, int num_points, int num_query, void* stream);

/* The same operator WITHOUT value_proj over the camera tokens (models/group_attn.py:176-179): sampling and the value
 * projection are both linear, so for head h of a query
 *   sum_s a_s bilinear(W_h x + b_h)(s) = W_h . [sum_s a_s bilinear(x)(s)] + b_h [sum_s a_s (valid tap weights of s)]
 * (the reference zero-pads the PROJECTED map, hence the second bracket). This entry computes the brackets from the raw
 * tokens; the caller applies W_h (folded with output_proj) as one query-sized product over agg. Softmax of the attention
 * logits and reference point + offset / (W_l, H_l) (group_attn.py:181-201) are done here as well.
 *   agg        f32 [batch_size, num_query, ld_agg >= 8 * 256 + 128]: per query [head][256 channel sums] | 8 tap-weight
 *              sums | zeros up to 128; rows of capacity slots (query_cam < 0 or >= *m_live) are NOT written
 *   tokens     f16 (tokens_are_f16 = 1) or f32 [batch_size, num_cams, num_value, 256]: the camera tokens themselves
 *   raw        f32 [batch_size * num_query, ld_raw]: sampling_offsets (heads x levels x points x 2) | attention logits
 *   ref        f32 [batch_size * num_query, ld_ref >= 2]: reference point (x, y) in [0, 1]
 * Compiled for the shipped layout (8 heads x 32 channels, 4 levels, 4 points); anything else returns SIMPB_EINVAL and
 * the caller uses value_proj + simpb_ms_deform_attn_grouped_forward. */
int simpb_msda_linear_forward(float* agg, int ld_agg, const void* tokens, int tokens_are_f16,
                              const long long* spatial_shapes, const long long* level_start, const float* raw,
                              int ld_raw, const float* ref, int ld_ref, const int* query_cam, const int* m_live,
                              int batch_size, int num_cams, int num_value, int num_heads, int channels,
                              int num_levels, int num_points, int num_query, void* stream);

/* Backward of simpb_ms_deform_attn_grouped_forward (what mmcv's ms_deform_attn_backward does per camera
 * group behind models/group_attn.py:227-235). grad_output f32 [bs, num_query, heads*channels]; all three
 * gradients are fully written (grad_value is cleared by the callee and accumulated with float atomics;
 * the other two are deterministic). Supported layout: heads * channels == 256, channels/4 a power of two. */
int simpb_ms_deform_attn_grouped_backward(
    float* grad_value, float* grad_sampling_loc, float* grad_attn_weight, const float* value,
    const long long* spatial_shapes, const long long* level_start, const float* sampling_loc, const float* attn_weight,
    const int* query_cam, const float* grad_output, int batch_size, int num_cams, int num_value, int num_heads,
    int channels, int num_levels, int num_points, int num_query, void* stream);

/* y[M, N] = x[M, K] . weight[N, K]^T + bias[N] (bias may be NULL), optional ReLU; exact fp32 on the
 * f32 matrix cores. Replaces nn.Linear where the reference runs it over every camera token:
 * value_proj in QueryGroupMultiScaleDeformableAttention.forward (models/group_attn.py:176), and the
 * other large-M Linear layers of the head. Row-major, K contiguous; K % 32 == 0; x and weight
 * 16-byte aligned. */
int simpb_linear_f32(float* y, const float* x, const float* weight, const float* bias, int M, int N, int K,
                     int relu, void* stream);

/* Same product on the FP16 matrix cores at fp32-grade accuracy: weight = weight_hi + weight_lo / 2048 with both parts
 * f16 [N, K] (weight_hi = half(weight), weight_lo = half((weight - weight_hi) * 2048), prepared once by the caller);
 * x is split the same way while it is staged; y = x_hi.W_hi^T + (x_hi.W_lo^T + x_lo.W_hi^T) / 2048 + bias in fp32
 * accumulators (the dropped x_lo.W_lo^T term is ~2^-22 relative). Any finite x (rows outside [2^-10, 2^15) are staged
 * with a power-of-two exponent, as simpb_gemm_f32); every weight row's largest |w| must lie in that window or be 0. Used for value_proj
 * (models/group_attn.py:176), where the exact kernel above is compute-bound. K % 32 == 0; 16-byte aligned. */
int simpb_linear_f16x3(float* y, const float* x, const void* weight_hi, const void* weight_lo, const float* bias, int M,
                       int N, int K, void* stream);

/* The same product for an x that is already half precision (f16 [M, K]; e.g. the camera tokens as the fp16 backbone
 * produced them, simpb.py:63): its trailing part is zero, so y = x.W_hi^T + (x.W_lo^T) / 2048 + bias in two passes with the
 * error of the three-pass form, half the bytes of x and no splitting arithmetic. K % 64 == 0; 16-byte aligned. */
int simpb_linear_f16in_split(float* y, const void* x_f16, const void* weight_hi, const void* weight_lo, const float* bias,
                             int M, int N, int K, void* stream);

/* ResNet stem in one launch: conv 7x7 / stride 2 / padding 3 (3 -> 64, BN folded) + bias + ReLU + max_pool 3x3 / stride 2 /
 * padding 1 = mmdet ResNet.forward's maxpool(relu(bn1(conv1(x)))) (config :79-99 after tools/fuse_conv_bn.py:10-48).
 *   img_nhwc4      f16 [num_images, height, width, 4]  RGB + a zero channel (simpb_image_to_nhwc4_f16 makes it)
 *   weight_packed  f16 [28][2][64][4]: entry [ky * 4 + g][kb][n][c] = weight[n][c][ky][2 g + kb] (0 for c = 3 or tap 7)
 *   bias f16 [64];  out f16 [num_images, Hp, Wp, 64] (NHWC), Hp = ((height + 6 - 7) / 2 + 1 + 2 - 3) / 2 + 1
 * Conv results are rounded to f16 before bias / ReLU / maximum (fp32), i.e. what a stored f16 conv map + the fused
 * epilogue (simpb_bias_relu_maxpool_nhwc_f16) give. out_channels must be 64. */
int simpb_stem_conv7x7_pool_f16(void* out, const void* img_nhwc4, const void* weight_packed, const void* bias,
                                int num_images, int height, int width, int out_channels, void* stream);

/* f32 image with arbitrary element strides [num_images, channels <= 3, height, width] -> f16 [N, H, W, 4], missing
 * channels zero: the cast + channels_last copy in front of the stem. */
int simpb_image_to_nhwc4_f16(void* out, const float* img, long long stride_n, long long stride_c, long long stride_h,
                             long long stride_w, int num_images, int channels, int height, int width, void* stream);

/* Camera frame ingest: raw u8 frames as an image decoder delivers them -> the stem's operand, in place of the reference's
 * host pipeline ResizeCropFlipImage (datasets/pipelines/augment.py:86-106: PIL.Image.resize(resize_dims).crop(crop), optional
 * left-right flip) + NormalizeMultiviewImage (transform_3d.py:438-466) and of simpb_image_to_nhwc4_f16 behind it.
 *   src  u8  [num_images, src_height, src_width, 3]  interleaved pixels
 *   out  f16 [num_images, out_height, out_width, 4]  channel 3 = 0 (what simpb_stem_conv7x7_pool_f16 reads); 16-byte aligned
 *   mid  u8  scratch of num_images * src_rows * simpb_preprocess_mid_pitch(out_width) bytes, 16-byte aligned: the
 *        horizontally resampled rows between the two launches
 * The resize is Pillow's 8-bit resampler (bicubic for RGB), byte for byte: per kept output column j of the RESIZED image
 * (the crop's columns only, left to right) xn[j] <= taps_x integer coefficients kx[j][0..] with 22 fractional bits over
 * source columns xlo[j].., and the same per kept output row (ky [out_height][taps_y], ylo, yn) over source ROWS; a pass
 * computes clamp((2^21 + sum(pixel * k)) >> 22, 0, 255), horizontally first, the result stored as u8, then vertically.
 * The tables are device pointers (int32) that the caller computes once per (source size, resize, crop), as Pillow's
 * precompute_coeffs does, in float64; 2^21 + 255 * sum|k| < 2^31 per row is the caller's to assert. src_row0 / src_rows:
 * the range of source rows the ylo / yn tables touch (min ylo, max (ylo + yn) - min ylo): only those rows are resampled
 * horizontally. flip: output column j reads kept column out_width - 1 - j. lut f16 [3][256]: out channel c =
 * lut[c][resampled byte of input channel (swap_rb ? 2 - c : c)], i.e. mean / std / channel order / rounding as a table.
 * SIMPB_EINVAL, and nothing launched: a null pointer, a non-positive size, src_width > 4096, out_width > 2048, a table
 * wider than SIMPB_PREPROCESS_MAX_TAPS, a row range outside [0, src_height), more than 65535 images or output rows. The
 * kernels clamp every table entry into the staged row / the row range, so a wrong table gives wrong pixels, never an
 * access outside src, mid or out. Two launches on `stream`; no allocation, no synchronisation (graph capture safe). */
#define SIMPB_PREPROCESS_MAX_TAPS 64
int simpb_preprocess_u8_nhwc4_f16(void* out, const void* src, void* mid, const int* kx, const int* xlo, const int* xn,
                                  const int* ky, const int* ylo, const int* yn, const void* lut, int num_images,
                                  int src_height, int src_width, int out_height, int out_width, int taps_x, int taps_y,
                                  int src_row0, int src_rows, int flip, int swap_rb, void* stream);

/* The same ingest for 4:2:0 semi-planar YCbCr frames (NV12 / NV21), what hardware video and JPEG decoders deliver: the
 * horizontal pass stages a luma row and its chroma row, converts them once to the (B, G, R) bytes the entry point above
 * stages, and goes on as above; `out` equals simpb_preprocess_u8_nhwc4_f16 on the converted frames bit for bit.
 *   src  u8  [num_images, src_height * 3 / 2, src_width]: src_height luma rows, then src_height / 2 rows of interleaved
 *        chroma pairs, (Cb, Cr) with vu_order = 0 (NV12) or (Cr, Cb) with vu_order = 1 (NV21). Row pitch = src_width.
 *        Chroma sample (i, j) belongs to luma rows 2i, 2i + 1 and columns 2j, 2j + 1 (replicated, not interpolated).
 * Conversion, int32 with 16 fractional bits (>> arithmetic, clamp to 0..255):
 *   c = iy * (Y - yoff) + 2^15
 *   R = clamp((c + irv * (Cr - 128)) >> 16)
 *   G = clamp((c + igu * (Cb - 128) + igv * (Cr - 128)) >> 16)
 *   B = clamp((c + ibu * (Cb - 128)) >> 16)
 * The coefficients are the caller's (simpb_amd/preprocess.py:yuv_coefficients: JFIF full range, BT.601 and BT.709 limited
 * range); that every partial sum stays inside int32 is the caller's to assert. Every other argument, the scratch and the
 * refusals are those of simpb_preprocess_u8_nhwc4_f16; SIMPB_EINVAL also for an odd src_height or src_width, a vu_order
 * outside {0, 1} and iy <= 0. Two launches on `stream`; no allocation, no synchronisation (graph capture safe). */
int simpb_preprocess_yuv420sp_nhwc4_f16(void* out, const void* src, void* mid, const int* kx, const int* xlo, const int* xn,
                                        const int* ky, const int* ylo, const int* yn, const void* lut, int num_images,
                                        int src_height, int src_width, int out_height, int out_width, int taps_x, int taps_y,
                                        int src_row0, int src_rows, int flip, int swap_rb, int vu_order, int yoff, int iy,
                                        int irv, int igu, int igv, int ibu, void* stream);

/* The same ingest for surfaces as a hardware decoder allocates them: padded row pitch, aligned plane height, the chroma
 * plane at its own offset and pitch, 10-bit samples, and one allocation per image. `out` equals the two entry points above
 * on the same pictures bit for bit (they pass the tight layout to the same kernel).
 *   format        SIMPB_SURFACE_BGR (rows of src_width * 3 bytes), _NV12 / _NV21 (u8, (Cb, Cr) / (Cr, Cb) pairs) or _P010
 *                 (semi-planar (Cb, Cr), u16 little-endian, sample = word >> 6: the low six bits are ignored)
 *   pitch         bytes from one luma (BGR) row to the next, >= the row's sample bytes (3, 1 or 2 per pixel)
 *   chroma_pitch  bytes from one chroma row to the next, >= src_width sample widths         } not looked at
 *   chroma_offset bytes from the image's first byte to chroma row 0, behind the last luma sample  } for _BGR
 *   The images, exactly one of the two non-NULL:
 *   src           a contiguous batch: image n starts at src + n * image_stride; image_stride >= the offset one past the
 *                 image's last sample
 *   image_table   device array of num_images 64-bit addresses, one per image, 8-byte aligned; image_stride is not looked
 *                 at. The kernel reads the table when it runs: a captured launch follows whatever addresses the table
 *                 holds at each replay. Each address must be readable up to the image's last sample (even for _P010).
 * Of a needed source row exactly the sample bytes are read: no byte between two rows, behind the last row, of a luma row
 * outside src_row0 .. src_row0 + src_rows - 1 or of a chroma row under no such row. A row that starts on a 16-byte
 * boundary is read in 16-byte chunks plus a bytewise tail, any other row bytewise; any pitch and base alignment is taken.
 * 10-bit conversion, the integers of the 8-bit rule with two more fractional bits (int32, >> arithmetic):
 *   c = iy * (Y10 - 4 * yoff) + 2^17
 *   R = clamp((c + irv * (Cr10 - 512)) >> 18)
 *   G = clamp((c + igu * (Cb10 - 512) + igv * (Cr10 - 512)) >> 18)
 *   B = clamp((c + ibu * (Cb10 - 512)) >> 18)
 * so that an 8-bit sample stored as v << 8 gives the 8-bit rule's byte. yoff .. ibu are not looked at for _BGR.
 * SIMPB_EINVAL, and nothing launched: whatever the entry points above refuse; both or neither of src / image_table; a
 * format outside the four; a pitch below the row's sample bytes (or above 2^30); a chroma plane that starts before the
 * luma plane ends; an odd pitch, chroma_pitch, chroma_offset, image_stride or src for _P010; with src, an image_stride
 * below the image's last sample. Two launches on `stream`; no allocation, no synchronisation (graph capture safe). */
#define SIMPB_SURFACE_BGR 0
#define SIMPB_SURFACE_NV12 1
#define SIMPB_SURFACE_NV21 2
#define SIMPB_SURFACE_P010 3
int simpb_preprocess_surface_nhwc4_f16(void* out, const void* src, const void* image_table, void* mid, const int* kx,
                                       const int* xlo, const int* xn, const int* ky, const int* ylo, const int* yn,
                                       const void* lut, int num_images, int src_height, int src_width, int out_height,
                                       int out_width, int taps_x, int taps_y, int src_row0, int src_rows, int flip, int swap_rb,
                                       int format, long long pitch, long long chroma_pitch, long long chroma_offset,
                                       long long image_stride, int yoff, int iy, int irv, int igu, int igv, int ibu,
                                       void* stream);

/* The same ingest for the frames of the other producers in a vehicle: a software decoder's planar 4:2:0, the packed 4:2:2 of
 * a camera that reaches the host without a codec, and the RGB-order and 4-byte pixels of loaders, ISPs and compositors. The
 * arguments are those of simpb_preprocess_surface_nhwc4_f16 plus chroma2_offset, and formats 0..3 ARE that entry point (the
 * same kernels, the same refusals, the same bits). The further formats:
 *   _YUV420P      three planes, u8: src_height luma rows at `pitch`, src_height / 2 Cb rows of src_width / 2 bytes at
 *                 chroma_offset + i * chroma_pitch, and as many Cr rows at chroma2_offset + i * chroma_pitch. I420 has the Cb
 *                 plane first in memory and YV12 the Cr plane: that is said by the two offsets alone. Even sizes.
 *   _YUYV / _UYVY one plane, rows of src_width / 2 groups (Y0, Cb, Y1, Cr) / (Cb, Y0, Cr, Y1), 2 bytes per pixel; the chroma
 *                 pair belongs to columns 2j, 2j + 1 of its own row. Even src_width, any src_height.
 *   _RGB          one plane, 3 bytes per pixel, R first
 *   _BGRA / _RGBA one plane, 4 bytes per pixel; byte 3 of a pixel is read and ignored
 * YCbCr samples are converted by the 8-bit rule of simpb_preprocess_yuv420sp_nhwc4_f16 (16 fractional bits, chroma replicated,
 * not interpolated); the RGB-order formats are a byte permutation into the (B, G, R) row, and yoff .. ibu are not looked at
 * for them. So `out` equals simpb_preprocess_u8_nhwc4_f16 on the converted / permuted frames bit for bit. chroma_pitch and
 * chroma_offset are not looked at for the one-plane formats, chroma2_offset for every format but _YUV420P. The promise about
 * the bytes read is that of the entry point above: of a needed row exactly its sample bytes (all four of a 4-byte pixel), no
 * chroma row under no needed luma row, 16-byte chunks only for a row that starts on a 16-byte boundary.
 * SIMPB_EINVAL, and nothing launched: whatever simpb_preprocess_surface_nhwc4_f16 refuses; a format outside {0..3, 8..13}; an
 * odd src_width for a YCbCr format, an odd src_height for _YUV420P; iy <= 0 for a YCbCr format; a pitch below the row's
 * sample bytes (src_width * 1, 2, 2, 3, 4, 4 in the order above), a chroma_pitch below src_width / 2; a chroma plane that
 * starts before the luma samples end; Cb and Cr planes that overlap; with src, an image_stride below the image's last
 * sample. Two launches on `stream`; no allocation, no synchronisation (graph capture safe).
 *
 * JPEG-DECODER PLANES. A JPEG's images reach the reference through libjpeg at its defaults, whose "fancy" upsampling
 * interpolates the subsampled chroma planes before the colour conversion. Two additions give that decoder's bytes to a caller
 * who hands over the file's own planes (or those of any decoder whose chroma is centre-sited):
 *   _YUV444P      three planes, u8, of src_height rows of src_width bytes: luma at `pitch`, Cb at chroma_offset + r *
 *                 chroma_pitch, Cr at chroma2_offset + r * chroma_pitch; every pixel has its own chroma sample. Any size. What a
 *                 4:4:4 JPEG decodes to. Refused like _YUV420P: a chroma_pitch below src_width, planes that overlap.
 *   format | SIMPB_SURFACE_CHROMA_JPEG, for _NV12, _NV21, _YUV420P, _YUYV and _UYVY: the same samples, the same layout rules
 *                 and the same colour rule, but every pixel gets its own interpolated Cb / Cr. C a chroma plane [Hc][Wc],
 *                 int32, j = x >> 1, l = max(j - 1, 0), r = min(j + 1, Wc - 1):
 *                 4:2:0 (libjpeg h2v2_fancy_upsample), luma row y, i = y >> 1:
 *                   near = C[i],  far = C[clamp(i + (y odd ? 1 : -1), 0, Hc - 1)],  s[k] = 3 * near[k] + far[k]
 *                   x even: (3 * s[j] + s[l] + 8) >> 4        x odd: (3 * s[j] + s[r] + 7) >> 4
 *                 4:2:2 (libjpeg h2v1_fancy_upsample), c the row's own chroma:
 *                   x even: (3 * c[j] + c[l] + 1) >> 2        x odd: (3 * c[j] + c[r] + 2) >> 2
 *                 The far row of 4:2:0 is read even where no needed luma row lies over it (exactly its sample bytes, like
 *                 every row). With libjpeg's own constants (yoff, iy, irv, igu, igv, ibu) = (0, 65536, 91881, -22554, -46802,
 *                 116130) -- its FIX(1.40200), FIX(0.34414), FIX(0.71414), FIX(1.77200), colour "jpeg" of
 *                 simpb_amd/preprocess.py -- the (B, G, R) row is the one libjpeg decodes from the same planes, byte for byte
 *                 (pinned to libjpeg-turbo through Pillow for 4:2:0, 4:4:4 and the constants; the 4:2:2 rule is stated from
 *                 libjpeg's published algorithm, which hands out no native 4:2:2 planes to pin it to).
 *   The flag is taken in `format` here, by simpb_preprocess_roll_nhwc4_f16 and in simpb_rig_camera.format (a rig may mix
 *   cameras with and without it). SIMPB_EINVAL, and nothing launched or written: the flag on a format without subsampled 8-bit
 *   chroma (_BGR, _RGB, _BGRA, _RGBA, _P010, _YUV444P), any other bit above the codes, codes 4..7, 14, 15 and negative ones.
 *   simpb_preprocess_surface_nhwc4_f16 takes codes 0..3 and no flag. */
#define SIMPB_SURFACE_YUV420P 8
#define SIMPB_SURFACE_YUYV 9
#define SIMPB_SURFACE_UYVY 10
#define SIMPB_SURFACE_RGB 11
#define SIMPB_SURFACE_BGRA 12
#define SIMPB_SURFACE_RGBA 13
#define SIMPB_SURFACE_YUV444P 16
#define SIMPB_SURFACE_CHROMA_JPEG 0x100
int simpb_preprocess_planes_nhwc4_f16(void* out, const void* src, const void* image_table, void* mid, const int* kx,
                                      const int* xlo, const int* xn, const int* ky, const int* ylo, const int* yn,
                                      const void* lut, int num_images, int src_height, int src_width, int out_height,
                                      int out_width, int taps_x, int taps_y, int src_row0, int src_rows, int flip, int swap_rb,
                                      int format, long long pitch, long long chroma_pitch, long long chroma_offset,
                                      long long chroma2_offset, long long image_stride, int yoff, int iy, int irv, int igu,
                                      int igv, int ibu, void* stream);

/* Bytes of one row of the `mid` scratch above (whole groups of 4 pixels, rounded up to 16); 0 for a width outside 1..2048. */
int simpb_preprocess_mid_pitch(int out_width);

/* The same ingest for a RIG of cameras that differ: each camera has its own source size, format, surface layout, resize,
 * crop and flip, and all of them give one output size. Image n belongs to camera n % num_cams (images in (stream, camera)
 * order, num_images a multiple of num_cams). Two launches for the whole rig, whatever its cameras are; each output block
 * equals simpb_preprocess_planes_nhwc4_f16 of that camera alone bit for bit.
 *   simpb_rig_camera  one camera: format .. chroma_offset, chroma2_offset, src_row0 .. flip and yoff .. ibu mean what the
 *                 arguments of that name mean above (any of the ten formats; a field a format does not look at is not looked
 *                 at here), for this camera's images.
 *     kx_offset   ints from `kx` to this camera's [out_width][taps_x] coefficients;  x_offset: entries from `xlo` / `xn` to
 *                 its out_width entries;  ky_offset / y_offset: the same for [out_height][taps_y] and out_height
 *     mid_row     the camera's first row inside one stream's block of the intermediate (it takes src_rows rows)
 *   cams          HOST array of num_cams <= SIMPB_RIG_MAX_CAMS descriptors. They travel to the kernels by value: a captured
 *                 launch keeps the rig it was captured with, and only image_table is read at replay.
 *   kx, xlo, xn, ky, ylo, yn   device int32 arrays of kx_len, x_len, x_len, ky_len, y_len, y_len entries: the cameras'
 *                 tables, concatenated;  lut: one table for all cameras
 *   mid           scratch of (num_images / num_cams) * mid_rows * simpb_preprocess_mid_pitch(out_width) bytes, 16-byte aligned
 *   image_table   device array of num_images 64-bit addresses (8-byte aligned), read when the kernels run. An address of 0
 *                 skips that image: none of its source bytes is read and its output block is written as f16 zeros (a paused
 *                 stream, a camera that delivered nothing); every other image is unaffected.
 * The horizontal grid spans the largest src_rows of the rig; a workgroup past its camera's rows leaves at once. Its LDS is
 * sized for the rig's widest cameras, not for the widest source this file takes: at most 34832 bytes, reached by a 4096-wide
 * _P010 camera (two planes of 8192 bytes) and equally by a 4096-wide _BGRA / _RGBA one (its row of 16384 bytes is staged
 * before it is compacted), each beside the 12288-byte (B, G, R) row and the 6160-byte resampled row; a camera of interpolated
 * 4:2:0 chroma (SIMPB_SURFACE_CHROMA_JPEG) adds the far chroma row of the widest such camera, at most 4096 bytes more.
 * SIMPB_EINVAL, and nothing launched or written: num_cams outside 1..16; num_images no multiple of num_cams; for any camera,
 * whatever simpb_preprocess_planes_nhwc4_f16 refuses in its address-table form; a table range or an intermediate range
 * that leaves its array or overlaps another camera's. Two launches on `stream`; no allocation, no synchronisation. */
#define SIMPB_RIG_MAX_CAMS 16
typedef struct simpb_rig_camera {
  int format, src_height, src_width;
  int src_row0, src_rows, taps_x, taps_y, flip;
  long long pitch, chroma_pitch, chroma_offset;
  int kx_offset, x_offset, ky_offset, y_offset, mid_row;
  int yoff, iy, irv, igu, igv, ibu;
  long long chroma2_offset;
} simpb_rig_camera;
int simpb_preprocess_rig_nhwc4_f16(void* out, const void* image_table, void* mid, const int* kx, const int* xlo, const int* xn,
                                   const int* ky, const int* ylo, const int* yn, const void* lut, const simpb_rig_camera* cams,
                                   int num_cams, int num_images, int out_height, int out_width, int kx_len, int x_len, int ky_len,
                                   int y_len, int mid_rows, int swap_rb, void* stream);

/* The same ingest for cameras with a MOUNT ROLL: the fourth step of the reference's ResizeCropFlipImage._img_transform,
 * PIL.Image.rotate(r) with its defaults (augment.py:92,105), behind resize, crop and flip: a nearest-neighbour inverse affine
 * map in 16.16 fixed point about the image centre. The caller reduces a camera's roll to six integers a0 .. a5
 * (simpb_amd/preprocess.py:roll_integers restates Pillow's rule, its transposes for 180 and square 90 / 270 degrees included);
 * the kernels know the six integers and nothing else. With L the h x w image the entry points above compute BEFORE the table
 * (L[y][x][c], a byte), output pixel (x, y) is
 *   xin = (a2 + y * a1 + x * a0) >> 16,  yin = (a5 + y * a4 + x * a3) >> 16          (64-bit, arithmetic shift)
 *   out[y][x][c] = lut[c][L[yin][xin][swap_rb ? 2 - c : c]]  where 0 <= xin < out_width and 0 <= yin < out_height,
 *   out[y][x][c] = lut[c][0] (black, normalised) elsewhere;  out[y][x][3] = 0.
 * The row (65536, 0, 32768, 0, 65536, 32768) is the identity and gives the level entry point's bits.
 * The roll is a gather inside the vertical pass: the horizontal pass, `mid` and the row range src_row0 / src_rows are the
 * level path's own (a roll maps rows of the cropped image onto rows of the cropped image); still two launches and one
 * intermediate. The range test on (xin, yin) comes first and every index behind it is clamped as in the level pass: a wrong
 * table gives wrong pixels, never an access outside mid, ky, ylo or yn.
 *
 * simpb_preprocess_roll_nhwc4_f16: the arguments of simpb_preprocess_planes_nhwc4_f16 (every format, tight or padded, a
 * contiguous batch or an address table), then
 *   roll       HOST int32 [roll_cams][6], read before the call returns and handed to the kernel by value
 *   roll_cams  1 .. SIMPB_RIG_MAX_CAMS: image n takes row n % roll_cams (1: one roll for all images)
 * simpb_preprocess_rig_roll_nhwc4_f16: the arguments of simpb_preprocess_rig_nhwc4_f16, then roll HOST int32 [num_cams][6]:
 * camera c takes row c; a level camera of a mixed rig takes the identity row; a skipped image (address 0) stays f16 zeros.
 * SIMPB_EINVAL, and nothing launched or written: whatever the level form refuses; a null roll; roll_cams outside 1..16; an
 * out_height or out_width above SIMPB_PREPROCESS_MAX_ROLL_SIZE (Pillow leaves its fixed-point path where a corner coordinate
 * reaches 32768; below this size that cannot happen). Two launches on `stream`; no allocation, no synchronisation (graph
 * capture safe). The 2D records (simpb_decode2d_record*) do not change: the reference's decode_box2d does not look at rotate. */
#define SIMPB_PREPROCESS_MAX_ROLL_SIZE 8192
int simpb_preprocess_roll_nhwc4_f16(void* out, const void* src, const void* image_table, void* mid, const int* kx,
                                    const int* xlo, const int* xn, const int* ky, const int* ylo, const int* yn, const void* lut,
                                    int num_images, int src_height, int src_width, int out_height, int out_width, int taps_x,
                                    int taps_y, int src_row0, int src_rows, int flip, int swap_rb, int format, long long pitch,
                                    long long chroma_pitch, long long chroma_offset, long long chroma2_offset,
                                    long long image_stride, int yoff, int iy, int irv, int igu, int igv, int ibu, const int* roll,
                                    int roll_cams, void* stream);
int simpb_preprocess_rig_roll_nhwc4_f16(void* out, const void* image_table, void* mid, const int* kx, const int* xlo,
                                        const int* xn, const int* ky, const int* ylo, const int* yn, const void* lut,
                                        const simpb_rig_camera* cams, int num_cams, int num_images, int out_height, int out_width,
                                        int kx_len, int x_len, int ky_len, int y_len, int mid_rows, int swap_rb, const int* roll,
                                        void* stream);

/* Grouped small GEMM of the decoder: up to 4 independent problems per launch, each
 *   y[M, 0:N] (row stride ldy) = relu?( [x0 | x1 | ...][M, K] . w[N, K]^T (row stride ldw) + bias[N] )
 * where x is given as up to 4 column segments (pointer, row stride, width; widths sum to K). This is
 * how the reference's `torch.cat([feature, pos_embed], -1)` in front of every attention projection
 * (models/simpb_head.py:298-321), the `identity + out` branches followed by fc_after (:306-310) and
 * the identity_fc branch of AsymmetricFFN (models/blocks.py:384-393) become one product each, with
 * host-folded weights, instead of a concatenation, two vendor GEMMs and an add. Exact fp32
 * (v_mfma_f32_32x32x2_f32). Every segment width and K are multiples of 64; x, w 16-byte aligned,
 * row strides multiples of 4. m_live (device int, may be NULL): rows >= *m_live are capacity slots of the
 * static 2D query set and are written as zeros. Deterministic. */
#define SIMPB_GEMM_MAX_SEGS 4
#define SIMPB_GEMM_MAX_JOBS 4
#define SIMPB_GEMM_OUT_F32 0
#define SIMPB_GEMM_OUT_SPLIT_HALFS 1
typedef struct simpb_gemm_job {
  const float* x[SIMPB_GEMM_MAX_SEGS];
  int ldx[SIMPB_GEMM_MAX_SEGS];
  int kseg[SIMPB_GEMM_MAX_SEGS];
  int num_seg;
  int M, N, K;
  const float* w;
  const float* bias;
  float* y;
  const int* m_live;
  int ldw, ldy, relu;
  /* SIMPB_GEMM_OUT_F32 (0): y holds fp32 numbers. SIMPB_GEMM_OUT_SPLIT_HALFS (1): every element is written as the two halfs
   * the split-operand attention kernel multiplies (simpb_attention_split_halfs): low 16 bits half(v), high 16 bits
   * half((v - half(v)) * 2^11), in the element's own 32-bit word (ldy unchanged). Needs |v| < 65504. */
  int out_fmt;
  /* optional rank-1 term before the ReLU: rows with row_flag[row] != 0 also get bias2[col]. This is
   * the 257th input column of ReWeight.reduce (models/aggregation.py:19-21,71-72: Linear over
   * cat(query2d, is_center)) without materialising the concatenation. Both NULL = absent. */
  const int* row_flag;
  const float* bias2;
  /* optional pre-split weights, f16 [N, K] with dense rows: w_hi = half(w), w_lo = half((w - w_hi) * 2048). When every
   * job of a launch brings them (and its segment widths are multiples of 128) the products run on the FP16 matrix
   * cores in three passes at fp32-grade accuracy (see simpb_linear_f16x3); `w` stays the reference copy. Any finite x:
   * a row whose largest |x| is outside [2^-10, 2^15) is split as x * 2^-e and the sum scaled by 2^e before the bias (exact;
   * fp32 denormal rows may be flushed). Weights: the caller passes a split only when every row's largest |w| is in that
   * window or zero (plugin/dense.py split_in_window). Both NULL = exact fp32 path. */
  const void* w_hi;
  const void* w_lo;
} simpb_gemm_job;
typedef struct simpb_gemm_args {
  int num_jobs;
  int reserved;
  simpb_gemm_job job[SIMPB_GEMM_MAX_JOBS];
} simpb_gemm_args;
int simpb_gemm_f32(const simpb_gemm_args* args, void* stream);

/* out[M, 0:k0+k1] (row stride ldo) = LayerNorm([x0 | x1]) * gamma + beta over the concatenated width
 * (torch.nn.LayerNorm: eps 1e-5, biased variance); x1 may be NULL with k1 = 0. Width <= 512. The two
 * segments are the `cat` of residual_mode="cat" (models/blocks.py:158-161, group_attn.py:252-255) in front
 * of the FFN's pre_norm (blocks.py:385-386), and one segment is every `norm` op of the decoder.
 * m_live as in simpb_gemm_f32. out may alias x0 when k1 == 0. */
int simpb_layernorm_f32(float* out, int ldo, const float* x0, int ld0, int k0, const float* x1, int ld1, int k1,
                        const float* gamma, const float* beta, int num_rows, const int* m_live, void* stream);

/* Forward direction of feature_maps_format (ops/__init__.py:63-92) in one pass. Level l is
 * [num_images = bs*cams, H_l, W_l, channels] in memory (what a channels_last backbone emits), f16
 * (src_is_half) or f32; level_ptrs/level_hw are HOST arrays of num_levels device pointers / H_l*W_l.
 * col_feats f32 [bs, cams * sum_l H_l*W_l, channels], camera-major then level then row-major, as
 * ops/src/deformable_aggregation.cpp:22-28 expects. channels % 8 == 0. level_bias (HOST array of num_levels device
 * pointers, or NULL; entries may be NULL): per-channel bias of the same dtype added on the way (the last FPN
 * convolution then runs without its bias: mmdet FPN.fpn_convs, config :90-99); f16 sums are rounded to f16 first,
 * so the tokens are the numbers the separate bias pass produced. */
#define SIMPB_MAX_LEVELS 8
int simpb_format_tokens(float* col_feats, const void* const* level_ptrs, const void* const* level_bias,
                        const int* level_hw, int num_levels, int num_images, int channels, int src_is_half, void* stream);

/* Backbone convolution epilogue after conv-BN folding (tools/fuse_conv_bn.py:10-48): in place,
 * y f16 [num_pixels, channels] (NHWC) = relu?(y + bias[c] + residual?). bias f16 [channels]; residual f16
 * like y or NULL; channels % 8 == 0; all pointers 16-byte aligned. */
int simpb_bias_act_nhwc_f16(void* y, const void* bias, const void* residual, long long num_pixels, int channels,
                            int relu, void* stream);

/* Stem epilogue of the BN-folded ResNet (mmdet ResNet.forward: conv1 -> bn1 -> relu -> maxpool(3, stride 2, padding 1)):
 *   y[n, oy, ox, c] = relu( max over the window of x[n, 2*oy-1+dy, 2*ox-1+dx, c] + bias[c] ),  dy, dx in 0..2 (inside the map)
 * x f16 [num_images, in_h, in_w, channels] = the raw output of the 7x7 convolution (NHWC), y f16 [num_images, ho, wo, channels],
 * ho = (in_h - 1) / 2 + 1. Bias and ReLU commute with the maximum, so this equals the bias/ReLU pass followed by the pooling
 * kernel bit for bit, in one pass. channels % 8 == 0; 16-byte aligned. */
int simpb_bias_relu_maxpool_nhwc_f16(void* y, const void* x, const void* bias, int num_images, int in_h, int in_w,
                                     int channels, void* stream);

/* A whole BN-folded 1x1 convolution of the fp16 channels_last backbone in one launch:
 *   y[n, ho, wo, :] = relu?( x[n, ho*stride, wo*stride, :] . weight^T + bias (+ residual[n, ho, wo, :]) )
 * x f16 [num_images, in_h, in_w, in_channels] (NHWC), weight f16 [out_channels, in_channels], bias f16 [out_channels],
 * residual f16 like y or NULL (with residual_upsample2x: f16 [num_images, ho / 2, wo / 2, out_channels], read with
 * nearest-neighbour 2x upsampling = the FPN top-down sum lateral[i-1] += interpolate(lateral[i]) of mmdet FPN.forward;
 * ho, wo even), y f16 [num_images, ho, wo, out_channels] with ho = (in_h - 1) / stride + 1; input_bias f16
 * [in_channels] or NULL: x is first replaced by relu(x + input_bias) (rounded to f16), i.e. the epilogue of the
 * BN-folded 3x3 convolution that produced x (bottleneck conv2 -> conv3) without a pass of its own; fp32
 * accumulate. stride 1 or 2; in_channels % 64 == 0, out_channels % 8 == 0; 16-byte aligned. These are conv1 / conv3 /
 * downsample of every ResNet bottleneck and the FPN lateral convolutions (mmdet ResNet + FPN of
 * projects/configs/simpb_nus_r50_img_704x256.py:79-99 after tools/fuse_conv_bn.py:10-48). variant 0 = choose the kernel
 * from the shape; 1 = the round-1 kernel (single LDS stage; the only one that takes input_bias); 2 / 3 / 4 = 128 x 64 /
 * 128 x 128 / 64 x 64 tiles of the staged pipeline of simpb_conv3x3_nhwc_f16 (same sums up to fp32 summation order; 2 - 4
 * give the same bits as each other). */
int simpb_conv1x1_nhwc_f16(void* y, const void* x, const void* weight, const void* bias, const void* residual,
                           int num_images, int in_h, int in_w, int in_channels, int out_channels, int stride, int relu,
                           int residual_upsample2x, const void* input_bias, int variant, void* stream);

/* A whole BN-folded 3x3 convolution (padding 1) of the fp16 channels_last backbone in one launch, as an implicit GEMM:
 *   out[n, ho, wo, :] = relu?( sum_{dy,dx} x[n, ho*stride + dy - 1, wo*stride + dx - 1, :] . weight[:, dy, dx, :]^T + bias )
 * x f16 [num_images, in_h, in_w, in_channels] (NHWC), weight f16 [out_channels, 3, 3, in_channels] (what PyTorch keeps for a
 * channels_last Conv2d weight), bias f16 [out_channels]; fp32 accumulate, one rounding to f16. Exactly one destination:
 *   y      f16 [num_images, ho, wo, out_channels], ho = (in_h - 1) / stride + 1, or
 *   tokens f32: the decoder's token buffer col_feats [bs, cams * tokens_per_cam, out_channels] of feature_maps_format
 *          (projects/mmdet3d_plugin/ops/__init__.py:63-92); image n is camera block n, this level's pixels start at row
 *          level_start of the block; the value written is the f16 result widened to f32 (what a separate format pass over
 *          the f16 map would write): the FPN's output convolutions produce the tokens themselves. tokens_f16 (f16, same
 *          layout, or NULL): the same rows without the widening, for the samplers and simpb_linear_f16in_split
 *          (value_proj). tokens == NULL with tokens_f16 set: the f16 rows ALONE -- kernels without the fp32 conversions
 *          and stores (what a replayed frame runs: every reader of the tokens takes f16 rows). Exactly one of y and the
 *          token form; all three NULL is SIMPB_EINVAL.
 * These are conv2 of every ResNet bottleneck and FPN.fpn_convs (mmdet ResNet + FPN of
 * projects/configs/simpb_nus_r50_img_704x256.py:79-99 after tools/fuse_conv_bn.py:10-48). stride 1 or 2;
 * in_channels % 64 == 0, out_channels % 8 == 0; 16-byte aligned. variant 0 = choose the tiling from the shape; 1-13 force one
 * (pixels x channels per workgroup: 1 = 128 x 64 and 2 = 256 x 64 with the activations read straight into the MFMA layout;
 * 3 = 32 x 64 and 4 = 64 x 64 with K split over the workgroup's waves; 5 = 128 x 64, 6 = 128 x 128, 7 = 96 x 64,
 * 8 = 96 x 128 and 9 = 64 x 64 with both operands staged through LDS; 10 / 11 = 64 x 64 staged with K split over 2 / 4
 * groups of four waves, the partial sums added in group order) -- all give the same sums up to fp32 summation order, each
 * in a fixed order; 9 adds in the order of 1 and 2, 11 in the order of 3 and 4: the same bits.
 * 12 / 13 = the resident form: a workgroup keeps its 2-D tile of input pixels with the one-pixel halo, all in_channels, in
 * LDS and reads the nine taps as addresses into it (rows x columns of output pixels x channels: 12 = 4 x 16 x 64 with four
 * waves, 13 = 8 x 16 x 128 with eight); stride 1 and in_channels 64, 128 or 256 only, SIMPB_EINVAL otherwise. They add in the
 * order of 5-8: the same bits. */
int simpb_conv3x3_nhwc_f16(void* y, float* tokens, void* tokens_f16, int tokens_per_cam, int level_start, const void* x,
                           const void* weight, const void* bias, int num_images, int in_h, int in_w, int in_channels,
                           int out_channels, int stride, int relu, int variant, void* stream);

/* The tiling (1-11) that simpb_conv3x3_nhwc_f16 runs under variant 0 for p_out = num_images * out_h * out_w output pixels
 * (where the answer is 7 or 8, variant 0 then asks simpb_conv3x3_choose_resident below).
 * A pure function of its arguments: nothing is launched and no device is needed. */
int simpb_conv3x3_choose_variant(long long p_out, int in_channels, int out_channels);

/* Where simpb_conv3x3_choose_variant answers 7 or 8, variant 0 asks this second rule whether the resident form measured
 * faster on the shape: the resident variant (12 or 13) it then runs instead, or 0 for "stay". 0 as well wherever the first
 * rule answers anything else, for stride 2, for in_channels other than 64, 128, 256 and for out_channels != in_channels
 * (nothing else was measured). A pure function of its arguments. */
int simpb_conv3x3_choose_resident(long long p_out, int in_h, int in_w, int in_channels, int out_channels, int stride);

/* The same for simpb_conv3x3_group_tokens_f16, asked once for the whole launch: 13 = every level runs the resident
 * 8 x 16 x 128 form, 0 = every level runs the staged 96 x 128 tiles. */
int simpb_conv3x3_group_choose_resident(int num_levels, int num_images, const int* in_h, const int* in_w, int in_channels,
                                        int out_channels);

/* The same 3x3 / stride 1 convolution for up to four inputs of one channel count in ONE launch, each result written as its
 * level's token rows (f32 `tokens`, and f16 `tokens_f16` or NULL; or tokens == NULL and the f16 rows alone) exactly as
 * simpb_conv3x3_nhwc_f16 does with `tokens`:
 * the four `fpn_convs[i].conv` of mmdet's FPN (projects/configs/simpb_nus_r50_img_704x256.py:92-99) behind
 * feature_maps_format (ops/__init__.py:63-92). x[j] f16 NHWC [num_images, in_h[j], in_w[j], Cin]; weight[j] f16
 * [Cout, 3, 3, Cin]; bias[j] f16 [Cout]; level_start[j] = the level's first row inside a camera's tokens_per_cam rows.
 * One tile form for every level (simpb_conv3x3_group_choose_resident: 96 x 128 staged tiles, tiling 8 above, or the resident
 * tiling 13): the small levels' tiles fill the last round of the large one. */
int simpb_conv3x3_group_tokens_f16(int num_levels, float* tokens, void* tokens_f16, int tokens_per_cam, const int* level_start,
                                   const void* const* x, const void* const* weight, const void* const* bias, int num_images,
                                   const int* in_h, const int* in_w, int in_channels, int out_channels, int relu, void* stream);

/* The same with the form of every level given: variant[j] = 8 (the 96 x 128 staged tiles) or 13 (the resident 8 x 16 x 128
 * tiles; in_channels 64, 128 or 256); variant == NULL is what simpb_conv3x3_group_tokens_f16 runs. The levels of one form
 * share a launch, so mixed forms are two launches; the rows are the same bits whatever the forms. */
int simpb_conv3x3_group_tokens_forms_f16(int num_levels, float* tokens, void* tokens_f16, int tokens_per_cam,
                                         const int* level_start, const void* const* x, const void* const* weight,
                                         const void* const* bias, int num_images, const int* in_h, const int* in_w,
                                         int in_channels, int out_channels, int relu, const int* variant, void* stream);

/* ---- The backbone convolutions over the LIVE images of a batch only --------------------------------------------------------
 * A live-image table is a device array `live`, i32 [1 + num_images]: live[0] = L, the number of live images, and live[1 .. L]
 * their indices in strictly ascending order; what lies behind entry L is not read. The host builds it (runner.live_images).
 * Each entry point below is the one it is named after with one trailing argument, `const int* live`:
 *   live == NULL  the launch of the entry point without the suffix, the same kernels, unchanged (those entry points ARE
 *                 calls of these with NULL).
 *   live != NULL  the convolution of the live images alone, by kernels of their own that walk L * out_h * out_w virtual
 *                 pixels (csrc/conv_parts.h has the mapping): tiled and dealt over the XCDs as the full batch is, so the work
 *                 that remains fills the whole chip. The grid is sized for the full batch and the tile counts are made from
 *                 L in the kernel; a workgroup past the live total returns before its first load.
 * The contract:
 *   - The rows of a live image -- in y, tokens or tokens_f16 -- are BIT FOR BIT what the entry point without the suffix
 *     writes for that image on the full batch under the same `variant`: every form adds an output pixel's products in a
 *     fixed order that does not depend on which tile holds the pixel. variant 0 is still resolved from the FULL-batch shape
 *     (num_images), on the host.
 *   - No byte of a dead image's output rows is written, and none of its input, residual or source rows is read: they hold
 *     afterwards what they held before, and may hold anything (NaN, stale frames) beforehand.
 *   - L is clamped to 0 .. num_images and every index to 0 .. num_images - 1 inside the kernels: a wrong table gives wrong
 *     pixels, never an access outside the arrays (the rule of the ingest tables above).
 *   - L = 0 launches and writes nothing.
 *   - SIMPB_EINVAL exactly where the entry point without the suffix returns it; `live` itself is not validated on the host
 *     (it is a device pointer), 4-byte alignment is the caller's. */
int simpb_stem_conv7x7_pool_f16_live(void* out, const void* img_nhwc4, const void* weight_packed, const void* bias,
                                     int num_images, int height, int width, int out_channels, void* stream, const int* live);
int simpb_conv1x1_nhwc_f16_live(void* y, const void* x, const void* weight, const void* bias, const void* residual,
                                int num_images, int in_h, int in_w, int in_channels, int out_channels, int stride, int relu,
                                int residual_upsample2x, const void* input_bias, int variant, void* stream, const int* live);
int simpb_conv3x3_nhwc_f16_live(void* y, float* tokens, void* tokens_f16, int tokens_per_cam, int level_start, const void* x,
                                const void* weight, const void* bias, int num_images, int in_h, int in_w, int in_channels,
                                int out_channels, int stride, int relu, int variant, void* stream, const int* live);
int simpb_conv3x3_group_tokens_forms_f16_live(int num_levels, float* tokens, void* tokens_f16, int tokens_per_cam,
                                              const int* level_start, const void* const* x, const void* const* weight,
                                              const void* const* bias, int num_images, const int* in_h, const int* in_w,
                                              int in_channels, int out_channels, int relu, const int* variant, void* stream,
                                              const int* live);

/* Attention core of torch.nn.MultiheadAttention (between in_proj and out_proj), exact fp32, flash
 * style, head_dim = 64: out[b,q,h*64+d] = sum_k softmax_k(scale * Q[b,q,h,:].K[b,k,h,:]) V[b,k,h,d].
 * q/k/v/out are [batch, N, heads*64] with row strides ldq/ldk/ldv/ldo (floats; batches are N*ld apart),
 * so slices of a fused projection buffer can be passed as they are. q and k 16-byte aligned.
 * Camera-grouped form (both tables non-NULL, num_key == num_query): slot q only attends slots of its
 * own group: query_cam i32 [N] (-1 = slot outside every group -> zeros), group_start i32 [cams+1];
 * this equals the reference's additive -inf block mask + nan_to_num (models/group_attn.py:104-131). */
int simpb_attention_f32(float* out, const float* q, const float* k, const float* v, const int* query_cam,
                        const int* group_start, int batch_size, int num_heads, int head_dim, int num_query,
                        int num_key, int ldq, int ldk, int ldv, int ldo, float scale, void* stream);

/* The same operator (same arguments, same layouts, fp32 in and out) on the FP16 matrix cores with split operands:
 * every fp32 operand is carried as two halfs (x = xh + xl / 2^11, 22 bits), partial products are exact in fp32
 * accumulators (csrc/attention.hip attention_f16s_kernel; fp32-grade: tests/test_gpu_ops.py holds it to the exact
 * kernel's bound against float64). What a frame runs since round 4 (plugin/routes.py attention_split_fp16); operands
 * must be inside the half-precision range (|x| < 65504: the decoder's projected queries / keys / values are O(10)). */
int simpb_attention_f32_split(float* out, const float* q, const float* k, const float* v, const int* query_cam,
                              const int* group_start, int batch_size, int num_heads, int head_dim, int num_query,
                              int num_key, int ldq, int ldk, int ldv, int ldo, float scale, void* stream);

/* ... and on operands the producing GEMM already left split (simpb_gemm_job.out_fmt = SIMPB_GEMM_OUT_SPLIT_HALFS): every
 * element of q / k / v is a 32-bit word holding half(x) in its low and half((x - half(x)) * 2^11) in its high 16 bits, at
 * the position (same strides ldq / ldk / ldv, counted in 32-bit words) the fp32 element would have. The softmax scale is
 * NOT applied here: the producer folds it into the query rows (1 / sqrt(64) is a power of two, so that is exact). */
int simpb_attention_split_halfs(float* out, const void* q, const void* k, const void* v, const int* query_cam,
                                const int* group_start, int batch_size, int num_heads, int head_dim, int num_query,
                                int num_key, int ldq, int ldk, int ldv, int ldo, void* stream);

/* The ungrouped operator with one of TWO key / value sets per batch row: row b reads (k, v, num_key, ldk, ldv) where
 * select[b] == 0 and (k2, v2, num_key2, ldk2, ldv2) otherwise (select u8 [batch_size] on the device; batches of set 2 are
 * num_key2 * ld apart). split = 0 / 1 / 2 names the form: simpb_attention_f32, simpb_attention_f32_split,
 * simpb_attention_split_halfs (which ignores scale). A row's output is bit for bit what that entry point gives on the set
 * the row selected, and not a byte of the other set is read: it may hold anything. select == NULL: set 1 for every row
 * through that entry point's own kernel (k2 / v2 are not looked at). With a selector, k2 and v2 must be given and obey the
 * rules of k and v (k2 16-byte aligned, ldk2 % 4 == 0, ld >= num_heads * 64). */
int simpb_attention_select(int split, float* out, const void* q, const void* k, const void* v, const void* k2, const void* v2,
                           const unsigned char* select, int batch_size, int num_heads, int head_dim, int num_query,
                           int num_key, int num_key2, int ldq, int ldk, int ldv, int ldk2, int ldv2, int ldo, float scale,
                           void* stream);

/* Fused small-MLP chains: a whole `linear_relu_ln` stack (models/blocks.py:32-43) -- [Linear, ReLU]*,
 * LayerNorm, ..., optional last Linear and Scale -- in one launch; up to 8 independent chains over
 * the same rows share it (e.g. the pos/size/yaw/vel branches of SparseBox3DEncoder,
 * models/detection3d/blocks.py:57-74). The argument block is a plain host struct of device
 * pointers and sizes. Every width <= 256.
 *   op LINEAR:    w = weight, f32 [out_dim, in_dim] (or transposed, see weights_transposed); b = bias [out_dim] or NULL; relu 0/1
 *   op LAYERNORM: w = gamma, b = beta, f32 [in_dim]; eps 1e-5
 *   chain input:  IN_ROWS    x f32 rows of in_dim values, row stride ldx (floats); optional second
 *                            addend x2 (row stride ldx2): input = x + x2
 *                 IN_SINE2D  x f32 rows holding (x, y) in [0,1] at columns 0,1; the 256-d sine embedding
 *                            of models/utils.py:40-63 (cat(pos_y, pos_x)) is computed in the kernel
 *                 IN_ROWS_LN input = LayerNorm(x) * ln_w + ln_b (eps 1e-5) + x2: the decoder's `norm` operator in front of
 *                            a refinement head (models/simpb_head.py operation_order "norm", "refine*") inside the head's
 *                            launch; ln_out (row stride ld_ln_out, may be NULL) receives LayerNorm(x), the operator's
 *                            own output (rows >= *m_live as zeros). 4-row / 32-row kernels (weights_transposed == 2, 3) only.
 *                            With out == NULL, n_ops == 0 and ln_out set the job is that stage ALONE (the operator in front
 *                            of a head whose outputs nothing reads): the same prologue code, so ln_out is bit-equal to what
 *                            the job with its chain behind it writes. out == NULL in any other form is SIMPB_EINVAL.
 *   chain output: out rows of the last width, row stride ldo; out_scale (or NULL) multiplies column-wise
 *                 (mmcv Scale after the last Linear); then the optional `post` stage on v = out[row, t]:
 *     POST_REFINE3D  SparseBox3DRefinementModule.forward (models/detection3d/blocks.py:133-143):
 *                    v = (t >= div_col0 ? v / div[row / div_rows] : v) + res[row, t]   (res = anchor, ldres)
 *     POST_REFINE2D  SparseBox2DRefinementModule.forward (models/detection2d/blocks.py:122-125, 144):
 *                    v = sigmoid(v + (t < res_cols ? inverse_sigmoid(res[row, t]) : 0))   (res = anchor2d;
 *                    inverse_sigmoid of models/utils.py:4-8, eps 1e-5)
 *     POST_SIGMOID   v = sigmoid(v)   (ReWeight.alpha, models/aggregation.py:23-24) */
#define SIMPB_MLP_MAX_OPS 12
#define SIMPB_MLP_MAX_CHAINS 8
#define SIMPB_MLP_POST_NONE 0
#define SIMPB_MLP_POST_REFINE3D 1
#define SIMPB_MLP_POST_REFINE2D 2
#define SIMPB_MLP_POST_SIGMOID 3
#define SIMPB_MLP_LINEAR 0
#define SIMPB_MLP_LAYERNORM 1
#define SIMPB_MLP_IN_ROWS 0
#define SIMPB_MLP_IN_SINE2D 1
#define SIMPB_MLP_IN_ROWS_LN 2
typedef struct simpb_mlp_op {
  int type, in_dim, out_dim, relu;
  const float* w;
  const float* b;
} simpb_mlp_op;
typedef struct simpb_mlp_chain {
  const float* x;
  const float* x2;
  float* out;
  const float* out_scale;
  int ldx, ldx2, ldo, in_dim, in_mode, n_ops;
  int post, ldres, res_cols, div_rows, div_col0, reserved;
  const float* res;
  const float* div;
  simpb_mlp_op ops[SIMPB_MLP_MAX_OPS];
  const float* ln_w;   /* IN_ROWS_LN: gamma, beta f32 [in_dim] */
  const float* ln_b;
  float* ln_out;
  int ld_ln_out, reserved2;
} simpb_mlp_chain;
typedef struct simpb_mlp_args {
  int num_rows, num_chains;
  int weights_transposed;  /* 0: LINEAR.w is nn.Linear's [out_dim, in_dim] (16-row MFMA kernel); 1: [in_dim, out_dim] (VALU
                            * kernel); 2: k4-packed [in_dim / 4][out_dim][4] for layers with in_dim % 4 == 0, nn.Linear's
                            * layout for the others (4-row kernel on the 4x4 matrix blocks: 225 workgroups for 900 rows);
                            * 3: fragment-packed [ceil(out_dim / 32)][in_dim / 32][4][64][4] for layers with in_dim % 32 == 0
                            * -- element [t][c][q][32 h + r][e] = W[32 t + r][32 c + 16 h + 4 q + e], zeros past out_dim --
                            * nn.Linear's layout for the others (32-row kernel on the 32x32 matrix tiles: launches with
                            * thousands of rows, i.e. a batch of camera streams) */
  int reserved;
  simpb_mlp_chain chain[SIMPB_MLP_MAX_CHAINS];
  const int* m_live;       /* device int or NULL: rows >= *m_live are capacity slots of the static 2D query set; workgroups
                            * whose rows are all past it write zeros and leave (as in simpb_gemm_f32) */
} simpb_mlp_args;
int simpb_mlp_chain_forward(const simpb_mlp_args* args, void* stream);

/* InstanceBank (models/instance_bank.py) state updates for the 11-d box state. All tensors f32 unless noted;
 * A = instances per stream (<= 1024), T = cached instances, C = embed_dims (% 4 == 0).
 * simpb_bank_get (:83-113): anchor_out [bs, T, 11] = cached_anchor warped by T_temp2cur [bs, 4, 4] and advanced by
 *   its velocity over time_interval [bs] (anchor_projection with time_intervals = [-time_interval], :98-101);
 *   mask_out u8 [bs] = |time_interval| <= max_time_interval (:87); time_interval_out [bs] = time_interval where it is
 *   non-zero and valid, else default_time_interval (:108-113).
 * simpb_bank_update (:121-150): rows [0, T) of the outputs = cached rows, rows [T, A) = the A - T current instances
 *   with the largest max-class logit (cls [bs, A, num_classes]), for streams with mask != 0; other streams keep their
 *   current rows and get their instance_id (i64 [bs, A], may be NULL) reset to -1. index_scratch i32 [bs, A - T].
 * simpb_bank_cache (:152-196): cache() + get_instance_id() + update_instance_id(): confidence [bs, T] (in: last
 *   frame's, used when has_previous; out: this frame's), cached_feature [bs, T, C] / cached_anchor [bs, T, 11] out,
 *   instance_id i64 [bs, A] in/out (may be NULL), prev_id i64 [1] in/out, ids_out i64 [bs, A] = the ids
 *   get_instance_id returns; fresh ids are numbered over the flattened batch (:179-181); threshold applies to
 *   sigmoid(max class logit) when has_threshold. index_scratch i32 [bs, T]. hold i32 [num_hold] (may be NULL with
 *   num_hold = 0): overflow flags of this frame's 2D query sets (simpb_alloc_group_start); when any is non-zero the
 *   call writes NOTHING, so that the caller can re-run the frame with a larger capacity on the state the frame found. */
int simpb_bank_get(float* anchor_out, unsigned char* mask_out, float* time_interval_out, const float* cached_anchor,
                   const float* T_temp2cur, const float* time_interval, int batch_size, int num_temp,
                   float max_time_interval, float default_time_interval, void* stream);
int simpb_bank_update(float* feature_out, float* anchor_out, long long* instance_id, int* index_scratch,
                      const float* feature, const float* anchor, const float* cls, const float* cached_feature,
                      const float* cached_anchor, const unsigned char* mask, int batch_size, int num_anchors,
                      int num_classes, int num_temp, int embed_dims, void* stream);
/* simpb_bank_update in its two steps, for callers that can rank early: the ranking depends on the first decoder layer's
 * classification only, not on the bank, so a caller overlapping frames computes it beside the previous frame's decoder
 * (runner.SplitPipelinedRunner) and only the merge waits for the bank. The merge can also carry the anchor embeddings
 * (embed_out / embed [bs, A, E] / cached_embed [bs, T, E], all NULL = absent): embedding rows follow their anchor rows, which
 * replaces the encoder launch behind the update (models/simpb_head.py:621-622). hold (i32 [num_hold], may be NULL): when
 * any is set the instance_id reset of masked-out streams is skipped (the frame is going to be re-run). sticky (device i32,
 * may be NULL) chains the hold over frames decoded before the host has seen their predecessor's flags: simpb_bank_cache
 * writes "held back" (0 / 1) into it at the end of a frame, and a set word holds the NEXT frame's update and commit back
 * like one of its own flags. */
int simpb_bank_update_rank(int* index_scratch, const float* cls, int batch_size, int num_anchors, int num_classes,
                           int num_temp, void* stream);
int simpb_bank_update_merge(float* feature_out, float* anchor_out, float* embed_out, long long* instance_id, const int* index,
                            const float* feature, const float* anchor, const float* embed, const float* cached_feature,
                            const float* cached_anchor, const float* cached_embed, const unsigned char* mask, const int* hold,
                            int num_hold, const int* sticky, int batch_size, int num_anchors, int num_temp, int embed_dims,
                            int pos_embed_dims, void* stream);
int simpb_bank_cache(float* confidence, float* cached_feature, float* cached_anchor, long long* instance_id,
                     long long* prev_id, long long* ids_out, int* index_scratch, const float* feature, const float* anchor,
                     const float* cls, int batch_size, int num_anchors, int num_classes, int num_temp, int embed_dims,
                     int has_previous, float confidence_decay, int has_threshold, float threshold, const int* hold,
                     int num_hold, int* sticky, void* stream);
/* simpb_bank_cache with one workgroup per stream (a batch of streams: the serial form walks them, 13 us each). Same
 * arguments and results; sync_words: two persistent u32 words in device memory, zero before the first call and owned by
 * these calls from then on (an arrival counter and a launch count: the workgroups meet once between counting the fresh
 * instances of the streams in front of them and rewriting their own instance_id). batch_size <= 64; NULL sync_words or a
 * batch of one: the serial kernel. */
int simpb_bank_cache_streams(float* confidence, float* cached_feature, float* cached_anchor, long long* instance_id,
                             long long* prev_id, long long* ids_out, int* index_scratch, const float* feature, const float* anchor,
                             const float* cls, int batch_size, int num_anchors, int num_classes, int num_temp, int embed_dims,
                             int has_previous, float confidence_decay, int has_threshold, float threshold, const int* hold,
                             int num_hold, int* sticky, unsigned* sync_words, void* stream);

/* A batch of independent streams in which some sit a frame out: `active` u8 [batch_size] (device; NULL = every stream is
 * active, results identical to the entry point without the suffix). A stream with active = 0:
 *   simpb_bank_update_merge_active: its instance_id row is not reset even when its mask is 0 (the only persistent write of
 *     this call does not happen); its output rows are written and unspecified.
 *   simpb_bank_cache_streams_active (both forms: serial when sync_words is NULL or batch_size is 1): confidence,
 *     cached_feature, cached_anchor and instance_id rows stay exactly as found, its ids_out row is -1, it takes no fresh ids
 *     (prev_id advances by the active streams' only, and the streams behind it number theirs as if it were not in the
 *     batch); its cls / feature / anchor rows are never read and may hold anything. hold / sticky take precedence: a held
 *     frame writes nothing for anyone. The per-stream form still launches batch_size workgroups and all of them meet. */
int simpb_bank_update_merge_active(float* feature_out, float* anchor_out, float* embed_out, long long* instance_id,
                                   const int* index, const float* feature, const float* anchor, const float* embed,
                                   const float* cached_feature, const float* cached_anchor, const float* cached_embed,
                                   const unsigned char* mask, const int* hold, int num_hold, const int* sticky, int batch_size,
                                   int num_anchors, int num_temp, int embed_dims, int pos_embed_dims,
                                   const unsigned char* active, void* stream);
int simpb_bank_cache_streams_active(float* confidence, float* cached_feature, float* cached_anchor, long long* instance_id,
                                    long long* prev_id, long long* ids_out, int* index_scratch, const float* feature,
                                    const float* anchor, const float* cls, int batch_size, int num_anchors, int num_classes,
                                    int num_temp, int embed_dims, int has_previous, float confidence_decay, int has_threshold,
                                    float threshold, const int* hold, int num_hold, int* sticky, unsigned* sync_words,
                                    const unsigned char* active, void* stream);

/* A batch of streams in which some RESTART: `restart` u8 [batch_size] (device; NULL = no stream, results identical to the
 * entry point without the suffix). A stream with restart != 0 is decoded as the first frame of a fresh bank
 * (InstanceBank.reset() + get() without history, :71-77,115-117) while the others go on:
 *   simpb_bank_get_restart: its mask_out is 0 and its time_interval_out the default, whatever its time_interval; its
 *     anchor_out rows are written and unspecified (simpb_bank_update_merge never reads the cached rows of a stream with a
 *     zero mask: it keeps the stream's current set and resets its instance_id row, hold / sticky permitting).
 *   simpb_bank_cache_streams_restart (both forms): the decay-maximum against the previous confidence (:157-162) is not applied
 *     to it (cache() with confidence = None) and its previous confidence row is never read, so it may hold anything. Its ids
 *     come from the running prev_id like every stream's. `active` as above; a stream should not be paused and restarted at
 *     once (the pause wins). hold / sticky take precedence. */
int simpb_bank_get_restart(float* anchor_out, unsigned char* mask_out, float* time_interval_out, const float* cached_anchor,
                           const float* T_temp2cur, const float* time_interval, int batch_size, int num_temp,
                           float max_time_interval, float default_time_interval, const unsigned char* restart, void* stream);
int simpb_bank_cache_streams_restart(float* confidence, float* cached_feature, float* cached_anchor, long long* instance_id,
                                     long long* prev_id, long long* ids_out, int* index_scratch, const float* feature,
                                     const float* anchor, const float* cls, int batch_size, int num_anchors, int num_classes,
                                     int num_temp, int embed_dims, int has_previous, float confidence_decay, int has_threshold,
                                     float threshold, const int* hold, int num_hold, int* sticky, unsigned* sync_words,
                                     const unsigned char* active, const unsigned char* restart, void* stream);

/* One stream of the bank as a STREAM RECORD: a contiguous u8 buffer that holds everything the persistent state keeps for
 * batch row `stream`, so that the stream can go on in another slot, another bank of the same model or another process.
 * Every section starts at a multiple of 16 bytes from the record's first byte; padding is zero:
 *   header         64 bytes: i32 magic 0x42504D53, i32 layout version 1, i32 num_temp (T), i32 num_anchor (N),
 *                  i32 embed_dims (C), i32 anchor_dims (D), i64 largest id of the id row (-1: none), zeros
 *   confidence     f32 [T]
 *   cached_anchor  f32 [T, D]
 *   cached_feature f32 [T, C]
 *   instance_id    i64 [N]
 * so its size is 64 + pad16(4 T) + pad16(4 T D) + pad16(4 T C) + pad16(8 N) bytes. Bank tensors as in simpb_bank_cache:
 * confidence [bs, T], cached_feature [bs, T, C], cached_anchor [bs, T, D], instance_id i64 [bs, N], prev_id i64 [1]. `blob`
 * is device memory at a multiple of 8 bytes (16-byte accesses are used where record and rows both sit at multiples of 16).
 *   simpb_bank_export_stream: one launch writes the whole record (header included) from the stream's rows; the bank is
 *     only read.
 *   simpb_bank_import_stream: one launch writes the record's four sections into the stream's rows and raises prev_id, the
 *     next id to issue, to max(prev_id, 1 + largest id of the record's id row) -- computed from the row: the header is
 *     neither read nor trusted here, the caller checks it. Importing the same record twice leaves what importing it once
 *     leaves. Nothing but the stream's rows and prev_id is written.
 * Both return SIMPB_EINVAL for a NULL pointer, `stream` outside [0, batch_size), a non-positive size or a misaligned blob. */
int simpb_bank_export_stream(unsigned char* blob, const float* confidence, const float* cached_feature,
                             const float* cached_anchor, const long long* instance_id, int stream, int batch_size, int num_temp,
                             int num_anchor, int embed_dims, int anchor_dims, void* stream_handle);
int simpb_bank_import_stream(float* confidence, float* cached_feature, float* cached_anchor, long long* instance_id,
                             long long* prev_id, const unsigned char* blob, int stream, int batch_size, int num_temp,
                             int num_anchor, int embed_dims, int anchor_dims, void* stream_handle);

/* Fixed-shape detection records of SparseBox3DDecoder.decode_with2d (models/detection3d/decoder.py:124-252).
 * 3D (:133-167 with squeezed classes + decode_box :23-34), one workgroup per sample:
 *   score = max_c sigmoid(cls), label = the first class whose fp32 sigmoid reaches it (torch.max on the sigmoids: not the
 *   argmax of the logits where two of them saturate); the num_output best anchors; re-scored by sigmoid(quality[..., 0]) (quality
 *   may be NULL) and sorted again; rec3d f32 [bs, num_output, SIMPB_RECORD3D_WIDTH = 15] = x y z exp(w) exp(l) exp(h)
 *   atan2(sin, cos) vx vy vz | score | label | score before the re-score | the int64 instance id (or -1) as two
 *   32-bit lanes, low dword first, bit-cast into columns 13 and 14 (read them back through an int64 view: the
 *   reference keeps ids int64 end to end, decoder.py:247-251, and a float is exact only up to 2^24); rank_of_anchor i32 [bs, A] =
 *   rank of the anchor in that order, or -1. cls f32 [bs, A, C]; quality f32 [bs, A, 2]; box f32 [bs, A, 11];
 *   instance_id i64 [bs, A] or NULL. A <= 1024, num_output <= 512.
 * 2D (:168-175 + decode_box2d :36-51), one thread per slot: rec2d f32 [bs, N2, 8] = xyxy box in original image
 *   pixels | max_c sigmoid(cls2d) | label | rank of the slot's anchor (rank_of_anchor[q2a], or -1) | camera. */
int simpb_decode3d_record(float* rec3d, int* rank_of_anchor, const float* cls, const float* quality, const float* box,
                          const long long* instance_id, int batch_size, int num_anchors, int num_classes,
                          int num_output, void* stream);
int simpb_decode2d_record(float* rec2d, const float* cls2d, const float* box2d, const int* q2a, const int* query_cam,
                          const int* rank_of_anchor, int batch_size, int num_query2d, int num_classes, int num_anchors,
                          float crop_w, float crop_h, float crop_y0, float resize, void* stream);

/* The 2D record for a batch of INDEPENDENT streams (simpb_alloc_ragged below): cls2d [slots, C], box2d [slots, 4], q2a and
 * query_cam [slots] are the flat slot array, group_start i32 [bs * cams + 1] its group table, rank_of_anchor i32 [bs * A]
 * (simpb_decode3d_record's output, indexed by the flat anchor b * A + a that q2a holds). rec2d f32 [bs, rows_per_stream, 8]:
 * stream b's slots in its leading rows exactly as simpb_decode2d_record writes them for a batch of one (camera counted
 * within the stream), pad rows (rank -1, camera -1) behind them. (decoder.py:168-175 per sample) */
int simpb_decode2d_record_ragged(float* rec2d, const float* cls2d, const float* box2d, const int* q2a, const int* query_cam,
                                 const int* group_start, const int* rank_of_anchor, int batch_size, int rows_per_stream,
                                 int num_cams, int num_classes, int num_anchors, float crop_w, float crop_h, float crop_y0,
                                 float resize, void* stream);

/* Both 2D records for a rig whose cameras differ in crop and resize (simpb_preprocess_rig_nhwc4_f16): cam_rule, device f32
 * [num_cams, 4], 16-byte aligned, holds (crop_w, crop_h, crop_y0, 1 / resize) per camera in place of the four scalars, and
 * a slot's box is decoded with the row of the slot's own camera (query_cam; counted within the stream in the ragged form).
 * The arithmetic is the scalar entry points': a table of equal rows, 1 / resize rounded to fp32, gives their bits. */
int simpb_decode2d_record_cams(float* rec2d, const float* cls2d, const float* box2d, const int* q2a, const int* query_cam,
                               const int* rank_of_anchor, int batch_size, int num_query2d, int num_classes, int num_anchors,
                               const float* cam_rule, int num_cams, void* stream);
int simpb_decode2d_record_ragged_cams(float* rec2d, const float* cls2d, const float* box2d, const int* q2a,
                                      const int* query_cam, const int* group_start, const int* rank_of_anchor, int batch_size,
                                      int rows_per_stream, int num_cams, int num_classes, int num_anchors, const float* cam_rule,
                                      void* stream);

/* Exchange form of a 2D record (simpb_amd/dist.py): out f32 [bs, rows_out, 8] = the rows of rec2d [bs, rows_in, 8] that
 * decode_with2d returns (rank >= 0 and camera >= 0: slots of the kept 3D boxes, decoder.py:176-251) in their order, pad rows
 * (zeros, rank -1, camera -1) behind them. num_output x num_cams rows always suffice (one slot per anchor and camera), so
 * the exchange shape does not depend on a runner's slot capacity. Rows past rows_out would be dropped (cannot happen at
 * that size). out_stride / in_stride: floats between consecutive streams (multiples of 4; the output may be a column range
 * of a wider send buffer). Both buffers 16-byte aligned. */
int simpb_record2d_compact(float* out, long long out_stride, const float* rec2d, long long in_stride, int batch_size, int rows_in,
                           int rows_out, void* stream);

/* World record (csrc/world.hip): a frame's rec3d as a serving caller consumes it -- boxes in the global frame, score
 * threshold and per-class range limit applied, surviving rows packed in rank order -- restating `_format_bbox`,
 * `output_to_nusc_box` and `lidar_nusc_box_to_global` (datasets/nuscenes_dataset.py:504-586, 824-899) in double.
 *   rec3d f32 [streams, num_output, 15] as simpb_decode3d_record writes it;
 *   pose f64 [streams, 14] = lidar->ego quaternion (w, x, y, z) and translation, ego->global quaternion and translation, raw
 *   (rotation matrices come from q / |q|, quaternion products from q itself); active u8 [streams] or NULL.
 *   A row is kept when its label is a class of the table with class_range >= 0, the ego-frame distance of its centre in
 *   the plane is not above class_range[label], and (has_threshold) its score before the re-score (lane 12) >= threshold.
 *   world f64 [streams, num_output, SIMPB_WORLD_WIDTH = 16] (16-byte aligned) = translation (3) | size w l h (3) | rotation
 *   quaternion (4) | velocity x y (2) | scores_3d | label | attribute code (attr_moving[label] when the global-frame speed
 *   in the plane is above 0.2, attr_still[label] otherwise) | the int64 track id, bit-cast. Kept rows first, in rank order;
 *   every row behind them is zeros with label -1. count i32 [streams] = kept rows, or -1 for a stream with active == 0
 *   (all its rows are pad rows). The tables travel by value: nothing is allocated, so the launch can sit in a capture.
 *   num_output <= 512, one thread per row. */
#define SIMPB_WORLD_WIDTH 16
#define SIMPB_WORLD_MAX_CLASSES 32
typedef struct simpb_world_tables {
  float class_range[SIMPB_WORLD_MAX_CLASSES];        /* metres; negative: the class is never kept */
  unsigned char attr_moving[SIMPB_WORLD_MAX_CLASSES]; /* attribute codes (simpb_amd/results.py: ATTRIBUTE_NAMES) */
  unsigned char attr_still[SIMPB_WORLD_MAX_CLASSES];
  float threshold;
  int has_threshold;
  int num_output;
} simpb_world_tables;
int simpb_world_record(double* world, int* count, const float* rec3d, const double* pose, const unsigned char* active,
                       simpb_world_tables tables, int num_streams, void* stream);

/* Top-k of each score row, sorted descending (ties: lower index first; -0.0 ties with +0.0, and the values
 * returned are the input's own bits): values f32 [bs, k], indices
 * i32 [bs, k] from scores f32 [bs, n], n <= 2048, k <= n. What `topk` of models/instance_bank.py:13-20
 * and the ranking of SparseBox3DDecoder.decode (models/detection3d/decoder.py:145-167) ask of torch.topk /
 * torch.sort; one launch, one workgroup per row. */
int simpb_topk_rows(float* values, int* indices, const float* scores, int batch_size, int n, int k, void* stream);

/* out[row] = sigmoid(dot(x[row, 0:k], w) + b[0]) : ReWeight.alpha (models/aggregation.py:23-24:
 * Linear(f_dim, 1) + Sigmoid) over rows of stride ldx. Rows >= *m_live (may be NULL) get 0. k % 4 == 0. */
int simpb_rowdot_sigmoid(float* out, const float* x, int ldx, const float* w, const float* b, int num_rows, int k,
                         const int* m_live, void* stream);

/* SparseBox3DKeyPointsGenerator.anchor_projection (models/detection3d/blocks.py:248-280) for one
 * transform: out[b, a] = anchor[b, a] with centre = R (centre - vel * time_interval[b]) + t (time_interval
 * may be NULL), velocity = R vel, size kept, and the yaw pair handled exactly as written there (:271-278:
 * the 2x2 block applied to [cos, sin], stored into the [sin, cos] slots in that order). This is what
 * InstanceBank.get (models/instance_bank.py:98-101) runs on the 600 cached anchors at the start of every
 * frame. anchor/out f32 [bs, A, 11]; T_src2dst f32 [bs, 4, 4] row-major; time_interval f32 [bs]. */
int simpb_anchor_projection(float* out, const float* anchor, const float* T_src2dst, const float* time_interval,
                            int batch_size, int num_anchors, void* stream);

/* Operands of simpb_ms_deform_attn_grouped_forward from the raw projections (models/group_attn.py:181-201):
 * raw rows (stride ldraw) = [sampling_offsets heads*L*P*2 | attention logits heads*L*P];
 * attn_weight = softmax over the L*P logits of each head; sampling_loc = ref[row, 0:2] + offset / (W_l, H_l).
 * ref rows have stride ldref (the 2-d reference points, simpb_head.py:523); spatial_shapes i64 [L, 2] = (H, W).
 * Rows >= *m_live (may be NULL) get zeros. Outputs in the layouts of simpb_ms_deform_attn_grouped_forward. */
int simpb_msda_prep(float* sampling_loc, float* attn_weight, const float* raw, int ldraw, const float* ref, int ldref,
                    const long long* spatial_shapes, int num_rows, int num_heads, int num_levels, int num_points,
                    const int* m_live, void* stream);

/* Sampling locations of the 3D deformable aggregation in its own layout: key points of
 * SparseBox3DKeyPointsGenerator.forward (models/detection3d/blocks.py:181-222: num_fix fixed scales x
 * exp(wlh) plus num_learn (sigmoid(learnable) - 0.5) x exp(wlh), rotated by yaw, + centre) projected by
 * DeformableFeatureAggregation.project_points (models/blocks.py:198-213: / clamp(depth, 1e-5), / image_wh).
 *   anchor f32 [bs, A, 11]; learnable f32 [bs, A, num_learn, 3] (output of learnable_fc);
 *   fix_scale f32 [num_fix, 3]; projection_mat f32 [bs, cams, 4, 4]; image_wh f32 [bs, cams, 2]
 *   loc f32 [bs, A, num_fix + num_learn, cams, 2]; key_points f32 [bs, A, P, 3] or NULL */
int simpb_dfa_points(float* loc, float* key_points, const float* anchor, const float* learnable,
                     const float* fix_scale, const float* projection_mat, const float* image_wh, int batch_size,
                     int num_anchors, int num_fix, int num_learn, int num_cams, void* stream);
/* The same with `cam_valid` u8 [batch_size, num_cams] (device; NULL = every camera, identical to simpb_dfa_points): a camera
 * with 0 gets loc = (-1, -1), which the aggregation operator skips (outside (0, 1)), so its tokens are never touched; its
 * projection_mat and image_wh rows are not read and may hold anything. */
int simpb_dfa_points_cams(float* loc, float* key_points, const float* anchor, const float* learnable,
                          const float* fix_scale, const float* projection_mat, const float* image_wh, int batch_size,
                          int num_anchors, int num_fix, int num_learn, int num_cams, const unsigned char* cam_valid,
                          void* stream);

/* Weights of the 3D deformable aggregation in its own layout (models/blocks.py:164-187 + :132-143):
 *   feat_logits f32 [bs, A, lvl*pts*groups] = weights_fc(feature + anchor_embed)
 *   cam_logits  f32 [bs, cams, lvl*pts*groups] = camera_embed @ weights_fc.weight^T (no bias)
 *   weights     f32 [bs, A, pts, cams, lvl, groups] = softmax over (cam, lvl, pts) per group of their sum */
int simpb_dfa_weights(float* weights, const float* feat_logits, const float* cam_logits, int batch_size,
                      int num_anchors, int num_cams, int num_levels, int num_pts, int num_groups, void* stream);
/* The same with `cam_valid` u8 [batch_size, num_cams] (device; NULL = every camera, identical to simpb_dfa_weights): the
 * softmax runs over the valid cameras only. A masked camera's logits count as -inf without its cam_logits row being read
 * (it may hold NaN): its weights are exactly 0.0, the others are renormalised. No valid camera: all weights 0.0. */
int simpb_dfa_weights_cams(float* weights, const float* feat_logits, const float* cam_logits, int batch_size,
                           int num_anchors, int num_cams, int num_levels, int num_pts, int num_groups,
                           const unsigned char* cam_valid, void* stream);

/* Adaptive query allocation, replaces DynamicQueryAllocation.projection_allocation
 * (models/allocation.py:27-144) in three steps; the caller reads `count` back between steps 2
 * and 3 to size the 2D query set (the reference does the same with .tolist() at :94).
 *
 * Step 1 (:30-83): project the 8 box corners (size = exp(wlh) clamped to limit_*) and the centre of
 * every anchor into every camera.
 *   anchor         f32 [batch_size, num_anchors, 11]   x,y,z,log w,log l,log h,sin,cos,vx,vy,vz
 *   projection_mat f32 [batch_size, num_cams, 4, 4]
 *   flag           u8  [batch_size, num_cams, num_anchors]   0 none, 1 corner-only, 2 centre valid
 *   sel_xy         f32 [batch_size, num_cams, num_anchors, 2] reference point in pixels
 *   depth          f32 [batch_size, num_cams, num_anchors]    centre depth (signed) */
int simpb_alloc_project(unsigned char* flag, float* sel_xy, float* depth, const float* anchor,
                        const float* projection_mat, int batch_size, int num_anchors, int num_cams,
                        float img_w, float img_h, float limit_w, float limit_l, float limit_h, void* stream);
/* The same with `cam_valid` u8 [batch_size, num_cams] (device; NULL = every camera, identical to simpb_alloc_project): a
 * (stream, camera) with 0 delivered no frame -- its flag row is 0 (forced: its matrix is not read and may hold anything), so
 * step 2 counts 0 and step 3 gives it an empty camera group. This is the single place of the allocation that knows the
 * camera mask: the stepwise, static and independent-streams forms all get it through this step. */
int simpb_alloc_project_cams(unsigned char* flag, float* sel_xy, float* depth, const float* anchor,
                             const float* projection_mat, int batch_size, int num_anchors, int num_cams, float img_w,
                             float img_h, float limit_w, float limit_l, float limit_h, const unsigned char* cam_valid,
                             void* stream);

/* Step 2 (:86-123): per (batch, cam) stable compaction in ascending anchor order.
 *   count i32 [batch_size, num_cams]; order i32 [batch_size, num_cams, num_anchors] (first count valid) */
int simpb_alloc_compact(int* count, int* order, const unsigned char* flag, int batch_size, int num_anchors,
                        int num_cams, void* stream);

/* Step 2b, optional (:91-99 without the host round trip): group_start i32 [num_cams + 1] =
 * prefix sums of the max-over-batch counts, clipped to `capacity`; overflow i32 [1] = 1 when the 2D
 * query set does not fit `capacity` (the caller must then redo the frame with a larger capacity). */
int simpb_alloc_group_start(int* group_start, int* overflow, const int* count, int batch_size, int num_cams,
                            int capacity, void* stream);

/* Step 3 (:103-142): fill the slot tables. group_start i32 [num_cams + 1] (device) are the
 * max-over-batch prefix sums (:91-99); slots past a sample's own count are pads (q2a = -1, zeros).
 *   ref_pts2d f32 [bs, num_query, 2] (divided by img_w, img_h); ref_depth2d f32 [bs, num_query, 1] = |depth|
 *   q2a i32 [bs, num_query] slot -> anchor; is_center i32 [bs, num_query];
 *   a2q i32 [bs, num_anchors, num_cams] (anchor, cam) -> slot or -1; query_cam i32 [num_query]
 *   (num_query may exceed group_start[num_cams]: those capacity slots get query_cam = -1 and pad values)
 * q2a/is_center are the index form of the reference's one-hot trans_matrix / center_matrix. */
int simpb_alloc_scatter(float* ref_pts2d, float* ref_depth2d, int* q2a, int* is_center, int* a2q, int* query_cam,
                        const int* group_start, const int* count, const int* order, const unsigned char* flag,
                        const float* sel_xy, const float* depth, int batch_size, int num_anchors, int num_cams,
                        int num_query, float img_w, float img_h, void* stream);

/* Steps 1-3 with a fixed capacity as three launches instead of five (a replayed frame pays ~4.7 us of dispatch per
 * kernel whatever it does, and these run three times per frame): the -1 fill of a2q rides in step 1 (same index space), the
 * group table of simpb_alloc_group_start (capacity = num_query) is derived by step 3's threads from the counts and
 * published by one of them. Every output of the four stepwise calls, same arithmetic, same tables; num_cams <= 8. (One workgroup walking
 * all steps was measured at 49 us against 24 us for the five launches: its steps hand over through global memory and
 * serialise the round trips.) */
int simpb_alloc_static(unsigned char* flag, float* sel_xy, float* depth, int* count, int* order, int* group_start,
                       int* overflow, float* ref_pts2d, float* ref_depth2d, int* q2a, int* is_center, int* a2q,
                       int* query_cam, const float* anchor, const float* projection_mat, int batch_size, int num_anchors,
                       int num_cams, int capacity, float img_w, float img_h, float limit_w, float limit_l, float limit_h,
                       void* stream);
/* The same with `cam_valid` u8 [batch_size, num_cams] (device; NULL = every camera, identical to simpb_alloc_static): see
 * simpb_alloc_project_cams. A masked (stream, camera) has count 0 and a2q = -1 and cannot raise overflow. */
int simpb_alloc_static_cams(unsigned char* flag, float* sel_xy, float* depth, int* count, int* order, int* group_start,
                            int* overflow, float* ref_pts2d, float* ref_depth2d, int* q2a, int* is_center, int* a2q,
                            int* query_cam, const float* anchor, const float* projection_mat, int batch_size,
                            int num_anchors, int num_cams, int capacity, float img_w, float img_h, float limit_w,
                            float limit_l, float limit_h, const unsigned char* cam_valid, void* stream);

/* The allocation for a batch of INDEPENDENT camera streams ("keep per-sample counts in the native path"):
 * DynamicQueryAllocation.projection_allocation (models/allocation.py:27-144) pads every camera group to the max over the
 * batch (:91-99), so a batch of streams with different headings carries ~3x the 2D slots a stream needs and attends the
 * pads as keys; here every stream keeps the set a batch of one gives it. Steps 1-2 as simpb_alloc_static; step 3 lays the
 * 2D set out as ONE flat slot array [batch_size * per_stream], stream-major then camera-major, live slots first:
 *   group_start i32 [bs * cams + 1] (group g = b * cams + cam), query_cam i32 [slots] = g (or -1: capacity slot),
 *   q2a i32 [slots] = b * num_anchors + a (or -1), is_center, ref_pts2d f32 [slots, 2], ref_depth2d f32 [slots],
 *   a2q i32 [bs, A, cams] = flat slot (or -1); overflow[0] = 1 when a stream needs more than per_stream slots (clipped).
 * The 2D operators then run as a batch of one over bs * cams camera groups (they take the group tables as they are),
 * and the 3D side sees [1, bs * A, .] views. batch_size * num_cams <= 96. */
int simpb_alloc_ragged(unsigned char* flag, float* sel_xy, float* depth, int* count, int* order, int* group_start,
                       int* overflow, float* ref_pts2d, float* ref_depth2d, int* q2a, int* is_center, int* a2q,
                       int* query_cam, const float* anchor, const float* projection_mat, int batch_size, int num_anchors,
                       int num_cams, int per_stream, float img_w, float img_h, float limit_w, float limit_l, float limit_h,
                       void* stream);
/* The same with `active` u8 [batch_size] (device; NULL = every stream, identical to simpb_alloc_ragged): a stream with
 * active = 0 gets no 2D slots -- flag rows 0 (forced: its anchors and matrices are not read and may hold anything), count 0,
 * empty groups, a2q rows -1 -- and cannot raise overflow. The slot array stays "live slots first": the streams behind it
 * move down and group_start[bs * cams] shrinks, so a paused stream costs the 2D operators nothing. */
int simpb_alloc_ragged_active(unsigned char* flag, float* sel_xy, float* depth, int* count, int* order, int* group_start,
                              int* overflow, float* ref_pts2d, float* ref_depth2d, int* q2a, int* is_center, int* a2q,
                              int* query_cam, const float* anchor, const float* projection_mat, int batch_size,
                              int num_anchors, int num_cams, int per_stream, float img_w, float img_h, float limit_w,
                              float limit_l, float limit_h, const unsigned char* active, void* stream);
/* The same with `cam_valid` u8 [batch_size, num_cams] as well (device; NULL = every camera, identical to
 * simpb_alloc_ragged_active): a camera with 0 in an active stream is an empty group -- flag row 0 without its matrix being
 * read, count 0, a2q = -1 -- and the groups behind it move down, as the streams behind a paused one do. A paused stream's
 * camera row is not looked at. */
int simpb_alloc_ragged_cams(unsigned char* flag, float* sel_xy, float* depth, int* count, int* order, int* group_start,
                            int* overflow, float* ref_pts2d, float* ref_depth2d, int* q2a, int* is_center, int* a2q,
                            int* query_cam, const float* anchor, const float* projection_mat, int batch_size,
                            int num_anchors, int num_cams, int per_stream, float img_w, float img_h, float limit_w,
                            float limit_l, float limit_h, const unsigned char* active, const unsigned char* cam_valid,
                            void* stream);

/* out[b, s, :] = src[b, q2a[b, s], :], zeros where q2a < 0: replaces
 * torch.matmul(ref_trans_matrix, instance_feature) (models/simpb_head.py:438). channels % 4 == 0. */
int simpb_gather_rows(float* out, const float* src, const int* q2a, int batch_size, int num_anchors,
                      int num_query, int channels, void* stream);

/* 2D -> 3D re-weighted mean, replaces ReWeight.forward's two dense matmuls
 * (models/aggregation.py:30-35) plus the adds at :88-89:
 *   out_q[b,a]   = q3d[b,a]   + sum_s alpha[b,s] q2d[b,s]   / clamp(sum_s alpha[b,s], 1e-5)
 *   out_pos[b,a] = pos3d[b,a] + sum_s alpha[b,s] pos2d[b,s] / clamp(...)      s over a2q[b,a,:] >= 0 */
int simpb_aggregate_2d_to_3d(float* out_q, float* out_pos, const float* q3d, const float* pos3d, const float* q2d,
                             const float* pos2d, const float* alpha, const int* a2q, int batch_size,
                             int num_anchors, int num_cams, int num_query, int channels, void* stream);

/* The same with ReWeight.alpha (models/aggregation.py:23-24) computed inside the launch instead of read from memory:
 * alpha[b,s] = sigmoid(hidden[b,s,:] . w_alpha + b_alpha) with hidden f32 [bs, num_query, hidden_dim] (row stride
 * ld_hidden) = ReLU(ReWeight.reduce(...)); every slot belongs to one anchor, so each alpha is computed once. hidden NULL:
 * alpha is read as above. num_cams <= 8; hidden_dim % 4 == 0; hidden, w_alpha 16-byte aligned. */
int simpb_aggregate_2d_to_3d_alpha(float* out_q, float* out_pos, const float* q3d, const float* pos3d, const float* q2d,
                                   const float* pos2d, const float* alpha, const int* a2q, const float* hidden,
                                   int ld_hidden, int hidden_dim, const float* w_alpha, const float* b_alpha,
                                   int batch_size, int num_anchors, int num_cams, int num_query, int channels,
                                   void* stream);

/* ---- Camera health: which cameras of a frame delivered a usable image, decided on the device behind the ingest ----
 * Two launches. The first reads every image once and leaves integer statistics; the second turns them, the host's masks and
 * a small persistent state into the u8 [batch_size, num_cams] camera mask the *_cams entry points above read, in the same
 * frame, without a host round trip. Every statistic is an integer that does not depend on the order of summation, and the
 * verdict's float64 arithmetic rounds once per operation (no contraction): a host model reproduces both bit for bit.
 *
 * Statistics of image n, X = f16 [height, width, 4] as the ingest writes it (channels 0..2 used, channel 3 never looked at):
 *   q(x) = x * 2^24 as int64 (exact for every finite f16); a non-finite x counts in nonfinite[n] and contributes 0;
 *   S[n][i][j][k] = sum of q over cell (i, j) of the fixed SIMPB_HEALTH_GRID x SIMPB_HEALTH_GRID grid, per channel k: rows
 *     [i * height / 8, (i + 1) * height / 8), columns [j * width / 8, (j + 1) * width / 8) (integer division);
 *   hash[n] = sum over (y, x, k < 3) of mix(bits16(X[y, x, k]) | (((y * width + x) * 3 + k) << 16)) mod 2^64, mix = the
 *     splitmix64 finaliser (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31).
 * They are left as PARTIAL ROWS, int64 [num_images, SIMPB_HEALTH_BANDS, SIMPB_HEALTH_PARTIAL_WORDS]: band i * 8 + b is the
 * b-th eighth of the rows of cell row i (rows r0 + b * n / 8 .. r0 + (b + 1) * n / 8 of its n rows; possibly none), and a
 * row holds S of that band's pixels as [j * 3 + k] (24 words), the band's part of the hash (word 24) and its non-finite
 * count (word 25). Every word of every row is written by plain stores on every call: nothing has to be zeroed in between.
 * images: 8-byte aligned (any image may start off a 16-byte boundary). 8 <= height, width <= 16384; num_images <= 65535. */
#define SIMPB_HEALTH_GRID 8
#define SIMPB_HEALTH_BANDS 64
#define SIMPB_HEALTH_PARTIAL_WORDS 26
int simpb_image_health_stats(long long* partials, const void* images, int num_images, int height, int width, void* stream);
/* Bytes of the partial rows of num_images images (a multiple of 8, below 2^31); SIMPB_EINVAL (1: no size is that small)
 * for sizes the launch refuses. */
int simpb_image_health_partials_bytes(int num_images, int height, int width);

#define SIMPB_HEALTH_DARK 1
#define SIMPB_HEALTH_BRIGHT 2
#define SIMPB_HEALTH_FLAT 4
#define SIMPB_HEALTH_FROZEN 8
#define SIMPB_HEALTH_FAIL_OPEN 16
#define SIMPB_HEALTH_NONFINITE 32
typedef struct simpb_health_params {
  double dark_below, bright_above, flat_below; /* levels 0..255 of the preprocessed image; read where the check is on */
  double mean[3], std[3];                      /* of the normalisation, in the channel order of the normalised tensor */
  int check_dark, check_bright, check_flat, check_frozen; /* 0: the check is off */
  int frozen_after;                            /* >= 1 where check_frozen */
  int act;                                     /* 0: flags are reported, cam_out = cam_in */
} simpb_health_params;
/* Persistent state per (stream, camera), 16 bytes: what the frozen check remembers. */
typedef struct simpb_health_state {
  unsigned long long prev_hash;
  unsigned int repeats, frames;
} simpb_health_state;
/* The verdict for image s * num_cams + c of `partials` (the rows are added in band order). A camera is CONSIDERED iff
 * active[s] && cam_in[s][c] (u8, device; NULL = all ones); one that is not keeps its state, gets flags 0, and its rows are
 * not read. For a considered one, per channel level_k = double(sum_ij S[k]) / (double(height * width) * 2^24) * std_k +
 * mean_k, L = (level_0 + level_1 + level_2) / 3, and Lc[i][j] the same from one cell and its pixel count;
 *   DARK: L < dark_below   BRIGHT: L > bright_above   FLAT: max Lc - min Lc < flat_below   NONFINITE: nonfinite > 0
 *   FROZEN: repeats >= frozen_after after { repeats = frames > 0 && hash == prev_hash ? repeats + 1 : 0; prev_hash = hash;
 *   frames += 1 } (all comparisons strict as written).
 * If every considered camera of a stream has one of these, none is dropped and each gets FAIL_OPEN as well.
 * flags u8 [batch_size, num_cams]; cam_out u8 [batch_size, num_cams] = cam_in && !(fault && act && !fail_open);
 * state: simpb_health_state [batch_size, num_cams], read and written. num_cams <= 64, batch_size <= 65535. */
int simpb_camera_health_verdict(unsigned char* cam_out, unsigned char* flags, simpb_health_state* state,
                                const long long* partials, const unsigned char* cam_in, const unsigned char* active,
                                simpb_health_params params, int batch_size, int num_cams, int height, int width,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif
