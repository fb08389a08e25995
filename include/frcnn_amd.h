/*
 * frcnn_amd.h — C-ABI of the MI355X (gfx950) Faster R-CNN detection hot path.
 *
 * Every entry point replaces one function/type of the reference
 * (pengfeidip/pytorch-faster-rcnn, cited as path:line) or of the third-party
 * torchvision kernels the reference calls.  Conventions:
 *   - plain device pointers + sizes; no framework types.  Boxes are
 *     coordinate-major "[4, n]" float32 (row k = coordinate k, row stride `ld`
 *     elements), exactly the reference's channel-first layout, unless a
 *     parameter says "[n,4]" (row-major xyxy, torchvision layout).
 *   - `stream` is a hipStream_t; every call is asynchronous on it and never
 *     synchronises, allocates or frees (capturable into a hipGraph).
 *   - scratch memory comes from the caller through (workspace, ws_bytes);
 *     each op has a *_workspace() size query.  The library keeps no global
 *     mutable state: reentrant and thread-safe per stream.
 *   - variable-size results are written into caller-sized maxima plus a
 *     device-side int32 count.
 *   - return 0 on success, a negative FRH_E* code otherwise;
 *     frh_last_error() gives a thread-local message.
 */
#ifndef FRCNN_AMD_H
#define FRCNN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRH_ABI_VERSION 3

#define FRH_OK 0
#define FRH_EINVAL (-1)
#define FRH_EUNSUPPORTED (-2)
#define FRH_ELAUNCH (-3)

#define FRH_MAX_LEVELS 8

int32_t frh_abi_version(void);
const char* frh_last_error(void);

/* Device status word (ABI 2).  The one-launch kernels of frh_rpn_proposals* and
 * frh_sample_random hand data between the workgroups of ONE launch through bounded
 * in-launch waits, sized to the device's resident capacity (CU count x occupancy, queried
 * per device).  A wait that runs out -- a workgroup it needs was never scheduled, e.g. beside
 * other kernels or on a partitioned GPU -- ORs one of these bits into the caller's device
 * int32 `status` word and ends that workgroup's work: the call's outputs are then undefined
 * and the workspace's zero region may be left dirty (re-zero it).  The library never reads
 * the word except (ABI 3) the loss entries, which write NaN losses while it is nonzero, and
 * frh_sample_random's one-launch form, which does nothing while it is nonzero (its zero region
 * may be dirty): the step's own loss read carries a failure, and the caller checks the word
 * where it synchronises anyway (frcnn_amd: every training step before the optimizer update,
 * the numpy sampler's count read, or after every call with FRCNN_AMD_DEBUG=1) and clears it. */
#define FRH_DEVERR_SELECT_BARRIER 1   /* rpn_select_kernel: a segment barrier timed out */
#define FRH_DEVERR_NMS_COLUMN 2       /* nms_fused_kernel: a mask column never completed */
#define FRH_DEVERR_SAMPLER_BARRIER 4  /* sampler_fused_kernel: an image barrier timed out */

/* ---- a1: AnchorCreator.__call__ over all FPN levels in one launch ------------
 * Replaces lib/anchor.py:107-129 (called per level from
 * lib/heads/anchor_head.py:66-67).  Level l has grid (grid_hw[2l], grid_hw[2l+1]),
 * stride strides[l] and per-anchor sizes ws/hs[l*num_anchors + a] (the f32
 * casts of the reference's float64 base*s*sqrt(ar), anchor.py:92-97).
 * Output: [4, ld] with level l occupying columns [off_l, off_l + A*H*W) in
 * the reference's [4, A, H, W].view(4,-1) order, off_l = sum of earlier levels. */
int32_t frh_anchor_grid(int32_t num_levels, const int32_t* grid_hw, const float* strides,
                        const float* ws, const float* hs, int32_t num_anchors,
                        int32_t center_lt, float* out, int64_t ld, void* stream);

/* ---- a2: inside_anchor_mask & inside_grid_mask --------------------------------
 * Replaces lib/region.py:10-29 as combined in lib/heads/anchor_head.py:93-99.
 * in_hw[2l..] = min(grid, int(img/stride)+1) computed by the caller in double
 * exactly as region.py:12-13.  allowed_border < 0 disables the image test. */
int32_t frh_inside_mask(const float* anchors, int64_t ld, int32_t num_levels,
                        const int32_t* grid_hw, const int32_t* in_hw, int32_t num_anchors,
                        int32_t img_h, int32_t img_w, int32_t allowed_border,
                        uint8_t* mask, void* stream);

/* ---- a3: calc_iou / elem_iou ----------------------------------------------------
 * calc_iou: lib/utils.py:151-172 -> out[n, k] (row-major), bit-exact.
 * elem_iou: lib/utils.py:174-182 (no +1) -> out[n]. */
int32_t frh_iou_table(const float* a, int64_t lda, int64_t n, const float* b, int64_t ldb,
                      int64_t k, float* out, void* stream);
int32_t frh_elem_iou(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t n,
                     float* out, void* stream);

/* ---- a4: MaxIoUAssigner.__call__, batched over segments (images) -------------
 * Replaces lib/region.py:60-107.  Segment s: boxes at boxes + s*box_seg_stride
 * ([4, box_ld]), count num_boxes[s] (device), optional validity mask
 * valid + s*valid_seg_stride (nullptr = all valid; invalid boxes get label -1
 * and take no part in the per-gt maxima), gts at gts + s*gt_seg_stride
 * ([4, gt_ld]), count num_gts[s] (device).  Labels are int64:
 * -1 ignore, 0 negative, g+1 positive for gt g; max_iou f32.  Thresholds are
 * compared in f32 like the reference (`f32 tensor < python float`).  Rows in
 * [num_boxes[s], max_boxes) are padding: label -1, max_iou 0.
 * max_boxes / max_gts bound the launch (host-known maxima of the counts).  One launch: the
 * last workgroup of each segment labels the boxes tied at a gt's maximum (hand-off inside
 * the launch).  Workspace: frh_maxiou_assign_workspace bytes whose leading
 * frh_maxiou_assign_zero_bytes(num_segs, max_gts) bytes are zero before the call; every call
 * leaves them zero, so a caller zero-fills them once per (num_segs, max_gts) layout and reuses
 * the buffer for calls ordered on one stream. */
size_t frh_maxiou_assign_zero_bytes(int32_t num_segs, int32_t max_gts);
size_t frh_maxiou_assign_workspace(int32_t num_segs, int32_t max_gts, int64_t max_boxes);
int32_t frh_maxiou_assign(int32_t num_segs, const float* boxes, int64_t box_ld,
                          int64_t box_seg_stride, const int32_t* num_boxes,
                          const uint8_t* valid, int64_t valid_seg_stride,
                          const float* gts, int64_t gt_ld, int64_t gt_seg_stride,
                          const int32_t* num_gts, float pos_iou, float neg_iou,
                          float min_pos_iou, int64_t* labels, int64_t label_seg_stride,
                          float* max_iou, int64_t iou_seg_stride, int64_t max_boxes,
                          int32_t max_gts, void* workspace, size_t ws_bytes, void* stream);

/* ---- a5: RandomSampler / random_sample_label ----------------------------------
 * Replaces lib/region.py:43-57,112-126.  Two modes:
 *  (1) reference-RNG parity: frh_sample_candidates lists, per segment and in
 *      ascending box order, the positive (label>0) and negative (label==0)
 *      boxes plus their counts ([S,2] device int32).  The host draws the
 *      reference's numpy permutation, then frh_sample_apply keeps the chosen
 *      list positions (keep_pos/keep_neg [S, keep_ld] device, counts in
 *      keep_counts [S,2]) and writes labels_out (-1 for everything else).
 *  (2) device RNG: frh_sample_random keeps min(npos,pos_num) positives and
 *      min(nneg, max_num-kept_pos) negatives, each chosen uniformly without
 *      replacement by the smallest 32-bit hash(seed, seg, box) keys.  Outputs
 *      (either or both): labels_out (the sampled labels, -1 elsewhere) and / or
 *      sel [S][2][max_num] (the kept positives / negatives, in no order) with
 *      sel_counts [S][2] -- the form frh_anchor_target / frh_bbox_target take
 *      without a compaction pass over every box. */
size_t frh_sample_workspace(int32_t num_segs, int64_t max_boxes);
/* frh_sample_random's workspace contract: its leading frh_sample_zero_bytes(num_segs) bytes
 * (the same for every num_segs <= 64: nothing else is placed there) are zero before the call
 * and every completed call leaves them zero (images above 16 384 boxes take a one-launch
 * sampler whose per-image counters and histograms live there and are reset by the launch's
 * last workgroup), so a caller zero-fills the buffer once and reuses it for calls ordered on
 * one stream, whatever their num_segs.  After FRH_DEVERR_SAMPLER_BARRIER, re-zero it.
 * num_segs <= 64. */
size_t frh_sample_zero_bytes(int32_t num_segs);
int32_t frh_sample_candidates(int32_t num_segs, const int64_t* labels, int64_t label_seg_stride,
                              const int32_t* num_boxes, int64_t max_boxes, int32_t* pos_list,
                              int32_t* neg_list, int64_t list_seg_stride, int32_t* counts,
                              void* workspace, size_t ws_bytes, void* stream);
int32_t frh_sample_apply(int32_t num_segs, const int64_t* labels_in, int64_t label_seg_stride,
                         const int32_t* num_boxes, int64_t max_boxes, const int32_t* pos_list,
                         const int32_t* neg_list, int64_t list_seg_stride,
                         const int32_t* keep_pos, const int32_t* keep_neg, int64_t keep_ld,
                         const int32_t* keep_counts, int64_t* labels_out, void* stream);
int32_t frh_sample_random(int32_t num_segs, const int64_t* labels_in, int64_t label_seg_stride,
                          const int32_t* num_boxes, int64_t max_boxes, int32_t max_num,
                          int32_t pos_num, uint64_t seed, int64_t* labels_out, int32_t* sel,
                          int32_t* sel_counts, int32_t* status, void* workspace, size_t ws_bytes,
                          void* stream);

/* ---- a5b: IoUBalancedNegSampler -----------------------------------------------
 * Replaces lib/region.py:128-172.  Per image: kp = min(#positives, pos_num) positives are
 * kept; num_neg = max_num - kp; the negatives (label == 0) are binned by their IoU
 * (row i's IoU is ious[s * iou_seg_stride + i - iou_offsets[s]]: frh_maxiou_assign's max_iou,
 * with iou_offsets (device int32 [S], NULL = 0) the number of rows frh_prepend_gt_labels put
 * in front; read for label == 0 rows only, so the prepended ground truth needs no value) into num_bins (1..8) bins
 * bin_lo[j] <= iou < bin_hi[j] (host arrays, ascending, computed by the caller with the
 * reference's i*bin_size / s+bin_size and rounded to f32; bins that overlap are refused
 * with FRH_EINVAL where the reference would count a box twice).  Bins are visited from the
 * highest to the lowest; each but the lowest takes min(count, int(num_neg / num_bins)), the
 * lowest min(count, num_neg - taken so far); negatives in no bin (iou >= max_iou) are never
 * chosen and the total may stay below max_num (region.py:158-165).
 *  device mode: frh_sample_iou_balanced; each class (the positives, each bin) keeps its
 *   quota uniformly without replacement by the extreme hash(seed, class, box) keys, as
 *   frh_sample_random.  Outputs as frh_sample_random's (labels_out and / or sel
 *   [S][2][max_num] + sel_counts [S][2], every bin's choices in the negatives' list), so
 *   frh_bbox_target consumes them unchanged.  One workgroup per (class, image), no
 *   cross-workgroup wait: no status word and no workspace.  Images above 16 384 rows
 *   return FRH_EUNSUPPORTED.
 *  reference-RNG parity: frh_sample_iou_candidates lists, per image s and class w (0 the
 *   positives, 1 + j the j-th VISITED bin, i.e. the highest bin first), the class's rows in
 *   ascending order at lists[(s * (1 + num_bins) + w) * list_ld ..] and their number in
 *   counts[s * (1 + num_bins) + w]; the host draws the reference's np.random.choice per
 *   over-full class and frh_sample_apply keeps the chosen positions (pos_list = the class-0
 *   list, neg_list = the class-1 list with positions j * list_ld + p for bin j, segment
 *   stride (1 + num_bins) * list_ld).  Same row capacity. */
int32_t frh_sample_iou_balanced(int32_t num_segs, const int64_t* labels_in, int64_t label_seg_stride,
                                const float* ious, int64_t iou_seg_stride, const int32_t* iou_offsets,
                                const int32_t* num_boxes, int64_t max_boxes, int32_t max_num, int32_t pos_num, int32_t num_bins,
                                const float* bin_lo, const float* bin_hi, uint64_t seed,
                                int64_t* labels_out, int32_t* sel, int32_t* sel_counts, void* stream);
int32_t frh_sample_iou_candidates(int32_t num_segs, const int64_t* labels, int64_t label_seg_stride,
                                  const float* ious, int64_t iou_seg_stride, const int32_t* iou_offsets,
                                  const int32_t* num_boxes, int64_t max_boxes, int32_t num_bins, const float* bin_lo,
                                  const float* bin_hi, int32_t* lists, int64_t list_ld, int32_t* counts,
                                  void* stream);

/* ---- a6: anchor_target (lib/anchor.py:11-76) after assign+sample -------------
 * Chosen = boxes with sampled label >= 0, ascending.  Segment outputs are
 * concatenated in segment order (the reference's per-image results followed
 * by torch.cat in anchor_head.py:189-192); out_counts[s] = chosen count of s,
 * out_counts[num_segs] = total.  Outputs (column j of the concatenation):
 *   chosen_idx[j] (int64, index into the per-segment box space),
 *   seg_of[j] (int32), tar_labels[j] (int64: gt_label[g] or 0 for negatives;
 *   gt_label == nullptr => 1/0), tar_anchors/tar_bbox/tar_param [4, out_ld].
 * tar_param = (bbox2param(anchor, gt) - means) / stds (anchor.py:69-73).
 * sel / sel_counts (nullable; frh_sample_random's lists, max_num = max_out_per_seg
 * <= 8192): the chosen boxes are those lists (ranked into ascending box order in
 * the gather itself) and `labels` are the assignment labels before sampling; no
 * workspace is needed.  With sel, columns [total, num_segs*max_out_per_seg) are padding
 * (seg_of -1, tar_labels -1, zero boxes), so a caller may consume the whole capacity
 * against the device total instead of reading it back. */
int32_t frh_anchor_target(int32_t num_segs, const int64_t* labels, int64_t label_seg_stride,
                          const int32_t* num_boxes, int64_t max_boxes, const float* anchors,
                          int64_t anchor_ld, int64_t anchor_seg_stride, const float* gts,
                          int64_t gt_ld, int64_t gt_seg_stride, const int64_t* gt_labels,
                          int64_t gt_label_seg_stride, const float* means, const float* stds,
                          int64_t max_out_per_seg, const int32_t* sel, const int32_t* sel_counts,
                          int64_t* chosen_idx, int32_t* seg_of,
                          int64_t* tar_labels, float* tar_anchors, float* tar_bbox,
                          float* tar_param, int64_t out_ld, int32_t* out_counts,
                          void* workspace, size_t ws_bytes, void* stream);
size_t frh_anchor_target_workspace(int32_t num_segs, int64_t max_boxes);

/* gather of per-level head outputs at chosen anchors (anchor.py:51-56) and its
 * adjoint (autograd backward).  Level l tensor: [B, C*A, H, W] contiguous
 * viewed per image as [C, A*H*W] (anchor_head.py:82); level_off[l] = first
 * flat index of the level.  out: [C, out_ld].  A column with seg_of < 0 (padding) gathers
 * zeros and scatters nothing. */
int32_t frh_gather_level_outputs(int32_t num_levels, const float* const* level_ptrs,
                                 const int64_t* level_off, const int64_t* level_hw_a,
                                 int32_t channels, int64_t total, const int64_t* chosen_idx,
                                 const int32_t* seg_of, float* out, int64_t out_ld,
                                 void* stream);
int32_t frh_scatter_level_grads(int32_t num_levels, float* const* level_grads,
                                const int64_t* level_off, const int64_t* level_hw_a,
                                int32_t channels, int64_t total, const int64_t* chosen_idx,
                                const int32_t* seg_of, const float* grad, int64_t grad_ld,
                                void* stream);
/* The same for head outputs of any layout (NCHW or channels-last): level l is
 * [B, C*A, H_l, W_l] with element strides level_strides[4l..4l+3] = (b, c, y, x),
 * level_hw[2l..2l+1] = (H_l, W_l), A = num_anchors; anchor index a*H*W + y*W + x of the
 * reference's [C, A*H*W] view reads tensor channel c*A + a. */
int32_t frh_gather_level_outputs_strided(int32_t num_levels, const float* const* level_ptrs,
                                         const int64_t* level_off, const int32_t* level_hw,
                                         const int64_t* level_strides, int32_t num_anchors,
                                         int32_t channels, int64_t total, const int64_t* chosen_idx,
                                         const int32_t* seg_of, float* out, int64_t out_ld,
                                         void* stream);
int32_t frh_scatter_level_grads_strided(int32_t num_levels, float* const* level_grads,
                                        const int64_t* level_off, const int32_t* level_hw,
                                        const int64_t* level_strides, int32_t num_anchors,
                                        int32_t channels, int64_t total, const int64_t* chosen_idx,
                                        const int32_t* seg_of, const float* grad, int64_t grad_ld,
                                        void* stream);

/* ---- a12: bbox_target (lib/bbox.py:6-82) ------------------------------------
 * frh_prepend_gt_labels builds the reference's candidate list
 * [gts ; proposals] (bbox.py:27-29): rows_out[s, j] = j+1 for j < G_s, else
 * prop_labels[s, j-G_s]; num_rows[s] = G_s + n_s; rows in [G_s + n_s, max_rows) are
 * padding, label -1.  After sampling those rows,
 * frh_bbox_target (labels = the sampled rows, num_rows from the prepend)
 * gathers the chosen rows (ascending) into concatenated
 * outputs: tar_props/tar_bbox/tar_param [4, out_ld], tar_label (int64, gt
 * class or 0), tar_is_gt (int64 0/1), out_counts[S+1] as in frh_anchor_target;
 * sel / sel_counts as in frh_anchor_target (labels = the prepended rows; padding columns
 * past the total: tar_label -1, tar_is_gt 0, zero boxes). */
int32_t frh_prepend_gt_labels(int32_t num_segs, const int64_t* prop_labels,
                              int64_t prop_label_seg_stride, const int32_t* num_props,
                              const int32_t* num_gts, int64_t max_rows, int64_t* rows_out,
                              int64_t rows_seg_stride, int32_t* num_rows, void* stream);
size_t frh_bbox_target_workspace(int32_t num_segs, int64_t max_rows);
int32_t frh_bbox_target(int32_t num_segs, const int64_t* labels, int64_t label_seg_stride,
                        const int32_t* num_rows, const int32_t* num_gts, int64_t max_rows,
                        const float* props, int64_t prop_ld, int64_t prop_seg_stride,
                        const float* gts, int64_t gt_ld, int64_t gt_seg_stride,
                        const int64_t* gt_labels, int64_t gt_label_seg_stride,
                        const float* means, const float* stds, int64_t max_out_per_seg,
                        const int32_t* sel, const int32_t* sel_counts,
                        float* tar_props, float* tar_bbox, int64_t* tar_label,
                        float* tar_param, int64_t* tar_is_gt, int64_t out_ld,
                        int32_t* out_counts, void* workspace, size_t ws_bytes, void* stream);

/* ---- a7/a8: bbox2param / param2bbox (+clamp_bbox) ----------------------------
 * lib/utils.py:47-70 and 83-144.  param2bbox handles the batched
 * [4*ncls, n] layout of batched_param2bbox (utils.py:96-106): class c of
 * coordinate k is row k*ncls + c, output in the same layout.  clamp != 0
 * clamps x to [0, img_w-1] and y to [0, img_h-1] (utils.py:109-120). */
int32_t frh_bbox2param(const float* base, int64_t ldb, const float* bbox, int64_t ldx,
                       int64_t n, const float* means, const float* stds, float* out,
                       int64_t ldo, void* stream);
int32_t frh_param2bbox(const float* base, int64_t ldb, const float* param, int64_t ldp,
                       int64_t n, int32_t ncls, const float* means, const float* stds,
                       int32_t clamp, float img_h, float img_w, float* out, int64_t ldo,
                       void* stream);

/* ---- a9/a10: RPNHead.predict_single_image, all images x levels ----------------
 * lib/heads/rpn_head.py:68-120 with torchvision.ops.nms semantics.  Per
 * (image, level): score = sigmoid(cls) (use_sigmoid) or softmax(cls)[1];
 * top pre_nms by (score desc, index asc); decode+clamp (param2bbox); drop
 * boxes with w+1 < min_size or h+1 < min_size when min_size > 0; greedy NMS
 * (IoU > nms_iou in double); first post_nms.  Then per image the levels are
 * concatenated and, if more than max_num survive, the max_num best are kept
 * in (score desc, concat order) order.  cls level l: [B, C*A, H_l, W_l],
 * reg level l: [B, 4*A, H_l, W_l]; anchors [4, anchor_ld] from
 * frh_anchor_grid.  img_hw / min_size are host arrays [B*2] / [B].
 * Outputs: boxes [B, 4, max_num], scores [B, max_num], counts [B] (device).
 * status: the device status word (FRH_DEVERR_SELECT_BARRIER, FRH_DEVERR_NMS_COLUMN). */
size_t frh_rpn_proposals_workspace(int32_t num_imgs, int32_t num_levels,
                                   const int32_t* grid_hw, int32_t num_anchors,
                                   int32_t pre_nms);
int32_t frh_rpn_proposals(int32_t num_imgs, int32_t num_levels, const float* const* cls_ptrs,
                          const float* const* reg_ptrs, const int32_t* grid_hw,
                          int32_t num_anchors, int32_t cls_channels, const float* anchors,
                          int64_t anchor_ld, const float* means, const float* stds,
                          const float* img_hw, const float* min_size, int32_t pre_nms,
                          int32_t post_nms, int32_t max_num, double nms_iou, float* out_boxes,
                          float* out_scores, int32_t* out_counts, int32_t* status, void* workspace,
                          size_t ws_bytes, void* stream);

/* The same for head outputs of any layout (NCHW or the channels-last outputs of an NHWC
 * RPN head): cls_strides / reg_strides [L][4] element strides (b, c, y, x) of each level;
 * anchor a*H*W + y*W + x reads channel c*A + a (cls) / coord*A + a (reg), as the
 * reference's views (anchor_head.py:82, rpn_head.py:72). */
int32_t frh_rpn_proposals_strided(int32_t num_imgs, int32_t num_levels, const float* const* cls_ptrs,
                                  const float* const* reg_ptrs, const int64_t* cls_strides,
                                  const int64_t* reg_strides, const int32_t* grid_hw,
                                  int32_t num_anchors, int32_t cls_channels, const float* anchors,
                                  int64_t anchor_ld, const float* means, const float* stds,
                                  const float* img_hw, const float* min_size, int32_t pre_nms,
                                  int32_t post_nms, int32_t max_num, double nms_iou, float* out_boxes,
                                  float* out_scores, int32_t* out_counts, int32_t* status,
                                  void* workspace, size_t ws_bytes, void* stream);

/* Measurement hook: byte offsets in the frh_rpn_proposals workspace of its per-level
 * NMS input (out[0] boxes [S, P, 4] in descending-score order, out[1] counts [S]
 * int32), out[2] = P, out[3] = S = num_imgs * num_levels.  bench.py replays that
 * NMS alone for its roofline line. */
int32_t frh_rpn_proposals_nms_view(int32_t num_imgs, int32_t num_levels, const int32_t* grid_hw,
                                   int32_t num_anchors, int32_t pre_nms, int64_t* out);

/* ---- a10: torchvision.ops.nms on pre-sorted segments --------------------------
 * boxes [S, n_max, 4] row-major xyxy, already in descending-score order
 * (stable); count[s] valid rows, n_max <= 184320 (the offset-trick batched_nms of
 * lib/utils.py:211-221 runs one NMS over up to 1000 proposals x 20 classes).
 * keep[s, :] = kept row positions (ascending = score order), keep_counts[s].
 * max_keep >= 0 stops after that many.  Workspace: one upper-triangle suppression
 * mask of ceil(n_max / 64) column blocks per segment (512 B per 64x64 tile). */
size_t frh_nms_workspace(int32_t num_segs, int32_t n_max);
int32_t frh_nms_sorted(int32_t num_segs, const float* boxes, int64_t seg_stride,
                       const int32_t* counts, int32_t n_max, double iou_thr, int32_t max_keep,
                       int32_t* keep, int64_t keep_seg_stride, int32_t* keep_counts,
                       void* workspace, size_t ws_bytes, void* stream);

/* ---- a11: class-wise batched multiclass NMS ------------------------------------
 * Replaces utils.multiclass_nms + batched_nms (lib/utils.py:211-269), called per
 * image by anchor_head.py:207-262, fcos_head.py:566-627, bbox_head.py:122-146 --
 * here for B images at once, one NMS segment per (image, class).  Per image b:
 * boxes [n_max][4] (box_per_class = 0) or [n_max][4 * C] viewed (n, 4, C), scores
 * [n_max][C], optional score_factor [n_max] (or [n_max][C] with sf_per_class, official
 * mode) and row_valid [n_max] (0 = a row the reference removed before the call), rows
 * < num_rows[b] (device int32).
 * channel_mask [C] (device uint8) = the nms_channel set; mode 0 official (every
 * (row, class) pair), 1 strict (argmax class per row); pairs need score >=
 * min_score; the score is multiplied by score_factor after that test.
 * by_class = 1: one segment per (image, class); 0: one per image (the reference's
 * single pass; needed when a candidate coordinate is < 0).  Two calls, neither of
 * which allocates or synchronises: prepare (candidates + per-segment NMS mask
 * offsets) writes the device int32 info[4]: info[0] = the largest segment (limit
 * 65536), info[1] = 1 if a candidate coordinate is < 0 (with by_class = 1 the caller
 * then redoes prepare with by_class = 0), info[2] | info[3] << 32 = the NMS mask
 * tiles.  The caller copies info to the host, then calls finish (same mode /
 * by_class; scores needed in strict mode) with max_count = info[0], mask_tiles =
 * info[2..3] and an NMS workspace of frh_mcnms_nms_workspace(..., max_count,
 * mask_tiles) bytes: per-segment sort (score desc, candidate asc), torchvision nms per
 * segment, the keeps of all classes merged in (score desc, candidate asc) order, the
 * first max_num (<= 0: all) written to out_boxes [B][out_cap][4], out_scores
 * [B][out_cap], out_labels [B][out_cap] (the class index), out_counts [B] (device). */
size_t frh_mcnms_workspace(int32_t num_imgs, int32_t num_classes, int64_t n_max);
int32_t frh_mcnms_prepare(int32_t num_imgs, int32_t num_classes, int64_t n_max, const int32_t* num_rows,
                          const float* boxes, int64_t box_img_stride, int32_t box_per_class,
                          const float* scores, int64_t score_img_stride, const float* score_factor,
                          int64_t sf_img_stride, int32_t sf_per_class, const uint8_t* row_valid,
                          int64_t valid_img_stride, const uint8_t* channel_mask, int32_t mode,
                          int32_t by_class, float min_score, void* workspace, size_t ws_bytes,
                          int32_t* info, void* stream);
size_t frh_mcnms_nms_workspace(int32_t num_imgs, int32_t num_classes, int32_t max_count, int64_t mask_tiles);
int32_t frh_mcnms_finish(int32_t num_imgs, int32_t num_classes, int64_t n_max, int32_t max_count,
                         int64_t mask_tiles, const float* boxes, int64_t box_img_stride, int32_t box_per_class,
                         const float* scores, int64_t score_img_stride, int32_t mode, int32_t by_class,
                         double nms_iou, int32_t max_num, float* out_boxes, float* out_scores,
                         int64_t* out_labels, int32_t* out_counts, int64_t out_cap, void* workspace,
                         size_t ws_bytes, void* nms_ws, size_t nms_ws_bytes, void* stream);

/* ---- a13/a14: BasicRoIExtractor.map_rois_to_levels + RoIAlign ----------------
 * level = clamp(floor(log2(sqrt((x2-x1+1)(y2-y1+1))/finest_scale + 1e-6)),
 * 0, L-1) (lib/region.py:256-264).  rois [K,5] = (batch_idx, x1, y1, x2, y2)
 * (torchvision convention).  roi_levels == nullptr => every roi on level 0.
 * RoIAlign = torchvision legacy aligned=False semantics (lib/builder.py:9,
 * used at lib/region.py:250-276); feats[l] is [B, C, H_l, W_l] NCHW
 * (layout 0) or NHWC (layout 1, i.e. channels_last strides); out [K, C, ph, pw]. */
int32_t frh_roi_level_map(const float* rois, int64_t num_rois, float finest_scale,
                          int32_t num_levels, int64_t* levels, void* stream);
/* The RoI rows the extractor feeds RoIAlign: rois [K, 5] = (image b, x1, y1, x2, y2) for the
 * boxes of num_segs images (<= 64) concatenated in image order (the reference attaches the
 * index per image, region.py:266-269, in its per-image forward, :303-306), and with
 * num_levels > 1 their levels as frh_roi_level_map computes them (region.py:256-264).  seg_offsets: HOST array [num_segs + 1] of row offsets
 * (0, n_0, n_0 + n_1, ...).  Boxes are [4, box_ld] coordinate-major: image b's box j at column
 * j of boxes + b * box_seg_stride, or (flat != 0) at column offsets[b] + j of boxes. */
int32_t frh_roi_rows(int32_t num_segs, const float* boxes, int64_t box_ld, int64_t box_seg_stride,
                     int32_t flat, const int64_t* seg_offsets, float finest_scale, int32_t num_levels,
                     float* rois, int64_t* levels, void* stream);
/* frh_roi_rows for rows of a fixed capacity whose per-image counts stay on the device
 * (seg_counts[b], image b's rows back to back from column 0 of boxes, images in order; rows
 * past their total are padding rows of image 0): the RCNN targets' buffer consumed without a
 * host synchronisation on its size (num_rows = the capacity). */
int32_t frh_roi_rows_dev(int32_t num_segs, const float* boxes, int64_t box_ld, int64_t num_rows,
                         const int32_t* seg_counts, float finest_scale, int32_t num_levels,
                         float* rois, int64_t* levels, void* stream);
int32_t frh_roi_align_fwd(int32_t num_levels, const float* const* feats, const int32_t* feat_hw,
                          const float* scales, int32_t batch, int32_t channels, int32_t layout,
                          const float* rois, const int64_t* roi_levels, int64_t num_rois,
                          int32_t pooled_h, int32_t pooled_w, int32_t sampling_ratio,
                          int32_t aligned, float* out, void* stream);
int32_t frh_roi_align_bwd(int32_t num_levels, float* const* grad_feats, const int32_t* feat_hw,
                          const float* scales, int32_t batch, int32_t channels, int32_t layout,
                          const float* rois, const int64_t* roi_levels, int64_t num_rois,
                          int32_t pooled_h, int32_t pooled_w, int32_t sampling_ratio,
                          int32_t aligned, const float* grad_out, void* stream);
/* Same ops with explicit per-level element strides strides[4l..4l+3] =
 * (batch, channel, y, x): any dense or strided feature view (NCHW,
 * channels_last, the FPN's P5[..., ::2, ::2] extra level). */
int32_t frh_roi_align_fwd_strided(int32_t num_levels, const float* const* feats,
                                  const int32_t* feat_hw, const int64_t* strides,
                                  const float* scales, int32_t batch, int32_t channels,
                                  const float* rois, const int64_t* roi_levels, int64_t num_rois,
                                  int32_t pooled_h, int32_t pooled_w, int32_t sampling_ratio,
                                  int32_t aligned, float* out, void* stream);
/* Measurement entry (bench.py's roofline line): frh_roi_align_fwd_strided with the forward
 * kernel launched through hipExtLaunchKernel, which binds the two caller-created hipEvent_t
 * to the dispatch's own start and end timestamps (no extra stream packets).  span (nullable,
 * device, FRH_SPAN_SHARDS x FRH_SPAN_STRIDE u64, shard k's words {0, 1} initialised to
 * {UINT64_MAX, 0}): the kernel's own span on the GPU's 100 MHz s_memrealtime clock -- the
 * earliest wave start (min over shards of word 0) and the latest wave end (max of word 1);
 * one lane per wave records both with memory-side atomic min / max on its workgroup's shard. */
#define FRH_SPAN_SHARDS 256
#define FRH_SPAN_STRIDE 16
int32_t frh_roi_align_fwd_strided_timed(int32_t num_levels, const float* const* feats,
                                        const int32_t* feat_hw, const int64_t* strides,
                                        const float* scales, int32_t batch, int32_t channels,
                                        const float* rois, const int64_t* roi_levels,
                                        int64_t num_rois, int32_t pooled_h, int32_t pooled_w,
                                        int32_t sampling_ratio, int32_t aligned, float* out,
                                        void* start_event, void* stop_event, uint64_t* span,
                                        void* stream);
/* Backward of the strided forward: grad_feats (same strides) must be cleared by the
 * caller; contributions are added with float atomics (sampling 2, up to 8x8 bins:
 * one atomic per row run of a RoI's taps), so the summation order -- and the last
 * bits -- vary from run to run, as in torchvision's CUDA backward. */
int32_t frh_roi_align_bwd_strided(int32_t num_levels, float* const* grad_feats,
                                  const int32_t* feat_hw, const int64_t* strides,
                                  const float* scales, int32_t batch, int32_t channels,
                                  const float* rois, const int64_t* roi_levels, int64_t num_rois,
                                  int32_t pooled_h, int32_t pooled_w, int32_t sampling_ratio,
                                  int32_t aligned, const float* grad_out, void* stream);

/* Deterministic backward (parity runs; SURVEY §5 race detection): the gradient of
 * frh_roi_align_bwd_strided, accumulated in fixed point -- int64, each (RoI, row, column)
 * partial sum rounded once and added with integer atomics, which are associative -- so the
 * result is bit-identical across runs whatever order the RoIs are scheduled in (float atomics
 * reorder sums).  The unit is set per call from the gradient's own magnitude (ABI 3; was a
 * fixed 2^-40): 2^-(62 - hb - E) with max|grad_out| < 2^E and hb = ceil(log2(num_rois *
 * pooled_h * pooled_w)) -- the most any cell can receive is max|grad_out| * num_rois * bins, so
 * no accumulator can overflow, and the resolution is ~2^-(62 - hb) of the largest gradient
 * element (about 2^-46 at cfg2) whatever its scale.  A non-finite grad_out makes every
 * gradient element NaN.  acc_feats: per level an int64 buffer with the element strides of
 * grad_feats, zeroed by the caller; grad_feats (dense: every element is written) = acc * unit
 * rounded to f32.  scale_word: 4 bytes of caller-owned device memory (the call writes it: the
 * bits of max|grad_out|).  sampling_ratio 2 and up to 8 x 8 bins (the reference configs' 7 x 7). */
int32_t frh_roi_align_bwd_fixed(int32_t num_levels, float* const* grad_feats, int64_t* const* acc_feats,
                                const int32_t* feat_hw, const int64_t* strides, const float* scales,
                                int32_t batch, int32_t channels, const float* rois,
                                const int64_t* roi_levels, int64_t num_rois, int32_t pooled_h,
                                int32_t pooled_w, int32_t sampling_ratio, int32_t aligned,
                                const float* grad_out, uint32_t* scale_word, void* stream);

/* ---- RoIPool (torchvision.ops.RoIPool; C4 config configs/faster_rcnn_r50.py:26) --
 * feat [B, C, H, W] with element strides strides[0..3] = (b, c, y, x); rois
 * [K, 5]; out [K, C, ph, pw] + int32 argmax (flat y*W+x, -1 for empty bins). */
int32_t frh_roi_pool_fwd(const float* feat, const int64_t* strides, int32_t height, int32_t width,
                         int32_t channels, float spatial_scale, const float* rois, int64_t num_rois,
                         int32_t pooled_h, int32_t pooled_w, float* out, int32_t* argmax,
                         void* stream);
int32_t frh_roi_pool_bwd(float* grad_feat, const int64_t* strides, int32_t height, int32_t width,
                         int32_t channels, const float* rois, int64_t num_rois, int32_t pooled_h,
                         int32_t pooled_w, const float* grad_out, const int32_t* argmax, void* stream);

/* ---------------------------------------------------------------- a16 ATSS / LTRB targets
 * Replaces FCOSHead.single_image_targets_atss (lib/heads/fcos_head.py:283-368) with
 * topk_by_center (:106-116, row index by floor division), bbox2ltrb (:78-87),
 * positive_ltrb (:51-53), centerness (:56-59) and paint_value (:90-94), for all
 * images of a batch.  Levels: grid_hw[2l..2l+1] = (H_l, W_l), strides[l] (host arrays);
 * anchors [4, anchor_ld] f32 = one anchor per cell, levels concatenated (AnchorCreator
 * scale atss_cfg.scale, ratio 1).  gts [B][4][max_gts] f32 (segment stride gt_seg_stride),
 * num_gts [B] (device), gt_labels [B][max_gts] i64, img_hw [B][2] (device, img_shape h, w).
 * Outputs over the N level-concatenated cells: cls [B][N] i64 (-1 outside the painted
 * image, 0 background, label), reg [B][N][4] f32 ltrb (-1 when not positive),
 * ctr [B][N] f32 (-1 / 0 / centerness).  topk <= 16, num_levels <= 16.  Top-k ties
 * break by ascending cell index; the per-gt IoU mean / unbiased std use double sums. */
size_t frh_atss_workspace(int32_t batch, int32_t max_gts, int32_t num_levels, int32_t topk,
                          int64_t num_cells);
int32_t frh_atss_assign(int32_t batch, int32_t num_levels, const int32_t* grid_hw,
                        const float* strides, const float* anchors, int64_t anchor_ld,
                        const float* gts, int64_t gt_seg_stride, const int32_t* num_gts,
                        const int64_t* gt_labels, int32_t max_gts, const int32_t* img_hw,
                        int32_t topk, int64_t* cls, float* reg, float* ctr, void* workspace,
                        size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- a17 FCOS scale-range targets
 * Replaces FCOSHead.single_image_targets (lib/heads/fcos_head.py:371-416) with utils.sort_bbox
 * (lib/utils.py:362-366), bbox2ltrb (:78-87), positive_ltrb (:51-53), centerness (:56-59) and
 * paint_value (:90-94), for all images of a batch in ONE launch.  Levels, gts, num_gts,
 * gt_labels, img_hw and the three outputs exactly as frh_atss_assign takes and writes them;
 * scale_thr [num_levels + 1] (host): the head's level_scale_thr.  For cell (y, x) of level l with
 * centre (x*stride + stride/2, y*stride + stride/2), gt g matches when its four ltrb distances
 * are > 0 and scale_thr[l] <= max(ltrb) < scale_thr[l+1]; the cell's owner is the matching gt of
 * smallest area (x2-x1+1)*(y2-y1+1), the largest index among equal areas -- the gt the reference,
 * painting in descending-area order behind a stable sort, paints last.  The owner writes cls =
 * its label and reg = its ltrb (also outside the painted image area, as the reference does) and,
 * where the label is > 0, ctr = centerness(ltrb + 1e-6).  All f32 in the reference's operation
 * order: bit-exact.  num_gts[b] is clamped to [0, max_gts]; max_gts == 0 is legal (background
 * only).  No workspace. */
int32_t frh_fcos_assign(int32_t batch, int32_t num_levels, const int32_t* grid_hw,
                        const float* strides, const float* scale_thr, const float* gts,
                        int64_t gt_seg_stride, const int32_t* num_gts, const int64_t* gt_labels,
                        int32_t max_gts, const int32_t* img_hw, int64_t* cls, float* reg, float* ctr,
                        void* stream);

/* ---------------------------------------------------------------- a18 Guided Anchoring targets
 * Replaces GuidedAnchor.loc_target_single_image (lib/heads/guided_head.py:342-397) and the
 * painting of shape_target_single_image_v2 (:195-231), with paint_value / paint_bbox (:23-39) and
 * region.inside_grid_mask (lib/region.py:10-16), for all images of a batch in ONE launch.
 * Levels, gts, num_gts and img_hw exactly as frh_fcos_assign takes them; gt_levels [batch,
 * max_gts] i32: the level of each gt (region.map_gt2level, computed by the caller).  The region
 * of gt (x1, y1, x2, y2) at ratio r on a level of stride s is, in f32, w = (x2 - x1 + 1) * r,
 * cx = (x2 + x1) / 2 (h, cy likewise), (cx - w/2, cy - h/2, cx + w/2, cy + h/2) * (1 / s) rounded
 * half to even; it covers cell (y, x) when rx1 <= x <= rx2 and ry1 <= y <= ry2.  Per cell of
 * level l over the level-concatenated cells (N in all):
 *   loc [batch, N] i64: 1 if a gt of level l has its center_ratio region over the cell; else -1
 *     if a gt with |level - l| <= 1 has its ignore_ratio region over it; else 0 if y <
 *     min(H_l, int(img_h / s) + 1) and x < min(W_l, int(img_w / s) + 1); else -1.
 *   shape_mask [batch, N] i64 / shape_box [batch, N, 4] f32 (16-byte aligned): 1 and the box of
 *     the highest-index gt of level l whose shape_center_ratio region covers the cell; 0 and
 *     zeros elsewhere.
 * This is what the reference's three painting passes leave behind, bit for bit, PROVIDED every
 * gt coordinate is >= 0: a negative rounded edge is a negative slice index there and wraps
 * around the map, which is not reproduced.  num_gts[b] is clamped to [0, max_gts]; max_gts == 0
 * is legal.  No workspace. */
int32_t frh_ga_targets(int32_t batch, int32_t num_levels, const int32_t* grid_hw, const float* strides,
                       const float* gts, int64_t gt_seg_stride, const int32_t* num_gts,
                       const int32_t* gt_levels, int32_t max_gts, const int32_t* img_hw, float center_ratio,
                       float ignore_ratio, float shape_center_ratio, int64_t* loc, int64_t* shape_mask,
                       float* shape_box, void* stream);

/* ---------------------------------------------------------------- backbone epilogue
 * Frozen BatchNorm (+ residual) (+ ReLU) of the reference ResNet's bottlenecks
 * (lib/backbones.py:69-76 keeps every BN in eval mode; torchvision Bottleneck.forward):
 * y = act(x * s + b (+ skip)), s = gamma / sqrt(var + eps), b = beta - mean * s, per
 * channel; x / skip / y contiguous NCHW f32 [n, c, hw], 16-byte aligned, hw % 4 == 0;
 * gamma / beta may be NULL (1 / 0); y may alias x. */
int32_t frh_bn_act(const float* x, const float* skip, float* y, const float* gamma,
                   const float* beta, const float* mean, const float* var, float eps,
                   int64_t n, int32_t c, int64_t hw, int32_t relu, void* stream);

/* The ResNet stem's frozen BN + ReLU + max_pool2d(kernel 3, stride 2, padding 1)
 * (lib/backbones.py, ResNet stem) in one pass: y [n, c, (h - 1) / 2 + 1, w / 2] =
 * maxpool(act(x * s + b)); x contiguous NCHW f32 [n, c, h, w], w % 8 == 0, x / y 16-byte
 * aligned.  Equal to frh_bn_act followed by the max pool, bit for bit. */
int32_t frh_bn_act_maxpool(const float* x, float* y, const float* gamma, const float* beta, const float* mean,
                           const float* var, float eps, int64_t n, int32_t c, int32_t h, int32_t w, void* stream);

/* A bottleneck's 1x1 / stride-1 convolution with the frh_bn_act epilogue on the accumulator
 * (torchvision Bottleneck.forward: conv1 / conv3 / the stride-1 projection, each followed by
 * its frozen BN): y[n, co, p] = act((sum_ci w[co, ci] * x[n, ci, p]) * s[co] + b[co]
 * (+ skip[n, co, p])), s and b as in frh_bn_act; the raw conv output is never written.
 * x [n, cin, hw], skip / y [n, cout, hw] contiguous NCHW f32, w [cout, cin] contiguous, all
 * 16-byte aligned; hw % 4 == 0, cin % 16 == 0, cout % 64 == 0 (anything else: FRH_EINVAL);
 * gamma / beta may be NULL (1 / 0); mean == var == NULL: no BN (the raw convolution, plus
 * skip, plus ReLU); y must not alias x or skip.  One launch, no workspace.  The sum over ci
 * is an exact-f32 fmaf chain (f32 MFMA) in a fixed order: the same inputs give the same bits
 * on every launch, and given the same accumulator the epilogue gives frh_bn_act's bits. */
int32_t frh_conv1x1_bn_act(const float* x, const float* w, const float* skip, float* y, const float* gamma,
                           const float* beta, const float* mean, const float* var, float eps, int64_t n,
                           int32_t cin, int32_t cout, int64_t hw, int32_t relu, void* stream);

/* frh_conv1x1_bn_act with the frozen BN (+ ReLU when pre_relu) that precedes the convolution
 * (a bottleneck's bn2 in front of conv3) applied to x on its way into the GEMM: x is the raw
 * output of the previous convolution, x' = act(x * s_in[ci] + b_in[ci]) with s_in / b_in from
 * pre_gamma / pre_beta (may be NULL: 1 / 0) / pre_mean / pre_var / pre_eps as in frh_bn_act,
 * then frh_conv1x1_bn_act on x'.  Same conditions, plus cin <= 512.  The result is bit for
 * bit that of frh_bn_act followed by frh_conv1x1_bn_act; x' is never written. */
int32_t frh_conv1x1_bn_act_pre(const float* x, const float* w, const float* skip, float* y, const float* gamma,
                               const float* beta, const float* mean, const float* var, float eps,
                               const float* pre_gamma, const float* pre_beta, const float* pre_mean,
                               const float* pre_var, float pre_eps, int32_t pre_relu, int64_t n, int32_t cin,
                               int32_t cout, int64_t hw, int32_t relu, void* stream);

/* frh_conv1x1_bn_act for a 1x1 / stride-2 convolution (the bottleneck projections of stages 2
 * to 4): x [n, cin, h, wd] contiguous NCHW is read at its even rows and columns,
 * y / skip [n, cout, (h + 1) / 2, wd / 2].  wd % 8 == 0 (the output width a multiple of 4:
 * anything else FRH_EINVAL), the other conditions as frh_conv1x1_bn_act.  The result is bit
 * for bit that of frh_conv1x1_bn_act on a contiguous copy of x[:, :, ::2, ::2]. */
int32_t frh_conv1x1_s2_bn_act(const float* x, const float* w, const float* skip, float* y, const float* gamma,
                              const float* beta, const float* mean, const float* var, float eps, int64_t n,
                              int32_t cin, int32_t cout, int32_t h, int32_t wd, int32_t relu, void* stream);

/* The RPN head's classifier and regressor (lib/heads/rpn_head.py, RPNHead.forward: two 1x1
 * convolutions on every level of the pyramid) in one launch: for num_levels (1..8) inputs
 * xs[i] [n, level_hw[2i], level_hw[2i + 1], cin] f32 with channel stride 1 and element strides
 * level_strides[3i..] = (image, row, column; non-negative multiples of 4),
 * cls_outs[i][n, h, w, c_cls] = x . w_cls^T + b_cls and reg_outs[i][n, h, w, c_reg] =
 * x . w_reg^T + b_reg, both contiguous channels-last; w_cls [c_cls, cin], w_reg [c_reg, cin]
 * contiguous, the biases may be NULL.  cin % 8 == 0, cin <= 256, c_cls + c_reg <= 16, xs and
 * the weights 16-byte aligned (anything else: FRH_EINVAL).  Every input element is read once
 * and every output written once; each output is one exact-f32 fmaf chain (f32 MFMA) over cin
 * in one fixed order, then + bias, with no atomics: the bits depend neither on the level, nor
 * on the pixel, nor on what else is in the launch, nor on the launch. */
int32_t frh_rpn_head1x1_levels(int32_t num_levels, const void* const* xs, void* const* cls_outs,
                               void* const* reg_outs, const float* w_cls, const float* b_cls, const float* w_reg,
                               const float* b_reg, int64_t n, int32_t cin, int32_t c_cls, int32_t c_reg,
                               const int32_t* level_hw, const int64_t* level_strides, void* stream);

/* The FPN output convs and the RPN head's shared conv (lib/necks.py, FPN.forward;
 * lib/heads/rpn_head.py, RPNHead.forward): y = act(conv3x3(x, w) + bias), padding 1, stride 1,
 * no dilation, no groups, as Winograd F(2x2, 3x3) on the f32 MFMA with the bias / ReLU
 * epilogue on the accumulators (two launches: the weight transform into the workspace, which
 * is redone on every call, then the convolution).
 * x: f32 [n, h, wd, cin] with channel stride 1 and element strides sn / sy / sx (image, row,
 * column; multiples of 4, so a strided view such as P5[:, :, ::2, ::2] runs without a copy);
 * w: the channels-last Conv2d weight [cout][3][3][cin]; bias [cout] or NULL; y: contiguous
 * NHWC [n, h, wd, cout]; workspace: frh_conv3x3_workspace(cin, cout) bytes.  cin % 8 == 0,
 * cout % 64 == 0, every pointer 16-byte aligned, y not overlapping x or the workspace
 * (anything else: FRH_EINVAL); any h, wd >= 1.  The sums run in a fixed order with no atomics:
 * the same inputs give the same bits on every launch, and given the same pre-bias value the
 * epilogue gives frh_bias_act_nhwc's bits.
 * _levels: num_levels (1..8) inputs xs[i] [n, level_hw[2i], level_hw[2i + 1], cin] with
 * strides level_strides[3i..] = (sn, sy, sx), weights[i], biases[i] (entries may be NULL) and
 * outputs ys[i] in one weight-transform launch and one convolution launch.  Consecutive levels
 * with the same weights pointer share one transform; the workspace holds
 * frh_conv3x3_workspace(cin, cout) bytes per distinct weight.  Each level's bits are those of
 * its own frh_conv3x3_bias_act call. */
size_t frh_conv3x3_workspace(int32_t cin, int32_t cout);
int32_t frh_conv3x3_bias_act(const float* x, const float* w, const float* bias, float* y, float* workspace,
                             int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t wd, int64_t sn, int64_t sy,
                             int64_t sx, int32_t relu, void* stream);
int32_t frh_conv3x3_bias_act_levels(int32_t num_levels, const void* const* xs, const void* const* weights,
                                    const void* const* biases, void* const* ys, float* workspace,
                                    size_t workspace_bytes, int64_t n, int32_t cin, int32_t cout,
                                    const int32_t* level_hw, const int64_t* level_strides, int32_t relu,
                                    void* stream);

/* A VGG16 conv with the max pool behind it (lib/backbones.py:7-31, VGG16: torchvision's
 * features, Conv2d 3x3 + ReLU, MaxPool2d(2, 2) after layers 2, 4, 7, 10):
 * y = max_pool2d(act(conv3x3(x, w) + bias), kernel 2, stride 2), no padding, floor mode, in
 * frh_conv3x3_bias_act's launch pair with the pool in the epilogue: Winograd's 2 x 2 output
 * tiles start at even coordinates, so a lane holds a whole pool window in registers and stores
 * its largest value; the full-resolution map is never written.
 * Arguments and preconditions are frh_conv3x3_bias_act's (cin % 8 == 0, cout % 64 == 0, the
 * strides, 16-byte alignment, the workspace of frh_conv3x3_workspace; anything else
 * FRH_EINVAL), except y: contiguous NHWC [n, h / 2, wd / 2, cout] (integer division), which
 * must not overlap x or the workspace.  An odd last row or column takes part in the
 * convolution as a neighbour and is dropped by the pool.  h < 2, wd < 2 or n == 0: FRH_OK,
 * nothing is written.
 * Contract: for finite inputs the result is bit for bit torch.nn.functional.max_pool2d(., 2) of
 * frh_conv3x3_bias_act's output for the same arguments (the four values of a window are formed
 * by the same expressions in the same order; of equal values, -0 and +0 included, the first in
 * row-major window order is kept, as max_pool2d does).  Fixed summation order, no atomics: the
 * same bits on every launch.  Capturable: no synchronisation, no allocation, no global state. */
int32_t frh_conv3x3_bias_act_pool(const float* x, const float* w, const float* bias, float* y, float* workspace,
                                  int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t wd, int64_t sn,
                                  int64_t sy, int64_t sx, int32_t relu, void* stream);

/* VGG16's first layer (3 input channels) for the kernel above, whose cin is a multiple of 8:
 * x contiguous NCHW f32 [n, c, h, w], 1 <= c <= 8, to y contiguous NHWC [n, h, w, 8] with
 * channels >= c zero (exact zeros in every Winograd sum, so the conv's bits are those of a
 * c-channel sum).  One thread per pixel, two 16-byte stores.  Any h, w >= 0 (an empty tensor:
 * FRH_OK, no launch); x and y 16-byte aligned, y not overlapping x (anything else FRH_EINVAL). */
int32_t frh_nchw_to_nhwc8(const float* x, float* y, int64_t n, int32_t c, int32_t h, int32_t w, void* stream);

/* The prediction convs of a one-stage head (lib/heads/retina_head.py:87, RetinaHead.forward:
 * retina_cls / retina_reg; lib/heads/fcos_head.py:266-281, FCOSHead.forward: fcos_cls / fcos_reg /
 * fcos_center): 3x3, stride 1, padding 1, no groups, no dilation, over every level of the pyramid
 * in one launch, with no weight-transform launch and no workspace.  One conv (c1 == 0, w1 NULL)
 * or two that read the same input, each level read once for both.
 * Inputs: num_levels (1..8) levels xs[i] f32 [n, level_hw[2i], level_hw[2i + 1], cin] with channel
 * stride 1 and element strides level_strides[3i..] = (image, row, column; non-negative multiples
 * of 4, so a [:, :, ::2, ::2] view runs without a copy).  Weights: w0 [c0][3][3][cin] and w1
 * [c1][3][3][cin], the channels-last Conv2d weight as it lies in memory; b0 / b1 [c0] / [c1] or
 * NULL.  Outputs: ys0[i] [n, h_i, w_i, c0] and ys1[i] [n, h_i, w_i, c1], contiguous channels-last
 * (ys1 is not read when c1 == 0).  cin % 8 == 0, c0 >= 1, c0 + c1 <= 192, inputs and weights
 * 16-byte aligned, no output sharing a byte with an input or a weight (anything else:
 * FRH_EINVAL and no launch); a level with n, h or w zero launches nothing.
 * Epilogue of conv k, in this order, each statement rounded once (no contraction):
 * v = acc + bias; v = v * scales_k[i][c] where scales_k (an array of num_levels device pointers
 * to [c_k] floats) and its entry i are not NULL; v = expf(v) where exp_k != 0.  That is plain
 * logits, FCOS's exp(conv(x) * reg_coef[i]), and DFL's conv(x) * coef with
 * coef[bin * 4 + side] = reg_coef[i][bin].
 * A direct convolution on the exact-f32 MFMA (16x16x4), not Winograd: every output element is
 * one fmaf chain over its 9 * cin products in one fixed order (16-channel group, then tap, then
 * channel within the group), with no atomics and no split over cin.  The bits of an output
 * element depend on its inputs only: not on the level, the pixel's place in a tile, the other
 * conv or the other levels of the launch, nor on the launch.  Asynchronous on stream: no
 * synchronisation, allocation or global state (capturable into a hipGraph). */
int32_t frh_conv3x3_out_levels(int32_t num_levels, const void* const* xs, void* const* ys0, void* const* ys1,
                               const float* w0, const float* b0, const float* w1, const float* b1,
                               const void* const* scales0, const void* const* scales1, int32_t exp0, int32_t exp1,
                               int64_t n, int32_t cin, int32_t c0, int32_t c1, const int32_t* level_hw,
                               const int64_t* level_strides, void* stream);

/* A bottleneck's 3x3 / stride-1 / padding-1 convolution (torchvision Bottleneck.forward: conv2,
 * followed by its frozen BN and ReLU) as Winograd F(2x2, 3x3) on the f32 MFMA with the
 * frh_bn_act epilogue on the accumulators: y[n, co] = act(conv3x3(x[n], w[co]) * s[co] + b[co]),
 * zero padding, no dilation, no groups, no bias, s and b as in frh_bn_act.  Two launches: the
 * weight transform into the workspace, which is redone on every call (nothing is cached), then
 * the convolution.  x [n, cin, h, wd], y [n, cout, h, wd] contiguous NCHW f32; w the Conv2d
 * weight [cout, cin, 3, 3], contiguous; workspace: frh_conv3x3_nchw_workspace(cin, cout) bytes.
 * Any h; wd % 2 == 0 (rows are read and written as aligned float pairs), cin % 4 == 0,
 * cout % 16 == 0, cin * h * wd and cout * h * wd below 2^31, every pointer 16-byte aligned,
 * neither y nor the workspace sharing a byte with x or w, nor with each other (anything else:
 * FRH_EINVAL and no launch); n == 0 or an empty plane launches nothing.  gamma / beta may be
 * NULL (1 / 0); mean == var == NULL: no BN (the raw convolution, plus ReLU when relu).  The sum
 * over cin runs in ascending order with no atomics and no split: the same inputs give the same
 * bits on every launch, an image's bits do not depend on n, and with a BN the result is bit
 * for bit frh_bn_act applied to the raw output of the same entry. */
size_t frh_conv3x3_nchw_workspace(int32_t cin, int32_t cout);
int32_t frh_conv3x3_nchw_bn_act(const float* x, const float* w, const float* gamma, const float* beta,
                                const float* mean, const float* var, float eps, float* y, float* workspace,
                                int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t wd, int32_t relu,
                                void* stream);

/* The Double-Head regression branch's conv over RoI tiles (lib/heads/double_head.py:63-76,
 * 119-122: Conv2d(cin, cout, 3, padding=1, bias=False), BatchNorm2d in eval mode, ReLU):
 * y[i, co, p] = act((sum_ci sum_tap w[co, ci, tap] * x[i, ci, p + tap]) * s[co] + b[co]) over
 * each RoI's 7 x 7 tile with zero padding 1 and stride 1, s and b as in frh_bn_act; the raw
 * conv output is never written.  x [r, cin, 7, 7], y [r, cout, 7, 7] contiguous NCHW f32; w
 * the Conv2d weight [cout, cin, 3, 3], contiguous; workspace:
 * frh_roi_conv3x3_workspace(cin, cout) bytes (two launches: the weight repack into the
 * workspace, which is redone on every call, then the convolution).  cin % 16 == 0,
 * cout % 64 == 0, every pointer 16-byte aligned, y not overlapping x, w or the workspace
 * (anything else: FRH_EINVAL); r == 0 launches nothing.  gamma / beta may be NULL (1 / 0);
 * mean == var == NULL: no BN (the raw convolution, plus ReLU).  Each output is one exact-f32
 * fmaf chain (f32 MFMA) in a fixed order with no atomics: a RoI's bits depend neither on r,
 * nor on its index in the batch, nor on the launch, and given the same accumulator the
 * epilogue gives frh_bn_act's bits. */
size_t frh_roi_conv3x3_workspace(int32_t cin, int32_t cout);
int32_t frh_roi_conv3x3_bn_act(const float* x, const float* w, float* y, const float* gamma, const float* beta,
                               const float* mean, const float* var, float eps, int64_t r, int32_t cin,
                               int32_t cout, int32_t relu, float* workspace, void* stream);

/* The Guided Anchoring adaption layer (lib/heads/guided_head.py:92-96 offset_layer / adapt_layer,
 * :404-405 GuidedAnchor.forward: DeformConv(cin, cout, 3, padding=1, deformable_groups=dg) on the
 * offsets of a 1x1 conv of the shape map, then ReLU): a deformable (DCNv1, as mmdet v1's
 * mmdet.ops.dcn.DeformConv and torchvision's deform_conv2d define it) 3x3 / stride-1 / padding-1 /
 * dilation-1 convolution without bias, y = act(sum_{c, k} w[co, c, k] * sample(x, c, k)), as an
 * implicit GEMM on the f32 MFMA fed by a bilinear gather (two launches: the weight repack into
 * the workspace, which is redone on every call, then the convolution).
 * Input channel c is in deformable group g = c / (cin / dg).  Tap k = 3 (ky + 1) + (kx + 1),
 * ky, kx in {-1, 0, 1}, of group g at output (y, x) samples at (py, px) = (y + ky + dy,
 * x + kx + dx) with dy = offset channel g * 18 + 2 k and dx = channel g * 18 + 2 k + 1 at (y, x).
 * The sample is 0 unless -1 < py < h and -1 < px < wd; the test is made in float before any
 * conversion to an integer, so a non-finite or huge offset gives 0 and forms no address.
 * Otherwise it is bilinear from the four neighbours, ((hy hx) v00 + (hy lx) v01) + (ly hx) v10 +
 * (ly lx) v11 with ly = py - floor(py), hy = 1 - ly, neighbours outside the map contributing 0.
 * x: f32 [n, h, wd, cin] with channel stride 1 and element strides sn / sy / sx (image, row,
 * column; non-negative multiples of 4, sx >= cin, so P5[:, :, ::2, ::2] runs without a copy);
 * w: the weight [cout, cin, 3, 3], contiguous; y: contiguous NHWC [n, h, wd, cout]; workspace:
 * frh_deform_conv3x3_workspace(cin, cout) bytes.
 * offset_w == NULL (explicit): offset is f32 [n, 18 dg, h, wd] with the element strides
 * offset_strides[0..3] (image, channel, row, column; any values).
 * offset_w != NULL (guided): offset is the 2-channel shape map [n, 2, h, wd] with those
 * strides and offset_w the offset layer's weight [18 dg, 2], contiguous; offset channel c is
 * formed in registers as (offset_w[c][0] * s0) + (offset_w[c][1] * s1), in this f32 order -- the
 * bits of the 1x1 convolution without bias -- and the 18 dg-channel map is never written.  The
 * result is bit for bit that of the explicit mode on that map.
 * cin % 16 == 0, (cin / dg) % 4 == 0, cout % 64 == 0, x / y / w / workspace / offset_w 16-byte
 * aligned, y overlapping none of the other tensors (anything else: FRH_EINVAL); a level of 2^31
 * positions or more: FRH_EUNSUPPORTED; n == 0 launches nothing.  The sums run in one fixed
 * order (tap-major, then channel) with no atomics: the same inputs give the same bits on every
 * launch, and an image's bits depend neither on n nor on its index.
 * _levels: num_levels (1..8) inputs xs[i] [n, level_hw[2i], level_hw[2i + 1], cin] with strides
 * level_strides[3i..] = (sn, sy, sx), offsets[i] with offset_strides[4i..] and outputs ys[i],
 * sharing w and offset_w, in one repack launch and one convolution launch.  Each level's bits
 * are those of its own frh_deform_conv3x3_act call. */
size_t frh_deform_conv3x3_workspace(int32_t cin, int32_t cout);
int32_t frh_deform_conv3x3_act(const float* x, const float* offset, const float* offset_w, const float* w,
                               float* y, float* workspace, int64_t n, int32_t cin, int32_t cout, int32_t dg,
                               int32_t h, int32_t wd, int64_t sn, int64_t sy, int64_t sx,
                               const int64_t* offset_strides, int32_t relu, void* stream);
int32_t frh_deform_conv3x3_act_levels(int32_t num_levels, const void* const* xs, const void* const* offsets,
                                      const float* offset_w, const float* w, void* const* ys, float* workspace,
                                      int64_t n, int32_t cin, int32_t cout, int32_t dg, const int32_t* level_hw,
                                      const int64_t* level_strides, const int64_t* offset_strides, int32_t relu,
                                      void* stream);

/* The backward of frh_deform_conv3x3_act for one level, with that entry's definition, layouts
 * and sample-point arithmetic.  gy = dL/dy and y (the forward's output; NULL: the forward ran
 * without ReLU, otherwise gy counts only where y > 0) are contiguous NHWC [n, h, wd, cout].  With
 * S[n, c, k, p] the blended sample of input channel c, tap k at position p and
 * G[n, c, k, p] = sum_co w[co, c, k] gy[n, co, p]:
 *   gx   (NULL: skipped) contiguous NHWC [n, h, wd, cin], ACCUMULATED into -- the caller zeroes
 *        it: every G adds G (hy hx, hy lx, ly hx, ly lx) to its four neighbours;
 *   goff (NULL: skipped) [n, 18 dg, h, wd] contiguous, always the full offset map, also in the
 *        guided mode (the gradients of the shape map and of offset_w are two contractions of
 *        it): goff[n, g 18 + 2 k, p] = sum_{c in g} G (hx (v10 - v00) + lx (v11 - v01)), channel
 *        + 1 = sum_{c in g} G (hy (v01 - v00) + ly (v11 - v10)); floor has derivative 0, so at an
 *        integer coordinate this is the one-sided derivative;
 *   gw   (NULL: skipped) [cout, cin, 3, 3] = sum_{n, p} gy[n, co, p] S[n, c, k, p].
 * Neighbours outside the map count as 0 and receive nothing; where the forward's float range
 * test fails (a non-finite or huge offset included) no address is formed and the sample
 * contributes exact zeros to gx, goff and gw.  offset_w != NULL (guided): the offsets are
 * re-formed in registers exactly as the forward does, and goff is bit for bit that of the
 * explicit mode on that map.
 * Launches: the weight repack and the data launch (G on the f32 MFMA from a gy tile held in
 * LDS; gx with no-return float atomics, so its last bits depend on arrival order; goff summed
 * over a group's channels in a fixed order and stored once) when gx or goff is wanted; the
 * weight launch (per-position-split partial slabs in the workspace) and a reduce in split order
 * when gw is.  goff and gw are bit-identical from launch to launch.  workspace:
 * frh_deform_conv3x3_bwd_workspace(n, cin, cout, h, wd) bytes.
 * Checks as the forward's: cin % 16 == 0, (cin / dg) % 4 == 0, cout % 64 == 0, every pointer but
 * offset and goff 16-byte aligned, no output or workspace overlapping an input or another
 * output (anything else: FRH_EINVAL); 2^31 positions or more, or cout > 256 (the gy tile is 64 x
 * cout floats of LDS): FRH_EUNSUPPORTED; n == 0, or no output wanted, launches nothing. */
size_t frh_deform_conv3x3_bwd_workspace(int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t wd);
int32_t frh_deform_conv3x3_bwd(const float* x, const float* offset, const float* offset_w, const float* w,
                               const float* y, const float* gy, float* gx, float* goff, float* gw,
                               float* workspace, int64_t n, int32_t cin, int32_t cout, int32_t dg, int32_t h,
                               int32_t wd, int64_t sn, int64_t sy, int64_t sx, const int64_t* offset_strides,
                               void* stream);

/* FPN top-down merge into channels-last levels (lib/necks.py:72-84):
 * out[b, y, x, c] = (lat[b, c, y, x] + bias[c]) + up[b, iy, ix, c] with torch's nearest rule
 * (iy = min(floor(y * (float)up_h / height), up_h - 1); y / 2 when height == 2 * up_h);
 * lat: any strides (lat_strides = element strides b, c, y, x) -- the lateral conv's output
 * without its bias when bias ([channels]) is given, with it when bias is NULL; up: NHWC
 * contiguous [batch, up_h, up_w, channels] or NULL (the top level: a transpose); out: NHWC
 * contiguous [batch, height, width, channels].  f32 adds in that order (bit-identical to
 * the conv's bias add followed by the reference's upsample add). */
int32_t frh_fpn_merge_nhwc(const float* lat, const int64_t* lat_strides, const float* bias, const float* up,
                           int32_t up_h, int32_t up_w, float* out, int32_t batch, int32_t channels, int32_t height,
                           int32_t width, void* stream);

/* BFP neck, refine_type=None (lib/necks.py:93-141, BFP.forward): with r = refine_level,
 * refine = (sum over i != r, in level order, of [i < r: adaptive_max_pool2d(feats[i],
 * size_r); i > r: interpolate(feats[i], size_r, 'nearest')]) / (num_levels - 1) and
 * out[i] = feats[i] + [i < r: interpolate(refine, size_i, 'nearest'); i > r:
 * adaptive_max_pool2d(refine, size_i); i == r: refine], with torch's index rules (window
 * [floor(o*in/out), ceil((o+1)*in/out)), nearest min(floor(d * (float)in / out), in - 1)) and
 * its CPU maximum (row-major scan, `>` or NaN replaces).  Two launches; bit-identical to the
 * reference on the CPU.  2 <= num_levels <= FRH_MAX_LEVELS, any refine_level, any level
 * sizes up to 32767 (level_hw[2i], level_hw[2i+1] = H_i, W_i; host array), channels >= 1
 * (16-byte lanes when channels % 4 == 0 and strides / pointers allow, scalar otherwise).
 * feats[i] (host array of device pointers): f32 with element strides level_strides[4i..] =
 * (b, c, y, x), any layout; refine [batch, H_r, W_r, channels] and outs[i] NHWC contiguous.
 * argmax (nullable; frh_bfp_argmax_elems() int32 elements): the winning cell y*W + x of every
 * window, for frh_bfp_bwd.
 * Backward: grad_feats[i] (NHWC contiguous; entry refine_level is not written and may be
 * NULL: that gradient is grad_outs[refine_level] itself) from grad_outs[i] (strides
 * grad_strides), routing the max-pool gradients to the stored argmax cells (a cell that is
 * the argmax of several overlapping windows gets their sum); grad_refine [batch, H_r, W_r,
 * channels] is scratch.  Two launches, gathers in a fixed order: deterministic, no atomics. */
size_t frh_bfp_argmax_elems(int32_t num_levels, int32_t refine_level, int32_t batch, int32_t channels,
                            const int32_t* level_hw);
int32_t frh_bfp_fwd(int32_t num_levels, int32_t refine_level, int32_t batch, int32_t channels,
                    const void* const* feats, const int32_t* level_hw, const int64_t* level_strides,
                    float* refine, void* const* outs, int32_t* argmax, int64_t argmax_elems, void* stream);
int32_t frh_bfp_bwd(int32_t num_levels, int32_t refine_level, int32_t batch, int32_t channels,
                    const void* const* grad_outs, const int32_t* level_hw, const int64_t* grad_strides,
                    const int32_t* argmax, int64_t argmax_elems, float* grad_refine,
                    void* const* grad_feats, void* stream);

/* Conv epilogue on a channels-last map viewed as [rows, channels] (rows = batch * H * W):
 * y = relu ? max(y + bias[c], 0) : y + bias[c], in place -- the RPN head's
 * relu(conv(x)) (lib/heads/rpn_head.py, RPNHead.forward) after a bias-free NHWC conv, one
 * pass for PyTorch's bias add + ReLU.  channels % 4 == 0, y and bias 16-byte aligned. */
int32_t frh_bias_act_nhwc(float* y, const float* bias, int64_t rows, int32_t channels, int32_t relu, void* stream);

/* ---------------------------------------------------------------- f1: fused losses
 * Classification losses of lib/losses.py on the head outputs, summed (the reference's
 * reductions): kind 0 = sigmoid_focal_loss (losses.py:33-61, one-hot[:, 1:] targets),
 * 1 = CrossEntropyLoss(use_sigmoid=True) (losses.py:139-150; C == 1 takes the target
 * value itself, int64 or, with target_is_float, f32), 2 = CrossEntropyLoss softmax
 * (losses.py:151-153, labels in [0, C)).  alpha / gamma are read by kind 0 only; the supported
 * focal gamma is 0 or >= 1 (for 0 < gamma < 1 the derivative gamma * q^(gamma-1) is infinite
 * where the logit saturates, q = 1 - pt == 0, in torch as here; gamma == 0 drops that term,
 * as torch's pow backward does).  Logit (i, k) is x[i*sr + k*sc] (any strides,
 * so AnchorHead's [C, S] targets need no transpose copy); out is one f32 on the device.
 * status (nullable, ABI 3): the device status word; while it is nonzero the forward writes NaN.
 * Backward writes grad_x (i, k) at grad_x[i*gsr + k*gsc] = grad_out[0] * dL/dx.  Rows with an
 * int64 label < 0 (padding rows of a fixed-capacity target buffer) add nothing, gradient 0.
 * Callers: AnchorHead.calc_loss (anchor_head.py:113-139), BBoxHead.calc_loss
 * (bbox_head.py:56-87), FCOSHead losses (fcos_head.py:418-534). */
/* Forward workspace: frh_loss_workspace() bytes whose first 256 bytes (the arrival counter of
 * the in-launch finalisation) are zero before the first call; every call leaves them zero, so
 * a caller zero-fills the buffer once and reuses it for calls ordered on one stream. */
size_t frh_loss_workspace(void);
int32_t frh_cls_loss_fwd(int32_t kind, const float* x, int64_t n, int64_t c, int64_t sr,
                         int64_t sc, const void* target, int32_t target_is_float, float alpha,
                         float gamma, const int32_t* status, float* out, void* workspace,
                         size_t ws_bytes, void* stream);
int32_t frh_cls_loss_bwd(int32_t kind, const float* x, int64_t n, int64_t c, int64_t sr,
                         int64_t sc, const void* target, int32_t target_is_float, float alpha,
                         float gamma, const float* grad_out, float* grad_x, int64_t gsr,
                         int64_t gsc, void* stream);
/* smooth_l1_loss_v2 (losses.py:77-83) summed over rows i < n, columns j < m of
 * x(i, j) = x[i*xs_i + j*xs_j + label[i]*xs_l] against y[i*ys_i + j*ys_j].  label (optional)
 * masks rows with label <= 0 -- the reference's positive-row selection
 * (anchor_head.py:126-128, bbox_head.py:71-76) -- and, with xs_l != 0, picks the labelled
 * class's deltas (reg_out.view(-1, 4, C)[arange, :, label], bbox_head.py:70-72); labels
 * >= n_sel make the sum NaN.  Backward writes only the selected unmasked elements of
 * grad_x (zero-filled by the caller). */
int32_t frh_smooth_l1_fwd(const float* x, int64_t xs_i, int64_t xs_j, int64_t xs_l,
                          const float* y, int64_t ys_i, int64_t ys_j, const int64_t* label,
                          int64_t n, int64_t m, int64_t n_sel, float beta, const int32_t* status,
                          float* out, void* workspace, size_t ws_bytes, void* stream);
int32_t frh_smooth_l1_bwd(const float* x, int64_t xs_i, int64_t xs_j, int64_t xs_l,
                          const float* y, int64_t ys_i, int64_t ys_j, const int64_t* label,
                          int64_t n, int64_t m, int64_t n_sel, float beta,
                          const float* grad_out, float* grad_x, int64_t gs_i, int64_t gs_j,
                          int64_t gs_l, void* stream);
/* balanced_l1_loss (losses.py:158-180, BalancedL1Loss): frh_smooth_l1_fwd / _bwd with the
 * element, for d = |x - y| and b = e^(gamma / alpha) - 1,
 *   d < beta ? alpha / b * (b*d + 1) * log(b*d / beta + 1) - alpha*d : gamma*d + gamma / b - alpha*beta
 * (f32, in the reference's operation order) and its derivative times sign(x - y) backward.
 * Same strided access, label mask / class select, status word and workspace. */
int32_t frh_balanced_l1_fwd(const float* x, int64_t xs_i, int64_t xs_j, int64_t xs_l,
                            const float* y, int64_t ys_i, int64_t ys_j, const int64_t* label,
                            int64_t n, int64_t m, int64_t n_sel, float beta, float alpha, float gamma,
                            const int32_t* status, float* out, void* workspace, size_t ws_bytes,
                            void* stream);
int32_t frh_balanced_l1_bwd(const float* x, int64_t xs_i, int64_t xs_j, int64_t xs_l,
                            const float* y, int64_t ys_i, int64_t ys_j, const int64_t* label,
                            int64_t n, int64_t m, int64_t n_sel, float beta, float alpha, float gamma,
                            const float* grad_out, float* grad_x, int64_t gs_i, int64_t gs_j,
                            int64_t gs_l, void* stream);
/* One head's two losses in ONE launch, scaled as the heads scale them: out[0] =
 * (cls_sum * cls_weight) / cls_div, out[1] = (reg_sum * reg_weight) / reg_div (f32), cls_sum
 * as frh_cls_loss_fwd, reg_sum as frh_smooth_l1_fwd (both sums bit-identical to theirs).
 * Replaces `loss_cls(...) / avg_factor` and `loss_bbox.masked / class_selected(...) /
 * avg_factor` of AnchorHead.calc_loss (anchor_head.py:113-139) and BBoxHead.calc_loss
 * (bbox_head.py:56-87) with a sampler (avg_factor = the sample count, a host value).
 * Workspace as frh_cls_loss_fwd.  Backward: frh_cls_loss_bwd / frh_smooth_l1_bwd.
 * div_count (nullable): both divisors are this device int32 count instead (a fixed-capacity
 * target buffer consumed without a host sync; 0 gives zero losses, as the heads return). */
int32_t frh_det_loss_fwd(int32_t kind, const float* x, int64_t n, int64_t c, int64_t sr, int64_t sc,
                         const void* target, int32_t target_is_float, float alpha, float gamma,
                         float cls_weight, float cls_div, const float* rx, int64_t xs_i,
                         int64_t xs_j, int64_t xs_l, const float* ry, int64_t ys_i, int64_t ys_j,
                         const int64_t* label, int64_t rn, int64_t rm, int64_t n_sel, float beta,
                         float reg_weight, float reg_div, const int32_t* div_count,
                         const int32_t* status, float* out, void* workspace, size_t ws_bytes,
                         void* stream);

/* ---------------------------------------------------------------- f1b: GFL head losses
 * The three losses of the Generalized Focal Loss head (FCOSHead.calc_loss with QualityFocalLoss,
 * DistributionFocalLoss and GIoULoss: lib/heads/fcos_head.py:419-515 with lib/losses.py:13-30,
 * :221-282 and utils.elem_iou, lib/utils.py:174-182) of one batch in ONE launch, straight from
 * the head outputs: class logit (k, i) at cls[k*cls_sk + i*cls_si] (k < c), regression logit of
 * channel ch = bin*4 + side (fcos_head.py:231, :464) at reg[ch*reg_sc + i*reg_si], label [m]
 * int64 (-1 ignored, 0 negative, > 0 the class), ltrb [m, 4] f32 pixels; positions ordered
 * images outer, levels inner.  For a positive j (label > 0, counted on the device):
 * w_j = max_k sigmoid(cls(k, j)); y_s = (ltrb_s - reg_mean) / reg_std;
 *   DFL (losses.py:265-282) per side: left = trunc(clamp(y, 0, (bins-1)*stride) / stride),
 *     -(((left+1)*stride - y) * logsm[left] + (y - left*stride) * logsm[left+1]), / stride with
 *     norm_prob; summed, * dfl_weight / dfl_avg_factor.  The weight the reference passes in is
 *     unused there and here.
 *     DIVERGENCE: at left == bins-1 (y >= (bins-1)*stride) the reference indexes bin `bins` and
 *     raises IndexError; here that right-hand term is dropped and bin `bins` is never read.
 *   box (fcos_head.py:474-483): len_s = sum_b softmax(z_s)[b] * b*stride, boxes
 *     (-len_l, -len_t, len_r, len_b) against (-y_l, -y_t, y_r, y_b); giou_loss * w_j summed,
 *     * bbox_weight / num_pos.  q_j = their plain IoU (no +1).
 * QFL (losses.py:221-247) over every position with label >= 0 and class k: t = (label == k+1) ?
 * q : 0, |t - sigmoid(x)|^beta * bce_with_logits(x, t), summed, * cls_weight / num_pos.
 * out[4] = {cls_loss, dfl_loss, bbox_loss, (float)num_pos}; with no positive the sums are
 * divided by max(num_pos, 1) (the reference raises).  status / workspace as frh_cls_loss_fwd
 * (NaN losses while the status word is set); partial sums are finalised in a fixed order, no
 * float atomics: two calls on one input are bit-identical.  bins*4 > 64: FRH_EUNSUPPORTED.
 * Backward writes d(g[0]*cls_loss + g[1]*dfl_loss + g[2]*bbox_loss) / d logits: g [3] and
 * fwd_out (the forward's out) are device memory (no host sync); every element of grad_cls
 * (k, i) at grad_cls[k*gc_sk + i*gc_si] and grad_reg (ch, i) at grad_reg[ch*gr_sc + i*gr_si]
 * is written exactly once (0 at ignored positions / at non-positive positions); q and w are
 * constants, as the reference's detach()s make them. */
int32_t frh_gfl_loss_fwd(const float* cls, int64_t c, int64_t cls_sk, int64_t cls_si, const float* reg,
                         int32_t bins, int64_t reg_sc, int64_t reg_si, const int64_t* label,
                         const float* ltrb, int64_t m, float reg_mean, float reg_std, double stride,
                         int32_t norm_prob, float beta, float cls_weight, float dfl_weight,
                         float bbox_weight, float dfl_avg_factor, const int32_t* status, float* out,
                         void* workspace, size_t ws_bytes, void* stream);
int32_t frh_gfl_loss_bwd(const float* cls, int64_t c, int64_t cls_sk, int64_t cls_si, const float* reg,
                         int32_t bins, int64_t reg_sc, int64_t reg_si, const int64_t* label,
                         const float* ltrb, int64_t m, float reg_mean, float reg_std, double stride,
                         int32_t norm_prob, float beta, float cls_weight, float dfl_weight,
                         float bbox_weight, float dfl_avg_factor, const float* g, const float* fwd_out,
                         float* grad_cls, int64_t gc_sk, int64_t gc_si, float* grad_reg, int64_t gr_sc,
                         int64_t gr_si, void* stream);
/* f1c: the three losses of the FCOS head without GFL (FCOSHead.calc_loss's last arm,
 * fcos_head.py:419-515, which plain FCOS and ATSS-without-GFL both take; sigmoid_focal_loss
 * lib/losses.py:33-61, giou_loss :13-30, CrossEntropyLoss(use_sigmoid=True) on one channel
 * :144-147) of one batch in ONE launch, straight from the un-indexed head outputs: class logit
 * (k, i) at cls[k*cls_sk + i*cls_si] (k < c), ltrb prediction of side s (the head's exp output) at
 * reg[s*reg_ss + i*reg_si], centerness logit at ctr[i*ctr_si]; label [m] int64 (-1 ignored, 0
 * negative, > 0 the class), ltrb [m, 4] f32 pixels (16-byte aligned), ctr_t [m] f32.
 *   focal: every position with label >= 0 and every class k, the element frh_cls_loss_fwd kind 0
 *     sums (target label == k+1), * cls_weight / num_pos;
 *   box: positives (label > 0, counted on the device): y_s = (ltrb_s - reg_mean) / reg_std,
 *     giou_loss of (-p_l, -p_t, p_r, p_b) against (-y_l, -y_t, y_r, y_b), * ctr_t, summed,
 *     * bbox_weight / num_pos;
 *   centerness: positives, bce_with_logits(ctr, ctr_t) summed, * ctr_weight / num_pos.
 * out[4] = {cls_loss, bbox_loss, ctr_loss, (float)num_pos}.  DIVERGENCE: with no positive the
 * sums are divided by max(num_pos, 1); the reference divides by zero.  status / workspace /
 * determinism as frh_gfl_loss_fwd.  Backward writes d(g[0]*cls_loss + g[1]*bbox_loss +
 * g[2]*ctr_loss) / d(cls, reg, ctr): g [3] and fwd_out are device memory; every element of the
 * three gradients is written exactly once (0 at ignored / non-positive positions); the targets
 * are constants; a tie of GIoU's min / max gives each operand a half, as torch does. */
int32_t frh_fcos_loss_fwd(const float* cls, int64_t c, int64_t cls_sk, int64_t cls_si, const float* reg,
                          int64_t reg_ss, int64_t reg_si, const float* ctr, int64_t ctr_si,
                          const int64_t* label, const float* ltrb, const float* ctr_t, int64_t m,
                          float reg_mean, float reg_std, float alpha, float gamma, float cls_weight,
                          float bbox_weight, float ctr_weight, const int32_t* status, float* out,
                          void* workspace, size_t ws_bytes, void* stream);
int32_t frh_fcos_loss_bwd(const float* cls, int64_t c, int64_t cls_sk, int64_t cls_si, const float* reg,
                          int64_t reg_ss, int64_t reg_si, const float* ctr, int64_t ctr_si,
                          const int64_t* label, const float* ltrb, const float* ctr_t, int64_t m,
                          float reg_mean, float reg_std, float alpha, float gamma, float cls_weight,
                          float bbox_weight, float ctr_weight, const float* g, const float* fwd_out,
                          float* grad_cls, int64_t gc_sk, int64_t gc_si, float* grad_reg, int64_t gr_ss,
                          int64_t gr_si, float* grad_ctr, int64_t gt_si, void* stream);
/* The DFL ("integral") box decode of one level for a batch (FCOSHead.predict_single_image,
 * fcos_head.py:579-600 with ltrb2bbox :63-75 and utils.clamp_bbox, lib/utils.py:109-120):
 * reg [batch, 4*bins, h, w] f32 with element strides (sb, sc, sy, sx) -- any layout, channels-
 * last included; per side the softmax expectation sum_b p_b * b*stride, * reg_std + reg_mean;
 * the box around the cell centre (x*cell + cell/2, y*cell + cell/2), clamped to
 * [0, img_w-1] x [0, img_h-1]; boxes [batch, 4, h*w] contiguous.  bins*4 > 64: FRH_EUNSUPPORTED. */
int32_t frh_dfl_decode(const float* reg, int32_t batch, int32_t bins, int32_t h, int32_t w, int64_t sb,
                       int64_t sc, int64_t sy, int64_t sx, double stride, float reg_std, float reg_mean,
                       float cell, float img_h, float img_w, float* boxes, void* stream);

/* ---- dense-head candidates: the one-stage heads' NMS input for all images x levels ------
 * FCOSHead.predict_single_image (fcos_head.py:570-621) and AnchorHead.predict_single_image
 * (anchor_head.py:207-250) up to their multiclass NMS, in one memset and four launches
 * whatever num_imgs, num_levels and num_classes; no device-to-host copy, no in-launch wait
 * between workgroups (no device status word).
 * Segment (image b, level l) has n_l = A * H_l * W_l columns; column a*H*W + y*W + x reads
 * class channel c*A + a and reg channel coord*A + a, as frh_rpn_proposals_strided.
 * cls / reg / ctr_strides [L][4]: element strides (b, c, y, x) of each level (NCHW or
 * channels-last, no copy).  ctr_ptrs (with ctr_strides and out_factor) may be NULL.
 * mode:
 *  FRH_DENSE_DELTA  param2bbox(anchor, reg, means, stds) clamped to img_hw (frh_param2bbox's
 *                   arithmetic); anchors [4][anchor_ld] from frh_anchor_grid.  Every column is
 *                   a candidate; after the decode a row is invalid when min_size > 0 and
 *                   w + 1 < min_size or h + 1 < min_size.
 *  FRH_DENSE_LTRB   A = 1; ltrb = reg * reg_std + reg_mean around the cell centre
 *                   (x*s + s/2, y*s + s/2), s = cell_strides[l], clamped.  Only columns with
 *                   w + 1 > min_size and h + 1 > min_size are candidates (dropped BEFORE the
 *                   top-k); a segment with fewer than k_l of them ends in invalid rows.
 *  FRH_DENSE_DFL    as LTRB with, per side, the softmax expectation over `bins` x dfl_stride
 *                   (reg channel bin*4 + side, frh_dfl_decode's arithmetic with the bins summed
 *                   in one fixed tree order for every layout).  bins*4 > 64: FRH_EUNSUPPORTED.
 * Key of a column: max_c sigmoid(cls_c), times sigmoid(ctr) with centerness maps.  Per segment
 * the k_l = min(pre_nms, n_l) (n_l when pre_nms <= 0) largest keys are taken, ties to the
 * lowest column; a candidate whose key is exactly 0 is still a candidate.  k_l <= 16384.
 * Outputs (caller-owned, cap = sum_l k_l, level l's rows at offset sum_{l'<l} k_l' of every
 * image, in (key descending, column ascending) order): boxes [B, cap, 4] (16-byte aligned),
 * scores [B, cap, C] (the sigmoid of every class channel), factor [B, cap] (sigmoid(ctr)),
 * valid [B, cap] uint8, index [B, cap] int32 (the column within its level, -1 for invalid
 * rows).  Invalid rows hold zeros.  img_hw [B*2] / min_size [B]: host arrays, B <= 64. */
#define FRH_DENSE_DELTA 0
#define FRH_DENSE_LTRB 1
#define FRH_DENSE_DFL 2
size_t frh_dense_candidates_workspace(int32_t num_imgs, int32_t num_levels, const int32_t* grid_hw,
                                      int32_t num_anchors, int32_t pre_nms);
int32_t frh_dense_candidates(int32_t num_imgs, int32_t num_levels, const float* const* cls_ptrs,
                             const float* const* reg_ptrs, const float* const* ctr_ptrs,
                             const int64_t* cls_strides, const int64_t* reg_strides,
                             const int64_t* ctr_strides, const int32_t* grid_hw, int32_t num_anchors,
                             int32_t num_classes, int32_t mode, const float* anchors, int64_t anchor_ld,
                             const float* means, const float* stds, const float* cell_strides,
                             int32_t bins, double dfl_stride, float reg_std, float reg_mean,
                             const float* img_hw, const float* min_size, int32_t pre_nms,
                             float* out_boxes, float* out_scores, float* out_factor, uint8_t* out_valid,
                             int32_t* out_index, int64_t cap, void* workspace, size_t ws_bytes,
                             void* stream);

/* ---------------------------------------------------------------- f4: image pipeline
 * The train/test pipelines of configs/faster_rcnn_r50_fpn.py:120-139 (mmdet v1: Resize
 * keep_ratio -> RandomFlip -> Normalize -> Pad(size_divisor) -> DefaultFormatBundle ->
 * collate), fused: src holds uint8 HWC 3-channel images (image b at byte offset
 * src_offsets[b], size src_hw[2b..2b+1] = h, w; host arrays); each is resized to
 * dst_hw[b] with cv2.resize INTER_LINEAR's fixed-point arithmetic (exact 2x downscale:
 * INTER_AREA), flipped horizontally when flip[b] (may be NULL), normalised
 * (v - mean[c]) / std[c] in f32 (channels reversed first when to_rgb), and written to
 * dst [batch][3][out_h][out_w] f32 with zeros outside [0, dst_h) x [0, dst_w).  The host
 * side (lib-mirror frcnn_amd.datasets) computes the sizes, scale factors, box transforms
 * and img_meta exactly as mmcv/mmdet do. */
int32_t frh_image_preprocess(const uint8_t* src, int32_t batch, const int64_t* src_offsets,
                             const int32_t* src_hw, const int32_t* dst_hw, const int32_t* flip,
                             const float* mean, const float* std, int32_t to_rgb, float* dst,
                             int32_t out_h, int32_t out_w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_AMD_H */
