/* ABI version of include/mmsa.h (its own header so that the library's sources can include it without the declarations).
 * Bumped whenever an entry point changes its arguments or their meaning.  101 (round 5): round 4 added arguments to mmsa_gemm_split3,
 * mmsa_convnext_mlp_fused and the attention entries and removed mmsa_gemm_next_extras / mmsa_debug_*_flavour / mmsa_dwconv7_ln without bumping it.
 * 102 (round 6): mmsa_convnext_mlp_fused takes clamp_max; new entry mmsa_msda_fused_planes.
 * 103: mmsa_gemm_split3's `fmt` accepts MMSA_FMT_W8 (fp8 weights against h8c activation planes).
 * 104: new entries mmsa_preprocess_nhwc / mmsa_preprocess_crops (raw HWC frames -> normalised NCHW, whole or as windows).
 * 105: new entries mmsa_preprocess_resize_nhwc / mmsa_preprocess_resize_crops (the same from sources of another size: bilinear resize first).
 * 106: new entries mmsa_eval_confusion_u8 / mmsa_slide_argmax_eval (confusion counts of a class map against a label map, alone or fused into the class-map kernel).
 * 107: new entry mmsa_gfe_qkv_conv (the GFE's 1x1 and 3x3 qkv convs as one grouped 3x3 conv with folded weights).
 * 108: new entries mmsa_render_u8 / mmsa_render_denorm_f32 (the picture of a prediction: palette map blended over nothing, the raw frame or the de-normalised input tensor).
 * 109: new entry mmsa_slide_argmax_resized (the class map at a rescaled size: second bilinear resize + crop + argmax in the class-map pass).
 * 110: new entries mmsa_softmax_flip_accum_nchw / mmsa_aug_argmax (test-time augmentation: softmax, un-flip, mean over the views and argmax, as a canvas step or in one launch).
 * 111: new entries mmsa_argmax_max_nchw / mmsa_slide_argmax_conf / mmsa_slide_argmax_resized_conf / mmsa_aug_argmax_conf (the confidence map, max class probability, next to every class map).
 * 112: new entry mmsa_eval_calibration (reliability bins of a class map and its confidence map against a label map: total / correct / confidence sum per bin).
 * 113: new entries mmsa_eval_selective / mmsa_abstain_u8 (one confusion matrix per confidence bin of a class map and its confidence map, and the map thresholded by confidence bin).
 * 114: new entries mmsa_slide_argmax_conf_t / mmsa_slide_argmax_resized_conf_t / mmsa_softmax_flip_accum_nchw_t (the confidence of softmax(x / T)) and
 *      mmsa_temperature_sweep_nchw (reliability bins and NLL of a logits canvas for a grid of temperatures in one pass).
 *      Still 114: new entries mmsa_argmax_score_nchw / mmsa_slide_argmax_score / mmsa_slide_argmax_resized_score (the top-2 margin or the entropy score in the
 *      confidence's place).  No existing entry changed its arguments or their meaning, and a library without the new symbols fails the binding's symbol lookup
 *      (mmsa/lib.py) before the number is read, so the number that tests/test_temperature_cpu.py pins stays.
 *      Still 114, for the same reason: new entries mmsa_slide_argmax_topk / mmsa_argmax_topk_nchw / mmsa_eval_topk_u8 (the first K classes of every pixel and
 *      their probabilities as rank-major planes, and the rank of the label's class counted per class).
 *      Still 114, for the same reason: new entry mmsa_eval_boundary_u8 (the confusion counts of a class map split by whether the pixel lies within a Chebyshev
 *      radius of a label boundary and of a prediction boundary: trimap metrics and Boundary IoU).
 *      Still 114, for the same reason: new entries mmsa_render_labels_u8 / mmsa_render_values_f32 / mmsa_render_band_u8 (the diagnostic pictures: the ground
 *      truth and the wrong pixels, a heat map of any float32 score and the abstained pixels, the boundary band, each one paint per pixel from a packed table
 *      and the blend of mmsa_render_u8).
 *      Still 114, for the same reason: new entries mmsa_boundary_distance_u8 / mmsa_eval_boundary_d2 / mmsa_eval_boundary_displacement (the exact squared
 *      Euclidean distance map of a code map, the boundary counts at a Euclidean radius from two such maps, and the displacement histogram of the two contours:
 *      boundary F-score and Hausdorff percentiles).
 *      Still 114, for the same reason: new entries mmsa_components_u8 / mmsa_component_area / mmsa_suppress_small_u8 / mmsa_eval_segments (the connected
 *      components of a code map as the smallest linear index of each, their areas, the class map without its small blobs, and the segment counts of a
 *      prediction against the ground truth by class, size bucket and coverage bin: segment recall and precision).
 *      Still 114, for the same reason: new entries mmsa_segment_table / mmsa_segment_table_block / mmsa_select_segments_u8 (the segments of a code map handed out: dense ids in raster
 *      order of the first pixel by a device-wide prefix sum, one record per segment -- class, area, box, coordinate sums, fixed-point score sum -- and the
 *      class map with chosen segments painted over).
 *      Still 114, for the same reason: new entries mmsa_run_lengths_u8 / mmsa_run_lengths_i32 / mmsa_run_lengths_block / mmsa_run_decode_i32 (the runs of a
 *      class map or an ids map in row-major or column-major order -- starts and values in ascending order by a device-wide prefix sum over the run heads --
 *      and the map of such a table).
 *      Still 114, for the same reason: new entry mmsa_fill_nearest_u8 (the holes of a byte map filled with the value of the nearest source pixel within a cap
 *      of up to 255 pixels, ties to the topmost and then the leftmost, and the squared distance taken).
 *      Still 114, for the same reason: new entry mmsa_majority_filter_u8 (the majority filter of a byte map: every target pixel takes the most frequent voter
 *      value of its (2 r + 1) x (2 r + 1) window, ties kept by the own value or else resolved to the smallest, and the count that won).
 *      Still 114, for the same reason: new entry mmsa_vote_filter_u8 (the guided vote filter of a byte map: the majority filter with every vote weighted by a
 *      range table of the guide frame's L1 difference and by the voter's quantised confidence, and the sum that won).
 *      Still 114, for the same reason: new entries mmsa_track_pairs / mmsa_track_update / mmsa_track_trip (the segments of a stream tracked across frames:
 *      the intersections of current and previous segments in the pair table of segment_pairs, and the association by IoU > 1/2 that hands every segment a
 *      persistent track id, its age and its predecessor, with new ids in raster order of the first pixel). */
#ifndef MMSA_VERSION_H
#define MMSA_VERSION_H
#define MMSA_ABI_VERSION 114
#endif
