"""mmsa -- MI355X-native image-encoder forward of Multimodal-SAM-Adapter behind the reference's mmseg backbone API.

Importing this package loads libmmsa_hip.so (hard requirement; no CPU fallback) and registers the backbone
classes under the reference's names."""
from . import lib  # noqa: F401  (raises if the HIP library is missing)
from . import ops  # noqa: F401
from . import inference  # noqa: F401  (encode_decode / slide_inference / argmax map of the reference's EncoderDecoder)
from .inference import AugPlan, aug_class_map, aug_inference, probabilities  # noqa: F401  (test-time augmentation: aug_test)
from .inference import argmax_max_map  # noqa: F401  (class map + confidence map of a probability canvas)
from .inference import argmax_score_map  # noqa: F401  (class map + uncertainty map -- top-2 margin or entropy score -- of a probability canvas)
from .inference import TopK, argmax_topk_map  # noqa: F401  (the first K classes of every pixel and their probabilities, as rank-major planes)
from .backbone import OperandRangeError, SAMAdapterbimodalMixModNewInTwinConvNEW, SAMAdapterbimodalMixModNewInTwinConvNEWwithcp
from .head import SegformerHead
from .chains import AttentionRangeError, Chains, Replay
from . import preprocess  # noqa: F401  (raw frames -> normalised NCHW, whole or as windows; FrameFeeder)
from .preprocess import FrameFeeder, Preprocess
from . import evaluate  # noqa: F401  (confusion counts and mIoU on device: LabelPrep, confusion, Evaluator)
from .evaluate import Evaluator, LabelPrep, confusion
from .evaluate import Calibration, calibration  # noqa: F401  (reliability bins, ECE and risk-coverage of the confidence map on device)
from .evaluate import SelectiveEvaluator, selective, abstain  # noqa: F401  (confusion counts per confidence bin: mIoU against coverage; the thresholded map)
from .evaluate import TemperatureSweep, temperature_sweep  # noqa: F401  (temperature scaling: NLL and reliability bins of a logits canvas over a grid of T)
from .evaluate import TopKEvaluator, topk_counts  # noqa: F401  (the rank of the label's class in a top-k map: top-k pixel accuracy and recall@k)
from .evaluate import BoundaryEvaluator, boundary_counts, boundary_zone_sum_of, trimap_counts_of, boundary_iou_of  # noqa: F401  (confusion counts by nearness to a label / prediction boundary: trimap metrics and Boundary IoU)
from .evaluate import (EuclideanBoundaryEvaluator, boundary_distance, boundary_counts_d2, boundary_displacement, boundary_f_of,  # noqa: F401  (exact distance
                       boundary_f_curve_of, boundary_distance_percentile_of)  # maps of the code maps: Euclidean bands up to 255 pixels, boundary F-score, Hausdorff percentiles)
from .evaluate import (SegmentEvaluator, components, component_areas, suppress_small, segment_counts, segment_totals_of,  # noqa: F401  (connected components
                       segment_rate_of, segment_f_of)  # of the code maps: segment recall and precision by class and size, and the map without its small blobs)
from .evaluate import (PanopticEvaluator, PairTable, segment_pairs, panoptic_counts, panoptic_quality_of,  # noqa: F401  (segments matched by IoU > 1/2:
                       panoptic_summary_of)  # the pair table of two root maps, TP / FP / FN and the IoU sum by class and size, PQ / SQ / RQ)
from .evaluate import SegmentTable, segment_table, select_segments, segment_records_of  # noqa: F401  (the segments handed out: dense ids, and one record
#                                                            per segment -- class, area, box, centroid, mean score -- by a prefix sum over the root pixels)
from .evaluate import SegmentTracker, track_pairs, track_records_of, track_summary_of  # noqa: F401  (the segments of a stream followed across frames:
#                                                            persistent track ids by IoU > 1/2 against the previous frame, new ids in raster order)
from .evaluate import (RunTable, run_lengths, run_decode, runs_of_value, coco_rle_of, rle_area_of, rle_bbox_of)  # noqa: F401  (run-length tables of a class
#                                                            map or an ids map, row-major or column-major, and the uncompressed COCO RLE of one id or class)
from .evaluate import fill_nearest  # noqa: F401  (the holes of a class map filled from the nearest kept pixel: what suppress_small / select_segments / abstain removed)
from .evaluate import majority_filter  # noqa: F401  (the majority filter of a class map: every target pixel takes the most frequent class of its window)
from .evaluate import vote_filter  # noqa: F401  (the guided vote filter: the majority filter with votes weighted by a guide frame and by the confidence)
from . import render  # noqa: F401  (the picture of a prediction on device: palette map over the frame, show_result)
from .render import Renderer
from .registry import BACKBONES, HEADS, build_backbone, build_head

for _cls in (SAMAdapterbimodalMixModNewInTwinConvNEW, SAMAdapterbimodalMixModNewInTwinConvNEWwithcp):
    BACKBONES.register_module(force=True)(_cls)



def register_head():
    """Register this package's SegformerHead under the reference's name in HEADS (segformer_head.py:11 registers with force=True
    as well).  With mmseg installed this is OPT-IN: the backbone alone is the drop-in of BASELINE's path and the reference's own
    head keeps working behind it; an import-time override would depend on whether mmseg_custom is imported before or after mmsa."""
    HEADS.register_module(force=True)(SegformerHead)
    return SegformerHead


from .registry import HAVE_MMSEG as _HAVE_MMSEG  # noqa: E402

if not _HAVE_MMSEG:     # local registry (no mmseg in the process): nothing to override, mmsa.build_head works out of the box
    register_head()

__all__ = ["SegformerHead", "HEADS", "build_head", "register_head", "SAMAdapterbimodalMixModNewInTwinConvNEW", "SAMAdapterbimodalMixModNewInTwinConvNEWwithcp",
           "BACKBONES", "build_backbone", "ops", "lib", "inference", "Chains", "Replay", "AttentionRangeError", "OperandRangeError",
           "preprocess", "Preprocess", "FrameFeeder", "evaluate", "Evaluator", "LabelPrep", "confusion", "Calibration", "calibration", "SelectiveEvaluator", "selective", "abstain", "TemperatureSweep", "temperature_sweep", "render", "Renderer",
           "probabilities", "aug_inference", "aug_class_map", "AugPlan", "argmax_max_map", "argmax_score_map", "TopK", "argmax_topk_map",
           "TopKEvaluator", "topk_counts", "BoundaryEvaluator", "boundary_counts", "boundary_zone_sum_of", "trimap_counts_of", "boundary_iou_of",
           "EuclideanBoundaryEvaluator", "boundary_distance", "boundary_counts_d2", "boundary_displacement", "boundary_f_of", "boundary_f_curve_of",
           "boundary_distance_percentile_of", "SegmentEvaluator", "components", "component_areas", "suppress_small", "segment_counts", "segment_totals_of",
           "segment_rate_of", "segment_f_of", "PanopticEvaluator", "PairTable", "segment_pairs", "panoptic_counts", "panoptic_quality_of",
           "panoptic_summary_of", "SegmentTable", "segment_table", "select_segments", "segment_records_of", "RunTable", "run_lengths",
           "run_decode", "runs_of_value", "coco_rle_of", "rle_area_of", "rle_bbox_of", "fill_nearest", "majority_filter", "vote_filter", "SegmentTracker",
           "track_pairs", "track_records_of", "track_summary_of"]
