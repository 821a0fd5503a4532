"""Scoring of `PascoNet.step_inference` outputs against SemanticKITTI ground truth: the reference's SSC (P / R / IoU / mIoU),
panoptic (PQ-dagger, PQ, SQ, RQ, per class) and calibration (ins / mask / ssc ECE and NLL) tables, with the passes over voxels
in HIP (include/pasco_eval.h, csrc/eval.hip)."""
from .gt import GroundTruth
from .metrics import CLASS_NAMES, THING_IDS, SceneEvaluator, calibration_error, panoptic_rows

__all__ = ["GroundTruth", "SceneEvaluator", "calibration_error", "panoptic_rows", "CLASS_NAMES", "THING_IDS"]
