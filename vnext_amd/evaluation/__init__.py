"""Local evaluation of the result records the models write (YTVIS AP: ytvis_eval.py; COCO AP: coco_eval.py)."""
from .coco_eval import COCOEval, COCOEvaluator  # noqa: F401
from .ytvis_eval import STAT_NAMES, YTVISEval, YTVISEvaluator  # noqa: F401
