"""Local evaluation of the result records the models write: one AP evaluation (ap_eval.py) under COCO AP (coco_eval.py)
and YTVIS AP (ytvis_eval.py)."""
from .ap_eval import STAT_NAMES  # noqa: F401
from .coco_eval import COCOEval, COCOEvaluator  # noqa: F401
from .ytvis_eval import YTVISEval, YTVISEvaluator  # noqa: F401
