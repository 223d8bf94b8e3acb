"""Local evaluation of the result records the models write (YTVIS AP: ytvis_eval.py)."""
from .ytvis_eval import STAT_NAMES, YTVISEval, YTVISEvaluator  # noqa: F401
