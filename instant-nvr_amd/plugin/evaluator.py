"""`cfg.evaluator_module` target: exports `Evaluator` (lib/evaluators/make_evaluator.py:5-8)."""
from . import _config  # noqa: F401
from ..evaluator import Evaluator  # noqa: F401
