"""prob_mbrl.models.activations (models/activations.py): Swish, Exp, Sin, SinLU, hhSinLU."""
from prob_mbrl_amd.activations import Exp, Sin, SinLU, Swish, hhSinLU  # noqa: F401
