"""prob_mbrl.models.activations (models/activations.py: Swish :4-6; the other activations there are not offered)."""
from prob_mbrl_amd.activations import Swish  # noqa: F401
