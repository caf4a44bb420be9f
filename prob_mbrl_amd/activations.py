"""Hidden-layer activations of the device path (models/activations.py of the reference).

`mlp(..., nonlin=...)` takes torch.nn.ReLU, torch.nn.Tanh, torch.nn.SiLU or Swish below; one activation for all hidden
layers of a network.  The modules only mark the choice: the layers run inside the kernels (include/pmbrl.h, PMBRL_ACT_*)."""
import torch

RELU, TANH, SILU = 0, 1, 2                       # PMBRL_ACT_*
NAMES = {'relu': RELU, 'tanh': TANH, 'silu': SILU}
OFFERED = 'torch.nn.ReLU, torch.nn.Tanh and torch.nn.SiLU / prob_mbrl_amd.activations.Swish'


class Swish(torch.nn.Module):
    """x * sigmoid(x) (models/activations.py:4-6) -- torch.nn.SiLU under the reference's name."""

    def forward(self, x):
        return x * x.sigmoid()


def code_of(module):
    """PMBRL_ACT_* of an activation module, or None if it is not one the device path offers."""
    if isinstance(module, torch.nn.ReLU):
        return RELU
    if isinstance(module, torch.nn.Tanh):
        return TANH
    if isinstance(module, (torch.nn.SiLU, Swish)):
        return SILU
    return None


def module_of(name):
    """The module class for 'relu' | 'tanh' | 'silu' (command-line switches)."""
    return {'relu': torch.nn.ReLU, 'tanh': torch.nn.Tanh, 'silu': Swish}[name]
