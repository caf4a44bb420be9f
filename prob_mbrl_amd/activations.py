"""Hidden-layer activations of the device path (models/activations.py of the reference).

`mlp(..., nonlin=...)` takes torch.nn.ReLU, torch.nn.Tanh, torch.nn.SiLU or one of Swish, Exp, Sin, SinLU, hhSinLU below --
one for all hidden layers, or a list with one entry per hidden layer; an entry that is not callable (None) means no
activation on that layer.  The modules only mark the choice: the layers run inside the kernels (include/pmbrl.h,
PMBRL_ACT_*)."""
import torch

RELU, TANH, SILU, SIN, EXP, SINLU, HHSINLU, NONE = range(8)      # PMBRL_ACT_*
PER_LAYER = 1 << 30                                               # PMBRL_ACT_PER_LAYER
MAX_HIDDEN = 7                                                    # PMBRL_MAX_LAYERS - 1
NAMES = {'relu': RELU, 'tanh': TANH, 'silu': SILU, 'sin': SIN, 'exp': EXP, 'sinlu': SINLU, 'hhsinlu': HHSINLU,
         'none': NONE}
OFFERED = ('torch.nn.ReLU, torch.nn.Tanh, torch.nn.SiLU / prob_mbrl_amd.activations.Swish and '
           'prob_mbrl_amd.activations.Exp, Sin, SinLU, hhSinLU, one per hidden layer (None: no activation on that layer)')


class Swish(torch.nn.Module):
    """x * sigmoid(x) (models/activations.py:4-6) -- torch.nn.SiLU under the reference's name."""

    def forward(self, x):
        return x * x.sigmoid()


class Exp(torch.nn.Module):
    """exp(-x^2 / 2) (models/activations.py:9-11)."""

    def forward(self, x):
        return torch.exp(-0.5 * x * x)


class Sin(torch.nn.Module):
    """sin(x) (models/activations.py:14-16)."""

    def forward(self, x):
        return torch.sin(x)


class SinLU(torch.nn.Module):
    """x where x > 0, sin(x) elsewhere (models/activations.py:19-25)."""

    def forward(self, x):
        return torch.where(x > 0, x, torch.sin(x))


class hhSinLU(torch.nn.Module):
    """Half sine, half ReLU, on x with the sign of every even unit flipped (models/activations.py:28-39): unit j of n
    takes sin(s_j x) for j < ceil(n / 2) and relu(s_j x) behind, s_j = -1 for even j and +1 for odd j."""

    def forward(self, x):
        n = x.shape[-1]
        j = torch.arange(n, device=x.device)
        sx = x * (2 * (j % 2) - 1).to(x.dtype)
        return torch.where(j < (n + 1) // 2, torch.sin(sx), torch.relu(sx))


_MODULES = {'relu': torch.nn.ReLU, 'tanh': torch.nn.Tanh, 'silu': Swish, 'sin': Sin, 'exp': Exp, 'sinlu': SinLU,
            'hhsinlu': hhSinLU, 'none': None}


def code_of(module):
    """PMBRL_ACT_* of an activation module, or None if it is not one the device path offers."""
    for cls, code in ((torch.nn.ReLU, RELU), (torch.nn.Tanh, TANH), ((torch.nn.SiLU, Swish), SILU), (Sin, SIN),
                      (Exp, EXP), (SinLU, SINLU), (hhSinLU, HHSINLU)):
        if isinstance(module, cls):
            return code
    return None


def module_of(name):
    """The `nonlin` argument for a name of NAMES, or for a comma list of them, one per hidden layer ('relu,sin';
    command-line switches): a module class, None for 'none', or a list of these."""
    if ',' in name:
        return [_MODULES[n.strip()] for n in name.split(',')]
    return _MODULES[name]


def pack(codes):
    """The value of an `act` field of the C ABI for the hidden layers' codes: the plain code when they all agree on ReLU,
    Tanh or SiLU -- what such a network has always passed, and the only plain values the ABI takes -- else
    PMBRL_ACT_PER_LAYER | code_l << 3 l (a uniform Sin network too: the same code in every layer)."""
    codes = [int(c) for c in codes]
    if len(codes) > MAX_HIDDEN or any(not 0 <= c <= NONE for c in codes):
        raise ValueError('at most %d hidden layers, each with a code 0 .. %d: %r' % (MAX_HIDDEN, NONE, codes))
    if not codes:
        return RELU
    if len(set(codes)) == 1 and codes[0] <= SILU:
        return codes[0]
    v = PER_LAYER
    for l, c in enumerate(codes):
        v |= c << (3 * l)
    return v


def unpack(act, n_hidden):
    """The per-layer codes of a packed `act` value (either form)."""
    act = int(act)
    if act & PER_LAYER:
        return [(act >> (3 * l)) & 7 for l in range(n_hidden)]
    return [act] * n_hidden
