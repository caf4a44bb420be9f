"""The envelope of the network-fit kernels (csrc/pmbrl_bnn.h: pm_bnn_fwd_bwd, pm_bnn_finish, pm_bnn_loss, pm_bnn_tail; the dW
block kernel and its reduction; gemm_tiles / gemm_narrow of csrc/pmbrl_dev.h) as a table of small synthetic fits, and the
arithmetic both envelope tests judge them with:

  tests/test_fit_envelope_cases.py   (CPU) the table reaches every branch it is there for, every ReLU case is clear of the
                                     kink, every case is well conditioned: the oracle's own fp32 run stays within a
                                     quarter of each bar of its fp64 run
  tests/test_gpu_fit_envelope.py     (GPU) pmbrl_bnn_loss_grad and pmbrl_bnn_train_steps on every case against the fp64 oracle

One axis varies per case around [6, 40, 24, 8], M = 24, N = 60, where the recorded fixtures sit.  Cases are generated from
a seed (as tests/test_bernoulli_fit_oracle.py::example_width_case is), nothing is stored: each is a fixture-like dict that
oracle.ref_torch.bnn_train and tests/test_gpu_bernoulli_fit.py's bnn_step / flat_params / noise understand."""
import functools

import numpy as np
import torch

from oracle import ref_torch as R
from prob_mbrl_amd import activations as ACT
from tests import common

# the project's bars (tests/test_gpu_bernoulli_fit.py::replay_loss_grad)
LOSS_RTOL, LOSS_ATOL = 3e-5, 2e-6
GRAD_BAR = 5e-5
# tests/test_bernoulli_fit_oracle.py: the distance every kept pre-activation of a ReLU case keeps from 0
KINK_MARGIN = 1e-5

B, C, N = R.BERNOULLI, R.CONCRETE, R.NONE
RELU, TANH, SILU = ACT.RELU, ACT.TANH, ACT.SILU
CENTRE = [6, 40, 24, 8]


def _case(cid, seed, dims, M, act, kinds, n_rows=60, n_components=0):
    """dims: the Linear layers' widths, input first; kinds: the dropout kind behind each hidden layer; n_rows: the data
    set's size (the fixture key N); n_components > 1: the mixture likelihood, the head (2 D + 1) n + 1 wide."""
    assert len(kinds) == len(dims) - 2 and M <= n_rows
    return dict(id=cid, seed=seed, dims=list(dims), M=M, act=act, kinds=tuple(kinds), N=n_rows, n_components=n_components)


CASES = [
    _case('in20', 1, [20, 40, 24, 8], 24, RELU, [B, C]),                     # nt[0] = 2: the gather, layer 0's stash
    _case('one_hidden', 42, [6, 40, 4], 17, RELU, [C]),                      # nl = 2, M % 16 = 1
    _case('eight_linear', 3, [5, 24, 24, 24, 24, 24, 24, 24, 6], 20, TANH, [C, B, N, C, B, N, C]),      # nl = 8, all kinds
    _case('kb8', 4, [6, 128, 120, 8], 33, TANH, [C, B]),                     # gemm_tiles_group_full, forward and backward
    _case('w256_edge', 5, [6, 256, 256, 8], 20, RELU, [B, C]),               # n_kb = 16, the LDS edge, dW blocks from 16 tiles
    _case('w272_relu', 35, [20, 272, 8], 20, RELU, [B]),                     # 17 output tiles: the second tile group
    _case('w272_silu', 7, [6, 272, 8], 20, SILU, [C]),                       # ... on the ACT instances, with logits
    _case('nt4', 8, [6, 64, 64, 8], 24, RELU, [C, C]),                       # dW blocks of 4 input tiles
    _case('nt5', 9, [6, 80, 72, 8], 24, TANH, [C, B]),                       # ... of 5: the part-filled NJ = 6 class
    _case('head64', 10, [6, 48, 48, 64], 30, TANH, [C, C]),                  # gemm_narrow's tile-split head
    _case('gmm_head53', 11, [6, 40, 24, 53], 24, RELU, [B, C], n_components=4),      # D = 6: mixture, tile-split head
    _case('gmm_8comp', 12, [6, 40, 24, 41], 24, TANH, [C, C], n_components=8),       # D = 2: PMBRL_MAX_COMP components
    _case('m1_bern', 13, CENTRE, 1, RELU, [B, B]),                           # one row
    _case('m1_tanh', 14, CENTRE, 1, TANH, [C, C]),
    _case('m16', 35, CENTRE, 16, RELU, [B, C]),                              # one full tile
    _case('m17', 16, CENTRE, 17, RELU, [B, C]),                              # a tile and a row
    _case('m144', 17, CENTRE, 144, RELU, [B, C], n_rows=300),                # 9 chunks: the tail's second pass
    _case('m272', 18, [6, 80, 72, 8], 272, TANH, [C, B], n_rows=400),        # 17 chunks: a third, part-filled pass
    # (beyond the tiles a tail wave takes at once: nine output tiles, so that a wave's second tile follows a first one whose
    #  second pass has replaced the input-side operands -- the restore behind the chunk loop)
    _case('m144_w144', 19, [6, 144, 8], 144, TANH, [C], n_rows=300),
]
assert len({c['id'] for c in CASES}) == len(CASES)
GAUSSIAN = [c for c in CASES if c['n_components'] <= 1]


def ids(cases):
    return [c['id'] for c in cases]


def by_id(cid):
    return next(c for c in CASES if c['id'] == cid)


def generate(case, seed=None):
    """The fit of a case as a fixture-like dict, two iterations.  seed: numpy's (weights, data, minibatches) and torch's
    (uniforms, Bernoulli draws).  Every number the device receives as a float is an fp32 value here, so that the fp64
    oracle and the device start from the same problem."""
    seed = case['seed'] if seed is None else seed
    rs = np.random.RandomState(seed)
    torch.manual_seed(seed)
    dims, M, n_rows, kinds = case['dims'], case['M'], case['N'], case['kinds']
    nl = len(dims) - 1
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    d = dict(n_layers=nl, act=case['act'], N=n_rows, M=M, iters=2, lr=f32(1e-3), reg_weight=1.0,
             max_log_std=f32(np.log(5.0)))
    n_comp = case['n_components']
    if n_comp > 1:
        d['n_components'] = n_comp
        D = ((dims[-1] - 1) // n_comp - 1) // 2
        assert (2 * D + 1) * n_comp + 1 == dims[-1]
    else:
        D = dims[-1] // 2
    for l in range(nl):
        d['W%d_init' % l] = (rs.randn(dims[l + 1], dims[l]) * np.sqrt(2.0 / dims[l])).astype(np.float32)
        d['b%d_init' % l] = rs.uniform(-0.1, 0.1, dims[l + 1]).astype(np.float32)
    for l, kind in enumerate(kinds):
        d['kind%d' % l] = kind
        if kind != N:
            d['reg_scale%d' % l] = 0.5
        if kind == B:
            d['keep%d' % l] = np.array([np.float32((0.9, 0.75)[l % 2])])
        if kind == C:
            d['temp%d' % l], d['drop_reg%d' % l] = f32(0.1), 1.0
            d['logit_p%d_init' % l] = (np.log(9.0) + 0.3 * rs.randn(dims[l + 1])).astype(np.float32)
    n_in = dims[0]
    X = rs.randn(n_rows, n_in)
    d['Xn'] = X.astype(np.float32)
    j = np.arange(D)
    d['Yn'] = (0.3 * rs.randn(n_rows, D) + 0.5 * X[:, j % n_in] * X[:, (j + 1) % n_in]).astype(np.float32)
    for it in range(2):
        d['idx_it%d' % it] = rs.permutation(n_rows)[:M]
        for l, kind in enumerate(kinds):
            h = dims[l + 1]
            if kind == B:
                d['hard%d_it%d' % (l, it)] = torch.bernoulli(torch.full((M, h), float(d['keep%d' % l][0]))).numpy()
            if kind == C:
                # CDropout.forward (models/modules.py:120-160): hard ~ Bernoulli(probs) of the layer's own probs, here at
                # the initial logits in both iterations (the draws are inputs of the fit, recorded before it runs)
                u = torch.rand(M, h)
                u64 = u.double()
                cp = torch.tensor(d['logit_p%d_init' % l], dtype=torch.float64) + ((u64 + 1e-7) / (1 - (u64 - 1e-7))).log()
                d['u%d_it%d' % (l, it)] = u.numpy()
                d['hard%d_it%d' % (l, it)] = torch.bernoulli((cp / d['temp%d' % l]).sigmoid()).float().numpy()
    return d


@functools.lru_cache(maxsize=None)
def _problem(cid):
    return generate(by_id(cid))


def problem(case):
    """The case's fit, generated once and shared (leave it unchanged)."""
    return _problem(case['id'])


def keys_of(d):
    return R.fit_problem_from_npz(d)[3]


def restart(d, it, params):
    """The one-iteration fit that starts at `params` (arrays in the order of keys_of(d)) with the minibatch and the draws of
    iteration `it`."""
    out = {k: v for k, v in d.items() if '_it' not in k and not k.endswith('_init')}
    out['iters'] = 1
    for key, p in zip(keys_of(d), params):
        out[key + '_init'] = np.asarray(p)
    for k, v in d.items():
        if k.endswith('_it%d' % it):
            out[k[:-len('_it%d' % it)] + '_it0'] = v
    return out


def run_oracle(d, dtype):
    """R.bnn_train on d -> dict(losses [iters, 3], grads: per iteration the list of arrays, params: the final ones)."""
    grads = []
    params, losses, _ = R.bnn_train(d, dtype, grads=grads)
    return dict(losses=np.asarray(losses, np.float64), grads=[[g.numpy() for g in gs] for gs in grads],
                params=[p.detach().numpy() for p in params])


def reference_of(d):
    o = run_oracle(d, torch.float64)
    # the parameters after the FIRST step, cast to fp32: where the second iteration of every comparison starts, so that
    # Adam's conditioning (its first step is g / (|g| + eps)) stays out of the gradients' comparison
    p1 = run_oracle(dict(d, iters=1), torch.float64)['params']
    o['second'] = restart(d, 1, [p.astype(np.float32) for p in p1])
    return o


@functools.lru_cache(maxsize=None)
def _reference(cid):
    return reference_of(_problem(cid))


def conditioning(d, ref):
    """The oracle's own fp32 run of both iterations the GPU test judges against the fp64 run `ref` (reference_of(d)):
    [(iteration, loss figure, gradient figures)]."""
    keys = keys_of(d)
    out = []
    for it, fit in enumerate((d, ref['second'])):
        o32 = run_oracle(dict(fit, iters=1), torch.float32)
        out.append((it, loss_figure(o32['losses'][0], ref['losses'][it]), grad_figures(o32['grads'][0], ref['grads'][it], keys)))
    return out


def reference(case):
    """The fp64 oracle's run of the case (shared, leave it unchanged): losses, grads, params, and `second`: the
    one-iteration fit at its parameters after the first step, cast to fp32.  The expectation of that fit is the run's
    own second iteration (losses[1], grads[1])."""
    return _reference(case['id'])


def loss_figure(got, want):
    """np.allclose's criterion at the loss bar as one number: max |got - want| / (atol + rtol |want|); it holds at <= 1."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    return float(np.max(np.abs(got - want) / (LOSS_ATOL + LOSS_RTOL * np.abs(want))))


def grad_figures(got, want, keys):
    """[(key, common.rel)] of every parameter tensor's gradient on its own."""
    assert len(got) == len(want) == len(keys)
    return [(k, common.rel(np.asarray(g).reshape(-1), np.asarray(w).reshape(-1))) for k, g, w in zip(keys, got, want)]


def hold(what, loss_fig, grad_figs, share=1.0):
    """Print every figure, then hold each to `share` of its bar."""
    print('%s: loss %.3f of its bar; %s' % (what, loss_fig, ', '.join('%s %.2e' % e for e in grad_figs)))
    assert loss_fig <= share, (what, 'loss', loss_fig)
    for key, e in grad_figs:
        assert e < share * GRAD_BAR, (what, key, e)


# ---- the branch arithmetic of the kernels, mirrored (csrc/pmbrl_dev.h, pmbrl_bnn.h, pmbrl_bnn.hip, pmbrl_dw.hip)
PM_NW, PM_KS_NT, PM_CK = 8, 3, 4            # pmbrl_dev.h
PM_BNT_NW, TAIL_TB, TAIL_CB = 8, 2, 8       # pm_bnn_tail: waves, tiles per wave and pass, chunks per pass
PM_DW_TM, PM_DW_TN = 4, 7                   # pmbrl_dw.h: a dW block is at most 4 x 7 tiles
MAX_COMP = 8                                # PMBRL_MAX_COMP
LDS_LIMIT = 160 * 1024


def tiles(w):
    return (w + 15) // 16


def split(n, maxsz):
    """build_dw_blocks' balanced split of n tiles into parts of at most maxsz: the parts' sizes."""
    parts = max(-(-n // maxsz), min(n, 1))
    return [n // parts + (1 if i < n % parts else 0) for i in range(parts)]


def lds_bytes(dims, act):
    """pm_bnn_lds_floats * 4 of a plan."""
    nl = len(dims) - 1
    LD = 16 * max(tiles(w) for w in dims) + 8
    return 4 * ((nl + (nl - 1) + 3 + (1 if act != RELU else 0)) * 16 * LD + PM_NW * PM_KS_NT * 256 + PM_NW * 64)


def regimes(case):
    """The names of the branches a case's plan takes."""
    dims, M, kinds = case['dims'], case['M'], case['kinds']
    nl = len(dims) - 1
    nt = [tiles(w) for w in dims]
    out = set()
    # gemm_tiles(n_ot, n_kb): the hidden layers forward, the head when gemm_narrow splits it by tiles, and every layer but
    # the first backward
    fwd = [(nt[l + 1], nt[l]) for l in range(nl - 1)]
    if nt[nl] > PM_KS_NT:
        fwd.append((nt[nl], nt[nl - 1]))
        out.add('head_tile_split')
    bwd = [(nt[l], nt[l + 1]) for l in range(1, nl)]
    for name, calls in (('fwd', fwd), ('bwd', bwd)):
        if any(n_kb % (2 * PM_CK) == 0 for _, n_kb in calls):
            out.add('gemm_group_full_' + name)
        if any(n_ot > 2 * PM_NW for n_ot, _ in calls):
            out.add('gemm_second_group_' + name)
    if nt[0] > 1:
        out.add('input_tiles_gt1')
    out.add('nl%d' % nl)
    if nl > 4:
        out.add('nl_gt4')
    if M == 1:
        out.add('m1')
    out.add('m_mod16_%d' % (M % 16))
    chunks = -(-M // 16)
    if TAIL_CB < chunks <= 2 * TAIL_CB:
        out.add('tail_chunks_9_16')
    if chunks > 2 * TAIL_CB:
        out.add('tail_chunks_gt16')
    if any(nt[l + 1] > TAIL_TB * PM_BNT_NW for l in range(nl)):
        out.add('tail_second_group')
    if chunks > TAIL_CB and any(nt[l + 1] > PM_BNT_NW for l in range(nl)):
        out.add('tail_restore')      # a wave's second tile behind a first one that ran more than one pass
    for l in range(nl):
        for n_it in split(nt[l], PM_DW_TN):
            out.add('dw_n_it%d' % n_it)
        if nt[l] == 16 or nt[l + 1] == 16:
            out.add('dw_from_16_tiles')
        if nt[l] == 17 or nt[l + 1] == 17:
            out.add('dw_from_17_tiles')
    out.update({B: 'bernoulli', C: 'concrete', N: 'no_dropout'}[k] for k in kinds)
    out.add({RELU: 'relu', TANH: 'tanh', SILU: 'silu'}[case['act']])
    n = case['n_components']
    out.add('mixture' if n > 1 else 'gaussian')
    if n > 2:
        out.add('mixture_gt2')
    if n == MAX_COMP:
        out.add('mixture_max_comp')
    widest = list(dims)
    for l in range(1, nl):
        widest[l] = dims[l] + 16 if tiles(dims[l]) == max(nt) else dims[l]
    if lds_bytes(dims, case['act']) <= LDS_LIMIT < lds_bytes(widest, case['act']):
        out.add('lds_edge')
    return out
