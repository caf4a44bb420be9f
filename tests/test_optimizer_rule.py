"""CPU: the optimiser rule's host side -- pmbrl_opt_rule_check (every refusal of include/pmbrl.h and the accepting case at
the limits), the translator from a torch optimiser (optim.layout, algorithms._adam_flat_state / _sync_adam_state) and the
fixtures of tests/golden/optimizers.  No compute calls."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from tests import common

OPT_DIR = os.path.join(common.GOLDEN, 'optimizers')
OPT_FIXTURES = ['opt_mcp_adamw_groups', 'opt_mcp_adam_l2_amsgrad', 'opt_mcp_adamw_mmg', 'opt_bnn_adamw_logit_lr',
                'opt_bnn_adam_amsgrad', 'opt_critic_adamw']


def _rule(n=100, groups=None, segments=None, vmax=None):
    from prob_mbrl_amd import optim
    groups = groups if groups is not None else [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, flags=0)]
    segments = segments if segments is not None else [(n, 0)]
    return optim.Rule(groups, segments, vmax)


def _check(rule, n=100):
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    r = rule.struct()
    rc = lib.pmbrl_opt_rule_check(ctypes.byref(r), n)
    return rc, lib.pmbrl_last_error()


class _Ptr:
    """stands for a device buffer: the check only asks whether there is one"""

    def data_ptr(self):
        return 4096


G = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, flags=0)


def test_symbols_are_declared_exported_and_bound():
    from prob_mbrl_amd import _lib
    header = open(os.path.join(common.ROOT, 'include', 'pmbrl.h')).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pmbrl_opt_rule_check', 'pmbrl_clip_adam_rule', 'pmbrl_clip_adam_rule_guarded', 'pmbrl_plan_set_optimizer',
                 'pmbrl_bnn_plan_set_optimizer'):
        assert name in header and hasattr(so, name) and name in _lib.EXPORTS, name
    # the mirror of pmbrl_opt_rule: 4 + 8 * 48 + 4 + 32 * 8 + 32 * 4 + 8, with the compiler's padding
    assert ctypes.sizeof(_lib.OptGroup) == 48
    assert _lib.OptRule.group.offset == 8 and _lib.OptRule.n_segments.offset == 8 + 8 * 48
    assert _lib.OptRule.seg_end.offset == 400 and _lib.OptRule.seg_group.offset == 656
    assert _lib.OptRule.max_exp_avg_sq_d.offset == 784 and ctypes.sizeof(_lib.OptRule) == 792
    assert (_lib.OPT_MAX_GROUPS, _lib.OPT_MAX_SEGMENTS) == (8, 32)
    for k, v in (('PMBRL_OPT_MAX_GROUPS', 8), ('PMBRL_OPT_MAX_SEGMENTS', 32), ('PMBRL_OPT_DECOUPLED', 1),
                 ('PMBRL_OPT_AMSGRAD', 2), ('PMBRL_OPT_MAXIMIZE', 4)):
        assert '#define %s' % k in header and int(header.split('#define %s' % k)[1].split()[0]) == v


def test_check_accepts_the_plain_rule_and_the_limits():
    assert _check(_rule())[0] == 0
    groups = [dict(G, lr=1e-3 * (k + 1), weight_decay=0.01 * k, flags=k % 8) for k in range(8)]
    segments = [(4 * (q + 1), q % 8) for q in range(31)] + [(1000, 7)]
    assert _check(_rule(1000, groups, segments, _Ptr()), 1000)[0] == 0
    # lr, eps and weight_decay of exactly 0 and beta of exactly 0 are inside the ranges
    assert _check(_rule(groups=[dict(lr=0.0, betas=(0.0, 0.0), eps=0.0, weight_decay=0.0, flags=0)]))[0] == 0


@pytest.mark.parametrize('kw, text', [
    (dict(groups=[]), b'n_groups'),
    (dict(groups=[G] * 9), b'n_groups'),
    (dict(segments=[]), b'n_segments'),
    (dict(segments=[(q + 1, 0) for q in range(32)] + [(100, 0)]), b'n_segments'),
    (dict(segments=[(50, 0), (50, 0), (100, 0)]), b'ascend'),
    (dict(segments=[(60, 0), (50, 0), (100, 0)]), b'ascend'),
    (dict(segments=[(0, 0), (100, 0)]), b'ascend'),
    (dict(segments=[(50, 0), (99, 0)]), b'not n'),
    (dict(segments=[(50, 0), (101, 0)]), b'not n'),
    (dict(segments=[(50, 0), (100, 1)]), b'seg_group'),
    (dict(segments=[(50, -1), (100, 0)]), b'seg_group'),
    (dict(groups=[dict(G, lr=-1e-3)]), b'lr < 0'),
    (dict(groups=[dict(G, betas=(1.0, 0.999))]), b'beta'),
    (dict(groups=[dict(G, betas=(0.9, -0.1))]), b'beta'),
    (dict(groups=[dict(G, betas=(float('nan'), 0.9))]), b'beta'),
    (dict(groups=[dict(G, eps=-1e-8)]), b'eps < 0'),
    (dict(groups=[dict(G, weight_decay=-0.01)]), b'weight_decay < 0'),
    (dict(groups=[dict(G, flags=8)]), b'unknown flag'),
    (dict(groups=[G, dict(G, flags=2)], segments=[(50, 0), (100, 1)]), b'AMSGRAD without'),
])
def test_check_refuses(kw, text):
    rc, msg = _check(_rule(**kw))
    assert rc == -2 and text in msg, (rc, msg)


def test_check_refuses_null_and_setters_refuse_a_null_plan():
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    assert lib.pmbrl_opt_rule_check(None, 10) == -2
    r = _rule().struct()
    assert lib.pmbrl_plan_set_optimizer(None, ctypes.byref(r)) < 0 and b'null' in lib.pmbrl_last_error()
    assert lib.pmbrl_bnn_plan_set_optimizer(None, ctypes.byref(r)) < 0 and b'null' in lib.pmbrl_last_error()
    # every call goes through the check, before anything touches a device
    bad = _rule(groups=[dict(G, lr=-1.0)]).struct()
    p = ctypes.c_void_p(4096)
    assert lib.pmbrl_clip_adam_rule(None, p, p, p, p, 100, 1, 0.0, None, ctypes.byref(bad)) == -2
    assert lib.pmbrl_clip_adam_rule_guarded(None, p, p, p, p, 100, p, 0.0, None, p, 1, ctypes.byref(bad)) == -2


# ---------------------------------------------------------------------------------------------------------------------
def _policy_net():
    import prob_mbrl_amd as pm
    return pm.models.mlp(5, 8, [16, 16], dropout_layers=[pm.models.BDropout(0.1) for _ in range(2)])


def _weights_biases(net):
    ps = [p for p in net.parameters() if p.requires_grad]
    return ps, [p for p in ps if p.dim() > 1], [p for p in ps if p.dim() == 1]


def test_segments_of_weights_and_biases_groups_follow_the_flat_vector():
    from prob_mbrl_amd import optim
    ps, W, b = _weights_biases(_policy_net())
    opt = torch.optim.AdamW([dict(params=W, weight_decay=1e-2), dict(params=b, weight_decay=0.0, lr=3e-3)], lr=1e-3)
    seg = optim.layout(opt, ps)
    ends = np.cumsum([p.numel() for p in ps]).tolist()       # W0 b0 W1 b1 W2 b2: nothing to merge
    assert seg == list(zip(ends, [0, 1, 0, 1, 0, 1]))
    # biases first in the optimiser, and the last weight with the biases: b1 | W2 | b2 merge
    opt = torch.optim.AdamW([dict(params=b + W[2:]), dict(params=W[:2], weight_decay=1e-2)], lr=1e-3)
    assert optim.layout(opt, ps) == [(ends[0], 1), (ends[1], 0), (ends[2], 1), (ends[5], 0)]
    assert optim.group_flags(opt, opt.param_groups[0]) == 1            # AdamW: decoupled
    adam = torch.optim.Adam(ps, 1e-3, weight_decay=1e-2, amsgrad=True, maximize=True)
    assert optim.layout(adam, ps) == [(ends[5], 0)] and optim.group_flags(adam, adam.param_groups[0]) == 2 | 4
    assert not optim.is_plain(adam) and optim.is_plain(torch.optim.Adam(ps, 1e-3))
    assert optim.is_plain(torch.optim.AdamW(ps, 1e-3, weight_decay=0.0))


def test_a_third_group_over_the_dropout_logits():
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import optim
    net = pm.models.mlp(5, 8, [16, 16], dropout_layers=[pm.models.CDropout(0.1 * np.ones(16)) for _ in range(2)])
    ps = [p for p in net.parameters() if p.requires_grad]
    logits = [p for n, p in net.named_parameters() if 'logit_p' in n]
    assert len(logits) == 2 and len(ps) == 8
    W = [p for p in ps if p.dim() > 1]
    b = [p for p in ps if p.dim() == 1 and not any(p is q for q in logits)]
    opt = torch.optim.AdamW([dict(params=W, weight_decay=1e-2), dict(params=b, weight_decay=0.0),
                             dict(params=logits, weight_decay=0.0, lr=1e-2)], lr=1e-3)
    ends = np.cumsum([p.numel() for p in ps]).tolist()       # W0 b0 lp0 W1 b1 lp1 W2 b2
    assert optim.layout(opt, ps) == list(zip(ends, [0, 1, 2, 0, 1, 2, 0, 1]))


def test_translator_returns_none_for_what_is_not_offered():
    from prob_mbrl_amd import optim
    from prob_mbrl_amd.algorithms import _adam_flat_state
    ps, W, b = _weights_biases(_policy_net())
    flat = torch.cat([p.detach().reshape(-1) for p in ps])
    none = lambda opt, params=ps: optim.layout(opt, params) is None and _adam_flat_state(opt, params, flat) is None  # noqa: E731
    assert none(torch.optim.SGD(ps, 1e-3))
    assert none(torch.optim.RAdam(ps, 1e-3))
    assert none(torch.optim.Adam([dict(params=[p]) for p in ps] + [dict(params=[torch.nn.Parameter(torch.zeros(k + 1))])
                                                                   for k in range(3)], 1e-3))       # 9 groups
    assert none(torch.optim.Adam(W, 1e-3))                                  # the biases are in no group
    two = torch.optim.Adam([dict(params=W), dict(params=b)], 1e-3)
    two.param_groups[1]['params'].append(W[0])                              # (torch's constructor refuses this itself)
    assert none(two)
    assert none(torch.optim.Adam(ps + [torch.nn.Parameter(torch.zeros(3))], 1e-3))      # a trainable tensor not in params
    assert none(torch.optim.Adam(ps, 1e-3, capturable=True))
    assert none(torch.optim.Adam(ps, 1e-3, differentiable=True))
    assert none(torch.optim.Adam(ps, torch.tensor(1e-3)))
    # more than 32 segments after merging: 17 tensors in each of two groups, interleaved
    many = [torch.nn.Parameter(torch.zeros(2)) for _ in range(34)]
    assert none(torch.optim.Adam([dict(params=many[0::2]), dict(params=many[1::2])], 1e-3), many)
    # ... 32 are offered, and a frozen tensor in a group does not count
    frozen = torch.nn.Parameter(torch.zeros(4), requires_grad=False)
    ok = torch.optim.Adam([dict(params=many[0:32:2] + [frozen]), dict(params=many[1:32:2])], 1e-3)
    assert len(optim.layout(ok, many[:32])) == 32


@pytest.mark.parametrize('cls, kw', [(torch.optim.Adam, dict(weight_decay=1e-2, amsgrad=True)),
                                     (torch.optim.AdamW, dict(weight_decay=1e-2)),
                                     (torch.optim.Adam, {})])
def test_existing_state_is_imported_and_exposed_again(cls, kw):
    from prob_mbrl_amd import optim
    from prob_mbrl_amd.algorithms import _adam_flat_state, _sync_adam_state
    torch.manual_seed(3)
    ps, W, b = _weights_biases(_policy_net())
    opt = cls([dict(params=W), dict(params=b, lr=5e-3)], lr=1e-3, **kw)
    for it in range(3):
        for p in ps:
            p.grad = torch.randn_like(p) * (1.0 + it)
        opt.step()
    want = {k: [opt.state[p][k].clone() for p in ps] for k in opt.state[ps[0]] if k != 'step'}
    flat = torch.cat([p.detach().reshape(-1) for p in ps])
    cache = _adam_flat_state(opt, ps, flat)
    # (two groups with learning rates of their own: not the plain kernels' rule, whatever else is set)
    assert cache['step'] == 3 and not cache['plain'] and (cache['vmax'] is not None) == bool(kw.get('amsgrad'))
    assert cache['segments'] == optim.layout(opt, ps)
    off = 0
    for i, p in enumerate(ps):
        for key, buf in (('exp_avg', 'm'), ('exp_avg_sq', 'v'), ('max_exp_avg_sq', 'vmax')):
            if key in want:
                assert torch.equal(cache[buf][off:off + p.numel()], want[key][i].reshape(-1)), (key, i)
        off += p.numel()
    rule = optim.rule_of(cache)
    assert [g['lr'] for g in rule.groups] == [1e-3, 5e-3] and rule.segments == cache['segments']
    assert all(g['weight_decay'] == kw.get('weight_decay', 0) for g in rule.groups) and rule.vmax is cache['vmax']
    opt.param_groups[0]['lr'] = 7e-4          # a scheduler between two steps
    assert optim.rule_of(cache).groups[0]['lr'] == 7e-4
    opt.param_groups[0]['lr'] = 1e-3
    one = torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))], 1e-3)      # the plain rule: served by the plain calls
    assert optim.rule_of(_adam_flat_state(one, one.param_groups[0]['params'], torch.zeros(3))) is None
    # the device would step here; exposed again, torch continues from the same numbers as an untouched copy
    cache['step'] += 0
    _sync_adam_state(opt, ps, cache)
    sd = opt.state_dict()['state']
    assert len(sd) == len(ps) and all(float(s['step']) == 3.0 for s in sd.values())
    for i, p in enumerate(ps):
        for key in want:
            assert torch.equal(opt.state[p][key], want[key][i]), (key, i)
            assert opt.state[p][key].data_ptr() >= cache['m' if key == 'exp_avg' else 'v' if key == 'exp_avg_sq' else 'vmax'].data_ptr()
    ref = [p.detach().clone() for p in ps]
    ref_opt = cls([dict(params=[ref[i] for i, p in enumerate(ps) if p.dim() > 1]),
                   dict(params=[ref[i] for i, p in enumerate(ps) if p.dim() == 1], lr=5e-3)], lr=1e-3, **kw)
    for i, r in enumerate(ref):
        r.requires_grad_(True)
        ref_opt.state[r] = {k: want[k][i].clone() for k in want}
        ref_opt.state[r]['step'] = torch.tensor(3.0)
    for p, r in zip(ps, ref):
        p.grad = torch.full_like(p, 0.25)
        r.grad = torch.full_like(r, 0.25)
    opt.step()
    ref_opt.step()
    for p, r in zip(ps, ref):
        assert torch.equal(p.detach(), r.detach())


def test_refusal_messages_name_what_is_offered():
    from prob_mbrl_amd import optim
    assert 'torch.optim.Adam' in optim.OFFERED and 'AdamW' in optim.OFFERED


def test_optimizer_fixtures_hold_numeric_arrays_only():
    files = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(OPT_DIR, '*.npz')))
    assert files == sorted(OPT_FIXTURES)
    for name in files:
        path = os.path.join(OPT_DIR, name + '.npz')
        assert os.path.getsize(path) < 200 * 1024
        raw = np.load(path, allow_pickle=False)
        for k in raw.files:
            assert raw[k].dtype.kind in 'biuf' or k == 'rew_kind' and raw[k].dtype.kind == 'U', (name, k, raw[k].dtype)
        for k in ('opt_n_groups', 'opt_class', 'opt_group_lr', 'opt_group_betas', 'opt_group_eps', 'opt_group_weight_decay',
                  'opt_group_flags', 'opt_seg_end', 'opt_seg_group'):
            assert k in raw.files, (name, k)
        ng = int(raw['opt_n_groups'])
        assert 1 <= ng <= 8 and raw['opt_group_lr'].shape == (ng,) and raw['opt_group_betas'].shape == (ng, 2)
        assert len(raw['opt_seg_end']) == len(raw['opt_seg_group']) <= 32 and int(raw['opt_seg_group'].max()) < ng
