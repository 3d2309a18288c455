"""CPU tests of Grad-CAM++ for the severity and uncertainty outputs (``target=``): the Python entry refuses every bad target before it
touches the model, the C entries (rovit_explain_seed, rovit_vit_gradcam_seeded) reject bad arguments before anything is launched, and an
fp64 restatement of the five seeds -- the chain rule written out, as csrc/explain.hip computes it -- agrees with torch autograd through
the oracle."""
import ctypes

import pytest
import torch

from oracle import ref_cpu  # noqa: E402  (checker only)


@pytest.fixture(scope='module')
def native():
    from rovit_hip import native as n
    import os
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    n.load()
    return n


# ---- the Python entry ------------------------------------------------------------------------------------------------------------

def _refused(m, x, match, **kw):
    from rovit_hip import RovitHipError
    from rovit_hip.gradcam import grad_cam_pp
    with pytest.raises(RovitHipError, match=match):
        grad_cam_pp(m, x, **kw)


def test_python_entry_refuses_bad_targets_before_touching_the_model():
    from models.rovit_kan import RoViTKAN
    m = RoViTKAN(pretrained=False)
    x = torch.zeros(2, 3, 224, 224)
    for bad in ('severity', ['mu', 'sigma'], 'CLASS'):
        _refused(m, x, 'unknown target', target=bad)
    for bad in ([], (), 3, None, ['mu', 3]):
        _refused(m, x, 'target must be', target=bad)
    _refused(m, x, 'more than once', target=['mu', 'log_var', 'mu'])
    _refused(m, x, 'more than once', target=('class', 'class'))
    _refused(m, x, 'class_idx', target='mu', class_idx=1)
    _refused(m, x, 'class_idx', target=['mu', 'kan_severity'], class_idx=torch.tensor([0, 1]))
    for stage, bad in ((1, 'ordinal_severity'), (2, 'mu'), (2, 'log_var'), (3, 'kan_severity'), (3, ['class', 'kan_severity'])):
        m.curriculum_stage = stage
        _refused(m, x, 'curriculum stage', target=bad)
    m.curriculum_stage = 4
    for t in ('ordinal_severity', 'mu', 'log_var', 'kan_severity', ['class', 'mu']):      # accepted: the CPU tensor is what is refused
        _refused(m, x, 'GPU', target=t)
    assert all(p.grad is None for p in m.parameters())
    assert m.backbone.model._engine is None          # nothing was prepared


def test_python_entry_refuses_shapes_outside_the_fused_seed():
    from models.rovit_kan import RoViTKAN
    x = torch.zeros(1, 3, 224, 224)
    two_out = RoViTKAN(pretrained=False, kan_layers=[192, 16, 2])
    _refused(two_out, x, 'hook recipe', target='kan_severity')
    _refused(two_out, x, 'GPU', target='mu')                    # the heads are covered
    wide = RoViTKAN(pretrained=False, kan_layers=[192, 128, 1])
    _refused(wide, x, 'hook recipe', target='kan_severity')
    deep = RoViTKAN(pretrained=False, kan_layers=[192, 8, 8, 8, 8, 1])
    _refused(deep, x, 'hook recipe', target=['class', 'kan_severity'])
    odd = RoViTKAN(pretrained=False, hidden_dim=130)
    for t in ('ordinal_severity', 'mu', 'log_var'):
        _refused(odd, x, 'hook recipe', target=t)
    _refused(odd, x, 'GPU', target='kan_severity')
    many = RoViTKAN(pretrained=False, num_classes=9)
    _refused(many, x, 'hook recipe', target='ordinal_severity')
    _refused(many, x, 'GPU', target='class')
    for m in (two_out, wide, deep, odd, many):
        assert m.backbone.model._engine is None


def test_drop_in_class_takes_target():
    from explainability import GradCAMPlusPlus
    from models.rovit_kan import RoViTKAN
    from rovit_hip import RovitHipError
    m = RoViTKAN(pretrained=False)
    c = GradCAMPlusPlus(m, device='cpu')
    with pytest.raises(RovitHipError, match='unknown target'):
        c.compute(torch.zeros(1, 3, 224, 224), target='sigma')
    with pytest.raises(RovitHipError, match='GPU'):
        c.compute_batch(torch.zeros(1, 3, 224, 224), target=['mu', 'log_var'])
    with pytest.raises(RovitHipError, match='unknown target'):
        m.grad_cam_pp(torch.zeros(1, 3, 224, 224), target='sigma')


# ---- the C entries ---------------------------------------------------------------------------------------------------------------

def _desc(native, **kw):
    """A descriptor of dummy, 16-byte aligned non-null addresses: every call below is refused by the argument checks, so nothing is
    ever dereferenced."""
    d = native.HeadPhase()
    d.batch, d.embed, d.hid, d.num_classes, d.stage, d.kan_layers = 2, 192, 128, 4, 4, 3
    for l, w in enumerate((192, 64, 16, 1)):
        d.kan_dims[l] = w
    for l in range(3):
        d.kan_knots[l], d.kan_acts[l] = 11, 1
        d.kan_w[l] = d.kan_lw[l] = d.kan_lb[l] = d.kan_knots_p[l] = 256
    d.features = 256
    for i in range(14):
        d.head_params[i] = 256
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _seed(native, d, kinds=(1, 2, 3, 4), values=256, seeds=256):
    arr = (ctypes.c_int * len(kinds))(*kinds)
    native.call('rovit_explain_seed', ctypes.byref(d) if d is not None else None, ctypes.cast(arr, ctypes.c_void_p) if kinds else None,
                len(kinds), values, seeds, None)


def test_explain_seed_rejects_null_pointers(native):
    with pytest.raises(native.RovitHipError, match='null'):
        _seed(native, None)
    for kw in ({'values': None}, {'seeds': None}):
        with pytest.raises(native.RovitHipError, match='null'):
            _seed(native, _desc(native), **kw)
    with pytest.raises(native.RovitHipError, match='features'):
        _seed(native, _desc(native, features=None))
    d = _desc(native)
    d.head_params[10] = None
    with pytest.raises(native.RovitHipError, match='head parameter 10'):
        _seed(native, d)
    d = _desc(native)
    d.kan_w[2] = None
    with pytest.raises(native.RovitHipError, match='KAN layer 2'):
        _seed(native, d)


@pytest.mark.parametrize('kinds,match', [((0,), 'kind 0'), ((5,), 'kind 5'), ((-1, 2), 'kind -1'), ((2, 3, 2), 'repeated'),
                                         ((1, 2, 3, 4, 1), 'targets'), ((), 'null')])
def test_explain_seed_rejects_bad_target_kinds(native, kinds, match):
    with pytest.raises(native.RovitHipError, match=match):
        _seed(native, _desc(native), kinds=kinds)


@pytest.mark.parametrize('stage,kinds', [(1, (1,)), (2, (2,)), (2, (3,)), (3, (4,)), (3, (1, 4))])
def test_explain_seed_rejects_targets_the_stage_does_not_produce(native, stage, kinds):
    with pytest.raises(native.RovitHipError, match='stage'):
        _seed(native, _desc(native, stage=stage), kinds=kinds)


@pytest.mark.parametrize('kw,match', [({'batch': 0}, 'batch'), ({'embed': 384}, '192'), ({'hid': 260}, 'hidden'), ({'hid': 130}, 'hidden'),
                                      ({'num_classes': 9}, 'classes'), ({'num_classes': 1}, 'classes'), ({'stage': 5}, 'stage'),
                                      ({'kan_layers': 5}, 'KAN layers'), ({'kan_layers': 0}, 'KAN stack')])
def test_explain_seed_rejects_bad_shapes(native, kw, match):
    with pytest.raises(native.RovitHipError, match=match):
        _seed(native, _desc(native, **kw))


def test_explain_seed_rejects_bad_kan_stacks(native):
    d = _desc(native)
    d.kan_dims[3] = 2
    with pytest.raises(native.RovitHipError, match='one output'):
        _seed(native, d)
    d = _desc(native)
    d.kan_dims[1] = 65
    with pytest.raises(native.RovitHipError, match='wide'):
        _seed(native, d)
    d = _desc(native)
    d.kan_knots[0] = 65
    with pytest.raises(native.RovitHipError, match='knots'):
        _seed(native, d)
    d = _desc(native)
    d.kan_dims[0] = 128
    with pytest.raises(native.RovitHipError, match='input width'):
        _seed(native, d)


def _params(native, depth=12):
    n = native.load().rovit_vit_num_params(depth)
    return (ctypes.c_void_p * n)(*([16] * n))


def test_gradcam_seeded_rejects_bad_arguments(native):
    def run(params=True, prep=256, ws=256, dfeat=256, cam=256, batch=2, depth=12):
        native.call('rovit_vit_gradcam_seeded', _params(native) if params else None, prep, ws, dfeat, cam, None, None, batch, depth, None)
    for kw in ({'params': False}, {'prep': None}, {'ws': None}, {'dfeat': None}, {'cam': None}):
        with pytest.raises(native.RovitHipError, match='null'):
            run(**kw)
    for kw, match in (({'batch': 0}, 'batch'), ({'batch': -1}, 'batch'), ({'depth': 0}, 'depth'), ({'depth': 65}, 'depth'),
                      ({'dfeat': 264}, 'aligned')):
        with pytest.raises(native.RovitHipError, match=match):
            run(**kw)


def test_abi_version(native):
    assert native.load().rovit_version() == native.ABI_VERSION


# ---- the seeds, restated in fp64 -------------------------------------------------------------------------------------------------

def restate_seed(feats, sd, target, prefix_k='kan_module.'):
    """fp64 (value (B,), d target / d features (B,192)) with the chain rule written out, as csrc/explain.hip computes it."""
    x = feats.double()
    g = {k: v.double() for k, v in sd.items()}
    if target == 'ordinal_severity':
        h = torch.relu(x @ g['ordinal_head.fc1.weight'].T + g['ordinal_head.fc1.bias'])
        s = torch.sigmoid(h @ g['ordinal_head.fc2.weight'].T + g['ordinal_head.fc2.bias'])
        C = s.shape[1] + 1
        p = torch.cat([s[:, :1], s[:, 1:] - s[:, :-1], 1 - s[:, -1:]], 1)
        value = (p * torch.arange(C, dtype=torch.float64)).sum(1)
        dh = (-s * (1 - s)) @ g['ordinal_head.fc2.weight'] * (h > 0)
        return value, dh @ g['ordinal_head.fc1.weight']
    if target in ('mu', 'log_var'):
        h = torch.relu(x @ g['uncertainty_head.fc1.weight'].T + g['uncertainty_head.fc1.bias'])
        w = g['uncertainty_head.fc_mu.weight' if target == 'mu' else 'uncertainty_head.fc_logvar.weight']
        b = g['uncertainty_head.fc_mu.bias' if target == 'mu' else 'uncertainty_head.fc_logvar.bias']
        pre = (h @ w.T + b)[:, 0]
        value = pre if target == 'mu' else pre.clamp(-10, 10)
        gate = torch.ones_like(pre) if target == 'mu' else ((pre >= -10) & (pre <= 10)).double()
        return value, (gate[:, None] * w * (h > 0)) @ g['uncertainty_head.fc1.weight']
    assert target == 'kan_severity'
    n = 0
    while f'{prefix_k}kan_layers.{n}.spline_weights' in g:
        n += 1
    ins, pres, a = [], [], x
    for i in range(n):
        p = f'{prefix_k}kan_layers.{i}.'
        ins.append(a)
        z = ref_cpu.kan_layer_forward(a, g[p + 'spline_weights'], g[p + 'knots'], g[p + 'linear.weight'], g[p + 'linear.bias'])
        pres.append(z)
        a = torch.relu(z) if i < n - 1 else 3 * torch.sigmoid(z)
    value = a[:, 0]
    gz = value[:, None] * (1 - value[:, None] / 3)                       # d 3 sigmoid(z) / dz through its output
    for i in reversed(range(n)):
        p = f'{prefix_k}kan_layers.{i}.'
        xn = torch.tanh(ins[i]).detach().requires_grad_(True)
        j, vals = ref_cpu.closed_form_basis(xn, g[p + 'knots'])
        dvals = torch.stack([torch.autograd.grad(vals[..., m].sum(), xn, retain_graph=True)[0] for m in range(4)], -1)
        nb = g[p + 'knots'].numel() - 4
        idx = (j.unsqueeze(-1) - torch.arange(4)).clamp(0, nb - 1)            # basis j - m; dvals are zero where it does not exist
        W = g[p + 'spline_weights']                                           # (in, out, nb)
        Wg = W[torch.arange(W.shape[0])[None, :, None, None], torch.arange(W.shape[1])[None, None, :, None], idx[:, :, None, :]]
        dsp = (dvals[:, :, None, :] * Wg).sum(-1) * (1 - xn.detach() ** 2)[:, :, None]      # (B, in, out)
        gin = torch.einsum('bo,bio->bi', gz, dsp) + gz @ g[p + 'linear.weight']
        if i == 0:
            return value, gin
        gz = gin * (pres[i - 1] > 0)


def _autograd(feats, sd, stage, target):
    f = feats.double().clone().requires_grad_(True)
    sd64 = {k: v.double() for k, v in sd.items()}
    if target == 'kan_severity':
        out = ref_cpu.kan_module_forward(f, sd64, 'kan_module.')[:, 0]
    else:
        o = ref_cpu.heads_forward(f, sd64, stage)
        if target == 'ordinal_severity':
            p = ref_cpu.ordinal_probabilities(o['ordinal_logits'])
            out = (p * torch.arange(p.shape[1], dtype=torch.float64)).sum(1)
        else:
            out = o[target][:, 0]
    g, = torch.autograd.grad(out.sum(), f)
    return out.detach(), g


@pytest.mark.parametrize('config', ['default', 'non_default'])
def test_restated_seeds_match_autograd(config):
    g = torch.Generator().manual_seed(5)
    if config == 'default':
        sd = ref_cpu.init_rovit_state(seed=3)
    else:
        sd = ref_cpu.init_vit_state(1, g, prefix='backbone.model.')
        sd.update(ref_cpu.init_heads_state(hidden=64, num_classes=6, generator=g))
        sd.update(ref_cpu.init_kan_state([192, 32, 8, 1], 7, 3, g, prefix='kan_module.'))
    feats = torch.randn(16, 192, generator=g) * 0.8
    for t in ('ordinal_severity', 'mu', 'log_var', 'kan_severity'):
        v, d = restate_seed(feats, sd, t)
        v_ref, d_ref = _autograd(feats, sd, 4, t)
        assert torch.allclose(v, v_ref, rtol=1e-12, atol=1e-12), t
        scale = d_ref.abs().max(1)[0].clamp_min(1e-30)
        err = float(((d - d_ref).abs().max(1)[0] / scale).max())
        # the KAN derivative differentiates the closed-form basis (uniform-grid formula on the stored fp32 knots), autograd the oracle's
        # recursion on the same knots: the two bases differ by the knots' fp32 non-uniformity (~4e-7 of the image's maximum)
        assert err < (1e-6 if t == 'kan_severity' else 1e-10), (t, err)
        assert float(d.abs().max()) > 0, t


def test_restated_log_var_gate():
    sd = dict(ref_cpu.init_rovit_state(seed=4))
    feats = torch.randn(8, 192, generator=torch.Generator().manual_seed(6))
    sd['uncertainty_head.fc_logvar.bias'] = torch.full_like(sd['uncertainty_head.fc_logvar.bias'], 50.0)
    v, d = restate_seed(feats, sd, 'log_var')
    v_ref, d_ref = _autograd(feats, sd, 4, 'log_var')
    assert torch.equal(v, torch.full_like(v, 10.0)) and torch.equal(v_ref, v)
    assert float(d.abs().max()) == 0.0 and float(d_ref.abs().max()) == 0.0
