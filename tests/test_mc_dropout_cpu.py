"""CPU tests of the MC-dropout surface: rovit_head_mc_fwd refuses bad descriptors before anything is launched, the Python entry point's
argument checks, and the Dropout-flag semantics of the heads (each head's nn.Dropout module decides, as torch.nn.Dropout does)."""
import ctypes

import pytest
import torch


@pytest.fixture(scope='module')
def native():
    from rovit_hip import native as n
    import os
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    n.load()
    return n


def _desc(native, **kw):
    d = native.HeadMC()
    d.batch, d.embed, d.hid, d.num_classes, d.stage, d.num_samples, d.drop_p = 2, 192, 128, 4, 4, 8, 0.3
    d.features = 16          # dummy non-null, 16-byte aligned addresses: every call here is refused before a launch
    for i in range(14):
        d.head_params[i] = 16
    for f in ('class_probs', 'class_probs_std', 'pred_entropy', 'exp_entropy', 'mutual_info', 'ord_probs', 'ord_severity',
              'ord_severity_std', 'unc_mu', 'epistemic_var', 'aleatoric_var', 'unc_std'):
        setattr(d, f, 16)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_abi_version(native):
    assert native.ABI_VERSION == 440 and native.load().rovit_version() == 440


@pytest.mark.parametrize('kw,match', [({'num_samples': 0}, 'samples'), ({'num_samples': 4097}, 'samples'), ({'batch': 0}, 'batch'),
                                      ({'embed': 770}, 'embed'), ({'embed': 190}, 'embed'), ({'hid': 260}, 'hidden'), ({'hid': 66}, 'hidden'),
                                      ({'num_classes': 1}, 'classes'), ({'num_classes': 9}, 'classes'), ({'stage': 0}, 'stage'),
                                      ({'stage': 5}, 'stage'), ({'drop_p': 1.0}, 'dropout'), ({'drop_p': -0.1}, 'dropout'),
                                      ({'features': None}, 'features'), ({'features': 20}, 'features'), ({'class_probs': None}, 'missing'),
                                      ({'ord_severity': None}, 'ordinal'), ({'unc_std': None}, 'uncertainty')])
def test_head_mc_rejects_bad_descriptors(native, kw, match):
    with pytest.raises(native.RovitHipError, match=match):
        native.call('rovit_head_mc_fwd', ctypes.byref(_desc(native, **kw)), None)


def test_head_mc_stage_gates_outputs(native):
    # stage 1 needs no ordinal / uncertainty outputs, but refuses per-sample buffers of heads it does not run
    d = _desc(native, stage=1, s_mu=16, s_lv=16)
    with pytest.raises(native.RovitHipError, match='stage 1'):
        native.call('rovit_head_mc_fwd', ctypes.byref(d), None)


def _model():
    from models.rovit_kan import RoViTKAN
    return RoViTKAN(pretrained=False)


def test_python_entry_point_checks_before_any_launch():
    from rovit_hip.mc_dropout import mc_dropout_predict
    from rovit_hip.native import RovitHipError
    m = _model()
    x = torch.zeros(2, 3, 224, 224)
    for bad in (0, 4097, True, 1.0, None):
        with pytest.raises(RovitHipError, match='num_samples'):
            mc_dropout_predict(m, x, bad)
    with pytest.raises(RovitHipError, match='seed'):
        mc_dropout_predict(m, x, 4, seed=2 ** 64)
    with pytest.raises(RovitHipError, match='offset'):
        mc_dropout_predict(m, x, 4, seed=None, offset=5)
    with pytest.raises(RovitHipError, match='GPU'):
        m.predict_mc(x, num_samples=4)
    with pytest.raises(RovitHipError, match='images'):
        m.predict_mc(torch.zeros(3, 224, 224), num_samples=4)


def test_enable_disable_dropout_switch_only_the_heads():
    import torch.nn as nn
    m = _model().eval()
    m.enable_dropout()
    heads = (m.classification_head, m.ordinal_head, m.uncertainty_head)
    on = {id(h.dropout) for h in heads}
    assert not m.training and all(h.dropout.training for h in heads)
    assert all(not mod.training for mod in m.modules() if id(mod) not in on)
    assert all(not mod.training for mod in m.modules() if isinstance(mod, nn.Dropout) and id(mod) not in on)
    m.disable_dropout()
    assert not any(mod.training for mod in m.modules())


def test_each_head_obeys_its_own_dropout_module():
    from models.heads import ClassificationHead, dropout_active
    h = ClassificationHead(192, 128, 4, 0.3).eval()
    x = torch.zeros(2, 192)
    assert h._hidden_mask(x) is None
    h.dropout.train()                          # the reference's recipe: model.eval(), then the Dropout modules back to train()
    assert dropout_active(h.dropout)
    mk = h._hidden_mask(x)
    assert mk is not None and mk.shape == (2, 128)
    h.train()
    h.dropout.eval()                           # and the other way round: a Dropout in eval mode draws nothing
    assert h._hidden_mask(x) is None
    h.dropout.train()
    h.dropout.p = 0.0
    assert h._hidden_mask(x) is None and not dropout_active(h.dropout)


def test_model_dropout_probability_follows_the_modules():
    m = _model()
    heads = (m.classification_head, m.ordinal_head, m.uncertainty_head)
    m.train()
    assert [m._drop_p(h) for h in heads] == [0.3] * 3
    m.eval()
    assert [m._drop_p(h) for h in heads] == [0.0] * 3
    m.enable_dropout()
    assert [m._drop_p(h) for h in heads] == [0.3] * 3
