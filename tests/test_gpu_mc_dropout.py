"""GPU tests of Monte-Carlo dropout over the heads (csrc/mc_dropout.hip, rovit_head_mc_fwd; rovit_hip/mc_dropout.py; RoViTKAN.predict_mc)
and of the Dropout-flag semantics the reference's MC-dropout recipe relies on (model.eval(), then the heads' nn.Dropout modules back to
train(): models/heads.py:14,35,87, experiments/baselines.py:48-52).

The masks are replayed with oracle/philox.py (pinned to the Random123 known-answer vectors); per-sample outputs are checked against an
fp64 restatement of models/heads.py on the replayed masks (1e-5 relative: fp32 sums of 192 and 128 terms), statistics against fp64
arithmetic on the kernel's own per-sample outputs."""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from oracle import ref_cpu  # noqa: E402  (checker only)
from oracle.philox import head_phase_masks, philox4x32_10  # noqa: E402


def dev():
    return torch.device('cuda:0')


def _model(seed=0, hid=128, classes=4):
    from models.rovit_kan import RoViTKAN
    sd = ref_cpu.init_rovit_state(seed=seed)
    if (hid, classes) != (128, 4):
        sd.update(ref_cpu.init_heads_state(192, hid, classes, torch.Generator().manual_seed(seed + 1)))
    m = RoViTKAN(pretrained=False, hidden_dim=hid, num_classes=classes)
    m.load_state_dict(sd, strict=True)
    return m.to(dev()).eval()


def _images(B, seed):
    return torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(seed)).to(dev())


def _masks(B, hid, p, seed, offset, T):
    """(T, 3, B, hid) scaled keep-masks of the kernel's draw: counter (b * hid + k, t, offset lo, offset hi), key seed."""
    n = B * hid
    keep = np.float32(1.0) - np.float32(p)
    out = np.empty((T, 3, B, hid), np.float32)
    for t in range(T):
        words = philox4x32_10([np.arange(n, dtype=np.uint64), np.full(n, t, np.uint64), np.full(n, offset & 0xFFFFFFFF, np.uint64),
                               np.full(n, (offset >> 32) & 0xFFFFFFFF, np.uint64)], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
        for h in range(3):
            u = (words[h] >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
            out[t, h] = np.where(u < keep, np.float32(1.0) / keep, np.float32(0.0)).reshape(B, hid)
    return torch.from_numpy(out)


def _restate(m, features, masks):
    """fp64 heads.py (:17-22, 38-43, 91-102) of every sample: masks (T, 3, B, hid) -> dict of (T, B, .)"""
    f = features.double().cpu()
    P = [p.detach().double().cpu() for p in m._head_params()]
    out = {'cls_logits': [], 'ordinal_logits': [], 'mu': [], 'log_var': []}
    for t in range(masks.shape[0]):
        mk = masks[t].double()
        h0 = torch.relu(f @ P[0].T + P[1]) * mk[0]
        h1 = torch.relu(f @ P[4].T + P[5]) * mk[1]
        h2 = torch.relu(f @ P[8].T + P[9]) * mk[2]
        out['cls_logits'].append(h0 @ P[2].T + P[3])
        out['ordinal_logits'].append(h1 @ P[6].T + P[7])
        out['mu'].append(h2 @ P[10].T + P[11])
        out['log_var'].append(torch.clamp(h2 @ P[12].T + P[13], -10.0, 10.0))
    return {k: torch.stack(v) for k, v in out.items()}


def _stats(samples, stage):
    """fp64 statistics over the sample axis of the kernel's own per-sample outputs (variances divided by T)."""
    cl = samples['cls_logits'].double().cpu()
    lp = torch.log_softmax(cl, dim=2)
    p = lp.exp()
    ent = -torch.where(p > 0, p * lp, torch.zeros_like(p)).sum(2)
    pbar = p.mean(0)
    hp = -torch.where(pbar > 0, pbar * pbar.log(), torch.zeros_like(pbar)).sum(1)
    out = {'class_probs': pbar, 'class_probs_std': p.var(0, unbiased=False).sqrt(), 'predictive_entropy': hp,
           'expected_entropy': ent.mean(0), 'mutual_information': (hp - ent.mean(0)).clamp_min(0.0)}
    if stage >= 2:
        cp = torch.sigmoid(samples['ordinal_logits'].double().cpu())
        po = torch.cat([cp[..., :1], cp[..., 1:] - cp[..., :-1], 1.0 - cp[..., -1:]], dim=2)
        lv = torch.arange(po.shape[2], dtype=torch.float64)
        sev = (po * lv).sum(2, keepdim=True)
        out.update(ordinal_probs=po.mean(0), ordinal_severity=(po.mean(0) * lv).sum(1, keepdim=True),
                   ordinal_severity_std=sev.var(0, unbiased=False).sqrt())
    if stage >= 3:
        mu, lvar = samples['mu'].double().cpu(), samples['log_var'].double().cpu()
        epi, ale = mu.var(0, unbiased=False), lvar.exp().mean(0)
        out.update(uncertainty_mu=mu.mean(0), epistemic_var=epi, aleatoric_var=ale, uncertainty_std=(epi + ale).sqrt())
    return out


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1.0))


NEW_KEYS = {1: {'class_probs_std', 'predictive_entropy', 'expected_entropy', 'mutual_information'},
            2: {'ordinal_severity_std'}, 3: {'epistemic_var', 'aleatoric_var'}}


def _new_keys(stage):
    return set().union(*(v for s, v in NEW_KEYS.items() if s <= stage))


# ---- 1. masks pinned; every sample against the fp64 restatement ------------------------------------------------------------------
@pytest.mark.parametrize('cfg', [(128, 4), (64, 6)], ids=['default', 'hid64_c6'])
@pytest.mark.parametrize('T', [1, 5, 64])
@pytest.mark.parametrize('B', [1, 7, 256])
def test_samples_match_replayed_masks(B, T, cfg):
    from rovit_hip.mc_dropout import mc_dropout_predict
    hid, classes = cfg
    m = _model(seed=3, hid=hid, classes=classes)
    x = _images(B, 100 + B)
    seed, offset = 0x1234ABCD5678, 0x0000000300000010
    pred = mc_dropout_predict(m, x, T, seed, True, offset=offset)
    masks = _masks(B, hid, 0.3, seed, offset, T)
    ref0 = head_phase_masks(B, hid, 0.3, seed, offset)
    for h in range(3):
        assert np.array_equal(masks[0, h].numpy(), ref0[h])                       # sample 0 is the head phase's draw
    s = pred['samples']
    ref = _restate(m, pred['features'], masks)
    for k in ('cls_logits', 'ordinal_logits', 'mu', 'log_var'):
        assert s[k].shape == ref[k].shape, k
        assert _rel(s[k], ref[k]) < 1e-5, (k, _rel(s[k], ref[k]))
    # sample 0 against the training head phase launched with the same seed and offset (same kernels' arithmetic)
    from rovit_hip.functions import HeadPhaseFn
    cfgd = {'stage': 3, 'masks': None, 'drop_p': 0.3, 'seed': seed, 'offset': offset, 'kan_dims': [], 'kan_knots': [], 'kan_acts': [],
            'grad_views': None}
    with torch.no_grad():
        hp = HeadPhaseFn.apply(pred['features'], cfgd, *m._head_params())
    for k, o in zip(('cls_logits', 'ordinal_logits', 'mu', 'log_var'), hp[:4]):
        torch.testing.assert_close(s[k][0], o, rtol=1e-6, atol=1e-6)


# ---- 2. statistics -------------------------------------------------------------------------------------------------------------
def _check_stats(pred, stage, rtol=5e-6, var_rtol=1e-6):
    ref = _stats(pred['samples'], stage)
    for k, r in ref.items():
        got = pred[k].double().cpu().reshape(r.shape)
        tol = var_rtol if k in ('epistemic_var', 'uncertainty_mu') else rtol
        err = float((got - r).abs().max())
        assert err <= tol * max(1.0, float(r.abs().max())) + 1e-7, (k, err)
    torch.testing.assert_close(pred['class'].cpu(), pred['class_probs'].argmax(1).cpu())


@pytest.mark.parametrize('stage', [1, 2, 3, 4])
def test_statistics_match_fp64_restatement(stage):
    m = _model(seed=4)
    m.curriculum_stage = stage
    pred = m.predict_mc(_images(7, 7), num_samples=64, seed=99, return_samples=True)
    _check_stats(pred, stage)
    assert float(pred['mutual_information'].min()) >= 0.0
    assert float(pred['class_probs_std'].max()) > 0.0


def test_statistics_t4096_low_variance_mu():
    """mu ~ 100 with a spread ~1e-3: E[x^2] - E[x]^2 in fp32 would lose every digit of the variance."""
    m = _model(seed=5)
    with torch.no_grad():
        m.uncertainty_head.fc_mu.weight.mul_(1e-3)
        m.uncertainty_head.fc_mu.bias.fill_(100.0)
    pred = m.predict_mc(_images(3, 8), num_samples=4096, seed=7, return_samples=True)
    epi = pred['epistemic_var']
    assert float(epi.min()) > 0.0 and float(epi.max()) < 1e-3 * float(pred['uncertainty_mu'].abs().min()) ** 2
    _check_stats(pred, 4)
    ref = _stats(pred['samples'], 4)['epistemic_var']
    assert float(((epi.double().cpu() - ref).abs() / ref).max()) < 1e-5


# ---- 3. p = 0 is predict() -----------------------------------------------------------------------------------------------------
def test_p0_degenerates_to_predict():
    m = _model(seed=6)
    for h in (m.classification_head, m.ordinal_head, m.uncertainty_head):
        h.dropout.p = 0.0
    x = _images(9, 9)
    mc = m.predict_mc(x, num_samples=16, seed=1)
    pr = m.predict(x)
    torch.testing.assert_close(mc['class_probs'], pr['class_probs'], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(mc['ordinal_probs'], pr['ordinal_probs'], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(mc['uncertainty_mu'], pr['uncertainty_mu'], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(mc['aleatoric_var'], pr['uncertainty_std'] ** 2, rtol=1e-5, atol=1e-7)
    for k in ('class_probs_std', 'mutual_information', 'ordinal_severity_std', 'epistemic_var'):
        assert float(mc[k].abs().max()) == 0.0, k
    assert torch.equal(mc['class'], pr['class'])
    assert torch.equal(mc['kan_severity'], pr['kan_severity'])
    assert torch.equal(mc['features'], pr['features'])


# ---- 4. stage gating -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stage', [1, 2, 3, 4])
def test_stage_gating_matches_predict(stage):
    m = _model(seed=7)
    m.curriculum_stage = stage
    x = _images(3, 3)
    mc = m.predict_mc(x, num_samples=4, seed=2, return_samples=True)
    pr = m.predict(x)
    assert set(mc) - {'samples'} == set(pr) | _new_keys(stage)
    want = {'cls_logits'} | ({'ordinal_logits'} if stage >= 2 else set()) | ({'mu', 'log_var'} if stage >= 3 else set())
    assert set(mc['samples']) == want


# ---- 5. determinism and seeding ------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a if k != 'samples')


def test_determinism_and_seeding():
    m = _model(seed=8)
    x = _images(16, 16)
    a = m.predict_mc(x, num_samples=32, seed=5)
    b = m.predict_mc(x, num_samples=32, seed=5)
    c = m.predict_mc(x, num_samples=32, seed=6)
    assert _same(a, b)
    assert not torch.equal(a['class_probs'], c['class_probs'])
    torch.manual_seed(123)
    g = torch.cuda.default_generators[0]
    off0 = g.get_offset()
    d1 = m.predict_mc(x, num_samples=32)
    d2 = m.predict_mc(x, num_samples=32)
    assert g.get_offset() > off0
    assert not torch.equal(d1['class_probs'], d2['class_probs'])
    torch.manual_seed(123)
    e1 = m.predict_mc(x, num_samples=32)
    e2 = m.predict_mc(x, num_samples=32)
    assert _same(d1, e1) and _same(d2, e2)
    # an explicit seed ignores (and leaves) the generator's state
    off = g.get_offset()
    f = m.predict_mc(x, num_samples=32, seed=5)
    assert g.get_offset() == off and _same(a, f)


# ---- 6. batch independence -----------------------------------------------------------------------------------------------------
def test_batch_independence():
    m = _model(seed=9)
    x1 = _images(37, 37)
    x2 = _images(37, 38)
    keep = [0, 5, 36]
    x2[keep] = x1[keep]
    a = m.predict_mc(x1, num_samples=20, seed=3)
    b = m.predict_mc(x2, num_samples=20, seed=3)
    for k in a:
        if a[k].dim() >= 1 and a[k].shape[0] == 37:
            assert torch.equal(a[k][keep], b[k][keep]), k
    assert not torch.equal(a['class_probs'][1], b['class_probs'][1])


# ---- 7. no side effects ----------------------------------------------------------------------------------------------------------
def _train_step(m, x, y):
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    out = m(x)
    loss = ref_cpu.joint_loss(out, y, y, 4)['total_loss']
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def test_no_side_effects():
    m = _model(seed=10)
    m.train()
    m.ordinal_head.eval()
    m.backbone.model.blocks[3].attn.attn_drop.eval()
    flags = [mod.training for mod in m.modules()]
    x = _images(4, 4)
    m.predict_mc(x, num_samples=8, seed=1)
    m.predict_mc(x, num_samples=8)
    assert [mod.training for mod in m.modules()] == flags
    assert all(p.grad is None for p in m.parameters())

    y = torch.tensor([0, 1, 2, 3], device=dev())
    a = _model(seed=10).train()
    b = _model(seed=10).train()
    torch.manual_seed(42)
    sa = _train_step(a, x, y)
    torch.manual_seed(42)
    b.predict_mc(x, num_samples=8, seed=11)
    assert all(p.grad is None for p in b.parameters())
    sb = _train_step(b, x, y)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


# ---- 8. the reference's recipe on the fused forward --------------------------------------------------------------------------------
def _restate_logits(m, features, masks):
    return _restate(m, features, torch.from_numpy(np.stack(masks))[None])


def test_reference_recipe_draws_dropout():
    m = _model(seed=11)
    x = _images(6, 6)
    with torch.no_grad():
        base = m(x)
    m.eval()
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.train()
    g = torch.cuda.default_generators[0]
    B, hid = 6, 128
    outs, draws = [], []
    with torch.no_grad():
        for _ in range(2):
            draws.append((g.initial_seed(), g.get_offset()))
            outs.append(m(x))
    assert not torch.equal(outs[0]['cls_logits'], outs[1]['cls_logits'])
    for o in outs:                                  # the backbone's Dropout(0.0) modules in train mode change nothing
        assert torch.equal(o['features'], base['features'])
        assert torch.equal(o['kan_severity'], base['kan_severity'])
    for o, (seed, off) in zip(outs, draws):
        ref = _restate_logits(m, o['features'], head_phase_masks(B, hid, 0.3, seed, off))
        for k in ('cls_logits', 'ordinal_logits', 'mu', 'log_var'):
            assert _rel(o[k], ref[k][0]) < 1e-5, k
    # the same through enable_dropout() / disable_dropout()
    m.eval()
    m.enable_dropout()
    assert all(h.dropout.training for h in (m.classification_head, m.ordinal_head, m.uncertainty_head)) and not m.training
    with torch.no_grad():
        e1, e2 = m(x), m(x)
    assert not torch.equal(e1['cls_logits'], e2['cls_logits'])
    m.disable_dropout()
    with torch.no_grad():
        assert torch.equal(m(x)['cls_logits'], base['cls_logits'])


def test_each_head_follows_its_own_dropout_flag():
    """Heads that disagree take the per-module path with explicit masks: only the head whose Dropout is in train mode changes."""
    m = _model(seed=12)
    x = _images(5, 5)
    with torch.no_grad():
        base = m(x)
        m.classification_head.dropout.train()
        a, b = m(x), m(x)
    assert not torch.equal(a['cls_logits'], b['cls_logits'])
    for k in ('ordinal_logits', 'mu', 'log_var', 'kan_severity', 'features'):
        torch.testing.assert_close(a[k], base[k], rtol=1e-4, atol=1e-4)
        assert torch.equal(a[k], b[k]), k


def test_fp32_backbone_features():
    m = _model(seed=13)
    m.backbone.model.precision = 'fp32'
    x = _images(3, 13)
    mc = m.predict_mc(x, num_samples=8, seed=4)
    pr = m.predict(x)
    assert torch.equal(mc['features'], pr['features'])
    assert torch.equal(mc['kan_severity'], pr['kan_severity'])


# ---- 9. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    from rovit_hip.native import RovitHipError
    m = _model(seed=14)
    x = _images(2, 2)
    for bad in (0, -1, 4097, True, 2.5):
        with pytest.raises(RovitHipError, match='num_samples'):
            m.predict_mc(x, num_samples=bad)
    with pytest.raises(RovitHipError, match='GPU'):
        m.predict_mc(x.cpu(), num_samples=4)
    with pytest.raises(RovitHipError, match='empty'):
        m.predict_mc(x[:0], num_samples=4)
    m.curriculum_stage = 1
    m.ordinal_head.dropout.p = 0.5                  # inactive at stage 1: allowed
    m.predict_mc(x, num_samples=2, seed=0)
    m.curriculum_stage = 2
    with pytest.raises(RovitHipError, match='dropout'):
        m.predict_mc(x, num_samples=2, seed=0)
    with pytest.raises(RovitHipError, match='seed'):
        m.predict_mc(x, num_samples=2, seed=-1)
