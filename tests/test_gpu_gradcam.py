"""GPU tests of Grad-CAM++ (csrc/gradcam.hip, rovit_vit_gradcam, rovit_hip/gradcam.py, explainability/gradcam.py): the CAM arithmetic
against an fp64 restatement of the reference's GradCAMPlusPlus.compute (explainability/gradcam.py:62-101) on the same taps, the taps
against the fp32 oracle and against the hook path, targets, determinism, batch independence, side effects and the drop-in class."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref_cpu  # noqa: E402  (checker only)

RAW_RTOL = 1e-4          # raw cam vs the restatement on the same taps, max-abs / that image's max (only summation order differs)
MAP_TOL = 2e-4           # (B,224,224) map, max-abs, same comparison


def dev():
    return torch.device('cuda:0')


def restate(act, grad):
    """gradcam.py:62-101 in fp64 for every image of the batch; F.interpolate(bilinear, align_corners=False) stands in for
    cv2.resize.  Returns (raw relu'd cam (B,14,14), map (B,224,224))."""
    a, g = act.double(), grad.double()
    num = g.pow(2)
    den = 2 * g.pow(2) + (a * g.pow(3)).sum(dim=1, keepdim=True)
    den = torch.where(den != 0.0, den, torch.ones_like(den))
    w = (num / den * torch.relu(g)).sum(dim=2, keepdim=True)
    B = a.shape[0]
    raw = torch.relu((w * a).sum(dim=2)[:, 1:].reshape(B, 14, 14))
    m = F.interpolate(raw[:, None], size=(224, 224), mode='bilinear', align_corners=False)[:, 0]
    mx = m.flatten(1).max(1)[0][:, None, None]
    mn = m.flatten(1).min(1)[0][:, None, None]
    return raw, torch.where(mx > 0, (m - mn) / (mx - mn), m)


def _model(seed=0, sd=None, **kw):
    from models.rovit_kan import RoViTKAN
    m = RoViTKAN(pretrained=False, **kw)
    m.load_state_dict(sd if sd is not None else ref_cpu.init_rovit_state(seed=seed), strict=True)
    return m.to(dev()).eval()


def _images(B, seed):
    return torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(seed))


def _corr(a, b):
    return float(np.corrcoef(a.flatten().double().cpu().numpy(), b.flatten().double().cpu().numpy())[0, 1])


def _cos(a, b):
    return float(F.cosine_similarity(a.flatten().double().cpu(), b.flatten().double().cpu(), dim=0))


@pytest.mark.parametrize('B', [1, 7, 64])
def test_cam_arithmetic_matches_restatement_on_the_same_taps(B):
    from rovit_hip.gradcam import grad_cam_pp
    m = _model(seed=1)
    x = _images(B, 10 + B).to(dev())
    amap, taps = grad_cam_pp(m, x, return_taps=True)
    raw = grad_cam_pp(m, x, upsample=False)
    assert amap.shape == (B, 224, 224) and raw.shape == (B, 14, 14) and taps.act.shape == (B, 197, 192) and taps.grad.shape == (B, 197, 192)
    ref_raw, ref_map = restate(taps.act, taps.grad)
    scale = ref_raw.flatten(1).abs().max(1)[0].clamp_min(1e-30)
    rel = float(((raw.double() - ref_raw).flatten(1).abs().max(1)[0] / scale).max())
    err = float((amap.double() - ref_map).abs().max())
    print(f'B={B}: raw max-abs / image max {rel:.2e}, map max-abs {err:.2e}')
    assert rel <= RAW_RTOL, rel
    assert err <= MAP_TOL, err


def _oracle(sd, x, classes=None):
    taps = {}
    rp = {k: v.clone() for k, v in sd.items()}
    feats = ref_cpu.vit_forward(x, rp, prefix='backbone.model.', tap_norm1=(11, taps))
    logits = ref_cpu.heads_forward(feats, rp, 1)['cls_logits']
    if classes is None:
        classes = logits.argmax(1)
    g, = torch.autograd.grad(logits.gather(1, classes[:, None]).sum(), taps['y'])
    return taps['y'].detach(), g, logits.detach(), classes


def _check_against_oracle(m, sd, x, label):
    from rovit_hip.gradcam import grad_cam_pp
    a_ref, g_ref, logits_ref, cls_ref = _oracle(sd, x)
    raw, taps = grad_cam_pp(m, x.to(dev()), class_idx=cls_ref.to(dev()), upsample=False, return_taps=True)
    raw_ref, _ = restate(a_ref, g_ref)
    # the head's ReLU mask from the bf16 engine's features and from the oracle's: where a hidden unit near zero flips, the two gradients
    # seed the backward with different rows of W1 (a discrete difference, not rounding)
    w1, b1 = sd['classification_head.fc1.weight'], sd['classification_head.fc1.bias']
    with torch.no_grad():
        f_ours = m.backbone(x.to(dev())).cpu()
        f_ref = ref_cpu.vit_forward(x, {k: v.clone() for k, v in sd.items()}, prefix='backbone.model.')
    flips = ((f_ours @ w1.T + b1 > 0) != (f_ref @ w1.T + b1 > 0)).sum(1)
    for b in range(x.shape[0]):
        a_err = float((taps.act[b].cpu() - a_ref[b]).abs().max())
        cos = _cos(taps.grad[b], g_ref[b])
        cc = _corr(raw[b], raw_ref[b])
        top2 = raw_ref[b].flatten().topk(2)[0]
        lead = float(top2[0] - top2[1]) >= 0.05 * float(top2[0])
        same = int(raw[b].argmax()) == int(raw_ref[b].argmax())
        print(f'{label} image {b}: act max-abs {a_err:.2e}, grad cosine {cos:.5f}, raw-cam correlation {cc:.5f}, '
              f'top patch lead {lead}, same top {same}, head-mask flips {int(flips[b])}')
        assert a_err < 6e-2 and cc > 0.99, (b, a_err, cc)
        assert cos > (0.97 if flips[b] == 0 else 0.9), (b, cos, int(flips[b]))
        if lead:
            assert same, b


def test_against_fp32_oracle():
    sd = ref_cpu.init_rovit_state(seed=17)
    _check_against_oracle(_model(sd=sd), sd, _images(8, 3), 'default head')


def test_against_fp32_oracle_non_default_head():
    g = torch.Generator().manual_seed(23)
    sd = ref_cpu.init_vit_state(12, g, prefix='backbone.model.')
    sd.update(ref_cpu.init_heads_state(hidden=64, num_classes=6, generator=g))
    sd.update(ref_cpu.init_kan_state([192, 64, 16, 1], 5, 3, g, prefix='kan_module.'))
    m = _model(sd=sd, hidden_dim=64, num_classes=6)
    _check_against_oracle(m, sd, _images(8, 4), 'hidden 64 / 6 classes')


def _hook_path(m, x, cls):
    """The reference's recipe on the fused path (gradcam.py:18-60), all images at once: one backward of sum_b logits[b, cls_b]."""
    cap = {}
    target = m.backbone.model.blocks[-1].norm1
    h1 = target.register_forward_hook(lambda mod, inp, outp: cap.__setitem__('act', outp.detach()))
    h2 = target.register_full_backward_hook(lambda mod, gin, gout: cap.__setitem__('grad', gout[0].detach()))
    try:
        out = m(x.requires_grad_(True))
        m.zero_grad()
        out['cls_logits'].gather(1, cls[:, None]).sum().backward()
    finally:
        h1.remove()
        h2.remove()
    m.zero_grad(set_to_none=True)
    return cap['act'], cap['grad']


def test_against_hook_path():
    from rovit_hip.gradcam import grad_cam_pp
    m = _model(seed=29)
    x = _images(4, 5).to(dev())
    cls = torch.tensor([0, 1, 2, 3], device=dev())
    amap, taps = grad_cam_pp(m, x, class_idx=cls, return_taps=True)
    act_h, grad_h = _hook_path(m, x.clone(), cls)
    _, map_h = restate(act_h, grad_h)
    scale = float(act_h.abs().max())
    a_err = float((taps.act - act_h).abs().max())
    print(f'vs hook path: act max-abs {a_err:.2e} (scale {scale:.2e})')
    assert a_err <= 1e-5 * scale, a_err
    for b in range(4):
        cos = _cos(taps.grad[b], grad_h[b])
        cc = _corr(amap[b], map_h[b])
        print(f'  image {b} (class {b}): grad cosine {cos:.6f}, map correlation {cc:.6f}')
        assert cos > 0.995 and cc > 0.999, (b, cos, cc)


def test_targets():
    from rovit_hip.gradcam import grad_cam_pp
    from rovit_hip import RovitHipError
    m = _model(seed=31)
    x = _images(6, 6).to(dev())
    with torch.no_grad():
        ref = m(x)['cls_logits']
    amap, taps = grad_cam_pp(m, x, return_taps=True)
    assert float((taps.logits - ref).abs().max()) < 1e-4
    top2 = ref.topk(2, dim=1)[0]
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3
    assert bool(clear.any())
    assert torch.equal(taps.target[clear], ref.argmax(1)[clear])
    # an int and a (B,) tensor give the maps of batch-1 calls with those classes
    per = torch.tensor([3, 0, 2, 1, 1, 0], device=dev())
    m_int = grad_cam_pp(m, x, class_idx=2)
    m_vec = grad_cam_pp(m, x, class_idx=per)
    for k in range(6):
        one_int = grad_cam_pp(m, x[k:k + 1], class_idx=2)[0]
        one_vec = grad_cam_pp(m, x[k:k + 1], class_idx=int(per[k]))[0]
        assert float((m_int[k] - one_int).abs().max()) <= MAP_TOL, k
        assert float((m_vec[k] - one_vec).abs().max()) <= MAP_TOL, k
    # distinct targets: distinct gradients always, and distinct maps wherever the relu'd cam is not all zero (sum_d a[n,d] has one
    # sign over most tokens after a LayerNorm, so a target whose w is small there can leave an all-zero map)
    runs = [[grad_cam_pp(m, x[k:k + 1], class_idx=c, return_taps=True) for c in range(4)] for k in range(6)]
    k = max(range(6), key=lambda k: sum(bool(mp.any()) for mp, _ in runs[k]))
    assert sum(bool(mp.any()) for mp, _ in runs[k]) >= 2
    for i in range(4):
        for j in range(i + 1, 4):
            assert not torch.equal(runs[k][i][1].grad, runs[k][j][1].grad), (i, j)
            if runs[k][i][0].any() or runs[k][j][0].any():
                assert not torch.equal(runs[k][i][0], runs[k][j][0]), (i, j)
    for bad in (-1, 4, torch.tensor([0, 1, 2, 3, 4, 0], device=dev()), torch.tensor([0, 1], device=dev()),
                torch.zeros(6, device=dev()), 1.0):
        with pytest.raises(RovitHipError, match='class_idx'):
            grad_cam_pp(m, x, class_idx=bad)


def test_determinism_and_batch_independence():
    from rovit_hip.gradcam import grad_cam_pp
    m = _model(seed=37)
    x = _images(64, 7).to(dev())
    a = grad_cam_pp(m, x)
    b = grad_cam_pp(m, x)
    assert torch.equal(a, b)
    assert bool(torch.isfinite(a).all())
    x37 = _images(37, 8).to(dev())
    batch = grad_cam_pp(m, x37)
    worst, identical = 0.0, True
    for k in (0, 18, 36):
        one = grad_cam_pp(m, x37[k:k + 1])[0]
        worst = max(worst, float((one - batch[k]).abs().max()))
        identical = identical and torch.equal(one, batch[k])
    print(f'batch of 37 vs alone: map max-abs {worst:.2e}, bit-identical: {identical}')
    assert worst <= MAP_TOL, worst


def test_no_side_effects():
    from rovit_hip.gradcam import grad_cam_pp
    from rovit_hip import RovitHipError
    m = _model(seed=41)
    x = _images(5, 9).to(dev())
    ref = grad_cam_pp(m, x)
    assert all(p.grad is None for p in m.parameters())
    with torch.no_grad():
        assert torch.equal(grad_cam_pp(m, x), ref)
    # frozen backbone: the hook path refuses, this path works
    m.backbone.freeze()
    target = m.backbone.model.blocks[-1].norm1
    h = target.register_forward_hook(lambda *a: None)
    try:
        with pytest.raises(RovitHipError, match='norm1'):
            m(x)
    finally:
        h.remove()
    assert torch.equal(grad_cam_pp(m, x), ref)
    m.backbone.unfreeze()
    # fp32 precision and train mode: same maps, settings left as they were
    m.backbone.model.precision = 'fp32'
    assert torch.equal(grad_cam_pp(m, x), ref)
    assert m.backbone.model.precision == 'fp32'
    m.backbone.model.precision = 'bf16'
    m.train()
    assert torch.equal(grad_cam_pp(m, x), ref)
    assert m.training
    m.eval()
    for stage in (1, 2, 3, 4):
        m.curriculum_stage = stage
        assert torch.equal(grad_cam_pp(m, x), ref), stage
    assert all(p.grad is None for p in m.parameters())


def test_beside_a_training_step():
    from rovit_hip.gradcam import grad_cam_pp
    m = _model(seed=43)
    x = _images(24, 11).to(dev())
    y = torch.randint(0, 4, (24,), generator=torch.Generator().manual_seed(1)).to(dev())

    def step(with_cam):
        m.zero_grad(set_to_none=True)
        out = m(x)
        last = m.backbone.model.engine.last_ws
        if with_cam:
            grad_cam_pp(m, x[:7])
            grad_cam_pp(m, x)
            assert m.backbone.model.engine.last_ws is last
        ref_cpu.joint_loss(out, y, y, 4)['total_loss'].backward()
        torch.cuda.synchronize()
        return [None if p.grad is None else p.grad.clone() for p in m.parameters()]
    m.eval()
    plain = step(False)
    with_cam = step(True)
    assert sum(g is not None for g in plain) > 150
    for i, (a, b) in enumerate(zip(plain, with_cam)):
        assert (a is None and b is None) or torch.equal(a, b), i


def test_model_method_and_drop_in():
    from rovit_hip.gradcam import grad_cam_pp
    from explainability import GradCAMPlusPlus
    m = _model(seed=47)
    x = _images(3, 12)
    assert torch.equal(m.grad_cam_pp(x.to(dev())), grad_cam_pp(m, x.to(dev())))
    assert torch.equal(m.grad_cam_pp(x.to(dev()), class_idx=1, upsample=False), grad_cam_pp(m, x.to(dev()), 1, upsample=False))
    cam = GradCAMPlusPlus(m)
    m.train()
    xr = x.clone()
    one = cam.compute(xr)
    assert not m.training and not xr.requires_grad
    batch = cam.compute_batch(x)
    assert isinstance(one, np.ndarray) and one.shape == (224, 224)
    assert batch.shape == (3, 224, 224) and batch.is_cuda
    assert np.array_equal(one, batch[0].cpu().numpy())
    assert 0.0 <= float(one.min()) and float(one.max()) <= 1.0
    assert np.array_equal(cam.compute(x, class_idx=2), cam.compute_batch(x, 2)[0].cpu().numpy())
    with pytest.raises(NotImplementedError):
        cam.visualize(x, np.zeros((224, 224, 3), np.uint8))
