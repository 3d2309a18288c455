"""GPU tests of the gradient with respect to the input images (rovit_patch_embed_dgrad, rovit_vit_backward_input, VitFn's image gradient,
RoViTKAN.input_gradients): x.grad against fp64 autograd through the oracle, the frozen-backbone (dgrad-only) backward against the full
one, the trainable backbone's parameter gradients with and without images that require grad, the pixel kernel against fp64 torch, input
dtypes and layouts, the reference's Grad-CAM++ hook recipe on a frozen backbone, input_gradients against autograd through the model and
its side effects, and integrated gradients against an fp64 oracle."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref_cpu  # noqa: E402  (checker only)

COS_MIN = 0.999           # per-image cosine of d target / d images against fp64 autograd
REL_MAX = 6e-2            # max-abs error / the image's max |oracle gradient| (the backbone gradient bound)
COS_FLIP = 0.9            # images whose head / KAN ReLU unit flips between the bf16 and the fp64 features
KERNEL_RTOL = 1e-5        # the pixel kernel against fp64 torch on the same bf16 operands
# completeness of 32-step integrated gradients on the depth-2 model: |sum attr - (f(x) - f(x'))| / |f(x) - f(x')|; the right Riemann
# rule's own error dominates: 0.036-0.090 (class) and 0.037-0.105 (mu) measured.  kan_severity is reported, not bounded: the truncated
# spline jumps where a KAN input crosses the cutoff along the path, and a jump has no gradient (gaps 1.7-7.6 measured)
COMPLETENESS_MAX = 0.2


def dev():
    return torch.device('cuda:0')


def _model(depth=2, seed=0):
    from models.backbone import DeiTTiny
    from models.rovit_kan import RoViTKAN
    sd = ref_cpu.init_rovit_state(depth=depth, seed=seed)
    m = RoViTKAN(pretrained=False)
    if depth != 12:
        m.backbone.model = DeiTTiny(depth=depth)
    m.load_state_dict(sd, strict=True)
    return m.to(dev()).eval(), sd


def _images(B, seed):
    return torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(seed))


def _cos(a, b):
    return float(F.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0))


def _freeze(m, backbone=True):
    for p in m.backbone.parameters():
        p.requires_grad_(not backbone)


def _sd64(sd):
    return {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}


def _oracle_image_grad(x, sd64, seed_fn):
    """fp64 autograd of seed_fn(features) . features through the oracle backbone, seed_fn giving d target / d features (B,192)."""
    xd = x.double().detach().requires_grad_(True)
    feats = ref_cpu.vit_forward(xd, sd64, prefix='backbone.model.')
    g = seed_fn(feats.detach())
    gx, = torch.autograd.grad(feats, xd, grad_outputs=g)
    return gx, feats.detach()


def _head_seed(sd64, f, value_fn):
    """d value / d features of the oracle's heads and KAN at features f (fp64)."""
    f = f.double().detach().requires_grad_(True)
    out = ref_cpu.heads_forward(f, sd64, 4)
    out['kan_severity'] = ref_cpu.kan_module_forward(f, sd64, 'kan_module.')
    g, = torch.autograd.grad(value_fn(out).sum(), f)
    return g


def _hidden_signs(sd64, f):
    """Signs of the classification head's hidden pre-activation (its ReLU mask)."""
    return torch.sign(f.double() @ sd64['classification_head.fc1.weight'].t() + sd64['classification_head.fc1.bias'])


def _check_images(got, want, flipped=None):
    """Per-image cosine and max-abs error against the oracle; returns the worst (cosine, relative error) of the unflipped images."""
    worst_c, worst_r = 1.0, 0.0
    for b in range(got.shape[0]):
        g, w = got[b].double().cpu(), want[b].cpu()
        c = _cos(g, w)
        r = float((g - w).abs().max() / w.abs().max())
        if flipped is not None and bool(flipped[b]):
            assert c > COS_FLIP, (b, c)
            continue
        assert c >= COS_MIN and r <= REL_MAX, (b, c, r)
        worst_c, worst_r = min(worst_c, c), max(worst_r, r)
    return worst_c, worst_r


@pytest.fixture(params=['two_launch', 'one_launch'])
def mlp_path(request):
    from rovit_hip import native
    from rovit_hip.functions import VitEngine
    VitEngine.default_mlp_path = native.MLP_ONE_LAUNCH if request.param == 'one_launch' else native.MLP_TWO_LAUNCH
    yield request.param
    VitEngine.default_mlp_path = native.MLP_AUTO


# ---- 1. x.grad against the fp64 oracle -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('depth,B', [(2, 1), (2, 5), (12, 3)])
def test_image_grad_against_fp64_oracle(depth, B, mlp_path):
    m, sd = _model(depth, seed=10 + B)
    sd64 = _sd64(sd)
    x = _images(B, B)
    c = 1
    # (a) one class logit; (b) the joint loss at stage 4
    y = torch.randint(0, 4, (B,), generator=torch.Generator().manual_seed(3))
    sev = torch.randint(0, 4, (B,), generator=torch.Generator().manual_seed(4))
    seeds = {'class': lambda out: out['cls_logits'][:, c],
             'joint': lambda out: ref_cpu.joint_loss(out, y.to(out['cls_logits'].device), sev.to(out['cls_logits'].device),
                                                     stage=4)['total_loss'].expand(out['cls_logits'].shape[0]) / out['cls_logits'].shape[0]}
    for name, value_fn in seeds.items():
        xg = x.clone().to(dev()).requires_grad_(True)
        out = m(xg)
        value_fn(out).sum().backward()
        assert xg.grad is not None and xg.grad.dtype == torch.float32 and xg.grad.shape == xg.shape
        f_hip = out['features'].detach().cpu()
        # the backbone's image gradient on the same seed: the oracle's heads evaluated at the HIP features (no flips possible)
        want, f_ref = _oracle_image_grad(x, sd64, lambda f: _head_seed(sd64, f_hip, value_fn))
        wc, wr = _check_images(xg.grad, want)
        print(f'depth {depth} B {B} {mlp_path} {name}: cosine >= {wc:.6f}, max-abs / max <= {wr:.3e}')
        # end to end (the class logit): the oracle's own features and head; images with a flipped ReLU unit are held to COS_FLIP.  Not
        # for the joint loss: its KAN term is a truncated spline that jumps at the cutoff, and the bf16 features put some of the 192
        # inputs of most images on the other side of it, so its end-to-end gradient is not comparable there
        if name != 'class':
            m.zero_grad(set_to_none=True)
            continue
        want_e2e, _ = _oracle_image_grad(x, sd64, lambda f: _head_seed(sd64, f, value_fn))
        flipped = (_hidden_signs(sd64, f_hip) != _hidden_signs(sd64, f_ref)).any(dim=1)
        wc, wr = _check_images(xg.grad, want_e2e, flipped)
        print(f'  end to end: {int(flipped.sum())} of {B} flipped; others cosine >= {wc:.6f}, <= {wr:.3e}')
        m.zero_grad(set_to_none=True)


# ---- 2. frozen backbone ----------------------------------------------------------------------------------------------------------

def _run(m, x, loss_fn):
    xg = x.clone().requires_grad_(True)
    loss_fn(m(xg)).backward()
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return xg.grad, grads


def _joint(out):
    B = out['cls_logits'].shape[0]
    y = torch.arange(B, device=out['cls_logits'].device) % 4
    return ref_cpu.joint_loss(out, y, (y + 1) % 4, stage=4)['total_loss']


@pytest.mark.parametrize('B', [3, 40])
def test_frozen_backbone_image_grad_matches_trainable(B):
    import rovit_hip.functions as fn
    m, _ = _model(2, seed=7)
    x = _images(B, 11).to(dev())
    gx_t, grads_t = _run(m, x, _joint)
    _freeze(m)
    calls = []
    orig = fn.call
    fn.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        gx_f, grads_f = _run(m, x, _joint)
    finally:
        fn.call = orig
    assert torch.equal(gx_f, gx_t)
    assert not any(n.startswith('backbone.') for n in grads_f)
    assert all(p.grad is None for p in m.backbone.parameters())
    heads = {n: g for n, g in grads_t.items() if not n.startswith('backbone.')}
    assert heads.keys() == grads_f.keys()
    for n in heads:
        assert torch.equal(grads_f[n], heads[n]), n
    assert 'rovit_vit_backward_input' in calls and 'rovit_vit_backward' not in calls


def test_dgrad_only_backward_leaves_flat_gradients_alone():
    m, _ = _model(2, seed=8)
    x = _images(4, 12).to(dev())
    _run(m, x, _joint)                                  # the engine's flat buffers exist and hold this run's gradients
    eng = m.backbone.model.engine
    flat = eng.grad_flat.clone()
    _freeze(m)
    _run(m, x, lambda out: out['cls_logits'][:, 0].sum())
    assert torch.equal(eng.grad_flat, flat)


# ---- 3. trainable backbone -------------------------------------------------------------------------------------------------------

def test_trainable_backbone_parameter_gradients_unchanged_by_image_grad():
    import rovit_hip.functions as fn
    m, _ = _model(2, seed=9)
    x = _images(5, 13).to(dev())
    calls = []
    orig = fn.call
    fn.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        out = m(x.clone())
        _joint(out).backward()
    finally:
        fn.call = orig
    plain = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    assert 'rovit_vit_backward' in calls and 'rovit_vit_backward_input' not in calls and 'rovit_patch_embed_dgrad' not in calls
    gx, grads = _run(m, x, _joint)
    assert gx is not None and grads.keys() == plain.keys()
    for n in plain:
        assert torch.equal(grads[n], plain[n]), n
    # two backwards accumulate into x.grad
    xg = x.clone().requires_grad_(True)
    _joint(m(xg)).backward()
    first = xg.grad.clone()
    _joint(m(xg)).backward()
    assert torch.equal(xg.grad, first * 2)
    m.zero_grad(set_to_none=True)


# ---- 4. the kernel against fp64 torch --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,copies,accumulate,scale', [(1, 1, 0, 1.0), (7, 4, 1, 0.37), (7, 1, 1, 1.0), (256, 1, 0, 1.0),
                                                       (256, 4, 1, 0.125), (1, 4, 0, -2.5)])
def test_patch_embed_dgrad_kernel(B, copies, accumulate, scale):
    from rovit_hip.native import call, ptr, stream_ptr
    g = torch.Generator(device=dev()).manual_seed(B * 10 + copies)
    dY = torch.randn(copies * B * 197, 192, device=dev(), generator=g).to(torch.bfloat16)
    W = (torch.randn(192, 768, device=dev(), generator=g) * 0.05).to(torch.bfloat16)
    img = 3 * 224 * 224
    buf = torch.full(((B + 2) * img,), float('nan'), device=dev())          # one sentinel image on each side
    old = torch.randn(B * img, device=dev(), generator=g)
    if accumulate:
        buf[img:(B + 1) * img] = old
    out = buf[img:(B + 1) * img]
    call('rovit_patch_embed_dgrad', ptr(dY), 192, ptr(W), ptr(out), B, copies, scale, accumulate, stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(buf[:img]).all() and torch.isnan(buf[(B + 1) * img:]).all()
    rows = dY.double().view(copies, B, 197, 192)[:, :, 1:].sum(0)                 # (B,196,192)
    p = (rows @ W.double()).view(B, 14, 14, 3, 16, 16).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 224, 224)
    want = scale * p + (old.double().view(B, 3, 224, 224) if accumulate else 0)
    got = out.view(B, 3, 224, 224).double()
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= KERNEL_RTOL, err
    # the same thing as the transposed convolution of the patch embedding
    if copies == 1 and not accumulate:
        ct = F.conv_transpose2d(rows.view(B, 14, 14, 192).permute(0, 3, 1, 2), W.double().view(192, 3, 16, 16), stride=16)
        assert float((got - scale * ct).abs().max() / ct.abs().max()) <= KERNEL_RTOL


# ---- 5. input types ----------------------------------------------------------------------------------------------------------------

def test_input_dtypes_and_layouts():
    m, _ = _model(2, seed=14)
    base = _images(3, 15).to(dev())
    loss = lambda out: out['kan_severity'].sum()
    gx, _ = _run(m, base, loss)
    gcl, _ = _run(m, base.contiguous(memory_format=torch.channels_last), loss)
    assert gcl.shape == base.shape and torch.equal(gcl, gx)
    t = base.transpose(2, 3).contiguous().transpose(2, 3)           # same values, non-contiguous
    assert not t.is_contiguous()
    gt, _ = _run(m, t, loss)
    assert gt.shape == base.shape and torch.equal(gt, gx)
    for dt in (torch.float16, torch.bfloat16):
        xd = base.to(dt)
        g, _ = _run(m, xd, loss)
        ref, _ = _run(m, xd.float(), loss)
        assert g.dtype == dt and g.shape == base.shape
        assert torch.equal(g, ref.to(dt))


# ---- 6. the reference's Grad-CAM++ recipe on a frozen backbone ---------------------------------------------------------------------

def _recipe(m, x, cls):
    cap = {}
    target = m.backbone.model.blocks[-1].norm1
    h1 = target.register_forward_hook(lambda mod, inp, outp: cap.__setitem__('act', outp.detach().clone()))
    h2 = target.register_full_backward_hook(lambda mod, gin, gout: cap.__setitem__('grad', gout[0].detach().clone()))
    try:
        image = x.clone()
        image.requires_grad = True                      # explainability/gradcam.py:37
        out = m(image)
        m.zero_grad()
        out['cls_logits'][:, cls].sum().backward()
    finally:
        h1.remove()
        h2.remove()
    m.zero_grad(set_to_none=True)
    return cap['act'], cap['grad'], image.grad


@pytest.mark.parametrize('depth', [2, 12])
def test_reference_gradcam_recipe_on_frozen_backbone(depth):
    m, _ = _model(depth, seed=16)
    x = _images(2, 17).to(dev())
    act_t, grad_t, gx_t = _recipe(m, x, 2)
    _freeze(m)
    act_f, grad_f, gx_f = _recipe(m, x, 2)
    assert torch.equal(act_f, act_t) and torch.equal(grad_f, grad_t) and torch.equal(gx_f, gx_t)
    assert all(p.grad is None for p in m.backbone.parameters())


# ---- 7. input_gradients with steps = 0 -------------------------------------------------------------------------------------------

def _target_value(out, name, cls):
    if name == 'class':
        return out['cls_logits'].gather(1, cls[:, None])[:, 0]
    if name == 'ordinal_severity':
        from models.heads import OrdinalHead
        p = OrdinalHead.probabilities_from_logits(out['ordinal_logits'])
        return (p * torch.arange(p.shape[1], dtype=torch.float32, device=p.device)).sum(dim=1, keepdim=True)[:, 0]
    return out[name][:, 0]


@pytest.mark.parametrize('name', ['class', 'ordinal_severity', 'mu', 'log_var', 'kan_severity'])
def test_input_gradients_equal_autograd_through_the_model(name):
    m, _ = _model(2, seed=18)
    x = _images(6, 19).to(dev())
    _freeze(m)
    xg = x.clone().requires_grad_(True)
    out = m(xg)
    cls = out['cls_logits'].detach().argmax(1)
    want, = torch.autograd.grad(_target_value(out, name, cls).sum(), xg)
    m.zero_grad(set_to_none=True)
    flags = [p.requires_grad for p in m.parameters()]
    m.classification_head.dropout.train()                     # eval semantics whatever the flags say
    got, val = m.input_gradients(x, target=name, return_values=True)
    assert m.classification_head.dropout.training
    m.classification_head.dropout.eval()
    assert got.dtype == torch.float32 and got.shape == x.shape
    assert torch.equal(got, want), float((got - want).abs().max())
    assert torch.equal(val, _target_value(out, name, cls).detach())
    assert [p.requires_grad for p in m.parameters()] == flags and all(p.grad is None for p in m.parameters())
    # chunked: the same images through calls of 4 and 2
    m.backbone.model.engine.mlp_path = 1
    try:
        a = m.input_gradients(x, target=name, chunk=4)
        b = m.input_gradients(x, target=name, chunk=6)
    finally:
        m.backbone.model.engine.mlp_path = None
    assert float((a - b).abs().max() / b.abs().max()) <= 1e-6


def test_input_gradients_between_training_forward_and_backward():
    m, _ = _model(2, seed=20)
    x = _images(4, 21).to(dev())
    gx0, g0 = _run(m, x, _joint)
    xg = x.clone().requires_grad_(True)
    out = m(xg)
    eng = m.backbone.model.engine
    last = eng.last_ws
    ig = m.input_gradients(x, target='mu', steps=3, chunk=5)
    assert eng.last_ws is last
    assert all(p.grad is None for p in m.parameters())
    _joint(out).backward()
    assert torch.equal(xg.grad, gx0)
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, g0[n]), n
    assert torch.isfinite(ig).all()
    m.zero_grad(set_to_none=True)


def test_input_gradients_refuses_before_any_launch():
    import rovit_hip.functions as fn
    import rovit_hip.input_grad as ig
    from rovit_hip import RovitHipError
    m, _ = _model(2, seed=22)
    x = _images(2, 23).to(dev())
    calls = []
    o1, o2 = fn.call, ig.call
    fn.call = ig.call = lambda name, *a: calls.append(name)
    try:
        for kw in ({'steps': -1}, {'chunk': 0}, {'steps': 2, 'baseline': torch.zeros(3, 3, 224, 224, device=dev())},
                   {'steps': 2, 'baseline': torch.zeros(2, 3, 224, 224)}, {'target': 'sev'}, {'class_idx': 7},
                   {'target': 'mu', 'class_idx': 0}):
            with pytest.raises(RovitHipError):
                m.input_gradients(x, **kw)
        m.curriculum_stage = 3
        with pytest.raises(RovitHipError, match='curriculum stage'):
            m.input_gradients(x, target='kan_severity')
        with pytest.raises(RovitHipError, match='GPU'):
            m.input_gradients(x.cpu())
    finally:
        fn.call, ig.call = o1, o2
    assert calls == []


# ---- 8. integrated gradients ----------------------------------------------------------------------------------------------------

def test_integrated_gradients_against_fp64_oracle(mlp_path):
    from rovit_hip.input_grad import ig_reference
    m, sd = _model(2, seed=24)
    sd64 = _sd64(sd)
    x = _images(2, 25)
    xb = 0.3 * _images(1, 26)
    steps = 8
    got, fx, fxb = m.input_gradients(x.to(dev()), target='mu', steps=steps, baseline=xb.to(dev()), return_values=True)
    # oracle: the same right rule in fp64; heads evaluated at the HIP features of each interpolant (no flips possible)
    feats_hip = {}

    def f(xi):
        with torch.no_grad():
            fh = m(xi.float().to(dev()))['features'].detach().cpu()
        feats = ref_cpu.vit_forward(xi, sd64, prefix='backbone.model.')
        g = _head_seed(sd64, fh, lambda out: out['mu'][:, 0])
        return (feats * g).sum(1)
    want = ig_reference(f, x.double(), xb.double().expand_as(x), steps)
    for b in range(2):
        c = _cos(got[b].cpu(), want[b])
        print(f'IG {mlp_path} image {b}: cosine {c:.6f}')
        assert c >= COS_MIN, (b, c)
    # chunks that stack 8, 2 and 1 interpolants per call agree
    res = [m.input_gradients(x.to(dev()), target='mu', steps=steps, baseline=xb.to(dev()), chunk=ch) for ch in (16, 2, 1)]
    for r in res[1:]:
        assert float((r - res[0]).abs().max() / res[0].abs().max()) <= 1e-6
    assert torch.equal(res[0], got)


def test_integrated_gradients_completeness():
    m, _ = _model(2, seed=27)
    x = _images(3, 28).to(dev())
    for name in ('class', 'mu', 'kan_severity'):
        attr, fx, fxb = m.input_gradients(x, target=name, steps=32, return_values=True)
        delta = fx - fxb
        gap = (attr.flatten(1).sum(1) - delta).abs() / delta.abs()
        print(f'IG completeness {name}: f(x) - f(x\') {delta.tolist()}, gap {gap.tolist()}')
        live = delta.abs() > 1e-3          # a relative gap of a vanishing difference says nothing
        if name != 'kan_severity':
            assert bool(live.any()) and float(gap[live].max()) <= COMPLETENESS_MAX
