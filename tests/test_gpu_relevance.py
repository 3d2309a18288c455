"""GPU tests of the gradient-weighted attention relevance (rovit_attention_relevance_step, rovit_vit_backward_relevance,
RoViTKAN.attention_relevance): the step kernel against fp64 torch on the same bf16 operands, with NaN in the rows the last block never
writes; the whole relevance vector against the fp64 oracle for the five targets; the map; determinism and chunking; a stale workspace;
side effects on a training step; class_idx."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref_cpu  # noqa: E402  (checker only)

KERNEL_RTOL = 1e-5        # the step kernel against fp64 torch on the same bf16 operands (the pixel kernel's bound)
COS_MIN = 0.99            # per-image cosine of the (B,197) relevance against the fp64 oracle (an expectation)
COS_FLIP = 0.9            # end to end: images whose classification-head ReLU unit flips between the bf16 and the fp64 features
TARGETS = ['class', 'ordinal_severity', 'mu', 'log_var', 'kan_severity']


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


def _sd64(sd):
    return {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}


# ---- 1. the step kernel against fp64 torch ---------------------------------------------------------------------------------------

def _lse2(qkv, B):
    q, k = qkv.double().view(B, 197, 3, 3, 64).permute(2, 0, 3, 1, 4)[:2]
    return (torch.logsumexp((q @ k.transpose(-1, -2)) * 0.125, -1) / torch.log(torch.tensor(2.0, dtype=torch.float64))).float()


def _step_reference(qkv, lse2, dout, u, first):
    """u + u A in fp64 on the kernel's bf16 operands and fp32 lse2; first: u = e_0."""
    B = u.shape[0]
    q, k, v = qkv.double().view(B, 197, 3, 3, 64).permute(2, 0, 3, 1, 4)
    g = dout.double().view(B, 197, 3, 64).permute(0, 2, 1, 3)
    P = torch.exp2((q @ k.transpose(-1, -2)) * (0.125 / torch.log(torch.tensor(2.0, dtype=torch.float64))) - lse2.double()[..., None])
    A = (P * (g @ v.transpose(-1, -2))).clamp(min=0).mean(1)
    u0 = torch.zeros_like(u, dtype=torch.float64)
    if first:
        u0[:, 0] = 1
    else:
        u0 = u.double()
    return u0 + (u0.unsqueeze(1) @ A).squeeze(1)


@pytest.mark.parametrize('B', [1, 3, 64])
@pytest.mark.parametrize('first', [0, 1])
def test_step_kernel_against_fp64(B, first):
    from rovit_hip.native import call, ptr, stream_ptr
    g = torch.Generator(device=dev()).manual_seed(10 * B + first)
    qkv = torch.randn(B * 197, 576, device=dev(), generator=g).to(torch.bfloat16)
    dout = torch.randn(B * 197, 192, device=dev(), generator=g).to(torch.bfloat16)
    lse2 = _lse2(qkv, B).contiguous()
    u = torch.rand(B, 197, device=dev(), generator=g)
    want = _step_reference(qkv, lse2, dout, u, first)
    scratch = torch.empty(B * 3 * 197, device=dev())
    got = u.clone()
    call('rovit_attention_relevance_step', ptr(qkv), ptr(lse2), ptr(dout), ptr(got), ptr(scratch), B, first, stream_ptr())
    torch.cuda.synchronize()
    err = float((got.double() - want).abs().max() / want.abs().max())
    print(f'B {B} first {first}: max-abs / max {err:.3e}')
    assert err <= KERNEL_RTOL, err
    again = u.clone()
    call('rovit_attention_relevance_step', ptr(qkv), ptr(lse2), ptr(dout), ptr(again), ptr(scratch), B, first, stream_ptr())
    assert torch.equal(again, got)                                         # bit-identical run to run
    if first:
        # the last block: dO and lse2 hold stale bytes beyond the class-token rows, and u is not read
        dn, ln = dout.clone(), lse2.clone()
        dn.view(B, 197, 192)[:, 1:] = float('nan')
        ln[:, :, 1:] = float('nan')
        stale = torch.full_like(u, float('nan'))
        call('rovit_attention_relevance_step', ptr(qkv), ptr(ln), ptr(dn), ptr(stale), ptr(scratch), B, 1, stream_ptr())
        torch.cuda.synchronize()
        assert torch.isfinite(stale).all() and torch.equal(stale, got)


# ---- 2. the whole vector against the fp64 oracle ---------------------------------------------------------------------------------

def _value_fns(cls):
    def ordinal(out):
        from models.heads import OrdinalHead
        p = OrdinalHead.probabilities_from_logits(out['ordinal_logits'])
        return (p * torch.arange(p.shape[1], dtype=p.dtype)).sum(1)
    return {'class': lambda out: out['cls_logits'].gather(1, cls[:, None])[:, 0], 'ordinal_severity': ordinal,
            'mu': lambda out: out['mu'][:, 0], 'log_var': lambda out: out['log_var'][:, 0],
            'kan_severity': lambda out: out['kan_severity'][:, 0]}


def _head_seed(sd64, f, value_fn):
    f = f.double().detach().requires_grad_(True)
    out = ref_cpu.heads_forward(f, sd64, 4)
    out['kan_severity'] = ref_cpu.kan_module_forward(f, sd64, 'kan_module.')
    g, = torch.autograd.grad(value_fn(out).sum(), f)
    return g


@pytest.mark.parametrize('depth,B', [(1, 3), (2, 8), (12, 4)])
def test_relevance_against_fp64_oracle(depth, B):
    """Each target's seed d target / d features is the oracle's heads at the HIP features (no head flip possible), so the comparison is
    the backbone's relevance alone; the class logit is also compared end to end, images with a flipped head ReLU unit held to COS_FLIP."""
    from rovit_hip.relevance import relevance_reference, relevance_vectors
    m, sd = _model(depth, seed=30 + depth)
    sd64 = _sd64(sd)
    x = _images(B, 31 + depth)
    cls = torch.arange(B) % 4
    with torch.no_grad():
        f_hip = m(x.to(dev()))['features'].cpu()
    xd = x.double().requires_grad_(True)
    probs = []
    feats = ref_cpu.vit_forward(xd, sd64, prefix='backbone.model.', attn_probs=probs)
    fns = _value_fns(cls)
    worst = {}
    for name in TARGETS:
        got, val = relevance_vectors(m, x.to(dev()), name, cls.to(dev()) if name == 'class' else None)
        raw = m.attention_relevance(x.to(dev()), target=name, class_idx=cls.to(dev()) if name == 'class' else None, upsample=False)
        assert raw.shape == (B, 14, 14) and torch.equal(raw, got[:, 1:].reshape(B, 14, 14))
        seed = _head_seed(sd64, f_hip, fns[name])
        want = relevance_reference(probs, (feats * seed).sum(1))
        cs = [_cos(got[b].cpu(), want[b]) for b in range(B)]
        cm = [_cos(got[b, 1:].cpu(), want[b, 1:]) for b in range(B)]
        worst[name] = (min(cs), min(cm))
        print(f'depth {depth} B {B} {name}: cosine >= {min(cs):.6f} (tokens 1.. alone: >= {min(cm):.6f})')
        assert torch.isfinite(got).all() and bool((got >= 0).all())
        assert min(cs) >= COS_MIN, (name, cs)
    # end to end for the class logit: the oracle's own features and head
    seed = _head_seed(sd64, feats.detach(), fns['class'])
    want = relevance_reference(probs, (feats * seed).sum(1))
    got, _ = relevance_vectors(m, x.to(dev()), 'class', cls.to(dev()))
    w1, b1 = sd64['classification_head.fc1.weight'], sd64['classification_head.fc1.bias']
    flipped = ((f_hip.double() @ w1.t() + b1 > 0) != (feats.detach() @ w1.t() + b1 > 0)).any(1)
    for b in range(B):
        c = _cos(got[b].cpu(), want[b])
        print(f'  end to end image {b}: cosine {c:.6f}{" (flipped head unit)" if flipped[b] else ""}')
        assert c >= (COS_FLIP if flipped[b] else COS_MIN), (b, c)


# ---- 3. the map -----------------------------------------------------------------------------------------------------------------

def test_upsampled_map_is_the_rollout_map_of_the_raw_vector():
    from rovit_hip.native import call, ptr, stream_ptr
    from rovit_hip.relevance import relevance_vectors
    m, _ = _model(2, seed=40)
    x = _images(5, 41).to(dev())
    rel, _ = relevance_vectors(m, x, 'mu')
    want = torch.empty(5, 224, 224, device=dev())
    call('rovit_rollout_map', ptr(rel), ptr(want), 5, stream_ptr())
    got = m.attention_relevance(x, target='mu')
    assert got.shape == (5, 224, 224) and got.dtype == torch.float32
    assert torch.equal(got, want)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0


# ---- 4. determinism and chunking --------------------------------------------------------------------------------------------------

def test_determinism_and_chunks():
    m, _ = _model(2, seed=42)
    x = _images(300, 43).to(dev())
    a = m.attention_relevance(x, target='kan_severity', chunk=128, upsample=False)
    b = m.attention_relevance(x, target='kan_severity', chunk=128, upsample=False)
    assert torch.equal(a, b)
    parts = [m.attention_relevance(x[s:e], target='kan_severity', upsample=False) for s, e in ((0, 128), (128, 256), (256, 300))]
    assert torch.equal(torch.cat(parts), a)


# ---- 5. a stale workspace ---------------------------------------------------------------------------------------------------------

def test_stale_workspace_from_a_nan_call():
    """The pool hands the NaN call's workspace to the next call of the same batch size: the last block's dO and lse2 rows beyond the class
    token still hold its NaN, and must not reach the result."""
    m, _ = _model(2, seed=44)
    x = _images(6, 45).to(dev())
    clean = m.attention_relevance(x, class_idx=1, upsample=False)
    eng = m.backbone.model.engine
    pool = eng._ws_pool[(6, True, str(dev()))]
    ws = pool[-1]
    bad = x.clone()
    bad[2, :, 50:90, 30:200] = float('nan')
    poisoned = m.attention_relevance(bad, class_idx=1, upsample=False)
    assert not torch.isfinite(poisoned).all()
    assert pool[-1] is ws                                        # the same buffer went out and came back
    again = m.attention_relevance(x, class_idx=1, upsample=False)
    assert pool[-1] is ws
    assert torch.isfinite(again).all() and torch.equal(again, clean)


# ---- 6. side effects -------------------------------------------------------------------------------------------------------------

def _joint(out):
    B = out['cls_logits'].shape[0]
    y = torch.arange(B, device=out['cls_logits'].device) % 4
    return ref_cpu.joint_loss(out, y, (y + 1) % 4, stage=4)['total_loss']


def test_no_gradients_or_flags_touched():
    m, _ = _model(2, seed=46)
    x = _images(3, 47).to(dev())
    for p in m.backbone.parameters():
        p.requires_grad_(False)
    flags = [p.requires_grad for p in m.parameters()]
    m.classification_head.dropout.train()                      # eval semantics whatever the flags say
    got = m.attention_relevance(x, target='ordinal_severity', upsample=False)
    assert m.classification_head.dropout.training
    m.classification_head.dropout.eval()
    assert torch.equal(got, m.attention_relevance(x, target='ordinal_severity', upsample=False))
    assert [p.requires_grad for p in m.parameters()] == flags and all(p.grad is None for p in m.parameters())
    assert not m.training


def test_between_training_forward_and_backward():
    m, _ = _model(2, seed=48)
    x = _images(4, 49).to(dev())
    _joint(m(x.clone())).backward()
    g0 = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    out = m(x.clone())
    eng = m.backbone.model.engine
    last = eng.last_ws
    rel = m.attention_relevance(x, target='log_var', chunk=3)
    assert eng.last_ws is last
    assert all(p.grad is None for p in m.parameters())
    _joint(out).backward()
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, g0[n]), n
    assert torch.isfinite(rel).all()
    m.zero_grad(set_to_none=True)


# ---- 7. class_idx ----------------------------------------------------------------------------------------------------------------

def test_class_idx_forms():
    m, _ = _model(2, seed=50)
    x = _images(5, 51).to(dev())
    with torch.no_grad():
        am = m(x)['cls_logits'].argmax(1)
    explicit = lambda c: m.attention_relevance(x, class_idx=torch.as_tensor(c, device=dev()), upsample=False)
    assert torch.equal(m.attention_relevance(x, upsample=False), explicit(am))
    assert torch.equal(m.attention_relevance(x, class_idx=2, upsample=False), explicit([2] * 5))
    r0, v0 = m.attention_relevance(x, class_idx=0, upsample=False, return_values=True)
    r3, v3 = m.attention_relevance(x, class_idx=torch.full((5,), 3, dtype=torch.int32, device=dev()), upsample=False,
                                   return_values=True)
    with torch.no_grad():
        logits = m(x)['cls_logits']
    assert torch.allclose(v0, logits[:, 0], rtol=1e-4, atol=1e-4) and torch.allclose(v3, logits[:, 3], rtol=1e-4, atol=1e-4)
    assert not torch.equal(r0, r3)
