"""GPU tests of the deletion / insertion curves (rovit_vit_embed, rovit_vit_forward_tokens, RoViTKAN.perturbation_curves): identity
rows and 'replace' sequences bit-identical to rovit_vit_forward on the pixel images; 'drop' sequences at ragged token counts against an
fp64 forward of the kept tokens; the curves against the pixel recipe through the fp64 oracle and, bit for bit, through the engine's own
forward; independence of the batch, the maps and the step count; shared endpoints; clamped indices; side effects on a training step."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref_cpu  # noqa: E402  (checker only)

FEAT_TOL, FEAT_RMS = 5e-2, 1.2e-2     # the engine's stated feature tolerance against fp64
PROB_TOL = 1.5e-2                     # softmax probability: |dp| <= max|dlogit| / 2 of smoke()'s 3e-2 logit bound
E2E_TOL = 3e-2                        # ordinal_severity, mu, log_var: the end-to-end bound of tests/test_gpu_model.py
KAN_TOL = 1e-3                        # KAN on identical features (the spline is discontinuous)
TARGETS = ['class', 'ordinal_severity', 'mu', 'log_var', 'kan_severity']


def dev():
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
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


def _bb(m):
    from rovit_hip.input_grad import _Backbone
    return _Backbone(m, dev())


def _vit_forward(bb, imgs, mlp):
    from rovit_hip.native import call, ptr, stream_ptr
    n = imgs.shape[0]
    ws = bb.eng.take_ws(n, False, dev())
    f = torch.empty(n, 192, device=dev())
    call('rovit_vit_forward', ptr(imgs), bb.pa, ptr(bb.eng.prep), ptr(ws), ptr(f), n, bb.vit.depth, 0, mlp, stream_ptr())
    bb.eng.give_ws(n, False, ws)
    return f


def _tables(bb, imgs):
    t = torch.empty(imgs.shape[0], 197, 192, device=dev())
    bb.embed(imgs, t)
    return t


def _tokens(bb, img_t, base_t, shared, seq_img, src, mlp):
    ws = bb.eng.take_ws(src.shape[0], False, dev())
    f = bb.forward_tokens(img_t, base_t, shared, seq_img.int().to(dev()), src.int().to(dev()), ws, mlp)
    bb.eng.give_ws(src.shape[0], False, ws)
    return f


def _up(mask):
    """(n,196) patch mask -> (n,3,224,224) pixel mask."""
    n = mask.shape[0]
    return mask.view(n, 1, 14, 1, 14, 1).expand(n, 3, 14, 16, 14, 16).reshape(n, 3, 224, 224)


# ---- 1. identity rows ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mlp', [1, 2])
@pytest.mark.parametrize('depth', [2, 12])
@pytest.mark.parametrize('n', [1, 5, 37, 256])
def test_identity_rows_equal_the_forward(n, depth, mlp):
    m, sd = _model(depth, seed=depth)
    bb = _bb(m)
    x = _images(n, n).to(dev())
    t = _tables(bb, x)
    if n == 5:       # the token rows themselves: the fp32 embedding against fp64 (bf16 patch GEMM, fp32 bias and position)
        sd64 = {k[len('backbone.model.'):]: v.double() for k, v in sd.items() if k.startswith('backbone.model.')}
        e = F.conv2d(x.cpu().double(), sd64['patch_embed.proj.weight'], sd64['patch_embed.proj.bias'], stride=16).flatten(2).transpose(1, 2)
        e = torch.cat([sd64['cls_token'].expand(n, -1, -1), e], 1) + sd64['pos_embed']
        assert float((t.cpu().double() - e).abs().max()) < FEAT_TOL
        assert torch.equal(t[:, 0].cpu(), (sd['backbone.model.cls_token'][0] + sd['backbone.model.pos_embed'][:, 0]).expand(n, 192))
    src = torch.arange(197).repeat(n, 1)
    got = _tokens(bb, t, t, 0, torch.arange(n), src, mlp)
    want = _vit_forward(bb, x, mlp)
    assert torch.equal(got, want)


# ---- 2. 'replace' sequences against the pixel images -------------------------------------------------------------------------------

@pytest.mark.parametrize('mlp', [1, 2])
@pytest.mark.parametrize('shared', [0, 1])
def test_replace_rows_equal_the_forward_of_the_pixel_images(shared, mlp):
    from rovit_hip.perturbation import source_rows
    m, _ = _model(2, seed=3)
    bb = _bb(m)
    g = torch.Generator().manual_seed(5 + shared)
    n_img, n_seq = 5, 37
    x = _images(n_img, 7).to(dev())
    base = (torch.randn(1 if shared else n_img, 3, 224, 224, generator=g) * 0.5).to(dev())
    seq_img = torch.randint(0, n_img, (n_seq,), generator=g)
    keep_p = torch.rand(n_seq, 1, generator=g)
    mask = torch.rand(n_seq, 196, generator=g) < keep_p                  # perturbed patches, densities from 0 to 1
    mask[0] = False
    mask[1] = True
    src = source_rows(mask, 'replace')
    got = _tokens(bb, _tables(bb, x), _tables(bb, base), shared, seq_img, src, mlp)
    sidx = seq_img.to(dev())
    imgs = torch.where(_up(mask).to(dev()), base[torch.zeros_like(sidx) if shared else sidx], x[sidx])
    assert torch.equal(got, _vit_forward(bb, imgs.contiguous(), mlp))


def test_indices_are_clamped_into_the_tables():
    """Out-of-range descriptors read the nearest valid entry of their table (never outside it): image index into [0, n_img), row into
    [0, 197) of the image or the baseline."""
    m, _ = _model(2, seed=3)
    bb = _bb(m)
    x = _images(3, 8).to(dev())
    base = (_images(3, 9) * 0.3).to(dev())
    ti, tb = _tables(bb, x), _tables(bb, base)
    bad = torch.arange(197).repeat(4, 1)
    bad[0, 5], bad[1, 7], bad[2, 9] = 100000, -100000, -(2 ** 31)
    bad[3, 196] = 2 ** 31 - 1
    good = bad.clone()
    good[0, 5], good[1, 7], good[2, 9], good[3, 196] = 196, -197, -197, 196
    got = _tokens(bb, ti, tb, 0, torch.tensor([-4, 1, 99, 2]), bad, 2)
    want = _tokens(bb, ti, tb, 0, torch.tensor([0, 1, 2, 2]), good, 2)
    assert torch.equal(got, want)


# ---- 3. 'drop' sequences against an fp64 forward of the kept tokens ----------------------------------------------------------------

def _vit64_kept(x, sd, kept):
    """fp64 statement of the backbone on a subset of tokens: embed (conv 16/16, class token, position embedding), keep the rows
    `kept` (n, tokens) of each image's 197, then the pre-norm blocks and the final norm on those rows; token 0 is the feature."""
    p = 'backbone.model.'
    B = x.shape[0]
    t = F.conv2d(x, sd[p + 'patch_embed.proj.weight'], sd[p + 'patch_embed.proj.bias'], stride=16).flatten(2).transpose(1, 2)
    t = torch.cat([sd[p + 'cls_token'].expand(B, -1, -1), t], dim=1) + sd[p + 'pos_embed']
    t = torch.gather(t, 1, kept.view(B, -1, 1).expand(B, kept.shape[1], 192))
    i = 0
    while f'{p}blocks.{i}.norm1.weight' in sd:
        b = f'{p}blocks.{i}.'
        h = F.layer_norm(t, (192,), sd[b + 'norm1.weight'], sd[b + 'norm1.bias'], 1e-6)
        q, k, v = F.linear(h, sd[b + 'attn.qkv.weight'], sd[b + 'attn.qkv.bias']).reshape(B, -1, 3, 3, 64).permute(2, 0, 3, 1, 4)
        a = torch.softmax((q * 0.125) @ k.transpose(-2, -1), dim=-1)
        t = t + F.linear((a @ v).transpose(1, 2).reshape(B, -1, 192), sd[b + 'attn.proj.weight'], sd[b + 'attn.proj.bias'])
        h = F.layer_norm(t, (192,), sd[b + 'norm2.weight'], sd[b + 'norm2.bias'], 1e-6)
        t = t + F.linear(F.gelu(F.linear(h, sd[b + 'mlp.fc1.weight'], sd[b + 'mlp.fc1.bias'])), sd[b + 'mlp.fc2.weight'], sd[b + 'mlp.fc2.bias'])
        i += 1
    return F.layer_norm(t, (192,), sd[p + 'norm.weight'], sd[p + 'norm.bias'], 1e-6)[:, 0]


@pytest.mark.parametrize('depth', [2, 12])
@pytest.mark.parametrize('tokens', [1, 2, 17, 98, 150, 196])
def test_drop_against_fp64_forward_of_the_kept_tokens(tokens, depth):
    from rovit_hip.perturbation import source_rows
    m, sd = _model(depth, seed=20 + depth)
    sd64 = {k: v.double() for k, v in sd.items()}
    bb = _bb(m)
    g = torch.Generator().manual_seed(tokens)
    n_img, n_seq = 3, 19                        # >= 16 sequences: two half-batch chains of 10 and 9
    x = _images(n_img, 30 + tokens)
    # the fp64 statement itself: every token kept is oracle.ref_cpu.vit_forward
    full = torch.arange(197).repeat(n_img, 1)
    torch.testing.assert_close(_vit64_kept(x.double(), sd64, full), ref_cpu.vit_forward(x.double(), sd64, 'backbone.model.'),
                               rtol=1e-12, atol=1e-12)
    seq_img = torch.randint(0, n_img, (n_seq,), generator=g)
    mask = torch.stack([torch.randperm(196, generator=g) >= tokens - 1 for _ in range(n_seq)])       # tokens - 1 patches kept
    src = source_rows(mask, 'drop', tokens)
    assert tuple(src.shape) == (n_seq, tokens)
    mlp = 2 if depth == 12 else 1
    got = _tokens(bb, _tables(bb, x.to(dev())), _tables(bb, x.to(dev())), 0, seq_img, src, mlp).cpu().double()
    want = _vit64_kept(x.double()[seq_img], sd64, src.long())
    err = (got - want).abs()
    rms = float(err.pow(2).mean().sqrt())
    print(f'drop tokens {tokens} depth {depth}: max-abs {float(err.max()):.2e} rms {rms:.2e}')
    assert float(err.max()) < FEAT_TOL and rms < FEAT_RMS


# ---- 4. the curves against the pixel recipe through the fp64 oracle ----------------------------------------------------------------

def test_curves_against_the_fp64_pixel_recipe():
    from rovit_hip.native import MLP_ONE_LAUNCH
    from rovit_hip.perturbation import perturbation_reference
    from models.heads import OrdinalHead
    m, sd = _model(2, seed=40)
    sd64 = {k: v.double() for k, v in sd.items()}
    bb = _bb(m)
    B, steps = 4, 7
    x = _images(B, 41)
    sal = torch.randn(B, 14, 14, generator=torch.Generator().manual_seed(42))
    zero = torch.zeros(1, 3, 224, 224, dtype=torch.float64)
    res = {t: m.perturbation_curves(x.to(dev()), sal, target=t, steps=steps) for t in TARGETS}
    cls = res['class']['class_idx'].cpu()

    def f64(imgs):
        o = ref_cpu.rovit_forward(imgs, sd64, 4)
        lv = torch.arange(4, dtype=torch.float64)
        return torch.stack([torch.softmax(o['cls_logits'], 1).gather(1, cls.view(-1, 1))[:, 0],
                            (OrdinalHead.probabilities_from_logits(o['ordinal_logits']) * lv).sum(1), o['mu'][:, 0], o['log_var'][:, 0]], 1)

    def kan_same_features(imgs):         # the oracle KAN on the engine's own features (one-launch MLP as the curves' chunk of 256)
        feats = _vit_forward(bb, imgs.float().contiguous().to(dev()), MLP_ONE_LAUNCH)
        return ref_cpu.kan_module_forward(feats.cpu(), sd, 'kan_module.')[:, 0]

    for mode in ('deletion', 'insertion'):
        ref = perturbation_reference(f64, x.double(), sal, mode, steps, zero)
        for j, (t, tol) in enumerate([('class', PROB_TOL), ('ordinal_severity', E2E_TOL), ('mu', E2E_TOL), ('log_var', E2E_TOL)]):
            err = float((res[t][mode].cpu().double() - ref[..., j]).abs().max())
            print(f'{mode} {t}: max-abs {err:.2e}')
            assert err < tol, (mode, t, err)
        kan = perturbation_reference(kan_same_features, x, sal, mode, steps, zero.float())
        assert float((res['kan_severity'][mode].cpu() - kan).abs().max()) < KAN_TOL
        for t in TARGETS:
            r = res[t]
            assert r[mode].dtype == torch.float32 and r[mode].device == x.to(dev()).device and tuple(r[mode].shape) == (B, steps + 1)
            torch.testing.assert_close(r[mode + '_auc'], torch.trapezoid(r[mode], r['fractions'], dim=1), rtol=0, atol=0)
    assert torch.equal(res['class']['fractions'].cpu(), torch.tensor([k / 196 for k in (0, 28, 56, 84, 112, 140, 168, 196)]))
    assert 'class_idx' not in res['mu']


# ---- 5. bit for bit against the pixel recipe on the engine's own forward -----------------------------------------------------------

@pytest.mark.parametrize('target', ['class', 'mu'])
def test_curves_equal_the_pixel_recipe_on_the_engine_bit_for_bit(target):
    from rovit_hip.input_grad import _head_outputs, _target_value
    from rovit_hip.native import MLP_ONE_LAUNCH
    from rovit_hip.perturbation import perturbation_reference
    m, _ = _model(2, seed=50)
    bb = _bb(m)
    B, steps = 5, 7
    x = _images(B, 51).to(dev())
    base = (_images(B, 52) * 0.5).to(dev())
    sal = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(53)).abs()
    r = m.perturbation_curves(x, sal, target=target, steps=steps, baseline=base)
    cls = r.get('class_idx')

    def f(imgs):                         # chunk 256 x 197 rows: the one-launch MLP half, as the curves resolve it
        outs = _head_outputs(m, _vit_forward(bb, imgs.contiguous(), MLP_ONE_LAUNCH))
        if target == 'class':
            return torch.softmax(outs[0], dim=1).gather(1, cls.view(-1, 1))[:, 0]
        return _target_value(target, outs, None)

    with torch.no_grad():
        for mode in ('deletion', 'insertion'):
            assert torch.equal(r[mode], perturbation_reference(f, x, sal.to(dev()), mode, steps, base))


# ---- 6 / 7. independence and shared endpoints ------------------------------------------------------------------------------------

@pytest.mark.parametrize('perturbation', ['replace', 'drop'])
def test_independence_and_endpoints(perturbation):
    m, _ = _model(2, seed=60)
    g = torch.Generator().manual_seed(61)
    B = 37
    x = _images(B, 62).to(dev())
    maps = {'a': torch.randn(B, 196, generator=g), 'b': torch.randn(B, 14, 14, generator=g),
            'c': torch.randn(B, 224, 224, generator=g)}
    kw = dict(target='class', perturbation=perturbation, chunk=64)
    many = m.perturbation_curves(x, maps, **kw)
    for i in (0, 17, 36):
        alone = m.perturbation_curves(x[i:i + 1], maps['b'][i:i + 1], **kw)
        batch = m.perturbation_curves(x, maps['b'], **kw)
        for mode in ('deletion', 'insertion'):
            assert torch.equal(alone[mode][0], batch[mode][i])
            assert torch.equal(alone[mode][0], many['b'][mode][i])
            assert torch.equal(alone[mode + '_auc'][0], many['b'][mode + '_auc'][i])
        assert int(alone['class_idx'][0]) == int(many['b']['class_idx'][i])
    # every map's curves start and end on the same two values
    d0, dN = many['a']['deletion'][:, 0], many['a']['deletion'][:, -1]
    for r in many.values():
        assert torch.equal(r['deletion'][:, 0], r['insertion'][:, -1]) and torch.equal(r['deletion'][:, -1], r['insertion'][:, 0])
        assert torch.equal(r['deletion'][:, 0], d0) and torch.equal(r['deletion'][:, -1], dN)
    assert bool((d0 > 0).all())
    # steps = 28 points are the steps = 196 points at k = 7 s
    few = m.perturbation_curves(x[:3], maps['a'][:3], steps=28, **kw)
    all_ = m.perturbation_curves(x[:3], maps['a'][:3], steps=196, **kw)
    for mode in ('deletion', 'insertion'):
        assert torch.equal(few[mode], all_[mode][:, ::7])
        assert torch.equal(few[mode], many['a'][mode][:3])


# ---- 8. side effects -------------------------------------------------------------------------------------------------------------

def _joint(out):
    B = out['cls_logits'].shape[0]
    y = torch.arange(B, device=out['cls_logits'].device) % 4
    return ref_cpu.joint_loss(out, y, (y + 1) % 4, stage=4)['total_loss']


def test_between_training_forward_and_backward():
    from models.rovit_kan import RoViTKAN
    from models.backbone import DeiTTiny
    sd = ref_cpu.init_rovit_state(depth=2, seed=70)
    m = RoViTKAN(pretrained=False)
    m.backbone.model = DeiTTiny(depth=2)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev()).eval()
    x = _images(4, 71).to(dev())
    sal = torch.rand(4, 196, generator=torch.Generator().manual_seed(72))
    _joint(m(x.clone())).backward()
    g0 = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    out = m(x.clone())
    eng = m.backbone.model.engine
    last = eng.last_ws
    flags = [p.requires_grad for p in m.parameters()]
    r = m.perturbation_curves(x, {'s': sal, 't': -sal}, target='mu', steps=5, chunk=7)
    r2 = m.perturbation_curves(x, sal, perturbation='drop', steps=5)
    assert eng.last_ws is last and not m.training
    assert all(p.grad is None for p in m.parameters()) and [p.requires_grad for p in m.parameters()] == flags
    _joint(out).backward()
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, g0[n]), n
    assert torch.isfinite(r['s']['deletion']).all() and torch.isfinite(r2['insertion']).all()
    m.zero_grad(set_to_none=True)
