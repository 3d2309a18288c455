"""GPU tests of the Python layer that hands the fused kernels' gradients to autograd and the optimizer (rovit_hip/functions.py
HeadPhaseFn.backward, rovit_hip/optim.py RoViTAdamW.step), in the cases the kernel parity tests do not reach:
  * gradient accumulation into an existing .grad, zero-filled .grad tensors and gradient hooks on head / KAN parameters, with the
    head phase's side stream held back by a spin kernel so that a missing stream join shows up every time, not by chance;
  * two forwards of one model in one backward pass (two HeadPhaseFn nodes sharing the parameters);
  * gradient clipping over more than four disjoint gradient runs (the optimizer's many-segment branch).
References: the CPU oracle (oracle/ref_cpu.py) in fp64 with torch autograd on the same weights, inputs and targets, and for the
optimizer torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW in fp64 on copies of the GPU's own gradients.
Tolerances: head / KAN gradients 1e-4 relative, 5e-4 at the C5 KAN (num_knots 32); backbone gradients the bf16
tolerance of tests/test_gpu_model.py (cosine > 0.999, max error < 6e-2 of the largest entry).  GPU against itself: torch.equal.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu  # noqa: E402  (checker only)

# cycles of the spin kernel queued on the parameter-gradient stream: milliseconds whatever the counter's rate, far longer than the
# backward's own launches, so a consumer that does not wait for that stream reads the gradients before they are written
SPIN_CYCLES = 20_000_000
C5_TOL = 5e-4
HEAD_TOL = 1e-4


def dev():
    return torch.device('cuda:0')


def _model(num_knots=5, seed=0, sd=None):
    from models.rovit_kan import RoViTKAN
    from rovit_hip.optim import RoViTAdamW
    torch.manual_seed(seed)
    m = RoViTKAN(pretrained=False, dropout=0.0, kan_num_knots=num_knots)
    if sd is not None:
        m.load_state_dict(sd)
    m = m.to(dev()).train()
    opt = RoViTAdamW(m, lr=1e-3)            # sets model._head_grad_views: the fused phase may write into the optimizer's buffer
    assert m._head_grad_views
    return m, opt


def _head_named(m):
    named = [(n, p) for n, p in m.named_parameters() if not n.startswith('backbone.')]
    assert len(named) == 23
    return named


def _loss_fn():
    from rovit_hip.losses import JointLoss
    return JointLoss(1.0, 0.5, 0.5, 2.0)


def _phase_loss(m, f, y, stage=4):
    """The head phase on given features (what RoViTKAN.forward runs after the backbone) and the HIP joint loss."""
    fd = f.to(dev()).requires_grad_(True)
    assert m._head_phase_fusable(fd)
    yd = y.to(dev())
    return _loss_fn()(m._forward_head_phase(fd, stage), yd, yd, stage)['total_loss']


def _oracle_out(f, sd, stage=4):
    out = ref_cpu.heads_forward(f, sd, stage)
    out['kan_severity'] = ref_cpu.kan_module_forward(f, sd, 'kan_module.') if stage >= 4 else None
    return out


def _oracle_head_grads(m, feats, ys, stage=4):
    """fp64 gradients of sum_i joint_loss(heads + KAN (feats[i]), ys[i]) w.r.t. every head / KAN parameter of m (current values)."""
    names = [n for n, _ in _head_named(m)]
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items() if not k.startswith('backbone.')}
    for n in names:
        sd[n].requires_grad_(True)
    total = sum(ref_cpu.joint_loss(_oracle_out(f.detach().cpu().double(), sd, stage), y.cpu(), y.cpu(), stage)['total_loss']
                for f, y in zip(feats, ys))
    total.backward()
    return {n: sd[n].grad for n in names}


def _rel(got, ref):
    got = got.detach().cpu().double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _check_heads(got, ref, tol, what):
    worst = 0.0
    for n, r in ref.items():
        assert got[n] is not None, (what, n)
        e = _rel(got[n], r)
        worst = max(worst, e)
        assert e <= tol, (what, n, e)
    print(f'{what}: worst head / KAN gradient error {worst:.3g} relative (tolerance {tol:g})')
    return worst


def _hold_side_stream():
    """Queue a spin kernel on the head phase's parameter-gradient stream: whatever that stream runs next starts milliseconds late."""
    from rovit_hip.functions import HeadPhaseFn
    with torch.cuda.stream(HeadPhaseFn.param_grad_stream(dev())):
        torch.cuda._sleep(SPIN_CYCLES)


def _inline_only(monkeypatch):
    """Every HeadPhaseFn launches its parameter gradients inline on the backward's stream."""
    from rovit_hip.functions import HeadPhaseFn
    real = HeadPhaseFn.apply
    monkeypatch.setattr(HeadPhaseFn, 'apply', staticmethod(lambda f, cfg, *ps: real(f, dict(cfg, dw_side_stream=False), *ps)))


def _inputs(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(B, 192, generator=g) for _ in range(n)]
    ys = [torch.randint(0, 4, (B,), generator=g) for _ in range(n)]
    return feats, ys


def test_accumulated_head_phase_gradients_at_batch_1024_c5_kan(monkeypatch):
    """Two backwards into the same .grad at head_phase_max_batch with the C5 KAN: the second one adds into gradients that already
    exist, so AccumulateGrad reads its result at once; the side stream is held back when it runs."""
    from models.rovit_kan import RoViTKAN
    B = RoViTKAN.head_phase_max_batch
    m, _ = _model(num_knots=32, seed=1)
    named = _head_named(m)
    feats, ys = _inputs(B, 2, seed=2)
    ref = _oracle_head_grads(m, feats, ys)

    def run():
        for p in m.parameters():
            p.grad = None
        _phase_loss(m, feats[0], ys[0]).backward()
        _hold_side_stream()
        _phase_loss(m, feats[1], ys[1]).backward()
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in named}

    got = run()
    _check_heads(got, ref, C5_TOL, 'accumulation, B=1024, C5 KAN')
    _inline_only(monkeypatch)
    inline = run()
    for n, _ in named:
        assert torch.equal(got[n], inline[n]), n


def test_zero_filled_grads_receive_the_gradient():
    """optimizer.zero_grad(set_to_none=False): the .grad tensors exist (zero-filled views of the optimizer's buffer) and the next
    backward adds into them."""
    m, opt = _model(num_knots=32, seed=3)
    named = _head_named(m)
    feats, ys = _inputs(1024, 2, seed=4)
    _phase_loss(m, feats[0], ys[0]).backward()
    opt.step()
    opt.zero_grad(set_to_none=False)
    assert all(p.grad is not None and not bool(p.grad.any()) for _, p in named)
    ref = _oracle_head_grads(m, feats[1:], ys[1:])          # at the parameters after the step
    _hold_side_stream()
    _phase_loss(m, feats[1], ys[1]).backward()
    torch.cuda.synchronize()
    _check_heads({n: p.grad for n, p in named}, ref, C5_TOL, 'zero_grad(set_to_none=False)')


def test_gradient_hooks_on_head_and_kan_parameters_see_the_gradient():
    """A tensor hook receives the parameter's gradient and a post-accumulate-grad hook sees the final .grad, at the moment autograd
    calls them, with the side stream held back."""
    m, _ = _model(num_knots=32, seed=5)
    named = _head_named(m)
    w_head, w_kan = m.classification_head.fc1.weight, m.kan_module.kan_layers[0].spline_weights
    feats, ys = _inputs(1024, 1, seed=6)
    ref = _oracle_head_grads(m, feats, ys)
    keys = {'head': 'classification_head.fc1.weight', 'kan': 'kan_module.kan_layers.0.spline_weights'}

    seen = {}
    hs = [w_head.register_hook(lambda g: seen.__setitem__('head', g.clone())),
          w_kan.register_hook(lambda g: seen.__setitem__('kan', g.clone()))]
    _hold_side_stream()
    _phase_loss(m, feats[0], ys[0]).backward()
    torch.cuda.synchronize()
    for h in hs:
        h.remove()
    assert set(seen) == {'head', 'kan'}
    _check_heads({keys[k]: v for k, v in seen.items()}, {keys[k]: ref[keys[k]] for k in seen}, C5_TOL, 'tensor hooks')

    for p in m.parameters():
        p.grad = None
    post = {}
    hs = [w_head.register_post_accumulate_grad_hook(lambda p: post.__setitem__('head', p.grad.clone())),
          w_kan.register_post_accumulate_grad_hook(lambda p: post.__setitem__('kan', p.grad.clone()))]
    _hold_side_stream()
    _phase_loss(m, feats[0], ys[0]).backward()
    torch.cuda.synchronize()
    for h in hs:
        h.remove()
    assert set(post) == {'head', 'kan'}
    _check_heads({keys[k]: v for k, v in post.items()}, {keys[k]: ref[keys[k]] for k in post}, C5_TOL, 'post-accumulate hooks')
    _check_heads({n: p.grad for n, p in named}, ref, C5_TOL, '.grad after hooked backward')


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _fp64_reference_step(opt, max_norm=1.0):
    """clip_grad_norm_ + torch.optim.AdamW in fp64 on copies of the GPU's parameters and gradients (RoViTAdamW's two groups).
    The hyperparameters are rounded to fp32 first, as the kernel receives them: beta2 = 0.999 is 0.99900001287 in fp32, so the second
    moment's (1 - beta2) differs by 1.29e-5 relative from the exact value (the bias correction cancels it in the parameters)."""
    d = opt.defaults
    betas, eps, weight_decay = tuple(_f32(b) for b in d['betas']), _f32(d['eps']), _f32(d['weight_decay'])
    groups, flat = [], []
    for grp in opt.param_groups:
        ps = []
        for p in grp['params']:
            q = p.detach().cpu().double().requires_grad_(True)
            q.grad = None if p.grad is None else p.grad.detach().cpu().double()
            ps.append(q)
        groups.append({'params': ps, 'lr': _f32(grp['lr'])})
        flat += ps
    norm = torch.nn.utils.clip_grad_norm_([q for q in flat if q.grad is not None], max_norm)
    ref_opt = torch.optim.AdamW(groups, betas=betas, eps=eps, weight_decay=weight_decay)
    ref_opt.step()
    return flat, ref_opt, float(norm)


def _gpu_moments(opt):
    """(m, v) views of every parameter in param-group order."""
    out = [(opt.m_flat[o:o + p.numel()].view_as(p), opt.v_flat[o:o + p.numel()].view_as(p)) for o, p in zip(opt._bb_offsets, opt.bb_params)]
    for s in opt.segments:
        out += [(opt.o_m[o:o + p.numel()].view_as(p), opt.o_v[o:o + p.numel()].view_as(p)) for o, p in zip(s.offsets, s.params)]
    return out


def _check_step(opt, flat, ref_opt, tol=1e-5):
    params = [p for g in opt.param_groups for p in g['params']]
    worst = 0.0
    for p, q, (mg, vg) in zip(params, flat, _gpu_moments(opt)):
        if q.grad is None:
            continue
        e = _rel(p, q.detach())
        st = ref_opt.state[q]
        e = max(e, _rel(mg, st['exp_avg']), _rel(vg, st['exp_avg_sq']))
        worst = max(worst, e)
        assert e <= tol, (tuple(p.shape), e)
    print(f'optimizer step: worst parameter / moment error {worst:.3g} relative against fp64 clip_grad_norm_ + AdamW')


def test_two_forwards_one_backward_sum_both_gradients():
    """(loss(m(x1)) + loss(m(x2))).backward() with the optimizer's gradient views in place: two HeadPhaseFn nodes in one pass must give
    g(x1) + g(x2), equal to the per-module path and the fp64 oracle, and the optimizer step after it must be clip_grad_norm_ + AdamW."""
    sd = ref_cpu.init_rovit_state(seed=41)
    m, opt = _model(sd=sd)
    named = _head_named(m)
    loss_fn = _loss_fn()
    g = torch.Generator().manual_seed(42)
    xs = [torch.randn(4, 3, 224, 224, generator=g) for _ in range(2)]
    ys = [torch.randint(0, 4, (4,), generator=g) for _ in range(2)]

    def both():
        outs = [m(x.to(dev())) for x in xs]
        total = sum(loss_fn(o, y.to(dev()), y.to(dev()), 4)['total_loss'] for o, y in zip(outs, ys))
        total.backward()
        torch.cuda.synchronize()
        return outs

    # per-module path: a forward hook on a head keeps the model off the fused phase
    h = m.classification_head.register_forward_hook(lambda mod, i, o: None)
    assert not m._head_phase_fusable(torch.zeros(4, 192, device=dev()))
    both()
    per_module = {n: p.grad.detach().clone() for n, p in named}
    h.remove()
    opt.zero_grad(set_to_none=True)

    assert m._head_phase_fusable(torch.zeros(4, 192, device=dev()))
    outs = both()
    got = {n: p.grad for n, p in named}
    worst = max(_rel(got[n], per_module[n].cpu().double()) for n, _ in named)
    print(f'fused against per-module path: worst head / KAN gradient difference {worst:.3g} relative')
    assert worst <= 1e-5

    # fp64 oracle: heads / KAN at the features the GPU produced, the gradient flowing through the oracle's own backbone
    ref_p = {k: (v.double().requires_grad_(True) if 'knots' not in k else v.double()) for k, v in sd.items()}
    total = 0
    for x, y, o in zip(xs, ys, outs):
        f_ref = ref_cpu.vit_forward(x.double(), ref_p, prefix='backbone.model.')
        f_used = f_ref + (o['features'].detach().cpu().double() - f_ref).detach()
        total = total + ref_cpu.joint_loss(_oracle_out(f_used, ref_p), y, y, 4)['total_loss']
    total.backward()
    _check_heads(got, {n: ref_p[n].grad for n, _ in named}, HEAD_TOL, 'two forwards, one backward')
    worst_bb = 0.0
    for n, p in m.named_parameters():
        if not n.startswith('backbone.'):
            continue
        ref, gp = ref_p[n].grad, p.grad.detach().cpu().double()
        rel = _rel(gp, ref)
        cos = float(torch.nn.functional.cosine_similarity(gp.flatten(), ref.flatten(), dim=0))
        worst_bb = max(worst_bb, rel)
        assert cos > 0.999 and rel < 6e-2, (n, cos, rel)
    print(f'two forwards, one backward: worst backbone gradient error {worst_bb:.3g} relative')

    flat, ref_opt, norm = _fp64_reference_step(opt)
    opt.step()
    torch.cuda.synchronize()
    assert abs(float(opt.last_grad_norm) - norm) <= 1e-5 * norm
    _check_step(opt, flat, ref_opt)


class _ManySegments(torch.nn.Module):
    """A model the optimizer accepts (backbone.model + top-level modules with their own parameters) whose loss uses every other
    module: the live head gradients form five disjoint runs of the optimizer's flat buffer, six buffers with the backbone's."""

    N = 9

    def __init__(self):
        super().__init__()
        from models.backbone import DeiTTinyBackbone
        self.backbone = DeiTTinyBackbone(pretrained=False, freeze=False)
        for i in range(self.N):
            setattr(self, f'lin{i}', torch.nn.Linear(192, 3 + i % 3))

    def forward(self, x):
        f = self.backbone(x)
        return [getattr(self, f'lin{i}')(f) for i in range(0, self.N, 2)]


def test_clipping_over_many_disjoint_gradient_runs_is_exact_and_bit_reproducible(monkeypatch):
    from rovit_hip import optim
    from rovit_hip.optim import RoViTAdamW
    torch.manual_seed(7)
    m = _ManySegments().to(dev()).train()
    opt = RoViTAdamW(m, lr=1e-3)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 3, 224, 224, generator=g).to(dev())
    ws = [torch.randn(2, 3 + i % 3, generator=g).to(dev()) for i in range(0, m.N, 2)]
    sum(((o * w).sum() for o, w in zip(m(x), ws)), torch.zeros((), device=dev())).backward()
    torch.cuda.synchronize()
    live = [s for s in opt.segments if any(p.grad is not None for p in s.params)]
    assert len(opt._runs(live)) >= 5 and opt._backbone_active()

    calls = []
    real_call = optim.call
    monkeypatch.setattr(optim, 'call', lambda name, *a: (calls.append((name, a)), real_call(name, *a))[1])
    bufs = {'p_flat': opt.p_flat, 'm_flat': opt.m_flat, 'v_flat': opt.v_flat, 'o_flat': opt.o_flat, 'o_m': opt.o_m, 'o_v': opt.o_v}
    start = {k: v.clone() for k, v in bufs.items()}
    start_t = (opt.t, [s.t for s in opt.segments])
    flat, ref_opt, norm = _fp64_reference_step(opt)

    results = []
    for _ in range(3):                                 # the same step three times from the same state and gradients
        for k, v in bufs.items():
            v.copy_(start[k])
        opt.t = start_t[0]
        for s, t in zip(opt.segments, start_t[1]):
            s.t = t
        calls.clear()
        opt.step()
        torch.cuda.synchronize()
        names = [c[0] for c in calls]
        assert 'rovit_sq_norm_clip' not in names and names.count('rovit_sq_norm_accum') >= 6, names    # the many-run branch
        assert all(c[1][3] is not None for c in calls if c[0] == 'rovit_sq_norm_accum'), 'float-atomic norm accumulation'
        results.append({'norm': opt.last_grad_norm.clone(), **{k: v.clone() for k, v in bufs.items()}})
        if len(results) == 1:
            got = float(opt.last_grad_norm)
            print(f'many runs: grad norm {got:.9g} against fp64 {norm:.9g} (relative {abs(got - norm) / norm:.3g})')
            assert abs(got - norm) <= 1e-6 * norm
            _check_step(opt, flat, ref_opt)
    for r in results[1:]:
        for k in results[0]:
            assert torch.equal(results[0][k], r[k]), k
