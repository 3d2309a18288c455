"""GPU tests of the weight average: rovit_adamw_ema_flat_multi against rovit_adamw_flat_multi (p, m, v bit for bit) and against the fp64
restatement ``rovit_hip.optim.ema_reference`` (the average), its per-segment modes and argument checks, rovit_swap_flat_multi,
``RoViTAdamW(ema_decay=...)`` against a twin without an average, ``swap_ema()``, and the Trainer / checkpoint / evaluation path.

Tolerance of the average, derived rather than tuned: one fp32 step e + omd (p - e) commits at most three roundings of
magnitude <= 2^-24 S, S = max(|p|, |e|) over the segment, so against ``ema_reference`` fed with the kernel's own p_new each step the error
after t steps is at most 3 t 2^-24 S.  Every test prints its worst error as a fraction of t 2^-24 S."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu  # noqa: E402  (checker only: seeded initial weights)

U = 2.0 ** -24
GUARD = 64                       # sentinel floats either side of every buffer
SENTINEL = 12345.0
PIECE = 2048                     # floats per block (ADAM_PIECE4 float4)
SIZES = [1, 3, 4, 5, PIECE - 1, PIECE, PIECE + 1, 3 * PIECE + 5]
# four-segment calls: every size of SIZES, the tail-only sizes first, last and between multi-block segments
COMBOS = [(1, 3, 4, 5), (PIECE - 1, PIECE, PIECE + 1, 3 * PIECE + 5), (3 * PIECE + 5, 1, PIECE + 1, 3), (5, PIECE, 4, PIECE - 1)]
LRS, TS, DECAYS = (1e-3, 3e-4, 1e-2, 5e-5), (1, 2, 7, 1000), (0.5, 0.9, 0.999, 2.0 / 11.0)
BETAS_EPS_WD = (0.9, 0.999, 1e-8, 1e-2)


def dev():
    return torch.device('cuda:0')


# ---- buffers with sentinels, and the two entries through the C ABI -------------------------------------------------------------------------

class Guarded:
    """n floats with GUARD sentinel floats on each side; ``.t`` is the 16-byte aligned view a kernel gets."""

    def __init__(self, values: torch.Tensor):
        n = values.numel()
        self.full = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev())
        self.t = self.full[GUARD:GUARD + n]
        self.t.copy_(values)
        assert self.t.data_ptr() % 16 == 0

    def copy(self):
        return Guarded(self.t)

    def intact(self) -> bool:
        return bool((self.full[:GUARD] == SENTINEL).all()) and bool((self.full[GUARD + self.t.numel():] == SENTINEL).all())


def _segment(n, gen):
    r = lambda s=1.0: torch.randn(n, generator=gen) * s
    return {'p': Guarded(r()), 'g': Guarded(r()), 'm': Guarded(r(0.1)), 'v': Guarded(torch.rand(n, generator=gen) * 1e-2), 'e': Guarded(r())}


def _ptrs(bufs):
    return (C.c_void_p * len(bufs))(*[None if b is None else b.t.data_ptr() for b in bufs])


def _plain(segs, lrs, ts, coef):
    from rovit_hip import native
    k = len(segs)
    native.call('rovit_adamw_flat_multi', *(_ptrs([s[x] for s in segs]) for x in 'pgmv'), (C.c_size_t * k)(*[s['p'].t.numel() for s in segs]),
                (C.c_float * k)(*lrs), (C.c_int * k)(*ts), k, None if coef is None else coef.data_ptr(), *BETAS_EPS_WD, native.stream_ptr())


def _ema_args(segs, lrs, ts, decays, coef):
    from rovit_hip import native
    k = len(segs)
    return (*(_ptrs([s.get(x) for s in segs]) for x in 'pgmve'), (C.c_size_t * k)(*[s['p'].t.numel() for s in segs]),
            (C.c_float * k)(*lrs), (C.c_int * k)(*ts), (C.c_float * k)(*decays), k, None if coef is None else coef.data_ptr(), *BETAS_EPS_WD,
            native.stream_ptr())


def _ema(segs, lrs, ts, decays, coef):
    from rovit_hip import native
    native.call('rovit_adamw_ema_flat_multi', *_ema_args(segs, lrs, ts, decays, coef))


def _copy(segs):
    return [{k: b.copy() for k, b in s.items()} for s in segs]


def _np(t):
    return t.detach().cpu().numpy()


def _ema_ratio(e_new, e_old, p_new, decay, steps=1, S=None):
    """Worst |e_new - ema_reference(e_old, p_new)| as a fraction of steps * 2^-24 * S; the caller asserts <= 3."""
    from rovit_hip.optim import ema_reference
    ref = ema_reference(e_old, p_new, decay)
    S = max(float(np.abs(p_new).max()), float(np.abs(e_old).max())) if S is None else S
    return float(np.abs(e_new.astype(np.float64) - ref).max()) / (steps * U * S)


def _all_intact(*seg_lists):
    return all(b.intact() for segs in seg_lists for s in segs for b in s.values())


# ---- 1. against the plain kernel ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('with_scale', [True, False])
@pytest.mark.parametrize('sizes', COMBOS)
def test_kernel_matches_the_plain_kernel_bit_for_bit_and_the_average_is_within_one_step(sizes, with_scale):
    gen = torch.Generator().manual_seed(sum(sizes) + int(with_scale))
    segs = [_segment(n, gen) for n in sizes]
    want = _copy(segs)
    before = _copy(segs)
    coef = torch.tensor(0.37, device=dev()) if with_scale else None
    _plain(want, LRS, TS, coef)
    _ema(segs, LRS, TS, DECAYS, coef)
    torch.cuda.synchronize()
    worst = 0.0
    for i, (s, w, b) in enumerate(zip(segs, want, before)):
        for x in 'pmv':
            assert torch.equal(s[x].t, w[x].t), (sizes, i, x)
        assert not torch.equal(s['p'].t, b['p'].t) and torch.equal(s['g'].t, b['g'].t)
        assert torch.equal(w['e'].t, b['e'].t)
        ratio = _ema_ratio(_np(s['e'].t), _np(b['e'].t), _np(s['p'].t), DECAYS[i])
        worst = max(worst, ratio)
        assert ratio <= 3.0, (sizes, i, ratio)
    assert _all_intact(segs, want)
    print(f'sizes {sizes} grad_scale {with_scale}: worst average error {worst:.3f} x 2^-24 S (bound 3)')


# ---- 2. the recursion ---------------------------------------------------------------------------------------------------------------------

def _recursion_run(n=3 * PIECE + 5, steps=24, decay=0.999):
    from rovit_hip.optim import ema_reference
    gen = torch.Generator().manual_seed(11)
    s = _segment(n, gen)
    s['m'].t.zero_(); s['v'].t.zero_()
    s['e'].t.copy_(s['p'].t)                                  # the average starts as the parameters
    ref = _np(s['e'].t).astype(np.float64)
    S, averages, ratios = float(np.abs(ref).max()), [], []
    for t in range(1, steps + 1):
        s['g'].t.copy_(torch.randn(n, generator=gen))         # fresh gradients
        d = min(decay, (1.0 + t) / (10.0 + t))                # warm-up
        _ema([s], [1e-2], [t], [d], None)
        p_new, e_new = _np(s['p'].t), _np(s['e'].t)
        S = max(S, float(np.abs(p_new).max()), float(np.abs(e_new).max()))
        ref = ema_reference(ref, p_new, d)
        ratios.append(float(np.abs(e_new.astype(np.float64) - ref).max()) / (t * U * S))
        averages.append(e_new.copy())
    assert all(b.intact() for b in s.values())
    return averages, ratios


def test_recursion_of_24_warmup_steps_stays_within_the_bound_and_reproduces_itself():
    a1, r1 = _recursion_run()
    for t, r in enumerate(r1, 1):
        assert r <= 3.0, (t, r)
    assert not np.array_equal(a1[0], a1[-1])
    a2, _ = _recursion_run()
    for x, y in zip(a1, a2):
        assert np.array_equal(x, y)
    print(f'24 steps: worst average error {max(r1):.3f} x t 2^-24 S (bound 3), at the last step {r1[-1]:.3f}')


# ---- 3. segment modes and argument checks -------------------------------------------------------------------------------------------------

MODE_SIZES = (PIECE + 1, 5, 3 * PIECE + 5, 3)


@pytest.mark.parametrize('k', [0, 1, 3])
def test_an_ema_only_segment_leaves_p_m_v_alone_and_its_neighbours_are_right(k):
    gen = torch.Generator().manual_seed(20 + k)
    segs = [_segment(n, gen) for n in MODE_SIZES]
    before = _copy(segs)
    others = [i for i in range(4) if i != k]
    want = [_copy(segs)[i] for i in others]
    coef = torch.tensor(0.5, device=dev())
    _plain(want, [LRS[i] for i in others], [TS[i] for i in others], coef)
    call = [dict(s) for s in segs]
    call[k]['g'] = None
    if k != 1:                                                # m, v may be NULL for an EMA-only segment; given, they are not written
        call[k]['m'] = call[k]['v'] = None
    ts = list(TS)
    ts[k] = 0                                                 # ignored for an EMA-only segment
    _ema(call, LRS, ts, DECAYS, coef)
    torch.cuda.synchronize()
    for x in 'pgmv':
        assert torch.equal(segs[k][x].t, before[k][x].t), x
    assert _ema_ratio(_np(segs[k]['e'].t), _np(before[k]['e'].t), _np(before[k]['p'].t), DECAYS[k]) <= 3.0
    assert not torch.equal(segs[k]['e'].t, before[k]['e'].t)
    for i, w in zip(others, want):
        for x in 'pmv':
            assert torch.equal(segs[i][x].t, w[x].t), (i, x)
        assert _ema_ratio(_np(segs[i]['e'].t), _np(before[i]['e'].t), _np(segs[i]['p'].t), DECAYS[i]) <= 3.0, i
    assert _all_intact(segs, want)


def test_a_segment_without_an_average_is_the_plain_kernel():
    gen = torch.Generator().manual_seed(30)
    segs = [_segment(n, gen) for n in MODE_SIZES]
    before, want = _copy(segs), _copy(segs)
    _plain(want, LRS, TS, None)
    call = [dict(s) for s in segs]
    call[2]['e'] = None
    decays = list(DECAYS)
    decays[2] = 7.0                                           # not read without an average
    _ema(call, LRS, TS, decays, None)
    torch.cuda.synchronize()
    for i in range(4):
        for x in 'pmv':
            assert torch.equal(segs[i][x].t, want[i][x].t), (i, x)
        if i == 2:
            assert torch.equal(segs[i]['e'].t, before[i]['e'].t)
        else:
            assert _ema_ratio(_np(segs[i]['e'].t), _np(before[i]['e'].t), _np(segs[i]['p'].t), DECAYS[i]) <= 3.0, i
    assert _all_intact(segs, want)


def test_bad_arguments_return_their_error_codes_without_a_launch():
    from rovit_hip import native
    lib = native.load()
    gen = torch.Generator().manual_seed(31)
    segs = [_segment(n, gen) for n in (5, PIECE + 1)]
    before = _copy(segs)
    both_null = [dict(s) for s in segs]
    both_null[1]['g'] = both_null[1]['e'] = None
    assert lib.rovit_adamw_ema_flat_multi(*_ema_args(both_null, LRS[:2], TS[:2], DECAYS[:2], None)) == -3          # ROVIT_ERR_NULL
    for bad in (1.0, -0.1):
        assert lib.rovit_adamw_ema_flat_multi(*_ema_args(segs, LRS[:2], TS[:2], [0.5, bad], None)) == -1           # ROVIT_ERR_SHAPE
    ema_only = [dict(s, g=None) for s in segs]
    assert lib.rovit_adamw_ema_flat_multi(*_ema_args(ema_only, LRS[:2], TS[:2], [1.0, 0.5], None)) == -1
    with pytest.raises(native.RovitHipError):
        _ema(segs, LRS[:2], TS[:2], [0.5, 1.0], None)
    torch.cuda.synchronize()
    for s, b in zip(segs, before):
        for x in 'pgmve':
            assert torch.equal(s[x].full, b[x].full), x


# ---- 4. swap ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('sizes', COMBOS)
def test_swap_exchanges_exactly_twice_is_the_identity_and_sentinels_stay(sizes):
    from rovit_hip import native
    gen = torch.Generator().manual_seed(40 + sum(sizes))
    a = [Guarded(torch.randn(n, generator=gen)) for n in sizes]
    b = [Guarded(torch.randn(n, generator=gen)) for n in sizes]
    a0, b0 = [x.copy() for x in a], [x.copy() for x in b]
    args = (_ptrs(a), _ptrs(b), (C.c_size_t * 4)(*sizes), 4, native.stream_ptr())
    native.call('rovit_swap_flat_multi', *args)
    torch.cuda.synchronize()
    for i in range(4):
        assert torch.equal(a[i].t, b0[i].t) and torch.equal(b[i].t, a0[i].t), (sizes, i)
        assert a[i].intact() and b[i].intact()
    native.call('rovit_swap_flat_multi', *args)
    torch.cuda.synchronize()
    for i in range(4):
        assert torch.equal(a[i].full, a0[i].full) and torch.equal(b[i].full, b0[i].full), (sizes, i)


# ---- 5. the optimizer against a twin without an average ------------------------------------------------------------------------------------

def _depth2_model(seed=21):
    from models.backbone import DeiTTiny
    from models.rovit_kan import RoViTKAN
    sd = ref_cpu.init_rovit_state(depth=2, seed=seed)
    m = RoViTKAN(pretrained=False)
    m.backbone.model = DeiTTiny(depth=2)
    m.load_state_dict(sd, strict=True)
    return m.to(dev()).eval()                                # no dropout: twins must agree bit for bit


def _loss_fn():
    from rovit_hip.losses import JointLoss
    return JointLoss(1.0, 0.5, 0.5, 2.0, focal_alpha=torch.ones(4, device=dev()), num_classes=4)


def _batch(i, B=8):
    g = torch.Generator().manual_seed(100 + i)
    return torch.randn(B, 3, 224, 224, generator=g).to(dev()), torch.randint(0, 4, (B,), generator=g).to(dev())


def _train_step(m, opt, loss_fn, i, stage):
    x, y = _batch(i)
    m.curriculum_stage = stage
    loss = loss_fn(m(x), y, y, stage)['total_loss']
    opt.zero_grad()
    loss.backward()
    opt.step()


def _group(name):
    return name.split('.')[0]


def test_optimizer_with_an_average_trains_like_its_twin_and_tracks_the_fp64_recursion():
    from rovit_hip.optim import RoViTAdamW, ema_reference
    m_ema, m_twin = _depth2_model(), _depth2_model()
    opt = RoViTAdamW(m_ema, lr=1e-3, ema_decay=0.99)
    twin = RoViTAdamW(m_twin, lr=1e-3)
    assert opt.ema_flat is not None and twin.ema_flat is None
    loss_fn = _loss_fn()
    names = [n for n, _ in m_ema.named_parameters()]
    groups = sorted({_group(n) for n in names})
    assert 'backbone' in groups and 'kan_module' in groups and len(groups) == 5
    ref = {n: _np(p).astype(np.float64) for n, p in m_ema.named_parameters()}
    t = dict.fromkeys(groups, 0)
    S = {g: max(float(np.abs(ref[n]).max()) for n in names if _group(n) == g) for g in groups}
    worst = 0.0
    # steps 1-2: backbone frozen, stage 3; step 3: unfrozen; steps 4-6: stage 4 (the KAN segment starts late); step 7, beyond the six
    # the feature was specified with: backbone frozen again, so its average goes on trailing parameters that no longer move
    for m in (m_ema, m_twin):
        m.freeze_backbone()
    for step in range(1, 8):
        if step in (3, 7):
            for m in (m_ema, m_twin):
                m.unfreeze_backbone() if step == 3 else m.freeze_backbone()
        stage = 3 if step <= 3 else 4
        _train_step(m_ema, opt, loss_fn, step, stage)
        _train_step(m_twin, twin, loss_fn, step, stage)
        twin_p = dict(m_twin.named_parameters())
        for n, p in m_ema.named_parameters():
            assert torch.equal(p, twin_p[n]), (step, n)
        active = {g: (3 <= step < 7) if g == 'backbone' else (step >= 4 if g == 'kan_module' else True) for g in groups}
        for g in groups:
            t[g] += int(active[g])
        ema_sd = opt.ema_state_dict()
        assert list(ema_sd) == list(m_ema.state_dict()) and all(ema_sd[k].shape == v.shape for k, v in m_ema.state_dict().items())
        snap = {n: _np(p) for n, p in m_ema.named_parameters()}
        for n in names:
            g = _group(n)
            got = _np(ema_sd[n])
            if t[g] == 0:                                     # never stepped: the average IS the parameters
                assert np.array_equal(got, snap[n]), (step, n)
                continue
            S[g] = max(S[g], float(np.abs(snap[n]).max()), float(np.abs(got).max()))
        for n in names:
            g = _group(n)
            if t[g] == 0:
                continue
            ref[n] = ema_reference(ref[n], snap[n], opt.ema_decay_at(t[g]))          # active, or frozen after having been stepped
            # updates so far: one per step since the segment's first (a re-frozen segment keeps being averaged)
            updates = t[g] + (1 if g == 'backbone' and step == 7 else 0)
            ratio = float(np.abs(_np(ema_sd[n]).astype(np.float64) - ref[n]).max()) / (updates * U * S[g])
            worst = max(worst, ratio)
            assert ratio <= 3.0, (step, n, ratio)
        for k, v in m_ema.state_dict().items():
            if k not in snap:
                assert torch.equal(ema_sd[k], v), k           # buffers (the KAN knots) come from the model
    assert opt.t == twin.t == t['backbone'] == 4
    assert {s.name: s.t for s in opt.segments} == {s.name: s.t for s in twin.segments} == {g: t[g] for g in groups if g != 'backbone'}
    assert t['kan_module'] == 4 and t['classification_head'] == 7
    assert not np.array_equal(_np(opt.ema_state_dict()[names[0]]), _np(dict(m_ema.named_parameters())[names[0]]))
    print(f'optimizer, 7 steps: worst average error {worst:.3f} x t 2^-24 S (bound 3)')


# ---- 6. swap_ema ------------------------------------------------------------------------------------------------------------------------

def _trained(steps=3):
    from rovit_hip.optim import RoViTAdamW
    m = _depth2_model(seed=22)
    opt = RoViTAdamW(m, lr=1e-3, ema_decay=0.9, ema_warmup=False)
    loss_fn = _loss_fn()
    for i in range(steps):
        _train_step(m, opt, loss_fn, 50 + i, 4)
    return m, opt, loss_fn


def test_swap_ema_computes_with_the_average_and_leaves_training_untouched():
    from rovit_hip import RovitHipError
    from rovit_hip.optim import RoViTAdamW
    m, opt, loss_fn = _trained()
    twin_m, twin_opt, _ = _trained()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    ema_sd = opt.ema_state_dict()
    assert any(not torch.equal(ema_sd[k], before[k]) for k in before)
    loaded = _depth2_model(seed=23)
    loaded.load_state_dict(ema_sd)
    x, _ = _batch(60)
    with torch.no_grad():
        raw = m.eval()(x)
        want = loaded.eval()(x)
        with opt.swap_ema():
            got = m.eval()(x)
            with pytest.raises(RovitHipError):
                with opt.swap_ema():
                    pass
            with pytest.raises(RovitHipError):
                opt.step()
            inside = opt.ema_state_dict()                     # still the average while it sits under the model
        after = m.eval()(x)
    keys = ('features', 'cls_logits', 'ordinal_logits', 'mu', 'log_var', 'kan_severity')
    for k in keys:
        assert torch.equal(got[k], want[k]), k
        assert torch.equal(after[k], raw[k]), k
    assert not torch.equal(got['cls_logits'], raw['cls_logits']) and not torch.equal(got['kan_severity'], raw['kan_severity'])
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
        assert torch.equal(inside[k], ema_sd[k]), k
    for k, v in opt.ema_state_dict().items():
        assert torch.equal(v, ema_sd[k]), k
    # one more training step: a missing re-preparation of the bf16 / KAN weights after the swap back would show here
    _train_step(m, opt, loss_fn, 70, 4)
    _train_step(twin_m, twin_opt, loss_fn, 70, 4)
    twin_p = dict(twin_m.named_parameters())
    for n, p in m.named_parameters():
        assert torch.equal(p, twin_p[n]), n
    twin_ema = twin_opt.ema_state_dict()
    for k, v in opt.ema_state_dict().items():
        assert torch.equal(v, twin_ema[k]), k
    with pytest.raises(RovitHipError):
        with RoViTAdamW(loaded, lr=1e-3).swap_ema():
            pass
    # load_ema_state_dict is the inverse of ema_state_dict
    opt.load_ema_state_dict(ema_sd)
    for k, v in opt.ema_state_dict().items():
        assert torch.equal(v, ema_sd[k]), k
    covered = torch.zeros(opt._o_total, dtype=torch.bool)
    for seg in opt.segments:
        for o, p in zip(seg.offsets, seg.params):
            covered[o:o + p.numel()] = True
    assert bool((opt.o_ema.cpu()[~covered] == 0).all())       # the padding floats of the average stay zero


# ---- 7. Trainer, checkpoint, evaluation ---------------------------------------------------------------------------------------------------

def _stage_for_epoch(epoch):          # module level: the config is pickled into the checkpoint
    return min(4, epoch + 2)


def _loaders():
    g = torch.Generator().manual_seed(5)
    mk = lambda: (torch.randn(8, 3, 224, 224, generator=g), torch.randint(0, 4, (8,), generator=g))
    train = [(x, y, y.clone()) for x, y in (mk() for _ in range(4))]          # a four-batch loader, host tensors like a DataLoader's
    val = [(x, y, y.clone()) for x, y in (mk() for _ in range(2))]
    return train, val


def _make_trainer(seed, tmp_path, ema_decay=0.9):
    from models.rovit_kan import RoViTKAN
    from training import JointLoss, Trainer, build_optimizer, build_scheduler
    torch.manual_seed(seed)
    np.random.seed(seed)
    train = SimpleNamespace(learning_rate=1e-3, weight_decay=1e-4, epochs=2, early_stop_patience=5)
    if ema_decay is not None:
        train.ema_decay, train.ema_warmup = ema_decay, True
    cfg = SimpleNamespace(
        train=train,
        flags=SimpleNamespace(use_cutmix=True, use_mixup=True, cutmix_alpha=1.0, mixup_alpha=0.2, mixed_precision=True, gradient_clip=1.0,
                              freeze_backbone_epochs=1, curriculum=True),
        model=SimpleNamespace(embed_dim=192, hidden_dim=128, kan_layers=[192, 64, 16, 1], kan_num_knots=5, kan_degree=3, dropout=0.3,
                              pretrained=False),
        data=SimpleNamespace(num_classes=4),
        paths=SimpleNamespace(checkpoints_dir=tmp_path), get_stage_for_epoch=_stage_for_epoch)
    tr, va = _loaders()
    model = RoViTKAN(pretrained=False)
    opt = build_optimizer(model, cfg)                        # before the model moves to the device, as scripts/train.py does
    return Trainer(model, tr, va, opt, build_scheduler(opt, cfg), JointLoss(), cfg, dev()), cfg


def _third_epoch(trainer):
    torch.manual_seed(77)                                    # dropout and the device permutation of CutMix / MixUp
    np.random.seed(77)                                       # the mixing draws
    trainer.train_epoch(3)
    torch.cuda.synchronize()


def test_trainer_validates_checkpoints_and_resumes_with_the_average(tmp_path):
    from evaluation.evaluator import load_model_for_evaluation
    from models.rovit_kan import RoViTKAN
    from rovit_hip.evaluation import validate
    t, cfg = _make_trainer(0, tmp_path)
    assert t.optimizer.ema_decay == 0.9
    history = t.fit()                                        # two epochs; the backbone is frozen for the first
    assert all(len(v) == 2 and np.isfinite(v).all() for v in history.values())
    # val_epoch validates the averaged weights
    got = t.val_epoch()
    ema_sd = t.optimizer.ema_state_dict()
    averaged = RoViTKAN(pretrained=False)
    averaged.load_state_dict(ema_sd)
    assert got == validate(averaged.to(dev()), t.val_loader, t.loss_fn)
    assert got['loss'] != validate(t.model, t.val_loader, t.loss_fn)['loss']
    assert history['val_loss'][-1] == got['loss']
    # the best checkpoint holds both sets of weights
    best = torch.load(tmp_path / 'best_model.pth', map_location='cpu', weights_only=False)
    assert set(best) == {'epoch', 'model_state_dict', 'optimizer_state_dict', 'scheduler_state_dict', 'best_val_loss', 'metrics', 'config',
                         'ema_state_dict'}
    assert set(best['ema_state_dict']) == set(best['model_state_dict'])
    assert {'ema_flat', 'o_ema'} <= set(best['optimizer_state_dict']['rovit_flat'])
    assert any(not torch.equal(best['ema_state_dict'][k], best['model_state_dict'][k]) for k in best['model_state_dict'])
    # resume: a fresh Trainer from the end-of-epoch-2 state trains epoch 3 exactly like the uninterrupted run
    resume = tmp_path / 'resume.pth'
    t.save_checkpoint(resume, 2, got)
    fresh, _ = _make_trainer(7, tmp_path)
    fresh.load_checkpoint(resume)
    for k, v in fresh.optimizer.ema_state_dict().items():
        assert torch.equal(v, ema_sd[k]), k
    _third_epoch(t)
    _third_epoch(fresh)
    fresh_p = dict(fresh.model.named_parameters())
    for n, p in t.model.named_parameters():
        assert torch.equal(p, fresh_p[n]), n
    fresh_ema = fresh.optimizer.ema_state_dict()
    for k, v in t.optimizer.ema_state_dict().items():
        assert torch.equal(v, fresh_ema[k]), k
    assert any(not torch.equal(fresh_ema[k], ema_sd[k]) for k in ema_sd)          # and epoch 3 moved it
    # evaluation loads the average unless told otherwise
    ck = torch.load(resume, map_location='cpu', weights_only=False)
    for use_ema, key in ((None, 'ema_state_dict'), (True, 'ema_state_dict'), (False, 'model_state_dict')):
        m = load_model_for_evaluation(resume, cfg, dev(), use_ema=use_ema)
        assert not m.training
        for k, v in m.state_dict().items():
            assert torch.equal(v.cpu(), ck[key][k]), (use_ema, k)
    plain = tmp_path / 'plain.pth'
    torch.save({k: v for k, v in ck.items() if k != 'ema_state_dict'}, plain)
    m = load_model_for_evaluation(plain, cfg, dev())
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), ck['model_state_dict'][k]), k
    with pytest.raises(KeyError):
        load_model_for_evaluation(plain, cfg, dev(), use_ema=True)


def test_trainer_without_an_average_writes_the_keys_it_wrote_before(tmp_path):
    t, _ = _make_trainer(0, tmp_path, ema_decay=None)
    assert t.optimizer.ema_decay is None and t.optimizer.ema_flat is None
    t.train_epoch(1)
    t.save_checkpoint(tmp_path / 'c.pth', 1, t.val_epoch())
    ck = torch.load(tmp_path / 'c.pth', map_location='cpu', weights_only=False)
    assert set(ck) == {'epoch', 'model_state_dict', 'optimizer_state_dict', 'scheduler_state_dict', 'best_val_loss', 'metrics', 'config'}
    assert set(ck['optimizer_state_dict']['rovit_flat']) == {'m_flat', 'v_flat', 'o_m', 'o_v', 't', 'segment_t'}
