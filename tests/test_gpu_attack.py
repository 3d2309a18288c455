"""GPU tests of the attack kernels (csrc/attack.hip), of ``rovit_hip.attack`` on them (``objective_gradient``, ``PGD``,
``pgd_attack``, ``robustness_radius``) and of ``Evaluator.evaluate_adversarial``.

Oracles: ``step_reference`` / ``init_reference`` (numpy, pinned on the CPU in tests/test_attack_cpu.py): fp32 and bit for bit for the
L-infinity kernels, fp64 within the derived tolerance of tests/attack_cases.py for the L2 kernels; fp64 autograd through the oracle
backbone and heads for the objective's gradient, with the bounds tests/test_gpu_input_grad.py holds the same chain to."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attack_cases as ac  # noqa: E402
import test_gpu_input_grad as tig  # noqa: E402  (the depth-2 model, the fp64 oracle chain and its bounds)
from oracle import ref_cpu  # noqa: E402  (checker only)
from rovit_hip import attack as A  # noqa: E402
from rovit_hip import native  # noqa: E402

pytestmark = pytest.mark.gpu

CLASS_NAMES = ["Healthy Leaf", "Leaf Holes", "Black Spot", "Dry Leaf"]
VALUE_TOL = 1e-3          # the head phase against the fp64 heads on the SAME features (the fp32 tolerance of the smoke test)


def dev():
    return torch.device('cuda:0')


def _dev(a, misaligned=False):
    """A contiguous device copy; ``misaligned``: at a storage offset of one float (4-byte, not 16-byte aligned)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not misaligned:
        return t.to(dev())
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev())
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def _consts(clip):
    import ctypes as C
    return [(C.c_float * 3)(*[float(v) for v in arr]) for arr in A.constants(ac.MEAN, ac.STD, clip)]


def _scratch(B, shape):
    words = int(native.load().rovit_attack_scratch_doubles(B, shape[0], shape[1]))
    assert words == 2 * B * 3 * -(-shape[0] * shape[1] // 1024)
    return torch.empty(words, dtype=torch.float64, device=dev())


def _run_step(case, norm, shape, misaligned=False):
    """The step kernel on a case: (delta', x_adv, best_delta) as numpy."""
    B = case['x'].shape[0]
    inv_s, s, lo, hi = _consts(case['clip'])
    x, g, best = (_dev(case[k], misaligned) for k in ('x', 'g', 'best'))
    delta = _dev(case['delta'] if norm == 'linf' else case['delta_l2'], misaligned)
    x_adv = _dev(np.full_like(case['x'], np.nan), misaligned)
    eps, alpha, mask = _dev(case['eps']), _dev(case['alpha']), _dev(case['copy_mask'])
    p, sp = native.ptr, native.stream_ptr
    if norm == 'linf':
        native.call('rovit_attack_step_linf', p(x), p(g), p(delta), p(x_adv), p(best), p(mask.view(torch.uint8)), p(eps), p(alpha), inv_s, lo,
                    hi, B, shape[0], shape[1], sp())
    else:
        scratch = _scratch(B, shape)
        native.call('rovit_attack_step_l2', p(x), p(g), p(delta), p(x_adv), p(best), p(mask.view(torch.uint8)), p(eps), p(alpha), inv_s, s, lo,
                    hi, p(scratch), B, shape[0], shape[1], sp())
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), torch.from_numpy(case['x'])) and ac.same_bits(g.cpu().numpy(), case['g'])          # inputs untouched
    return delta.cpu().numpy(), x_adv.cpu().numpy(), best.cpu().numpy()


def _run_init(x, ids, eps, norm, shape, clip, seed, restart, misaligned=False):
    B = x.shape[0]
    inv_s, s, lo, hi = _consts(clip)
    xd = _dev(x, misaligned)
    delta, x_adv = _dev(np.full_like(x, np.nan), misaligned), _dev(np.full_like(x, np.nan), misaligned)
    p = native.ptr
    ids_d, eps_d, scratch = _dev(np.asarray(ids, np.int64)), _dev(eps), _scratch(B, shape) if norm == 'l2' else None          # kept alive
    native.call('rovit_attack_init', p(xd), p(delta), p(x_adv), p(ids_d), p(eps_d), A.NORMS[norm], seed, restart, inv_s, s, lo, hi, p(scratch),
                B, shape[0], shape[1], native.stream_ptr())
    torch.cuda.synchronize()
    return delta.cpu().numpy(), x_adv.cpu().numpy()


def _check_best(case, best, start):
    for b, copied in enumerate(case['copy_mask']):
        assert ac.same_bits(best[b], start[b] if copied else case['best'][b]), b          # the old delta, or untouched bit for bit


CASES = [(s, B, False) for s in ac.SHAPES for B in ac.BATCHES] + [(ac.MISALIGNED_SHAPE, 2, True)]
CASE_IDS = [f'{ac.shape_id(s)}-B{B}' + ('-misaligned' if m else '') for s, B, m in CASES]


# ---- 1. the L-infinity step ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('clip', [(0., 1.), None], ids=['box', 'nobox'])
@pytest.mark.parametrize('shape,B,misaligned', CASES, ids=CASE_IDS)
def test_linf_step_equals_the_fp32_reference_bit_for_bit(shape, B, misaligned, clip):
    case = ac.build(shape, B, clip)
    want_d, want_xa = A.step_reference(case['x'], case['g'], case['delta'], case['eps'], case['alpha'], 'linf', ac.MEAN, ac.STD, clip, np.float32)
    d, xa, best = _run_step(case, 'linf', shape, misaligned)
    assert ac.same_bits(d, want_d), int((ac.bits(d) != ac.bits(want_d)).sum())
    assert ac.same_bits(xa, want_xa), int((ac.bits(xa) != ac.bits(want_xa)).sum())
    _check_best(case, best, case['delta'])
    assert (np.abs(d) <= case['r']).all()
    _, _, lo, hi = A.constants(ac.MEAN, ac.STD, clip)
    assert (xa >= lo.reshape(1, 3, 1, 1)).all() and (xa <= hi.reshape(1, 3, 1, 1)).all()
    zero = case['eps'] == 0
    if clip is not None and zero.any():
        assert (xa[zero] == case['x'][zero]).all() and (d[zero] == 0).all()


# ---- 2. the L2 step -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('clip', [(0., 1.), None], ids=['box', 'nobox'])
@pytest.mark.parametrize('shape,B,misaligned', CASES, ids=CASE_IDS)
def test_l2_step_within_the_derived_tolerance_of_fp64(shape, B, misaligned, clip):
    case = ac.build(shape, B, clip, dead_image=True)
    start = case['delta_l2']
    want_d, _ = A.step_reference(case['x'], case['g'], start, case['eps'], case['alpha'], 'l2', ac.MEAN, ac.STD, clip, np.float64)
    d, xa, best = _run_step(case, 'l2', shape, misaligned)
    assert np.isfinite(d).all() and np.isfinite(xa).all()
    err, tol = np.abs(d.astype(np.float64) - want_d), ac.l2_tolerance(case, want_d)
    print(f'L2 step {ac.shape_id(shape)} B {B} {"box" if clip else "nobox"}: worst error / tolerance {float((err / tol).max()):.3f}')
    assert (err <= tol).all()
    _check_best(case, best, start)
    assert (ac.pixel_norm(d) <= ac.l2_norm_bound(case['eps'], d[0].size)).all()
    # x_adv is the box of fl32(x + delta'), to the bit, on the kernel's own delta'
    _, _, lo, hi = (v.reshape(1, 3, 1, 1) for v in A.constants(ac.MEAN, ac.STD, clip))
    assert ac.same_bits(xa, A._clamp(case['x'] + d, lo, hi))
    # the last image's gradient is zeros and NaN: no move (it starts inside its ball when B % 5 == 0; the box may still bite)
    if clip is None and ac.pixel_norm(start)[B - 1] < case['eps'][B - 1]:
        assert ac.same_bits(d[B - 1], start[B - 1])
    d2, xa2, _ = _run_step(case, 'l2', shape, misaligned)
    assert ac.same_bits(d, d2) and ac.same_bits(xa, xa2)                                   # two runs, the same bits


# ---- 3. the random start ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('clip', [(0., 1.), None], ids=['box', 'nobox'])
@pytest.mark.parametrize('shape,B,misaligned', CASES, ids=CASE_IDS)
def test_init_equals_the_references(shape, B, misaligned, clip):
    case = ac.build(shape, B, clip)
    ids = (np.arange(B, dtype=np.int64) * 37 + 5) | (np.int64(1) << 40)          # only the low 32 bits count
    seed, restart = (3 << 32) | 99, 1
    want_d, want_xa = A.init_reference(case['x'], ids, case['eps'], 'linf', seed, restart, ac.MEAN, ac.STD, clip, np.float32)
    d, xa = _run_init(case['x'], ids, case['eps'], 'linf', shape, clip, seed, restart, misaligned)
    assert ac.same_bits(d, want_d) and ac.same_bits(xa, want_xa)
    want_d, _ = A.init_reference(case['x'], ids, case['eps'], 'l2', seed, restart, ac.MEAN, ac.STD, clip, np.float64)
    d, xa = _run_init(case['x'], ids, case['eps'], 'l2', shape, clip, seed, restart, misaligned)
    err, tol = np.abs(d.astype(np.float64) - want_d), ac.l2_tolerance(case, want_d)
    print(f'L2 start {ac.shape_id(shape)} B {B}: worst error / tolerance {float((err / tol).max()):.3f}')
    assert (err <= tol).all() and np.isfinite(xa).all()
    assert (ac.pixel_norm(d) <= ac.l2_norm_bound(case['eps'], d[0].size)).all()
    assert (d[case['eps'] == 0] == 0).all()


@pytest.mark.parametrize('norm', ['linf', 'l2'])
@pytest.mark.parametrize('shape', [(3, 85), (16, 16), (224, 224)], ids=ac.shape_id)
def test_init_does_not_depend_on_the_split_and_restarts_differ(shape, norm):
    case = ac.build(shape, 5)
    ids = np.array([3, 9, 4, 1, 7])
    eps = np.full(5, 4 / 255 if norm == 'linf' else 0.5, np.float32)
    run = lambda sl, restart: _run_init(case['x'][sl], ids[sl], eps[sl], norm, shape, case['clip'], 17, restart)
    whole = run(slice(0, 5), 0)
    parts = [run(slice(0, 2), 0), run(slice(2, 5), 0)]
    for i in range(2):
        assert ac.same_bits(whole[i], np.concatenate([p[i] for p in parts]))
    assert not ac.same_bits(whole[0], run(slice(0, 5), 1)[0])


def test_kernels_refuse_bad_arguments_before_a_launch():
    from rovit_hip import RovitHipError
    case = ac.build((1, 5), 2)
    inv_s, s, lo, hi = _consts((0., 1.))
    x, g, delta, best, x_adv = (_dev(case[k]) for k in ('x', 'g', 'delta', 'best', 'x'))
    eps, alpha, mask = _dev(case['eps']), _dev(case['alpha']), _dev(case['copy_mask']).view(torch.uint8)
    ids = _dev(np.arange(2))
    p, sp = native.ptr, native.stream_ptr
    import ctypes as C
    bad = lambda v: (C.c_float * 3)(1.0, float(v), 1.0)
    good = [p(x), p(g), p(delta), p(x_adv), p(best), p(mask), p(eps), p(alpha), inv_s, lo, hi, 2, 1, 5, sp()]
    for i, v in [(0, None), (1, None), (2, None), (3, None), (4, None), (6, None), (7, None), (8, None), (9, None), (11, 0), (12, 0), (13, 0),
                 (8, bad('nan')), (8, bad(0.0)), (9, bad('nan')), (10, bad('-inf')), (9, bad('inf')), (3, p(x)), (4, p(delta))]:
        args = list(good)
        args[i] = v
        with pytest.raises(RovitHipError):
            native.call('rovit_attack_step_linf', *args)
    with pytest.raises(RovitHipError):
        native.call('rovit_attack_init', p(x), p(delta), p(x_adv), p(ids), p(eps), 2, 0, 0, inv_s, s, lo, hi, None, 2, 1, 5, sp())
    with pytest.raises(RovitHipError):           # the L2 start needs its scratch
        native.call('rovit_attack_init', p(x), p(delta), p(x_adv), p(ids), p(eps), 1, 0, 0, inv_s, s, lo, hi, None, 2, 1, 5, sp())
    torch.cuda.synchronize()
    assert ac.same_bits(delta.cpu().numpy(), case['delta'])


# ---- 4. the objective's gradient ----------------------------------------------------------------------------------------------------

def _box_images(B, seed):
    """Normalised images whose pixels are inside [0, 1]."""
    z = torch.rand(B, 3, 224, 224, generator=torch.Generator().manual_seed(seed))
    return (z - torch.tensor(ac.MEAN).view(1, 3, 1, 1)) / torch.tensor(ac.STD).view(1, 3, 1, 1)


def _oracle_value(out, objective, y, direction):
    z = out['cls_logits']
    if objective == 'ce':
        return -torch.log_softmax(z, dim=1).gather(1, y[:, None])[:, 0]
    if objective == 'margin':
        other = z.masked_fill(torch.nn.functional.one_hot(y, z.shape[1]).bool(), -float('inf')).max(dim=1).values
        return other - z.gather(1, y[:, None])[:, 0]
    return direction * out[objective][:, 0]


@pytest.mark.parametrize('objective,direction', [('ce', 1), ('margin', 1), ('mu', 1), ('mu', -1), ('kan_severity', 1)])
@pytest.mark.parametrize('B', [1, 5])
def test_objective_gradient_against_the_fp64_oracle(B, objective, direction):
    m, sd = tig._model(2, seed=30 + B)
    sd64 = tig._sd64(sd)
    x = _box_images(B, 31 + B)
    y = torch.randint(0, 4, (B,), generator=torch.Generator().manual_seed(5))
    is_class = objective in A.CLASS_OBJECTIVES
    val, grad = A.objective_gradient(m, x.to(dev()), y.to(dev()) if is_class else None, objective, None, direction)
    assert val.shape == (B,) and grad.shape == x.shape and grad.dtype == torch.float32
    value_fn = lambda out: _oracle_value(out, objective, y, direction)
    f_hip = m(x.to(dev()).requires_grad_(True))['features'].detach().cpu()          # the forward that keeps its activations, as the call's
    # the backbone's gradient on the same seed: the oracle's heads at the HIP features (no unit can flip)
    want, f_ref = tig._oracle_image_grad(x, sd64, lambda f: tig._head_seed(sd64, f_hip, value_fn))
    wc, wr = tig._check_images(grad, want)
    out_hip = ref_cpu.heads_forward(f_hip.double(), sd64, 4)
    out_hip['kan_severity'] = ref_cpu.kan_module_forward(f_hip.double(), sd64, 'kan_module.')
    verr = float((val.cpu().double() - value_fn(out_hip)).abs().max())
    print(f'{objective} {direction:+d} B {B}: cosine >= {wc:.6f}, max-abs / max <= {wr:.3e}, value error {verr:.2e}')
    assert verr <= VALUE_TOL
    if is_class:          # end to end for the class objectives; an image whose hidden unit flips is held to COS_FLIP
        want_e2e, _ = tig._oracle_image_grad(x, sd64, lambda f: tig._head_seed(sd64, f, value_fn))
        flipped = (tig._hidden_signs(sd64, f_hip) != tig._hidden_signs(sd64, f_ref)).any(dim=1)
        wc, wr = tig._check_images(grad, want_e2e, flipped)
        print(f'  end to end: {int(flipped.sum())} of {B} flipped; others cosine >= {wc:.6f}, <= {wr:.3e}')
    # labels=None is the model's own prediction; a target makes it targeted
    if objective == 'ce':
        pred = m.predict(x.to(dev()))['class']
        v0, g0 = A.objective_gradient(m, x.to(dev()), None, 'ce')
        v1, g1 = A.objective_gradient(m, x.to(dev()), pred, 'ce')
        assert torch.equal(v0, v1) and torch.equal(g0, g1)
        vt, gt = A.objective_gradient(m, x.to(dev()), None, 'ce', target_class=y.to(dev()))
        assert torch.equal(vt, -val) and float((gt + grad).abs().max() / grad.abs().max()) <= 2.0 ** -8          # not to the bit: log p and -log p round apart before the chain's bf16


# ---- 5. FGSM ------------------------------------------------------------------------------------------------------------------------

def test_one_step_attack_is_the_reference_step_on_the_objective_gradient():
    m, _ = tig._model(2, seed=40)
    x = _box_images(3, 41).to(dev())
    y = torch.tensor([0, 1, 2], device=dev())
    eps = 4 / 255
    val, grad = A.objective_gradient(m, x, y, 'ce')
    x_adv, info = A.pgd_attack(m, x, y, objective='ce', norm='linf', eps=eps, steps=1, step_size=eps, random_start=False, clip=None,
                               return_info=True)
    want_d, want_xa = A.step_reference(x, grad, torch.zeros_like(x), eps, eps, 'linf', clip=None, dtype=np.float32)
    # the best of {clean, stepped} by objective value is what comes back; the stepped image's value decides which
    stepped = A.objective_gradient(m, torch.from_numpy(want_xa).to(dev()), y, 'ce')[0]
    keep = (stepped > val).cpu().numpy()
    assert keep.any()
    for b in range(3):
        assert ac.same_bits(x_adv[b].cpu().numpy(), want_xa[b] if keep[b] else x[b].cpu().numpy())
        assert ac.same_bits(info['delta'][b].cpu().numpy(), want_d[b] if keep[b] else np.zeros_like(want_d[b]))
    assert torch.equal(info['value_clean'], val) and torch.equal(info['value'], torch.maximum(val, stepped))


# ---- 6. invariants of pgd_attack ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('random_start', [False, True], ids=['clean_start', 'random_start'])
@pytest.mark.parametrize('norm,eps', [('linf', 4 / 255), ('l2', 1.0)])
def test_pgd_attack_invariants(norm, eps, random_start):
    m, _ = tig._model(2, seed=42)
    x = _box_images(3, 43).to(dev())
    y = m.predict(x)['class']
    flags = [p.requires_grad for p in m.parameters()]
    kw = dict(objective='margin', norm=norm, eps=eps, steps=4, random_start=random_start, seed=9, return_info=True)
    x_adv, info = m.adversarial_examples(x, y, **kw)
    d = info['delta'].cpu().numpy()
    inv_s, _, lo, hi = A.constants()
    if norm == 'linf':
        assert (np.abs(d) <= (np.float32(eps) * inv_s).reshape(1, 3, 1, 1)).all()
    else:
        assert (ac.pixel_norm(d) <= eps * (1 + 2.0 ** -20)).all()
    xa = x_adv.cpu().numpy()
    assert (xa >= lo.reshape(1, 3, 1, 1)).all() and (xa <= hi.reshape(1, 3, 1, 1)).all()
    print(f'{norm} random_start {random_start}: value {info["value_clean"].tolist()} -> {info["value"].tolist()}, success {info["success"].tolist()}')
    if not random_start:
        assert bool((info['value'] >= info['value_clean']).all())
    pred = m.predict(x_adv)['class']
    assert torch.equal(info['success'], pred != y) and torch.equal(info['outputs']['cls_logits'].argmax(1), pred)
    x_adv2, info2 = m.adversarial_examples(x, y, **kw)
    assert torch.equal(x_adv, x_adv2) and torch.equal(info['delta'], info2['delta']) and torch.equal(info['value'], info2['value'])
    assert [p.requires_grad for p in m.parameters()] == flags and all(p.grad is None for p in m.parameters())


def test_pgd_attack_between_a_training_forward_and_its_backward():
    m, _ = tig._model(2, seed=44)
    x = _box_images(3, 45).to(dev())
    gx0, g0 = tig._run(m, x, tig._joint)
    xg = x.clone().requires_grad_(True)
    out = m(xg)
    eng = m.backbone.model.engine
    last = eng.last_ws
    x_adv = m.adversarial_examples(x, norm='l2', eps=0.5, steps=2)
    assert eng.last_ws is last and all(p.grad is None for p in m.parameters())
    tig._joint(out).backward()
    assert torch.equal(xg.grad, gx0)
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, g0[n]), n
    assert torch.isfinite(x_adv).all()
    m.zero_grad(set_to_none=True)


# ---- 7. severity --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('direction', [1, -1])
def test_severity_attack_moves_mu_its_way(direction):
    m, _ = tig._model(2, seed=46)
    x = _box_images(3, 47).to(dev())
    x_adv, info = m.adversarial_examples(x, objective='mu', direction=direction, eps=4 / 255, steps=4, random_start=False, return_info=True)
    with torch.no_grad():
        before, after = m(x)['mu'][:, 0], m(x_adv)['mu'][:, 0]
    print(f'mu {direction:+d}: {before.tolist()} -> {after.tolist()}')
    assert bool((direction * (after - before) >= 0).all())
    assert torch.equal(info['outputs']['mu'][:, 0], after) and 'success' not in info


# ---- 8. the radius ------------------------------------------------------------------------------------------------------------------

def test_robustness_radius():
    m, _ = tig._model(2, seed=48)
    x = _box_images(4, 49).to(dev())
    with torch.no_grad():
        logits = m(x)['cls_logits']
    y = logits.argmax(1)
    y[3] = (y[3] + 1) % 4                                  # a wrong label: radius 0
    # eps_max: four times the largest first-order estimate of the radius, clean margin / sum_e |d margin / d pixel_e|, so that the attack
    # at eps_max should break every correctly labelled image and the halvings have something to find on both sides
    yc = logits.argmax(1)
    val, grad = A.objective_gradient(m, x, yc, 'margin')                                   # val = -(clean margin) < 0
    l1 = (grad.abs() * torch.from_numpy(A.constants()[0]).to(dev()).view(1, 3, 1, 1)).flatten(1).sum(1)
    estimate = (-val) / l1
    eps_max = 4.0 * float(estimate.max())
    print(f'first-order radius estimates {(estimate * 255).tolist()} / 255, eps_max {eps_max * 255:.4f} / 255')
    res = m.robustness_radius(x, y, 'linf', eps_max, 3, 2)
    radius, lower, broken = res['radius'].cpu(), res['lower'].cpu(), res['broken'].cpu()
    print(f'radius {(radius * 255).tolist()} / 255, lower {(lower * 255).tolist()} / 255, broken {broken.tolist()}')
    assert radius[3] == 0 and not broken[3] and torch.equal(res['x_adv'][3], x[3])
    pred = m.predict(res['x_adv'])['class'].cpu()
    inv_s = torch.from_numpy(A.constants()[0]).view(3, 1, 1)
    for b in range(3):
        if broken[b]:
            assert pred[b] != y[b].cpu() and 0 <= lower[b] <= radius[b] <= np.float32(eps_max)
            assert bool(((res['x_adv'][b] - x[b]).cpu().abs() <= radius[b] * inv_s + 2.0 ** -23 * x[b].cpu().abs().clamp_min(1)).all())
        else:
            assert torch.isinf(radius[b]) and torch.equal(res['x_adv'][b], x[b])
    assert bool(broken[:3].any())          # eps_max was chosen large enough for this model to break at least one image
    # an eps_max at which nothing can break.  How it is chosen: to first order the margin z_y - max_other moves by at most
    # eps * sum_e |d margin / d pixel_e| under an L-infinity change of eps (the estimate above); a hundredth of the smallest estimate
    # leaves a factor of 100 for the curvature
    tiny = float(estimate.min()) / 100.0
    assert tiny > 0
    res = m.robustness_radius(x, yc, 'linf', tiny, 3, 2)
    assert bool(torch.isinf(res['radius']).all()) and not bool(res['broken'].any()) and torch.equal(res['x_adv'], x)
    assert torch.equal(res['lower'].cpu(), torch.full((4,), np.float32(tiny)))


# ---- 9. the score card --------------------------------------------------------------------------------------------------------------

def test_evaluate_adversarial(tmp_path):
    from evaluation.evaluator import Evaluator
    m, _ = tig._model(2, seed=50)
    x = _box_images(7, 51)
    labels = torch.arange(7) % 4
    loader = [(x[0:3], labels[0:3], labels[0:3]), (x[3:6], labels[3:6], labels[3:6]), (x[6:7], labels[6:7], labels[6:7])]
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=CLASS_NAMES, num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    ev = Evaluator(m, loader, cfg, dev())
    result = ev.evaluate_adversarial(eps=(0.0, 8 / 255), steps=2, severity_targets=('ordinal_severity', 'mu'), seed=3)
    assert result['eps'] == [0.0, 8 / 255] and len(result['cells']) == 2 and result['norm'] == 'linf' and result['objective'] == 'ce'
    clean, zero, cell = result['clean'], result['cells'][0], result['cells'][1]
    for card in (zero, cell):
        assert {'accuracy', 'macro_f1', 'mae', 'brier_score', 'ece', 'n', 'correct', 'mean_confidence', 'mean_sigma', 'flip_rate', 'severity',
                'eps'} <= set(card)
        assert card['n'] == 7 and set(card['severity']) == {'ordinal_severity', 'mu'}
        for moves in card['severity'].values():
            assert set(moves) == {'mean_up', 'max_up', 'mean_down', 'max_down'} and moves['max_up'] >= moves['mean_up']
    assert 'severity' not in clean and clean['flip_rate'] == 0
    assert zero['accuracy'] == clean['accuracy'] and zero['correct'] == clean['correct'] and zero['flip_rate'] == 0
    assert all(v == 0 for moves in zero['severity'].values() for v in moves.values())
    print(f"flip rates {[c['flip_rate'] for c in result['cells']]} (not asserted to grow: PGD is not monotone), "
          f"accuracy {[c['accuracy'] for c in result['cells']]}, moves {cell['severity']}")
    text = (tmp_path / 'adversarial_results.txt').read_text()
    assert 'Adversarial robustness' in text and text.count('\n') >= 6 and (tmp_path / 'adversarial_results.json').exists()
    import json
    assert json.loads((tmp_path / 'adversarial_results.json').read_text())['cells'][1]['eps'] == 8 / 255
