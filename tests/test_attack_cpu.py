"""CPU tests of the attack references (rovit_hip/attack.py: ``step_reference`` / ``init_reference``, the oracles of
tests/test_gpu_attack.py), of the ``PGD`` loop on CPU tensors (where it runs those references) and of the argument checks of
``pgd_attack``, ``robustness_radius`` and ``Evaluator.evaluate_adversarial``, which come before the check for a GPU."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attack_cases as ac  # noqa: E402
from oracle.philox import philox4x32_10  # noqa: E402  (checker only)
from rovit_hip import RovitHipError, native  # noqa: E402
from rovit_hip import attack as A  # noqa: E402

SMALL = [s for s in ac.SHAPES if s != (224, 224)]


def _box(case):
    _, _, lo, hi = A.constants(ac.MEAN, ac.STD, case['clip'])
    return lo.reshape(1, 3, 1, 1), hi.reshape(1, 3, 1, 1)


@pytest.mark.parametrize('clip', [(0., 1.), None], ids=['box', 'nobox'])
@pytest.mark.parametrize('norm', ['linf', 'l2'])
@pytest.mark.parametrize('shape', SMALL, ids=ac.shape_id)
def test_step_reference_invariants_in_fp32_and_fp64(shape, norm, clip):
    case = ac.build(shape, 5, clip, dead_image=norm == 'l2')
    lo, hi = _box(case)
    start = case['delta'] if norm == 'linf' else case['delta_l2']
    out = {}
    for T in (np.float32, np.float64):
        d, xa = A.step_reference(case['x'], case['g'], start, case['eps'], case['alpha'], norm, ac.MEAN, ac.STD, clip, T)
        assert d.dtype == T and xa.dtype == T and np.isfinite(d).all() and np.isfinite(xa).all()
        assert (xa >= lo.astype(T)).all() and (xa <= hi.astype(T)).all()                    # the box, exactly
        if norm == 'linf':
            assert (np.abs(d) <= case['r'].astype(T)).all()                                 # the ball, exactly
        else:
            assert (ac.pixel_norm(d) <= ac.l2_norm_bound(case['eps'], d[0].size)).all()
        zero = case['eps'] == 0
        assert (d[zero] == 0).all()
        if clip is not None:
            assert (xa[zero] == case['x'][zero].astype(T)).all()                            # eps == 0: x_adv == x inside the box
        out[T] = d
    # the two precisions state the same step.  A sanity bound, not a kernel bound: the fp32 statement rounds up to a dozen times, the
    # L-infinity chain at the size of x (x + d2 and y - x), so the scale is |x| + r, not r
    scale = np.abs(case['x']) + case['r'] + np.abs(out[np.float64])
    assert (np.abs(out[np.float32] - out[np.float64]) <= 32 * 2.0 ** -24 * scale + 2.0 ** -149).all()
    if norm == 'l2' and clip is None:           # a zero / NaN gradient does not move its image (the last one, which starts inside its ball)
        b = case['x'].shape[0] - 1
        assert ac.pixel_norm(start)[b] < case['eps'][b]
        for T in out:
            assert (out[T][b] == start[b].astype(T)).all()


def test_linf_step_hits_the_ball_edge_cases():
    """The builder's landings are what they claim (fl32(delta + sg a) is +-r, one ulp inside, one ulp outside), and the step brings each
    back inside the ball, up to the documented rounding of x + delta in the later operations."""
    case = ac.build((16, 16), 5, None)
    d, _ = A.step_reference(case['x'], case['g'], case['delta'], case['eps'], case['alpha'], 'linf', ac.MEAN, ac.STD, None, np.float32)
    flat = lambda v: np.broadcast_to(v, d.shape).reshape(5, -1)
    df, rf, af, xf, old, gf = d.reshape(5, -1), flat(case['r']), flat(case['a']), flat(case['x']), flat(case['delta']), flat(case['g'])
    for b in (0, 3, 4):                                   # the rows with a normal radius larger than the step
        for k in range(6):
            p, sign = 17 * k + 1, np.float32(1.0 if k < 3 else -1.0)
            edge = rf[b, p]
            landed = [edge, np.nextafter(edge, np.float32(0.0)), np.nextafter(edge, np.float32(np.inf))][k % 3]
            assert np.sign(gf[b, p]) == sign and np.float32(old[b, p] + sign * af[b, p]) == sign * landed, (b, k)
            assert abs(df[b, p]) <= edge and abs(abs(df[b, p]) - min(landed, edge)) <= 2.0 ** -23 * (abs(xf[b, p]) + edge), (b, k)
    for k in range(3):                                    # +0, -0 and NaN gradients: no step, only the projection
        p = 7 * k + 3
        assert not (gf[:, p] > 0).any() and not (gf[:, p] < 0).any()
        assert (np.abs(df[:, p] - np.clip(old[:, p], -rf[:, p], rf[:, p])) <= 2.0 ** -23 * (np.abs(xf[:, p]) + rf[:, p])).all()


def test_init_reference_draws_the_documented_words():
    assert native.ATTACK_STREAM == int.from_bytes(b'Adav', 'big') == 0x41646176
    seed, restart, ids = (7 << 32) | 12345, 2, [3, 1 << 33 | 5]
    x = np.zeros((2, 3, 1, 5), np.float32)
    words = A.attack_words(ids, 15, seed, restart)
    for row, i in enumerate(ids):
        for e in range(15):
            w = philox4x32_10([e // 4, i & 0xFFFFFFFF, native.ATTACK_STREAM, restart], [seed & 0xFFFFFFFF, seed >> 32])
            assert int(words[row, e]) == int(w[e % 4])
    eps = np.array([4 / 255, 8 / 255], np.float32)
    d, xa = A.init_reference(x, ids, eps, 'linf', seed, restart, ac.MEAN, ac.STD, None, np.float32)
    inv_s = (1.0 / np.array(ac.STD)).astype(np.float32)
    u = (words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    want = ((np.float32(2) * u - np.float32(1)).reshape(2, 3, 1, 5) * (eps.reshape(2, 1, 1, 1) * inv_s.reshape(1, 3, 1, 1)))
    assert ac.same_bits(d, want) and ac.same_bits(xa, want)                               # x = 0, no box: x_adv = delta
    # L2: the documented pairing, and the norm
    d2, _ = A.init_reference(x, ids, eps, 'l2', seed, restart, ac.MEAN, ac.STD, None, np.float64)
    calls = A.attack_calls(ids, 15, seed, restart)
    for row in range(2):
        z = np.empty(15)
        for e in range(15):
            wa, wb = (calls[0], calls[1]) if e % 4 < 2 else (calls[2], calls[3])
            rad = np.sqrt(-2 * np.log(((int(wa[row, e]) >> 8) + 1) / 2 ** 24))
            ang = 2 * np.pi * (int(wb[row, e]) >> 8) / 2 ** 24
            z[e] = np.float32(rad * (np.sin(ang) if e % 2 else np.cos(ang)))
        u_want = eps[row].astype(np.float64) * z / np.sqrt((z ** 2).sum())
        got = (d2[row] * np.array(ac.STD, np.float32).astype(np.float64).reshape(3, 1, 1)).reshape(-1)
        assert np.abs(got - u_want).max() <= 2.0 ** -22 * eps[row]          # s_c inv_s_c is 1 only up to their fp32 roundings
    assert np.abs(ac.pixel_norm(d2) / eps - 1).max() <= 1e-9
    assert not ac.same_bits(d, A.init_reference(x, ids, eps, 'linf', seed, restart + 1, ac.MEAN, ac.STD, None, np.float32)[0])
    assert (A.init_reference(x, ids, [0.0, 0.0], 'l2', seed, restart, ac.MEAN, ac.STD, None)[0] == 0).all()


@pytest.mark.parametrize('norm', ['linf', 'l2'])
def test_init_reference_does_not_depend_on_the_split(norm):
    case = ac.build((3, 85), 5)
    ids = np.array([3, 9, 4, 1, 7])
    whole = A.init_reference(case['x'], ids, case['eps'], norm, 5, 1, ac.MEAN, ac.STD, case['clip'])
    parts = [A.init_reference(case['x'][sl], ids[sl], case['eps'][sl], norm, 5, 1, ac.MEAN, ac.STD, case['clip']) for sl in (slice(0, 2), slice(2, 5))]
    for i in range(2):
        assert ac.same_bits(whole[i], np.concatenate([p[i] for p in parts]))
    back = A.init_reference(case['x'][::-1], ids[::-1], case['eps'][::-1], norm, 5, 1, ac.MEAN, ac.STD, case['clip'])
    assert ac.same_bits(whole[0], back[0][::-1])


# ---- the loop on CPU tensors --------------------------------------------------------------------------------------------------------

def _linear(w):
    return lambda xa: ((xa * w).flatten(1).sum(1), w.expand_as(xa).contiguous())


def test_pgd_linf_on_a_linear_objective_ends_on_the_corner():
    g = torch.Generator().manual_seed(1)
    w = torch.randn(1, 3, 5, 7, generator=g)
    eps = torch.tensor([4 / 255, 1 / 255])
    inv_s = torch.from_numpy((1.0 / np.array(ac.STD)).astype(np.float32)).view(1, 3, 1, 1)
    want = torch.sign(w) * (eps.view(2, 1, 1, 1) * inv_s)                                 # eps sign(w) / std_c
    # x = 0: x + delta and y - x round nothing, so the end point is the corner to the bit
    x = torch.zeros(2, 3, 5, 7)
    res = A.PGD('linf', eps, steps=4, step_size=eps * 0.3, random_start=False, mean=ac.MEAN, std=ac.STD, clip=None)(_linear(w), x)
    assert torch.equal(res['delta'], want) and torch.equal(res['x_adv'], want)
    assert torch.equal(res['value'], (want * w).flatten(1).sum(1))
    # a random start changes nothing about the end point
    res = A.PGD('linf', eps, steps=8, step_size=eps * 0.3, random_start=True, seed=3, mean=ac.MEAN, std=ac.STD, clip=None)(_linear(w), x)
    assert torch.equal(res['delta'], want)
    # any x: the corner up to the documented rounding of x + delta, never outside the ball
    x = torch.randn(2, 3, 5, 7, generator=g)
    res = A.PGD('linf', eps, steps=4, step_size=eps * 0.3, random_start=False, mean=ac.MEAN, std=ac.STD, clip=None)(_linear(w), x)
    assert bool((res['delta'].abs() <= want.abs()).all())
    assert bool(((res['delta'] - want).abs() <= 2.0 ** -23 * (x.abs() + want.abs())).all())
    assert torch.equal(res['x_adv'], x + res['delta'])


def test_pgd_l2_on_a_linear_objective_ends_on_the_sphere():
    g = torch.Generator().manual_seed(2)
    w = torch.randn(1, 3, 5, 7, generator=g)
    x = torch.randn(2, 3, 5, 7, generator=g)
    eps = torch.tensor([0.5, 0.125])
    res = A.PGD('l2', eps, steps=4, step_size=eps * 0.3, random_start=False, mean=ac.MEAN, std=ac.STD, clip=None)(_linear(w), x)
    inv_s = (1.0 / np.array(ac.STD)).astype(np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    gh = w.numpy().astype(np.float64) * inv_s                                             # the gradient in pixel units
    want = eps.numpy().astype(np.float64).reshape(2, 1, 1, 1) * gh / np.sqrt((gh ** 2).sum()) * inv_s
    r = eps.numpy().reshape(2, 1, 1, 1) * inv_s
    err = np.abs(res['delta'].numpy().astype(np.float64) - want)
    # the L2 tolerance of one step holds for the four: each step rounds delta to fp32 once (2^-24 relative), and they add up to less than 8
    assert (err <= ac.L2_FACTOR * np.maximum(r, np.abs(want))).all(), float((err / np.maximum(r, np.abs(want))).max())
    assert (ac.pixel_norm(res['delta'].numpy()) <= eps.numpy().astype(np.float64) * (1 + 2.0 ** -20)).all()


def test_pgd_keeps_the_best_iterate_not_the_last():
    """f = -|x_adv - c|^2 with c next to x and a step far longer than |c - x|: the iterates are x, x + a s, x, x + a s (s = sign(c - x));
    the clean image has the highest value, the later visit ties with it (a tie keeps the earlier), and the last iterate is the far one."""
    x = torch.zeros(2, 3, 4, 4)
    c = x + 0.01

    def f(xa):
        return -((xa - c) ** 2).flatten(1).sum(1), -2 * (xa - c)
    res = A.PGD('linf', 0.5, steps=3, step_size=0.2, random_start=False, mean=ac.MEAN, std=ac.STD, clip=None)(f, x)
    assert torch.equal(res['delta'], torch.zeros_like(x)) and torch.equal(res['x_adv'], x)
    assert torch.equal(res['value'], f(x)[0])
    seen = []
    A.PGD('linf', 0.5, steps=3, step_size=0.2, random_start=False, mean=ac.MEAN, std=ac.STD, clip=None)(
        lambda xa: (seen.append(xa.clone()), f(xa))[1], x)
    assert len(seen) == 4 and not torch.equal(seen[-1], x) and torch.equal(seen[2], x)    # K gradient calls + one value call
    # NaN never improves
    res = A.PGD('linf', 0.5, steps=2, step_size=0.2, random_start=False, clip=None)(lambda xa: (torch.full((2,), float('nan')), torch.ones_like(xa)), x)
    assert torch.equal(res['delta'], torch.zeros_like(x)) and bool(torch.isinf(res['value']).all())


@pytest.mark.parametrize('norm', ['linf', 'l2'])
def test_restarts_never_lower_the_value(norm):
    g = torch.Generator().manual_seed(4)
    x = torch.rand(3, 3, 6, 6, generator=g)
    x = (x - torch.tensor(ac.MEAN).view(1, 3, 1, 1)) / torch.tensor(ac.STD).view(1, 3, 1, 1)
    c = 0.3 * torch.randn(1, 3, 6, 6, generator=g)

    def f(xa):                                            # many local maxima: the start matters
        t = 9.0 * (xa - c)
        return torch.sin(t).flatten(1).sum(1), 9.0 * torch.cos(t)
    eps = 0.1 if norm == 'linf' else 1.0
    values = [A.PGD(norm, eps, steps=3, random_start=True, restarts=k, seed=5)(f, x)['value'] for k in (1, 2, 4)]
    assert bool((values[1] >= values[0]).all()) and bool((values[2] >= values[1]).all())
    ids = torch.tensor([7, 8, 9])
    a = A.PGD(norm, eps, steps=3, seed=5)(f, x, ids)
    b = A.PGD(norm, eps, steps=3, seed=5)(f, x[1:], ids[1:])
    assert torch.equal(a['delta'][1:], b['delta'])        # a start belongs to (seed, id), not to the batch


# ---- arguments ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def cpu_model():
    from models.rovit_kan import RoViTKAN
    return RoViTKAN(pretrained=False).eval()


BAD_ATTACK = [{'norm': 'l1'}, {'eps': -1.0}, {'eps': float('nan')}, {'eps': 'big'}, {'eps': torch.ones(3)}, {'steps': 0}, {'steps': 2.5},
              {'step_size': -0.1}, {'step_size': torch.ones(2, 2)}, {'restarts': 0}, {'seed': -1}, {'random_start': 1}, {'clip': (1., 0.)},
              {'clip': 3}, {'std': (0.2, 0.2, 0.0)}, {'mean': (0.5, 0.5)}, {'ids': torch.zeros(2)}, {'ids': torch.zeros(3, dtype=torch.long)},
              {'chunk': 0}]
BAD_OBJECTIVE = [{'objective': 'class'}, {'objective': 'sev'}, {'direction': 0}, {'direction': -1}, {'objective': 'mu', 'direction': 2},
                 {'objective': 'mu', 'target_class': 1}, {'target_class': 4}, {'target_class': torch.tensor([0, 9])},
                 {'target_class': torch.tensor([0.0, 1.0])}]


def test_pgd_attack_refuses_bad_arguments_before_the_gpu_check(cpu_model):
    x = torch.zeros(2, 3, 224, 224)
    for kw in BAD_ATTACK + BAD_OBJECTIVE:
        with pytest.raises(RovitHipError) as err:
            cpu_model.adversarial_examples(x, **kw)
        assert 'on the GPU' not in str(err.value), kw
    for labels in (4, -1, torch.tensor([0, 1, 2]), torch.tensor([0.5, 1.0]), 'a'):
        with pytest.raises(RovitHipError) as err:
            cpu_model.adversarial_examples(x, labels)
        assert 'on the GPU' not in str(err.value), labels
    for bad in (torch.zeros(2, 3, 32, 32), torch.zeros(0, 3, 224, 224), torch.zeros(2, 3, 224, 224, dtype=torch.long), 'x'):
        with pytest.raises(RovitHipError) as err:
            cpu_model.adversarial_examples(bad)
        assert 'on the GPU' not in str(err.value)
    cpu_model.curriculum_stage = 2
    try:
        with pytest.raises(RovitHipError, match='curriculum stage'):
            cpu_model.adversarial_examples(x, objective='kan_severity')
    finally:
        cpu_model.curriculum_stage = 4
    with pytest.raises(RovitHipError, match='on the GPU'):      # every argument good: only now the device is looked at
        cpu_model.adversarial_examples(x, torch.tensor([0, 1]), objective='margin', norm='l2', eps=0.5, steps=2)
    with pytest.raises(RovitHipError, match='on the GPU'):
        A.objective_gradient(cpu_model, x, objective='mu', direction=-1)


def test_robustness_radius_refuses_bad_arguments_before_the_gpu_check(cpu_model):
    x, y = torch.zeros(2, 3, 224, 224), torch.tensor([0, 1])
    for kw in ({'eps_max': 0.0}, {'eps_max': float('inf')}, {'eps_max': torch.ones(2)}, {'search_steps': -1}, {'search_steps': 1.5},
               {'objective': 'mu'}, {'norm': 'l0'}, {'steps': 0}, {'restarts': 0}, {'clip': (2., 1.)}, {'chunk': 0}):
        with pytest.raises(RovitHipError) as err:
            cpu_model.robustness_radius(x, y, **kw)
        assert 'on the GPU' not in str(err.value), kw
    for labels in (None, 7, torch.tensor([0, 5]), torch.tensor([0])):
        with pytest.raises(RovitHipError) as err:
            cpu_model.robustness_radius(x, labels)
        assert 'on the GPU' not in str(err.value), labels
    with pytest.raises(RovitHipError, match='on the GPU'):
        cpu_model.robustness_radius(x, y, 'l2', 0.5, 2, 2)


def test_evaluate_adversarial_refuses_bad_arguments_before_the_gpu_check(cpu_model, tmp_path):
    from evaluation.evaluator import Evaluator
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=['a', 'b', 'c', 'd'], num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    batch = (torch.zeros(2, 3, 224, 224), torch.tensor([0, 1]), torch.tensor([0, 1]))
    ev = Evaluator(cpu_model, [batch], cfg, 'cpu')
    for kw in ({'eps': ()}, {'eps': 0.1}, {'eps': (-1.0,)}, {'eps': (torch.ones(2),)}, {'norm': 'l1'}, {'steps': 0}, {'objective': 'mu'},
               {'severity_targets': ('class',)}, {'severity_targets': 'mu'}, {'severity_targets': ('sev',)}, {'seed': -1},
               {'source': iter([batch])}):
        with pytest.raises(RovitHipError) as err:
            ev.evaluate_adversarial(**kw)
        assert 'on the GPU' not in str(err.value), kw
    with pytest.raises(RovitHipError):
        Evaluator(cpu_model, None, cfg, 'cpu').evaluate_adversarial()
    assert not list(tmp_path.iterdir())
