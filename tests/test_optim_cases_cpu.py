"""Everything about tests/optim_cases.py that needs no GPU: the fp32 restatement of the optimizer kernels inside R's bounds on every case (a
bound that plain fp32 arithmetic cannot meet fails here, before a GPU sees it), the exact norm cases (exact in fp32, and sensitive to one
element through the square root), and the presence of every position class, computed from the constants read out of csrc/optim.hip."""
import math
import os
import re

import numpy as np
import pytest

import optim_cases as oc
from conftest import PKG

SRC = open(os.path.join(PKG, 'csrc', 'optim.hip')).read()


def _const(name):
    m = re.search(rf'constexpr int {name} = (\d+);', SRC)
    assert m, name
    return int(m.group(1))


def test_the_restated_constants_are_those_of_the_kernels():
    assert _const('ADAM_PIECE4') == oc.ADAM_PIECE4 and _const('NORM_PIECE4') == oc.NORM_PIECE4
    assert _const('NORM_THREADS') == oc.NORM_THREADS and _const('NORM_MAX_BLOCKS') == oc.NORM_MAX_BLOCKS
    caps = [int(a) for a, b in re.findall(r'blocks > (\d+) \? (\d+) : blocks', SRC) if a == b]
    assert caps == [oc.ACCUM_MAX_BLOCKS, oc.FLAT_MAX_BLOCKS]           # rovit_sq_norm_accum, then rovit_adamw_flat, in file order
    assert SRC.count('(n / 4 + 255) / 256') == 2                       # 256 float4 a block, as accum_layout and adam_classes('flat') restate
    assert 'norm != norm ? norm : fminf(1.f, max_norm / (norm + 1e-6f))' in SRC and SRC.count('clip_coefficient(n, max_norm)') == 2


# ---- the norm kernels --------------------------------------------------------------------------------------------------------------------

CLIP = {c.name: c for c in oc.clip_small_cases()}
CLIP.update({c.name: c for c in oc.clip_coef_cases()})


def _emulated_clip(bufs, max_norm):
    return oc.emulate_clip(bufs, max_norm)[1:]


def test_clip_restatement_is_within_the_bounds_and_exact_where_the_case_says_so():
    rec = {}
    for case in oc.clip_cases():
        oc.judge_clip(case, _emulated_clip, rec)
        if case.exact:
            sq = oc.sq_truth(case.bufs)
            got = float(oc.emulate_clip(case.bufs, case.max_norm)[0])
            assert got == sq or (math.isnan(got) and math.isnan(sq)), (case.name, got, sq)
    print(rec)
    assert rec['norm'][0] <= 1 and rec['coef'][0] <= 1, rec


def test_required_outcomes_of_the_coefficient():
    t = {n: oc.clip_truth(c) for n, c in CLIP.items()}
    assert t['norm_zero'][:2] == ((0.0, 0.0), (1.0, 0.0)) and t['norm_far_below_max'][1] == (1.0, 0.0)
    assert t['sum_overflows'][:2] == ((math.inf, 0.0), (0.0, 0.0))
    for n in ('nan_first', 'nan_last'):
        assert math.isnan(t[n][0][0]) and math.isnan(t[n][1][0])
        _, norm, coef = oc.emulate_clip(CLIP[n].bufs, 1.0)
        assert np.isnan(norm) and np.isnan(coef)
    assert t['norm_equals_max'][1][0] < 1 and t['norm_just_above_max'][1][0] < t['norm_equals_max'][1][0] < t['norm_just_below_max'][1][0] < 1
    for n in ('norm_equals_max', 'norm_just_above_max', 'norm_just_below_max'):
        assert 0 < t[n][1][1] < 1e-6                                   # a bound, not an exact value: 5 + 1e-6 is rounded


def test_every_exact_norm_case_shows_one_lost_or_repeated_element_through_the_square_root():
    n = 0
    for case in oc.clip_cases():
        sq = oc.sq_truth(case.bufs)
        if not case.exact or not math.isfinite(sq) or sq == 0 or case.name.startswith('norm_'):
            continue
        allowance, move = oc.clip_sensitivity(case)
        assert move > 2 * allowance, (case.name, move, allowance)
        assert sq < 2 ** 24 and sq == int(sq)
        if case.probes:                                                # disjoint base-4 digits: the sum names its probes
            assert sq == sum(4 ** j for j in range(len(case.probes)))
        n += 1
    assert n >= 30


def test_clip_cases_sit_on_every_edge_the_walk_has():
    P4, MAXB = _const('NORM_PIECE4'), _const('NORM_MAX_BLOCKS')
    piece = 4 * P4
    cases = list(oc.clip_small_cases()) + list(oc.clip_coef_cases())
    classes = set().union(*(c.classes for c in cases))
    want = {f'single{n}' for n in (4, piece - 4, piece, piece + 4)} | {'bufs2', 'bufs3', 'bufs4', 'zero_first', 'zero_middle', 'zero_last',
            'norm_equals_max', 'norm_just_above_max', 'norm_just_below_max', 'norm_zero', 'overflow', 'nan', 'random', 'coef_one'}
    assert want <= classes, want - classes
    for c in cases:
        if c.name.startswith('bufs'):                                  # every buffer's last piece is partly full
            assert all(b.size % piece for b in c.bufs), c.name
        if c.name.startswith('bufs') and c.probes:
            at = {(k, i) for k, i, _, _ in c.probes}
            for q in range(len(c.bufs) - 1):
                assert (q, c.bufs[q].size - 1) in at and (q + 1, 0) in at, c.name
    for name, pos in (('zero_first', 0), ('zero_middle', 1), ('zero_last', 2)):
        assert [b.size == 0 for b in CLIP[name + '_dense'].bufs] == [i == pos for i in range(3)]
    by_total = {}
    for c in oc.clip_piece_cases():
        n = c.bufs[0].size
        P = -(-(n // 4) // P4)
        grid = min(P, MAXB)
        by_total.setdefault(P, set()).add(c.name.split('_')[1])
        cnt = [(b + 1) * P // grid - b * P // grid for b in range(grid)]
        blocks = (0, grid - 1) if c.name.endswith('ends') else (cnt.index(max(cnt)), cnt.index(min(cnt)))
        at = {i for _, i, _, _ in c.probes}
        for b in blocks:
            p0, p1 = b * P // grid, (b + 1) * P // grid
            for pc in (p0, p1 - 1):
                assert pc * piece in at and min((pc + 1) * piece, n) - 1 in at, (c.name, b, pc)
        if P > MAXB:
            assert max(cnt) >= 2 and (P < 2 * MAXB or max(cnt) == 3 or P == 2 * MAXB - 1)
    assert by_total == {P: {'ends', 'mid'} for P in (1, 2, MAXB - 1, MAXB, MAXB + 1, 2 * MAXB - 1, 2 * MAXB + 1)}
    assert max(c.bufs[0].size for c in oc.clip_piece_cases()) == (2 * MAXB + 1) * piece      # the largest case: about 8.4 M floats


def test_accum_restatement_is_exact_on_the_exact_cases_and_within_the_bound_elsewhere():
    cap = oc.ACCUM_MAX_BLOCKS * 1024
    assert set(oc.ACCUM_SIZES) == {1, 3, 4, 5, 1023, 1024, 1025, cap - 4, cap, cap + 5}
    assert oc.accum_layout(cap)[1:] == (oc.ACCUM_MAX_BLOCKS, 1) and oc.accum_layout(cap + 5)[1:] == (oc.ACCUM_MAX_BLOCKS, 2)
    rec = {}

    def run(bufs, scratch):
        out = np.float32(0)
        for b in bufs:
            out = oc.emulate_accum(b, out, scratch)
        return out
    names = set()
    for case in oc.accum_cases():
        names.add(case.name)
        for scratch in (True, False):
            oc.judge_accum(case, run, rec, scratch)
            if case.exact:
                sq = oc.accum_truth(case, scratch)[0]
                assert float(run(case.bufs, scratch)) == sq and sq < 2 ** 24, case.name
                # one element less, or the tail started one late, is another integer: bit equality sees it
                assert float(run([case.bufs[0][:-1]] + case.bufs[1:], scratch)) != sq or case.bufs[0][-1] == 0, case.name
    print(rec)
    assert rec['sq'][0] <= 1 and rec['sq_atomic'][0] <= 1, rec
    assert {'three_buffers_dense', 'three_buffers_random'} <= names


# ---- AdamW -----------------------------------------------------------------------------------------------------------------------------

def _all_small_adam_cases():
    for n in oc.SINGLE_N:
        yield from oc.adam_single_cases(n)
    yield from oc.adam_product_cases()
    for sizes in oc.MULTI_SIZES:
        yield from oc.adam_multi_cases(sizes)
    yield oc.adam_steps_case()


def test_adamw_restatement_is_within_the_bounds_on_every_small_case():
    rec = {}
    for case in _all_small_adam_cases():
        oc.judge_adam(case, oc.emulate_run, rec, True)
    print(rec)
    for x in 'pmve':
        assert rec[x][0] <= 1, (x, rec[x])


@pytest.mark.parametrize('shift', range(oc.K))
def test_adamw_restatement_is_within_the_bounds_above_the_block_cap(shift):
    rec = {}
    case, = oc.adam_flat_large_cases([shift])
    oc.judge_adam(case, oc.emulate_run, rec, False)
    for x in 'pmv':
        assert rec[x][0] <= 1, (x, rec[x])


def test_required_outcomes_of_adamw_have_no_tolerance():
    case = next(iter(oc.adam_single_cases(2 * oc.ADAM_PIECE + 3)))    # shift 0: t 1, coef NULL
    s = case.segs[0]
    want, bound = oc.adam_truth(s, s['g'], s['lr'], s['t'], s['decay'], case.coef, case.hyper)
    rec = s['recipe']
    zero, over = rec == oc.RECIPES.index('zero_grad'), rec == oc.RECIPES.index('gr2_overflows')
    dec = oc.decay32(s['lr'], case.hyper.wd)
    assert dec < 1 and zero.sum() > 100 and over.sum() > 100
    for on in (zero, over):
        assert np.array_equal(want['p'][on], (dec * s['p'][on]).astype(np.float64)) and not bound['p'][on].any()
    assert not want['m'][zero].any() and not want['v'][zero].any() and not bound['m'][zero].any() and not bound['v'][zero].any()
    assert np.isinf(want['v'][over]).all() and not bound['v'][over].any() and np.isfinite(want['m'][over]).all()
    emu = oc.adam_emulate(s, s['g'], s['lr'], s['t'], s['decay'], case.coef, case.hyper)
    assert np.isinf(emu['v'][over]).all() and np.array_equal(emu['p'][over], dec * s['p'][over])
    under = rec == oc.RECIPES.index('gr2_underflows')
    assert not emu['v'][under].any() and emu['m'][under].all()          # gr^2 is 0 in fp32, gr is not
    sub = rec == oc.RECIPES.index('gr_subnormal')
    assert (np.abs(s['g'][sub]) < np.finfo(np.float32).tiny).all() and s['g'][sub].all()
    # cancellation: the result is far smaller than its terms, and the bound stays at the terms' size
    can = rec == oc.RECIPES.index('cancel')
    assert (np.abs(want['m'][can]) <= 1e-6 * np.abs(float(case.hyper.b1) * s['m'][can])).all()
    assert (bound['m'][can] >= 4 * oc.U * np.abs(float(case.hyper.b1) * s['m'][can].astype(np.float64))).all()
    # sqrt(v') / sqrt(bc2) far below, near and far above eps
    with np.errstate(all='ignore'):
        sv = np.sqrt(want['v']) / math.sqrt(1 - float(case.hyper.b2) ** s['t'])
    eps = float(case.hyper.eps)
    assert (sv[rec == oc.RECIPES.index('denom_below_eps')] < 1e-3 * eps).all()
    near = sv[rec == oc.RECIPES.index('denom_near_eps')]
    assert (near > 0.4 * eps).all() and (near < 2.1 * eps).all()
    assert (sv[rec == oc.RECIPES.index('denom_above_eps')] > 1e6 * eps).all()


def test_the_weight_decay_factor_is_the_same_fused_or_not_and_rounds_to_one_for_the_backbone():
    for hyper in (oc.HYPER, oc.HYPER_BACKBONE):
        for lr in oc.LRS:
            assert oc.decay32(lr, hyper.wd) == np.float32(1) - lr * hyper.wd
    assert float(oc.LRS[3]) * float(oc.HYPER_BACKBONE.wd) < 2.0 ** -24 and oc.decay32(oc.LRS[3], oc.HYPER_BACKBONE.wd) == 1


def test_adamw_cases_put_every_recipe_on_every_position_class_and_segment():
    P4 = _const('ADAM_PIECE4')
    piece = 4 * P4
    assert set(oc.SINGLE_N) == {1, 3, 4, 5, piece - 4, piece - 1, piece, piece + 1, piece + 4, 2 * piece + 3}
    assert oc.FLAT_LARGE_N == oc.FLAT_MAX_BLOCKS * 1024 + 4 * 1024 + 3
    every = set(range(oc.K))
    seen = {}
    per_size = {}
    backbone = False
    for n in oc.SINGLE_N:
        for case in oc.adam_single_cases(n):
            s = case.segs[0]
            per_size.setdefault(n, set()).update({('t', s['t']), ('coef', None if case.coef is None else float(case.coef))})
            backbone |= case.hyper is oc.HYPER_BACKBONE and oc.decay32(s['lr'], case.hyper.wd) == 1
            for entry in ('flat', 'multi'):
                for cls, r in zip(oc.adam_classes(n, entry), s['recipe']):
                    seen.setdefault((entry, cls), set()).add(int(r))
    assert backbone
    for n, got in per_size.items():
        assert got >= {('t', t) for t in oc.TS} | {('coef', None), ('coef', 1.0), ('coef', 0.5), ('coef', 0.0)}, n
    for cls in ('body', 'last4_of_piece', 'first4_of_next_piece', 'tail'):
        assert seen[('multi', cls)] == every, cls
    for case in oc.adam_flat_large_cases():
        # only the classes' elements: the second trip and the tail
        cls = oc.adam_classes(oc.FLAT_LARGE_N, 'flat')
        for c in ('second_trip', 'last4_of_first_trip', 'first4_of_second_trip', 'tail'):
            seen.setdefault(('flat', c), set()).update(int(r) for r in case.segs[0]['recipe'][cls == c])
    stride = oc.FLAT_MAX_BLOCKS * 256
    assert oc.FLAT_LARGE_N // 4 - stride == 1024 and oc.FLAT_LARGE_N % 4 == 3
    for cls in ('body', 'tail', 'second_trip', 'last4_of_first_trip', 'first4_of_second_trip'):
        assert seen[('flat', cls)] == every, cls
    assert {(t, None if c is None else float(c)) for case in oc.adam_product_cases() for t, c in [(case.segs[0]['t'], case.coef)]} == \
        {(t, c) for t in oc.TS for c in (None, 1.0, 0.5, 0.0)}
    nsegs = set()
    for sizes in oc.MULTI_SIZES:
        nsegs.add(len(sizes))
        seg_seen = [set() for _ in sizes]
        lr_t = set()
        for case in oc.adam_multi_cases(sizes):
            for k, s in enumerate(case.segs):
                seg_seen[k].update(int(r) for r in s['recipe'])
            lr_t.add(len({(float(s['lr']), s['t']) for s in case.segs}) == len(sizes))
        assert lr_t == {True}, sizes                                  # each segment its own lr and t
        for k, n in enumerate(sizes):
            assert seg_seen[k] == (every if n else set()), (sizes, k)
    assert nsegs == {2, 3, 4}
    assert any(s[1] == 1 and s[0] > piece and s[2] > piece for s in oc.MULTI_SIZES if len(s) == 3)     # one float between two large segments
    assert any(0 in s for s in oc.MULTI_SIZES)
    steps = oc.adam_steps_case()
    assert len(steps.steps) == 8 and len({None if c is None else float(c) for _, c in steps.steps}) == 8
