"""CPU tests of tests/attention_cases.py, the references and bounds behind tests/test_gpu_attention_rows.py: the selector conditions at every
token count, the emulation E inside the derived bounds of the truth R, the mutation table (E with one fault injected must fail), and the
refusals of the C entry points, which happen before any launch."""
import ctypes
import math
import os

import pytest
import torch

import attention_cases as ac


@pytest.fixture(scope='module')
def native():
    from rovit_hip import native as n
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return n


def test_edge_token_counts():
    for t in (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 191, 192, 193, 197, 207, 208):
        assert t in ac.EDGE_T
    assert ac.EDGE_T[-1] == 208 and ac.ALL_T == list(range(1, 209)) and ac.CLS_T[-1] == 224
    # every shape of the backward's last block: no tail, a tail of at most 16 rows (TailHalf), a longer one (TailBoth / Full)
    assert {(t & 31 == 0, 0 < t & 31 <= 16, t & 31 > 16) for t in ac.EDGE_T} == {(True, False, False), (False, True, False), (False, False, True)}


def test_selector_conditions_and_closed_forms_at_every_token_count():
    """make() raises where a condition does not hold (selector_gap); the fp64 softmax of the selector is v[pi], that of the pair selector the
    closed form, to 1e-12.  209 .. 224: the class-token kernels' range."""
    for T in ac.CLS_T:
        for gen in ('selector', 'pair_selector'):
            case = ac.make(gen, T, H=1, seed=0)
            assert case.info['gap_log2'] > ac.UNDERFLOW_LOG2
            R, cf = ac.truth(case, softmax=True), ac.closed_form(case)
            for n in cf:
                assert float((R[n] - cf[n]).abs().max()) <= 1e-12 * max(1.0, float(cf[n].abs().max())), (gen, T, n)
            tgt = case.info['targets'][0, 0]
            v = case.heads()[2][0, 0]
            if gen == 'selector':
                assert torch.equal(tgt[:, 0], tgt[:, 1]) and sorted(tgt[:, 0].tolist()) == list(range(T))       # a permutation
                assert float((R['out'][0, 0] - v[tgt[:, 0]]).abs().max()) <= 1e-12
                assert float(cf['dq'].abs().max()) == 0.0 and float(cf['dk'].abs().max()) == 0.0
            elif T > 1:
                assert bool((tgt[:, 0] != tgt[:, 1]).all())
                assert float(cf['dq'].abs().max()) > 0.0 and float(cf['dk'].abs().max()) > 0.0
            # V distinguishes every key in every column
            assert all(len(set(v[:, d].tolist())) == T for d in range(ac.HD))


def test_selector_condition_is_checked_not_assumed():
    case = ac.make('selector', 40, seed=0)
    case.qkv = case.qkv.clone()
    case.qkv.view(1, 40, 3, 64)[0, :, 1] /= 4.0                   # keys 1.5 c_j: the gap shrinks fourfold
    with pytest.raises(ValueError, match='off-target gap'):
        ac.selector_gap(case)
    case = ac.make('pair_selector', 40, seed=0)
    case.info['targets'][0, 0, 3, 1] = next(j for j in range(40) if j not in case.info['targets'][0, 0, 3].tolist())
    with pytest.raises(ValueError, match='do not tie'):
        ac.selector_gap(case)


@pytest.mark.parametrize('gen', ac.GENERATORS)
def test_emulation_stays_inside_the_bounds(gen):
    """E, rounded as the kernels round, against R at every edge token count, dense and class-token: the bounds hold for their own emulation."""
    for T in ac.EDGE_T + [209, 223, 224]:
        case = ac.make(gen, T, H=2, B=1, seed=3)
        if T <= 208:
            R = ac.truth(case)
            rep = ac.compare(ac.stand_in(case), R, ac.bounds(case, R))
            assert not ac.failures(rep), (gen, T, rep)
        R = ac.truth(case, cls=True)
        res = ac.stand_in(case, cls=True)
        rep = ac.compare(res, R, ac.bounds(case, R, cls=True), rows=slice(0, 1))
        assert not ac.failures(rep), (gen, 'cls', T, rep)
        assert float(res['dq'][:, :, 1:].abs().max()) == 0.0 if T > 1 else True


def test_selector_emulation_is_exact_where_the_gpu_test_asserts_bits():
    """What test_gpu_attention_rows asserts bit for bit on the selectors, shown on E: out and dV equal bf16(R) (every operand an exactly
    representable integer or half integer, the unnormalised probability 1 after its bf16 rounding), dQ and dK of the selector exactly zero
    (dP - delta cancels in integers on the target key, every other probability underflows)."""
    for gen in ('selector', 'pair_selector'):
        for T in (1, 2, 17, 33, 64, 197, 208):
            case = ac.make(gen, T, H=2, seed=1)
            R, res = ac.truth(case), ac.stand_in(case)
            assert torch.equal(res['out'], ac.bf(R['out'])) and torch.equal(ac.bf(R['out']), R['out'])
            assert torch.equal(res['dv'], ac.bf(R['dv']))
            if gen == 'selector':
                assert float(res['dq'].abs().max()) == 0.0 and float(res['dk'].abs().max()) == 0.0


def test_mutation_table():
    """Every fault fails the per-row comparators at T = 197 and at one T per shape of the backward's last block (33 TailHalf, 49 TailBoth /
    Full, 64 no tail), in at least one generator -- a fault cannot show where the data hide it (two exchanged keys under uniform
    probabilities, a padded key or a missing log2 l next to a one-hot row, a dK that the truth makes zero).

    Against the old max-norm criteria of test_attention_fwd_bwd (old_criteria) on the same faulty results:
      * tail_dv_without_x8 PASSES them in pair_selector at every T: dV is eight times too small in the whole tail block while dQ and dK
        are 500 times larger than dV, and the one number for the three thirds of dqkv never looks at dV;
      * no other fault passes them in a generator where the new comparators catch it.  In particular the 0.125 / scale fault does NOT: in
        all of these inputs dQ and dK are as large as dV, and a factor 1/2 on them breaks a 3e-2 max-norm criterion.  The old suite missed
        it because it never ran a scale other than 1/8, not because of its norm.  The masking faults (last key dropped, padded key unmasked)
        fail the old lse2 criterion (1e-3) wherever they show at all."""
    table = ac.mutation_table()
    assert list(table) == list(ac.FAULTS)
    for fault, rec in table.items():
        for T, gens in rec['caught'].items():
            assert gens, f'{fault} is not caught at T = {T}'
    assert 'random' in table['dq_dk_times_eighth_over_scale']['caught'][197]
    assert {f for f, rec in table.items() if rec['slipped']} == {'tail_dv_without_x8'}
    assert table['tail_dv_without_x8']['slipped'] == [('pair_selector', T) for T in (197, 33, 49, 64)]
    # the unfaulted stand-in passes both
    for gen in ('random', 'selector', 'pair_selector', 'uniform'):
        case = ac.make(gen, 197)
        R = ac.truth(case)
        res = ac.stand_in(case)
        assert not ac.failures(ac.compare(res, R, ac.bounds(case, R))) and ac.old_criteria(res, R)


def test_comparator_is_per_row_and_per_tensor():
    case = ac.make('random', 50, H=2, B=2, seed=5)
    R = ac.truth(case)
    B = ac.bounds(case, R)
    res = ac.stand_in(case)
    res['dk'] = res['dk'].clone()
    res['dk'][1, 0, 37] *= 2.0                                     # one dK row wrong by 100 %
    rep = ac.compare(res, R, B)
    assert set(ac.failures(rep)) == {'dk'} and rep['dk'][1] == (1, 0, 37)
    res['lse2'] = res['lse2'].clone()
    res['lse2'][0, 1, 49] = math.nan
    rep = ac.compare(res, R, B)
    assert rep['lse2'] == (math.inf, (0, 1, 49))


# ---- the C entry points refuse before anything is launched ---------------------------------------------------------------------------

def _err(lib):
    return lib.rovit_last_error_string().decode()


def test_attention_entries_refuse_bad_scale_tokens_and_head_dim(native):
    lib = native.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    off = (ctypes.c_int * 5)(0, 5, 9, 12, 20)
    # name -> (function, good arguments, index of tokens (None: ragged), of head_dim, of scale, largest token count)
    entries = {
        'attention_fwd': (lib.rovit_attention_fwd, [p, p, p, 2, 197, 3, 64, 0.125, None], 4, 6, 7, 208),
        'attention_bwd': (lib.rovit_attention_bwd, [p, p, p, p, p, 2, 197, 3, 64, 0.125, None], 6, 8, 9, 208),
        'attention_cls_fwd': (lib.rovit_attention_cls_fwd, [p, p, p, 2, 197, 3, 64, 0.125, None], 4, 6, 7, 224),
        'attention_cls_bwd': (lib.rovit_attention_cls_bwd, [p, p, p, p, p, 2, 197, 3, 64, 0.125, None], 6, 8, 9, 224),
        'attention_fwd_ragged': (lib.rovit_attention_fwd_ragged, [p, p, None, p, off, 4, 3, 64, 0.125, None], None, 7, 8, None),
        'attention_cls_fwd_ragged': (lib.rovit_attention_cls_fwd_ragged, [p, p, None, None, None, p, off, 4, 3, 64, 0.125, None], None, 9, 10,
                                     None),
    }
    SHAPE = -1                                                         # ROVIT_ERR_SHAPE
    for what, (fn, good, k_tok, k_hd, k_scale, t_max) in entries.items():
        for bad in (0.0, -0.125, -0.0, math.nan, math.inf, -math.inf):
            args = list(good)
            args[k_scale] = bad
            assert fn(*args) == SHAPE, (what, bad)
            assert _err(lib).startswith(what + ': scale must be ') and ('%g' % bad).lstrip('-') in _err(lib), _err(lib)
        if k_tok is not None:
            for bad in (0, -1, t_max + 1):
                args = list(good)
                args[k_tok] = bad
                assert fn(*args) == SHAPE, (what, bad)
                assert 'attention' in _err(lib)
        for bad in (32, 63, 128, 0):
            args = list(good)
            args[k_hd] = bad
            assert fn(*args) == SHAPE, (what, bad)
            assert 'attention' in _err(lib)
    # attn_bwd_kernel folds 2^-3: every other scale is refused with the value in the message
    fn, good = entries['attention_bwd'][:2]
    for bad, text in ((0.25, '0.25'), (0.0625, '0.0625'), (0.1, '0.1'), (0.12500001, '0.125')):
        args = list(good)
        args[9] = bad
        assert fn(*args) == SHAPE
        assert _err(lib).startswith('attention_bwd: scale must be 0.125') and f'(got {text}' in _err(lib), _err(lib)
    assert lib.rovit_version() == native.ABI_VERSION
