"""Honesty conditions of the per-row backward comparators (tests/backward_rows.py), without a GPU: the CPU emulation E stands in the
kernels' place.  E itself must pass every comparator, and a copy of it with one element of one row moved, one token row's outer product
missing from a weight gradient, or two rows of the pos_embed gradient swapped must fail."""
import functools

import pytest
import torch

from backward_rows import (ROWS, block_stages, check_run, dact_ratio, emulate_run, grad_ratio, grad_refs, images, loss_weights, lse_error,
                           row_scale, stage_ratios, vit_sd, worst_of, LSE_TOL)

DEPTH = 6


@functools.lru_cache(maxsize=None)
def _case(B):
    """The emulated run of one batch size; shared by the tests, never modified."""
    sd = vit_sd(DEPTH, seed=100 + B)
    x = images(B, seed=B)
    run = emulate_run(sd, x, loss_weights(B, seed=7 + B), DEPTH, want_dx=True)
    return sd, x, run


@pytest.mark.parametrize('B', [1, 3])
def test_the_emulation_passes_every_comparator(B):
    sd, x, run = _case(B)
    report, fails = check_run(run, sd, x, f'emulation b{B}')
    assert not fails, fails
    # every family was looked at: the two forward leftovers, 8 dgrad tensors (dx_in in the last block), 12 block parameters, 6 others and the image gradient
    assert sum(k.endswith(' vs R') for k in report) == 8 and sum(k.endswith(' vs E') for k in report) == 5
    assert sum(k.startswith('grad ') for k in report) == 12 + 7 and 'dact' in report and 'lse' in report


def _bad_row(rows, B):
    """A patch row of the last image but one (class-token rows: that image's)."""
    return (ROWS if B > 1 else 0) + 100 if rows > B else min(1, B - 1)


def test_one_element_moved_by_five_percent_of_its_row_fails_every_dgrad_comparator():
    B = 3
    sd, x, run = _case(B)
    seen = set()
    for i in range(DEPTH):
        for st in block_stages(run, sd, i):
            r = _bad_row(st.got.shape[0], B)
            bad = st.got.clone()
            bad[r, bad.shape[1] // 2] += 0.05 * float(row_scale(st.R)[r])
            rE, rR, _ = stage_ratios(st)
            assert float(rR.max()) <= 1.0 and (rE is None or float(rE.max()) <= 1.0), (st.name, i)
            rE, rR, _ = stage_ratios(st, bad)
            assert float(rR[r]) > 1.0 and (rE is None or float(rE[r]) > 1.0), (st.name, i, float(rR[r]))
            seen.add(st.name)
        f = run['fwd'][i]
        r = _bad_row(f['dact'].shape[0], B)
        bad = f['dact'].clone()
        bad[r, 384] += 0.05 * float(f['dact'][r].abs().max())
        assert float(dact_ratio(run, sd, i).max()) <= 1.0 and float(dact_ratio(run, sd, i, bad)[r].max()) > 1.0, i
        bad = f['lse'].clone()
        bad[1, 1, 0] *= 1.05
        assert float(lse_error(run, i).max()) <= LSE_TOL < float(lse_error(run, i, bad).max()), i
    assert seen == {'dx_in', 'dpre', 'dx_mid', 'dO', 'dqkv_q', 'dqkv_k', 'dqkv_v', 'dx_out'}


def _with(run, block, field, rows):
    """A copy of the run whose backward field has the given rows replaced."""
    out = dict(run)
    out['bwd'] = list(run['bwd'])
    out['bwd'][block] = dict(run['bwd'][block])
    out['bwd'][block][field] = rows
    return out


@pytest.mark.parametrize('B', [1, 3])
def test_a_weight_gradient_without_one_token_rows_outer_product_fails(B):
    """M = 197 and 591 rows: the missing term is about 1 / M of the sum of |terms|, the bound (M + 16 + 2) 2^-23 of it.  (The LayerNorm
    dgamma / dbeta are not in the list: they sum the weight gradient over its 768 or 576 rows as well, one token row is 1 / (M sqrt(N)) of
    their sum of |terms| and a single missing row can stay inside the accumulation bound; a wrong row shows in the weight itself.)"""
    sd, x, run = _case(B)
    refs = grad_refs(run, sd, x)
    r = _bad_row(B * ROWS, B)
    for block, field, names in ((2, 'dx_in', ('mlp.fc2.weight', 'mlp.fc2.bias')),
                                (2, 'dpre', ('mlp.fc1.weight', 'mlp.fc1.bias')),
                                (1, 'dx_mid', ('attn.proj.weight', 'attn.proj.bias')),
                                (1, 'dqkv', ('attn.qkv.weight', 'attn.qkv.bias')),
                                (DEPTH - 1, 'dqkv', ('attn.qkv.weight',)),
                                (0, 'dx_out', ('patch_embed.proj.weight', 'patch_embed.proj.bias', 'pos_embed'))):
        rows = run['bwd'][block][field].clone()
        rows[r] = 0
        dropped = grad_refs(_with(run, block, field, rows), sd, x)
        for n in names:
            key = n if block == 0 and field == 'dx_out' else f'blocks.{block}.{n}'
            ref, bound = refs[key]
            assert worst_of(grad_ratio(run['grads'][key], ref, bound))[0] <= 1.0, key
            assert worst_of(grad_ratio(dropped[key][0], ref, bound))[0] > 1.0, key


def test_a_pos_embed_gradient_with_two_token_rows_swapped_fails():
    sd, x, run = _case(3)
    ref, bound = grad_refs(run, sd, x)['pos_embed']
    got = run['grads']['pos_embed']
    assert worst_of(grad_ratio(got, ref, bound))[0] <= 1.0
    bad = got.clone()
    bad[0, [17, 18]] = bad[0, [18, 17]]
    v, row, _ = worst_of(grad_ratio(bad, ref, bound))
    assert v > 1.0 and row in (17, 18)


def test_a_gradient_that_is_not_finite_fails():
    sd, x, run = _case(1)
    ref, bound = grad_refs(run, sd, x)['norm.weight']
    bad = run['grads']['norm.weight'].clone()
    bad[5] = float('nan')
    assert not worst_of(grad_ratio(bad, ref, bound))[0] <= 1.0
    st = block_stages(run, sd, 0)[0]
    bad = st.got.clone()
    bad[3, 3] = float('inf')
    assert not float(stage_ratios(st, bad)[1].max()) <= 1.0
