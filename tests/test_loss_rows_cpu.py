"""CPU tests of tests/loss_rows.py: the closed-form fp64 reference against fp64 autograd, the tensor-op restatement and the fp32 emulation of
joint_loss::row (the forms of its log-softmax) through the per-row comparator, and the comparator itself."""
import numpy as np
import pytest
import torch

import loss_rows as lr
from training_fp64 import HEADS, LOSSES, mixed_fp64


def _weights(case):
    return (lr.LAMBDA_ORD, lr.MU_UNC, lr.NU_KAN, case.gamma)


def _saturated(case, dtype):
    """Rows whose p_t rounds to 1 in ``dtype`` for a label the launch reads."""
    out, ta, tb, _, _ = lr.torch_case(case, dtype=dtype)
    p = torch.softmax(out['cls_logits'], dim=1)
    sat = p.gather(1, ta.unsqueeze(1)).squeeze(1) == 1
    if case.lam is not None:
        sat |= p.gather(1, tb.unsqueeze(1)).squeeze(1) == 1
    return sat.numpy()


@pytest.mark.parametrize('family', lr.FAMILIES)
def test_closed_form_is_finite_and_equals_fp64_autograd_where_that_is_finite(family):
    """fp64 autograd of training_fp64.joint_loss_fp64 / mixed_fp64 forms (1 - p_t)^gamma by subtraction: for gamma < 1 its gradient is 0 * inf
    once p_t rounds to 1, and before that 1 - p_t carries 1e-16 / (1 - p_t) of itself.  So: the closed form is finite on every row; autograd
    is non-finite exactly on the gamma < 1 rows whose p_t is 1 in fp64; on all other rows the two agree to 1e-10 of the row's scale
    max(1, max_j |G|) in every head, and to 1e-10 of the row's own largest entry in the class head where the gap is at most 5 (1 - p_t is at
    least e^-10 there, so the subtraction costs autograd 1e-11 at the most).  The losses agree to 1e-10 relative.  The rows that this leaves
    to the floored bound are checked without a floor by test_closed_form_against_400_digit_arithmetic_on_every_focal_row."""
    n_bad = 0
    for case in lr.cases(family):
        L, G = lr.reference(case)
        assert all(np.isfinite(G[k]).all() for k in HEADS) and all(np.isfinite(L[k]) for k in LOSSES), case.name
        out, ta, tb, sev, alpha = lr.torch_case(case, dtype=torch.float64)
        lam = 1.0 if case.lam is None else case.lam
        La, ga = mixed_fp64(out, ta, ta if case.lam is None else tb, lam, sev, case.stage, _weights(case), alpha)
        Ga = lr.per_sample(ga, case)
        bad = ~np.all(np.stack([np.isfinite(Ga[k]).all(axis=1) for k in HEADS]), axis=0)
        want_bad = _saturated(case, torch.float64) if case.gamma < 1.0 and case.gamma != 0.0 else np.zeros(case.B, bool)
        assert np.array_equal(bad, want_bad), (case.name, np.nonzero(bad != want_bad)[0][:5])
        n_bad += int(bad.sum())
        for k in LOSSES:
            assert abs(La[k] - L[k]) <= 1e-10 * abs(L[k]), (case.name, k, La[k], L[k])
        for k in HEADS:
            err = np.abs(Ga[k] - G[k]).max(axis=1)
            scale = np.abs(G[k]).max(axis=1)
            ok = err <= 1e-10 * np.maximum(1.0, scale)
            if k == 'cls_logits':
                strict = ~(case.gap > 5.0)                      # NaN (a family with mild logits) counts as a small gap
                ok &= ~strict | (err <= 1e-10 * scale)
            i = int(np.argmin(ok | bad))
            assert (ok | bad)[i], (case.name, case.names[i], k, err[i], scale[i])
    print(f'{family}: fp64 autograd is non-finite on {n_bad} rows (gamma < 1, p_t = 1 in fp64)')
    assert (n_bad > 0) == (family == 'focal')


@pytest.mark.parametrize('family', lr.FAMILIES)
def test_tensor_op_form_in_fp32_passes_on_every_row_where_it_is_finite(family):
    """JointLoss._forward_tensor_ops in fp32 on the CPU.  Its backward is 0 * inf for 0 < gamma < 1 where p_t rounds to 1 in fp32: those rows
    are counted, must all be of that kind, and are the only ones left out.  Its forward is finite everywhere, so every loss is compared."""
    from rovit_hip.losses import JointLoss
    worst_g = worst_l = 0.0
    n_bad = 0
    for case in lr.cases(family):
        out, ta, tb, sev, alpha = lr.torch_case(case)
        out = {k: v.requires_grad_(True) for k, v in out.items()}
        lf = JointLoss(lr.LAMBDA_ORD, lr.MU_UNC, lr.NU_KAN, case.gamma, alpha, num_classes=case.C)
        losses = lf(out, ta, sev, case.stage) if case.lam is None else lf.mixed(out, ta, tb, case.lam, sev, case.stage)
        losses['total_loss'].backward()
        G = lr.per_sample({k: out[k].grad for k in HEADS}, case)
        bad = ~np.all(np.stack([np.isfinite(G[k]).all(axis=1) for k in HEADS]), axis=0)
        if bad.any():
            assert 0.0 < case.gamma < 1.0 and _saturated(case, torch.float32)[bad].all(), (case.name, np.nonzero(bad)[0][:5])
        n_bad += int(bad.sum())
        L_ref, G_ref = lr.reference(case)
        ratios = lr.grad_ratios({k: np.where(bad[:, None], G_ref[k], G[k]) for k in HEADS}, G_ref)
        for k in HEADS:
            i = int(np.argmax(ratios[k]))
            worst_g = max(worst_g, float(ratios[k][i]))
            assert ratios[k][i] <= 1.0, (case.name, case.names[i], k, ratios[k][i])
        for k, v in lr.loss_ratios({k: float(v.detach()) for k, v in losses.items()}, L_ref).items():
            worst_l = max(worst_l, v)
            assert v <= 1.0, (case.name, k, v)
    print(f'{family}: tensor-op form in fp32: worst gradient {worst_g:.3g}, worst loss {worst_l:.3g} of the bound; {n_bad} non-finite rows '
          '(0 < gamma < 1, p_t = 1 in fp32) left out')
    assert (n_bad > 0) == (family == 'focal')


@pytest.mark.parametrize('form', ['reordered', 'kernel'])
@pytest.mark.parametrize('family', lr.FAMILIES)
def test_emulation_with_the_reordered_log_softmax_passes_on_the_whole_grid(family, form):
    """'reordered' everywhere, as the issue asks, and the kernel's own choice: the direct sum where |zmax| < 4, reordered elsewhere.  Both
    regimes of the kernel have rows in the grid: offset 0 with a gap below 4, and every other row."""
    worst_g = worst_l = 0.0
    n_direct = 0
    for case in lr.cases(family):
        L, G = lr.emulate(case, form)
        g, l = lr.compare(case, L, G, what=f'emulation ({form})')
        worst_g, worst_l = max(worst_g, g), max(worst_l, l)
        n_direct += int((np.abs(case.cls.max(axis=1)) < lr.DIRECT_BELOW).sum())
    print(f'{family}: emulation, {form}: worst gradient {worst_g:.3g}, worst loss {worst_l:.3g} of the bound; {n_direct} rows with |zmax| < 4')
    assert n_direct > 0


def test_the_switch_constant_is_the_headers_and_both_sides_of_it_pass():
    """tests/loss_rows.py restates joint_loss::DIRECT_BELOW: read the header, so that the two cannot drift apart.  The rows whose largest logit
    is the last fp32 below 4, 4, -4 and the first fp32 above -4 pass in the kernel's form (and in the reordered one), so the change of form
    leaves no step in the result that the bound would see."""
    import os
    import re
    from conftest import PKG
    text = open(os.path.join(PKG, 'csrc', 'joint_loss_row.h')).read()
    m = re.search(r'constexpr float DIRECT_BELOW = ([0-9.]+)f;', text)
    assert m and float(m.group(1)) == lr.DIRECT_BELOW
    assert 'fabsf(zmax) < DIRECT_BELOW' in text
    worst = 0.0
    for case in lr.cases('switch'):
        direct = np.abs(case.cls.max(axis=1)) < lr.DIRECT_BELOW
        assert direct.sum() * 2 == case.B                       # half of the rows on each side
        for form in ('kernel', 'reordered'):
            L, G = lr.emulate(case, form)
            worst = max(worst, lr.compare(case, L, G, what=f'emulation ({form})')[0])
    print(f'switch rows: worst gradient {worst:.3g} of the bound')


def _focal_mp(z, t, gamma, alpha):
    """The focal gradient of one row with 400 digits, in the plain form that needs them: softmax by division, 1 - p_t by subtraction."""
    import mpmath as mp
    e = [mp.e ** (mp.mpf(float(v)) - mp.mpf(float(max(z)))) for v in z]
    S = mp.fsum(e)
    p = [v / S for v in e]
    om, logpt = 1 - p[t], mp.log(p[t])
    coef = (gamma * om ** (gamma - 1) * p[t] * logpt if gamma != 0.0 else 0) - om ** gamma
    a = 1.0 if alpha is None else float(alpha[t])
    return [a * coef * ((1 if j == t else 0) - p[j]) for j in range(len(z))], a * om ** gamma * (-logpt)


def test_closed_form_against_400_digit_arithmetic_on_every_focal_row():
    """fp64 autograd cannot check the saturated rows: it forms 1 - p_t by subtraction.  With 400 digits the subtraction is harmless (1 - p_t is
    never below 1e-105 on the grid), so the plain formula checks the closed form's stable one on every row, target, gamma and alpha of the
    focal family: every entry of the row to 1e-10 of the row's own largest entry, with no floor, and the row's loss to 1e-10 relative (the figure the issue sets for the reference); what lies below 1e-300 has left fp64's range (gamma = 5 at a gap of 80 gives 1e-347) and is held to 1e-300 absolute."""
    import mpmath as mp
    worst = 0.0
    with mp.workdps(400):
        tiny = mp.mpf(10) ** -300
        for C in lr.CS:
            p = lr.focal_pool(C)
            z64 = p.cls.astype(np.float64)
            for gamma in lr.GAMMAS:
                for alpha in (None, lr.alpha_of(C)):
                    for t in (p.ta, p.tb):
                        val, G = lr._focal_fp64(z64, t, gamma, alpha)
                        for r in (range(len(t)) if t is p.ta else np.nonzero(p.tb != p.ta)[0]):
                            g_mp, v_mp = _focal_mp(p.cls[r], int(t[r]), gamma, alpha)
                            scale = max(abs(x) for x in g_mp)
                            err = max(abs(mp.mpf(float(a)) - b) for a, b in zip(G[r], g_mp))
                            rel = float(err / scale) if scale > tiny else 0.0
                            worst = max(worst, rel)
                            assert err <= mp.mpf(1e-10) * scale + tiny, (C, gamma, p.names[r], rel)
                            assert abs(mp.mpf(float(val[r])) - v_mp) <= mp.mpf(1e-10) * abs(v_mp) + tiny, (C, gamma, p.names[r])
    print(f'closed form against 400 digits: worst entry {worst:.3g} of its row')


def test_emulation_with_the_lse_form_fails_and_only_on_the_offset_1000_rows():
    """lse = zmax + log(se) is rounded at the size of zmax: around 1000 every log-probability of a row is off by up to 3e-5, and so is the
    relative error of every gradient of the row, three bounds.  Around 0 and around +-30 the same form stays inside the bound."""
    n_fail = 0
    worst = {0.0: 0.0, 30.0: 0.0, 1000.0: 0.0}
    for family in lr.FAMILIES:
        for case in lr.cases(family):
            _, G = lr.emulate(case, 'lse')
            gr = lr.grad_ratios(G, lr.reference(case)[1])
            row = np.max(np.stack([gr[k] for k in HEADS]), axis=0)
            bad = lr.failing_rows(case, G)
            n_fail += len(bad)
            assert np.all(np.abs(case.off[bad]) == 1000.0), (case.family, case.name, [case.names[i] for i in bad[:5]])
            for off in worst:
                sel = np.abs(case.off) == off
                if sel.any():
                    worst[off] = max(worst[off], float(row[sel].max()))
    print(f'emulation, lse form: {n_fail} rows above the bound, all at |off| = 1000; worst ratio by |off|: {worst}')
    assert n_fail > 0 and worst[1000.0] > 1.0


@pytest.mark.parametrize('head', HEADS)
def test_comparator_rejects_one_element_moved_by_twice_its_bound(head):
    case = next(c for c in lr.cases('batch') if c.B == 513 and c.stage == 4 and c.lam is None)
    L, G = lr.reference(case)
    assert lr.compare(case, L, G) == (0.0, 0.0)
    row = 300
    bound = lr.GRAD_TOL * max(1.0, float(np.abs(G[head][row]).max()))
    for factor, rejected in ((0.5, False), (2.0, True)):
        moved = {k: v.copy() for k, v in G.items()}
        moved[head][row, -1] += factor * bound
        if rejected:
            with pytest.raises(AssertionError, match=f'family batch .* row {row} .* head {head}'):
                lr.compare(case, L, moved)
            assert list(lr.failing_rows(case, moved)) == [row]
        else:
            g, _ = lr.compare(case, L, moved)
            assert 0.49 < g < 0.51
    nan = {k: v.copy() for k, v in G.items()}
    nan[head][row, 0] = np.nan                                   # a row that a kernel never wrote
    with pytest.raises(AssertionError, match=f'row {row} '):
        lr.compare(case, L, nan)
    for k in LOSSES:
        off = dict(L)
        off[k] = L[k] + 2.0 * lr.LOSS_TOL * max(1.0, abs(L[k]))
        with pytest.raises(AssertionError, match=k):
            lr.compare(case, off, G)
