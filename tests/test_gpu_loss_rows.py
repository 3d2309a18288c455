"""GPU tests of the fused joint loss at its numerical edges: every family of tests/loss_rows.py through rovit_joint_loss and
rovit_joint_loss_mixed (C ABI, so that lam = 1 and C = 16 reach the kernels), each row of each head against the closed-form fp64 reference;
the upstream-gradient path (rovit_scale_buffers) through JointLoss / JointLoss.mixed; the two kernels bit for bit on the whole grid; and the
epoch record's correct-count against torch.max on ties and NaN.  Every launch is one workgroup over at most 513 rows."""
import ctypes

import numpy as np
import pytest
import torch

import loss_rows as lr
from training_fp64 import HEADS, LOSSES

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def launch(case, mixed, second_column=None, table=None, inputs=None):
    """One launch through the C ABI on output buffers pre-filled with NaN (a row that is never written stays NaN and fails the comparator)
    -> (losses (5,), [gradient or None per head]).  ``mixed``: rovit_joint_loss_mixed, with label column b iff ``second_column``."""
    from rovit_hip import native
    from rovit_hip.native import ptr
    out, ta, tb, sev, alpha = inputs if inputs is not None else lr.torch_case(case, dev())
    h = [out[k].contiguous() if case.stage >= lr.GATE[k] else None for k in HEADS]
    sev_i64 = sev.dtype == torch.int64
    losses = torch.full((5,), float('nan'), device=dev())
    g = [None if t is None else torch.full_like(t, float('nan')) for t in h]
    if not mixed:
        native.call('rovit_joint_loss', *(ptr(t) for t in h), ptr(ta), ptr(sev), int(sev_i64), ptr(alpha), *(ptr(t) for t in g), ptr(losses),
                    case.B, case.C, lr.LAMBDA_ORD, lr.MU_UNC, lr.NU_KAN, case.gamma, native.stream_ptr())
    else:
        d = native.TrainLoss()
        d.batch, d.num_classes, d.severity_is_int64 = case.B, case.C, int(sev_i64)
        d.lam = float(case.lam) if second_column else 0.37          # without a second column lam is not read
        d.lambda_ord, d.mu_unc, d.nu_kan, d.focal_gamma = lr.LAMBDA_ORD, lr.MU_UNC, lr.NU_KAN, case.gamma
        d.cls_logits, d.ordinal_logits, d.mu, d.log_var, d.kan_severity = (ptr(t) for t in h)
        d.class_targets_a, d.class_targets_b, d.severity_targets, d.focal_alpha = ptr(ta), ptr(tb if second_column else None), ptr(sev), ptr(alpha)
        d.d_cls, d.d_ord, d.d_mu, d.d_lv, d.d_kan = (ptr(t) for t in g)
        d.losses_out = ptr(losses)
        if table is not None:
            d.table, d.row, d.capacity = ptr(table), 0, table.shape[0]
        native.call('rovit_joint_loss_mixed', ctypes.byref(d), native.stream_ptr())
    return losses, g


def _check(case, losses, grads, what, upstream=1.0):
    return lr.compare(case, dict(zip(LOSSES, losses.cpu().tolist())) if losses is not None else None, lr.per_sample(grads, case), upstream, what)


def family_through_both_kernels(family):
    """Every launch of a family against the closed form -> {kernel: (worst gradient ratio, worst loss ratio)} in units of the bounds.  The
    unmixed launches go through both kernels, the mixed ones through rovit_joint_loss_mixed."""
    worst = {'rovit_joint_loss': [0.0, 0.0], 'rovit_joint_loss_mixed': [0.0, 0.0]}
    for case in lr.cases(family):
        inputs = lr.torch_case(case, dev())
        runs = [('rovit_joint_loss_mixed', True, True)] if case.lam is not None else [('rovit_joint_loss', False, False), ('rovit_joint_loss_mixed', True, False)]
        for name, mixed, second in runs:
            losses, g = launch(case, mixed, second, inputs=inputs)
            e = _check(case, losses, g, name)
            worst[name] = [max(a, b) for a, b in zip(worst[name], e)]
    return worst


@pytest.mark.parametrize('family', lr.FAMILIES + ('switch',))
def test_every_row_of_the_family_matches_the_closed_form(family):
    """'switch': the rows whose largest logit sits on either side of +-4, where the row changes the form of its log-softmax."""
    for name, (g, l) in family_through_both_kernels(family).items():
        print(f'{family} {name}: worst gradient {g:.3g}, worst loss {l:.3g} of the bound')


@pytest.mark.parametrize('family', lr.FAMILIES)
def test_unmixed_and_mixed_kernels_are_bit_identical_on_the_grid(family):
    for case in lr.cases(family):
        if case.lam is not None:
            continue
        inputs = lr.torch_case(case, dev())
        (l_old, g_old), (l_new, g_new) = launch(case, False, inputs=inputs), launch(case, True, False, inputs=inputs)
        assert torch.isfinite(l_old).all() and torch.equal(l_old, l_new), (case.name, l_old, l_new)
        for k, x, y in zip(HEADS, g_old, g_new):
            assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), (case.name, k)


def test_upstream_gradient_path_on_the_batch_family():
    """JointLoss and JointLoss.mixed chain the kernel's gradients with the upstream one in rovit_scale_buffers: upstream 1 and 3 at every
    batch size and stage of the batch family."""
    from rovit_hip.losses import JointLoss
    worst = 0.0
    for case in lr.cases('batch'):
        out, ta, tb, sev, alpha = lr.torch_case(case, dev())
        lf = JointLoss(lr.LAMBDA_ORD, lr.MU_UNC, lr.NU_KAN, case.gamma, alpha, num_classes=case.C)
        for upstream in ((1.0, 3.0) if case.lam is None else (3.0,)):
            o = {k: v.clone().requires_grad_(True) for k, v in out.items()}
            losses = lf(o, ta, sev, case.stage) if case.lam is None else lf.mixed(o, ta, tb, case.lam, sev, case.stage)
            (upstream * losses['total_loss']).backward()
            got = lr.per_sample({k: o[k].grad for k in HEADS}, case)
            g, _ = lr.compare(case, {k: float(v.detach()) for k, v in losses.items()}, got, upstream, f'JointLoss upstream {upstream:g}')
            worst = max(worst, g)
    print(f'upstream path: worst gradient {worst:.3g} of the bound')


def _argmax_rows(B, C):
    """Logits whose argmax is a matter of convention, four kinds in turn, and labels at the first maximum (first half of the batch) or the last
    (second half): all equal; a tie between a low and a high index; one NaN among larger finite values; two NaN."""
    nan = float('nan')
    z = np.empty((B, C), np.float32)
    t = np.empty(B, np.int64)
    for b in range(B):
        row = -1.0 - 0.25 * np.arange(C)
        kind = b % 4
        if kind == 0:
            row[:] = 0.5
            first, last = 0, C - 1
        elif kind == 1:
            row[1] = row[C - 1] = 2.0
            first, last = 1, C - 1
        elif kind == 2:
            row[:] = 5.0 + np.arange(C)
            row[C // 2] = nan
            first = last = C // 2
        else:
            row[:] = 3.0 + np.arange(C)
            row[0] = row[C - 2] = nan
            first, last = 0, C - 2
        z[b], t[b] = row, (first if b < B // 2 else last)
    return z, t


@pytest.mark.parametrize('B', [64, 257, 513])
def test_correct_count_of_the_epoch_record_equals_torch_max_on_ties_and_nan(B):
    from rovit_hip import native
    for C in (4, 16):
        z, t = _argmax_rows(B, C)
        want = int((torch.max(torch.from_numpy(z), dim=1).indices == torch.from_numpy(t)).sum())
        assert 0 < want < B
        case = next(c for c in lr.cases('kan') if c.C == C and c.lam is None)
        i = np.arange(B) % case.B
        big = lr.make_case('argmax', f'B {B} C {C}', C, case.sev[i], dict(cls=z, ta=t, tb=t[::-1].copy(), kan=case.kan[i]), [str(b) for b in range(B)], lam=0.3)
        for second in (False, True):
            table = torch.zeros(1, native.TRAIN_ROW_WORDS, dtype=torch.int32, device=dev())
            launch(big, True, second, table=table)
            row = table.cpu()[0].tolist()
            assert row[native.TRAIN_ROW_CORRECT] == want and row[native.TRAIN_ROW_BATCH] == B, (C, second, row, want)
