"""GPU tests of the calibration kernels (csrc/calibrate.hip) and their Python layer (rovit_hip/evaluation.py: EvalAccumulator.calibrate,
Calibration.apply), against the numpy fp64 restatement ``calibration_block`` evaluated on the kernel's OWN recorded arrays (``arrays()``
plus the extra columns), so that expf on the device against torch.softmax on the host never enters.

Bounds.  Integer words (row counts, status, coverage counts): equal.  The others are the maximum distance measured on an MI355X over the
cases below times the stated headroom, under a cap that does not move.  Where the measured distance is 0 the smallest distance the
comparison can show takes its place (the host's exp and log differ by an ulp between numpy builds, so equality cannot be asked for):
  ln T*            measured 0 in all nine cases (the secant of a 4.4e-7 wide bracket absorbs the rounding of g: both sides round to the
                   same double), so one ulp of u at |u| <= ln 32, 2^-51, times 8 = 3.6e-15; the cap is 1e-6, about two final brackets
                   (farther off means a wrong bracket)
  fp64 sums, NLLs  measured 4.566e-16 relative (exact600; 2.0e-16 on the random cases), times 8 = 3.7e-15; the cap is 1e-9
  p', sigma'       measured 0 ulp of fp32 against the numpy fp64 formula rounded to fp32 in all four cases, times 4 is still 0, so one
                   rounding flip, 1 ulp; the cap is 4 ulp
Refitting on the device after ``apply``: |ln T| <= 1e-6 (the fp32 rounding of p', averaged over the rows; measured 4.2e-9 at most, and
|s - 1| 1.1e-8)."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import ref_cpu  # noqa: E402  (checker only)
import calibration_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

MEASURED_LN_T, MEASURED_REL, MEASURED_ULP = 0.0, 4.566e-16, 0.0          # the maxima over the cases below, see the docstring
BOUND_LN_T = min(1e-6, 8 * max(MEASURED_LN_T, 2.0 ** -51))
BOUND_REL = min(1e-9, 8 * MEASURED_REL)
BOUND_ULP = min(4.0, max(4 * MEASURED_ULP, 1.0))

# name: (n, C, seed, data).  One row and the at_min bound (n1), a partial chunk (n2, n5), more than one chunk (n257: 2, n1027: 5), more
# chunks than one wave of the step kernel's fold takes one each (n2051: 9 chunks over 4 waves), both class-count limits, the clamped zeros.
CASES = {'n1': (1, 4, 301, 'random'), 'n2': (2, 4, 204, 'random'), 'n5': (5, 4, 500, 'random'), 'n257': (257, 4, 25704, 'random'),
         'n1027': (1027, 4, 102704, 'random'), 'n2051': (2051, 4, 205104, 'random'), 'n300_c2': (300, 2, 30002, 'random'),
         'n300_c8': (300, 8, 30008, 'random'), 'exact600': (600, 4, 41, 'exact')}
INTERIOR = ('n5', 'n257', 'n1027', 'n2051', 'n300_c2', 'n300_c8')


def dev():
    return torch.device('cuda:0')


def _ev():
    from rovit_hip import evaluation
    return evaluation


def _data(name):
    n, C, seed, kind = CASES[name]
    return cc.exact_case(n, C, seed) if kind == 'exact' else cc.make_data(n, C, seed)


def _acc(name, sizes=(1 << 30,), extra=('mu',)):
    return cc.feed(_ev().EvalAccumulator(CASES[name][1]), _data(name), sizes, device=dev(), extra=extra)


_cache = {}


def _case(name):
    """(accumulator, Calibration with the kernel's block, the reference block from the accumulator's own arrays): computed once, shared,
    never changed."""
    if name not in _cache:
        acc = _acc(name)
        cal = acc.calibrate(return_block=True)
        arrays, extras = cc.recorded(acc)
        _cache[name] = (acc, cal, _ev().calibration_block(arrays, extras, CASES[name][1], 9))
    return _cache[name]


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


@pytest.mark.parametrize('name', list(CASES))
def test_block_against_the_reference_on_the_recorded_arrays(name):
    N = _ev().native
    acc, cal, ref = _case(name)
    blk, f, g = cal.block, cal.block.view(np.float64), ref.view(np.float64)
    n, C = CASES[name][:2]
    ints = [N.EVAL_CAL_N_VALID, N.EVAL_CAL_BAD_LABELS, N.EVAL_CAL_N_REG, N.EVAL_CAL_BAD_SIGMA, N.EVAL_CAL_STATUS, N.EVAL_CAL_N]
    assert [int(blk[w]) for w in ints] == [int(ref[w]) for w in ints] and int(blk[N.EVAL_CAL_N]) == n == int(blk[N.EVAL_CAL_N_REG])
    assert np.array_equal(blk[N.EVAL_CAL_COVERAGE:], ref[N.EVAL_CAL_COVERAGE:]) and len(blk) == N.EVAL_CAL_COVERAGE + 9
    assert not blk[5 + 1:N.EVAL_CAL_U].any() and not blk[N.EVAL_CAL_SUM_LOG_SIGMA + 1:N.EVAL_CAL_COVERAGE].any()          # padding stays 0
    d_u = abs(f[N.EVAL_CAL_U] - g[N.EVAL_CAL_U])
    rel = {w: _rel(f[w], g[w]) for w in (N.EVAL_CAL_NLL, N.EVAL_CAL_NLL_CAL, N.EVAL_CAL_SUM_Z2, N.EVAL_CAL_SUM_LOG_SIGMA)}
    print(f'{name}: status {cal.status}, |ln T - reference| {d_u:.3e}, relative distance of the sums {max(rel.values()):.3e}')
    assert d_u <= BOUND_LN_T
    assert max(rel.values()) <= BOUND_REL, rel
    a = acc.arrays()
    want = cc.expected_status(cc.log_probs(a['y_probs']), a['y_true'])          # from g at the two ends alone
    assert cal.status == want == {'n1': 'at_min', 'exact600': 'at_max'}.get(name, 'interior' if name in INTERIOR else want)
    if cal.status == 'interior':
        assert f[N.EVAL_CAL_G_LO] < 0.0 <= f[N.EVAL_CAL_G_HI] and f[N.EVAL_CAL_U_LO] <= f[N.EVAL_CAL_U] <= f[N.EVAL_CAL_U_HI]
        assert f[N.EVAL_CAL_U_HI] - f[N.EVAL_CAL_U_LO] <= 4.5e-7
    assert cal.diagnostics['nll_calibrated'] <= cal.diagnostics['nll'] and cal.diagnostics['gaussian_nll_calibrated'] <= cal.diagnostics['gaussian_nll']


def test_block_is_bit_identical_over_batch_splits_grids_and_runs():
    blocks = []
    for sizes in ((1 << 30,), (1,), (100, 57)):
        acc = _acc('n1027', sizes)
        for wg in (0, 1, 3):
            for run in range(2):
                blocks.append(acc.calibrate(return_block=True, _max_workgroups=wg).block)
    assert all(b.tobytes() == blocks[0].tobytes() for b in blocks) and len(blocks) == 18
    assert blocks[0].tobytes() == _case('n1027')[1].block.tobytes()


@pytest.mark.parametrize('name', ['n5', 'n1027', 'n300_c8', 'exact600'])
def test_apply_against_the_formula_and_the_applied_accumulator(name):
    ev = _ev()
    acc, cal, _ = _case(name)
    C = CASES[name][1]
    applied = cal.apply(acc)
    a, b = acc.arrays(), applied.arrays()
    l = cc.log_probs(a['y_probs'])
    w = np.exp((1.0 / cal.temperature) * (l - l.max(axis=1, keepdims=True)))
    want_p = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    want_s = (cal.sigma_scale * a['uncertainty'].astype(np.float64)).astype(np.float32)
    ulp_p = float((np.abs(b['y_probs'].astype(np.float64) - want_p) / np.spacing(np.maximum(want_p, np.float32(2.0 ** -126)))).max())
    ulp_s = float((np.abs(b['uncertainty'].astype(np.float64) - want_s) / np.spacing(want_s)).max())
    print(f'{name}: p\' within {ulp_p:.2f} ulp, sigma\' within {ulp_s:.2f} ulp of the fp64 formula')
    assert ulp_p <= BOUND_ULP and ulp_s <= BOUND_ULP
    assert all(np.array_equal(a[k], b[k]) for k in ('y_pred', 'y_true', 'severity_true', 'severity_pred'))
    assert np.array_equal(acc._extra_column('mu'), applied._extra_column('mu'))
    assert np.array_equal(a['y_probs'], acc.arrays()['y_probs'])                              # the input accumulator is untouched
    block = ev.result_block_from_arrays(b['y_true'], b['y_pred'], b['y_probs'], b['severity_true'], b['severity_pred'], C, applied.n_bins)
    # the ECE's confidence sums are fp64 sums of n values in [0, 1] in another order: n * 2^-52 on both sides
    assert abs(applied.compute()['ece'] - ev.metrics_from_block(block, C, applied.n_bins)['ece']) <= applied.n * 2.0 ** -51
    sel = applied.selective()
    assert sel['n'] == applied.n and list(sel['scores']) == ['confidence', 'entropy', 'sigma']
    again = applied.calibrate()
    print(f'{name}: refit after apply: ln T {math.log(again.temperature):.3e}, s - 1 {again.sigma_scale - 1.0:.3e}')
    if name in INTERIOR:
        assert abs(math.log(again.temperature)) <= 1e-6 and abs(again.sigma_scale - 1.0) <= 1e-6


def test_missing_regression_part_leaves_the_classification_part_intact():
    import bootstrap_cases
    ev = _ev()
    full = _case('n257')[1]
    no_mu = _acc('n257', extra=()).calibrate(return_block=True)
    no_head = bootstrap_cases.feed(ev.EvalAccumulator(4), _data('n257'), device=dev()).calibrate(return_block=True)
    N = ev.native
    for cal in (no_mu, no_head):
        assert cal.sigma_scale is None and cal.diagnostics['coverage'] is None and cal.bad_sigma == 0
        assert cal.temperature == full.temperature and cal.status == full.status and cal.diagnostics['nll'] == full.diagnostics['nll']
        assert not cal.block[N.EVAL_CAL_SUM_Z2:].any() and int(cal.block[N.EVAL_CAL_N_REG]) == 0
    applied = no_mu.apply(_acc('n257', extra=()))
    assert np.array_equal(applied.arrays()['uncertainty'], _case('n257')[0].arrays()['uncertainty'])
    assert applied.calibrate().sigma_scale is None


def test_bad_rows_on_the_device():
    ev = _ev()
    d = cc.make_data(300, 4, 77)
    d['labels'][[0, 299]] = 9
    d['log_var'][17] = float('nan')
    d['mu'][256] = float('inf')
    acc = cc.feed(ev.EvalAccumulator(4), d, (128,), device=dev())
    cal = acc.calibrate(return_block=True)
    arrays, extras = cc.recorded(acc)
    ref = ev.calibration_block(arrays, extras, 4, 9)
    N = ev.native
    assert (cal.n, cal.bad_labels, cal.bad_sigma) == (300, 2, 2) and np.array_equal(cal.block[:8], ref[:8])
    assert np.array_equal(cal.block[N.EVAL_CAL_COVERAGE:], ref[N.EVAL_CAL_COVERAGE:])
    assert abs(cal.block.view(np.float64)[N.EVAL_CAL_U] - ref.view(np.float64)[N.EVAL_CAL_U]) <= BOUND_LN_T
    all_bad = dict(d, labels=torch.full((300,), -3))
    with pytest.raises(ev.RovitHipError, match='none of the 300 recorded rows'):
        cc.feed(ev.EvalAccumulator(4), all_bad, device=dev()).calibrate()


def test_descriptor_is_refused_before_any_launch():
    import ctypes
    ev = _ev()
    N = ev.native
    d = N.EvalCal()
    d.n, d.num_classes, d.num_levels = 4, 4, 65
    with pytest.raises(ev.RovitHipError, match='coverage levels'):
        N.call('rovit_eval_calibrate', ctypes.byref(d), N.stream_ptr())
    r = N.EvalRecal()
    r.n, r.num_classes, r.beta, r.sigma_scale = 4, 4, 0.0, 1.0
    with pytest.raises(ev.RovitHipError, match='beta'):
        N.call('rovit_eval_recalibrate', ctypes.byref(r), N.stream_ptr())
    assert N.load().rovit_eval_calibrate_workspace_bytes(0, 4) == 0 and N.load().rovit_eval_calibrate_workspace_bytes(257, 4) >= 2 * 64 * 8


def test_evaluator_end_to_end(tmp_path):
    from evaluation.evaluator import Evaluator
    from models.rovit_kan import RoViTKAN
    model = RoViTKAN(pretrained=False)
    model.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    model = model.to(dev()).eval()
    g = torch.Generator().manual_seed(11)
    loader = [(torch.randn(8, 3, 224, 224, generator=g), torch.randint(0, 4, (8,), generator=g), torch.randint(0, 4, (8,), generator=g))
              for _ in range(2)]
    names = ["Healthy Leaf", "Leaf Holes", "Black Spot", "Dry Leaf"]
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=names, num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    ev = Evaluator(model, loader, cfg, dev())                     # the same two batches serve as "validation" and as "test"
    cal = ev.fit_calibration(loader)
    assert ev.calibration is cal and cal.n == 16
    metrics = ev.evaluate(calibration=cal)
    card = metrics['calibration']
    assert set(card) == {'temperature', 'sigma_scale', 'status', 'before', 'after'}
    assert math.isfinite(card['temperature']) and card['temperature'] > 0 and math.isfinite(card['sigma_scale']) and card['sigma_scale'] > 0
    for side in ('before', 'after'):
        assert set(card[side]) == {'nll', 'ece', 'brier_score', 'gaussian_nll', 'coverage', 'levels', 'sigma_scale_refit'}
    print(f"T {card['temperature']:.4f} ({card['status']}), s {card['sigma_scale']:.4f}, NLL {card['before']['nll']:.6f} -> {card['after']['nll']:.6f}")
    assert card['after']['nll'] <= card['before']['nll']
    assert card['before']['ece'] == metrics['ece'] and 'Calibration (temperature' in (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
