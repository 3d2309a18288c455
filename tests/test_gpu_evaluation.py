"""GPU tests of test-set evaluation and validation (csrc/evaluate.hip, rovit_hip/evaluation.py, evaluation/): the two kernels against
the reference's arithmetic (sklearn / scipy on the kernel's own recorded probabilities), bit-reproducibility, ties and degenerate
inputs, the drop-in Evaluator end to end in the reference-precision mode, validate() against the reference-shaped loop, and the absence
of hidden synchronisation.

Bounds.  Recorded probabilities against torch.softmax in fp64: 1e-5 (a correctly rounded expf and a sum of at most 8 terms give about
1.5e-6).  Float metrics against the reference functions on the SAME probabilities: 1e-9 (fp64 sums of at most 20 000 terms of size at
most 2 carry at most 20 000 * 2^-52 ~ 5e-12, times 100 for the percent values); rho 1e-12; integers equal."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_cpu  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu

CLASS_NAMES = ["Healthy Leaf", "Leaf Holes", "Black Spot", "Dry Leaf"]
SEVERITY = {n: i for i, n in enumerate(CLASS_NAMES)}


def dev():
    return torch.device('cuda:0')


def _full_model(sd):
    from models.rovit_kan import RoViTKAN
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(sd, strict=True)
    return m.to(dev())


def _data(n, C, seed, ties=False):
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, C, (n,), generator=g)
    logits = torch.randn(n, C, generator=g) * 2.0
    logits[torch.arange(n), labels] += 1.5
    sev_true = torch.randint(0, 4, (n,), generator=g)
    sev_pred = (sev_true.float() + torch.randn(n, generator=g) * 0.8).clamp(0, 3)
    if ties:
        sev_pred = (sev_pred * 10).round() / 10
    log_var = torch.randn(n, generator=g)
    return {'logits': logits, 'labels': labels, 'sev_true': sev_true, 'sev_pred': sev_pred, 'log_var': log_var}


def _batches(d, sizes, labels_on_device=True):
    out, i, k, n = [], 0, 0, d['logits'].shape[0]
    while i < n:
        j = min(n, i + sizes[k % len(sizes)])
        k += 1
        o = {'cls_logits': d['logits'][i:j].to(dev()), 'kan_severity': d['sev_pred'][i:j].reshape(-1, 1).to(dev()),
             'mu': torch.zeros(j - i, 1, device=dev()), 'log_var': d['log_var'][i:j].reshape(-1, 1).to(dev())}
        cl, sv = d['labels'][i:j], d['sev_true'][i:j]
        if labels_on_device:
            cl, sv = cl.to(dev()), sv.to(dev())
        out.append((o, cl, sv))
        i = j
    return out


def _feed(acc, d, sizes, labels_on_device=True, losses=None):
    for o, cl, sv in _batches(d, sizes, labels_on_device):
        acc.update(o, cl, sv, losses=losses)


def _reference_metrics(y_true, y_pred, y_prob, s_true, s_pred, n_bins=10):
    """evaluation/metrics.py:9-61 and evaluator.py:78-91 restated on fp64 arrays, with sklearn and scipy themselves."""
    from scipy.stats import spearmanr
    from sklearn.metrics import confusion_matrix, f1_score, precision_recall_fscore_support
    C = y_prob.shape[1]
    onehot = np.zeros_like(y_prob)
    onehot[np.arange(len(y_true)), y_true] = 1
    conf, hit = y_prob.max(1), (y_prob.argmax(1) == y_true).astype(float)
    ece, counts = 0.0, []
    edges = np.linspace(0, 1, n_bins + 1)
    for lo, hi in zip(edges[:-1], edges[1:]):
        m = (conf > lo) & (conf <= hi)
        counts.append(int(m.sum()))
        if m.mean() > 0:
            ece += abs(conf[m].mean() - hit[m].mean()) * m.mean()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        p, r, f, s = precision_recall_fscore_support(y_true, y_pred, labels=range(C), zero_division=0)
        return {'accuracy': float(np.mean(y_true == y_pred) * 100), 'macro_f1': float(f1_score(y_true, y_pred, average='macro') * 100),
                'weighted_f1': float(f1_score(y_true, y_pred, average='weighted') * 100), 'mae': float(np.mean(np.abs(s_true - s_pred))),
                'spearman_rho': float(spearmanr(s_true, s_pred)[0]), 'brier_score': float(np.mean(np.sum((y_prob - onehot) ** 2, axis=1))),
                'ece': float(ece), 'bin_counts': counts, 'confusion': confusion_matrix(y_true, y_pred, labels=range(C)),
                'precision': p * 100, 'recall': r * 100, 'f1': f * 100, 'support': s}


FLOATS = ('accuracy', 'macro_f1', 'weighted_f1', 'mae', 'brier_score', 'ece')


@pytest.mark.parametrize('n,C,sizes', [(257, 4, (1, 7, 64)), (4099, 4, (256, 1, 33, 1000)), (20000, 8, (4096, 1, 511))])
def test_kernels_against_the_reference_arithmetic(n, C, sizes):
    from rovit_hip import native as N
    from rovit_hip.evaluation import EvalAccumulator
    d = _data(n, C, seed=n)
    acc = EvalAccumulator(C, capacity=64)                 # grows by doubling several times
    _feed(acc, d, sizes)
    m, blk, a = acc.compute(), acc.result_block(), acc.arrays()
    soft = torch.softmax(d['logits'].double(), dim=1).numpy()
    perr = float(np.abs(a['y_probs'].astype(np.float64) - soft).max())
    print(f'N={n} C={C}: max |recorded probability - fp64 softmax| = {perr:.3e}')
    assert perr < 1e-5
    p64 = a['y_probs'].astype(np.float64)
    assert np.array_equal(a['y_pred'], p64.argmax(1)) and np.array_equal(a['y_true'], d['labels'].numpy())
    assert np.array_equal(a['severity_true'], d['sev_true'].float().numpy()) and np.array_equal(a['severity_pred'], d['sev_pred'].numpy())
    uerr = float(np.abs(a['uncertainty'] - torch.exp(0.5 * d['log_var'].double()).numpy()).max())
    assert uerr < 1e-5 * float(a['uncertainty'].max()), uerr
    ref = _reference_metrics(a['y_true'], a['y_pred'], p64, a['severity_true'].astype(np.float64), a['severity_pred'].astype(np.float64))
    assert np.array_equal(m['confusion_matrix'], ref['confusion'])
    assert [int(v) for v in blk[N.EVAL_BIN_COUNT:N.EVAL_BIN_COUNT + 10]] == ref['bin_counts'] and m['n'] == n
    for k in FLOATS:
        print(f'  {k}: {m[k]!r} reference {ref[k]!r} diff {abs(m[k] - ref[k]):.3e}')
        assert abs(m[k] - ref[k]) <= 1e-9, (k, m[k], ref[k])
    print(f"  spearman_rho: {m['spearman_rho']!r} reference {ref['spearman_rho']!r} diff {abs(m['spearman_rho'] - ref['spearman_rho']):.3e}")
    assert abs(m['spearman_rho'] - ref['spearman_rho']) <= 1e-12 and m['spearman'] == m['spearman_rho']
    for c in range(C):
        assert m['per_class'][c]['support'] == int(ref['support'][c])
        for k in ('precision', 'recall', 'f1'):
            assert abs(m['per_class'][c][k] - ref[k][c]) <= 1e-9, (c, k)


def test_result_block_is_bit_reproducible_and_independent_of_the_batch_split():
    from rovit_hip.evaluation import EvalAccumulator
    d = _data(4099, 4, seed=5, ties=True)
    loss = torch.tensor([0.25, 0.5, 0.125, 1.0, 1.875], device=dev())
    blocks = []
    for sizes, cap in (((256,), 4096), ((256,), 4096), ((1, 7, 300), 16), ((4099,), 8192)):
        acc = EvalAccumulator(4, capacity=cap)
        _feed(acc, d, sizes)
        blocks.append(acc.result_block().tobytes())
    assert blocks[0] == blocks[1], 'two runs of the same split differ'
    assert blocks[0] == blocks[2] == blocks[3], 'the result block depends on the batch split'
    # with losses the column sums are part of the block: two runs are byte-identical
    two = []
    for _ in range(2):
        acc = EvalAccumulator(4)
        _feed(acc, d, (100,), losses=loss)
        two.append(acc.result_block().tobytes())
        m = acc.compute()
    assert two[0] == two[1]
    assert (m['cls_loss'], m['ord_loss'], m['unc_loss'], m['kan_loss'], m['loss']) == (0.25, 0.5, 0.125, 1.0, 1.875)


@pytest.mark.parametrize('n', [1023, 1024, 1025])
def test_rho_with_ties_around_the_rank_tile(n):
    """The counting rank stages 1024 rows per LDS tile: a last tile one short, exactly full, and a single row in a new tile (there the
    row range is also split over two workgroups).  Tie-heavy columns, so both the `less` and the `equal` counts matter."""
    from scipy.stats import spearmanr
    from rovit_hip.evaluation import EvalAccumulator
    d = _data(n, 4, seed=n, ties=True)
    acc = EvalAccumulator(4)
    _feed(acc, d, (512,))
    m = acc.compute()
    want = float(spearmanr(d['sev_true'].numpy(), d['sev_pred'].double().numpy())[0])
    print(f"n={n}: rho {m['spearman_rho']!r} scipy {want!r} diff {abs(m['spearman_rho'] - want):.3e}")
    assert m['n'] == n and abs(m['spearman_rho'] - want) <= 1e-12
    again = EvalAccumulator(4)
    _feed(again, d, (1, 7, 300))
    assert again.result_block().tobytes() == acc.result_block().tobytes(), 'the result block depends on the batch split'


def test_ties_and_degenerate_inputs():
    from scipy.stats import spearmanr
    from rovit_hip.evaluation import EvalAccumulator
    d = _data(3001, 4, seed=9, ties=True)                 # integer severities 0..3 against predictions rounded to one decimal
    acc = EvalAccumulator(4)
    _feed(acc, d, (512,), labels_on_device=False)
    m = acc.compute()
    want = float(spearmanr(d['sev_true'].numpy(), d['sev_pred'].double().numpy())[0])
    print('rho with ties:', m['spearman_rho'], want)
    assert abs(m['spearman_rho'] - want) <= 1e-12
    # a constant column: NaN, as scipy
    const = dict(d, sev_pred=torch.full((3001,), 1.5))
    acc.reset()
    _feed(acc, const, (512,))
    assert np.isnan(acc.compute()['spearman_rho'])
    # a missing KAN head: the label stands in (evaluator.py:50-53): rho 1, MAE 0
    acc.reset()
    acc.update({'cls_logits': d['logits'].to(dev()), 'kan_severity': None, 'mu': None, 'log_var': None}, d['labels'], d['sev_true'])
    m = acc.compute()
    assert m['mae'] == 0.0 and abs(m['spearman_rho'] - 1.0) <= 1e-12 and acc.arrays()['uncertainty'] is None
    # one NaN prediction: rho is NaN, the classification and calibration metrics stay finite (the MAE is NaN, as numpy's mean is)
    bad = dict(d, sev_pred=d['sev_pred'].clone())
    bad['sev_pred'][1234] = float('nan')
    acc.reset()
    _feed(acc, bad, (512,))
    m = acc.compute()
    assert np.isnan(m['spearman_rho']) and np.isnan(m['mae'])
    assert all(np.isfinite(m[k]) for k in ('accuracy', 'macro_f1', 'weighted_f1', 'brier_score', 'ece'))


def test_evaluator_end_to_end_in_fp32_mode_matches_the_oracle(tmp_path):
    """The loader, seeds and oracle of tests/test_gpu_round2.py::test_evaluator_shaped_loop_reproduces_the_oracle_metrics; the metrics of
    Evaluator.evaluate() against those of the CPU oracle's predictions, that test's tolerance 1e-3 max(1, |ref|); arrays: classes equal,
    severity 1e-3, probabilities 1e-4."""
    from types import SimpleNamespace
    from data.dataset import create_dataloaders
    from data.transforms import original_transforms
    from evaluation.evaluator import Evaluator
    sd = ref_cpu.init_rovit_state(seed=23)
    model = _full_model(sd).eval()
    _, _, test_loader = create_dataloaders('data/Augmented Image', 'data/Original Image', CLASS_NAMES, SEVERITY,
                                           original_transform=original_transforms(), batch_size=8, synthetic=96, seed=7, device=dev())
    preds, labels, sev_p, sev_t, probs, unc = [], [], [], [], [], []
    with torch.no_grad():
        for images, class_labels, severity_labels in test_loader:
            o = ref_cpu.rovit_forward(images.cpu(), sd, 4)
            p = torch.softmax(o['cls_logits'], dim=1)
            preds.append(torch.argmax(p, dim=1).numpy())
            labels.append(class_labels.numpy())
            sev_p.append(o['kan_severity'].reshape(-1).numpy())
            sev_t.append(severity_labels.numpy())
            probs.append(p.numpy())
            unc.append(torch.exp(0.5 * o['log_var']).reshape(-1).numpy())
    ref = [np.concatenate(v) for v in (preds, labels, sev_p, sev_t, probs, unc)]
    mr = _reference_metrics(ref[1], ref[0], ref[4].astype(np.float64), ref[3].astype(np.float64), ref[2].astype(np.float64))
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=CLASS_NAMES, num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    model.backbone.model.precision = 'fp32'
    try:
        mg, a = Evaluator(model, test_loader, cfg, dev()).evaluate(return_arrays=True)
    finally:
        model.backbone.model.precision = 'bf16'
    assert len(a['y_true']) == 24 and np.array_equal(a['y_true'], ref[1]) and np.array_equal(a['y_pred'], ref[0])
    assert np.abs(a['severity_pred'] - ref[2]).max() < 1e-3 and np.abs(a['y_probs'] - ref[4]).max() < 1e-4
    assert np.abs(a['uncertainty'] - ref[5]).max() < 1e-4 and np.array_equal(a['severity_true'], ref[3].astype(np.float32))
    for k in FLOATS + ('spearman_rho',):
        print(k, mg[k], mr[k])
        assert abs(mg[k] - mr[k]) < 1e-3 * max(1.0, abs(mr[k])), (k, mg[k], mr[k])
    assert mg['fps'] > 0 and mg['params'] == sum(p.numel() for p in model.parameters() if p.requires_grad) and list(mg['per_class']) == CLASS_NAMES
    assert (tmp_path / 'evaluation_results.txt').exists()


def test_validate_matches_the_reference_shaped_loop():
    """training/trainer.py:183-231 restated (six .item() per batch) against validate() on the same model and the package's JointLoss: the
    five loss means within 1e-6 relative (fp32 per-batch values summed in fp64 against Python float sums of .item()), accuracy equal."""
    from data.dataset import create_dataloaders
    from data.transforms import original_transforms
    from rovit_hip.evaluation import validate
    from rovit_hip.losses import JointLoss
    model = _full_model(ref_cpu.init_rovit_state(seed=23))
    _, val_loader, _ = create_dataloaders('data/Augmented Image', 'data/Original Image', CLASS_NAMES, SEVERITY,
                                          original_transform=original_transforms(), batch_size=8, synthetic=96, seed=7, device=dev())
    loss_fn = JointLoss(1.0, 0.5, 0.5, 2.0, num_classes=4)
    model.train()
    got = validate(model, val_loader, loss_fn)
    assert not model.training
    sums, correct, total = [0.0] * 5, 0, 0
    with torch.no_grad():
        for images, class_labels, severity_labels in val_loader:
            images, class_labels, severity_labels = images.to(dev()), class_labels.to(dev()), severity_labels.to(dev())
            outputs = model(images)
            losses = loss_fn(outputs, class_labels, severity_labels, stage=4)
            for i, k in enumerate(('total_loss', 'cls_loss', 'ord_loss', 'unc_loss', 'kan_loss')):
                sums[i] += losses[k].item()
            _, predicted = outputs['cls_logits'].max(1)
            total += class_labels.size(0)
            correct += predicted.eq(class_labels).sum().item()
    nb = len(val_loader)
    want = dict(zip(('loss', 'cls_loss', 'ord_loss', 'unc_loss', 'kan_loss'), (s / nb for s in sums)))
    assert set(got) == set(want) | {'accuracy'}
    for k, v in want.items():
        print(k, got[k], v)
        assert abs(got[k] - v) <= 1e-6 * abs(v), (k, got[k], v)
    assert got['accuracy'] == 100. * correct / total


def test_update_never_synchronises_and_compute_copies_once(monkeypatch):
    from rovit_hip.evaluation import EvalAccumulator
    d = _data(1500, 4, seed=2)
    loss = {k: v for k, v in zip(('cls_loss', 'ord_loss', 'unc_loss', 'kan_loss', 'total_loss'), torch.arange(5.0, device=dev()).unbind(0))}
    acc = EvalAccumulator(4, capacity=32)
    _feed(acc, d, (8,))                                    # warm: allocator pools, code objects
    acc.result_block()
    acc.reset()
    on_device, on_host = _batches(d, (64, 1, 300)), _batches(d, (128,), labels_on_device=False)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for o, cl, sv in on_device:                       # growth by doubling inside
            acc.update(o, cl, sv, losses=loss)
        for o, cl, sv in on_host:                         # host labels: asynchronous copies
            acc.update(o, cl, sv)
        with pytest.raises(RuntimeError):                                    # compute() is where the epoch synchronises
            acc.compute()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    copies = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: (copies.append(tuple(self.shape)), real(self, *a, **k))[1])
    m = acc.compute()
    monkeypatch.undo()
    assert copies == [(272,)], copies                     # one device-to-host copy: the result block
    assert m['n'] == 3000 and np.isfinite(m['ece'])
