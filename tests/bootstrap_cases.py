"""Data shared by tests/test_evaluation_bootstrap_cpu.py and tests/test_gpu_evaluation_bootstrap.py: the generator of
tests/test_gpu_evaluation.py's ``_data`` and the deterministic pair of score cards of the paired-bootstrap tests."""
import math

import torch


def make_data(n, C, seed, ties=False):
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, C, (n,), generator=g)
    logits = torch.randn(n, C, generator=g) * 2.0
    logits[torch.arange(n), labels] += 1.5
    sev_true = torch.randint(0, 4, (n,), generator=g)
    sev_pred = (sev_true.float() + torch.randn(n, generator=g) * 0.8).clamp(0, 3)
    if ties:
        sev_pred = (sev_pred * 10).round() / 10
    return {'logits': logits, 'labels': labels, 'sev_true': sev_true, 'sev_pred': sev_pred}


def feed(acc, d, sizes=(1 << 30,), device=None):
    """Record ``d`` in batches of ``sizes`` (cycled) on ``device`` (None: the CPU path)."""
    to = (lambda t: t) if device is None else (lambda t: t.to(device))
    i, k, n = 0, 0, d['logits'].shape[0]
    while i < n:
        j = min(n, i + sizes[k % len(sizes)])
        k += 1
        acc.update({'cls_logits': to(d['logits'][i:j]), 'kan_severity': to(d['sev_pred'][i:j].reshape(-1, 1)), 'mu': None, 'log_var': None},
                   to(d['labels'][i:j]), to(d['sev_true'][i:j]))
        i = j
    return acc


PAIR_N, PAIR_C, PAIR_R, PAIR_SEED = 600, 4, 200, 11


def exact_data(n, C, seed):
    """Score cards whose recorded probabilities do not depend on who computes the softmax.  A row's logits are 0 on m in 1..C classes and
    -200 on the rest: exp(0) is 1, exp(-200) underflows to 0 in fp32, the sum m is exact, and 1 / m is one IEEE division (or the same
    value as 1 * fl(1 / m)), so every fp32 softmax gives exactly 1/m and 0, and the first argmax is the first of the m classes.  The
    confidences 1, 1/2, 1/3, 1/4 fall in four calibration bins, so Brier score and ECE are not trivial."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, C, (n,), generator=g)
    m = torch.randint(1, C + 1, (n,), generator=g)
    score = torch.rand(n, C, generator=g)
    boost = torch.rand(n, generator=g) < 0.6                 # the label is among the m classes in six rows of ten, and by chance
    score[torch.arange(n)[boost], labels[boost]] += 1.0
    rank = score.argsort(dim=1, descending=True).argsort(dim=1)
    logits = torch.where(rank < m[:, None], torch.zeros(n, C), torch.full((n, C), -200.0))
    sev_true = torch.randint(0, 4, (n,), generator=g)
    sev_pred = (sev_true.float() + torch.randn(n, generator=g) * 0.8).clamp(0, 3)
    return {'logits': logits, 'labels': labels, 'sev_true': sev_true, 'sev_pred': sev_pred}


def _improved(a, n):
    """The same logits, made right on the first ceil(0.1 n) rows that a gets wrong, and a better severity prediction."""
    b = {k: v.clone() for k, v in a.items()}
    wrong = (a['logits'].argmax(1) != a['labels']).nonzero().reshape(-1)
    fix = wrong[:math.ceil(0.1 * n)]
    assert len(fix) == math.ceil(0.1 * n), 'model a must be wrong on at least 10 % of the rows'
    b['logits'][fix] = -200.0
    b['logits'][fix, b['labels'][fix]] = 0.0
    b['sev_pred'] = (a['sev_pred'] + a['sev_true'].float()) / 2
    return b


def paired_data():
    """Model a: ``exact_data(600, 4, seed=41)``.  Model b: the same, right on 60 more rows.  Deterministic, and both models' recorded
    probabilities are the same bits on the host and on the device (``exact_data``): the paired-bootstrap tests compare the two paths'
    bootstrap, not two roundings of expf."""
    a = exact_data(PAIR_N, PAIR_C, seed=41)
    return a, _improved(a, PAIR_N)


def paired_data_random_logits():
    """The same pair on ``make_data``'s random logits, whose fp32 softmax differs in the last bit between expf on the device and
    torch.softmax on the host: for comparisons on ONE side's recorded arrays."""
    a = make_data(PAIR_N, PAIR_C, seed=41)
    return a, _improved(a, PAIR_N)
