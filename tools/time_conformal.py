"""Time split conformal prediction and append one JSON line per (case, arm) to profiles/conformal_time.jsonl.

  conformal : EvalAccumulator.conformal() on device-resident rows: the ten kernels of rovit_eval_conformal, ONE device-to-host copy and
              the Conformal on the host
  evaluate  : Conformal.evaluate() of the same rows: the two kernels of rovit_eval_conformal_apply, one copy, the dict on the host
  compute   : the bare compute() on the same rows, from scratch (the finalise and its copy): the floor of a call that launches and copies
  torch_fit : the recipe a user would write on the same device: sort of the probabilities, cumsum, gather, the six score columns, and
              torch.kthvalue per column and group (a boolean mask per class with class_conditional), one copy of the thresholds
  torch_eval: the same scores for every candidate class, the comparison with the thresholds, coverage and set sizes, one copy
  numpy     : arrays() and conformal_reference on the host

Cases: --rows device-resident rows, C = 4, the six default scores, one level (alpha = 0.1), with and without class_conditional.
Every arm is warmed once; the arms alternate in one process; --repeats timed runs each; host clock between two device synchronisations.
median, min and max per arm; the ratios from the medians.  Nothing here promises a speed-up: the ratios are what was measured.

--kernels-only: five conformal() and evaluate() calls per case for a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_conformal.py --kernels-only`` run; --kernel-stats CSV appends the conf_* rows of
that run's kernel_stats.csv to the same .jsonl (pass the same --rows to both, one size per profiled run, and the record carries it).
"""
import argparse
import csv
import json
import os
import re
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)
from tools.time_selective import forget, time_arms  # noqa: E402

ALPHA, LAMBDA, K_REG = 0.1, 0.01, 1


def make_accumulator(n, dev, seed=0):
    from rovit_hip.evaluation import EvalAccumulator
    g = torch.Generator().manual_seed(n + seed)
    labels = torch.randint(0, 4, (n,), generator=g)
    logits = torch.randn(n, 4, generator=g) * 2.0
    logits[torch.arange(n), labels] += 1.5
    sev = (labels.float() + torch.randn(n, generator=g) * 0.8).clamp(0, 3).reshape(-1, 1)
    mu = labels.float() + torch.randn(n, generator=g) * 0.6
    log_var = torch.log((mu - labels.float()).abs() + 0.1) + torch.randn(n, generator=g) * 0.5
    acc = EvalAccumulator(4, capacity=n)
    acc.update({'cls_logits': logits.to(dev), 'kan_severity': sev.to(dev), 'mu': mu.reshape(-1, 1).to(dev), 'log_var': log_var.reshape(-1, 1).to(dev)},
               labels.to(dev), labels.to(dev), extra={'mu': mu.reshape(-1, 1).to(dev)})
    return acc


def torch_class_scores(probs, u):
    """(lac, aps, raps) for every candidate class, (n, C) each: sort, cumsum, the rank through a second argsort, gather."""
    ps, order = torch.sort(probs, dim=1, descending=True, stable=True)
    rank = torch.argsort(order, dim=1)
    cum = torch.gather(torch.cumsum(ps, dim=1), 1, rank)
    aps = cum - u[:, None] * probs
    return 1 - probs, aps, aps + LAMBDA * (rank + 1 - K_REG).clamp_min(0)


def torch_columns(acc):
    n, rec = acc.n, acc._rec
    y = rec['label'][:n].long()
    u = torch.rand(n, device=y.device)
    cols = [s.gather(1, y[:, None]).reshape(-1) for s in torch_class_scores(rec['probs'][:n], u)]
    res = (rec['sev_true'][:n] - acc._extra['mu'][:n]).abs()
    return cols + [(rec['sev_true'][:n] - rec['sev_pred'][:n]).abs(), res, res / rec['uncertainty'][:n]], y, u


def kth(v):
    n = v.shape[0]
    k = n + 1 - (n + 1) // 10
    return torch.kthvalue(v, k)[0] if k <= n else torch.full((), float('inf'), device=v.device)


def torch_fit(acc, class_conditional):
    cols, y, _ = torch_columns(acc)
    out = [kth(c) for c in cols]
    if class_conditional:
        for c in range(acc.num_classes):
            mask = y == c
            out += [kth(col[mask]) for col in cols]          # a boolean mask: one synchronisation per class and column
    return torch.stack(out).cpu()


def torch_eval(acc, thresholds):
    n, rec = acc.n, acc._rec
    y = rec['label'][:n].long()
    u = torch.rand(n, device=y.device)
    out = []
    for s, q in zip(torch_class_scores(rec['probs'][:n], u), thresholds[:3]):
        inside = s <= q
        size = inside.sum(dim=1)
        hit = inside.gather(1, y[:, None]).reshape(-1)
        out += [hit.float().mean(), size.float().mean(), (size == 1).float().mean()]
        out += list(torch.zeros(acc.num_classes + 1, device=y.device).index_add_(0, size, torch.ones(n, device=y.device)))
    res = (rec['sev_true'][:n] - acc._extra['mu'][:n]).abs()
    for v, q in zip(((rec['sev_true'][:n] - rec['sev_pred'][:n]).abs(), res, res / rec['uncertainty'][:n]), thresholds[3:]):
        out.append((v <= q).float().mean())
    out.append(rec['uncertainty'][:n].double().mean().float())
    return torch.stack(out).cpu()


def numpy_recipe(acc, class_conditional):
    from rovit_hip.evaluation import conformal_reference
    a = acc.arrays()
    return conformal_reference(a, {'mu': acc._extra_column('mu')}, acc.num_classes, (ALPHA,), ('lac', 'aps', 'raps', 'kan_abs', 'mu_abs', 'mu_scaled'),
                               class_conditional=class_conditional)['block']


def kernel_stats(path, out, rows):
    with open(path) as f, open(out, 'a') as o:
        for row in csv.DictReader(f):
            if 'conf_' in row['Name']:
                rec = {'case': 'kernel', 'rows': rows, 'kernel': re.search(r'conf_[a-z_]+', row['Name']).group(0), 'calls': int(row['Calls']),
                       'avg_us': round(float(row['AverageNs']) / 1e3, 2), 'min_us': round(float(row['MinNs']) / 1e3, 2),
                       'max_us': round(float(row['MaxNs']) / 1e3, 2)}
                print(json.dumps(rec))
                o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[4096, 65536])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--kernel-stats', metavar='CSV')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conformal_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out, a.rows[0] if len(a.rows) == 1 else a.rows)
    dev = torch.device('cuda:0')
    lines = []
    for n in a.rows:
        acc, test = make_accumulator(n, dev), make_accumulator(n, dev, seed=1)
        for cc in (False, True):
            if a.kernels_only:
                for _ in range(5):
                    acc.conformal(alphas=(ALPHA,), class_conditional=cc).evaluate(test)
                torch.cuda.synchronize()
                print(f'kernels-only run done: rows = {n}, class_conditional = {cc}')
                continue
            # the arms agree before they are timed: 'lac' draws nothing and is one IEEE subtraction, so its thresholds are the same bits
            cp, recipe = acc.conformal(alphas=(ALPHA,), class_conditional=cc), torch_fit(acc, cc)
            lac = cp.thresholds['lac'][ALPHA]
            assert float(recipe[0]) == float(lac[0] if cc else lac), 'the torch recipe finds another threshold'
            thresholds = [float(recipe[m]) for m in range(6)]
            arms = {'conformal': lambda: acc.conformal(alphas=(ALPHA,), class_conditional=cc), 'evaluate': lambda: cp.evaluate(test),
                    'compute': lambda: (forget(acc), acc.compute()), 'torch_fit': lambda: torch_fit(acc, cc),
                    'torch_eval': lambda: torch_eval(test, thresholds), 'numpy': lambda: numpy_recipe(acc, cc)}
            times = time_arms(arms, a.repeats)
            med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}
            for name, v in times.items():
                t = sorted(x * 1e3 for x in v)
                rec = {'case': 'conformal', 'rows': n, 'classes': 4, 'scores': 6, 'levels': 1, 'class_conditional': cc, 'arm': name,
                       'median_ms': round(med[name], 3), 'min_ms': round(t[0], 3), 'max_ms': round(t[-1], 3), 'repeats': len(t),
                       'device': torch.cuda.get_device_name(0)}
                if name == 'conformal':
                    rec.update(conformal_over_compute=round(med['conformal'] / med['compute'], 2),
                               torch_fit_over_conformal=round(med['torch_fit'] / med['conformal'], 2),
                               numpy_over_conformal=round(med['numpy'] / med['conformal'], 2))
                if name == 'evaluate':
                    rec.update(evaluate_over_compute=round(med['evaluate'] / med['compute'], 2),
                               torch_eval_over_evaluate=round(med['torch_eval'] / med['evaluate'], 2))
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
