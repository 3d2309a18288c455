"""Time the bootstrap of the score card and append one JSON line per (case, arm) to profiles/bootstrap_time.jsonl.

  bootstrap : EvalAccumulator.bootstrap(R) on device-resident rows, from scratch: the finalise, rovit_eval_bootstrap, ONE device-to-host
              copy, the summaries on the host
  compute   : the bare compute() on the same rows (the finalise and its copy): the floor bootstrap() cannot go below
  host      : the recipe a user would write without the kernel: arrays() once, then per replicate a numpy resample
              (Generator.integers) and the seven metrics of this repository's evaluation.metrics.  It is timed over --host-resamples
              replicates per repeat and scaled to R (the replicates are independent and cost the same); the record says so.
  sklearn   : the same recipe with sklearn / scipy, only where they import.

Cases: --rows device-resident rows (4 096: H in LDS; 65 536: H in the workspace), C = 4, 10 bins, R = --resamples.  Every arm is warmed
once; the arms alternate in one process; --repeats timed runs each; host clock between two device synchronisations.  median, min and
max per arm; the ratios from the medians.  Nothing here promises a speed-up: the ratios are what was measured.

--kernels-only: no host arm; five bootstrap() calls per case for a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_bootstrap.py --kernels-only`` run; --kernel-stats CSV appends the eval_* rows of that
run's kernel_stats.csv to the same .jsonl.
"""
import argparse
import csv
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)


def make_accumulator(n, dev):
    from rovit_hip.evaluation import EvalAccumulator
    g = torch.Generator().manual_seed(n)
    labels = torch.randint(0, 4, (n,), generator=g)
    logits = torch.randn(n, 4, generator=g) * 2.0
    logits[torch.arange(n), labels] += 1.5
    sev = (labels.float() + torch.randn(n, generator=g) * 0.8).clamp(0, 3).reshape(-1, 1)
    acc = EvalAccumulator(4, capacity=n)
    acc.update({'cls_logits': logits.to(dev), 'kan_severity': sev.to(dev), 'mu': None, 'log_var': None}, labels.to(dev), labels.to(dev))
    return acc


def forget(acc):
    """Drop the cached finalise, so that the next call pays for all of its work."""
    acc._block = acc._block_dev = acc._rank_counts = None


def host_recipe(acc, resamples, seed, use_sklearn=False):
    from evaluation import metrics as M
    a = acc.arrays()
    y, p, prob, st, sp = a['y_true'], a['y_pred'], a['y_probs'], a['severity_true'], a['severity_pred']
    rng = np.random.default_rng(seed)
    rows = []
    if use_sklearn:
        from scipy.stats import spearmanr
        from sklearn.metrics import accuracy_score, f1_score
    for _ in range(resamples):
        i = rng.integers(0, len(y), len(y))
        if use_sklearn:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                rows.append((accuracy_score(y[i], p[i]) * 100, f1_score(y[i], p[i], average='macro') * 100,
                             f1_score(y[i], p[i], average='weighted') * 100, M.mae(st[i], sp[i]), spearmanr(st[i], sp[i])[0],
                             M.brier_score(y[i], prob[i]), M.ece(y[i], prob[i])))
        else:
            rows.append((M.accuracy(y[i], p[i]), M.macro_f1(y[i], p[i]), M.weighted_f1(y[i], p[i]), M.mae(st[i], sp[i]),
                         M.spearman_rho(st[i], sp[i]), M.brier_score(y[i], prob[i]), M.ece(y[i], prob[i])))
    t = np.asarray(rows)
    return t.std(axis=0, ddof=1), np.nanquantile(t, [0.025, 0.975], axis=0)


def time_arms(arms, repeats):
    for fn in arms.values():                                 # the warm run
        fn()
    times = {k: [] for k in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    return times


def kernel_stats(path, out):
    with open(path) as f, open(out, 'a') as o:
        for row in csv.DictReader(f):
            if 'eval_' in row['Name']:
                rec = {'case': 'kernel', 'kernel': row['Name'].split('::')[-1].split('(')[0], 'calls': int(row['Calls']),
                       'avg_us': round(float(row['AverageNs']) / 1e3, 2), 'min_us': round(float(row['MinNs']) / 1e3, 2),
                       'max_us': round(float(row['MaxNs']) / 1e3, 2)}
                print(json.dumps(rec))
                o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[4096, 65536])
    ap.add_argument('--resamples', type=int, default=1000)
    ap.add_argument('--host-resamples', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--kernel-stats', metavar='CSV')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bootstrap_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out)
    from rovit_hip import native
    dev = torch.device('cuda:0')
    have_sklearn = True
    try:
        import scipy.stats  # noqa: F401
        import sklearn.metrics  # noqa: F401
    except ImportError:
        have_sklearn = False
    lines = []
    for n in a.rows:
        acc = make_accumulator(n, dev)
        if a.kernels_only:
            for _ in range(5):
                forget(acc)
                acc.bootstrap(a.resamples)
            torch.cuda.synchronize()
            print(f'kernels-only run done: rows = {n}, resamples = {a.resamples}')
            continue
        R, Rh = a.resamples, min(a.host_resamples, a.resamples)
        arms = {'bootstrap': lambda: (forget(acc), acc.bootstrap(R)), 'compute': lambda: (forget(acc), acc.compute()),
                'host': lambda: host_recipe(acc, Rh, 0)}
        if have_sklearn:
            arms['sklearn'] = lambda: host_recipe(acc, Rh, 0, use_sklearn=True)
        times = time_arms(arms, a.repeats)
        scale = {'bootstrap': 1.0, 'compute': 1.0, 'host': R / Rh, 'sklearn': R / Rh}
        med = {k: sorted(v)[len(v) // 2] * 1e3 * scale[k] for k, v in times.items()}
        for name, v in times.items():
            t = sorted(x * 1e3 * scale[name] for x in v)
            rec = {'case': 'bootstrap', 'rows': n, 'classes': 4, 'bins': 10, 'resamples': R, 'h_path': 'lds' if n <= native.EVAL_BOOT_LDS_ROWS
                   else 'workspace', 'arm': name, 'median_ms': round(med[name], 3), 'min_ms': round(t[0], 3), 'max_ms': round(t[-1], 3),
                   'repeats': len(t), 'device': torch.cuda.get_device_name(0)}
            if name in ('host', 'sklearn'):
                rec['timed_resamples'] = Rh
                rec['scaled_to_resamples'] = R
            if name == 'bootstrap':
                rec['host_over_bootstrap'] = round(med['host'] / med['bootstrap'], 2)
                rec['bootstrap_over_compute'] = round(med['bootstrap'] / med['compute'], 2)
                rec['bootstrap_minus_compute_us_per_replicate_row'] = round((med['bootstrap'] - med['compute']) * 1e3 / (R * n), 6)
                if 'sklearn' in med:
                    rec['sklearn_over_bootstrap'] = round(med['sklearn'] / med['bootstrap'], 2)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
