"""Time the selective-prediction score card and append one JSON line per (case, arm) to profiles/selective_time.jsonl.

  selective : EvalAccumulator.selective() on device-resident rows: nothing is cached between calls, so every call pays for the seven
              kernels of rovit_eval_selective, ONE device-to-host copy and the dict on the host
  compute   : the bare compute() on the same rows, from scratch (the finalise and its copy): the floor of a call that ranks and copies
  torch     : the recipe a user would write on the same device: per score one torch.sort, per (score, risk) pair an fp64 cumsum and the
              tie handling (unique_consecutive group bounds), the oracle pairs the same way, one copy of the results
  numpy     : arrays() and selective_reference on the host (the columns through selective_columns)

Cases: --rows device-resident rows, C = 4, the three built-in scores (confidence, entropy, sigma), two risks (error, abs_err), P = 20.
Every arm is warmed once; the arms alternate in one process; --repeats timed runs each; host clock between two device synchronisations.
median, min and max per arm; the ratios from the medians.  Nothing here promises a speed-up: the ratios are what was measured.

--kernels-only: five selective() calls per case for a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_selective.py --kernels-only`` run; --kernel-stats CSV appends the sel_* rows of that
run's kernel_stats.csv to the same .jsonl (pass the same --rows to both, one size per profiled run, and the record carries it).
"""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)

P = 20


def make_accumulator(n, dev):
    from rovit_hip.evaluation import EvalAccumulator
    g = torch.Generator().manual_seed(n)
    labels = torch.randint(0, 4, (n,), generator=g)
    logits = torch.randn(n, 4, generator=g) * 2.0
    logits[torch.arange(n), labels] += 1.5
    sev = (labels.float() + torch.randn(n, generator=g) * 0.8).clamp(0, 3).reshape(-1, 1)
    mu = labels.float() + torch.randn(n, generator=g) * 0.6
    log_var = torch.log((mu - labels.float()).abs() + 0.1) + torch.randn(n, generator=g) * 0.5
    acc = EvalAccumulator(4, capacity=n)
    acc.update({'cls_logits': logits.to(dev), 'kan_severity': sev.to(dev), 'mu': mu.reshape(-1, 1).to(dev), 'log_var': log_var.reshape(-1, 1).to(dev)},
               labels.to(dev), labels.to(dev))
    return acc


def forget(acc):
    """Drop the cached finalise, so that the next compute() pays for all of its work."""
    acc._block = acc._block_dev = acc._rank_counts = None


def torch_curve(u, l, kp):
    """AURC and the P curve points of one pair on the device: sort, fp64 cumsum, tie groups through unique_consecutive."""
    n = u.shape[0]
    us, order = torch.sort(u, stable=True)
    pref = torch.cat([torch.zeros(1, dtype=torch.float64, device=u.device), torch.cumsum(l[order].double(), 0)])
    _, inverse, counts = torch.unique_consecutive(us, return_inverse=True, return_counts=True)
    starts = torch.cumsum(counts, 0) - counts
    g, m = starts[inverse], counts[inverse]
    k = torch.arange(1, n + 1, device=u.device)
    r = (pref[g] + (k - g) * (pref[g + m] - pref[g]) / m) / k
    return torch.cat([r.sum().reshape(1) / n, r[kp - 1], us[kp - 1].double()])


def torch_recipe(acc):
    n = acc.n
    rec = acc._rec
    probs = rec['probs'][:n]
    keys = [1 - probs.max(dim=1)[0], -(torch.where(probs > 0, probs * torch.log(probs), torch.zeros_like(probs))).sum(dim=1), rec['uncertainty'][:n]]
    risks = [(rec['pred'][:n] != rec['label'][:n]).float(), (rec['sev_true'][:n] - rec['sev_pred'][:n]).abs()]
    kp = torch.from_numpy((np.arange(1, P + 1) * n + P - 1) // P).to(probs.device)
    out = []
    for l in risks:
        out.append(torch_curve(l, l, kp))
        for u in keys:
            out.append(torch_curve(u, l, kp))
    return torch.stack(out).cpu()


def numpy_recipe(acc):
    from rovit_hip.evaluation import selective_columns, selective_reference
    a = acc.arrays()
    arrays = {'probs': a['y_probs'], 'pred': a['y_pred'], 'label': a['y_true'], 'sev_true': a['severity_true'], 'sev_pred': a['severity_pred'],
              'uncertainty': a['uncertainty']}
    keys, risks = selective_columns(arrays, {}, ['confidence', 'entropy', 'sigma'], ['error', 'abs_err'])
    return selective_reference(keys, risks, P)


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


def kernel_stats(path, out, rows):
    with open(path) as f, open(out, 'a') as o:
        for row in csv.DictReader(f):
            if 'sel_' in row['Name']:
                rec = {'case': 'kernel', 'rows': rows, 'kernel': re.search(r'sel_[a-z_]+', row['Name']).group(0), 'calls': int(row['Calls']),
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'selective_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out, a.rows[0] if len(a.rows) == 1 else a.rows)
    dev = torch.device('cuda:0')
    lines = []
    for n in a.rows:
        acc = make_accumulator(n, dev)
        if a.kernels_only:
            for _ in range(5):
                acc.selective(coverages=P)
            torch.cuda.synchronize()
            print(f'kernels-only run done: rows = {n}')
            continue
        # the arms agree before they are timed: the torch recipe's AURC of (sigma, error) against the kernel's
        card, recipe = acc.selective(coverages=P), torch_recipe(acc)
        assert abs(card['scores']['sigma']['error']['aurc'] - float(recipe[3, 0])) <= n * 2.0 ** -50, 'the torch recipe computes another AURC'
        arms = {'selective': lambda: acc.selective(coverages=P), 'compute': lambda: (forget(acc), acc.compute()),
                'torch': lambda: torch_recipe(acc), 'numpy': lambda: numpy_recipe(acc)}
        times = time_arms(arms, a.repeats)
        med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}
        for name, v in times.items():
            t = sorted(x * 1e3 for x in v)
            rec = {'case': 'selective', 'rows': n, 'classes': 4, 'scores': 3, 'risks': 2, 'coverages': P, 'arm': name,
                   'median_ms': round(med[name], 3), 'min_ms': round(t[0], 3), 'max_ms': round(t[-1], 3), 'repeats': len(t),
                   'device': torch.cuda.get_device_name(0)}
            if name == 'selective':
                rec.update(selective_over_compute=round(med['selective'] / med['compute'], 2), torch_over_selective=round(med['torch'] / med['selective'], 2),
                           numpy_over_selective=round(med['numpy'] / med['selective'], 2))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
