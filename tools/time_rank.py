"""Time the counting rank against the sorted rank and append one JSON line per (case, rows, method) to profiles/rank_time.jsonl.
ROVIT_RANK_SORT_ROWS (include/rovit_hip.h, native.RANK_SORT_ROWS) is read off this file's ``crossover`` record.

  rank      : the bare rank_columns() of ONE device-resident fp32 column (values rounded to two decimals: ties)
  compute   : EvalAccumulator.compute() from scratch on device-resident rows (the finalise, its copy and the dict)
  selective : EvalAccumulator.selective() with the three built-in scores and two risks, P = 20 (tools/time_selective.py's case)
  ood       : ood_metrics() of rows + rows scores, where 2 rows <= 2^20 (tools/time_density.py's case)
  torch     : at --recipe-rows only, the recipes the README names for selective (torch.sort + cumsum per pair) and ood_metrics

Rows: 2^10 .. 2^20 in powers of two, device-resident.  ``count`` and ``sort`` alternate in one process; every arm is warmed once; --repeats
timed runs each, host clock between two device synchronisations; median, min and max per arm.  The blocks of the two methods are
compared before they are timed.  crossover: per consumer the smallest measured rows from which on, at every larger measured size too,
the SLOWEST sort repeat beats the FASTEST count repeat; the constant is the largest of the three (2^20 + 1 when sort never wins).
Nothing here promises a speed-up: the records are what was measured.

--kernels-only: five compute(), selective() and ood_metrics() calls of each method at --rows (behind the one call each of the agreement
check) for a separate ``rocprofv3 --kernel-trace --stats -- python tools/time_rank.py --kernels-only --rows 65536`` run; --kernel-stats CSV
appends that run's rank and sort kernels to the same .jsonl (pass the same --rows; the kernel names tell the method).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)
from time_density import torch_ood  # noqa: E402
from time_selective import P, forget, make_accumulator, torch_recipe  # noqa: E402

METHODS = ('count', 'sort')
RANK_KERNELS = r'(sort_[a-z_]+|rank_[a-z_]+|sel_rank_kernel|sel_perm_kernel|eval_rank_count_kernel|ood_rank_kernel)'


def column(n, seed):
    rng = np.random.default_rng([seed, n])
    return torch.from_numpy(rng.standard_normal(n).round(2).astype(np.float32))


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


def cases(n, dev):
    """{case: {arm: callable}} for n rows, after checking that the two methods agree."""
    from rovit_hip.density import ood_block, ood_metrics
    from rovit_hip.rank import rank_columns
    x = column(n, 0).to(dev)
    acc = make_accumulator(n, dev)

    def with_method(m, fn):
        def run():
            acc.rank_method = m
            return fn()
        return run
    out = {'rank': {m: (lambda m=m: rank_columns(x, method=m)) for m in METHODS},
           'compute': {m: with_method(m, lambda: (forget(acc), acc.compute())) for m in METHODS},
           'selective': {m: with_method(m, lambda: acc.selective(coverages=P)) for m in METHODS}}
    a, b = rank_columns(x, method='count'), rank_columns(x, method='sort')
    assert all(torch.equal(u, v) for u, v in zip(a, b)), 'rank_columns: the methods disagree'
    blocks = []
    for m in METHODS:
        acc.rank_method = m
        forget(acc)
        blocks.append((acc.result_block().copy(), acc.selective(coverages=P, return_keys=True)['block']))
    assert np.array_equal(blocks[0][0], blocks[1][0]) and np.array_equal(blocks[0][1], blocks[1][1]), 'the score cards disagree'
    if 2 * n <= 1 << 20:
        s_in, s_out = column(n, 1).to(dev), (column(n, 2) + 1.0).to(dev)
        assert np.array_equal(ood_block(s_in, s_out, rank='count'), ood_block(s_in, s_out, rank='sort')), 'the OOD cards disagree'
        out['ood'] = {m: (lambda m=m: ood_metrics(s_in, s_out, rank=m)) for m in METHODS}
        out['ood_torch'] = {'torch': lambda: torch_ood(s_in, s_out)}
    out['selective_torch'] = {'torch': lambda: torch_recipe(acc)}
    return out


def crossover(records):
    """Per consumer the smallest measured rows from which the slowest sort repeat beats the fastest count repeat at every measured size."""
    res = {}
    for case in ('compute', 'selective', 'ood'):
        rows = sorted({r['rows'] for r in records if r['case'] == case})
        wins = {n: next(r['max_ms'] for r in records if r['case'] == case and r['rows'] == n and r['method'] == 'sort') <
                next(r['min_ms'] for r in records if r['case'] == case and r['rows'] == n and r['method'] == 'count') for n in rows}
        first = None
        for n in reversed(rows):
            if not wins[n]:
                break
            first = n
        res[case] = first
    const = None if any(v is None for v in res.values()) else max(res.values())
    return {'case': 'crossover', 'first_rows_sort_wins': res, 'rank_sort_rows': const if const is not None else (1 << 20) + 1}


def kernel_stats(path, out, rows):
    with open(path) as f, open(out, 'a') as o:
        for row in csv.DictReader(f):
            m = re.search(RANK_KERNELS, row['Name'])
            if m:
                rec = {'case': 'kernel', 'rows': rows, 'kernel': m.group(0), 'calls': int(row['Calls']),
                       'avg_us': round(float(row['AverageNs']) / 1e3, 2), 'min_us': round(float(row['MinNs']) / 1e3, 2),
                       'max_us': round(float(row['MaxNs']) / 1e3, 2)}
                print(json.dumps(rec))
                o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[1 << k for k in range(10, 21)])
    ap.add_argument('--recipe-rows', type=int, default=65536)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--kernel-stats', metavar='CSV')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rank_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out, a.rows[0] if len(a.rows) == 1 else a.rows)
    dev = torch.device('cuda:0')
    records = []
    for n in a.rows:
        arms = cases(n, dev)
        if a.kernels_only:
            for case in ('compute', 'selective', 'ood'):
                for m in METHODS if case in arms else ():
                    for _ in range(5):
                        arms[case][m]()
            torch.cuda.synchronize()
            print(f'kernels-only run done: rows = {n}')
            continue
        for case, fns in arms.items():
            if case.endswith('_torch') and n != a.recipe_rows:
                continue
            for name, v in time_arms(fns, a.repeats).items():
                t = sorted(x * 1e3 for x in v)
                rec = {'case': case, 'rows': n, 'method': name, 'median_ms': round(t[len(t) // 2], 3), 'min_ms': round(t[0], 3),
                       'max_ms': round(t[-1], 3), 'repeats': len(t), 'device': torch.cuda.get_device_name(0)}
                print(json.dumps(rec), flush=True)
                records.append(rec)
    if not a.kernels_only:
        records.append(crossover(records))
        print(json.dumps(records[-1]), flush=True)
        with open(a.out, 'a') as f:
            for rec in records:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
