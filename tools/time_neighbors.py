"""Time the nearest-neighbour entry points and append one JSON line per (case, size, arm) to profiles/neighbors_time.jsonl.

Device-resident fp32 feature rows, E = 192, k = 10, metric cosine, drawn like the backbone's (class means of norm 3, a covariance spectrum
from 1 down to 1e-3, every row's mean removed).

  --case build   4096 and 65536 recorded rows: `ours` = FeatureIndex.build (one launch: norms, flags, the normalised copy, the counts)
                 against `torch` = torch.nn.functional.normalize of the same rows.
  --case search  (B, N) in {(256, 4096), (256, 65536), (65536, 65536)}: `ours` = FeatureIndex.search on a built index (three kernels, no
                 (B, N) tensor) against `torch` = the recipe a user would write on the same device: normalise the queries, `q @ r.T` against
                 the normalised rows in chunks of --chunk queries (a (chunk, N) fp32 block each), `torch.topk(1 - sim, k, largest=False)`.
                 The record carries the share of queries whose index SETS agree between the two arms (the recipe has no tie rule and its
                 reduction order depends on the shape, so the sets may differ where two distances are a rounding apart) and the bytes of
                 the recipe's largest temporary.

Every arm is warmed once; the arms alternate in one process; --repeats timed runs each; host clock between two device synchronisations;
median, min and max per arm.  No ratio is promised: the records say what was measured, whichever arm wins.

--kernels-only: five calls of `ours` per size for a separate ``rocprofv3 --kernel-trace --stats -- python tools/time_neighbors.py --case
... --kernels-only`` run; --kernel-trace CSV appends, per size, the median of the kernels' five launches in that run's kernel_trace.csv to
the same .jsonl.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)

E, C, K = 192, 4, 10
BUILD_SIZES = (4096, 65536)
SEARCH_SIZES = ((256, 4096), (256, 65536), (65536, 65536))


def make_rows(n, seed=0):
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((C, E))
    mu *= 3.0 / np.linalg.norm(mu, axis=1, keepdims=True)
    Q, _ = np.linalg.qr(rng.standard_normal((E, E)))
    y = rng.integers(0, C, n)
    x = mu[y] + (rng.standard_normal((n, E)) * np.sqrt(np.geomspace(1.0, 1e-3, E))[None]) @ Q.T
    x -= x.mean(axis=1, keepdims=True)
    return x.astype(np.float32)


def torch_search(q, r_hat, chunk):
    qn = torch.nn.functional.normalize(q, dim=1)
    dist, idx = [], []
    for r0 in range(0, q.shape[0], chunk):
        d, i = torch.topk(1.0 - qn[r0:r0 + chunk] @ r_hat.T, K, dim=1, largest=False)
        dist.append(d)
        idx.append(i)
    return torch.cat(dist), torch.cat(idx)


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


def records(case, size, times, extra):
    out = []
    med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}
    for name, v in times.items():
        t = sorted(x * 1e3 for x in v)
        rec = {'case': case, 'size': size, 'embed': E, 'k': K, 'arm': name, 'median_ms': round(med[name], 3), 'min_ms': round(t[0], 3),
               'max_ms': round(t[-1], 3), 'repeats': len(t), 'device': torch.cuda.get_device_name(0)}
        if name == 'ours':
            rec.update(torch_over_ours=round(med['torch'] / med['ours'], 2), **extra)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def kernel_times(path, out, case):
    """Per size, the median / min / max of the search and merge kernels' launches in a --kernels-only run's kernel_trace.csv: the launches
    in start order, five per size."""
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp']))
    sizes = BUILD_SIZES if case == 'build' else SEARCH_SIZES
    with open(out, 'a') as o:
        for kernel in ('knn_rows_kernel',) if case == 'build' else ('knn_search_kernel', 'knn_merge_kernel'):
            us = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows if kernel in r['Kernel_Name']]
            if len(us) != 5 * len(sizes):
                raise SystemExit(f'{path}: {len(us)} launches of {kernel}, expected {5 * len(sizes)}')
            for i, size in enumerate(sizes):
                t = sorted(us[5 * i:5 * i + 5])
                rec = {'case': 'kernel', 'of': case, 'size': list(size) if isinstance(size, tuple) else size, 'kernel': kernel, 'calls': 5,
                       'median_us': round(t[2], 2), 'min_us': round(t[0], 2), 'max_us': round(t[-1], 2)}
                print(json.dumps(rec))
                o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', choices=('build', 'search'), required=True)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--chunk', type=int, default=4096, help="queries per block of the recipe's q @ r.T (4096 x 65536 fp32 = 1 GiB)")
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--kernel-trace', metavar='CSV')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'neighbors_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.kernel_trace:
        return kernel_times(a.kernel_trace, a.out, a.case)
    from rovit_hip import neighbors as NB
    dev = torch.device('cuda:0')
    rows_all = torch.from_numpy(make_rows(65536, seed=0)).to(dev)
    queries_all = torch.from_numpy(make_rows(65536, seed=1)).to(dev)
    lines = []
    sizes = BUILD_SIZES if a.case == 'build' else SEARCH_SIZES
    for size in sizes:
        if a.case == 'build':
            fi = NB.FeatureIndex(E, None, 'cosine', capacity=size)
            fi.update(rows_all[:size])
            rows = rows_all[:size]
            arms, extra = {'ours': fi.build, 'torch': lambda: torch.nn.functional.normalize(rows, dim=1)}, {}
            if not a.kernels_only:
                extra = {'counts': fi.build().counts(),
                         'max_abs_difference': float((fi._normalized - torch.nn.functional.normalize(rows, dim=1)).abs().max())}
        else:
            B, N = size
            fi = NB.FeatureIndex(E, None, 'cosine', capacity=N)
            fi.update(rows_all[:N])
            fi.build()
            q, r_hat = queries_all[:B], torch.nn.functional.normalize(rows_all[:N], dim=1)
            chunk = a.chunk
            arms, extra = {'ours': lambda: fi.search(q, k=K), 'torch': lambda: torch_search(q, r_hat, chunk)}, {}
            if not a.kernels_only:
                mine, theirs = fi.search(q, k=K)['indices'].long().sort(dim=1).values, torch_search(q, r_hat, chunk)[1].sort(dim=1).values
                extra = {'index_sets_agree': float((mine == theirs).all(dim=1).double().mean()),
                         'torch_temporary_bytes': 4 * min(chunk, B) * N, 'ours_workspace_bytes': int(NB.native.load().rovit_knn_workspace_bytes(B, N, E, K))}
        if a.kernels_only:
            for _ in range(5):
                arms['ours']()
            torch.cuda.synchronize()
            print(f'kernels-only run done: {a.case} size = {size}')
            continue
        lines += records(a.case, list(size) if isinstance(size, tuple) else size, time_arms(arms, a.repeats), extra)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
