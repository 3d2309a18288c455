"""Time the training-data influence entry points and append one JSON line per (case, size, arm) to profiles/influence_time.jsonl.

Device-resident fp32 rows for the default heads (E = 192, hid = 128, C = 4, so a whitened gradient is N = 640 wide), k = 10, a Laplace fit
on the first 4096 rows; the features are drawn like the backbone's (tools/time_neighbors.py), the logits are the head's own.

  --case embed   4096 and 65536 rows: `ours` = HeadInfluence.update of the classification head (one rovit_influence_embed launch) against
                 `torch` = the recipe a user would write on the same device: a = [relu(fc1 f + b1); 1], r = softmax(l) - onehot(y),
                 g = (r[:, :, None] * a[:, None, :]) flattened and padded, u = g @ W.T.
  --case search  (B, n) in {(256, 4096), (256, 65536), (65536, 65536)}: `ours` = HeadInfluence.search (the queries' embed launch, the
                 search and the merge kernel; no (B, n) tensor) against `torch` = the recipe's embed of the queries, `q @ u.T` in chunks of
                 --chunk queries (a (chunk, n) fp32 block each) and `torch.topk` at both ends.  The record carries the share of queries
                 whose proponent and opponent index SETS agree between the arms (the recipe has no tie rule and another summation order)
                 and the bytes of the recipe's largest temporaries.

Every arm is warmed once; the arms alternate in one process; --repeats timed runs each; host clock between two device synchronisations;
median, min and max per arm.  Nothing about speed is promised: the records say what was measured, whichever arm wins.

--kernels-only: five calls of `ours` per size for a separate ``rocprofv3 --kernel-trace --stats -- python tools/time_influence.py --case
... --kernels-only`` run; --kernel-trace CSV appends, per size, the median of the kernels' five launches in that run's kernel_trace.csv to
the same .jsonl.
"""
import argparse
import csv
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)

E, HID, C, K = 192, 128, 4, 10
P = HID + 32
N = C * P
EMBED_SIZES = (4096, 65536)
SEARCH_SIZES = ((256, 4096), (256, 65536), (65536, 65536))
KERNELS = {'embed': ('inf_embed_kernel',), 'search': ('inf_search_kernel', 'inf_merge_kernel')}


def make_rows(n, seed=0):
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((C, E))
    mu *= 3.0 / np.linalg.norm(mu, axis=1, keepdims=True)
    Q, _ = np.linalg.qr(rng.standard_normal((E, E)))
    y = rng.integers(0, C, n)
    x = mu[y] + (rng.standard_normal((n, E)) * np.sqrt(np.geomspace(1.0, 1e-3, E))[None]) @ Q.T
    x -= x.mean(axis=1, keepdims=True)
    return x.astype(np.float32), y.astype(np.int32)


def torch_embed(x, lg, y, w1, b1, W):
    a = torch.cat([torch.relu(x @ w1.T + b1), torch.ones((x.shape[0], 1), device=x.device)], dim=1)
    r = torch.softmax(lg, dim=1)
    r[torch.arange(x.shape[0], device=x.device), y.long()] -= 1.0
    g = torch.nn.functional.pad(r[:, :, None] * a[:, None, :], (0, P - a.shape[1])).reshape(x.shape[0], N)
    return g @ W.T


def torch_search(q, u, chunk):
    pro, opp = [], []
    for r0 in range(0, q.shape[0], chunk):
        s = q[r0:r0 + chunk] @ u.T
        pro.append(torch.topk(s, K, dim=1)[1])
        opp.append(torch.topk(s, K, dim=1, largest=False)[1])
    return torch.cat(pro), torch.cat(opp)


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
        rec = {'case': case, 'size': size, 'embed': E, 'hid': HID, 'classes': C, 'dim': N, 'k': K, 'arm': name, 'median_ms': round(med[name], 3),
               'min_ms': round(t[0], 3), 'max_ms': round(t[-1], 3), 'repeats': len(t), 'device': torch.cuda.get_device_name(0)}
        if name == 'ours':
            rec.update(torch_over_ours=round(med['torch'] / med['ours'], 2), **extra)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def kernel_times(path, out, case):
    """Per size, the median / min / max of the kernels' launches in a --kernels-only run's kernel_trace.csv: the launches in start order,
    five per size."""
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp']))
    sizes = EMBED_SIZES if case == 'embed' else SEARCH_SIZES
    with open(out, 'a') as o:
        for kernel in KERNELS[case]:
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
    ap.add_argument('--case', choices=('embed', 'search'), required=True)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--chunk', type=int, default=4096, help="queries per block of the recipe's q @ u.T (4096 x 65536 fp32 = 1 GiB)")
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--kernel-trace', metavar='CSV')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'influence_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.kernel_trace:
        return kernel_times(a.kernel_trace, a.out, a.case)
    from rovit_hip import influence as INF
    from rovit_hip import laplace as LAP
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    head = SimpleNamespace(fc1=torch.nn.Linear(E, HID).to(dev), fc2=torch.nn.Linear(HID, C).to(dev))
    x_np, y_np = make_rows(65536, seed=0)
    q_np, yq_np = make_rows(65536, seed=1)
    x_all, y_all, q_all, yq_all = (torch.from_numpy(v).to(dev) for v in (x_np, y_np, q_np, yq_np))
    with torch.no_grad():
        logits = lambda f: 4.0 * head.fc2(torch.relu(head.fc1(f)))
        lg_all, lgq_all = logits(x_all), logits(q_all)
    la = LAP.HeadLaplace(head, capacity=4096)
    la.update(x_all[:4096], lg_all[:4096])
    la.fit()
    t = la.tables
    w1, b1, W = t['fc1_weight'], t['fc1_bias'], t['whitening']
    lines = []
    for size in EMBED_SIZES if a.case == 'embed' else SEARCH_SIZES:
        n = size if a.case == 'embed' else size[1]
        x, lg, y = x_all[:n], lg_all[:n], y_all[:n]
        inf = INF.HeadInfluence(la, capacity=n)

        def ours_embed():
            inf.reset()
            inf.update(x, lg, y)
        if not (a.kernels_only and a.case == 'embed'):          # a search needs the rows; the trace of an embed run counts launches
            ours_embed()
        extra = {}
        if a.case == 'embed':
            arms = {'ours': ours_embed, 'torch': lambda: torch_embed(x, lg, y, w1, b1, W)}
            if not a.kernels_only:
                extra = {'counts': inf.counts(), 'max_abs_difference': float((inf.rows() - torch_embed(x, lg, y, w1, b1, W)).abs().max()),
                         'torch_temporary_bytes': 2 * 4 * n * N, 'ours_bytes': 4 * n * N}
        else:
            B = size[0]
            q, lq, yq = q_all[:B], lgq_all[:B], yq_all[:B]
            u, chunk = inf.rows(), a.chunk
            arms = {'ours': lambda: inf.search(q, lq, yq, k=K), 'torch': lambda: torch_search(torch_embed(q, lq, yq, w1, b1, W), u, chunk)}
            if not a.kernels_only:
                mine, theirs = inf.search(q, lq, yq, k=K), torch_search(torch_embed(q, lq, yq, w1, b1, W), u, chunk)
                same = lambda m, th: float((m.long().sort(dim=1).values == th.sort(dim=1).values).all(dim=1).double().mean())
                extra = {'proponent_sets_agree': same(mine['pro_indices'], theirs[0]), 'opponent_sets_agree': same(mine['opp_indices'], theirs[1]),
                         'torch_temporary_bytes': 4 * min(chunk, B) * n + 2 * 4 * B * N,
                         'ours_workspace_bytes': int(INF.native.load().rovit_influence_workspace_bytes(B, n, N, K)) + 4 * B * N}
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
