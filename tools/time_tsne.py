"""Time exact t-SNE and append one JSON line per (size, arm) to profiles/tsne_time.jsonl.

Device-resident fp32 feature rows, E = 192, drawn like the backbone's (class means of norm 3, a covariance spectrum from 1 down to
1e-3, every row's mean removed); perplexity 30, 1 000 iterations of which 250 exaggerated, n = 1 024, 4 096 and 16 384.

  ours     `TSNE(init=Y0).fit_transform(rows)`: affinities and descent in csrc/tsne.hip, nothing copied to the host.
  torch    the recipe a user would write on the same device, the same algorithm in dense fp32 torch ops: `torch.cdist` squared, the
           64-step bisection as tensor ops over all rows at once, the symmetrised P, and per iteration the classic matrix form
           num = 1 / (1 + |y_i|^2 + |y_j|^2 - 2 Y Y^T), PQ = alpha P num - num^2 / sum num, g = 4 (rowsum(PQ) Y - PQ Y), the gains rule.
  sklearn  `sklearn.manifold.TSNE` (Barnes-Hut, on the host, the device-to-host copy included) if and only if `import sklearn` works:
           context, never required.
Both device arms start from the same explicit init (the 'pca' init computed once, outside the timed region).  Every arm is warmed
once; the arms alternate in one process; --repeats timed runs each; host clock between two device synchronisations; median, min and
max per arm.  The record of `ours` carries the final KL divergence of both arms (each recomputed from its own map by the torch
recipe's formula on the device) and the 10-NN preservation of both maps.  No ratio is promised: the records say what was measured.

--kernels-only N: one `ours` run at n = N with --iterations iterations, for a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_tsne.py --kernels-only N`` run.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)

E, C = 192, 4
SIZES = (1024, 4096, 16384)
PERPLEXITY, EXAGGERATION, EXAGGERATION_ITER = 30.0, 12.0, 250


def make_rows(n, seed=0):
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((C, E))
    mu *= 3.0 / np.linalg.norm(mu, axis=1, keepdims=True)
    Q, _ = np.linalg.qr(rng.standard_normal((E, E)))
    y = rng.integers(0, C, n)
    x = mu[y] + (rng.standard_normal((n, E)) * np.sqrt(np.geomspace(1.0, 1e-3, E))[None]) @ Q.T
    x -= x.mean(axis=1, keepdims=True)
    return x.astype(np.float32)


def torch_affinities(x):
    n = x.shape[0]
    D = torch.cdist(x, x).pow_(2)
    D.fill_diagonal_(float('inf'))
    D -= D.min(dim=1, keepdim=True).values
    D.fill_diagonal_(0.0)
    log_u = math.log(PERPLEXITY)
    beta = torch.ones(n, device=x.device)
    lo, hi = torch.full_like(beta, -float('inf')), torch.full_like(beta, float('inf'))
    for step in range(65):
        W = torch.exp(-beta[:, None] * D)
        W.fill_diagonal_(0.0)
        S = W.sum(dim=1)
        if step == 64:
            break
        H = torch.log(S) + beta * (D * W).sum(dim=1) / S
        up = H > log_u
        lo, hi = torch.where(up, beta, lo), torch.where(up, hi, beta)
        beta = torch.where(up, torch.where(torch.isinf(hi), beta * 2, (beta + hi) / 2), torch.where(torch.isinf(lo), beta / 2, (beta + lo) / 2))
    W /= S[:, None]
    P = ((W + W.T) / (2 * n)).clamp_(min=1e-12)
    P.fill_diagonal_(0.0)
    return P


def torch_num(Y):
    sq = (Y * Y).sum(dim=1)
    num = 1.0 / (1.0 + (sq[:, None] + sq[None, :] - 2.0 * (Y @ Y.T)).clamp_(min=0.0))
    num.fill_diagonal_(0.0)
    return num


def torch_kl(P, Y):
    num = torch_num(Y)
    Q = (num / num.sum()).clamp_(min=1e-30)
    return float((P * (torch.log(P.clamp(min=1e-30)) - torch.log(Q))).double().sum())


def torch_tsne(x, Y0, n_iter):
    n = x.shape[0]
    P = torch_affinities(x)
    Y, V, G = Y0.clone(), torch.zeros_like(Y0), torch.ones_like(Y0)
    eta = max(n / EXAGGERATION / 4.0, 50.0)
    for t in range(n_iter):
        alpha, m = (EXAGGERATION, 0.5) if t < EXAGGERATION_ITER else (1.0, 0.8)
        num = torch_num(Y)
        PQ = alpha * P * num - num * num / num.sum()
        g = 4.0 * (PQ.sum(dim=1)[:, None] * Y - PQ @ Y)
        G = torch.where(V * g < 0, G + 0.2, G * 0.8).clamp_(min=0.01)
        V = m * V - eta * G * g
        Y = Y + V
    return Y - Y.mean(dim=0)


def sklearn_tsne(x, n_iter):
    from sklearn.manifold import TSNE as SK
    kw = {'perplexity': PERPLEXITY, 'init': 'pca', 'learning_rate': 'auto', 'random_state': 0}
    try:
        return SK(max_iter=n_iter, **kw).fit_transform(x.cpu().numpy())
    except TypeError:                                                # older releases name it n_iter
        return SK(n_iter=n_iter, **kw).fit_transform(x.cpu().numpy())


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--iterations', type=int, default=1000)
    ap.add_argument('--sizes', type=int, nargs='*', default=list(SIZES))
    ap.add_argument('--kernels-only', type=int, metavar='N')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tsne_time.jsonl'))
    a = ap.parse_args()
    from rovit_hip import embedding as EM
    dev = torch.device('cuda:0')
    rows_all = torch.from_numpy(make_rows(max(SIZES + (a.kernels_only or 0,)), seed=0)).to(dev)
    if a.kernels_only:
        x = rows_all[:a.kernels_only].contiguous()
        EM.TSNE(perplexity=PERPLEXITY, n_iter=a.iterations, init=EM.pca_init(x)).fit_transform(x)
        torch.cuda.synchronize()
        print(f'kernels-only run done: n = {a.kernels_only}, {a.iterations} iterations')
        return
    try:
        import sklearn  # noqa: F401
        have_sklearn = True
    except ImportError:
        have_sklearn = False
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for n in a.sizes:
        x = rows_all[:n].contiguous()
        Y0 = EM.pca_init(x)
        ours = EM.TSNE(perplexity=PERPLEXITY, n_iter=a.iterations, early_exaggeration=EXAGGERATION, exaggeration_iter=EXAGGERATION_ITER, init=Y0)
        arms = {'ours': lambda: ours.fit_transform(x), 'torch': lambda: torch_tsne(x, Y0, a.iterations)}
        if have_sklearn:
            arms['sklearn'] = lambda: sklearn_tsne(x, a.iterations)
        times = time_arms(arms, a.repeats)
        mine, theirs = ours.fit_transform(x), torch_tsne(x, Y0, a.iterations)
        P = ours.affinities(x)['P']
        extra = {'kl_ours': round(torch_kl(P, mine), 4), 'kl_torch': round(torch_kl(P, theirs), 4), 'kl_trace_last': round(ours.kl_divergence_, 4),
                 'knn_preservation_ours': round(EM.knn_preservation(x, mine), 4), 'knn_preservation_torch': round(EM.knn_preservation(x, theirs), 4),
                 'status': ours.status_}
        del P
        med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}
        with open(a.out, 'a') as f:
            for name, v in times.items():
                t = sorted(s * 1e3 for s in v)
                rec = {'n': n, 'embed': E, 'perplexity': PERPLEXITY, 'iterations': a.iterations, 'arm': name, 'median_ms': round(med[name], 2),
                       'min_ms': round(t[0], 2), 'max_ms': round(t[-1], 2), 'repeats': len(t), 'device': torch.cuda.get_device_name(0)}
                if name == 'ours':
                    rec.update(torch_over_ours=round(med['torch'] / med['ours'], 2), **extra)
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
