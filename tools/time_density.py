"""Time the feature-space density entry points and append one JSON line per (case, size, arm) to profiles/density_time.jsonl.

Device-resident fp32 feature rows, E = 192, C = 4, drawn like the backbone's (class means of norm 3, a covariance spectrum from 1 down to
1e-3, every row's mean removed: singular without shrinkage).

  --case fit    rows 4096 and 65536:   `ours` = FeatureDensity.update + fit (the row copy, four kernels, ONE device-to-host copy, covariance,
                two Cholesky factorisations and the condition number on the host in fp64, four table uploads) against `torch` = the recipe
                a user would write on the same device in fp32: one-hot means, centring, X^T @ X, torch.linalg.cholesky, solve_triangular,
                for the class-conditional and the background Gaussian.  The record carries the largest relative distance between the two
                arms' class distances on 256 rows, and each arm's against the fp64 reference.
  --case score  batch 256 and 65536:   `ours` = FeatureDensity.score with logits (one launch) against `torch` = two x @ W^T, the broadcast
                squared differences, min / argmin, logsumexp and softmax.
  --case ood    4096 + 4096 and 65536 + 65536 scores: `ours` = ood_metrics (three kernels, one copy) against `torch` = torch.sort of the
                concatenation, cumsum of the labels, trapezoid AUROC, average precision and FPR at 95 % TPR, one copy of the five numbers
                (no tie handling: continuous scores).

Every arm is warmed once; the arms alternate in one process; --repeats timed runs each; host clock between two device synchronisations;
median, min and max per arm.  No ratio is promised: the records say what was measured, whichever arm wins.

--kernels-only: five calls of `ours` per size for a separate ``rocprofv3 --kernel-trace --stats -- python tools/time_density.py --case
... --kernels-only`` run; --kernel-stats CSV appends the dens_* and ood_* rows of that run's kernel_stats.csv to the same .jsonl.
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

E, C, SHRINKAGE = 192, 4, 1e-3
SIZES = (4096, 65536)


def make_rows(n, seed=0):
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((C, E))
    mu *= 3.0 / np.linalg.norm(mu, axis=1, keepdims=True)
    Q, _ = np.linalg.qr(rng.standard_normal((E, E)))
    y = rng.integers(0, C, n)
    x = mu[y] + (rng.standard_normal((n, E)) * np.sqrt(np.geomspace(1.0, 1e-3, E))[None]) @ Q.T
    x -= x.mean(axis=1, keepdims=True)
    return x.astype(np.float32), y.astype(np.int64)


def torch_fit(x, y):
    n = x.shape[0]
    eye = torch.eye(E, device=x.device)
    onehot = torch.nn.functional.one_hot(y, C).float()
    means = (onehot.T @ x) / onehot.sum(0)[:, None]
    mean = x.mean(0)

    def whiten(centred, dof):
        cov = centred.T @ centred / dof
        cov = (1.0 - SHRINKAGE) * cov + SHRINKAGE * torch.trace(cov) / E * eye
        return torch.linalg.solve_triangular(torch.linalg.cholesky(cov), eye, upper=False)
    W, W0 = whiten(x - means[y], n - C), whiten(x - mean, n - 1)
    return {'whitening': W, 'class_means': means @ W.T, 'background_whitening': W0, 'background_mean': W0 @ mean}


def torch_score(x, t, logits):
    z, z0 = x @ t['whitening'].T, x @ t['background_whitening'].T
    d = ((z[:, None, :] - t['class_means'][None]) ** 2).sum(-1)
    d0 = ((z0 - t['background_mean'][None]) ** 2).sum(-1)
    m, arg = d.min(1)
    return {'class_distances': d, 'background_distance': d0, 'mahalanobis': m, 'nearest_class': arg, 'relative_mahalanobis': (d - d0[:, None]).min(1),
            'energy': -torch.logsumexp(logits, 1), 'max_prob_score': 1.0 - torch.softmax(logits, 1).max(1).values}


def torch_ood(a, b):
    s = torch.cat([a, b])
    pos = torch.cat([torch.zeros_like(a), torch.ones_like(b)]).double()
    order = torch.sort(s, descending=True).indices
    tp = torch.cumsum(pos[order], 0)
    fp = torch.cumsum(1.0 - pos[order], 0)
    tpr, fpr = tp / b.numel(), fp / a.numel()
    zero = torch.zeros(1, dtype=torch.float64, device=a.device)
    auroc = torch.trapezoid(torch.cat([zero, tpr]), torch.cat([zero, fpr]))
    ap_out = (pos[order] * tp / (tp + fp)).sum() / b.numel()
    rev = order.flip(0)                                       # the same cumsums from the other end
    tn = torch.cumsum(1.0 - pos[rev], 0)
    fn = torch.cumsum(pos[rev], 0)
    ap_in = ((1.0 - pos[rev]) * tn / (tn + fn)).sum() / a.numel()
    k = int(np.ceil(0.95 * a.numel()))
    t = torch.sort(a).values[k - 1]
    return torch.stack([auroc, ap_out, ap_in, (b <= t).double().mean(), t.double()]).cpu().tolist()


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
        rec = {'case': case, 'size': size, 'embed': E, 'classes': C, 'arm': name, 'median_ms': round(med[name], 3), 'min_ms': round(t[0], 3),
               'max_ms': round(t[-1], 3), 'repeats': len(t), 'device': torch.cuda.get_device_name(0)}
        if name == 'ours':
            rec.update(torch_over_ours=round(med['torch'] / med['ours'], 2), **extra)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def kernel_stats(path, out, case):
    with open(path) as f, open(out, 'a') as o:
        for row in csv.DictReader(f):
            m = re.search(r'(dens|ood)_[a-z]+_kernel(ILi\dE)?', row['Name'])
            if m:
                rec = {'case': 'kernel', 'of': case, 'kernel': m.group(0), 'calls': int(row['Calls']),
                       'avg_us': round(float(row['AverageNs']) / 1e3, 2), 'min_us': round(float(row['MinNs']) / 1e3, 2),
                       'max_us': round(float(row['MaxNs']) / 1e3, 2)}
                print(json.dumps(rec))
                o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', choices=('fit', 'score', 'ood'), required=True)
    ap.add_argument('--sizes', type=int, nargs='+')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--kernel-stats', metavar='CSV')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'density_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out, a.case)
    from rovit_hip import density as D
    dev = torch.device('cuda:0')
    sizes = a.sizes or ((256, 65536) if a.case == 'score' else SIZES)
    lines = []
    x_np, y_np = make_rows(max(max(sizes), 4096))
    x_all, y_all = torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)
    fitted = D.FeatureDensity(C, E)
    fitted.update(x_all[:4096], y_all[:4096])
    fitted.fit()
    logits_all = torch.randn(x_all.shape[0], C, device=dev) * 2.0
    for n in sizes:
        if a.case == 'fit':
            x, y = x_all[:n], y_all[:n]

            def ours():
                fd = D.FeatureDensity(C, E, capacity=n)
                fd.update(x, y)
                return fd.fit()
            arms, extra = {'ours': ours, 'torch': lambda: torch_fit(x, y)}, {}
            if not a.kernels_only:
                probe = x_np[:256]
                ref = D.score_reference(probe, D.density_reference(x_np[:n], y_np[:n], C, SHRINKAGE)['tables'])['class_distances']
                mine = ours().score(x[:256])['class_distances'].double().cpu().numpy()
                theirs = torch_score(x[:256], torch_fit(x, y), logits_all[:256])['class_distances'].double().cpu().numpy()
                rel = lambda u, v: float((np.abs(u - v) / v).max())
                extra = {'ours_vs_fp64': rel(mine, ref), 'torch_vs_fp64': rel(theirs, ref), 'ours_vs_torch': rel(mine, theirs)}
        elif a.case == 'score':
            x, lg = x_all[:n], logits_all[:n]
            tables = fitted.tables
            arms, extra = {'ours': lambda: fitted.score(x, lg), 'torch': lambda: torch_score(x, tables, lg)}, {}
            if not a.kernels_only:
                mine, theirs = fitted.score(x, lg), torch_score(x, tables, lg)
                extra = {'ours_vs_torch': float(((mine['class_distances'] - theirs['class_distances']).abs() / theirs['class_distances']).max()),
                         'nearest_class_agrees': float((mine['nearest_class'].long() == theirs['nearest_class']).double().mean())}
        else:
            g = torch.Generator().manual_seed(n)
            sa, sb = torch.randn(n, generator=g).to(dev), (torch.randn(n, generator=g) + 1.0).to(dev)
            arms, extra = {'ours': lambda: D.ood_metrics(sa, sb), 'torch': lambda: torch_ood(sa, sb)}, {}
            if not a.kernels_only:
                mine, theirs = D.ood_metrics(sa, sb), torch_ood(sa, sb)
                extra = {'auroc': mine['auroc'], 'auroc_distance': abs(mine['auroc'] - theirs[0]), 'aupr_out_distance': abs(mine['aupr_out'] - theirs[1]),
                         'aupr_in_distance': abs(mine['aupr_in'] - theirs[2]), 'fpr_distance': abs(mine['fpr_at_tpr'][0.95] - theirs[3])}
        if a.kernels_only:
            for _ in range(5):
                arms['ours']()
            torch.cuda.synchronize()
            print(f'kernels-only run done: {a.case} size = {n}')
            continue
        lines += records(a.case, n, time_arms(arms, a.repeats), extra)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
