"""Time the last-layer Laplace entry points and append one JSON line per (case, size, arm) to profiles/laplace_time.jsonl.

Device-resident fp32 feature rows, E = 192, hid = 128, C = 4 (the model's head shapes), rows drawn N(0, 1), the heads initialised as
torch.nn.Linear does, logits and log_var the heads' own.

  --case fit      rows 4096 and 65536: `ours` = HeadLaplace.update + fit (the row copies, the weight kernel, three gram kernels per head,
                  ONE device-to-host copy, eigenvalues, tau, Cholesky and the triangular inverse of both heads on the host in fp64, the
                  table uploads) against `torch` = the recipe a user would write on the same device in fp32: F.linear + relu, softmax, an
                  einsum for the K weighted Grams, the block assembly, torch.linalg.cholesky and solve_triangular at the SAME prior
                  precisions (the recipe has no evidence search; `ours` is timed with its search).  The record carries the largest
                  relative distance between the two arms' logit variances on 256 rows, and each arm's against the fp64 reference.
  --case predict  batch 256 and 65536: `ours` = HeadLaplace.predict with log_var (one launch per head) against `torch` = F.linear + relu,
                  the C products a @ W[:, block c]^T, an einsum for S, the probit softmax.

Every arm is warmed once; the arms alternate in one process; --repeats timed runs each; host clock between two device synchronisations;
median, min and max per arm.  No ratio is promised: the records say what was measured, whichever arm wins.

--kernels-only: five calls of `ours` per size for a separate ``rocprofv3 --kernel-trace --stats -- python tools/time_laplace.py --case
... --kernels-only`` run; --kernel-stats CSV appends the lap_* rows of that run's kernel_stats.csv to the same .jsonl.
"""
import argparse
import csv
import json
import math
import os
import re
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)

E, HID, C = 192, 128, 4
D, P = HID + 1, HID + 32


def make_heads(dev):
    torch.manual_seed(0)
    cls = SimpleNamespace(fc1=torch.nn.Linear(E, HID).to(dev), fc2=torch.nn.Linear(HID, C).to(dev))
    unc = SimpleNamespace(fc1=torch.nn.Linear(E, HID).to(dev), fc_mu=torch.nn.Linear(HID, 1).to(dev), fc_logvar=torch.nn.Linear(HID, 1).to(dev))
    return cls, unc


def head_outputs(cls, unc, x):
    with torch.no_grad():
        return cls.fc2(F.relu(cls.fc1(x))) * 4.0, unc.fc_logvar(F.relu(unc.fc1(x))).reshape(-1)


def augmented(fc1, x):
    h = F.relu(F.linear(x, fc1.weight, fc1.bias))
    return torch.cat([h, torch.ones(x.shape[0], 1, device=x.device)], dim=1)


def torch_whitening(H, tau):
    eye = torch.eye(H.shape[0], device=H.device)
    return torch.linalg.solve_triangular(torch.linalg.cholesky(H + tau * eye), eye, upper=False)


@torch.no_grad()
def torch_fit(cls, unc, x, lg, lv, tau, tau_mu):
    a = augmented(cls.fc1, x)
    p = torch.softmax(lg, dim=1)
    lam = torch.diag_embed(p) - p[:, :, None] * p[:, None, :]                 # (n, C, C)
    H = torch.einsum('ncd,na,nb->cadb', lam, a, a).reshape(C * D, C * D)
    am = augmented(unc.fc1, x)
    Hm = torch.einsum('n,na,nb->ab', torch.exp(-lv), am, am)
    return torch_whitening(H, tau), torch_whitening(Hm, tau_mu)


@torch.no_grad()
def torch_predict(cls, unc, x, lg, lv, W, Wm):
    a = augmented(cls.fc1, x)
    z = torch.stack([a @ W[:, c * D:(c + 1) * D].T for c in range(C)], dim=1)     # (B, C, C D)
    S = torch.einsum('bct,bdt->bcd', z, z)
    var = torch.diagonal(S, dim1=1, dim2=2)
    probs = torch.softmax(lg / torch.sqrt(1.0 + math.pi / 8.0 * var), dim=1)
    zm = augmented(unc.fc1, x) @ Wm.T
    mu_var = (zm * zm).sum(dim=1)
    return {'logit_cov': S, 'logit_var': var, 'probs': probs, 'confidence_score': 1.0 - probs.max(dim=1).values,
            'mean_logit_var': var.mean(dim=1), 'mu_var': mu_var, 'total_std': torch.sqrt(torch.exp(lv) + mu_var)}


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
        rec = {'case': case, 'size': size, 'embed': E, 'hid': HID, 'classes': C, 'arm': name, 'median_ms': round(med[name], 3),
               'min_ms': round(t[0], 3), 'max_ms': round(t[-1], 3), 'repeats': len(t), 'device': torch.cuda.get_device_name(0)}
        if name == 'ours':
            rec.update(torch_over_ours=round(med['torch'] / med['ours'], 2), **extra)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def kernel_stats(path, out, case):
    with open(path) as f, open(out, 'a') as o:
        for row in csv.DictReader(f):
            m = re.search(r'lap_[a-z]+_kernel(ILi\dE)?', row['Name'])
            if m:
                rec = {'case': 'kernel', 'of': case, 'kernel': m.group(0), 'calls': int(row['Calls']),
                       'avg_us': round(float(row['AverageNs']) / 1e3, 2), 'min_us': round(float(row['MinNs']) / 1e3, 2),
                       'max_us': round(float(row['MaxNs']) / 1e3, 2)}
                print(json.dumps(rec))
                o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', choices=('fit', 'predict'), required=True)
    ap.add_argument('--sizes', type=int, nargs='+')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--kernel-stats', metavar='CSV')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'laplace_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out, a.case)
    from rovit_hip import laplace as L
    dev = torch.device('cuda:0')
    sizes = a.sizes or ((256, 65536) if a.case == 'predict' else (4096, 65536))
    cls, unc = make_heads(dev)
    x_all = torch.randn(max(max(sizes), 4096), E, generator=torch.Generator().manual_seed(1)).to(dev)
    lg_all, lv_all = head_outputs(cls, unc, x_all)
    fitted = L.HeadLaplace((cls, unc))
    fitted.update(x_all[:4096], lg_all[:4096], lv_all[:4096])
    fitted.fit()
    lines = []
    for n in sizes:
        x, lg, lv = x_all[:n], lg_all[:n], lv_all[:n]
        extra = {}
        if a.case == 'fit':
            def ours():
                la = L.HeadLaplace((cls, unc), capacity=n)
                la.update(x, lg, lv)
                return la.fit()
            mine = ours()
            tau, tau_mu = mine.prior_precision, mine.prior_precision_mu
            arms = {'ours': ours, 'torch': lambda: torch_fit(cls, unc, x, lg, lv, tau, tau_mu)}
            if not a.kernels_only:
                q, ql, qv = x_all[:256], lg_all[:256], lv_all[:256]
                P_ = lambda t: t.detach().cpu().numpy()
                ref = L.laplace_reference(P_(x), P_(lg), P_(cls.fc1.weight), P_(cls.fc1.bias), np.concatenate([P_(cls.fc2.weight).ravel(), P_(cls.fc2.bias)]),
                                          prior_precision=tau)
                want = L.predict_reference(P_(q), P_(cls.fc1.weight), P_(cls.fc1.bias), ref['whitening64'], C)['logit_var']
                got = mine.predict(q, ql, log_var=qv)['logit_var'].double().cpu().numpy()
                W, Wm = torch_fit(cls, unc, x, lg, lv, tau, tau_mu)
                theirs = torch_predict(cls, unc, q, ql, qv, W, Wm)['logit_var'].double().cpu().numpy()
                rel = lambda u, v: float((np.abs(u - v) / v).max())
                extra = {'prior_precision': tau, 'status': mine.status, 'prior_precision_mu': tau_mu, 'status_mu': mine.status_mu,
                         'ours_vs_fp64': rel(got, want), 'torch_vs_fp64': rel(theirs, want), 'ours_vs_torch': rel(got, theirs)}
        else:
            W, Wm = torch_fit(cls, unc, x_all[:4096], lg_all[:4096], lv_all[:4096], fitted.prior_precision, fitted.prior_precision_mu)
            arms = {'ours': lambda: fitted.predict(x, lg, log_var=lv), 'torch': lambda: torch_predict(cls, unc, x, lg, lv, W, Wm)}
            if not a.kernels_only:
                mine, theirs = fitted.predict(x, lg, log_var=lv), torch_predict(cls, unc, x, lg, lv, W, Wm)
                extra = {'ours_vs_torch': float(((mine['logit_var'] - theirs['logit_var']).abs() / theirs['logit_var']).max()),
                         'argmax_agrees': float((mine['probs'].argmax(1) == theirs['probs'].argmax(1)).double().mean())}
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
