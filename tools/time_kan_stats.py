"""Time the KAN edge statistics three ways and append one JSON line per (case, arm) to profiles/kan_stats_time.jsonl.

  fused  : KANEdgeStats.update (chunks of --update-rows feature rows) + compute: the head's trajectory, one rovit_kan_edge_stats call per
           layer, ONE device-to-host copy, the statistics derived on the host
  recipe : what a user would write in torch on the same device.  Per layer, in chunks of 1 024 rows: BSplineBasis.compute_basis(tanh(x)),
           an einsum to (rows, in, out), the linear term added, then the same reductions (sum phi, sum phi^2, sum |phi|, sum |s|, sum z,
           sum z^2, sum |a|, interval counts with bucketize) accumulated in fp64 and copied to the host at the end
  floor  : get_activation_trajectory alone on the same rows, one synchronisation

Cases: N = --rows feature rows resident on the device, the default head ([192, 64, 16, 1], 5 knots) and the 32-knot one.  Every case is
warmed up; the arms alternate (fused, recipe, floor, fused, ...); each arm runs at least --repeats times and --min-seconds in all; host
clock between two device synchronisations.  median, min, max and spread per arm; recipe / fused and fused - floor from the medians.

--kernels-only N --knots K: the fused arm alone, five times, for one configuration, for a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_kan_stats.py --kernels-only N --knots K`` run (no counters in that run);
--kernel-stats CSV N --knots K appends the kan_* kernels' rows of that run's kernel_stats.csv to the same .jsonl: calls, and the kernel's
total over the head's three layers per compute() (the run's total / 5).
"""
import argparse
import csv
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)

CONFIGS = (([192, 64, 16, 1], 5), ([192, 64, 16, 1], 32))


def build(layers, num_knots, n, dev):
    from models.kan import KANSeverityModule
    from oracle import ref_cpu
    g = torch.Generator().manual_seed(n + num_knots)
    m = KANSeverityModule(layers, num_knots, 3)
    m.load_state_dict(ref_cpu.init_kan_state(layers, num_knots, 3, g))
    return m.to(dev).eval(), (torch.randn(n, layers[0], generator=g) * 1.5).to(dev)


def fused(m, x, rows):
    from rovit_hip.kan_stats import KANEdgeStats
    acc = KANEdgeStats(m, capacity=x.shape[0])
    for i in range(0, x.shape[0], rows):
        acc.update(x[i:i + rows])
    return acc.compute()


def recipe(m, x, chunk=1024):
    from models.kan import BSplineBasis
    out = []
    with torch.no_grad():
        traj = m.get_activation_trajectory(x)
        for layer, a in zip(m.kan_layers, traj):
            W, lw, lb, kn = layer.spline_weights, layer.linear.weight, layer.linear.bias, layer.knots
            nk = kn.numel()
            e = torch.zeros(4, layer.in_features, layer.out_features, dtype=torch.float64, device=x.device)
            pre = torch.zeros(2, layer.out_features, dtype=torch.float64, device=x.device)
            sabs = torch.zeros(layer.in_features, dtype=torch.float64, device=x.device)
            occ = torch.zeros(layer.in_features, nk, dtype=torch.int64, device=x.device)
            cols = torch.arange(layer.in_features, device=x.device).unsqueeze(0)
            for r0 in range(0, a.shape[0], chunk):
                xa = a[r0:r0 + chunk]
                xn = torch.tanh(xa)
                s = torch.einsum('nik,ijk->nij', BSplineBasis.compute_basis(xn, kn), W)
                phi = s + xa.unsqueeze(2) * lw.t().unsqueeze(0)
                e[0] += phi.sum(0, dtype=torch.float64)
                e[1] += (phi * phi).sum(0, dtype=torch.float64)
                e[2] += phi.abs().sum(0, dtype=torch.float64)
                e[3] += s.abs().sum(0, dtype=torch.float64)
                z = phi.sum(1) + lb
                pre[0] += z.sum(0, dtype=torch.float64)
                pre[1] += (z * z).sum(0, dtype=torch.float64)
                sabs += xa.abs().sum(0, dtype=torch.float64)
                t = (torch.bucketize(xn.clamp(kn[0], kn[-1]), kn, right=True) - 1).clamp(0, nk - 1)
                occ.view(-1).index_add_(0, (cols * nk + t).reshape(-1), torch.ones(t.numel(), dtype=torch.int64, device=x.device))
            out.append([v.cpu() for v in (e, pre, sabs, occ)])
    return out


def floor(m, x):
    with torch.no_grad():
        m.get_activation_trajectory(x)
    torch.cuda.synchronize()


def time_arms(arms, repeats, min_seconds, warmup):
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    times = {k: [] for k in arms}
    while min(len(v) for v in times.values()) < repeats or min(sum(v) for v in times.values()) < min_seconds:
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    return times


def records(case, times):
    med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}
    out = []
    for name, v in times.items():
        t = sorted(x * 1e3 for x in v)
        rec = dict(case, arm=name, median_ms=round(med[name], 3), min_ms=round(t[0], 3), max_ms=round(t[-1], 3),
                   spread_ms=round(t[-1] - t[0], 3), repeats=len(t), device=torch.cuda.get_device_name(0))
        if name == 'fused':
            rec['recipe_over_fused'] = round(med['recipe'] / med['fused'], 2)
            rec['fused_minus_floor_ms'] = round(med['fused'] - med['floor'], 3)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


KERNEL_RUNS = 5


def config_of(num_knots):
    return next(c for c in CONFIGS if c[1] == num_knots)


def kernels_only(n, rows, num_knots):
    dev = torch.device('cuda:0')
    layers, nk = config_of(num_knots)
    m, x = build(layers, nk, n, dev)
    for _ in range(KERNEL_RUNS):
        fused(m, x, rows)
    torch.cuda.synchronize()
    print('kernels-only run done: n =', n, 'knots =', nk)


def kernel_stats(path, n, num_knots, out):
    layers, nk = config_of(num_knots)
    with open(path) as f, open(out, 'a') as o:
        for row in csv.DictReader(f):
            if 'kan_edge_kernel' in row['Name'] or 'kan_pre_kernel' in row['Name'] or 'kan_fold_kernel' in row['Name']:
                name = row['Name'].split('::')[-1].split('(')[0]
                rec = {'case': 'kernel', 'layers': layers, 'num_knots': nk, 'rows': n, 'kernel': name, 'calls': int(row['Calls']),
                       'per_compute_us': round(float(row['TotalDurationNs']) / 1e3 / KERNEL_RUNS, 2),
                       'min_us': round(float(row['MinNs']) / 1e3, 2), 'max_us': round(float(row['MaxNs']) / 1e3, 2)}
                print(json.dumps(rec))
                o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[4096, 65536])
    ap.add_argument('--update-rows', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--kernels-only', type=int, default=0, metavar='N')
    ap.add_argument('--kernel-stats', nargs=2, metavar=('CSV', 'N'))
    ap.add_argument('--knots', type=int, default=5, choices=[c[1] for c in CONFIGS], help='configuration of the two kernel modes')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kan_stats_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats[0], int(a.kernel_stats[1]), a.knots, a.out)
    if a.kernels_only:
        return kernels_only(a.kernels_only, a.update_rows, a.knots)
    dev = torch.device('cuda:0')
    lines = []
    for layers, nk in CONFIGS:
        for n in a.rows:
            m, x = build(layers, nk, n, dev)
            arms = {'fused': lambda: fused(m, x, a.update_rows), 'recipe': lambda: recipe(m, x), 'floor': lambda: floor(m, x)}
            times = time_arms(arms, a.repeats, a.min_seconds, a.warmup)
            lines += records({'case': 'kan_stats', 'layers': layers, 'num_knots': nk, 'rows': n, 'update_rows': a.update_rows}, times)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
