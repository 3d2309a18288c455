"""Time the KAN grid extension two ways and append one JSON line per (case, arm) to profiles/kan_grid_time.jsonl.

  fused  : KANRegrid.update (chunks of --update-rows feature rows) + fit: per layer rovit_kan_regrid_moments, rovit_kan_regrid_solve and
           the layer forward to the next layer's rows; ONE device-to-host copy, the diagnostics
  recipe : what a user would write in torch on the same device.  Per layer, in chunks of 1 024 rows: BSplineBasis.compute_basis(tanh(x))
           on both grids, einsums to the per-input moments in fp64, the same prior added, torch.linalg.solve, c' = T c, the layer forward
           with the new coefficients (the module's own kernel) and ReLU; the new coefficients' largest magnitude copied to the host

Cases: N = --rows feature rows resident on the device, the default head [192, 64, 16, 1]: 5 -> 12 knots and 32 -> 58 knots, cover layout.
One warm run of both arms, then the arms alternate (fused, recipe, fused, ...) seven times each; host clock between two device
synchronisations; median with min and max.  Peak extra device memory of each arm: torch.cuda.max_memory_allocated over one run minus what
was allocated before it.

--kernels-only N --case K: the fused arm alone, five times, for one case, for a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_kan_grid.py --kernels-only N --case K`` run (no counters in that run);
--kernel-stats CSV N --case K appends the regrid_* kernels' rows of that run's kernel_stats.csv to the same .jsonl: calls, and the
kernel's total over the head's three layers per fit (the run's total / 5).
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

LAYERS = [192, 64, 16, 1]
CASES = ((5, 12), (32, 58))
REPEATS = 7
KERNEL_RUNS = 5


def build(num_knots, n, dev):
    from models.kan import KANSeverityModule
    from oracle import ref_cpu
    g = torch.Generator().manual_seed(n + num_knots)
    m = KANSeverityModule(LAYERS, num_knots, 3)
    m.load_state_dict(ref_cpu.init_kan_state(LAYERS, num_knots, 3, g))
    return m.to(dev).eval(), (torch.randn(n, LAYERS[0], generator=g) * 1.5).to(dev)


def fused(m, x, rows, new_knots):
    from rovit_hip.kan_grid import KANRegrid
    acc = KANRegrid(m, capacity=x.shape[0])
    for i in range(0, x.shape[0], rows):
        acc.update(x[i:i + rows])
    return acc.fit(num_knots=new_knots)


def recipe(m, x, new_knots, chunk=1024, prior_weight=1e-2):
    from models.kan import BSplineBasis
    from rovit_hip import kan_grid as kg
    from rovit_hip.functions import ACT_RELU, KANLayerFn
    kn_new_host = kg.make_grid(new_knots)
    kn_new = kn_new_host.to(x.device)
    out, a = [], x
    with torch.no_grad():
        for layer in m.kan_layers:
            kn, W = layer.knots, layer.spline_weights
            nbn, nb = kn_new.numel() - 4, kn.numel() - 4
            G = torch.zeros(layer.in_features, nbn, nbn, dtype=torch.float64, device=x.device)
            M = torch.zeros(layer.in_features, nbn, nb, dtype=torch.float64, device=x.device)
            for r0 in range(0, a.shape[0], chunk):
                xn = torch.tanh(a[r0:r0 + chunk])
                bn, bo = BSplineBasis.compute_basis(xn, kn_new).double(), BSplineBasis.compute_basis(xn, kn).double()
                G += torch.einsum('nia,nib->iab', bn, bn)
                M += torch.einsum('nia,nib->iab', bn, bo)
            pri = kg.prior_moments(kn_new_host.numpy(), kg.host_knots(layer))
            s = prior_weight / pri['L']
            A = G / a.shape[0] + torch.from_numpy(pri['G'] * s).to(x.device)
            T = torch.linalg.solve(A, M / a.shape[0] + torch.from_numpy(pri['M'] * s).to(x.device))
            w_new = torch.einsum('iab,ijb->ija', T, W.double()).float().contiguous()
            out.append(w_new)
            a = KANLayerFn.apply(a, w_new, kn_new, layer.linear.weight, layer.linear.bias, ACT_RELU)
    return float(torch.stack([w.abs().max() for w in out]).max().cpu())


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def time_arms(arms):
    for fn in arms.values():
        fn()
    times = {k: [] for k in arms}
    for _ in range(REPEATS):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    return times


def records(case, times, peaks):
    med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}
    out = []
    for name, v in times.items():
        t = sorted(x * 1e3 for x in v)
        rec = dict(case, arm=name, median_ms=round(med[name], 3), min_ms=round(t[0], 3), max_ms=round(t[-1], 3), repeats=len(t),
                   peak_extra_mib=round(peaks[name] / 2 ** 20, 1), device=torch.cuda.get_device_name(0))
        if name == 'fused':
            rec['recipe_over_fused'] = round(med['recipe'] / med['fused'], 2)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def case_of(k):
    return CASES[k]


def kernels_only(n, rows, k):
    dev = torch.device('cuda:0')
    old, new = case_of(k)
    m, x = build(old, n, dev)
    for _ in range(KERNEL_RUNS):
        fused(m, x, rows, new)
    torch.cuda.synchronize()
    print('kernels-only run done: n =', n, 'knots', old, '->', new)


def kernel_stats(path, n, k, out):
    old, new = case_of(k)
    with open(path) as f, open(out, 'a') as o:
        for row in csv.DictReader(f):
            if 'regrid_' in row['Name'] or 'kan_layer_fwd' in row['Name']:
                name = row['Name'].split('::')[-1].split('(')[0]
                rec = {'case': 'kernel', 'layers': LAYERS, 'knots_old': old, 'knots_new': new, 'rows': n, 'kernel': name, 'calls': int(row['Calls']),
                       'per_fit_us': round(float(row['TotalDurationNs']) / 1e3 / KERNEL_RUNS, 2),
                       'min_us': round(float(row['MinNs']) / 1e3, 2), 'max_us': round(float(row['MaxNs']) / 1e3, 2)}
                print(json.dumps(rec))
                o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[4096, 65536])
    ap.add_argument('--update-rows', type=int, default=256)
    ap.add_argument('--kernels-only', type=int, default=0, metavar='N')
    ap.add_argument('--kernel-stats', nargs=2, metavar=('CSV', 'N'))
    ap.add_argument('--case', type=int, default=0, choices=range(len(CASES)), help='case of the two kernel modes: 0 = 5 -> 12 knots, 1 = 32 -> 58')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kan_grid_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats[0], int(a.kernel_stats[1]), a.case, a.out)
    if a.kernels_only:
        return kernels_only(a.kernels_only, a.update_rows, a.case)
    dev = torch.device('cuda:0')
    lines = []
    for old, new in CASES:
        for n in a.rows:
            m, x = build(old, n, dev)
            arms = {'fused': lambda: fused(m, x, a.update_rows, new), 'recipe': lambda: recipe(m, x, new)}
            times = time_arms(arms)
            peaks = {k: peak_extra(fn) for k, fn in arms.items()}
            lines += records({'case': 'kan_grid', 'layers': LAYERS, 'knots_old': old, 'knots_new': new, 'rows': n, 'update_rows': a.update_rows},
                             times, peaks)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
