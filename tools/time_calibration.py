"""Time post-hoc calibration and append one JSON line per (case, arm) to profiles/calibration_time.jsonl.

  calibrate       : EvalAccumulator.calibrate() on device-resident rows: the memset, the regression kernel, four search and step rounds,
                    the NLL pair, ONE device-to-host copy and the Calibration on the host
  calibrate_apply : calibrate() + Calibration.apply() + compute() on the applied accumulator (a second copy: the calibrated score card)
  compute         : the bare compute() on the same rows, from scratch (the finalise and its copy): the floor of a call that reduces and copies
  lbfgs           : the recipe a user would write on the same device: torch.optim.LBFGS (max_iter=50) over ln T on the device's
                    log-probabilities with the NLL as closure, one .item() for T, plus the closed-form s and its .item()
  numpy           : arrays(), the extra column and calibration_reference on the host

Cases: --rows device-resident rows, C = 4, 9 coverage levels.  Every arm is warmed once; the arms alternate in one process; --repeats
timed runs each; host clock between two device synchronisations.  median, min and max per arm; the ratios from the medians.  Nothing here
promises a speed-up: the ratios are what was measured, and the record says how far the recipe's ln T lies from the kernel's.

--kernels-only: five calibrate() + apply() calls per case for a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_calibration.py --kernels-only`` run; --kernel-stats CSV appends the cal_* and
recalibrate rows of that run's kernel_stats.csv to the same .jsonl (pass the same --rows to both, one size per profiled run).
"""
import argparse
import csv
import json
import math
import os
import re
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)

LEVELS = 9


def make_accumulator(n, dev):
    from rovit_hip.evaluation import EvalAccumulator
    g = torch.Generator().manual_seed(n)
    labels = torch.randint(0, 4, (n,), generator=g)
    logits = torch.randn(n, 4, generator=g) * 6.0               # an over-confident classifier: T* is about 3
    logits[torch.arange(n), labels] += 4.5
    sev = (labels.float() + torch.randn(n, generator=g) * 0.8).clamp(0, 3).reshape(-1, 1)
    mu = labels.float() + torch.randn(n, generator=g) * 0.6
    log_var = torch.log((mu - labels.float()).abs() + 0.1) + torch.randn(n, generator=g) * 0.5
    acc = EvalAccumulator(4, capacity=n)
    acc.update({'cls_logits': logits.to(dev), 'kan_severity': sev.to(dev), 'mu': mu.reshape(-1, 1).to(dev), 'log_var': log_var.reshape(-1, 1).to(dev)},
               labels.to(dev), labels.to(dev), extra={'mu': mu.to(dev)})
    return acc


def forget(acc):
    """Drop the cached finalise, so that the next compute() pays for all of its work."""
    acc._block = acc._block_dev = acc._rank_counts = None


def lbfgs_recipe(acc):
    """Temperature scaling as it is usually written (Guo et al.'s reference code): LBFGS on the NLL, here over ln T and on the recorded
    log-probabilities, which gives the same softmax as the logits would; the sigma scale in closed form."""
    n = acc.n
    rec = acc._rec
    logp = torch.log(rec['probs'][:n].double()).clamp_min(-100.0 * math.log(2.0))
    label = rec['label'][:n].long()
    log_t = torch.zeros(1, dtype=torch.float64, device=logp.device, requires_grad=True)
    opt = torch.optim.LBFGS([log_t], lr=1.0, max_iter=50, line_search_fn='strong_wolfe')

    def closure():
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(logp * torch.exp(-log_t), label)
        loss.backward()
        return loss
    opt.step(closure)
    z = (rec['sev_true'][:n].double() - acc._extra['mu'][:n].double()) / rec['uncertainty'][:n].double()
    return float(log_t.item()), float(torch.sqrt((z * z).mean()).item())


def numpy_recipe(acc):
    from rovit_hip.evaluation import calibration_reference
    return calibration_reference(acc.arrays(), {'mu': acc._extra_column('mu')}, acc.num_classes, LEVELS)


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
            m = re.search(r'cal_[a-z_]+(ILi\dE)?|recalibrate_kernel', row['Name'])
            if m:
                rec = {'case': 'kernel', 'rows': rows, 'kernel': m.group(0), 'calls': int(row['Calls']),
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'calibration_time.jsonl'))
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
                acc.calibrate(levels=LEVELS).apply(acc)
            torch.cuda.synchronize()
            print(f'kernels-only run done: rows = {n}')
            continue
        # the arms agree before they are timed
        cal, (recipe_log_t, recipe_s), ref = acc.calibrate(levels=LEVELS), lbfgs_recipe(acc), numpy_recipe(acc)
        assert abs(math.log(cal.temperature) + ref['u']) <= 1e-6, 'the kernel and the numpy statement find another temperature'
        assert abs(recipe_s - cal.sigma_scale) <= 1e-9 * cal.sigma_scale, 'the recipe computes another sigma scale'
        arms = {'calibrate': lambda: acc.calibrate(levels=LEVELS),
                'calibrate_apply': lambda: acc.calibrate(levels=LEVELS).apply(acc).compute(),
                'compute': lambda: (forget(acc), acc.compute()), 'lbfgs': lambda: lbfgs_recipe(acc), 'numpy': lambda: numpy_recipe(acc)}
        times = time_arms(arms, a.repeats)
        med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}
        for name, v in times.items():
            t = sorted(x * 1e3 for x in v)
            rec = {'case': 'calibration', 'rows': n, 'classes': 4, 'levels': LEVELS, 'arm': name, 'median_ms': round(med[name], 3),
                   'min_ms': round(t[0], 3), 'max_ms': round(t[-1], 3), 'repeats': len(t), 'device': torch.cuda.get_device_name(0)}
            if name == 'calibrate':
                rec.update(temperature=cal.temperature, status=cal.status, calibrate_over_compute=round(med['calibrate'] / med['compute'], 2),
                           lbfgs_over_calibrate=round(med['lbfgs'] / med['calibrate'], 2), numpy_over_calibrate=round(med['numpy'] / med['calibrate'], 2))
            if name == 'lbfgs':
                rec.update(ln_t_distance_to_calibrate=abs(recipe_log_t - math.log(cal.temperature)))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
