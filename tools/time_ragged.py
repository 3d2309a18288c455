"""Time the token-dropping explanations with and without ragged batches and append one JSON line per (case, arm) to
profiles/ragged_time.jsonl.

  ragged  : perturbation='drop', ragged=True -- the sequences of all lengths packed longest first into calls of 256 x 197 rows
            (rovit_vit_forward_ragged)
  lengths : perturbation='drop', ragged=False -- one rovit_vit_forward_tokens call and more per sequence length
  replace : perturbation='replace' -- every sequence 197 tokens, about twice the token rows of 'drop'

Cases: patch_shap at P = 196 / M = 2048 and P = 49 / M = 1024, one and eight images; perturbation_curves at 28 steps, batch 16 and
256.  One warm run of every arm, then the arms alternate seven times each in one process; host clock between two device
synchronisations; median, min, max.

--kernels-only K ARM: arm ARM of case K alone, five times, for a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_ragged.py --kernels-only K ARM`` run (no counters in that run);
--kernel-stats CSV K ARM appends the attention and gather kernels' rows of that run's kernel_stats.csv to the same .jsonl.
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

REPEATS = 7
KERNEL_RUNS = 5
ARMS = ('ragged', 'lengths', 'replace')
CASES = [('patch_shap', B, g, M) for g, M in ((14, 2048), (7, 1024)) for B in (1, 8)] + [('perturbation_curves', B, 28, 0) for B in (16, 256)]
KERNELS = ('attn_fwd_ragged_kernel', 'attn_cls_fwd_ragged_kernel', 'attn_fwd_kernel', 'attn_cls_fwd_kernel', 'gather_token_rows_kernel',
           'gather_token_rows_ragged_kernel')


def build(dev):
    from models.rovit_kan import RoViTKAN
    from oracle import ref_cpu
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    return m.to(dev).eval()


def arm_fn(m, case, arm, dev):
    what, B, a, M = case
    x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B + a)).to(dev)
    pert = 'replace' if arm == 'replace' else 'drop'
    kw = {'perturbation': pert, 'ragged': arm == 'ragged'}
    if what == 'patch_shap':
        return lambda: m.patch_shap(x, players=a, num_samples=M, **kw)['player_values']
    sal = torch.rand(B, 14, 14, generator=torch.Generator().manual_seed(B)).to(dev)
    return lambda: m.perturbation_curves(x, sal, steps=a, **kw)['deletion_auc']


def describe(case):
    what, B, a, M = case
    return {'case': what, 'batch': B, 'players': a * a, 'num_samples': M} if what == 'patch_shap' else {'case': what, 'batch': B, 'steps': a}


def kernels_only(k, arm):
    dev = torch.device('cuda:0')
    fn = arm_fn(build(dev), CASES[k], arm, dev)
    for _ in range(KERNEL_RUNS):
        fn()
    torch.cuda.synchronize()
    print('kernels-only run done:', CASES[k], arm)


def kernel_stats(path, k, arm, out):
    with open(path) as f, open(out, 'a') as o:
        for row in csv.DictReader(f):
            name = row['Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0].split('<')[0]
            if name in KERNELS:
                rec = dict(describe(CASES[k]), arm=arm, kernel=name, calls=int(row['Calls']), runs=KERNEL_RUNS,
                           avg_us=round(float(row['AverageNs']) / 1e3, 2), min_us=round(float(row['MinNs']) / 1e3, 2),
                           max_us=round(float(row['MaxNs']) / 1e3, 2), total_us=round(float(row['TotalDurationNs']) / 1e3, 1))
                rec['case'] = 'kernel:' + rec['case']
                print(json.dumps(rec))
                o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels-only', nargs=2, metavar=('K', 'ARM'))
    ap.add_argument('--kernel-stats', nargs=3, metavar=('CSV', 'K', 'ARM'))
    ap.add_argument('--cases', type=int, nargs='*', default=None, help='indices into CASES (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ragged_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats[0], int(a.kernel_stats[1]), a.kernel_stats[2], a.out)
    if a.kernels_only:
        return kernels_only(int(a.kernels_only[0]), a.kernels_only[1])
    dev = torch.device('cuda:0')
    m = build(dev)
    for k in (a.cases if a.cases else range(len(CASES))):
        case = CASES[k]
        arms = {name: arm_fn(m, case, name, dev) for name in ARMS}
        got = {name: fn() for name, fn in arms.items()}                   # the warm run
        times = {name: [] for name in arms}
        for _ in range(REPEATS):
            for name, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        med = {name: sorted(v)[len(v) // 2] * 1e3 for name, v in times.items()}
        with open(a.out, 'a') as f:
            for name, v in times.items():
                t = sorted(s * 1e3 for s in v)
                rec = dict(describe(case), arm=name, median_ms=round(med[name], 3), min_ms=round(t[0], 3), max_ms=round(t[-1], 3),
                           repeats=len(t), device=torch.cuda.get_device_name(0))
                if name == 'ragged':
                    rec['lengths_over_ragged'] = round(med['lengths'] / med['ragged'], 2)
                    rec['replace_over_ragged'] = round(med['replace'] / med['ragged'], 2)
                    # the two 'drop' arms may take different MLP paths for short sequences: bf16 rounding apart, not bit for bit
                    rec['max_abs_diff_to_lengths'] = float((got['ragged'] - got['lengths']).abs().max())
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
