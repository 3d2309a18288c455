"""Time patch_shap two ways and append one JSON line per (case, arm) to profiles/shap_time.jsonl.

  fused  : model.patch_shap -- the host plan, rovit_shap_coalitions, one embedding per image, the gathered forwards
           (rovit_vit_forward_tokens) in chunks of 256 sequences, rovit_shap_gram and rovit_shap_solve; nothing is read back
  recipe : what a user would write in torch on the same device, GIVEN the same coalitions and weights for free (it pays for no sampler):
           the masked images built in pixels -- patches of absent players taken from the baseline -- through the model's inference forward
           in chunks of 256 images, softmax, then torch.linalg.lstsq in fp64 on the sqrt(w)-scaled design with the efficiency
           constraint eliminated (phi_P = delta - the sum of the others).  Pixels cannot drop tokens, so for perturbation='drop' the
           recipe arm still replaces by the zero baseline: the same cost structure, another value function (the record says so).

Cases: batch 1 and 8; P = 196 at M = 2048 and P = 49 at M = 1024; 'replace' and 'drop'.  One warm run of both arms, then the arms
alternate (fused, recipe, fused, ...) seven times each in one process; host clock between two device synchronisations; median, min, max.

--kernels-only K: the fused arm of case K alone, five times, for a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_shap.py --kernels-only K`` run (no counters in that run);
--kernel-stats CSV K appends the shap_* and token-gather kernels' rows of that run's kernel_stats.csv to the same .jsonl (calls over the
five runs plus the one coalition launch of the set-up; average, min, max and total).
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
CASES = [(B, g, M, pert) for g, M in ((14, 2048), (7, 1024)) for pert in ('replace', 'drop') for B in (1, 8)]


def build(dev):
    from models.rovit_kan import RoViTKAN
    from oracle import ref_cpu
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    return m.to(dev).eval()


def fused(m, x, g, M, pert):
    return m.patch_shap(x, players=g, num_samples=M, perturbation=pert)['player_values']


def recipe(m, x, Z, w, pmap, cls, chunk=256):
    B, (M, P) = x.shape[0], Z.shape
    with torch.no_grad():
        present = torch.cat([Z, torch.ones(1, P, dtype=torch.bool, device=x.device), torch.zeros(1, P, dtype=torch.bool, device=x.device)])[:, pmap]
        vals = torch.empty((M + 2) * B, device=x.device)
        for j0 in range(0, (M + 2) * B, chunk):
            j = torch.arange(j0, min((M + 2) * B, j0 + chunk), device=x.device)
            ci, b = j // B, j % B
            pix = present[ci].view(-1, 1, 14, 1, 14, 1).expand(-1, 3, 14, 16, 14, 16).reshape(-1, 3, 224, 224)
            imgs = torch.where(pix, x[b], torch.zeros((), device=x.device))
            p = torch.softmax(m(imgs)['cls_logits'].float(), dim=1)
            vals[j] = p.gather(1, cls[b].view(-1, 1))[:, 0]
        vals = vals.view(M + 2, B).double()
        v1, v0 = vals[M], vals[M + 1]
        Zd = Z.double()
        sw = w.sqrt().unsqueeze(1)
        A = (Zd[:, :-1] - Zd[:, -1:]) * sw
        rhs = (vals[:M] - v0 - Zd[:, -1:] * (v1 - v0)) * sw
        head = torch.linalg.lstsq(A, rhs).solution                      # (P - 1, B)
        return torch.cat([head, (v1 - v0 - head.sum(0)).unsqueeze(0)]).t().float()


def setup(m, B, g, M, dev):
    from rovit_hip import shap
    x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B + g)).to(dev)
    ks = shap.KernelShap(g, M, 0)
    co = ks.coalitions(dev)
    Z = shap.unpack_bits(co['bits'], ks.P)
    pmap = torch.from_numpy(ks.players).to(dev).long()
    with torch.no_grad():
        cls = m(x)['cls_logits'].argmax(dim=1)
    return x, Z, co['weights'], pmap, cls


def kernels_only(k):
    dev = torch.device('cuda:0')
    m = build(dev)
    B, g, M, pert = CASES[k]
    x = setup(m, B, g, M, dev)[0]
    for _ in range(KERNEL_RUNS):
        fused(m, x, g, M, pert)
    torch.cuda.synchronize()
    print('kernels-only run done:', CASES[k])


def kernel_stats(path, k, out):
    B, g, M, pert = CASES[k]
    with open(path) as f, open(out, 'a') as o:
        for row in csv.DictReader(f):
            name = row['Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0].split('<')[0]
            if name.startswith('shap_') or name == 'gather_token_rows_kernel':
                rec = {'case': 'kernel', 'batch': B, 'players': g * g, 'num_samples': M, 'perturbation': pert, 'kernel': name,
                       'calls': int(row['Calls']), 'runs': KERNEL_RUNS, 'avg_us': round(float(row['AverageNs']) / 1e3, 2),
                       'min_us': round(float(row['MinNs']) / 1e3, 2), 'max_us': round(float(row['MaxNs']) / 1e3, 2),
                       'total_us': round(float(row['TotalDurationNs']) / 1e3, 1)}
                print(json.dumps(rec))
                o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels-only', type=int, default=None, metavar='K', choices=range(len(CASES)))
    ap.add_argument('--kernel-stats', nargs=2, metavar=('CSV', 'K'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'shap_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats[0], int(a.kernel_stats[1]), a.out)
    if a.kernels_only is not None:
        return kernels_only(a.kernels_only)
    dev = torch.device('cuda:0')
    m = build(dev)
    lines = []
    for B, g, M, pert in CASES:
        x, Z, w, pmap, cls = setup(m, B, g, M, dev)
        arms = {'fused': lambda: fused(m, x, g, M, pert), 'recipe': lambda: recipe(m, x, Z, w, pmap, cls)}
        got = {k: fn() for k, fn in arms.items()}                        # the warm run
        times = {k: [] for k in arms}
        for _ in range(REPEATS):
            for name, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}
        for name, v in times.items():
            t = sorted(s * 1e3 for s in v)
            rec = {'case': 'patch_shap', 'batch': B, 'players': g * g, 'num_samples': M, 'perturbation': pert, 'arm': name,
                   'median_ms': round(med[name], 3), 'min_ms': round(t[0], 3), 'max_ms': round(t[-1], 3), 'repeats': len(t),
                   'device': torch.cuda.get_device_name(0)}
            if name == 'fused':
                rec['recipe_over_fused'] = round(med['recipe'] / med['fused'], 2)
                if pert == 'replace':                                    # the two arms estimate the same thing there
                    rec['max_abs_diff_to_recipe'] = float((got['fused'] - got['recipe']).abs().max())
            elif pert == 'drop':
                rec['recipe_perturbation'] = 'replace by zeros (pixels cannot drop tokens)'
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
