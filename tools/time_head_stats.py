"""Time the per-head attention statistics against what a user writes without them; appends JSON lines to --out.

Arms, at each batch of --batches (depth-12 backbone, seeded random weights and images):
  fused   : DeiTTinyBackbone.attention_head_stats (one fused forward, csrc/head_stats.hip)
  recipe  : get_attention_probabilities (12 fp32 (B,3,197,197) tensors) followed by the reductions of rovit_hip/head_stats.py's
            definitions in torch on the device -- summary and cls_attention, no per-token output
  forward : the plain inference forward (floor)
  rollout : attention_rollout(upsample=False) (floor: the other per-block attention reduction)

One warm call of every arm, then --repeats rounds in which the arms alternate; each call is timed with device events and the median
over the rounds is reported, with min, max and torch's peak allocation above the resting level during that arm's calls.
``recipe_over_fused`` and ``fused_minus_forward_ms`` on the fused line are derived from the medians.

  --kernels : instead, run the fused arm --repeats times and nothing else (for a kernel trace of that arm alone).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)


def recipe(model, x, tables):
    """The statistics of rovit_hip.head_stats from stored probabilities, in torch on the device: (summary (B,L,3,8), cls (B,L,3,196))."""
    dist, near = tables
    summ, cls = [], []
    for P in model.get_attention_probabilities(x):
        ent = -(P * torch.log(P.clamp_min(1e-45))).sum(-1)
        pp = P[:, :, 1:, 1:]
        mass = pp.sum(-1)
        d = torch.where(mass > 0, (pp * dist).sum(-1) / mass.clamp_min(1e-45), torch.zeros_like(mass))
        summ.append(torch.stack([ent.mean(-1), d.mean(-1), P[:, :, 1:, 0].mean(-1), torch.diagonal(P, dim1=-2, dim2=-1).mean(-1), ent[..., 0],
                                 P[:, :, 0, 0], P.max(-1)[0].mean(-1), (pp * near).sum(-1).mean(-1)], dim=-1))
        cls.append(P[:, :, 0, 1:])
    return torch.stack(summ, 1), torch.stack(cls, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[16, 256])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'head_stats_time.jsonl'))
    ap.add_argument('--kernels', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_head_stats: needs a GPU (a time taken elsewhere says nothing)')
    from oracle import ref_cpu
    from models.backbone import DeiTTinyBackbone
    from rovit_hip import head_stats as hs
    dev = torch.device('cuda:0')
    m = DeiTTinyBackbone(pretrained=False)
    m.model.load_state_dict(ref_cpu.init_vit_state(12, torch.Generator().manual_seed(0)))
    m = m.to(dev).eval()
    tables = (torch.from_numpy(hs.patch_distances()).float().to(dev), torch.from_numpy(hs.patch_neighbours()).float().to(dev))
    lines = []
    for B in a.batches:
        x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(dev)
        arms = {'fused': lambda: m.attention_head_stats(x), 'recipe': lambda: recipe(m, x, tables), 'forward': lambda: m(x),
                'rollout': lambda: m.attention_rollout(x, upsample=False)}
        if a.kernels:
            arms = {'fused': arms['fused']}
        times = {k: [] for k in arms}
        peak = {k: 0 for k in arms}
        with torch.no_grad():
            for fn in arms.values():                 # the warm run
                fn()
            torch.cuda.synchronize()
            # agreement of the two arms at the size that is timed (the recipe's log and sums are torch's fp32)
            if not a.kernels:
                f, (rs, rc) = arms['fused'](), arms['recipe']()
                agree = {'summary_max_abs_diff': float((f['summary'] - rs).abs().max()), 'cls_equal': bool(torch.equal(f['cls_attention'], rc))}
                del f, rs, rc
            for _ in range(a.repeats):
                for k, fn in arms.items():           # the arms alternate
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    out = fn()
                    e.record()
                    e.synchronize()
                    times[k].append(s.elapsed_time(e))
                    peak[k] = max(peak[k], torch.cuda.max_memory_allocated() - base)
                    del out
        if a.kernels:
            continue
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        for k, v in times.items():
            line = {'case': 'head_stats', 'depth': 12, 'batch': B, 'arm': k, 'median_ms': round(med[k], 3), 'min_ms': round(min(v), 3),
                    'max_ms': round(max(v), 3), 'peak_extra_mb': round(peak[k] / 2 ** 20, 1), 'repeats': a.repeats,
                    'device': torch.cuda.get_device_name(0)}
            if k == 'fused':
                line.update(recipe_over_fused=round(med['recipe'] / med['fused'], 2), fused_minus_forward_ms=round(med['fused'] - med['forward'], 3),
                            fused_minus_rollout_ms=round(med['fused'] - med['rollout'], 3), **agree)
            lines.append(line)
            print(json.dumps(line), flush=True)
    if lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            for line in lines:
                fh.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
