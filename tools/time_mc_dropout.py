"""Time MC-dropout uncertainty three ways at several (batch, samples) points and append one JSON line per (batch, T, mode) to
profiles/mc_dropout_time.jsonl.

  fused  : RoViTKAN.predict_mc (one backbone forward, the rovit_head_mc_fwd launch, the eval head phase for kan_severity)
  recipe : the reference's recipe -- model.eval(), the nn.Dropout modules back to train(), T forwards under no_grad -- and the
           statistics predict_mc reports computed in torch from the T outputs
  floor  : predict() (one deterministic forward)

Device-event times; --warmup calls of every mode first, then --repeats rounds in which the modes run interleaved (fused, recipe, floor,
...), one call each per round; the median and min per mode are reported.  peak_extra_mb: torch's peak allocation above the allocation
before one call, measured after the warm-up with the engine's workspace pools emptied, so the call allocates its own workspace.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)


def recipe(m, x, T):
    m.eval()
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.train()
    with torch.no_grad():
        outs = [m(x) for _ in range(T)]
        lp = torch.log_softmax(torch.stack([o['cls_logits'] for o in outs]), dim=2)
        p = lp.exp()
        ent = -(p * lp).nan_to_num().sum(2)
        pbar = p.mean(0)
        hp = -(pbar * pbar.log()).nan_to_num().sum(1)
        cp = torch.sigmoid(torch.stack([o['ordinal_logits'] for o in outs]))
        po = torch.cat([cp[..., :1], cp[..., 1:] - cp[..., :-1], 1.0 - cp[..., -1:]], dim=2)
        sev = (po * torch.arange(po.shape[2], device=x.device, dtype=po.dtype)).sum(2)
        mu = torch.stack([o['mu'] for o in outs])
        lv = torch.stack([o['log_var'] for o in outs])
        res = {'class_probs': pbar, 'class_probs_std': p.std(0, unbiased=False), 'mutual_information': (hp - ent.mean(0)).clamp_min(0),
               'ordinal_probs': po.mean(0), 'ordinal_severity_std': sev.std(0, unbiased=False), 'uncertainty_mu': mu.mean(0),
               'epistemic_var': mu.var(0, unbiased=False), 'aleatoric_var': lv.exp().mean(0), 'kan_severity': outs[0]['kan_severity']}
    m.eval()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, nargs='+', default=[1, 64, 256])
    ap.add_argument('--samples', type=int, nargs='+', default=[8, 32, 128])
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mc_dropout_time.jsonl'))
    a = ap.parse_args()
    from oracle import ref_cpu
    from models.rovit_kan import RoViTKAN
    dev = torch.device('cuda:0')
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    m = m.to(dev).eval()
    eng = m.backbone.model.engine
    lines = []
    for B in a.batch:
        x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B)).to(dev)
        for T in a.samples:
            modes = {'fused': lambda: m.predict_mc(x, num_samples=T), 'recipe': lambda: recipe(m, x, T), 'floor': lambda: m.predict(x)}
            for _ in range(a.warmup):
                for fn in modes.values():
                    fn()
            peak = {}
            for name in ('fused', 'recipe'):
                torch.cuda.synchronize()
                eng._ws_pool.clear()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                modes[name]()
                torch.cuda.synchronize()
                peak[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            times = {k: [] for k in modes}
            for _ in range(a.repeats):
                for name, fn in modes.items():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    fn()
                    e.record()
                    e.synchronize()
                    times[name].append(s.elapsed_time(e))
            for name in modes:
                t = sorted(times[name])
                rec = {'mode': name, 'batch': B, 'samples': T, 'median_ms': round(t[len(t) // 2], 3), 'min_ms': round(t[0], 3),
                       'repeats': a.repeats, 'device': torch.cuda.get_device_name(0)}
                if name in peak:
                    rec['peak_extra_mb'] = peak[name]
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
