"""Time attention rollout one way at one batch size; prints one JSON line.

  --mode fused : rovit_hip.rollout.attention_rollout (the fused per-block rollout + the map launch)
  --mode taps  : get_attention_probabilities (12 fp32 (B,3,197,197) tensors) + the torch restatement of the reference's
                 rollout (attention_maps.py:60-103; F.interpolate stands in for cv2.resize)

One mode and one batch per process: run each under its own `timeout`.  Times are CUDA-event medians over --iters calls
after --warmup; peak_mb is torch's peak allocation during the timed calls.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)


def restated(model, x):
    probs = model.get_attention_probabilities(x)
    B, N = x.shape[0], 197
    eye = torch.eye(N, device=x.device)
    roll = eye.expand(B, N, N)
    for a in probs:
        a = a.mean(1) + eye
        roll = roll @ (a / a.sum(-1, keepdim=True))
    m = F.interpolate(roll[:, 0, 1:].reshape(B, 1, 14, 14), size=(224, 224), mode='bilinear', align_corners=False)[:, 0]
    mn, mx = m.flatten(1).min(1)[0][:, None, None], m.flatten(1).max(1)[0][:, None, None]
    return (m - mn) / (mx - mn + 1e-8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['fused', 'taps'], required=True)
    ap.add_argument('--batch', type=int, required=True)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    from oracle import ref_cpu
    from models.backbone import DeiTTinyBackbone
    dev = torch.device('cuda:0')
    m = DeiTTinyBackbone(pretrained=False)
    m.model.load_state_dict(ref_cpu.init_vit_state(12, torch.Generator().manual_seed(0)))
    m = m.to(dev).eval()
    x = torch.randn(a.batch, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(dev)
    fn = (lambda: m.attention_rollout(x)) if a.mode == 'fused' else (lambda: restated(m, x))
    with torch.no_grad():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        times = []
        for _ in range(a.iters):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            times.append(s.elapsed_time(e))
    times.sort()
    print(json.dumps({'mode': a.mode, 'batch': a.batch, 'median_ms': round(times[len(times) // 2], 3),
                      'min_ms': round(times[0], 3), 'ms_per_image': round(times[len(times) // 2] / a.batch, 4),
                      'peak_extra_mb': round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1), 'iters': a.iters}))


if __name__ == '__main__':
    main()
