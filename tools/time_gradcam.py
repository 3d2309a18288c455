"""Time Grad-CAM++ three ways at one or more batch sizes and append one JSON line per (batch, mode) to profiles/gradcam_time.jsonl.

  fused : rovit_hip.gradcam.grad_cam_pp (last-block forward mode + class-token backward + CAM + map launches), maps included
  hooks : the reference's recipe on the fused path -- forward with a forward and a full-backward hook on blocks[-1].norm1, backward of
          the sum of the target logits (12 blocks, every weight gradient), then the Grad-CAM++ arithmetic of gradcam.py:62-101 in torch,
          F.interpolate for cv2.resize and the conditional min-max
  floor : the plain inference forward m(x) under no_grad

Device-event times; --warmup calls of every mode first, then --repeats rounds in which the modes run interleaved (fused, hooks, floor,
...), one call each per round; the median and min per mode are reported.  peak_extra_mb: torch's peak allocation above the
allocation before one call, measured after the warm-up (so state that persists across calls -- the prepared weights, the hook path's
flat gradient buffers -- is already allocated) with the engine's workspace pools emptied, so the call allocates its own workspace.
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


def hook_path(m, x):
    cap = {}
    target = m.backbone.model.blocks[-1].norm1
    h1 = target.register_forward_hook(lambda mod, inp, outp: cap.__setitem__('act', outp.detach()))
    h2 = target.register_full_backward_hook(lambda mod, gin, gout: cap.__setitem__('grad', gout[0].detach()))
    out = m(x)
    logits = out['cls_logits']
    cls = logits.argmax(1)
    m.zero_grad(set_to_none=True)
    logits.gather(1, cls[:, None]).sum().backward()
    h1.remove()
    h2.remove()
    with torch.no_grad():
        a, g = cap['act'], cap['grad']
        den = 2 * g.pow(2) + (a * g.pow(3)).sum(dim=1, keepdim=True)
        den = torch.where(den != 0.0, den, torch.ones_like(den))
        w = (g.pow(2) / den * torch.relu(g)).sum(dim=2, keepdim=True)
        B = a.shape[0]
        cam = torch.relu((w * a).sum(dim=2)[:, 1:].reshape(B, 1, 14, 14))
        mp = F.interpolate(cam, size=(224, 224), mode='bilinear', align_corners=False)[:, 0]
        mx, mn = mp.flatten(1).max(1)[0][:, None, None], mp.flatten(1).min(1)[0][:, None, None]
        mp = torch.where(mx > 0, (mp - mn) / (mx - mn), mp)
    m.zero_grad(set_to_none=True)
    return mp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, nargs='+', default=[1, 64, 256])
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gradcam_time.jsonl'))
    a = ap.parse_args()
    from oracle import ref_cpu
    from models.rovit_kan import RoViTKAN
    dev = torch.device('cuda:0')
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    m = m.to(dev).eval()
    eng = m.backbone.model.engine

    def floor(x):
        with torch.no_grad():
            return m(x)['cls_logits']
    modes = {'fused': lambda x: m.grad_cam_pp(x), 'hooks': lambda x: hook_path(m, x), 'floor': floor}
    lines = []
    for B in a.batch:
        x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B)).to(dev)
        for _ in range(a.warmup):
            for fn in modes.values():
                fn(x)
        peak = {}
        for name in ('fused', 'hooks'):
            torch.cuda.synchronize()
            eng._ws_pool.clear()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            modes[name](x)
            torch.cuda.synchronize()
            peak[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        torch.cuda.synchronize()
        times = {k: [] for k in modes}
        for _ in range(a.repeats):
            for name, fn in modes.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn(x)
                e.record()
                e.synchronize()
                times[name].append(s.elapsed_time(e))
        for name in modes:
            t = sorted(times[name])
            rec = {'mode': name, 'batch': B, 'median_ms': round(t[len(t) // 2], 3), 'min_ms': round(t[0], 3),
                   'ms_per_image': round(t[len(t) // 2] / B, 4), 'repeats': a.repeats, 'device': torch.cuda.get_device_name(0)}
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
