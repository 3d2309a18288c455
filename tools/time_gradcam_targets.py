"""Time Grad-CAM++ of the severity and uncertainty outputs (``target=``) at one or more batch sizes and append one JSON line per (batch,
mode) to profiles/gradcam_targets_time.jsonl.

  <target>     : grad_cam_pp(m, x, target=<target>) for each of the five targets, maps included
  all_one_call : grad_cam_pp(m, x, target=[all five]) -- one backbone forward, five tails
  all_separate : the five single-target calls one after the other
  hooks_kan    : the reference's recipe for kan_severity on the fused path -- forward with a forward and a full-backward hook on
                 blocks[-1].norm1, backward of the summed KAN severity (12 blocks, every weight gradient), then the Grad-CAM++ arithmetic
                 of gradcam.py:62-101 in torch, F.interpolate for cv2.resize and the conditional min-max

Device-event times; --warmup calls of every mode first, then --repeats rounds in which the modes run interleaved, one call each per
round; the median and min per mode are reported (the protocol of tools/time_gradcam.py).  The seed kernel alone:
rocprofv3 --kernel-trace --stats -- python tools/time_gradcam_targets.py --batch 256 --repeats 3 --out <scratch file>
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

TARGETS = ['class', 'ordinal_severity', 'mu', 'log_var', 'kan_severity']


def hook_path_kan(m, x):
    cap = {}
    target = m.backbone.model.blocks[-1].norm1
    h1 = target.register_forward_hook(lambda mod, inp, outp: cap.__setitem__('act', outp.detach()))
    h2 = target.register_full_backward_hook(lambda mod, gin, gout: cap.__setitem__('grad', gout[0].detach()))
    out = m(x)
    m.zero_grad(set_to_none=True)
    out['kan_severity'].sum().backward()
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gradcam_targets_time.jsonl'))
    a = ap.parse_args()
    from oracle import ref_cpu
    from models.rovit_kan import RoViTKAN
    dev = torch.device('cuda:0')
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    m = m.to(dev).eval()

    modes = {t: (lambda x, t=t: m.grad_cam_pp(x, target=t)) for t in TARGETS}
    modes['all_one_call'] = lambda x: m.grad_cam_pp(x, target=TARGETS)
    modes['all_separate'] = lambda x: [m.grad_cam_pp(x, target=t) for t in TARGETS]
    modes['hooks_kan'] = lambda x: hook_path_kan(m, x)
    lines = []
    for B in a.batch:
        x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B)).to(dev)
        for _ in range(a.warmup):
            for fn in modes.values():
                fn(x)
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
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
