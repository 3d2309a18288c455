"""Time the image gradients at one or more batch sizes and append one JSON line per (batch, mode) to profiles/input_grad_time.jsonl.

  train_fwd_bwd          : trainable backbone, forward + backward of the joint loss (every weight gradient), images without grad
  train_fwd_bwd_image    : the same with images that require grad (+ rovit_patch_embed_dgrad, x.grad)
  frozen_image           : frozen backbone, forward + backward to x.grad (rovit_vit_backward_input with no weight gradients)
  input_gradients        : m.input_gradients(x, target='class') (eval semantics, own workspace)
  ig32                   : m.input_gradients(x, steps=32) -- integrated gradients, interpolants stacked into the backbone calls
  ig32_loop              : the same integrated gradients as a Python loop of 32 autograd passes through the frozen model (at batch <= 8)

Device-event times; --warmup calls of every mode first, then --repeats rounds in which the modes run interleaved, one call each per
round; the median and min per mode are reported (the protocol of tools/time_gradcam.py).  The pixel kernel alone:
rocprofv3 --kernel-trace --stats -- python tools/time_input_grad.py --batch 256 --repeats 3 --out <scratch file>
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, nargs='+', default=[1, 8, 64, 256])
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'input_grad_time.jsonl'))
    a = ap.parse_args()
    from oracle import ref_cpu
    from models.rovit_kan import RoViTKAN
    dev = torch.device('cuda:0')
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    m = m.to(dev).eval()
    backbone = list(m.backbone.parameters())

    def joint(out):
        B = out['cls_logits'].shape[0]
        y = torch.arange(B, device=dev) % 4
        return ref_cpu.joint_loss(out, y, (y + 1) % 4, stage=4)['total_loss']

    def train(x, image):
        for p in backbone:
            p.requires_grad_(True)
        xg = x.clone().requires_grad_(image)
        joint(m(xg)).backward()
        m.zero_grad(set_to_none=True)

    def frozen(x):
        for p in backbone:
            p.requires_grad_(False)
        xg = x.clone().requires_grad_(True)
        out = m(xg)
        torch.autograd.grad(out['cls_logits'][:, 0].sum(), xg)
        for p in backbone:
            p.requires_grad_(True)

    def ig_loop(x, steps=32):
        for p in m.parameters():
            p.requires_grad_(False)
        tot = torch.zeros_like(x)
        for s in range(1, steps + 1):
            xi = ((s / steps) * x).requires_grad_(True)
            out = m(xi)
            tot += torch.autograd.grad(out['cls_logits'][:, 0].sum(), xi)[0]
        for p in m.parameters():
            p.requires_grad_(True)
        return x * tot / steps

    lines = []
    for B in a.batch:
        x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B)).to(dev)
        modes = {'train_fwd_bwd': lambda x: train(x, False), 'train_fwd_bwd_image': lambda x: train(x, True), 'frozen_image': frozen,
                 'input_gradients': lambda x: m.input_gradients(x, target='class', class_idx=0)}
        if B <= 8:
            modes['ig32'] = lambda x: m.input_gradients(x, target='class', class_idx=0, steps=32)
            modes['ig32_loop'] = ig_loop
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
