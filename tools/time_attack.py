"""Time a 10-step L-infinity PGD attack on the depth-12 model at batch 16 and 256 and append one JSON line per (batch, arm) to
profiles/attack_time.jsonl.

  pgd_attack      : model.adversarial_examples(x, y, eps=4/255, steps=10) -- the fused gradient route and the kernels of csrc/attack.hip
  torch_step      : the same gradient route and the same loop (random start, best-so-far bookkeeping) with the start and the step written
                    in torch elementwise operations: the difference to pgd_attack is the kernels alone
  autograd_recipe : what a user would write: x.requires_grad_(True), model(x) on a frozen backbone, F.cross_entropy(...).backward(), the
                    torch step (no best-so-far bookkeeping)
  input_gradients : one model.input_gradients(x) call, the yardstick a step is compared with (K steps should cost about K of them)

Device-event times.  One warm run of every arm, then --repeats (7) rounds in which the arms alternate, one call each per round; median,
min and max per arm are kept, and ms_per_step = median / steps for the three attacks.
--kernels-only: pgd_attack alone, three calls at batch 256, for a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_attack.py --kernels-only`` run that gives the step kernel's own time (no counters
in that run; nothing is written to the profile file)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)

EPS, STEPS = 4 / 255, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, nargs='+', default=[16, 256])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'attack_time.jsonl'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_attack.py measures on the GPU; no device found')
    from oracle import ref_cpu
    from models.rovit_kan import RoViTKAN
    from rovit_hip import attack as A
    dev = torch.device('cuda:0')
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    m = m.to(dev).eval()
    inv_s, _, lo, hi = (torch.from_numpy(v).to(dev).view(1, 3, 1, 1) for v in A.constants())
    mean, std = (torch.tensor(v, device=dev).view(1, 3, 1, 1) for v in A._mean_std())
    r, al = EPS * inv_s, (2.5 * EPS / STEPS) * inv_s
    clamp = lambda v, l, h: torch.minimum(torch.maximum(v, l), h)

    def project(x, d1):
        y = clamp(x + clamp(d1, -r, r), lo, hi)
        d = clamp(y - x, -r, r)
        return d, clamp(x + d, lo, hi)

    def torch_step(x, y):
        route = A._Route(m, dev, 'ce', y, None, 1, 256)
        with torch.no_grad():
            delta, x_adv = project(x, (2 * torch.rand_like(x) - 1) * r)
            best_delta = torch.zeros_like(x)
            best = torch.full((x.shape[0],), -float('inf'), device=dev)
            for _ in range(STEPS):
                v, g = route.value_and_grad(x_adv)
                mask = v > best
                best = torch.where(mask, v, best)
                best_delta = torch.where(mask.view(-1, 1, 1, 1), delta, best_delta)
                delta, x_adv = project(x, delta + torch.sign(g) * al)
            v = route.value(x_adv)
            best_delta = torch.where((v > best).view(-1, 1, 1, 1), delta, best_delta)
            return clamp(x + best_delta, lo, hi)

    def recipe(x, y):
        flags = [p.requires_grad for p in m.parameters()]
        for p in m.parameters():
            p.requires_grad_(False)
        delta, _ = project(x, (2 * torch.rand_like(x) - 1) * r)
        for _ in range(STEPS):
            xa = (x + delta).requires_grad_(True)
            F.cross_entropy(m(xa)['cls_logits'], y).backward()
            delta, _ = project(x, delta + torch.sign(xa.grad) * al)
        for p, f in zip(m.parameters(), flags):
            p.requires_grad_(f)
        return x + delta

    if a.kernels_only:
        x = ((torch.rand(256, 3, 224, 224, device=dev) - mean) / std).contiguous()
        y = torch.arange(256, device=dev) % 4
        for _ in range(3):
            m.adversarial_examples(x, y, eps=EPS, steps=STEPS)
        torch.cuda.synchronize()
        return
    lines = []
    for B in a.batch:
        x = ((torch.rand(B, 3, 224, 224, generator=torch.Generator().manual_seed(B)).to(dev) - mean) / std).contiguous()
        y = torch.arange(B, device=dev) % 4
        arms = {'pgd_attack': lambda: m.adversarial_examples(x, y, eps=EPS, steps=STEPS), 'torch_step': lambda: torch_step(x, y),
                'autograd_recipe': lambda: recipe(x, y), 'input_gradients': lambda: m.input_gradients(x, target='class', class_idx=0)}
        for fn in arms.values():          # the warm run
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(a.repeats):
            for name, fn in arms.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                e.synchronize()
                times[name].append(s.elapsed_time(e))
        for name in arms:
            t = sorted(times[name])
            rec = {'arm': name, 'batch': B, 'norm': 'linf', 'steps': STEPS if name != 'input_gradients' else 0, 'depth': 12,
                   'median_ms': round(t[len(t) // 2], 3), 'min_ms': round(t[0], 3), 'max_ms': round(t[-1], 3), 'repeats': a.repeats,
                   'device': torch.cuda.get_device_name(0)}
            if name != 'input_gradients':
                rec['ms_per_step'] = round(t[len(t) // 2] / STEPS, 3)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
