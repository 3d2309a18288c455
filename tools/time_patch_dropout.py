"""Time the training step with PatchDropout against the dense step, and append JSON lines to profiles/patch_dropout_time.jsonl.

One process, full model, curriculum stage 4, device-resident synthetic batches, one model and one RoViTAdamW.  A step is forward +
JointLoss + zero_grad + backward + ``optimizer.step()``.  Arms: ``dense`` (patch dropout off: the existing path) and ``keep0.75``,
``keep0.5``, ``keep0.25`` (``set_patch_dropout(keep)``: 147, 98 and 49 of the 196 patches).  The arms alternate inside every repeat; every
arm is warmed by one repeat; a repeat is --steps steps, host clock between two device synchronisations; median, min and max over --repeats
repeats per arm and batch size.  ``--arms dense`` also runs on a tree without the feature (the parent commit's dense step, same tool).

--trace ARM: --trace-steps steps of one arm, for a separate ``rocprofv3 --kernel-trace --stats -- python tools/time_patch_dropout.py
--trace ARM --batch B`` run (no counters in that run; profiler runs are not timed); --kernel-stats CSV --trace ARM --batch B: take the draw
and scatter kernels' rows of that run's kernel_stats.csv and append them to the same .jsonl.
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

STAGE = 4
KEEPS = {'dense': 1.0, 'keep0.75': 0.75, 'keep0.5': 0.5, 'keep0.25': 0.25}
KERNELS = ('patch_dropout_draw_kernel', 'scatter_token_rows_kernel')


def stats(v):
    s = sorted(v)
    return s[len(s) // 2], s[0], s[-1]


def setup(batch, dev, n_batches=2):
    from models.rovit_kan import RoViTKAN
    from oracle import ref_cpu
    from rovit_hip.losses import JointLoss
    from rovit_hip.optim import RoViTAdamW
    torch.manual_seed(0)
    model = RoViTKAN(pretrained=False)
    model.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    model = model.to(dev).train()
    model.curriculum_stage = STAGE
    opt = RoViTAdamW(model, lr=1e-4, weight_decay=1e-4, max_grad_norm=1.0)
    loss_fn = JointLoss(1.0, 0.5, 0.5, 2.0)
    g = torch.Generator(device=dev).manual_seed(1)
    batches = [(torch.randn(batch, 3, 224, 224, device=dev, generator=g), torch.randint(0, 4, (batch,), device=dev, generator=g))
               for _ in range(n_batches)]
    return model, opt, loss_fn, batches


def run_steps(arm, ctx, steps):
    model, opt, loss_fn, batches = ctx
    if arm != 'dense' or hasattr(model, 'set_patch_dropout'):
        step = model.backbone.patch_dropout_step
        model.set_patch_dropout(KEEPS[arm], seed=0)
        model.backbone.patch_dropout_step = step          # the counter runs on: new subsets in every repeat
    for i in range(steps):
        x, y = batches[i % len(batches)]
        loss = loss_fn(model(x), y, y, STAGE)['total_loss']
        opt.zero_grad()
        loss.backward()
        opt.step()


def measure(a, dev, lines):
    for batch in a.batch:
        ctx = setup(batch, dev)
        for arm in a.arms:                                    # warm every arm
            run_steps(arm, ctx, a.steps)
        torch.cuda.synchronize()
        times = {arm: [] for arm in a.arms}
        for _ in range(a.repeats):
            for arm in a.arms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_steps(arm, ctx, a.steps)
                torch.cuda.synchronize()
                times[arm].append((time.perf_counter() - t0) / a.steps)
        med = {arm: stats(v)[0] for arm, v in times.items()}
        for arm, v in times.items():
            m, lo, hi = stats(v)
            k = 196
            if arm != 'dense':                                # the module's own rounding rule (absent on a tree without the feature)
                from rovit_hip.patch_dropout import kept_patches
                k = kept_patches(KEEPS[arm])
            rec = {'case': 'step', 'arm': arm, 'keep': KEEPS[arm], 'kept_patches': k, 'token_rows': batch * (1 + k), 'batch': batch, 'stage': STAGE,
                   'steps_per_repeat': a.steps, 'repeats': len(v), 'median_ms_per_step': round(m * 1e3, 4),
                   'min_ms_per_step': round(lo * 1e3, 4), 'max_ms_per_step': round(hi * 1e3, 4), 'spread': round((hi - lo) / m, 4),
                   'device': torch.cuda.get_device_name(0)}
            if a.tag:
                rec['tree'] = a.tag
            if arm != 'dense' and 'dense' in med:
                rec['median_over_dense'] = round(med[arm] / med['dense'], 4)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del ctx
        torch.cuda.empty_cache()


def trace(a, dev):
    ctx = setup(a.batch[0], dev)
    run_steps(a.trace, ctx, a.trace_steps)                    # warm
    torch.cuda.synchronize()
    run_steps(a.trace, ctx, a.trace_steps)
    torch.cuda.synchronize()
    print(f'trace run done: 2 x {a.trace_steps} steps of arm {a.trace} at batch {a.batch[0]}')


def kernel_stats(a):
    with open(a.kernel_stats) as f:
        rows = list(csv.DictReader(f))
    total = sum(float(r['TotalDurationNs']) for r in rows)
    for r in rows:
        for name in KERNELS:
            if name in r['Name']:
                rec = {'case': 'kernel', 'kernel': name, 'arm': a.trace, 'batch': a.batch[0], 'calls': int(r['Calls']),
                       'average_us': round(float(r['AverageNs']) / 1e3, 3), 'min_us': round(float(r['MinNs']) / 1e3, 3),
                       'max_us': round(float(r['MaxNs']) / 1e3, 3), 'share_of_kernel_time': round(float(r['TotalDurationNs']) / total, 6)}
                print(json.dumps(rec))
                with open(a.out, 'a') as o:
                    o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, nargs='+', default=[32, 256])
    ap.add_argument('--arms', nargs='+', choices=sorted(KEEPS), default=list(KEEPS))
    ap.add_argument('--steps', type=int, default=100, help='steps per timed repeat')
    ap.add_argument('--repeats', type=int, default=7, help='timed repeats per arm')
    ap.add_argument('--tag', help="recorded as 'tree' (e.g. parent)")
    ap.add_argument('--trace', choices=sorted(KEEPS))
    ap.add_argument('--trace-steps', type=int, default=8)
    ap.add_argument('--kernel-stats', metavar='CSV')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'patch_dropout_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.kernel_stats:
        if not a.trace:
            raise SystemExit('--kernel-stats needs --trace ARM of the traced run')
        return kernel_stats(a)
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_patch_dropout.py measures on the GPU; no device found')
    dev = torch.device('cuda:0')
    if a.trace:
        return trace(a, dev)
    lines = []
    measure(a, dev, lines)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
