"""Time the weight average inside the AdamW launch against the recipe it replaces, and append JSON lines to profiles/ema_time.jsonl.

One process, full model at batch 256, curriculum stage 4, device-resident synthetic batches, one model and one RoViTAdamW (built with
``ema_decay``, so the average's buffers exist; ``optimizer.ema_decay`` is set to None for the arms without it, which is the whole switch
``step()`` looks at).  A step is forward + JointLoss + zero_grad + backward + ``optimizer.step()``.  Three arms alternate:
  off    : the average off -- ``step()`` calls rovit_adamw_flat_multi, the path the optimizer had before it could average
  fused  : the average on -- ``step()`` calls rovit_adamw_ema_flat_multi instead (same number of launches)
  recipe : the average off, then ``torch._foreach_lerp_(shadow_params, params, 1 - d)`` over a second set of tensors, what a user writes
           without this feature
Every arm is warmed by one repeat; a repeat is --steps steps, host clock between two device synchronisations; median, min and max over
--repeats repeats per arm.  Then ``Trainer.train_epoch`` over --images (8 192) resident images (uint8 store, CutMix / MixUp on) with the
average on and off, alternating, --epochs repeats each.

--trace ARM: --trace-steps steps of one arm between two marks, for a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_ema.py --trace ARM`` run (no counters in that run; profiler runs are not timed);
--kernel-trace CSV --trace ARM: count the kernel dispatches between the marks of that run's kernel_trace.csv and append the launches per
step to the same .jsonl.
"""
import argparse
import contextlib
import csv
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)
from time_train_epoch import cut_at_marks, make_mark, setup as trainer_setup, short_name, stats  # noqa: E402

STAGE = 4
DECAY = 0.999


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
    opt = RoViTAdamW(model, lr=1e-4, weight_decay=1e-4, max_grad_norm=1.0, ema_decay=DECAY)
    loss_fn = JointLoss(1.0, 0.5, 0.5, 2.0)
    g = torch.Generator(device=dev).manual_seed(1)
    batches = [(torch.randn(batch, 3, 224, 224, device=dev, generator=g), torch.randint(0, 4, (batch,), device=dev, generator=g))
               for _ in range(n_batches)]
    params = list(model.parameters())
    shadow = [p.detach().clone() for p in params]             # the recipe's second set of tensors
    return model, opt, loss_fn, batches, params, shadow


def run_steps(arm, ctx, steps):
    model, opt, loss_fn, batches, params, shadow = ctx
    opt.ema_decay = DECAY if arm == 'fused' else None
    for i in range(steps):
        x, y = batches[i % len(batches)]
        loss = loss_fn(model(x), y, y, STAGE)['total_loss']
        opt.zero_grad()
        loss.backward()
        opt.step()
        if arm == 'recipe':
            with torch.no_grad():
                torch._foreach_lerp_(shadow, params, 1.0 - DECAY)


ARMS = ('off', 'fused', 'recipe')


def measure_steps(a, dev, lines):
    ctx = setup(a.batch, dev)
    for arm in ARMS:                                          # warm every arm
        run_steps(arm, ctx, a.steps)
    torch.cuda.synchronize()
    times = {arm: [] for arm in ARMS}
    for _ in range(a.repeats):
        for arm in ARMS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(arm, ctx, a.steps)
            torch.cuda.synchronize()
            times[arm].append((time.perf_counter() - t0) / a.steps)
    n_params = sum(p.numel() for p in ctx[4])
    med = {arm: stats(v)[0] for arm, v in times.items()}
    for arm, v in times.items():
        m, lo, hi = stats(v)
        rec = {'case': 'step', 'arm': arm, 'batch': a.batch, 'stage': STAGE, 'steps_per_repeat': a.steps, 'repeats': len(v),
               'median_ms_per_step': round(m * 1e3, 4), 'min_ms_per_step': round(lo * 1e3, 4), 'max_ms_per_step': round(hi * 1e3, 4),
               'spread': round((hi - lo) / m, 4), 'parameters': n_params, 'tensors': len(ctx[4]), 'ema_decay': DECAY,
               'device': torch.cuda.get_device_name(0)}
        if arm != 'off':
            rec['median_minus_off_us'] = round((med[arm] - med['off']) * 1e6, 2)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    rec = {'case': 'step_condition', 'slowest_fused_ms': round(max(times['fused']) * 1e3, 4), 'fastest_recipe_ms': round(min(times['recipe']) * 1e3, 4),
           'slowest_fused_is_faster_than_fastest_recipe': max(times['fused']) < min(times['recipe'])}
    print(json.dumps(rec), flush=True)
    lines.append(rec)


def measure_epochs(a, dev, lines):
    t = trainer_setup(a.images, a.batch, dev)
    from rovit_hip.optim import RoViTAdamW
    # the same trainer with an averaging optimizer in place of its own: the model's parameters move into the new optimizer's buffers
    t.optimizer = RoViTAdamW(t.model, lr=1e-4, weight_decay=1e-4, max_grad_norm=1.0, ema_decay=DECAY)
    steps = len(t.train_loader)

    def epoch(on):
        t.optimizer.ema_decay = DECAY if on else None
        with open(os.devnull, 'w') as null, contextlib.redirect_stdout(null):
            return t.train_epoch(1)
    for on in (False, True):
        epoch(on)
    times = {False: [], True: []}
    for _ in range(a.epochs):
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            epoch(on)
            torch.cuda.synchronize()
            times[on].append(time.perf_counter() - t0)
    for on, v in times.items():
        m, lo, hi = stats(v)
        rec = {'case': 'epoch', 'ema': on, 'batch': a.batch, 'images': a.images, 'steps_per_epoch': steps, 'stage': STAGE,
               'median_ms_per_epoch': round(m * 1e3, 2), 'min_ms_per_epoch': round(lo * 1e3, 2), 'max_ms_per_epoch': round(hi * 1e3, 2),
               'median_ms_per_step': round(m * 1e3 / steps, 4), 'median_images_per_s': round(a.images / m, 1), 'epochs': len(v),
               'device': torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)


def trace(a, dev):
    ctx = setup(a.batch, dev)
    mark = make_mark(dev)
    run_steps(a.trace, ctx, a.trace_steps)                    # warm
    mark()
    run_steps(a.trace, ctx, a.trace_steps)
    mark()
    print(f'trace run done: {a.trace_steps} steps of arm {a.trace} at batch {a.batch} between two marks')


def kernel_trace(a):
    with open(a.kernel_trace) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp']))
    first, last = cut_at_marks([r['Kernel_Name'] for r in rows])
    inner = rows[first:last]
    names = {}
    for r in inner:
        names[short_name(r['Kernel_Name'])] = names.get(short_name(r['Kernel_Name']), 0) + 1
    optim = {k: v for k, v in names.items() if 'adamw' in k or 'sq_norm' in k or 'lerp' in k.lower() or 'swap' in k}
    rec = {'case': 'launches', 'arm': a.trace, 'batch': a.batch, 'steps': a.trace_steps, 'kernel_dispatches': len(inner),
           'launches_per_step': round(len(inner) / a.trace_steps, 2), 'distinct_kernels': len(names), 'optimizer_kernels': optim}
    print(json.dumps(rec))
    with open(a.out, 'a') as o:
        o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20, help='steps per timed repeat')
    ap.add_argument('--repeats', type=int, default=7, help='timed repeats per arm')
    ap.add_argument('--images', type=int, default=8192)
    ap.add_argument('--epochs', type=int, default=7, help='timed epochs with the average on and off')
    ap.add_argument('--trace', choices=ARMS)
    ap.add_argument('--trace-steps', type=int, default=8)
    ap.add_argument('--kernel-trace', metavar='CSV')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ema_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.kernel_trace:
        if not a.trace:
            raise SystemExit('--kernel-trace needs --trace ARM of the traced run')
        return kernel_trace(a)
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_ema.py measures on the GPU; no device found')
    dev = torch.device('cuda:0')
    if a.trace:
        return trace(a, dev)
    lines = []
    measure_steps(a, dev, lines)
    torch.cuda.empty_cache()
    measure_epochs(a, dev, lines)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
