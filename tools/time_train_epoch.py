"""Time one training epoch, the replaced loop against ``training.Trainer.train_epoch``, and append JSON lines to
profiles/train_epoch_time.jsonl.

--images (8 192) resident images from the uint8 store (DeviceAugmentLoader), curriculum stage 4, CutMix / MixUp on, RoViTAdamW, at every
batch size of --batch (32 and 256):
  loop    : the loop the repository's documents gave before (INTEGRATION.md section C as it stood, training/trainer.py:79-160): the loss
            twice on the same head outputs, lam * a[k] + (1 - lam) * b[k] on the five entries, six .item() per step
  trainer : training.Trainer.train_epoch -- one rovit_joint_loss_mixed launch per step, one synchronisation per epoch
Both arms drive the same model and optimizer in the same process and alternate; every shape is warmed by one epoch of each arm; a repeat
is one whole epoch, host clock between two device synchronisations; median, min and max over --epochs repeats per arm.

--trace ARM: run --trace-steps steps of one arm at one batch size between two marks (three train_final_kernel launches in a row, on
buffers made before the warm-up), for a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_train_epoch.py --trace ARM --batch B`` run (profiler runs are not timed);
--kernel-trace CSV --trace ARM --batch B: count the kernel dispatches between the last two marks of that run's kernel_trace.csv and append the
launches per step to the same .jsonl.
"""
import argparse
import contextlib
import csv
import ctypes
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)

CLASS_NAMES = ["Healthy Leaf", "Leaf Holes", "Black Spot", "Dry Leaf"]
SEVERITY = {n: i for i, n in enumerate(CLASS_NAMES)}
MIX = dict(use_cutmix=True, use_mixup=True, cutmix_alpha=1.0, mixup_alpha=0.2)
STAGE = 4
SENTINEL = 'train_final_kernel'


def stage_for_epoch(epoch):
    return STAGE


def setup(images, batch, dev):
    from data.dataset import create_dataloaders
    from models.rovit_kan import RoViTKAN
    from oracle import ref_cpu
    from training import JointLoss, Trainer, build_optimizer, build_scheduler
    torch.manual_seed(0)
    np.random.seed(0)
    n = int(round(images / 0.8))                         # the 80 % training split is then --images images
    loader = create_dataloaders(None, None, CLASS_NAMES, SEVERITY, batch_size=batch, seed=0, synthetic=n, device=dev, device_cache=True)[0]
    cfg = SimpleNamespace(train=SimpleNamespace(learning_rate=1e-4, weight_decay=1e-4, epochs=1, early_stop_patience=1),
                          flags=SimpleNamespace(mixed_precision=True, gradient_clip=1.0, freeze_backbone_epochs=0, curriculum=True, **MIX),
                          paths=SimpleNamespace(checkpoints_dir='.'), get_stage_for_epoch=stage_for_epoch)
    model = RoViTKAN(pretrained=False)
    model.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    model = model.to(dev)
    opt = build_optimizer(model, cfg)
    loss_fn = JointLoss(1.0, 0.5, 0.5, 2.0, focal_alpha=loader.dataset.dataset.get_class_weights().to(dev))
    trainer = Trainer(model, loader, None, opt, build_scheduler(opt, cfg), loss_fn, cfg, dev)
    return trainer


def loop_epoch(t, max_steps=None):
    """The replaced loop: training/trainer.py:79-160 on the drop-in pieces, six .item() per step."""
    from data.transforms import cutmix_or_mixup
    model, opt, loss_fn, dev = t.model, t.optimizer, t.loss_fn, t.device
    model.train()
    model.curriculum_stage = STAGE
    sums = [0.0] * 5
    correct = total = steps = 0
    for images, class_labels, severity_labels in t.train_loader:
        images, class_labels, severity_labels = images.to(dev), class_labels.to(dev), severity_labels.to(dev)
        images, la, lb, lam = cutmix_or_mixup(images, class_labels, **MIX)
        outputs = model(images)
        a, b = loss_fn(outputs, la, severity_labels, STAGE), loss_fn(outputs, lb, severity_labels, STAGE)
        losses = {k: lam * a[k] + (1 - lam) * b[k] for k in a}
        loss = losses['total_loss']
        opt.zero_grad()
        loss.backward()
        opt.step()
        sums[0] += loss.item()
        for i, k in enumerate(('cls_loss', 'ord_loss', 'unc_loss', 'kan_loss'), 1):
            sums[i] += losses[k].item()
        _, predicted = outputs['cls_logits'].max(1)
        total += class_labels.size(0)
        correct += predicted.eq(class_labels).sum().item()
        steps += 1
        if max_steps is not None and steps >= max_steps:
            break
    return {'loss': sums[0] / steps, 'accuracy': 100. * correct / total}


def trainer_epoch(t, max_steps=None):
    with open(os.devnull, 'w') as null, contextlib.redirect_stdout(null):          # the progress marks: written, not shown
        if max_steps is None:
            return t.train_epoch(1)
        import itertools
        from rovit_hip.training import train_epoch
        flags = t.config.flags
        return train_epoch(t.model, itertools.islice(iter(t.train_loader), max_steps), t.optimizer, t.loss_fn, STAGE, mix_loss=t.mix_loss,
                           gradient_clip=flags.gradient_clip, **MIX)


ARMS = {'loop': loop_epoch, 'trainer': trainer_epoch}


def stats(v):
    s = sorted(v)
    return s[len(s) // 2], s[0], s[-1]


def measure(a, dev, lines):
    for batch in a.batch:
        t = setup(a.images, batch, dev)
        steps = len(t.train_loader)
        last = {k: fn(t) for k, fn in ARMS.items()}          # warm every shape: one epoch of each arm
        times = {k: [] for k in ARMS}
        for _ in range(a.epochs):
            for name, fn in ARMS.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[name] = fn(t)
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        med = {k: stats(v)[0] for k, v in times.items()}
        for name, v in times.items():
            m, lo, hi = stats(v)
            rec = {'case': 'epoch', 'arm': name, 'batch': batch, 'images': a.images, 'steps_per_epoch': steps, 'stage': STAGE,
                   'median_ms_per_epoch': round(m * 1e3, 2), 'min_ms_per_epoch': round(lo * 1e3, 2), 'max_ms_per_epoch': round(hi * 1e3, 2),
                   'median_ms_per_step': round(m * 1e3 / steps, 4), 'median_images_per_s': round(a.images / m, 1),
                   'spread': round((hi - lo) / m, 4), 'epochs': len(v), 'last_loss': round(float(last[name]['loss']), 5),
                   'device': torch.cuda.get_device_name(0)}
            if name == 'trainer':
                rec['loop_over_trainer'] = round(med['loop'] / med['trainer'], 4)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del t
        torch.cuda.empty_cache()


MARK = 3          # a mark is MARK finalise launches in a row; neither arm ever launches more than one in a row


def make_mark(dev):
    """A mark for the trace: MARK train_final_kernel launches on a one-row table and nothing else.  The buffers are made and filled here,
    before the warm-up, so that launching a mark later dispatches no other kernel (no fill) inside the counted window."""
    from rovit_hip import native
    table = torch.zeros((1, native.TRAIN_ROW_WORDS), dtype=torch.int32, device=dev)
    result = torch.empty(native.TRAIN_RESULT_WORDS, dtype=torch.int64, device=dev)
    d = native.TrainFinal()
    d.n_rows, d.capacity, d.table, d.result = 1, 1, native.ptr(table), native.ptr(result)

    def mark():
        torch.cuda.synchronize()
        for _ in range(MARK):
            native.call('rovit_train_finalize', ctypes.byref(d), native.stream_ptr())
        torch.cuda.synchronize()
    mark.keep = (table, result, d)
    return mark


def trace(a, dev):
    t = setup(max(a.images, a.batch[0] * a.trace_steps), a.batch[0], dev)
    mark = make_mark(dev)
    ARMS[a.trace](t, a.trace_steps)                      # warm
    mark()
    ARMS[a.trace](t, a.trace_steps)
    mark()
    print(f'trace run done: {a.trace_steps} steps of arm {a.trace} at batch {a.batch[0]} between two marks of {MARK} {SENTINEL} launches')


def cut_at_marks(names):
    """(first, last): names[first:last] are the dispatches between the last two marks.  The trace carries no kernel arguments, so a mark
    is told by its position: a run of at least MARK consecutive train_final_kernel dispatches, of which the last MARK are the mark (a
    finalise of the arm's own that happens to touch the mark stays inside the window)."""
    runs, i = [], 0
    while i < len(names):
        if SENTINEL in names[i]:
            j = i
            while j < len(names) and SENTINEL in names[j]:
                j += 1
            if j - i >= MARK:
                runs.append((i, j))
            i = j
        else:
            i += 1
    if len(runs) < 2:
        raise SystemExit(f'{len(runs)} marks of {MARK} consecutive {SENTINEL} dispatches, expected two')
    return runs[-2][1], runs[-1][1] - MARK


def short_name(kernel_name):
    n = kernel_name.replace('(anonymous namespace)::', '')
    if n.startswith('void '):
        n = n[5:]
    for stop in '(<':
        n = n.split(stop)[0]
    return n[-60:]


def kernel_trace(a):
    with open(a.kernel_trace) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp']))
    first, last = cut_at_marks([r['Kernel_Name'] for r in rows])
    inner = rows[first:last]
    # the trainer arm ends its pass with its own finalise and the copy of the result block (a copy kernel in the trace): from that
    # finalise on, the dispatches are the epoch's, not a step's
    ends = [i for i, r in enumerate(inner) if SENTINEL in r['Kernel_Name']]
    if len(ends) > 1:
        raise SystemExit(f'{a.kernel_trace}: {len(ends)} {SENTINEL} dispatches inside the counted pass, expected at most one')
    own = len(inner) - ends[0] if ends else 0
    inner = inner[:len(inner) - own]
    launches = len(inner)
    names = {}
    for r in inner:
        names[short_name(r['Kernel_Name'])] = names.get(short_name(r['Kernel_Name']), 0) + 1
    top = sorted(names.items(), key=lambda kv: -kv[1])[:8]
    rec = {'case': 'launches', 'arm': a.trace, 'batch': a.batch[0], 'steps': a.trace_steps, 'kernel_dispatches': launches,
           'launches_per_step': round(launches / a.trace_steps, 2), 'epoch_end_launches': own, 'distinct_kernels': len(names),
           'most_frequent': [[k, v] for k, v in top]}
    print(json.dumps(rec))
    with open(a.out, 'a') as o:
        o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8192)
    ap.add_argument('--batch', type=int, nargs='+', default=[32, 256])
    ap.add_argument('--epochs', type=int, default=7, help='timed epochs per arm and batch size')
    ap.add_argument('--trace', choices=sorted(ARMS))
    ap.add_argument('--trace-steps', type=int, default=8)
    ap.add_argument('--kernel-trace', metavar='CSV')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_epoch_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.kernel_trace:
        if not a.trace:
            raise SystemExit('--kernel-trace needs --trace ARM and --batch B of the traced run')
        return kernel_trace(a)
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_train_epoch.py measures on the GPU; no device found')
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
