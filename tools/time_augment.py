"""Time the device-resident image store's fused augmentation and append one JSON line per (case, arm) to profiles/augment_time.jsonl.

Per batch, at batch 256 and 32 over --images synthetic 224 x 224 images, for the default config (flip + normalise) and the full one of
the tests (crop, ratio, rotation, both flips, four colour jitters):
  fused  : DeviceImageStore.batch -- ONE launch: gather, draw, resample, colour, normalise
  recipe : augment_reference in fp32 on the same device with the rows already drawn -- the torch recipe a user would write
  parent : (default config only) what the loaders did before: index_select on fp32-resident images + augmented_transforms()
           (RandomHorizontalFlip + Normalize as torch ops), the DeviceBatchLoader path
Every arm runs --batches consecutive batches per repeat (a repeat is then milliseconds, not microseconds); the arms alternate; every case
is warmed up; host clock between two device synchronisations; median, min, max per arm, per BATCH.  The fused arm is also set against
the traffic floor of its launch (uint8 read + fp32 written at 6.29 TB/s).
Per epoch (--epoch-batch, model + JointLoss + RoViTAdamW at curriculum stage 4): images/s of one training epoch fed by DeviceAugmentLoader
(uint8 store) and by DeviceBatchLoader (fp32-resident images, augmented_transforms()), alternating, median of --epochs each.
Resident bytes of both stores.

--kernels-only: the fused arm alone, KERNEL_RUNS launches for each of the four (config, batch) cases in a fixed order, for a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_augment.py --kernels-only`` run (no counters in that run);
--kernel-trace CSV appends the augment_batch_kernel durations of that run's kernel_trace.csv, split by case, to the same .jsonl.
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

CLASS_NAMES = ["Healthy Leaf", "Leaf Holes", "Black Spot", "Dry Leaf"]
SEVERITY = {n: i for i, n in enumerate(CLASS_NAMES)}
HBM_COPY_BYTES_PER_S = 6.29e12          # MI355X copy rate the floor is stated against
KERNEL_RUNS = 20
BATCHES = (256, 32)


def configs():
    from rovit_hip.augment import AugmentConfig
    return {'default': AugmentConfig(),
            'full': AugmentConfig(hflip=0.5, vflip=0.5, scale=(0.25, 1.0), ratio=(3 / 4, 4 / 3), rotate_deg=30.0, brightness=0.4,
                                  contrast=0.4, saturation=0.4, hue=0.1)}


def make_store(n, dev, seed=0):
    from rovit_hip.augment import DeviceImageStore
    lab = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(seed))
    return DeviceImageStore.synthetic(lab, lab, dev, size=(224, 224), seed=seed)


def time_arms(arms, repeats, min_seconds, warmup):
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    times = {k: [] for k in arms}
    while min(len(v) for v in times.values()) < repeats or min(sum(v) for v in times.values()) < min_seconds:
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    return times


def stats(v, scale):
    t = sorted(x * scale for x in v)
    return {'median': t[len(t) // 2], 'min': t[0], 'max': t[-1], 'repeats': len(t)}


def per_batch(a, dev, lines):
    from data.transforms import augmented_transforms
    from rovit_hip.augment import augment_reference
    store = make_store(a.images, dev)
    fp32 = torch.randn(a.images, 3, 224, 224, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    tf = augmented_transforms()
    order = torch.randperm(a.images, generator=torch.Generator().manual_seed(1)).to(dev)
    for cname, cfg in configs().items():
        for B in BATCHES:
            sels = [order[k * B:(k + 1) * B] for k in range(a.batches)]
            rows = [store.batch(s, cfg, 1, 0, return_params=True)[1] for s in sels]
            out = torch.empty(B, 3, 224, 224, device=dev)
            arms = {'fused': lambda: [store.batch(s, cfg, 1, 0, out=out) for s in sels],
                    'recipe': lambda: [augment_reference(store.images, s, r, (224, 224), dtype=torch.float32) for s, r in zip(sels, rows)]}
            if cname == 'default':
                arms['parent'] = lambda: [tf(fp32.index_select(0, s)) for s in sels]
            times = time_arms(arms, a.repeats, a.min_seconds, a.warmup)
            med = {k: stats(v, 1e6 / a.batches)['median'] for k, v in times.items()}
            floor_us = (B * 3 * 224 * 224 * (1 + 4)) / HBM_COPY_BYTES_PER_S * 1e6
            for name, v in times.items():
                s = stats(v, 1e6 / a.batches)
                rec = {'case': 'batch', 'config': cname, 'batch': B, 'images': a.images, 'arm': name, 'batches_per_repeat': a.batches,
                       'median_us_per_batch': round(s['median'], 2), 'min_us_per_batch': round(s['min'], 2),
                       'max_us_per_batch': round(s['max'], 2), 'repeats': s['repeats'], 'device': torch.cuda.get_device_name(0)}
                if name == 'fused':
                    rec['traffic_floor_us'] = round(floor_us, 2)
                    rec['fused_over_floor'] = round(med['fused'] / floor_us, 2)
                    rec['recipe_over_fused'] = round(med['recipe'] / med['fused'], 2)
                    if 'parent' in med:
                        rec['parent_over_fused'] = round(med['parent'] / med['fused'], 2)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    lines.append({'case': 'resident_bytes', 'images': a.images, 'uint8_store': store.nbytes,
                  'fp32_resident': fp32.numel() * 4 + 2 * a.images * 8})
    print(json.dumps(lines[-1]), flush=True)


def per_epoch(a, dev, lines):
    from data.dataset import create_dataloaders
    from data.transforms import augmented_transforms, original_transforms
    from models.rovit_kan import RoViTKAN
    from oracle import ref_cpu
    from rovit_hip.losses import JointLoss
    from rovit_hip.optim import RoViTAdamW
    n = int(round(a.images / 0.8))                       # the 80 % training split is then --images images
    kw = dict(class_names=CLASS_NAMES, severity_map=SEVERITY, batch_size=a.epoch_batch, seed=0, synthetic=n, device=dev)
    loaders = {'store_loader': create_dataloaders(None, None, device_cache=True, **kw)[0],
               'fp32_loader': create_dataloaders(None, None, augmented_transform=augmented_transforms(),
                                                 original_transform=original_transforms(), **kw)[0]}
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    m = m.to(dev).train()
    m.curriculum_stage = 4
    opt = RoViTAdamW(m, lr=1e-4)
    loss_fn = JointLoss(1.0, 0.5, 0.5, 2.0)

    def epoch(loader):
        seen = 0
        for x, c, s in loader:
            x, c, s = x.to(dev), c.to(dev), s.to(dev)
            opt.zero_grad()
            loss_fn(m(x), c, s, 4)['total_loss'].backward()
            opt.step()
            seen += x.shape[0]
        return seen

    seen = {k: epoch(v) for k, v in loaders.items()}         # warm-up epoch of each
    times = time_arms({k: (lambda v=v: epoch(v)) for k, v in loaders.items()}, a.epochs, 0.0, 0)
    for name, v in times.items():
        s = stats(v, 1.0)
        rec = {'case': 'epoch', 'arm': name, 'batch': a.epoch_batch, 'images_per_epoch': seen[name],
               'median_images_per_s': round(seen[name] / s['median'], 1), 'min_images_per_s': round(seen[name] / s['max'], 1),
               'max_images_per_s': round(seen[name] / s['min'], 1), 'epochs': s['repeats'], 'device': torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)


def kernel_cases():
    return [(c, B) for c in configs() for B in BATCHES]


def kernels_only(a, dev):
    store = make_store(a.images, dev)
    order = torch.randperm(a.images, generator=torch.Generator().manual_seed(1)).to(dev)
    cfgs = configs()
    for cname, B in kernel_cases():
        out = torch.empty(B, 3, 224, 224, device=dev)
        for k in range(KERNEL_RUNS):
            lo = (k * B) % (a.images - B + 1)
            store.batch(order[lo:lo + B], cfgs[cname], 1, 0, out=out)
        torch.cuda.synchronize()
    print('kernels-only run done:', KERNEL_RUNS, 'launches for each of', kernel_cases())


def kernel_trace(path, images, out):
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if 'augment_batch_kernel' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    cases = kernel_cases()
    if len(rows) != KERNEL_RUNS * len(cases):
        raise SystemExit(f'{path}: {len(rows)} augment_batch_kernel dispatches, expected {KERNEL_RUNS * len(cases)}')
    with open(out, 'a') as o:
        for k, (cname, B) in enumerate(cases):
            us = sorted((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows[k * KERNEL_RUNS:(k + 1) * KERNEL_RUNS])
            floor_us = (B * 3 * 224 * 224 * 5) / HBM_COPY_BYTES_PER_S * 1e6
            rec = {'case': 'kernel', 'kernel': 'augment_batch_kernel', 'config': cname, 'batch': B, 'images': images, 'calls': len(us),
                   'median_us': round(us[len(us) // 2], 2), 'min_us': round(us[0], 2), 'max_us': round(us[-1], 2),
                   'traffic_floor_us': round(floor_us, 2), 'median_over_floor': round(us[len(us) // 2] / floor_us, 2)}
            print(json.dumps(rec))
            o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8192)
    ap.add_argument('--batches', type=int, default=16, help='consecutive batches per timed repeat')
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--epoch-batch', type=int, default=256)
    ap.add_argument('--skip-epoch', action='store_true')
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--kernel-trace', metavar='CSV')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'augment_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.kernel_trace:
        return kernel_trace(a.kernel_trace, a.images, a.out)
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_augment.py measures on the GPU; no device found')
    dev = torch.device('cuda:0')
    if a.kernels_only:
        return kernels_only(a, dev)
    lines = []
    per_batch(a, dev, lines)
    if not a.skip_epoch:
        torch.cuda.empty_cache()
        per_epoch(a, dev, lines)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
