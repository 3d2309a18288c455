"""Time the image corruptions of the device-resident store and append one JSON line per (case, arm) to profiles/corrupt_time.jsonl.

Per batch, at batch 256 and 32 over --images synthetic 224 x 224 images, for each of the eleven corruptions at severities 3 and 5:
  fused  : DeviceImageStore.corrupt -- ONE launch from the uint8 store (two for contrast): gather, corrupt, clamp, normalise
  recipe : the torch recipe a user would write on the same device, in fp32: randn / rand for the noises, F.conv2d with the same 2-D
           weights for the Gaussian and the disk, 2R + 1 grid_sample calls for the motion blur, avg_pool2d + repeat_interleave for
           pixelate, plain tensor ops for brightness / contrast / saturate; for jpeg there is no device recipe: PIL on the host with 16
           threads (encode + decode at the same quality, 4:4:4), including the copy to the host and back
Every arm runs --batches consecutive batches per repeat (one for the host jpeg arm); the arms alternate in one process; every case is
warmed up; host clock between two device synchronisations; median of --repeats (seven), min, max per arm, per BATCH.  The fused arm is
also set against the traffic floor of its launch (uint8 read + fp32 written at 6.29 TB/s: 38.5 MB + 154 MB per 256 images).

--kernels-only: the fused arm alone, KERNEL_RUNS launches of one corruption of each kernel shape at severity 5 and batch 256, in a fixed
order, for a separate ``rocprofv3 --kernel-trace --stats --output-format csv -- python tools/time_corrupt.py --kernels-only`` run (no counters in that run);
--kernel-trace CSV appends the kernel durations of that run's kernel_trace.csv to the same .jsonl.
"""
import argparse
import csv
import io
import json
import math
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)

HBM_COPY_BYTES_PER_S = 6.29e12          # MI355X copy rate the floor is stated against
KERNEL_RUNS = 20
BATCHES = (256, 32)
SEVERITIES = (3, 5)
KERNEL_CASES = (('gaussian_noise', 'corrupt_point_kernel'), ('pixelate', 'corrupt_cell_kernel'), ('defocus_blur', 'corrupt_stencil_kernel'),
                ('jpeg', 'corrupt_jpeg_kernel'))


def make_store(n, dev, seed=0):
    from rovit_hip.augment import DeviceImageStore
    lab = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(seed))
    return DeviceImageStore.synthetic(lab, lab, dev, size=(224, 224), seed=seed)


def normalise(z):
    from rovit_hip.augment import IMAGENET_MEAN, IMAGENET_STD
    mean, std = (torch.tensor(t, device=z.device).view(1, 3, 1, 1) for t in (IMAGENET_MEAN, IMAGENET_STD))
    return (z.clamp_(0.0, 1.0) - mean) / std


def stencil_weights(name, p, dev):
    if name == 'gaussian_blur':
        R = math.ceil(3.0 * p)
        k = torch.arange(-R, R + 1, dtype=torch.float64)
        w = torch.exp(-k * k / (2.0 * p * p))
        w = w / w.sum()
        return R, torch.outer(w, w).float().to(dev)
    R = math.floor(p)
    k = torch.arange(-R, R + 1, dtype=torch.float64)
    disk = ((k.view(-1, 1) ** 2 + k.view(1, -1) ** 2) <= p * p).double()
    return R, (disk / disk.sum()).float().to(dev)


def recipe(store, sel, name, p, seed):
    """The torch recipe of one batch (fp32, same device).  Not the reference: its draws are torch's own."""
    from rovit_hip.corrupt import motion_theta
    v = store.images.index_select(0, sel).float().div_(255.0)
    B, _, H, W = v.shape
    if name == 'gaussian_noise':
        z = v + p * torch.randn_like(v)
    elif name == 'shot_noise':
        z = v + (v / p).sqrt() * torch.randn_like(v)
    elif name == 'impulse_noise':
        u = torch.rand_like(v)
        z = torch.where(u < p / 2, torch.zeros_like(v), torch.where(u >= 1 - p / 2, torch.ones_like(v), v))
    elif name == 'brightness':
        z = v + p
    elif name == 'contrast':
        m = v.mean(dim=(2, 3), keepdim=True)
        z = m + p * (v - m)
    elif name == 'saturate':
        g = (v * torch.tensor([0.299, 0.587, 0.114], device=v.device).view(1, 3, 1, 1)).sum(dim=1, keepdim=True)
        z = g + p * (v - g)
    elif name == 'pixelate':
        b = int(p)
        cells = F.avg_pool2d(v, b, ceil_mode=True, count_include_pad=False)
        z = cells.repeat_interleave(b, dim=2).repeat_interleave(b, dim=3)[:, :, :H, :W]
    elif name in ('gaussian_blur', 'defocus_blur'):
        R, w = stencil_weights(name, p, v.device)
        padded = F.pad(v, (R, R, R, R), mode='replicate').view(B * 3, 1, H + 2 * R, W + 2 * R)
        z = F.conv2d(padded, w.view(1, 1, 2 * R + 1, 2 * R + 1)).view(B, 3, H, W)
    elif name == 'motion_blur':
        R = int(p)
        theta = torch.from_numpy(motion_theta(sel.cpu().numpy(), seed, np.float32)).to(v.device)
        ys, xs = torch.meshgrid(torch.arange(H, device=v.device, dtype=torch.float32), torch.arange(W, device=v.device, dtype=torch.float32),
                                indexing='ij')
        z = torch.zeros_like(v)
        for k in range(-R, R + 1):
            sx = (xs.unsqueeze(0) + k * torch.cos(theta).view(B, 1, 1)).clamp(0, W - 1)
            sy = (ys.unsqueeze(0) + k * torch.sin(theta).view(B, 1, 1)).clamp(0, H - 1)
            grid = torch.stack([(2 * sx + 1) / W - 1, (2 * sy + 1) / H - 1], dim=-1)
            z += F.grid_sample(v, grid, mode='bilinear', padding_mode='border', align_corners=False)
        z /= 2 * R + 1
    else:
        raise SystemExit(f'no device recipe for {name}')
    return normalise(z)


def host_jpeg(store, sel, quality, pool):
    """PIL round trip on the host, 16 threads: device -> host, encode + decode, host -> device, normalise."""
    from PIL import Image
    host = store.images.index_select(0, sel).permute(0, 2, 3, 1).contiguous().cpu().numpy()

    def one(img):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, 'JPEG', quality=quality, subsampling=0)
        return np.asarray(Image.open(buf).convert('RGB'))

    back = np.stack(list(pool.map(one, host)))
    return normalise(torch.from_numpy(back).to(store.device).permute(0, 3, 1, 2).float().div_(255.0))


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
    from concurrent.futures import ThreadPoolExecutor
    from rovit_hip.corrupt import CORRUPTIONS, corruption_param
    store = make_store(a.images, dev)
    order = torch.randperm(a.images, generator=torch.Generator().manual_seed(1)).to(dev)
    names = a.only.split(',') if a.only else CORRUPTIONS
    with ThreadPoolExecutor(max_workers=16) as pool:
        for name in names:
            for severity in SEVERITIES:
                p = corruption_param(name, severity)
                for B in BATCHES:
                    sels = [order[k * B:(k + 1) * B] for k in range(a.batches)]
                    out = torch.empty(B, 3, 224, 224, device=dev)
                    per_repeat = {'fused': a.batches, 'recipe': 1 if name == 'jpeg' else a.batches}
                    arms = {'fused': lambda: [store.corrupt(s, name, severity, seed=1, out=out) for s in sels]}
                    if name == 'jpeg':
                        arms['recipe'] = lambda: host_jpeg(store, sels[0], int(p), pool)
                    else:
                        arms['recipe'] = lambda: [recipe(store, s, name, p, 1) for s in sels]
                    times = time_arms(arms, a.repeats, a.min_seconds, a.warmup)
                    med = {k: stats(v, 1e6 / per_repeat[k])['median'] for k, v in times.items()}
                    floor_us = (B * 3 * 224 * 224 * (1 + 4)) / HBM_COPY_BYTES_PER_S * 1e6
                    for arm, v in times.items():
                        s = stats(v, 1e6 / per_repeat[arm])
                        rec = {'case': 'batch', 'corruption': name, 'severity': severity, 'param': p, 'batch': B, 'images': a.images, 'arm': arm,
                               'recipe': ('PIL on the host, 16 threads' if name == 'jpeg' else 'torch on the device') if arm == 'recipe' else None,
                               'batches_per_repeat': per_repeat[arm], 'median_us_per_batch': round(s['median'], 2),
                               'min_us_per_batch': round(s['min'], 2), 'max_us_per_batch': round(s['max'], 2), 'repeats': s['repeats'],
                               'device': torch.cuda.get_device_name(0)}
                        if arm == 'fused':
                            rec['traffic_floor_us'] = round(floor_us, 2)
                            rec['fused_over_floor'] = round(med['fused'] / floor_us, 2)
                            rec['recipe_over_fused'] = round(med['recipe'] / med['fused'], 2)
                        print(json.dumps(rec), flush=True)
                        lines.append(rec)


def kernels_only(a, dev):
    store = make_store(a.images, dev)
    order = torch.randperm(a.images, generator=torch.Generator().manual_seed(1)).to(dev)
    B = BATCHES[0]
    out = torch.empty(B, 3, 224, 224, device=dev)
    for name, _ in KERNEL_CASES:
        for k in range(KERNEL_RUNS):
            lo = (k * B) % (a.images - B + 1)
            store.corrupt(order[lo:lo + B], name, 5, seed=1, out=out)
        torch.cuda.synchronize()
    print('kernels-only run done:', KERNEL_RUNS, 'launches at severity 5, batch', B, 'of', [n for n, _ in KERNEL_CASES])


def kernel_trace(path, images, out):
    with open(path) as f:
        rows = list(csv.DictReader(f))
    B = BATCHES[0]
    floor_us = (B * 3 * 224 * 224 * 5) / HBM_COPY_BYTES_PER_S * 1e6
    with open(out, 'a') as o:
        for name, kernel in KERNEL_CASES:
            us = sorted((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows if kernel in r['Kernel_Name'])
            if len(us) != KERNEL_RUNS:
                raise SystemExit(f'{path}: {len(us)} {kernel} dispatches, expected {KERNEL_RUNS}')
            rec = {'case': 'kernel', 'kernel': kernel, 'corruption': name, 'severity': 5, 'batch': B, 'images': images, 'calls': len(us),
                   'median_us': round(us[len(us) // 2], 2), 'min_us': round(us[0], 2), 'max_us': round(us[-1], 2),
                   'traffic_floor_us': round(floor_us, 2), 'median_over_floor': round(us[len(us) // 2] / floor_us, 2)}
            print(json.dumps(rec))
            o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8192)
    ap.add_argument('--batches', type=int, default=8, help='consecutive batches per timed repeat')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--min-seconds', type=float, default=0.2)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--only', default='', help='comma-separated corruption names (default: all)')
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--kernel-trace', metavar='CSV')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'corrupt_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.kernel_trace:
        return kernel_trace(a.kernel_trace, a.images, a.out)
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_corrupt.py measures on the GPU; no device found')
    dev = torch.device('cuda:0')
    if a.kernels_only:
        return kernels_only(a, dev)
    lines = []
    per_batch(a, dev, lines)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
