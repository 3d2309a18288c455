"""A/B of the training step between builds of the library (the backward with rovit_block_bwd_fused against the parent commit's), and
append JSON lines to profiles/block_bwd_time.jsonl.

    python tools/time_block_bwd.py parent=/path/to/parent/librovit_hip.so stage1=/path/to/this/librovit_hip.so [NAME=LIB ...]

An arm may also be NAME=LIB@ID=VALUE,ID=VALUE: LIB is then the developer library (make -C csrc dev) and the child runs with those knobs
(common.h RovitKnob ids, through ROVIT_DEV_KNOBS) -- several schedules of one build against each other.

One process tree on one box: this process starts ONE child per arm (``--child``, ROVIT_HIP_LIB = that arm's library), every child builds
bench.py's workload -- full RoViT-KAN, batch 256, curriculum stage 4, one resident randn batch, step = forward + JointLoss + zero_grad +
backward + GradSync.finish + RoViTAdamW.step -- and warms it, then waits.  The parent hands out the repeats one at a time, arm after
arm: one untimed round, then --repeats rounds (default 7) of --steps steps (default 20).  Only one child runs at any moment and all of
them stay resident, so the arms see the same box, clocks and neighbours.  A repeat is the host clock between two device
synchronisations inside the child.

Per arm: median, min, max and spread of the ms per step; then a ``step_condition`` line per arm that is not the first: the arm may ship as
the product path only if its SLOWEST repeat is faster than the FASTEST repeat of the first arm (the parent)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v):
    s = sorted(v)
    return s[len(s) // 2], s[0], s[-1]


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__  # noqa: F401  (puts the package on sys.path)
    import ctypes
    from rovit_hip import native
    # a build of an older commit does not export the entry points added since; the step calls none of them from Python
    probe = ctypes.CDLL(native.LIB_PATH)
    for name in [n for n in native.SIGNATURES if not hasattr(probe, n)]:
        del native.SIGNATURES[name]
    from models.rovit_kan import RoViTKAN
    from rovit_hip.losses import JointLoss
    from rovit_hip.optim import RoViTAdamW
    from rovit_hip.parallel import GradSync
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    model = RoViTKAN(pretrained=False).to(dev).train()
    model.curriculum_stage = 4
    opt = RoViTAdamW(model, lr=1e-4, weight_decay=1e-4, max_grad_norm=1.0)
    loss_fn = JointLoss(1.0, 0.5, 0.5, 2.0, torch.ones(4, device=dev))
    sync = GradSync(model, buckets=2, optimizer=opt)
    g = torch.Generator(device=dev).manual_seed(1000)
    images = torch.randn(a.batch, 3, 224, 224, device=dev, generator=g)
    labels = torch.randint(0, 4, (a.batch,), device=dev, generator=g)

    def step():
        out = model(images)
        loss = loss_fn(out, labels, labels, 4)['total_loss']
        opt.zero_grad(set_to_none=True)
        loss.backward()
        sync.finish()
        opt.step()
        return loss

    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    print(json.dumps({'ready': torch.cuda.get_device_name(0)}), flush=True)
    for line in sys.stdin:
        if line.strip() != 'go':
            break
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = step()
        torch.cuda.synchronize()
        print(json.dumps({'s_per_step': (time.perf_counter() - t0) / a.steps, 'loss': float(loss.detach())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('arms', nargs='*', metavar='NAME=LIB', help='first arm = the parent build')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20, help='steps per timed repeat')
    ap.add_argument('--repeats', type=int, default=7, help='timed repeats per arm')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'block_bwd_time.jsonl'))
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    arms = [x.split('=', 1) for x in a.arms]
    knobs = {}
    for x in arms:
        if len(x) == 2 and '@' in x[1]:
            x[1], knobs[x[0]] = x[1].split('@', 1)
    if len(arms) < 2 or any(len(x) != 2 or not os.path.exists(x[1]) for x in arms):
        raise SystemExit('usage: time_block_bwd.py parent=LIB stage1=LIB [...]: at least two existing libraries, the parent first')
    procs = {}
    try:
        for name, lib in arms:          # one after the other: a child is warm and idle before the next one starts
            env = dict(os.environ, ROVIT_HIP_LIB=os.path.abspath(lib))
            if name in knobs:
                env['ROVIT_DEV_KNOBS'] = knobs[name]
            p = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--child', '--batch', str(a.batch), '--steps', str(a.steps)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
            procs[name] = p
            ready = p.stdout.readline()
            if not ready:
                raise SystemExit(f'arm {name}: the child ended before it was ready (exit {p.wait()})')
            device = json.loads(ready)['ready']
        times = {name: [] for name, _ in arms}
        loss = {}
        for rep in range(-1, a.repeats):       # round -1: one untimed repeat per arm (the children idled while the others warmed up)
            for name, _lib in arms:
                p = procs[name]
                p.stdin.write('go\n')
                p.stdin.flush()
                line = p.stdout.readline()
                if not line:
                    raise SystemExit(f'arm {name}: the child ended inside a repeat (exit {p.wait()})')
                rec = json.loads(line)
                if rep < 0:
                    continue
                times[name].append(rec['s_per_step'])
                loss[name] = rec['loss']
    finally:
        for p in procs.values():
            try:
                p.stdin.close()
            except OSError:
                pass
            p.wait()
    lines = []
    base = arms[0][0]
    med = {n: stats(v)[0] for n, v in times.items()}
    for name, lib in arms:
        m, lo, hi = stats(times[name])
        rec = {'case': 'step', 'arm': name, 'batch': a.batch, 'stage': 4, 'steps_per_repeat': a.steps, 'repeats': len(times[name]),
               'median_ms_per_step': round(m * 1e3, 4), 'min_ms_per_step': round(lo * 1e3, 4), 'max_ms_per_step': round(hi * 1e3, 4),
               'spread': round((hi - lo) / m, 4), 'final_loss': round(loss[name], 5), 'device': device}
        if name in knobs:
            rec['dev_knobs'] = knobs[name]
        if name != base:
            rec['median_minus_%s_us' % base] = round((med[name] - med[base]) * 1e6, 2)
        lines.append(rec)
    for name, _lib in arms[1:]:
        lines.append({'case': 'step_condition', 'arm': name, 'slowest_%s_ms' % name: round(max(times[name]) * 1e3, 4),
                      'fastest_%s_ms' % base: round(min(times[base]) * 1e3, 4),
                      'slowest_%s_is_faster_than_fastest_%s' % (name, base): max(times[name]) < min(times[base])})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as f:
        for rec in lines:
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
