"""Time the deletion / insertion curves at one or more batch sizes and append one JSON line per (batch, mode) to
profiles/perturbation_time.jsonl.  steps and both modes (deletion, insertion) for every entry; target 'class'.

  replace        : m.perturbation_curves(x, map) -- one map, perturbation='replace' (zero baseline)
  drop           : the same with perturbation='drop'
  replace_5maps  : one call with a dict of five maps (rollout, Grad-CAM++, attention relevance, |input gradient|, integrated gradients;
                   computed once before timing, not timed)
  pixel_recipe   : the explicit recipe: torch-built perturbed images (torch.where on the patch mask), rovit_vit_forward and the heads
                   per chunk of 256 images, every step of both curves (endpoints included, as a caller of the pixel recipe runs them)
  forward        : the plain inference forward m(x) of the B images (bf16 engine and heads, no grad)

Device-event times; --warmup calls of every mode first, then --repeats rounds in which the modes run interleaved, one call each per
round; the median and min per mode are reported, with the sequences (backbone rows of 197 or fewer tokens) each call runs and the
median per sequence (the protocol of tools/time_relevance.py).  The gather kernel alone:
rocprofv3 --kernel-trace --stats -- python tools/time_perturbation.py --batch 256 --modes replace --repeats 3 --out <scratch file>
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)

MODES = ['replace', 'drop', 'replace_5maps', 'pixel_recipe', 'forward']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, nargs='+', default=[16, 256])
    ap.add_argument('--steps', type=int, default=28)
    ap.add_argument('--modes', nargs='+', default=MODES, choices=MODES)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'perturbation_time.jsonl'))
    a = ap.parse_args()
    from oracle import ref_cpu
    from models.rovit_kan import RoViTKAN
    from rovit_hip.input_grad import _Backbone, _head_outputs
    from rovit_hip.native import MLP_ONE_LAUNCH, call, ptr, stream_ptr
    from rovit_hip.perturbation import _ranks, patch_order, perturbed_mask
    dev = torch.device('cuda:0')
    sd = ref_cpu.init_rovit_state(seed=0)
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    steps = a.steps
    ks = [196 * s // steps for s in range(steps + 1)]

    def pixel_recipe(x, sal, chunk=256):
        """(2, B, steps+1) class probabilities of every step of both curves from perturbed pixel images."""
        B = x.shape[0]
        bb = _Backbone(m, dev)
        rank = _ranks(patch_order(sal))
        xb = torch.zeros(1, 3, 224, 224, device=dev)
        ws = bb.eng.take_ws(chunk, False, dev)
        out = torch.empty(2 * (steps + 1) * B, device=dev)
        total = out.numel()
        cls = None
        for j0 in range(0, total, chunk):
            j = torch.arange(j0, min(total, j0 + chunk), device=dev)
            mode, s, b = j // ((steps + 1) * B), (j // B) % (steps + 1), j % B
            k = torch.tensor(ks, device=dev)[s]
            mask = perturbed_mask(rank[b], mode == 0, k)
            n = j.numel()
            imgs = torch.where(mask.view(n, 1, 14, 1, 14, 1).expand(n, 3, 14, 16, 14, 16).reshape(n, 3, 224, 224), xb, x[b]).contiguous()
            f = torch.empty(n, 192, device=dev)
            call('rovit_vit_forward', ptr(imgs), bb.pa, ptr(bb.eng.prep), ptr(ws), ptr(f), n, bb.vit.depth, 0, MLP_ONE_LAUNCH, stream_ptr())
            logits = _head_outputs(m, f)[0]
            if cls is None:                                        # step 0 of the deletion curve: the unperturbed images
                cls = logits[:B].argmax(1)
            out[j] = torch.softmax(logits, 1).gather(1, cls[b].view(-1, 1))[:, 0]
        bb.eng.give_ws(chunk, False, ws)
        return out.view(2, steps + 1, B).transpose(1, 2)

    lines = []
    for B in a.batch:
        x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B)).to(dev)
        maps = {'rollout': m.attention_rollout(x), 'gradcam_pp': m.grad_cam_pp(x), 'relevance': m.attention_relevance(x),
                'input_grad_abs': m.input_gradients(x).abs(), 'integrated_grad': m.input_gradients(x, steps=16)}
        sal = maps['relevance']
        n_seq = {'replace': B * (2 + 2 * (steps - 1)), 'drop': B * (2 + 2 * (steps - 1)), 'replace_5maps': B * (2 + 10 * (steps - 1)),
                 'pixel_recipe': B * 2 * (steps + 1), 'forward': B}
        fns = {'replace': lambda: m.perturbation_curves(x, sal, steps=steps),
               'drop': lambda: m.perturbation_curves(x, sal, steps=steps, perturbation='drop'),
               'replace_5maps': lambda: m.perturbation_curves(x, maps, steps=steps),
               'pixel_recipe': lambda: pixel_recipe(x, sal),
               'forward': lambda: m(x)}
        modes = {k: fns[k] for k in a.modes}
        with torch.no_grad():
            # the two recipes agree on what they share: the deletion curve of the one map
            if 'replace' in modes and 'pixel_recipe' in modes:
                r, p = fns['replace'](), pixel_recipe(x, sal)
                same = bool(torch.equal(r['deletion'], p[0]) and torch.equal(r['insertion'], p[1]))
                print(f'batch {B}: fused curves bit-identical to the pixel recipe: {same}', flush=True)
            for _ in range(a.warmup):
                for fn in modes.values():
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in modes}
            for _ in range(a.repeats):
                for name, fn in modes.items():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    fn()
                    e.record()
                    e.synchronize()
                    times[name].append(s.elapsed_time(e))
        for name in modes:
            t = sorted(times[name])
            med = t[len(t) // 2]
            rec = {'mode': name, 'batch': B, 'steps': steps, 'sequences': n_seq[name], 'median_ms': round(med, 3), 'min_ms': round(t[0], 3),
                   'us_per_sequence': round(1000 * med / n_seq[name], 3), 'repeats': a.repeats, 'device': torch.cuda.get_device_name(0)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
