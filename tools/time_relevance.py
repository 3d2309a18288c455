"""Time the gradient-weighted attention relevance at one or more batch sizes and append one JSON line per (batch, mode, target) to
profiles/relevance_time.jsonl.

  attention_relevance : m.attention_relevance(x, target) (upsampled map; eval semantics, own workspace)
  input_gradients     : m.input_gradients(x, target) of the same target, in the same process
  torch_recipe        : the fp32 oracle backbone on the GPU (oracle.ref_cpu.vit_forward with attn_probs), the heads, autograd.grad to
                        the attention probabilities and the forward-order matrix recursion (rovit_hip.relevance.relevance_reference)

Device-event times; --warmup calls of every mode first, then --repeats rounds in which the modes run interleaved, one call each per
round; the median and min per mode are reported (the protocol of tools/time_input_grad.py).  The step kernel alone:
rocprofv3 --kernel-trace --stats -- python tools/time_relevance.py --batch 256 --repeats 3 --out <scratch file>
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
    ap.add_argument('--targets', nargs='+', default=['class', 'kan_severity'])
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--recipe-max-batch', type=int, default=64, help='largest batch the torch recipe is timed at (its memory grows fast)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'relevance_time.jsonl'))
    a = ap.parse_args()
    from oracle import ref_cpu
    from models.rovit_kan import RoViTKAN
    from rovit_hip.relevance import relevance_reference
    dev = torch.device('cuda:0')
    sd = ref_cpu.init_rovit_state(seed=0)
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    sdg = {k: v.to(dev) for k, v in sd.items()}

    def recipe(x, target):
        xg = x.clone().requires_grad_(True)
        probs = []
        feats = ref_cpu.vit_forward(xg, sdg, prefix='backbone.model.', attn_probs=probs)
        if target == 'class':
            out = ref_cpu.heads_forward(feats, sdg, 4)['cls_logits']
            value = out.gather(1, out.detach().argmax(1, keepdim=True))[:, 0]
        else:
            value = ref_cpu.kan_module_forward(feats, sdg, 'kan_module.')[:, 0]
        return relevance_reference(probs, value)

    lines = []
    for B in a.batch:
        x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B)).to(dev)
        for target in a.targets:
            modes = {'attention_relevance': lambda x: m.attention_relevance(x, target=target),
                     'input_gradients': lambda x: m.input_gradients(x, target=target)}
            if B <= a.recipe_max_batch:
                modes['torch_recipe'] = lambda x: recipe(x, target)
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
                rec = {'mode': name, 'target': target, 'batch': B, 'median_ms': round(t[len(t) // 2], 3), 'min_ms': round(t[0], 3),
                       'ms_per_image': round(t[len(t) // 2] / B, 4), 'repeats': a.repeats, 'device': torch.cuda.get_device_name(0)}
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
