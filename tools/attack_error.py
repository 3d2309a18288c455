"""Measure what the attack tests bound and append it to profiles/attack_error.jsonl: the worst error of the L2 step and start kernels
against ``step_reference`` / ``init_reference`` in fp64 over the cases of tests/attack_cases.py, in units of 2^-24 max(r, |reference|)
(the tests' tolerance is 8 of them), and the per-image cosine and relative error of ``objective_gradient`` against fp64 autograd through
the oracle on the depth-2 model (the figures tests/test_gpu_attack.py prints)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'attack_error.jsonl'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/attack_error.py measures on the GPU; no device found')
    import attack_cases as ac
    import test_gpu_attack as tg
    import test_gpu_input_grad as tig
    from rovit_hip import attack as A
    lines = []
    unit = 2.0 ** -24
    for clip in ((0., 1.), None):
        worst = {'step': 0.0, 'start': 0.0}
        for shape in ac.SHAPES:
            for B in ac.BATCHES:
                case = ac.build(shape, B, clip, dead_image=True)
                want, _ = A.step_reference(case['x'], case['g'], case['delta_l2'], case['eps'], case['alpha'], 'l2', ac.MEAN, ac.STD, clip, np.float64)
                got, _, _ = tg._run_step(case, 'l2', shape)
                scale = unit * np.maximum(case['r'].astype(np.float64), np.abs(want)) + ac.DENORMAL_STEP
                worst['step'] = max(worst['step'], float((np.abs(got - want) / scale).max()))
                ids = np.arange(B) + 11
                want, _ = A.init_reference(case['x'], ids, case['eps'], 'l2', 5, 0, ac.MEAN, ac.STD, clip, np.float64)
                got, _ = tg._run_init(case['x'], ids, case['eps'], 'l2', shape, clip, 5, 0)
                scale = unit * np.maximum(case['r'].astype(np.float64), np.abs(want)) + ac.DENORMAL_STEP
                worst['start'] = max(worst['start'], float((np.abs(got - want) / scale).max()))
        for kernel, v in worst.items():
            lines.append({'case': 'l2_' + kernel, 'clip': 'box' if clip else 'none', 'worst_error_in_2^-24_max(r,|ref|)': round(v, 3),
                          'tolerance': 8, 'shapes': len(ac.SHAPES), 'batches': ac.BATCHES})
    for B in (1, 5):
        m, sd = tig._model(2, seed=30 + B)
        sd64 = tig._sd64(sd)
        x = tg._box_images(B, 31 + B)
        y = torch.randint(0, 4, (B,), generator=torch.Generator().manual_seed(5))
        for objective, direction in (('ce', 1), ('margin', 1), ('mu', 1), ('mu', -1), ('kan_severity', 1)):
            is_class = objective in A.CLASS_OBJECTIVES
            _, grad = A.objective_gradient(m, x.to(tg.dev()), y.to(tg.dev()) if is_class else None, objective, None, direction)
            f_hip = m(x.to(tg.dev()).requires_grad_(True))['features'].detach().cpu()
            value_fn = lambda out: tg._oracle_value(out, objective, y, direction)
            want, _ = tig._oracle_image_grad(x, sd64, lambda f: tig._head_seed(sd64, f_hip, value_fn))
            cos = [tig._cos(grad[b].cpu(), want[b]) for b in range(B)]
            rel = [float((grad[b].double().cpu() - want[b]).abs().max() / want[b].abs().max()) for b in range(B)]
            lines.append({'case': 'objective_gradient', 'objective': objective, 'direction': direction, 'batch': B, 'depth': 2,
                          'min_cosine': round(min(cos), 6), 'max_rel_error': float(f'{max(rel):.3e}'), 'cos_min_bound': tig.COS_MIN,
                          'rel_max_bound': tig.REL_MAX})
    for rec in lines:
        rec['device'] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
