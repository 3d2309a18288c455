"""The measurements behind profiles/optim_rows_error.jsonl.

  errors OUT_DIR   (GPU) every case group of tests/test_gpu_optim_rows.py through the exported entries, nothing asserted about the ratios: per
                   group and tensor the largest |gpu - R| / bound (the bound with its SAFETY factor) and where it occurred, and the body /
                   tail / rovit_adamw_flat agreement record -> OUT_DIR/optim_rows_errors.json.  A protocol failure (a sentinel, an input, a
                   second call, a ticket, the plain against the EMA kernel) is recorded under `errors`.  The library is the one
                   rovit_hip.native loads (ROVIT_HIP_LIB selects another build).
  record DIR       (no GPU) DIR/optim_rows_errors.json -> profiles/optim_rows_error.jsonl, one line per case group.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'rovit-kan-interpretable-vision-transformer-for-rose-disease-severity-estimation_amd')
for p in (ROOT, PKG, os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import optim_cases as oc


def errors(out_dir):
    import test_gpu_optim_rows as G
    res = {}

    def group(key, sweeps):
        rec = {}
        for label, fn in sweeps:
            try:
                rep = fn()
            except AssertionError as e:
                rec.setdefault('errors', []).append(f'{label}: {str(e)[:160]}')
                continue
            for n, (v, where) in rep.items():
                if n not in rec or not v <= rec[n]['ratio']:
                    rec[n] = {'ratio': float(f'{v:.4g}'), 'where': where}
        res[key] = rec
        print(key, json.dumps(rec), flush=True)

    group('rovit_sq_norm_clip, rovit_clip_coef | one buffer of 4, 16 380, 16 384, 16 388 floats; 2, 3, 4 buffers; a zero-count buffer first, in the '
          'middle, last; dense +-1 fills and sparse power-of-two probes', [('', lambda: G.sweep_clip(oc.clip_small_cases()))])
    group('rovit_sq_norm_clip, rovit_clip_coef | norm = max_norm and one fp32 either side, 0, overflow, NaN, random sums',
          [('', lambda: G.sweep_clip(oc.clip_coef_cases()))])
    for P in oc.PIECE_TOTALS:
        group(f'rovit_sq_norm_clip | {P} pieces, probes in the first and last float4 of the first and last piece of four blocks',
              [('', lambda P=P: G.sweep_clip([c for c in oc.clip_piece_cases() if c.name.startswith(f'pieces{P}_')]))])
    group('rovit_sq_norm_accum | n 1, 3, 4, 5, 1023, 1024, 1025, 512 x 1024 - 4, + 0, + 5, three buffers; with scratch (sq) and without (sq_atomic)',
          [('', lambda: G.sweep_accum(oc.accum_cases()))])
    for n in oc.SINGLE_N:
        group(f'adamw, three entries | one segment of {n} floats, {oc.K} recipes x {oc.K} shifts, t and coef cycling',
              [('', lambda n=n: G.sweep_adam(oc.adam_single_cases(n)))])
    group(f'adamw, three entries | {2 * oc.ADAM_PIECE + 3} floats, t 1, 2, 10, 1 000 000 x coef NULL, 1, 0.5, 0',
          [('', lambda: G.sweep_adam(oc.adam_product_cases()))])
    for sizes in oc.MULTI_SIZES:
        group(f'rovit_adamw_flat_multi, rovit_adamw_ema_flat_multi | segments of {sizes} floats, own lr and t',
              [('', lambda s=sizes: G.sweep_adam(oc.adam_multi_cases(s), ('multi', 'ema')))])
    group(f'rovit_adamw_flat | {oc.FLAT_LARGE_N} floats: above the block cap, with a tail',
          [(str(s), lambda s=s: G.sweep_adam(oc.adam_flat_large_cases([s]), ('flat',))) for s in range(oc.K)])
    group('rovit_adamw_flat_multi, rovit_adamw_ema_flat_multi | eight steps, a coefficient of its own each, every step judged alone',
          [('', lambda: G.sweep_adam([oc.adam_steps_case()], ('multi', 'ema')))])
    res['agreement | the same element values in a body slot and in a tail slot, through the three entries (bit for bit on p, m, v)'] = G.body_tail_record()
    json.dump({'safety': oc.SAFETY, 'groups': res}, open(os.path.join(out_dir, 'optim_rows_errors.json'), 'w'), indent=1)


def record(src):
    run = json.load(open(os.path.join(src, 'optim_rows_errors.json')))
    with open(os.path.join(ROOT, 'profiles', 'optim_rows_error.jsonl'), 'w') as f:
        for key, rec in run['groups'].items():
            head = {'case': key, 'tool': 'tools/optim_rows_error.py errors'}
            if not key.startswith('agreement'):
                head.update(safety=run['safety'], unit='largest |gpu - R| / (safety x bound) per tensor (0: bit for bit; inf: a required value missed)')
            f.write(json.dumps({**head, **rec}) + '\n')


if __name__ == '__main__':
    if sys.argv[1] == 'record':
        record(sys.argv[2])
    else:
        os.makedirs(sys.argv[2], exist_ok=True)
        errors(sys.argv[2])
