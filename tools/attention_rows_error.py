"""The measurements behind profiles/attention_rows_error.jsonl.

  errors TAG OUT_DIR    (GPU) every case of tests/test_gpu_attention_rows.py through the exported entries, nothing asserted: per kernel family,
                        generator and tensor the largest |gpu - R| / bound over all token counts, with the T and the (image, head, row) where
                        it occurred -> OUT_DIR/attention_rows_errors_TAG.json.  The library is the one rovit_hip.native loads (ROVIT_HIP_LIB
                        selects another build, such as one of the parent commit); `scale` lines record what each entry does at 1/16, 1/4 and
                        0.1: the ratios, or that it refused.
  record DIR            (no GPU) merges DIR/attention_rows_errors_*.json with the CPU mutation table of tests/attention_cases.py (fault x
                        {caught by the new bounds, passed the old max-norm criteria}) and, if DIR/bench_ab.txt is there (``== parent 1`` /
                        ``== fixed 1`` ... each followed by the JSON line of a ``bench.py --gpus 1 --steps 40 --warmup 10`` run on that
                        build), with the step times -> profiles/attention_rows_error.jsonl
"""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'rovit-kan-interpretable-vision-transformer-for-rose-disease-severity-estimation_amd')
for p in (ROOT, PKG, os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import attention_cases as ac


def _note(rec, rep, T):
    for n, (v, where) in rep.items():
        if n not in rec or not v <= rec[n]['ratio']:
            rec[n] = {'ratio': float(f'{v:.4g}'), 'T': T, 'image_head_row': list(where)}


def errors(tag, out_dir):
    import test_gpu_attention_rows as G
    res = {}

    def sweep(key, cases, cls):
        rec = res.setdefault(key, {})
        for case in cases:
            R = ac.truth(case, cls=cls)
            got, _ = G.run(case, cls=cls)
            _note(rec, ac.compare(got, R, ac.bounds(case, R, cls=cls), rows=slice(0, 1) if cls else None), case.T)
        print(tag, key, json.dumps(rec), flush=True)

    sweep('dense | random | T 1..208, B 2, H 3', (ac.random(2, T, 3, seed=1) for T in ac.ALL_T), False)
    for gen in ('peaked', 'selector', 'pair_selector', 'uniform'):
        sweep(f'dense | {gen} | edge T, B 1, H 2', (ac.make(gen, T, H=2, B=1, seed=4) for T in ac.EDGE_T), False)
    sweep('class token | random | T 1..224, B 2, H 3', (ac.random(2, T, 3, seed=3) for T in ac.CLS_T), True)
    for gen in ('peaked', 'selector', 'pair_selector', 'uniform'):
        sweep(f'class token | {gen} | edge T and 209, 223, 224, B 1, H 2', (ac.make(gen, T, H=2, B=1, seed=4) for T in ac.EDGE_T + [209, 223, 224]), True)
    for scale in G.SCALES:
        for cls in (False, True):
            rec, refused = {}, []
            for T in (33, 197):
                case = ac.random(2, T, 3, seed=5, scale=scale)
                R = ac.truth(case, cls=cls)
                got, _ = G.run(case, cls=cls, refusals=refused)
                _note(rec, ac.compare(got, R, ac.bounds(case, R, cls=cls), rows=slice(0, 1) if cls else None), T)
            for name in set(refused):
                for n in (('out', 'lse2') if name.endswith('_fwd') else ('dq', 'dk', 'dv')):
                    rec[n] = 'refused'
            res[f'scale {scale} | ' + ('class token' if cls else 'dense') + ' | random | T 33, 197'] = rec
            print(tag, 'scale', scale, cls, json.dumps(rec), flush=True)
    json.dump(res, open(os.path.join(out_dir, f'attention_rows_errors_{tag}.json'), 'w'), indent=1)


def record(src):
    lines = []
    for path in sorted(glob.glob(os.path.join(src, 'attention_rows_errors_*.json'))):
        tag = os.path.basename(path)[len('attention_rows_errors_'):-len('.json')]
        for key, rec in json.load(open(path)).items():
            lines.append({'build': tag, 'case': key, 'tool': 'tools/attention_rows_error.py errors',
                          'unit': 'largest |gpu - R| / bound per tensor over the token counts (inf: a value that is not finite)', **rec})
    table = ac.mutation_table()
    for fault, rec in table.items():
        lines.append({'fault': fault, 'tool': 'tools/attention_rows_error.py record (CPU: E of tests/attention_cases.py with the fault injected)',
                      'caught_by_new_bounds_in': {str(T): g for T, g in rec['caught'].items()},
                      'caught_at_every_T': all(rec['caught'].values()),
                      'passed_old_max_norm_criteria_where_caught': [list(x) for x in rec['slipped']]})
    bench = os.path.join(src, 'bench_ab.txt')
    if os.path.exists(bench):
        import re
        runs = {w: [json.loads(x) for x in re.findall(r'== %s \d+\n(\{.*\})' % w, open(bench).read())] for w in ('parent', 'fixed')}
        lines.append({'what': 'bench.py --gpus 1 --steps 40 --warmup 10 on an MI355X, a build of the parent commit and this one alternating in one session',
                      'ms_per_step': {w: [x['ms_per_step'] for x in v] for w, v in runs.items()},
                      'final_loss': {w: sorted({x.get('final_loss') for x in v}, key=str) for w, v in runs.items()},
                      'note': 'only entry checks were added on the host side of the attention launches; the kernels are unchanged'})
    with open(os.path.join(ROOT, 'profiles', 'attention_rows_error.jsonl'), 'w') as f:
        f.write(''.join(json.dumps(x) + '\n' for x in lines))


if __name__ == '__main__':
    if sys.argv[1] == 'record':
        record(sys.argv[2])
    else:
        os.makedirs(sys.argv[3], exist_ok=True)
        errors(sys.argv[2], sys.argv[3])
