"""The measurements behind profiles/kan_rows_error.jsonl.

  errors TAG OUT_DIR [TAU EPS_EXP]   (GPU) every case group of tests/test_gpu_kan_rows.py through the exported entries, nothing asserted: per group
                        and tensor the largest |gpu - R| / bound and where it occurred (case, then row and element) and the hidden rows
                        skipped -> OUT_DIR/kan_rows_errors_TAG.json.  TAU (ulps of tanhf) and EPS_EXP (relative error of __expf, as a power
                        of two: -21 for 2^-21) replace the constants of tests/kan_cases.py for this run: that is how the committed values
                        were chosen.  The library is the one rovit_hip.native loads (ROVIT_HIP_LIB selects another build).
  record DIR            (no GPU) merges DIR/kan_rows_errors_*.json -> profiles/kan_rows_error.jsonl: one line per case group of the run made
                        with the committed constants (TAG `committed`), and one line with the largest ratio per tensor family for every
                        other pair of constants tried.
"""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'rovit-kan-interpretable-vision-transformer-for-rose-disease-severity-estimation_amd')
for p in (ROOT, PKG, os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import kan_cases as kc


def errors(tag, out_dir, tau=None, eps=None):
    if tau is not None:
        kc.TAU, kc.EPS_EXP = float(tau), 2.0 ** float(eps)
    import test_gpu_kan_rows as G
    G.PROBES = {p.name: p for p in kc.all_probes()}          # the either-side classification follows TAU
    res = {}

    def group(key, sweeps):
        rec, skipped, rows = {}, 0, 0
        for label, fn in sweeps:
            try:
                rep = fn()
            except AssertionError as e:
                rec.setdefault('errors', []).append(f'{label}: {str(e)[:120]}')
                continue
            skipped, rows = skipped + rep.skipped, rows + rep.rows
            for n, (v, where) in rep.items():
                n = ''.join(c for c in n if not c.isdigit()) if n[-1].isdigit() else n         # y0, y1 .. -> y: one figure a group
                if n.startswith('gz') and ' all ' in where + ' ':
                    n = 'gz + grad_outs'
                if n not in rec or not v <= rec[n]['ratio']:
                    rec[n] = {'ratio': float(f'{v:.4g}'), 'where': where}
        rec['hidden_rows_skipped'], rec['hidden_rows'] = skipped, rows
        res[key] = rec
        print(tag, key, json.dumps(rec), flush=True)

    uni = [n for n in G.PROBES if n not in G.NONUNIFORM]
    group('rovit_kan_basis | knot_probe | linspace(-1, 1, nk) for nk 8..64, a uniform grid with knots[nb] == 0; n 1, 255, 256, 257',
          [(n, lambda n=n: G.sweep_basis(n)) for n in uni])
    for n in G.NONUNIFORM:
        group(f'rovit_kan_basis | knot_probe | non-uniform: {n}', [(n, lambda n=n: G.sweep_basis(n))])
    for (i, o, k) in G.LAYERS:
        group(f'rovit_kan_layer_fwd / _bwd | probe rows, B 1, tb, tb + 1, all | {i} -> {o}, {k} knots, three activations',
              [(f'act {a}', lambda a=a: G.sweep_layer(i, o, k, a)) for a in kc.ACTS])
    for (i, o, k) in [(192, 64, 64), (7, 65, 38)]:
        bc = kc.dw_bc(o, k)
        group(f'rovit_kan_layer_bwd parameter gradients | random | {i} -> {o}, {k} knots, B 1, 2, bc - 1, bc, bc + 1, 2 bc + 1 (bc = {bc})',
              [('', lambda: G.sweep_dw_chunks(i, o, k, [1, 2, bc - 1, bc, bc + 1, 2 * bc + 1]))])
    group('rovit_kan_layer_bwd parameter gradients | random | 8 -> 1, 8 knots, B 3 (empty sample slices)',
          [(f'act {a}', lambda a=a: G.sweep_dw_chunks(8, 1, 8, [3], a)) for a in kc.ACTS])
    group('rovit_kan_layer_fwd / _bwd | selector | 8, 11, 38, 64 knots', [('', G.sweep_selector)])
    mf = ['default11', '8-40-8-4', '8-40-8-4 nk9', 'default38', 'zero_cut_guess']
    for n in G.STACKS:
        group(f'rovit_kan_stack_fwd | probe, random, relu_zeros rows, B 1, 15, 16, 17, all | {n} {G.STACKS[n][0]}', [(n, lambda n=n: G.sweep_stack_fwd(n))])
    group('rovit_kan_stack_fwd | B 4096, 4097 | default11', [(str(b), lambda b=b: G.sweep_stack_fwd_large('default11', b)) for b in (4096, 4097)])
    for n in mf:
        group(f'rovit_kan_stack_fwd_mfma | probe, random, relu_zeros rows, B 1, 31, 32, 33, 65, all | {n}',
              [(n, lambda n=n: G.sweep_stack_fwd(n, mfma=True, batches=(1, 31, 32, 33, 65)))])
    group('rovit_kan_stack_fwd_mfma | B 49152, 49153 | default38',
          [(str(b), lambda b=b: G.sweep_stack_fwd_large('default38', b, mfma=True)) for b in (49152, 49153)])
    for n in G.STACKS:
        group(f'rovit_kan_stack_bwd | B 33, grad_outs all / last, dx NULL, d_spline_w NULL | {n}',
              [(v, lambda v=v, n=n: G.sweep_stack_bwd(n, 33, v)) for v in ('last', 'all', 'no_dx', 'no_dw')])
    group('rovit_kan_stack_bwd | B 1, 1024, 1025, 4096, 4097, edge rows | default11',
          [(str(b), lambda b=b: G.sweep_stack_bwd('default11', b, 'last', edge=True)) for b in (1, 1024, 1025, 4096, 4097)])
    group('rovit_kan_stack_bwd | B 393 = 2 bc + 1 | default64', [('', lambda: G.sweep_stack_bwd('default64', 393, 'all'))])
    json.dump({'tau': kc.TAU, 'eps_exp': kc.EPS_EXP, 'groups': res}, open(os.path.join(out_dir, f'kan_rows_errors_{tag}.json'), 'w'), indent=1)


def _largest(groups):
    out = {}
    for rec in groups.values():
        for n, v in rec.items():
            if isinstance(v, dict) and (n not in out or v['ratio'] > out[n]):
                out[n] = v['ratio']
    return out


def record(src):
    lines = []
    for path in sorted(glob.glob(os.path.join(src, 'kan_rows_errors_*.json'))):
        tag = os.path.basename(path)[len('kan_rows_errors_'):-len('.json')]
        run = json.load(open(path))
        if tag == 'committed':
            for key, rec in run['groups'].items():
                lines.append({'case': key, 'tool': 'tools/kan_rows_error.py errors', 'tau': run['tau'], 'eps_exp': run['eps_exp'],
                              'unit': 'largest |gpu - R| / bound per tensor (inf: a value that is not finite)', **rec})
        big = _largest(run['groups'])
        lines.append({'constants': tag, 'tau': run['tau'], 'eps_exp': run['eps_exp'], 'largest_ratio_per_tensor': big,
                      'largest_that_depends_on_the_constants': max(v for n, v in big.items() if n not in ('dx+', 'gz + grad_outs', 'gz')),
                      'note': 'dx+ (the accumulating dx) and gz + grad_outs (dL/dz of a layer that also gets an outside gradient) are one fp32 '
                              'addition against its exact half-ulp bound: up to 1 by construction, whatever the constants; the largest gz is that of a SIGMOID3 output near y = 3: the '
                              'rounding of y * fl(1/3) left over by the cancellation in 1 - y / 3 against twice its half-ulp bound; it moves by 0.005 '
                              'between EPS_EXP 2^-21 and 2^-24 and not at all with TAU, so it is left out of the figure the constants were chosen by'})
    with open(os.path.join(ROOT, 'profiles', 'kan_rows_error.jsonl'), 'w') as f:
        f.write(''.join(json.dumps(x) + '\n' for x in lines))


if __name__ == '__main__':
    if sys.argv[1] == 'record':
        record(sys.argv[2])
    else:
        os.makedirs(sys.argv[3], exist_ok=True)
        errors(sys.argv[2], sys.argv[3], *sys.argv[4:6])
