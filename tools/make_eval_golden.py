"""Write tests/golden/eval_metrics.npz: seeded logits, labels and severities for three cases, and what the REFERENCE's
evaluation/metrics.py functions (sklearn / scipy inside) return on them.  Runs where a checkout of the reference exists; the tests read
the .npz only.  Data only: no reference source is copied.

  full      N = 257,  4 classes, all present
  absent    N = 4099, 4 classes, class 3 absent from labels and predictions; severities heavily tied
  constant  N = 64,   constant predicted severity (Spearman's rho is NaN)

The probabilities are torch-CPU fp32 softmax; the reference functions get fp64 COPIES of them (given fp32 arrays the reference's own
np.mean runs in fp32 and is 3.6e-8 (Brier) / 1.4e-9 (ECE) away from the fp64 value).  The fp32 probabilities are stored too, so the
tests do not depend on the last bit of another machine's softmax.

    python tools/make_eval_golden.py --reference DIR
"""
import argparse
import importlib.util
import os
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASS_NAMES = ['Healthy Leaf', 'Leaf Holes', 'Black Spot', 'Dry Leaf']


def case(name, n, seed):
    rng = np.random.default_rng(seed)
    C = 4
    labels = rng.integers(0, 3 if name == 'absent' else C, size=n)
    logits = rng.normal(size=(n, C)).astype(np.float32) * 2.0
    logits[np.arange(n), labels] += 1.5                    # better than chance, far from perfect
    if name == 'absent':
        logits[:, 3] = -30.0                               # never predicted
    sev_true = labels.astype(np.int64)                     # the reference's severity map is the class index
    if name == 'constant':
        sev_pred = np.full(n, 1.25, dtype=np.float32)
    else:
        sev_pred = np.clip(sev_true + rng.normal(size=n) * 0.8, 0, 3)
        sev_pred = (np.round(sev_pred, 1) if name == 'absent' else sev_pred).astype(np.float32)      # one decimal: many ties
    return logits, labels.astype(np.int64), sev_true, sev_pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference project')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'eval_metrics.npz'))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location('reference_metrics', os.path.join(a.reference, 'evaluation', 'metrics.py'))
    ref = importlib.util.module_from_spec(spec)            # by path: the package's own ``evaluation`` never comes into it
    spec.loader.exec_module(ref)
    from sklearn.metrics import f1_score
    out = {'cases': np.array(['full', 'absent', 'constant']), 'class_names': np.array(CLASS_NAMES)}
    for name, n, seed in (('full', 257, 11), ('absent', 4099, 12), ('constant', 64, 13)):
        logits, labels, sev_true, sev_pred = case(name, n, seed)
        probs32 = torch.softmax(torch.from_numpy(logits), dim=1).numpy()
        probs = probs32.astype(np.float64)
        pred = np.argmax(probs, axis=1)
        sp = sev_pred.astype(np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                # scipy's constant-input warning; sklearn's zero-division warning
            pc = ref.per_class_metrics(labels, pred, CLASS_NAMES)
            exp = {'accuracy': ref.accuracy(labels, pred), 'macro_f1': ref.macro_f1(labels, pred),
                   'weighted_f1': f1_score(labels, pred, average='weighted') * 100,         # as the reference's Evaluator calls it
                   'mae': ref.mae(sev_true, sp), 'spearman_rho': ref.spearman_rho(sev_true, sp), 'brier_score': ref.brier_score(labels, probs),
                   'ece': ref.ece(labels, probs), 'ece_15': ref.ece(labels, probs, n_bins=15)}
            cm = ref.compute_confusion_matrix(labels, pred, CLASS_NAMES)
        for k, v in (('logits', logits), ('labels', labels), ('sev_true', sev_true), ('sev_pred', sev_pred), ('probs', probs32),
                     ('pred', pred.astype(np.int64)), ('confusion', np.asarray(cm, dtype=np.int64))):
            out[f'{name}/{k}'] = v
        for k, v in exp.items():
            out[f'{name}/{k}'] = np.float64(v)
        for field in ('precision', 'recall', 'f1', 'support'):
            out[f'{name}/per_class_{field}'] = np.array([pc[c][field] for c in CLASS_NAMES], dtype=np.float64)
        print(name, n, {k: float(v) for k, v in exp.items()})
    np.savez_compressed(a.out, **out)
    print('wrote', a.out, os.path.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
