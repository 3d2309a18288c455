"""Time one evaluation epoch three ways and append one JSON line per (case, arm) to profiles/evaluation_time.jsonl.

  fused  : evaluation.Evaluator's loop (one forward and one rovit_eval_accumulate launch per batch, rovit_eval_finalize and ONE
           device-to-host copy per epoch, the metrics derived on the host)
  recipe : the reference's collection loop (evaluation/evaluator.py:37-67: softmax, argmax, squeeze, exp, five device-to-host copies
           per batch, host labels through .numpy()) and its sklearn / scipy metrics, written out below against the same model.  This is
           the yardstick: the reference's procedure, not the code under test.
  floor  : the bare ``model(images)`` loop with one final synchronisation

Cases: --images synthetic images resident on the device, at every --batch and --precision; and validate() against the reference's
val_epoch recipe (training/trainer.py:183-231, six .item() per batch) at --val-batch.  Every shape is warmed up; the arms alternate
(fused, recipe, floor, fused, ...); each arm runs at least --repeats epochs and at least --min-seconds in all; host clock between two
device synchronisations (none inside an epoch but the arm's own).  median, min, max and spread (max - min) per arm; fused - recipe and
fused - floor from the medians.

--kernels-only N: no model; the record launch at batch 32 and 256 and the finalise at N rows on seeded logits, for a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_evaluation.py --kernels-only N`` run; --kernel-stats CSV N appends the eval_*
rows of that run's kernel_stats.csv to the same .jsonl.
"""
import argparse
import csv
import json
import os
import sys
import time
import warnings
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)

CLASS_NAMES = ['Healthy Leaf', 'Leaf Holes', 'Black Spot', 'Dry Leaf']


def recipe_evaluate(model, loader, dev):
    from scipy.stats import spearmanr
    from sklearn.metrics import f1_score, precision_recall_fscore_support
    preds, labels, sev_p, sev_t, probs, unc = [], [], [], [], [], []
    with torch.no_grad():
        for images, class_labels, severity_labels in loader:
            outputs = model(images.to(dev))
            p = torch.softmax(outputs['cls_logits'], dim=1)
            pred = torch.argmax(p, dim=1)
            sev = outputs['kan_severity'].squeeze()
            preds.append(pred.cpu().numpy())
            labels.append(class_labels.numpy())
            sev_p.append(sev.cpu().numpy())
            sev_t.append(severity_labels.numpy())
            probs.append(p.cpu().numpy())
            unc.append(torch.exp(0.5 * outputs['log_var']).cpu().numpy())
    y_pred, y_true, s_pred, s_true, y_prob = (np.concatenate(v) for v in (preds, labels, sev_p, sev_t, probs))
    onehot = np.zeros_like(y_prob)
    onehot[np.arange(len(y_true)), y_true] = 1
    conf, hit = y_prob.max(1), (y_prob.argmax(1) == y_true).astype(float)
    ece = 0.0
    edges = np.linspace(0, 1, 11)
    for lo, hi in zip(edges[:-1], edges[1:]):
        m = (conf > lo) & (conf <= hi)
        if m.mean() > 0:
            ece += abs(conf[m].mean() - hit[m].mean()) * m.mean()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return {'accuracy': np.mean(y_true == y_pred) * 100, 'macro_f1': f1_score(y_true, y_pred, average='macro') * 100,
                'weighted_f1': f1_score(y_true, y_pred, average='weighted') * 100, 'mae': np.mean(np.abs(s_true - s_pred)),
                'spearman_rho': spearmanr(s_true, s_pred)[0], 'brier_score': np.mean(np.sum((y_prob - onehot) ** 2, axis=1)), 'ece': ece,
                'per_class': precision_recall_fscore_support(y_true, y_pred, labels=range(len(CLASS_NAMES)), zero_division=0)}


def recipe_val_epoch(model, loader, loss_fn, dev):
    model.eval()
    sums, correct, total = [0.0] * 5, 0, 0
    with torch.no_grad():
        for images, class_labels, severity_labels in loader:
            images, class_labels, severity_labels = images.to(dev), class_labels.to(dev), severity_labels.to(dev)
            outputs = model(images)
            losses = loss_fn(outputs, class_labels, severity_labels, stage=4)
            for i, k in enumerate(('total_loss', 'cls_loss', 'ord_loss', 'unc_loss', 'kan_loss')):
                sums[i] += losses[k].item()
            _, predicted = outputs['cls_logits'].max(1)
            total += class_labels.size(0)
            correct += predicted.eq(class_labels).sum().item()
    return [s / len(loader) for s in sums] + [100. * correct / total]


def floor(model, loader, dev):
    with torch.no_grad():
        for images, _, _ in loader:
            model(images.to(dev))
    torch.cuda.synchronize()


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


def records(case, times, n_batches):
    med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}
    out = []
    for name, v in times.items():
        t = sorted(x * 1e3 for x in v)
        rec = dict(case, arm=name, median_ms=round(med[name], 3), min_ms=round(t[0], 3), max_ms=round(t[-1], 3),
                   spread_ms=round(t[-1] - t[0], 3), median_ms_per_batch=round(med[name] / n_batches, 4), repeats=len(t),
                   device=torch.cuda.get_device_name(0))
        if name == 'fused':
            rec['fused_minus_recipe_ms'] = round(med['fused'] - med['recipe'], 3)
            if 'floor' in med:
                rec['fused_minus_floor_ms'] = round(med['fused'] - med['floor'], 3)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def kernels_only(n):
    from rovit_hip.evaluation import EvalAccumulator
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(n)
    logits, labels = torch.randn(n, 4, generator=g).to(dev), torch.randint(0, 4, (n,), generator=g).to(dev)
    sev, lv = (labels.float() + torch.randn(n, generator=g).to(dev)).reshape(-1, 1), torch.randn(n, 1, generator=g).to(dev)
    for rep in range(5):
        for B in (32, 256):
            acc = EvalAccumulator(4, capacity=n)
            for i in range(0, n, B):
                acc.update({'cls_logits': logits[i:i + B], 'kan_severity': sev[i:i + B], 'mu': lv[i:i + B], 'log_var': lv[i:i + B]},
                           labels[i:i + B], labels[i:i + B])
            acc.compute()
    torch.cuda.synchronize()
    print('kernels-only run done: n =', n)


def kernel_stats(path, n, out):
    with open(path) as f, open(out, 'a') as o:
        for row in csv.DictReader(f):
            if 'eval_' in row['Name']:
                name = row['Name'].split('::')[-1].split('(')[0]
                rec = {'case': 'kernel', 'rows': n, 'record_batches': [32, 256], 'kernel': name, 'calls': int(row['Calls']),
                       'avg_us': round(float(row['AverageNs']) / 1e3, 2), 'min_us': round(float(row['MinNs']) / 1e3, 2),
                       'max_us': round(float(row['MaxNs']) / 1e3, 2)}
                print(json.dumps(rec))
                o.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=4096)
    ap.add_argument('--batch', type=int, nargs='+', default=[32, 256])
    ap.add_argument('--precision', nargs='+', default=['bf16', 'fp32'])
    ap.add_argument('--val-batch', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--kernels-only', type=int, default=0, metavar='N')
    ap.add_argument('--kernel-stats', nargs=2, metavar=('CSV', 'N'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'evaluation_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats[0], int(a.kernel_stats[1]), a.out)
    if a.kernels_only:
        return kernels_only(a.kernels_only)
    from oracle import ref_cpu
    from evaluation.evaluator import Evaluator
    from models.rovit_kan import RoViTKAN
    from rovit_hip.evaluation import validate
    from rovit_hip.losses import JointLoss
    dev = torch.device('cuda:0')
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    m = m.to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.randn(a.images, 3, 224, 224, device=dev, generator=g)
    labels = torch.randint(0, 4, (a.images,), generator=torch.Generator().manual_seed(1))           # host labels, as a DataLoader's
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=CLASS_NAMES, num_classes=4))
    lines = []
    for B in a.batch:
        loader = [(images[i:i + B], labels[i:i + B], labels[i:i + B]) for i in range(0, a.images, B)]
        ev = Evaluator(m, loader, cfg, dev)
        for prec in a.precision:
            m.backbone.model.precision = prec
            arms = {'fused': lambda: ev.collect().compute(), 'recipe': lambda: recipe_evaluate(m, loader, dev), 'floor': lambda: floor(m, loader, dev)}
            times = time_arms(arms, a.repeats, a.min_seconds, a.warmup)
            lines += records({'case': 'evaluate', 'images': a.images, 'batch': B, 'precision': prec}, times, len(loader))
        m.backbone.model.precision = 'bf16'
    B = a.val_batch
    loader = [(images[i:i + B], labels[i:i + B], labels[i:i + B]) for i in range(0, a.images, B)]
    loss_fn = JointLoss(1.0, 0.5, 0.5, 2.0, num_classes=4)
    arms = {'fused': lambda: validate(m, loader, loss_fn), 'recipe': lambda: recipe_val_epoch(m, loader, loss_fn, dev),
            'floor': lambda: floor(m, loader, dev)}
    times = time_arms(arms, a.repeats, a.min_seconds, a.warmup)
    lines += records({'case': 'validate', 'images': a.images, 'batch': B, 'precision': 'bf16'}, times, len(loader))
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
