"""Time the k-means entry points and append one JSON line per (case, size, arm) to profiles/kmeans_time.jsonl.

Device-resident fp32 feature rows, E = 192, metric l2, ONE Gaussian blob with the backbone's covariance spectrum (1 down to 1e-3, every
row's mean removed): data without planted clusters, on which Lloyd does not stop within the timed 20 iterations (every `fused` record
carries `converged`, read from the status block after the timed runs, so that a run the stopping flag cut short is visible).

  --case run     n in {4096, 65536, 2^20} x k in {4, 64, 256}, 20 iterations from the same k given centroids (rows of the data):
                 `fused` = KMeans(k, max_iter=20, init=centroids).fit (rows kernel, then per iteration the assign kernel, the three
                 launches of the counting sort, the segment sums and the finalize launch; the final pass on top; no n x k matrix);
                 `torch` = the recipe on the same device: |x|^2 + |c|^2 - 2 x @ c.T in chunks of --chunk rows, argmin, index_add_ and
                 bincount for the update.
  --case assign  one assignment of the n rows against k centroids: `fused` = KMeans.predict; `knn` = FeatureIndex.search(k=1) over the
                 centroids (the general search kernel with its key workspace and merge launch); `torch` = one pass of the recipe.
  --case seed    k-means++ alone: `fused` = kmeans_pp (three launches per seed, nothing waits for the host); `torch` = the same D^2
                 sampling with torch ops on the device (cumsum + searchsorted, no host synchronisation either).
  --case sort    the alternative the update did not take: `radix_sort` = rovit_hip.rank.sort_columns of the n labels as fp32 (the stable
                 device radix sort: its permutation is the members of every cluster in ascending row index).  The counting sort inside
                 the run has no entry of its own; its three launches are in profiles/kmeans_kernel_stats.txt.
  --sklearn      with --case run: sklearn.cluster.KMeans on the host (lloyd, tol 0, the same init, 20 iterations) once per size up to
                 65536 rows: context only.

Every arm is warmed once; the arms alternate in one process; --repeats timed runs each; host clock between two device synchronisations;
median, min and max per arm.  No ratio is promised: the records say what was measured, whichever arm wins.

--kernels-only: three calls of the fused run per size for a separate ``rocprofv3 --kernel-trace --stats`` run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)

E, ITERS = 192, 20
SIZES = tuple((n, k) for n in (4096, 65536, 1 << 20) for k in (4, 64, 256))


def make_rows(n, seed=0):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((E, E)))
    x = (rng.standard_normal((n, E), dtype=np.float32) * np.sqrt(np.geomspace(1.0, 1e-3, E)).astype(np.float32)[None]) @ Q.T.astype(np.float32)
    x -= x.mean(axis=1, keepdims=True)
    return x.astype(np.float32)


def torch_assign(x, xn, c, chunk):
    cn = (c * c).sum(1)
    out = []
    for r0 in range(0, x.shape[0], chunk):
        d = (xn[r0:r0 + chunk, None] + cn[None]) - 2.0 * (x[r0:r0 + chunk] @ c.T)
        out.append(d.argmin(dim=1))
    return torch.cat(out)


def torch_run(x, c, chunk):
    xn = (x * x).sum(1)
    k = c.shape[0]
    for _ in range(ITERS):
        labels = torch_assign(x, xn, c, chunk)
        sums = torch.zeros_like(c).index_add_(0, labels, x)
        counts = torch.bincount(labels, minlength=k).clamp(min=1)
        c = sums / counts[:, None]
    return torch_assign(x, xn, c, chunk), c


def torch_seed(x, m, gen_seed=0):
    g = torch.Generator(device=x.device).manual_seed(gen_seed)
    r = torch.rand(m, generator=g, device=x.device)
    n = x.shape[0]
    xn = (x * x).sum(1)
    idx = torch.empty(m, dtype=torch.long, device=x.device)
    idx[0] = (r[0] * n).long().clamp(max=n - 1)
    d = None
    for j in range(1, m):
        c = x[idx[j - 1]]
        dj = ((xn + xn[idx[j - 1]]) - 2.0 * (x @ c)).clamp(min=0)
        d = dj if d is None else torch.minimum(d, dj)
        cs = torch.cumsum(d, 0)
        idx[j] = torch.searchsorted(cs, r[j] * cs[-1]).clamp(max=n - 1)
    return idx


def time_arms(arms, repeats):
    for fn in arms.values():                                 # the warm run
        fn()
    times = {k: [] for k in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    return times


def records(case, n, k, times, extra):
    out = []
    med = {name: sorted(v)[len(v) // 2] * 1e3 for name, v in times.items()}
    for name, v in times.items():
        t = sorted(x * 1e3 for x in v)
        rec = {'case': case, 'n': n, 'k': k, 'embed': E, 'arm': name, 'median_ms': round(med[name], 3), 'min_ms': round(t[0], 3),
               'max_ms': round(t[-1], 3), 'repeats': len(t), 'device': torch.cuda.get_device_name(0)}
        if case == 'run':
            rec['iterations'] = ITERS
        if name == 'fused':
            rec.update({f'{other}_over_fused': round(med[other] / med['fused'], 2) for other in med if other != 'fused'}, **extra)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', choices=('run', 'assign', 'seed', 'sort'), required=True)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--chunk', type=int, default=65536, help="rows per block of the recipe's x @ c.T (65536 x 256 fp32 = 64 MiB)")
    ap.add_argument('--max-rows', type=int, default=1 << 20)
    ap.add_argument('--sklearn', action='store_true')
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kmeans_time.jsonl'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    from rovit_hip import clustering as CL
    from rovit_hip import neighbors as NB
    dev = torch.device('cuda:0')
    sizes = [s for s in SIZES if s[0] <= a.max_rows]
    rows_all = torch.from_numpy(make_rows(max(n for n, _ in sizes))).to(dev)
    lines = []
    for n, k in sizes:
        x = rows_all[:n]
        c0 = x[torch.from_numpy(np.random.default_rng(1).permutation(n)[:k]).to(dev)].clone()
        extra = {}
        if a.case == 'run':
            km = CL.KMeans(k, max_iter=ITERS, init=c0)
            arms = {'fused': lambda: km.fit(x), 'torch': lambda: torch_run(x, c0, a.chunk)}
        elif a.case == 'assign':
            km = CL.KMeans(k).load_state_dict({'n_clusters': k, 'metric': 'l2', 'max_iter': 1, 'n_init': 1, 'seed': 0, 'cluster_centers': c0},
                                              device=dev)
            fi = NB.FeatureIndex(E, None, 'l2', capacity=k)
            fi.update(c0)
            fi.build()
            xn = (x * x).sum(1)
            arms = {'fused': lambda: km.predict(x), 'knn': lambda: fi.search(x, k=1), 'torch': lambda: torch_assign(x, xn, c0, a.chunk)}
        elif a.case == 'sort':
            from rovit_hip import rank as RK
            labels = torch.from_numpy(np.random.default_rng(2).integers(0, k, n).astype(np.float32)).to(dev)
            arms = {'radix_sort': lambda: RK.sort_columns(labels)}
        else:
            arms = {'fused': lambda: CL.kmeans_pp(x, k, 'l2', seed=0), 'torch': lambda: torch_seed(x, k)}
        if a.kernels_only:
            for _ in range(3):
                arms['fused']()
            torch.cuda.synchronize()
            print(f'kernels-only run done: {a.case} n = {n} k = {k}', flush=True)
            continue
        times = time_arms(arms, a.repeats)
        if a.case == 'run':
            st = km.status_
            mine, theirs = km.labels_.long(), torch_run(x, c0, a.chunk)[0]
            extra = {'converged': st['converged'], 'n_iter': st['n_iter'], 'labels_agree_with_torch': float((mine == theirs).double().mean()),
                     'workspace_bytes': int(CL.native.load().rovit_kmeans_workspace_bytes(n, E, k)),
                     'torch_temporary_bytes': 4 * min(a.chunk, n) * k}
        elif a.case == 'assign':
            extra = {'labels_agree_with_knn': float((km.predict(x)['labels'] == fi.search(x, k=1)['indices'][:, 0]).double().mean())}
        lines += records(a.case, n, k, times, extra)
        if a.sklearn and a.case == 'run' and n <= 65536:
            from sklearn.cluster import KMeans as SK
            xh, ch = x.cpu().numpy(), c0.cpu().numpy()
            t0 = time.perf_counter()
            SK(k, init=ch, n_init=1, max_iter=ITERS, tol=0.0, algorithm='lloyd').fit(xh)
            rec = {'case': 'run', 'n': n, 'k': k, 'embed': E, 'arm': 'sklearn_host', 'ms': round((time.perf_counter() - t0) * 1e3, 1),
                   'repeats': 1, 'iterations': ITERS, 'note': 'context only: host CPU, one run'}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    with open(a.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
