"""Exact t-SNE of the feature space on the GPU: the 2-D map of recorded backbone features (van der Maaten & Hinton 2008).

Every other tool on ``outputs['features']`` returns a score or a list of neighbours; this one returns the figure a user of a vision
backbone draws first: where the classes sit, where the rows a label audit names lie, whether new photographs fall off the training
cloud.  The exact algorithm is an all-pairs problem in two dimensions; ``csrc/tsne.hip`` runs it with a dense P and without the host
looking at the optimisation.  No tree, no neighbour list: the result is the exact method, not an approximation of it.

Definitions.  Rows x_i are fp32; a row is *valid* when every feature and its squared norm are finite (with 'cosine' also a positive
norm); a row that is not valid is absent from everything below and keeps NaN coordinates in the map.  With 'cosine' the distances are
taken between the unit rows x / |x|.
  D_ij = sum_k (x_ik - x_jk)^2, the difference form (no cancellation: D_ii = 0 and exact duplicates are at distance 0).
  p_j|i = w_j / sum_j w_j over the valid j != i, w_j = exp(-beta_i (D_ij - min_j D_ij)); beta_i from exactly 64 steps of van der
  Maaten's bisection on H(beta) = log S + beta sum d w / S against log(perplexity), from beta = 1: double while there is no upper
  bracket, halve while there is no lower one, else move half way to the other bracket.  A row whose two brackets never both existed
  is *unconverged*: it has at least ``perplexity`` exact duplicates, beta ends at 2^64 and the row is uniform over the duplicates.
  P_ij = max((p_j|i + p_i|j) / (2 n_valid), 1e-12) for valid i != j, else 0.
  One iteration, with w_ij = 1 / (1 + |y_i - y_j|^2) over the valid j != i: a_i = sum P_ij w_ij (y_i - y_j), r_i = sum w_ij^2 (y_i - y_j),
  Z = sum_i sum_j w_ij, g_i = 4 (alpha a_i - r_i / Z); gain = gain + 0.2 where v g < 0, else 0.8 gain, then max(gain, 0.01);
  v = m v - eta gain g; y += v (sklearn's ``_gradient_descent``).  KL = sum P_ij (log P_ij - log w_ij) + log Z sum P_ij, recorded
  at the iterations t with t % kl_every == 0 and at the last one, from the map the iteration starts from.
  alpha = early_exaggeration and m = 0.5 for the first ``exaggeration_iter`` iterations, then 1 and 0.8; ``learning_rate='auto'`` is
  max(n_valid / early_exaggeration / 4, 50).  After the last iteration the mean of the valid rows is subtracted once.

On CUDA tensors every method runs the kernels and copies nothing to the host: ``status_``, ``kl_divergence_`` and the host view of
the trace come from ONE device-to-host copy made on first access.  On CPU tensors every method runs the numpy fp64 statements below
(``distances_reference``, ``affinities_reference``, ``step_reference``, ``run_reference``), the kernels' oracle.
``init='pca'`` is plain torch (plumbing, once): the fp64 covariance of the valid rows and ``torch.linalg.eigh`` on the features' device.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from . import native
from .native import RovitHipError
from .neighbors import METRICS, FeatureIndex, valid_rows, _unit_rows

BISECTION_STEPS = 64
P_FLOOR = 1e-12
INIT_STD = 1e-4


def _np(t, dtype=None) -> np.ndarray:
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a if dtype is None else a.astype(dtype, copy=False)


def check_rows(n, E, who: str = 'TSNE') -> None:
    if not (4 <= n <= native.TSNE_MAX_ROWS):
        raise RovitHipError(f'{who}: {n} rows; the dense method takes 4..{native.TSNE_MAX_ROWS} rows (TSNE_MAX_ROWS)')
    if not (32 <= E <= 256 and E % 32 == 0):
        raise RovitHipError(f'{who}: embed must be a multiple of 32 in 32..256, got {E}')


def check_perplexity(perplexity, n, who: str = 'TSNE') -> None:
    if not (isinstance(perplexity, (int, float)) and 1.0 < float(perplexity) < n - 1):
        raise RovitHipError(f'{who}: perplexity must lie inside (1, n - 1) = (1, {n - 1}), got {perplexity!r}')


# ---- host statements: the oracle -------------------------------------------------------------------------------------------------------

def distances_reference(features, metric: str = 'l2'):
    """(D, valid): the (n, n) fp64 squared distances of the definition from fp32 rows (a double loop over the rows, the difference form;
    with 'cosine' between the fp64 unit rows), 0 where a row is not valid, and the (n,) validity flags."""
    if metric not in METRICS:
        raise RovitHipError(f'distances_reference: metric must be one of {sorted(METRICS)}, got {metric!r}')
    x32 = _np(features, np.float32)
    ok = valid_rows(x32, metric)
    x = _unit_rows(x32, ok) if metric == 'cosine' else np.where(ok[:, None], x32, 0).astype(np.float64)
    n = x.shape[0]
    D = np.zeros((n, n))
    for i in range(n):
        if ok[i]:
            diff = x[i][None, :] - x
            D[i] = np.where(ok, (diff * diff).sum(axis=1), 0.0)
    return D, ok


def conditional_row(d: np.ndarray, log_perplexity: float):
    """One row of the bisection in fp64: ``d`` the distances to the row's candidates.  Returns (p, beta, H, converged)."""
    d = d - d.min()
    beta, lo, hi = 1.0, None, None
    for step in range(BISECTION_STEPS + 1):
        w = np.exp(-(beta * d))
        S = w.sum()
        H = np.log(S) + beta * (d * w).sum() / S
        if step == BISECTION_STEPS:
            break
        if H > log_perplexity:
            lo = beta
            beta = beta * 2.0 if hi is None else 0.5 * (beta + hi)
        else:
            hi = beta
            beta = beta * 0.5 if lo is None else 0.5 * (beta + lo)
    return w / S, beta, H, (lo is not None and hi is not None)


def affinities_reference(features=None, perplexity: float = 30.0, metric: str = 'l2', symmetrize: bool = True, D=None, valid=None) -> Dict:
    """``TSNE.affinities`` in numpy fp64, from the rows or from given distances ``D`` (n, n) and flags ``valid``: ``P`` (the conditional
    matrix with ``symmetrize=False``), ``beta``, ``entropy`` and ``status`` (n, n_valid, bad_rows, unconverged, min_beta, max_beta)."""
    if D is None:
        D, valid = distances_reference(features, metric)
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    ok = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    check_perplexity(perplexity, n, 'affinities_reference')
    C, beta, H = np.zeros((n, n)), np.zeros(n), np.zeros(n)
    unconverged = 0
    for i in range(n):
        cand = ok.copy()
        cand[i] = False
        if not ok[i] or not cand.any():
            continue
        p, beta[i], H[i], conv = conditional_row(D[i, cand], float(np.log(perplexity)))
        C[i, cand] = p
        unconverged += 0 if conv else 1
    nv = int(ok.sum())
    status = {'n': n, 'n_valid': nv, 'bad_rows': n - nv, 'unconverged': unconverged,
              'min_beta': float(beta[ok].min()) if nv else float('inf'), 'max_beta': float(beta[ok].max()) if nv else float('-inf')}
    if symmetrize:
        pair = ok[:, None] & ok[None, :] & ~np.eye(n, dtype=bool)
        C = np.where(pair, np.maximum((C + C.T) / (2.0 * nv), P_FLOOR), 0.0)
    return {'P': C, 'beta': beta, 'entropy': H, 'status': status}


def map_valid(Y: np.ndarray) -> np.ndarray:
    return ~np.isnan(Y).any(axis=1)


def kl_reference(P, Y) -> float:
    """KL(P || Q) of the definition in fp64, Q_ij = w_ij / Z over the valid i != j (a row of Y with a NaN is absent)."""
    P, Y = np.asarray(P, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    ok = map_valid(Y)
    n = Y.shape[0]
    A = B = Z = 0.0
    for i in range(n):
        for j in range(n):
            if i == j or not (ok[i] and ok[j]):
                continue
            w = 1.0 / (1.0 + ((Y[i] - Y[j]) ** 2).sum())
            Z += w
            if P[i, j] > 0:
                A += P[i, j] * (np.log(P[i, j]) - np.log(w))
                B += P[i, j]
    return float(A + np.log(Z) * B)


def forces_reference(P, Y) -> Dict:
    """a (n, 2), r (n, 2), Z and the KL divergence of the definition in fp64, with ``abs_a`` and ``abs_r``, the sums of the absolute
    values of the terms of a and r (what an error bound of the device sums scales with)."""
    P, Y = np.asarray(P, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    ok = map_valid(Y)
    pair = ok[:, None] & ok[None, :] & ~np.eye(Y.shape[0], dtype=bool)
    Ys = np.where(ok[:, None], Y, 0.0)
    diff = Ys[:, None, :] - Ys[None, :, :]
    w = np.where(pair, 1.0 / (1.0 + (diff * diff).sum(axis=2)), 0.0)
    pw = np.where(pair, P, 0.0) * w
    Z = float(w.sum())
    with np.errstate(divide='ignore', invalid='ignore'):
        terms = np.where(pair & (P > 0), P * (np.log(np.where(P > 0, P, 1.0)) - np.log(np.where(pair, w, 1.0))), 0.0)
    B = float(np.where(pair & (P > 0), P, 0.0).sum())
    return {'a': (pw[:, :, None] * diff).sum(axis=1), 'r': ((w * w)[:, :, None] * diff).sum(axis=1), 'Z': Z,
            'abs_a': (pw[:, :, None] * np.abs(diff)).sum(axis=1), 'abs_r': ((w * w)[:, :, None] * np.abs(diff)).sum(axis=1),
            'kl': float(terms.sum() + np.log(Z) * B), 'valid': ok}


def step_reference(P, Y, V, G, exaggeration: float, momentum: float, learning_rate: float) -> Dict:
    """One iteration of the definition in fp64: the new ``Y``, ``V``, ``G``, and ``grad``, ``Z``, ``kl`` of the map it started from
    (with ``abs_a``, ``abs_r`` of ``forces_reference``).  Rows of Y with a NaN stay as they are."""
    Y, V, G = (np.array(_np(t), dtype=np.float64) for t in (Y, V, G))
    f = forces_reference(P, Y)
    ok = f['valid']
    g = 4.0 * (float(exaggeration) * f['a'] - f['r'] / f['Z'])
    g[~ok] = 0.0
    inc = V * g < 0.0
    Gn = np.maximum(np.where(inc, G + 0.2, G * 0.8), 0.01)
    Vn = float(momentum) * V - float(learning_rate) * Gn * g
    okc = ok[:, None]
    Gn, Vn = np.where(okc, Gn, G), np.where(okc, Vn, V)
    return {'Y': np.where(okc, Y + Vn, Y), 'V': Vn, 'G': Gn, 'grad': g, 'Z': f['Z'], 'kl': f['kl'], 'abs_a': f['abs_a'],
            'abs_r': f['abs_r'], 'valid': ok}


def resolve_learning_rate(learning_rate, n_valid: int, early_exaggeration: float) -> float:
    return max(n_valid / float(early_exaggeration) / 4.0, 50.0) if learning_rate == 'auto' else float(learning_rate)


def kl_slots(n_iter: int, kl_every: int):
    """The iterations whose KL divergence the trace holds, in order."""
    return [t for t in range(n_iter) if kl_every > 0 and (t % kl_every == 0 or t == n_iter - 1)]


def run_reference(P, Y0, n_iter: int = 1000, early_exaggeration: float = 12.0, exaggeration_iter: int = 250, learning_rate='auto',
                  kl_every: int = 50, dtype=np.float64) -> Dict:
    """The whole descent of the definition in numpy (fp64; ``dtype=np.float32`` restates it in fp32 for comparison): ``map`` (centred on
    the valid rows), ``kl_trace`` at ``kl_slots(n_iter, kl_every)``, ``kl_divergence`` (the last trace value)."""
    P = np.asarray(P, dtype=dtype)
    Y = np.array(_np(Y0), dtype=dtype)
    ok = map_valid(Y)
    pair = ok[:, None] & ok[None, :] & ~np.eye(Y.shape[0], dtype=bool)
    Pm = np.where(pair, P, 0).astype(dtype)
    eta = dtype(resolve_learning_rate(learning_rate, int(ok.sum()), early_exaggeration))
    V, G = np.zeros_like(Y), np.ones_like(Y)
    slots, trace = set(kl_slots(n_iter, kl_every)), []
    one = dtype(1.0)
    for t in range(n_iter):
        alpha, m = (dtype(early_exaggeration), dtype(0.5)) if t < exaggeration_iter else (one, dtype(0.8))
        Ys = np.where(ok[:, None], Y, 0).astype(dtype)
        diff = Ys[:, None, :] - Ys[None, :, :]
        w = np.where(pair, one / (one + (diff * diff).sum(axis=2)), 0).astype(dtype)
        Z = w.sum(dtype=dtype)
        if t in slots:
            with np.errstate(divide='ignore', invalid='ignore'):
                terms = np.where(Pm > 0, Pm * (np.log(np.where(Pm > 0, Pm, 1)) - np.log(np.where(pair, w, 1))), 0)
            trace.append(float(terms.sum(dtype=np.float64) + np.log(float(Z)) * float(Pm.sum(dtype=np.float64))))
        g = dtype(4.0) * (alpha * ((Pm * w)[:, :, None] * diff).sum(axis=1) - ((w * w)[:, :, None] * diff).sum(axis=1) / Z)
        g = np.where(ok[:, None], g, 0).astype(dtype)
        G = np.maximum(np.where(V * g < 0, G + dtype(0.2), G * dtype(0.8)), dtype(0.01)).astype(dtype)
        V = (m * V - eta * G * g).astype(dtype)
        Y = np.where(ok[:, None], Y + V, Y).astype(dtype)
    Y = Y - np.where(ok[:, None], Y, 0).sum(axis=0, dtype=np.float64).astype(dtype) / dtype(max(int(ok.sum()), 1))
    return {'map': Y, 'kl_trace': np.asarray(trace), 'kl_divergence': trace[-1] if trace else float('nan')}


def random_init_reference(n: int, seed: int) -> np.ndarray:
    """The 'random' init in numpy: 1e-4 x Box-Muller normals from ``oracle.philox``, counter (element, 0, TSNE_STREAM, 0), key = seed."""
    from oracle.philox import philox4x32_10 as philox          # checker only, like the other modules' draws
    e = np.arange(2 * n, dtype=np.uint64)
    full = lambda v: np.full(2 * n, v, np.uint64)
    w = philox([e, full(0), full(native.TSNE_STREAM), full(0)], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    u1 = ((w[0] >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (w[1] >> np.uint64(8)).astype(np.float64) / 16777216.0
    return (INIT_STD * np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)).reshape(n, 2)


def pca_init(features: torch.Tensor, metric: str = 'l2') -> torch.Tensor:
    """The 'pca' init on the features' device in fp64: the projection of the centred valid rows on the two leading eigenvectors of their
    covariance, each eigenvector's largest-magnitude component made positive, scaled so that column 0 has standard deviation 1e-4;
    NaN in the rows that are not valid.  Returns fp32 (n, 2)."""
    x = features.detach().to(torch.float64)
    norm2 = (features.detach().float() ** 2).sum(dim=1)
    ok = torch.isfinite(x).all(dim=1) & torch.isfinite(norm2)
    if metric == 'cosine':
        ok = ok & (norm2 > 0)
    okc = ok[:, None]
    xs = torch.where(okc, x, torch.zeros_like(x))
    cnt = ok.sum().clamp(min=1).to(torch.float64)
    xc = torch.where(okc, xs - xs.sum(dim=0) / cnt, torch.zeros_like(x))
    cov = xc.T @ xc / cnt
    _, vec = torch.linalg.eigh(cov)
    top = vec[:, [-1, -2]]
    pick = top.abs().argmax(dim=0)
    top = top * torch.sign(top.gather(0, pick[None, :]))
    y = xc @ top
    y = y * (INIT_STD / torch.sqrt((y[:, 0] ** 2).sum() / cnt - (y[:, 0].sum() / cnt) ** 2))
    return torch.where(okc, y, torch.full_like(y, float('nan'))).to(torch.float32)


# ---- the estimator ---------------------------------------------------------------------------------------------------------------------

def _rows_of(features) -> torch.Tensor:
    x = features.rows() if hasattr(features, 'rows') else features      # a FeatureIndex (or anything that records rows the same way)
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise RovitHipError(f'TSNE: features must be an (n, E) tensor or an index with rows(), got {type(features).__name__}')
    return x.detach()


class TSNE:
    """Exact t-SNE; see the module docstring.  ``max_workgroups`` > 0 caps every grid (tests); the results do not depend on it."""

    def __init__(self, perplexity: float = 30.0, n_iter: int = 1000, early_exaggeration: float = 12.0, exaggeration_iter: int = 250,
                 learning_rate='auto', metric: str = 'l2', init='pca', seed: int = 0, kl_every: int = 50):
        if metric not in METRICS:
            raise RovitHipError(f'TSNE: metric must be one of {sorted(METRICS)}, got {metric!r}')
        if not (isinstance(perplexity, (int, float)) and float(perplexity) > 1.0):
            raise RovitHipError(f'TSNE: perplexity must exceed 1, got {perplexity!r}')
        if not (isinstance(n_iter, int) and 1 <= n_iter <= native.TSNE_MAX_ITER):
            raise RovitHipError(f'TSNE: n_iter must be in 1..{native.TSNE_MAX_ITER}, got {n_iter!r}')
        if not (isinstance(exaggeration_iter, int) and exaggeration_iter >= 0 and isinstance(kl_every, int) and kl_every >= 0):
            raise RovitHipError(f'TSNE: exaggeration_iter and kl_every must be integers >= 0, got {exaggeration_iter!r}, {kl_every!r}')
        if not (isinstance(early_exaggeration, (int, float)) and float(early_exaggeration) > 0):
            raise RovitHipError(f'TSNE: early_exaggeration must be positive, got {early_exaggeration!r}')
        if not (learning_rate == 'auto' or (isinstance(learning_rate, (int, float)) and float(learning_rate) > 0)):
            raise RovitHipError(f"TSNE: learning_rate must be 'auto' or positive, got {learning_rate!r}")
        if not (isinstance(init, torch.Tensor) or init in ('pca', 'random')):
            raise RovitHipError(f"TSNE: init must be 'pca', 'random' or an (n, 2) tensor, got {init!r}")
        self.perplexity, self.n_iter, self.early_exaggeration = float(perplexity), n_iter, float(early_exaggeration)
        self.exaggeration_iter, self.learning_rate, self.metric, self.init = exaggeration_iter, learning_rate, metric, init
        self.seed, self.kl_every = int(seed), kl_every
        self.max_workgroups = 0
        self.embedding_: Optional[torch.Tensor] = None
        self.kl_trace_: Optional[torch.Tensor] = None
        self._packed = self._host = None

    # -- checks and buffers --------------------------------------------------------------------------------------------------------------
    def _checked(self, features, who: str) -> torch.Tensor:
        x = _rows_of(features)
        check_rows(int(x.shape[0]), int(x.shape[1]), who)
        check_perplexity(self.perplexity, int(x.shape[0]), who)
        return x.float().contiguous()

    @staticmethod
    def _workspace(n: int, E: int, device) -> torch.Tensor:
        nbytes = native.load().rovit_tsne_workspace_bytes(n, E)
        if nbytes == 0:
            raise RovitHipError(f'TSNE: no workspace for {n} rows of {E} features (outside the limits)')
        return torch.empty(nbytes, dtype=torch.uint8, device=device)

    def _affinities_device(self, x: torch.Tensor, symmetrize: bool, distances_only: bool = False) -> Dict[str, torch.Tensor]:
        n, E = x.shape
        out = {'P': torch.empty((n, n), dtype=torch.float32, device=x.device), 'beta': torch.empty(n, dtype=torch.float32, device=x.device),
               'entropy': torch.empty(n, dtype=torch.float32, device=x.device),
               'status': torch.zeros(native.TSNE_WORDS, dtype=torch.int64, device=x.device)}
        ws = self._workspace(n, E, x.device)
        d = native.TsneAffinity()
        d.n, d.embed, d.metric, d.symmetrize, d.distances_only, d.max_workgroups = n, E, METRICS[self.metric], int(symmetrize), int(distances_only), self.max_workgroups
        d.perplexity = self.perplexity
        d.features, d.workspace, d.workspace_bytes = native.ptr(x), native.ptr(ws), ws.numel()
        d.P, d.beta, d.entropy, d.status = (native.ptr(out[k]) for k in ('P', 'beta', 'entropy', 'status'))
        native.call('rovit_tsne_affinities', ctypes.byref(d), native.stream_ptr())
        out['valid'] = ws[:4 * n].view(torch.int32) != 0          # the workspace's first section: the flags of the rows
        return out

    # -- public --------------------------------------------------------------------------------------------------------------------------
    def distances(self, features) -> torch.Tensor:
        """The (n, n) squared distances D of the definition (fp32 on a CUDA device, the fp64 statement on the CPU)."""
        x = self._checked(features, 'TSNE.distances')
        if not x.is_cuda:
            return torch.from_numpy(distances_reference(x.numpy(), self.metric)[0])
        return self._affinities_device(x, False, True)['P']

    def affinities(self, features, symmetrize: bool = True) -> Dict:
        """``P`` (n, n) (the conditional matrix p_j|i with ``symmetrize=False``), ``beta`` (n), ``entropy`` (n) and ``status``: on a CUDA
        device fp32 tensors and the int64 status words (nothing copied to the host); on the CPU the fp64 statements and a dict."""
        x = self._checked(features, 'TSNE.affinities')
        if not x.is_cuda:
            ref = affinities_reference(x.numpy(), self.perplexity, self.metric, symmetrize)
            return {'P': torch.from_numpy(ref['P']), 'beta': torch.from_numpy(ref['beta']), 'entropy': torch.from_numpy(ref['entropy']),
                    'status': ref['status']}
        out = self._affinities_device(x, symmetrize)
        out.pop('valid')
        return out

    def _initial(self, x: torch.Tensor) -> torch.Tensor:
        n = x.shape[0]
        if isinstance(self.init, torch.Tensor):
            if tuple(self.init.shape) != (n, 2) or self.init.device != x.device:
                raise RovitHipError(f'TSNE: init must be ({n}, 2) on {x.device}, got {tuple(self.init.shape)} on {self.init.device}')
            return self.init.detach().float().clone().contiguous()
        if self.init == 'pca':
            return pca_init(x, self.metric).contiguous()
        if not x.is_cuda:
            return torch.from_numpy(random_init_reference(n, self.seed).astype(np.float32))
        Y = torch.empty((n, 2), dtype=torch.float32, device=x.device)
        native.call('rovit_tsne_random_init', ctypes.c_ulonglong(self.seed), native.ptr(Y), n, native.stream_ptr())
        return Y

    def fit_transform(self, features) -> torch.Tensor:
        """The (n, 2) map on the features' device; NaN in the rows that are not valid.  Nothing is copied to the host."""
        x = self._checked(features, 'TSNE.fit_transform')
        Y = self._initial(x)                                       # refusals come before any launch of the method's own
        n = x.shape[0]
        self._packed = self._host = None
        if not x.is_cuda:
            aff = affinities_reference(x.numpy(), self.perplexity, self.metric, True)
            ok = valid_rows(x.numpy(), self.metric)
            Y0 = np.where(ok[:, None], Y.numpy().astype(np.float64), np.nan)
            run = run_reference(aff['P'], Y0, self.n_iter, self.early_exaggeration, self.exaggeration_iter, self.learning_rate,
                                self.kl_every or self.n_iter)
            self.embedding_ = torch.from_numpy(run['map'].astype(np.float32))
            self.kl_trace_ = torch.from_numpy(run['kl_trace'].astype(np.float32))
            self._host = dict(aff['status'], iterations=self.n_iter, nonfinite=int((~np.isfinite(run['map'][ok])).any(axis=1).sum()),
                              kl_trace=run['kl_trace'], kl_divergence=run['kl_divergence'])
            return self.embedding_
        aff = self._affinities_device(x, True)
        Y = torch.where(aff['valid'][:, None], Y, torch.full_like(Y, float('nan'))).contiguous()
        V, G = torch.zeros_like(Y), torch.ones_like(Y)
        lr = 0.0 if self.learning_rate == 'auto' else float(self.learning_rate)
        trace, status = self._run_device(aff['P'], Y, V, G, self.n_iter, self.exaggeration_iter, self.early_exaggeration, 0.5, 0.8, lr,
                                         self.kl_every or self.n_iter, center=True)
        self.embedding_, self.kl_trace_ = Y, trace
        self._packed = torch.cat([aff['status'], status, trace.view(torch.int32).to(torch.int64)])      # on the device: no copy yet
        return Y

    def _run_device(self, P, Y, V, G, n_iter, exaggeration_iter, early_exaggeration, m_early, m_late, lr, kl_every, center,
                    grad_out=None, z_out=None):
        n = Y.shape[0]
        slots = len(kl_slots(n_iter, kl_every))
        trace = torch.zeros(max(slots, 1), dtype=torch.float32, device=Y.device)
        status = torch.zeros(native.TSNE_WORDS, dtype=torch.int64, device=Y.device)
        ws = self._workspace(n, 32, Y.device)
        d = native.TsneDescent()
        d.n, d.n_iter, d.exaggeration_iter, d.kl_every, d.center, d.max_workgroups = n, n_iter, exaggeration_iter, kl_every, int(center), self.max_workgroups
        d.trace_capacity, d.early_exaggeration, d.momentum_early, d.momentum_late, d.learning_rate = trace.numel(), early_exaggeration, m_early, m_late, lr
        d.P, d.Y, d.V, d.G = native.ptr(P), native.ptr(Y), native.ptr(V), native.ptr(G)
        d.workspace, d.workspace_bytes, d.trace, d.status = native.ptr(ws), ws.numel(), native.ptr(trace), native.ptr(status)
        d.grad_out, d.z_out = native.ptr(grad_out), native.ptr(z_out)
        native.call('rovit_tsne_run', ctypes.byref(d), native.stream_ptr())
        return trace[:slots], status

    def step(self, P, Y, V, G, exaggeration: float, momentum: float, learning_rate: float) -> Dict:
        """One iteration on (n, n) ``P`` and (n, 2) ``Y``, ``V``, ``G`` (updated in place; fp32 contiguous on a CUDA device): returns
        ``grad`` (n, 2), ``Z`` and ``kl`` of the map the iteration started from.  No centring.  For tests and tools."""
        n = Y.shape[0]
        if tuple(P.shape) != (n, n) or any(tuple(t.shape) != (n, 2) for t in (Y, V, G)) or not (4 <= n <= native.TSNE_MAX_ROWS):
            raise RovitHipError(f'TSNE.step: P (n, n) and Y, V, G (n, 2) with 4 <= n <= {native.TSNE_MAX_ROWS}, got {tuple(P.shape)}, {tuple(Y.shape)}')
        if not (float(learning_rate) > 0 and float(exaggeration) > 0 and 0 <= float(momentum) < 1):
            raise RovitHipError('TSNE.step: exaggeration and learning_rate must be positive, momentum inside [0, 1)')
        if not Y.is_cuda:
            ref = step_reference(_np(P), Y, V, G, exaggeration, momentum, learning_rate)
            for t, k in ((Y, 'Y'), (V, 'V'), (G, 'G')):
                t.copy_(torch.from_numpy(ref[k]).to(t.dtype))
            return {'grad': torch.from_numpy(ref['grad']), 'Z': torch.tensor(ref['Z'], dtype=torch.float64),
                    'kl': torch.tensor(ref['kl'], dtype=torch.float64)}
        if any(t.dtype != torch.float32 for t in (P, Y, V, G)):
            raise RovitHipError('TSNE.step: fp32 tensors on the device')
        grad, z = torch.empty_like(Y), torch.empty(1, dtype=torch.float32, device=Y.device)
        trace, _ = self._run_device(P, Y, V, G, 1, 1, float(exaggeration), float(momentum), float(momentum), float(learning_rate), 1,
                                    center=False, grad_out=grad, z_out=z)
        return {'grad': grad, 'Z': z[0], 'kl': trace[0]}

    # -- host values: one copy, on first access ------------------------------------------------------------------------------------------
    def _values(self) -> Dict:
        if self._host is None:
            if self._packed is None:
                raise RovitHipError('TSNE: fit_transform has not run yet')
            w = self._packed.cpu().numpy()                         # the single device-to-host copy
            r = w[native.TSNE_WORDS:2 * native.TSNE_WORDS]
            trace = w[2 * native.TSNE_WORDS:].astype(np.int32).view(np.float32).astype(np.float64)
            self._host = dict(decode_status(w[:native.TSNE_WORDS]), iterations=int(r[native.TSNE_RUN_ITERATIONS]),
                              nonfinite=int(r[native.TSNE_RUN_NONFINITE]), kl_trace=trace, kl_divergence=float(trace[-1]))
        return self._host

    @property
    def status_(self) -> Dict:
        """n, n_valid, bad_rows, unconverged, min_beta, max_beta, iterations, nonfinite (valid rows of the map with an infinite
        coordinate): reported, never raised."""
        return {k: v for k, v in self._values().items() if k not in ('kl_trace', 'kl_divergence')}

    @property
    def kl_divergence_(self) -> float:
        return self._values()['kl_divergence']


def decode_status(status) -> Dict:
    """The status words of ``TSNE.affinities`` as a dict (a device-to-host copy when they are a CUDA tensor)."""
    w = _np(status).astype(np.int64)
    bits = lambda v: float(np.array([v], dtype=np.int64).astype(np.uint32).view(np.float32)[0])
    return {'n': int(w[native.TSNE_N]), 'n_valid': int(w[native.TSNE_N_VALID]), 'bad_rows': int(w[native.TSNE_BAD_ROWS]),
            'unconverged': int(w[native.TSNE_UNCONVERGED]), 'min_beta': bits(w[native.TSNE_MIN_BETA]), 'max_beta': bits(w[native.TSNE_MAX_BETA])}


def knn_preservation(features, Y, k: int = 10, metric: str = 'l2') -> float:
    """The mean overlap |N_k^features(i) & N_k^map(i)| / k over the rows that are valid in both: each row's k nearest neighbours in
    feature space (``metric``) and in the map (l2), itself excluded.  Both searches run through ``FeatureIndex``; the map is zero-padded
    to 32 columns, which changes no l2 distance."""
    x, y = _rows_of(features).float(), Y.detach().float()
    n = x.shape[0]
    if tuple(y.shape) != (n, 2) or y.device != x.device:
        raise RovitHipError(f'knn_preservation: the map must be ({n}, 2) on {x.device}, got {tuple(y.shape)} on {y.device}')
    if not (isinstance(k, int) and 1 <= k <= native.KNN_MAX_K and k < n):
        raise RovitHipError(f'knn_preservation: k must be in 1..{native.KNN_MAX_K} and below n, got {k!r}')
    me = torch.arange(n, dtype=torch.int32, device=x.device)
    pad = torch.zeros((n, 32), dtype=torch.float32, device=x.device)
    pad[:, :2] = y
    found = []
    for rows, m in ((x.contiguous(), metric), (pad, 'l2')):
        fi = FeatureIndex(int(rows.shape[1]), None, m, capacity=n)
        fi.update(rows)
        found.append(fi.build().search(rows, k=k, exclude=me)['indices'].to(torch.int64))
    a, b = found
    both = (a[:, 0] >= 0) & (b[:, 0] >= 0)
    hits = ((a[:, :, None] == b[:, None, :]) & (a[:, :, None] >= 0)).any(dim=2).sum(dim=1)
    return float(hits[both].sum()) / float(max(int(both.sum()), 1) * k)
