"""Last-layer Laplace approximation of the heads: closed-form epistemic uncertainty, no sampling, no retraining, no labels.

The library's other epistemic figure, MC dropout (``predict_mc``), costs T head samples per image and means nothing for a head whose
dropout was never trained.  The standard post-hoc answer is a Gaussian posterior over the LAST linear layer of a trained head with the
generalised Gauss-Newton Hessian (Kristiadi et al., ICML 2020; Daxberger et al., "Laplace Redux", NeurIPS 2021).  The reference has
none of it ("parity unpinned": every rule below is this repository's own statement of the standard ones).

Definitions (eval semantics, no dropout; fp64 on the host unless said otherwise).  For a head with fc1 (hid, E):
  a_i = [relu(fc1 f_i + b1); 1]          the augmented hidden row of the fp32 feature row f_i = outputs['features'], D = hid + 1 wide
Classification head, theta = [fc2.weight, fc2.bias], C D parameters ordered class-major (index c D + a):
  p_i = softmax(cls_logits_i)             the model's own logits, taken as given
  lambda_i,cc = p_c (1 - p_c), lambda_i,cd = -p_c p_d;  G_cd = sum_i lambda_i,cd a_i a_i^T;  H = [G_cd] (the GGN, K = C (C + 1) / 2 Grams)
  S[c][d] = (e_c (x) a)^T (H + tau I)^-1 (e_d (x) a)            the logit covariance of a query row
Gaussian head, theta = [fc_mu.weight, fc_mu.bias], a' from the uncertainty head's own fc1:
  H_mu = sum_i exp(-log_var_i) a'_i a'_i^T;  v_mu = a'^T (H_mu + tau_mu I)^-1 a';  total_std = sqrt(exp(log_var) + v_mu)
  fc_logvar is treated as fixed: a block-diagonal approximation of the joint Hessian of the two output layers.
Prior precision: a given float, or 'marglik' (the default): the maximiser over [1e-6, 1e6] of the Laplace evidence
  -tau/2 |theta*|^2 + D/2 log tau - 1/2 sum_j log(e_j + tau), e_j the eigenvalues of H.  Its derivative is
  1/2 (sum_j e_j / (tau (e_j + tau)) - |theta*|^2), strictly decreasing in tau: one root, found by bisection on log tau; no root inside
  the range means the maximum sits at an end ('at_min' / 'at_max', as ``Calibration`` reports it).  ``log_marginal_likelihood`` is the
  expression above: the evidence up to the data term log p(D | theta*), which does not depend on tau and would need the labels.
Predictive: the generalised probit approximation p' = softmax(z_c / sqrt(1 + (pi / 8) S_cc)); S -> 0 gives softmax(z) exactly.
Numerical form: a^T P^-1 a with an fp32 P^-1 cancels.  The host factors P = R R^T in fp64 and sends W = R^-1 (lower-triangular) as fp32;
  z_c = W[:, block c] a and S[c][d] = z_c . z_d are sums of products that do not cancel.  On the device the rows are padded from D to
  P = hid + 32 columns with exact zeros, so W is (C P, C P) with the padding's rows and columns zero.

``HeadLaplace.update`` copies rows to an offset the host knows (no synchronisation); ``fit`` launches ``rovit_laplace_weights`` and one
``rovit_laplace_gram`` per head (csrc/laplace.hip), makes ONE device-to-host copy, and does the eigenvalues, tau, Cholesky and the
triangular inverse on the host in fp64; ``predict`` is one ``rovit_laplace_predict`` launch per head.  On CPU tensors the same entry
points run the numpy fp64 statements below (``weights_reference``, ``gram_reference``, ``laplace_reference``, ``predict_reference``),
the kernels' oracle, as every other accumulator here does.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import native
from .native import RovitHipError

TAU_MIN, TAU_MAX = 1e-6, 1e6
STATUS = ('interior', 'at_min', 'at_max')
PI_8 = math.pi / 8.0


def _np(t, dtype=None) -> np.ndarray:
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a if dtype is None else a.astype(dtype, copy=False)


def check_shape(E: int, hid: int, C: int) -> None:
    if not (isinstance(E, int) and 32 <= E <= 256 and E % 32 == 0):
        raise RovitHipError(f'HeadLaplace: embed_dim must be a multiple of 32 in 32..256, got {E!r}')
    if not (isinstance(hid, int) and 32 <= hid <= 256 and hid % 32 == 0):
        raise RovitHipError(f'HeadLaplace: the hidden width must be a multiple of 32 in 32..256, got {hid!r}')
    if not (isinstance(C, int) and 1 <= C <= native.EVAL_MAX_CLASSES):
        raise RovitHipError(f'HeadLaplace: num_classes must be in 1..{native.EVAL_MAX_CLASSES}, got {C!r}')


def pair_index(C: int):
    """The K = C (C + 1) / 2 pairs (c, d), c <= d, in the order of the weight table's columns."""
    return [(c, d) for c in range(C) for d in range(c, C)]


# ---- host statements (fp64) ----------------------------------------------------------------------------------------------------------

def augmented_hidden(features, fc1_weight, fc1_bias, dtype=np.float64) -> np.ndarray:
    """a = [relu(fc1 f + b1); 1], (n, hid + 1), evaluated in ``dtype`` from the fp32 inputs."""
    f = _np(features, np.float32).astype(dtype)
    w, b = _np(fc1_weight, np.float32).astype(dtype), _np(fc1_bias, np.float32).astype(dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        h = np.maximum(f @ w.T + b[None], 0)                      # a NaN passes, as torch.relu lets it
    return np.concatenate([h, np.ones((h.shape[0], 1), dtype=dtype)], axis=1)


def weights_reference(cls_logits=None, log_var=None, dtype=np.float32) -> Dict:
    """``rovit_laplace_weights`` on the host: ``cls_weights`` (n, K) and ``mu_weights`` (n) as fp32 (fp64 softmax / exp, rounded once),
    ``bad_logits`` and ``bad_log_var``: rows with a non-finite input (or a weight that is not finite in fp32), whose weights are 0.
    ``dtype=np.float64`` keeps the weights unrounded (the same rows are bad)."""
    out: Dict = {'bad_logits': 0, 'bad_log_var': 0}
    if cls_logits is not None:
        l = _np(cls_logits, np.float32).astype(np.float64)
        if l.ndim != 2 or not (1 <= l.shape[1] <= native.EVAL_MAX_CLASSES):
            raise RovitHipError(f'laplace weights: cls_logits must be (n, 1..{native.EVAL_MAX_CLASSES}), got {l.shape}')
        C = l.shape[1]
        bad = ~np.isfinite(l).all(axis=1)
        ls = np.where(bad[:, None], 0.0, l)
        e = np.exp(ls - ls.max(axis=1, keepdims=True))
        s = np.zeros(l.shape[0])
        for c in range(C):
            s = s + e[:, c]
        cols = []
        for c, d in pair_index(C):
            if c == d:
                rest = np.zeros(l.shape[0])
                for j in range(C):
                    if j != c:
                        rest = rest + e[:, j]
                cols.append(e[:, c] * rest * (1.0 / (s * s)))
            else:
                cols.append(-(e[:, c] * e[:, d]) * (1.0 / (s * s)))
        w = np.stack(cols, axis=1)
        w[bad] = 0.0
        out['cls_weights'], out['bad_logits'] = w.astype(dtype), int(bad.sum())
    if log_var is not None:
        v = _np(log_var, np.float32).astype(np.float64).reshape(-1)
        with np.errstate(over='ignore', invalid='ignore'):
            w64 = np.exp(-v)
            bad = ~np.isfinite(v) | ~np.isfinite(w64.astype(np.float32))
        w64[bad] = 0.0
        out['mu_weights'], out['bad_log_var'] = w64.astype(dtype), int(bad.sum())
    return out


def gram_reference(features, fc1_weight, fc1_bias, weights) -> Dict:
    """``rovit_laplace_gram`` in numpy fp64 on the kernel's own fp32 inputs: ``gram`` (K, D, D) = sum_i w_ik a_i a_i^T over the valid rows,
    ``n``, ``n_valid``, ``bad_rows`` (a non-finite feature or weight)."""
    x = _np(features, np.float32)
    w = _np(weights)
    w = w.astype(np.float32 if w.dtype != np.float64 else np.float64, copy=False).reshape(x.shape[0], -1)
    if x.ndim != 2 or x.shape[0] < 1 or not (1 <= w.shape[1] <= native.LAPLACE_MAX_WEIGHTS):
        raise RovitHipError(f'laplace gram: features (n >= 1, E) with weights (n, 1..{native.LAPLACE_MAX_WEIGHTS}), got {x.shape} and {w.shape}')
    valid = np.isfinite(x).all(axis=1) & np.isfinite(w).all(axis=1)
    a = augmented_hidden(x[valid], fc1_weight, fc1_bias)
    wv = w[valid].astype(np.float64)
    G = np.einsum('ik,ia,ib->kab', wv, a, a, optimize=True)
    return {'n': int(x.shape[0]), 'n_valid': int(valid.sum()), 'bad_rows': int((~valid).sum()), 'gram': 0.5 * (G + G.transpose(0, 2, 1))}


def gram_block_reference(features, fc1_weight, fc1_bias, weights) -> np.ndarray:
    """The result block of ``rovit_laplace_gram`` as int64 words from ``gram_reference``."""
    g = gram_reference(features, fc1_weight, fc1_bias, weights)
    K, D = g['gram'].shape[0], g['gram'].shape[1]
    blk = np.zeros(native.laplace_words(D - 1, K), dtype=np.int64)
    blk[native.LAPLACE_N], blk[native.LAPLACE_N_VALID], blk[native.LAPLACE_BAD_ROWS] = g['n'], g['n_valid'], g['bad_rows']
    blk.view(np.float64)[native.LAPLACE_HEADER:] = g['gram'].reshape(-1)
    return blk


def gram_from_block(blk: np.ndarray, hid: int, K: int) -> Dict:
    blk = np.asarray(blk, dtype=np.int64)
    D = hid + 1
    return {'n': int(blk[native.LAPLACE_N]), 'n_valid': int(blk[native.LAPLACE_N_VALID]), 'bad_rows': int(blk[native.LAPLACE_BAD_ROWS]),
            'gram': blk.view(np.float64)[native.LAPLACE_HEADER:native.LAPLACE_HEADER + K * D * D].reshape(K, D, D).copy()}


def assemble_hessian(gram: np.ndarray, C: int) -> np.ndarray:
    """H (C D, C D), class-major, from the K = C (C + 1) / 2 Grams: block (c, d) = block (d, c) = G_cd."""
    D = gram.shape[1]
    H = np.zeros((C * D, C * D))
    for k, (c, d) in enumerate(pair_index(C)):
        H[c * D:(c + 1) * D, d * D:(d + 1) * D] = gram[k]
        H[d * D:(d + 1) * D, c * D:(c + 1) * D] = gram[k]
    return 0.5 * (H + H.T)


def evidence(tau: float, eig: np.ndarray, theta_sq: float) -> float:
    """-tau/2 |theta|^2 + D/2 log tau - 1/2 sum log(e_j + tau)."""
    return float(-0.5 * tau * theta_sq + 0.5 * eig.shape[0] * math.log(tau) - 0.5 * np.log(eig + tau).sum())


def stationarity(tau: float, eig: np.ndarray, theta_sq: float) -> float:
    """sum_j e_j / (tau (e_j + tau)) - |theta|^2: twice the evidence's derivative, strictly decreasing in tau."""
    return float((eig / (tau * (eig + tau))).sum() - theta_sq)


def marglik_prior_precision(eig: np.ndarray, theta_sq: float) -> Tuple[float, str]:
    """The maximiser of ``evidence`` over [TAU_MIN, TAU_MAX] and its status, by bisection on log tau."""
    eig = np.maximum(np.asarray(eig, dtype=np.float64), 0.0)
    if stationarity(TAU_MIN, eig, theta_sq) <= 0.0:
        return TAU_MIN, 'at_min'
    if stationarity(TAU_MAX, eig, theta_sq) >= 0.0:
        return TAU_MAX, 'at_max'
    lo, hi = math.log(TAU_MIN), math.log(TAU_MAX)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if stationarity(math.exp(mid), eig, theta_sq) > 0.0:
            lo = mid
        else:
            hi = mid
    a, b = math.exp(lo), math.exp(hi)
    return (a if abs(stationarity(a, eig, theta_sq)) <= abs(stationarity(b, eig, theta_sq)) else b), 'interior'


def whitening_of(H: np.ndarray, tau: float) -> np.ndarray:
    """W = R^-1 with H + tau I = R R^T, lower-triangular (the upper triangle exactly zero)."""
    try:
        R = np.linalg.cholesky(H + tau * np.eye(H.shape[0]))
    except np.linalg.LinAlgError as e:
        raise RovitHipError(f'HeadLaplace.fit: the posterior precision is not positive definite ({e})') from None
    return np.tril(np.linalg.solve(R, np.eye(H.shape[0])))


def pad_whitening(W: np.ndarray, C: int, hid: int) -> np.ndarray:
    """(C D, C D) -> (C P, C P), P = hid + 32: parameter c D + a moves to c P + a, the padding's rows and columns are zero."""
    D, P = hid + 1, hid + 32
    idx = (np.arange(C)[:, None] * P + np.arange(D)[None]).reshape(-1)
    out = np.zeros((C * P, C * P), dtype=W.dtype)
    out[np.ix_(idx, idx)] = W
    return out


def fit_from_gram(gram: np.ndarray, C: int, theta, prior_precision='marglik') -> Dict:
    """H, its eigenvalues, tau with its status, the evidence and the padded whitening table (fp64 here) from the Grams of one head and
    its last layer's parameters ``theta`` (any shape; only |theta|^2 enters)."""
    hid = gram.shape[1] - 1
    H = assemble_hessian(gram, C)
    eig = np.maximum(np.linalg.eigvalsh(H), 0.0)
    theta_sq = float((np.asarray(theta, dtype=np.float64) ** 2).sum())
    if isinstance(prior_precision, str):
        if prior_precision != 'marglik':
            raise RovitHipError(f"HeadLaplace.fit: prior_precision must be a positive number or 'marglik', got {prior_precision!r}")
        tau, status = marglik_prior_precision(eig, theta_sq)
    else:
        tau, status = float(prior_precision), 'interior'
        if not (math.isfinite(tau) and tau > 0.0):
            raise RovitHipError(f"HeadLaplace.fit: prior_precision must be a positive number or 'marglik', got {prior_precision!r}")
    W = whitening_of(H, tau)
    return {'hessian': H, 'eigenvalues': eig, 'theta_sq': theta_sq, 'prior_precision': tau, 'status': status,
            'log_marginal_likelihood': evidence(tau, eig, theta_sq), 'whitening64': pad_whitening(W, C, hid)}


def laplace_reference(features, cls_logits, fc1_weight, fc1_bias, theta, prior_precision='marglik', log_var=None,
                      device_weights: bool = False) -> Dict:
    """The whole fit of ONE head in numpy fp64.  With ``log_var`` None the classification head (``cls_logits`` (n, C), ``theta`` = fc2's
    weight and bias); with ``log_var`` the Gaussian head (``cls_logits`` ignored, ``theta`` = fc_mu's weight and bias, C = 1).  Returns
    ``fit_from_gram``'s keys plus ``weights``, ``gram``, ``n``, ``n_valid``, ``bad_rows``, ``bad_inputs`` and ``whitening`` (the fp32
    table ``predict_reference`` and the kernel read).  The GGN weights stay in fp64 unless ``device_weights`` rounds them to fp32 as
    ``rovit_laplace_weights`` does."""
    wd = np.float32 if device_weights else np.float64
    if log_var is None:
        wr = weights_reference(cls_logits=cls_logits, dtype=wd)
        w, C, bad_inputs = wr['cls_weights'], _np(cls_logits).shape[1], wr['bad_logits']
    else:
        wr = weights_reference(log_var=log_var, dtype=wd)
        w, C, bad_inputs = wr['mu_weights'][:, None], 1, wr['bad_log_var']
    g = gram_reference(features, fc1_weight, fc1_bias, w)
    if g['n_valid'] < 1:
        raise RovitHipError(f"HeadLaplace.fit: no valid row among {g['n']}")
    out = fit_from_gram(g['gram'], C, theta, prior_precision)
    out.update(g)
    out.update({'weights': w, 'bad_inputs': bad_inputs, 'whitening': out['whitening64'].astype(np.float32)})
    return out


def probit_probs(logits: np.ndarray, var: np.ndarray) -> np.ndarray:
    t = logits / np.sqrt(1.0 + PI_8 * var)
    e = np.exp(t - t.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def predict_reference(features, fc1_weight, fc1_bias, whitening, num_classes: int, logits=None) -> Dict[str, np.ndarray]:
    """The predict kernel's outputs in fp64 from fp32 feature rows and the whitening table AS GIVEN (so a test against the kernel never
    involves the host's Cholesky): ``logit_cov`` (B, C, C), ``logit_var`` (B, C), and with ``logits`` ``probs``, ``confidence_score``
    = 1 - max probs and ``mean_logit_var``."""
    W = np.asarray(_np(whitening), dtype=np.float64)
    C = num_classes
    a = augmented_hidden(features, fc1_weight, fc1_bias)
    D, P = a.shape[1], W.shape[0] // C
    if W.shape != (C * P, C * P) or P != D + 31:
        raise RovitHipError(f'laplace predict: the whitening table must be ({C * (D + 31)}, {C * (D + 31)}), got {W.shape}')
    ap = np.zeros((a.shape[0], P))
    ap[:, :D] = a
    z = np.stack([ap @ W[:, c * P:(c + 1) * P].T for c in range(C)], axis=1)          # (B, C, C P)
    S = np.einsum('bct,bdt->bcd', z, z)
    var = np.einsum('bcc->bc', S).copy()
    out = {'logit_cov': S, 'logit_var': var}
    if logits is not None:
        l = _np(logits, np.float32).astype(np.float64)
        p = probit_probs(l, var)
        out['probs'] = p
        am = p.argmax(axis=1)
        rest = p.copy()
        rest[np.arange(p.shape[0]), am] = 0.0
        out['confidence_score'] = rest.sum(axis=1)
        out['mean_logit_var'] = var.mean(axis=1)
    return out


# ---- heads -----------------------------------------------------------------------------------------------------------------------------

def _resolve_heads(model_or_heads):
    """(classification head, uncertainty head or None) from a model (``classification_head`` / ``uncertainty_head`` attributes), a pair,
    or a lone classification head."""
    if hasattr(model_or_heads, 'classification_head'):
        return model_or_heads.classification_head, getattr(model_or_heads, 'uncertainty_head', None)
    if isinstance(model_or_heads, (tuple, list)) and len(model_or_heads) == 2:
        return model_or_heads[0], model_or_heads[1]
    return model_or_heads, None


def _cls_params(h):
    return [h.fc1.weight, h.fc1.bias, h.fc2.weight, h.fc2.bias]


def _mu_params(h):
    return [h.fc1.weight, h.fc1.bias, h.fc_mu.weight, h.fc_mu.bias]


class HeadLaplace:
    """Last-layer Laplace approximation of a classification head and, when ``log_var`` rows were recorded, of the Gaussian head's ``mu``
    layer; see the module docstring.  ``update`` never synchronises; ``fit`` copies one block to the host; ``predict`` is one launch per
    head.  Fields after ``fit``: ``prior_precision`` / ``status`` / ``log_marginal_likelihood`` (classification head), the same with
    the suffix ``_mu`` (None without a Gaussian part), ``n``, ``n_valid``, ``bad_rows``, ``bad_logits``, ``bad_log_var``."""

    def __init__(self, model_or_heads, capacity: int = 4096):
        cls_head, unc_head = _resolve_heads(model_or_heads)
        for name in ('fc1', 'fc2'):
            if not isinstance(getattr(cls_head, name, None), torch.nn.Linear):
                raise RovitHipError(f'HeadLaplace: the classification head needs a Linear {name}')
        if unc_head is not None and not all(isinstance(getattr(unc_head, k, None), torch.nn.Linear) for k in ('fc1', 'fc_mu')):
            raise RovitHipError('HeadLaplace: the uncertainty head needs Linear fc1 and fc_mu')
        if not (isinstance(capacity, int) and 1 <= capacity <= native.KAN_STATS_MAX_ROWS):
            raise RovitHipError(f'HeadLaplace: capacity must be in 1..{native.KAN_STATS_MAX_ROWS}, got {capacity!r}')
        self.cls_head, self.unc_head = cls_head, unc_head
        self.embed_dim, self.hid, self.num_classes = cls_head.fc1.in_features, cls_head.fc1.out_features, cls_head.fc2.out_features
        check_shape(self.embed_dim, self.hid, self.num_classes)
        if cls_head.fc2.in_features != self.hid or cls_head.fc1.bias is None or cls_head.fc2.bias is None:
            raise RovitHipError('HeadLaplace: the classification head must be fc1 -> ReLU -> fc2, both with a bias')
        if unc_head is not None:
            self.hid_mu = unc_head.fc1.out_features
            check_shape(unc_head.fc1.in_features, self.hid_mu, 1)
            if unc_head.fc1.in_features != self.embed_dim or unc_head.fc_mu.out_features != 1 or unc_head.fc1.bias is None or unc_head.fc_mu.bias is None:
                raise RovitHipError('HeadLaplace: the uncertainty head must read the same features and give one mu, with biases')
        self._capacity0 = capacity
        self.max_workgroups = 0                                    # > 0 caps every grid (tests); the results do not depend on it
        self.reset()

    def reset(self) -> None:
        self.n = 0
        self.device: Optional[torch.device] = None
        self._rows = self._logits = self._log_var = None
        self._has_log_var: Optional[bool] = None
        self._cpu = []
        self._clear_fit()

    def _clear_fit(self) -> None:
        self._block: Optional[np.ndarray] = None
        self.tables: Optional[Dict[str, torch.Tensor]] = None
        self._tables_on: Dict[torch.device, Dict[str, torch.Tensor]] = {}
        self._versions = None
        self.prior_precision = self.status = self.log_marginal_likelihood = None
        self.prior_precision_mu = self.status_mu = self.log_marginal_likelihood_mu = None
        self.n_valid = self.bad_rows = self.bad_logits = self.bad_log_var = 0
        self.n_valid_mu = self.bad_rows_mu = 0

    @property
    def fitted(self) -> bool:
        return self.tables is not None

    @property
    def has_gaussian(self) -> bool:
        return self.tables is not None and 'whitening_mu' in self.tables

    # -- recording --

    def _reserve(self, rows: int) -> None:
        cap = self._rows.shape[0] if self._rows is not None else 0
        if rows <= cap:
            return
        if rows > native.KAN_STATS_MAX_ROWS:
            raise RovitHipError(f'HeadLaplace: {rows} rows exceed the limit of {native.KAN_STATS_MAX_ROWS}')
        new_cap = min(native.KAN_STATS_MAX_ROWS, max(rows, 2 * cap, self._capacity0))
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
        new, lg, lv = f32(new_cap, self.embed_dim), f32(new_cap, self.num_classes), f32(new_cap) if self._has_log_var else None
        if self._rows is not None:
            new[:self.n].copy_(self._rows[:self.n])                # device-to-device, stream-ordered: no synchronisation
            lg[:self.n].copy_(self._logits[:self.n])
            if lv is not None:
                lv[:self.n].copy_(self._log_var[:self.n])
        self._rows, self._logits, self._log_var = new, lg, lv

    def update(self, features: torch.Tensor, cls_logits: torch.Tensor, log_var: Optional[torch.Tensor] = None) -> None:
        """Record a batch: (B, E) feature rows, their (B, C) classification logits and, from curriculum stage 3, their (B,) or (B, 1)
        ``log_var``.  Either every batch carries ``log_var`` or none does."""
        x, lg = features.detach(), cls_logits.detach()
        lv = None if log_var is None else log_var.detach().reshape(-1)
        E, C = self.embed_dim, self.num_classes
        if x.dim() != 2 or x.shape[1] != E or x.shape[0] < 1 or tuple(lg.shape) != (x.shape[0], C) or (lv is not None and lv.shape[0] != x.shape[0]):
            raise RovitHipError(f'HeadLaplace.update: features must be (B >= 1, {E}) with (B, {C}) logits and B log_var, got '
                                f'{tuple(x.shape)}, {tuple(lg.shape)} and {None if log_var is None else tuple(log_var.shape)}')
        if lg.device != x.device or (lv is not None and lv.device != x.device):
            raise RovitHipError('HeadLaplace.update: the features, logits and log_var must share a device')
        if lv is not None and self.unc_head is None:
            raise RovitHipError('HeadLaplace.update: log_var without an uncertainty head')
        if self._has_log_var is None:
            self._has_log_var = lv is not None
        elif self._has_log_var != (lv is not None):
            raise RovitHipError('HeadLaplace.update: either every batch carries log_var or none does; reset() first')
        if self.device is None:
            self.device = x.device
        elif x.device != self.device:
            raise RovitHipError(f'HeadLaplace.update: batch on {x.device}, earlier batches on {self.device}; reset() first')
        self._clear_fit()
        B = x.shape[0]
        if not x.is_cuda:
            self._cpu.append((x.float().clone(), lg.float().clone(), None if lv is None else lv.float().clone()))
        else:
            self._reserve(self.n + B)
            self._rows[self.n:self.n + B].copy_(x)
            self._logits[self.n:self.n + B].copy_(lg)
            if lv is not None:
                self._log_var[self.n:self.n + B].copy_(lv)
        self.n += B

    # -- fitting --

    def _layout(self) -> Dict[str, int]:
        """Word offsets of the one block ``fit`` copies: the weight kernel's counts, the classification Grams, the Gaussian Gram."""
        C = self.num_classes
        K = C * (C + 1) // 2
        cls = native.LAPLACE_COUNT_WORDS
        mu = cls + native.laplace_words(self.hid, K)
        return {'counts': 0, 'cls': cls, 'mu': mu, 'words': mu + (native.laplace_words(self.hid_mu, 1) if self._has_log_var else 0), 'K': K}

    def _head_arrays(self):
        c = [_np(p, np.float32) for p in _cls_params(self.cls_head)]
        u = [_np(p, np.float32) for p in _mu_params(self.unc_head)] if self._has_log_var else None
        return c, u

    def result_block(self) -> np.ndarray:
        """The block ``fit`` reads, as int64 words on the host (the fp64 part bit for bit): ``rovit_laplace_weights``' two counts, then
        ``rovit_laplace_gram``'s block of the classification head, then the Gaussian head's.  On the device this is the one
        synchronising call; the block is kept until the next ``update`` or ``reset``."""
        if self._block is not None:
            return self._block
        if self.n < 1:
            raise RovitHipError('HeadLaplace: nothing recorded yet')
        lay = self._layout()
        C, K, E = self.num_classes, lay['K'], self.embed_dim
        if self.device.type != 'cuda':
            x = torch.cat([b[0] for b in self._cpu]).numpy()
            lg = torch.cat([b[1] for b in self._cpu]).numpy()
            lv = torch.cat([b[2] for b in self._cpu]).numpy() if self._has_log_var else None
            (w1, b1, _, _), u = self._head_arrays()
            wr = weights_reference(lg, lv)
            blk = np.zeros(lay['words'], dtype=np.int64)
            blk[native.LAPLACE_BAD_LOGITS], blk[native.LAPLACE_BAD_LOG_VAR] = wr['bad_logits'], wr['bad_log_var']
            blk[lay['cls']:lay['mu']] = gram_block_reference(x, w1, b1, wr['cls_weights'])
            if lv is not None:
                blk[lay['mu']:] = gram_block_reference(x, u[0], u[1], wr['mu_weights'][:, None])
            self._block = blk
            return blk
        lib = native.load()
        dev, n = self.device, self.n
        result = torch.empty(lay['words'], dtype=torch.int64, device=dev)
        w_cls = torch.empty((n, K), dtype=torch.float32, device=dev)
        w_mu = torch.empty(n, dtype=torch.float32, device=dev) if self._has_log_var else None
        wa = native.LaplaceWeightArgs()
        wa.n, wa.num_classes, wa.max_workgroups = n, C, self.max_workgroups
        wa.cls_logits, wa.log_var = native.ptr(self._logits), native.ptr(self._log_var) if self._has_log_var else None
        wa.cls_weights, wa.mu_weights, wa.counts = native.ptr(w_cls), native.ptr(w_mu), native.ptr(result)
        native.call('rovit_laplace_weights', ctypes.byref(wa), native.stream_ptr())
        keep = []
        for head_params, hid, weights, k, off in ((_cls_params(self.cls_head), self.hid, w_cls, K, lay['cls']),
                                                  (_mu_params(self.unc_head) if self._has_log_var else None, getattr(self, 'hid_mu', 0), w_mu, 1, lay['mu'])):
            if head_params is None:
                continue
            w1, b1 = head_params[0].detach().float().contiguous(), head_params[1].detach().float().contiguous()
            nbytes = lib.rovit_laplace_workspace_bytes(n, E, hid, k)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            keep += [w1, b1, ws]
            d = native.LaplaceFit()
            d.n, d.embed, d.hid, d.num_weights, d.max_workgroups = n, E, hid, k, self.max_workgroups
            d.features, d.fc1_weight, d.fc1_bias, d.weights = native.ptr(self._rows), native.ptr(w1), native.ptr(b1), native.ptr(weights)
            d.workspace, d.workspace_bytes, d.result = native.ptr(ws), nbytes, native.ptr(result[off:])
            native.call('rovit_laplace_gram', ctypes.byref(d), native.stream_ptr())
        self._block = result.cpu().numpy()                        # the single device-to-host copy
        return self._block

    def _snapshot(self) -> Dict[str, torch.Tensor]:
        names = ('fc1_weight', 'fc1_bias', 'last_weight', 'last_bias')
        snap = {k: p.detach().float().clone().contiguous() for k, p in zip(names, _cls_params(self.cls_head))}
        if self._has_log_var:
            snap.update({k + '_mu': p.detach().float().clone().contiguous() for k, p in zip(names, _mu_params(self.unc_head))})
        return snap

    def _live_params(self):
        return _cls_params(self.cls_head) + (_mu_params(self.unc_head) if self.has_gaussian else [])

    def _version_key(self):
        return tuple((p.data_ptr(), p._version) for p in self._live_params())

    def fit(self, prior_precision='marglik') -> 'HeadLaplace':
        """Weights and Grams on the device, one copy, then on the host in fp64 the eigenvalues of H, tau (``prior_precision``: a positive
        number for both heads, or 'marglik'), the Cholesky factor and its inverse; the tables are uploaded as fp32 and the heads' fc1 and
        last-layer parameters are snapshotted.  Rows with a non-finite input are left out and counted; raises when none is left."""
        blk = self.result_block()
        lay = self._layout()
        C, K = self.num_classes, lay['K']
        g = gram_from_block(blk[lay['cls']:lay['mu']], self.hid, K)
        if g['n_valid'] < 1:
            raise RovitHipError(f"HeadLaplace.fit: no valid row among {g['n']} (bad_rows = {g['bad_rows']})")
        snap = self._snapshot()
        fc = fit_from_gram(g['gram'], C, np.concatenate([_np(snap['last_weight']).reshape(-1), _np(snap['last_bias']).reshape(-1)]), prior_precision)
        tables = dict(snap)
        tables['whitening'] = torch.from_numpy(fc['whitening64'].astype(np.float32))
        self.bad_logits, self.bad_log_var = int(blk[native.LAPLACE_BAD_LOGITS]), int(blk[native.LAPLACE_BAD_LOG_VAR])
        self.n_valid, self.bad_rows = g['n_valid'], g['bad_rows']
        self.prior_precision, self.status, self.log_marginal_likelihood = fc['prior_precision'], fc['status'], fc['log_marginal_likelihood']
        self.hessian_eigenvalues = fc['eigenvalues']
        if self._has_log_var:
            gm = gram_from_block(blk[lay['mu']:], self.hid_mu, 1)
            if gm['n_valid'] < 1:
                raise RovitHipError(f"HeadLaplace.fit: no valid row for the Gaussian head among {gm['n']} (bad_rows = {gm['bad_rows']})")
            fm = fit_from_gram(gm['gram'], 1, np.concatenate([_np(snap['last_weight_mu']).reshape(-1), _np(snap['last_bias_mu']).reshape(-1)]),
                               prior_precision)
            tables['whitening_mu'] = torch.from_numpy(fm['whitening64'].astype(np.float32))
            self.n_valid_mu, self.bad_rows_mu = gm['n_valid'], gm['bad_rows']
            self.prior_precision_mu, self.status_mu, self.log_marginal_likelihood_mu = fm['prior_precision'], fm['status'], fm['log_marginal_likelihood']
        self.tables = {k: v.contiguous().to(self.device) for k, v in tables.items()}
        self._tables_on = {}
        self._versions = self._version_key()
        return self

    # -- prediction --

    def _tables_for(self, device: torch.device) -> Dict[str, torch.Tensor]:
        if self.tables is None:
            raise RovitHipError('HeadLaplace.predict: fit() (or load_state_dict) first')
        if self._version_key() != self._versions:
            raise RovitHipError('HeadLaplace.predict: a head parameter has changed since fit(); the posterior tables are stale, fit again')
        if self.tables['whitening'].device == device:
            return self.tables
        if device not in self._tables_on:
            self._tables_on[device] = {k: v.to(device) for k, v in self.tables.items()}
        return self._tables_on[device]

    def _launch(self, x, t, suffix: str, hid: int, C: int, lg) -> Dict[str, torch.Tensor]:
        B = x.shape[0]
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
        out = {'logit_cov': f32(B, C, C), 'logit_var': f32(B, C)}
        if lg is not None:
            out['probs'], out['confidence_score'], out['mean_logit_var'] = f32(B, C), f32(B), f32(B)
        d = native.LaplaceQuery()
        d.batch, d.embed, d.hid, d.num_classes, d.max_workgroups = B, self.embed_dim, hid, C, self.max_workgroups
        d.features, d.cls_logits = native.ptr(x), native.ptr(lg)
        d.fc1_weight, d.fc1_bias, d.whitening = native.ptr(t['fc1_weight' + suffix]), native.ptr(t['fc1_bias' + suffix]), native.ptr(t['whitening' + suffix])
        for k, v in out.items():
            setattr(d, k, native.ptr(v))
        native.call('rovit_laplace_predict', ctypes.byref(d), native.stream_ptr())
        return out

    def predict(self, features: torch.Tensor, cls_logits: torch.Tensor, mu: Optional[torch.Tensor] = None,
                log_var: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Per row of (B, E) features with their (B, C) logits: ``logit_cov`` (B, C, C), ``logit_var`` (B, C), ``probs`` (B, C) (the
        probit-adjusted probabilities), ``confidence_score`` = 1 - max probs, ``mean_logit_var``; with a fitted Gaussian part ``mu_var``
        (B), the epistemic variance of mu, and with ``log_var`` also ``total_std`` = sqrt(exp(log_var) + mu_var).  Tensors on the
        features' device, one launch per head, nothing copied to the host.  ``mu`` is only checked for its shape."""
        x = features.detach()
        E, C = self.embed_dim, self.num_classes
        if x.dim() != 2 or x.shape[1] != E or x.shape[0] < 1:
            raise RovitHipError(f'HeadLaplace.predict: features must be (B >= 1, {E}), got {tuple(x.shape)}')
        B = x.shape[0]
        if cls_logits is None or tuple(cls_logits.shape) != (B, C) or cls_logits.device != x.device:
            raise RovitHipError(f'HeadLaplace.predict: cls_logits must be ({B}, {C}) on {x.device}, got '
                                f'{None if cls_logits is None else (tuple(cls_logits.shape), cls_logits.device)}')
        for name, v in (('mu', mu), ('log_var', log_var)):
            if v is not None and (v.numel() != B or v.device != x.device):
                raise RovitHipError(f'HeadLaplace.predict: {name} must hold {B} values on {x.device}, got {tuple(v.shape)} on {v.device}')
        t = self._tables_for(x.device)
        x = x.float().contiguous()
        lg = cls_logits.detach().float().contiguous()
        gaussian = 'whitening_mu' in t
        if not x.is_cuda:
            ref = predict_reference(x.numpy(), t['fc1_weight'], t['fc1_bias'], t['whitening'], C, lg.numpy())
            out = {k: torch.from_numpy(v.astype(np.float32)) for k, v in ref.items()}
            if gaussian:
                rm = predict_reference(x.numpy(), t['fc1_weight_mu'], t['fc1_bias_mu'], t['whitening_mu'], 1)
                out['mu_var'] = torch.from_numpy(rm['logit_var'].astype(np.float32)).reshape(-1)
        else:
            out = self._launch(x, t, '', self.hid, C, lg)
            if gaussian:
                out['mu_var'] = self._launch(x, t, '_mu', self.hid_mu, 1, None)['logit_var'].reshape(-1)
        if gaussian and log_var is not None:
            out['total_std'] = torch.sqrt(torch.exp(log_var.detach().float().reshape(-1)) + out['mu_var'])
        return out

    # -- state --

    def state_dict(self) -> Dict:
        """The fit as tensors and plain numbers (``torch.save`` takes it): the fp32 tables with the parameter snapshot, tau, status."""
        if self.tables is None:
            raise RovitHipError('HeadLaplace.state_dict: fit() first')
        sd = {'num_classes': self.num_classes, 'embed_dim': self.embed_dim, 'hid': self.hid, 'n': self.n, 'n_valid': self.n_valid,
              'bad_rows': self.bad_rows, 'bad_logits': self.bad_logits, 'bad_log_var': self.bad_log_var,
              'prior_precision': self.prior_precision, 'status': self.status, 'log_marginal_likelihood': self.log_marginal_likelihood,
              'prior_precision_mu': self.prior_precision_mu, 'status_mu': self.status_mu,
              'log_marginal_likelihood_mu': self.log_marginal_likelihood_mu, 'n_valid_mu': self.n_valid_mu, 'bad_rows_mu': self.bad_rows_mu}
        sd.update({f'tables.{k}': v.detach().cpu().clone() for k, v in self.tables.items()})
        return sd

    def load_state_dict(self, sd: Dict, device=None) -> 'HeadLaplace':
        """Restore a fit (not the recorded rows).  The heads this object was built on must hold the parameters the fit was made with:
        they are compared with the saved snapshot once, here."""
        if (sd['num_classes'], sd['embed_dim'], sd['hid']) != (self.num_classes, self.embed_dim, self.hid):
            raise RovitHipError(f"HeadLaplace.load_state_dict: the state is for {sd['num_classes']} classes, {sd['embed_dim']} features and "
                                f"{sd['hid']} hidden units, this object for {self.num_classes}, {self.embed_dim} and {self.hid}")
        tables = {k[len('tables.'):]: v.to(torch.float32).contiguous() for k, v in sd.items() if k.startswith('tables.')}
        if 'whitening_mu' in tables and self.unc_head is None:
            raise RovitHipError('HeadLaplace.load_state_dict: the state has a Gaussian part, this object no uncertainty head')
        names = ('fc1_weight', 'fc1_bias', 'last_weight', 'last_bias')
        live = list(zip(names, _cls_params(self.cls_head)))
        if 'whitening_mu' in tables:
            live += [(k + '_mu', p) for k, p in zip(names, _mu_params(self.unc_head))]
        for k, p in live:
            if tuple(p.shape) != tuple(tables[k].shape) or not torch.equal(p.detach().float().cpu(), tables[k]):
                raise RovitHipError(f"HeadLaplace.load_state_dict: the heads' {k} differs from the one the fit was made with")
        self.reset()
        self._has_log_var = 'whitening_mu' in tables
        for k in ('n', 'n_valid', 'bad_rows', 'bad_logits', 'bad_log_var', 'n_valid_mu', 'bad_rows_mu'):
            setattr(self, k, int(sd[k]))
        for k in ('prior_precision', 'log_marginal_likelihood', 'prior_precision_mu', 'log_marginal_likelihood_mu'):
            setattr(self, k, None if sd[k] is None else float(sd[k]))
        self.status, self.status_mu = sd['status'], sd['status_mu']
        self.tables = {k: v.to(device or 'cpu') for k, v in tables.items()}
        self._versions = self._version_key()
        return self


def fit_model_laplace(model, x_or_loader, prior_precision='marglik', chunk: int = 256, capacity: int = 4096) -> HeadLaplace:
    """``HeadLaplace`` of the model's own heads over images in eval mode under no_grad, ``chunk`` images at a time: an image tensor, or an
    iterable of batches whose first element is the images (host batches of a loader are copied to the model's device).  The Gaussian
    part is fitted when the model returns ``log_var`` (curriculum stage >= 3)."""
    if not (isinstance(chunk, int) and chunk >= 1):
        raise RovitHipError(f'fit_laplace: chunk must be a positive integer, got {chunk!r}')
    is_tensor = isinstance(x_or_loader, torch.Tensor)
    dev = next(model.parameters()).device
    la = HeadLaplace(model, capacity)
    batches = [(x_or_loader,)] if is_tensor else x_or_loader
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for batch in batches:
                images = batch[0] if isinstance(batch, (tuple, list)) else batch
                if is_tensor:
                    native.ptr(images)                              # a CPU tensor raises: the backbone has no CPU path
                else:
                    images = images.to(dev, non_blocking=True)
                for r0 in range(0, images.shape[0], chunk):
                    out = model(images[r0:r0 + chunk])
                    la.update(out['features'], out['cls_logits'], out.get('log_var'))
    finally:
        model.train(was_training)
    return la.fit(prior_precision)
