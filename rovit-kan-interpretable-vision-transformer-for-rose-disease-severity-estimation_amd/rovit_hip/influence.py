"""Training-data influence through the last layer of the heads: proponents, opponents and a label audit.

``nearest_examples`` names the training images that look alike in feature space.  It does not name the ones whose removal would change
this output (Koh & Liang, ICML 2017; Pruthi et al., NeurIPS 2020), nor does anything else here look at the training labels.  Everything
needed exists after ``HeadLaplace.fit``: the whitening table W = R^-1 of the posterior precision H + tau I = R R^T, for both heads, with
tau chosen by the evidence.  The reference has none of it ("parity unpinned": every rule below is this repository's own statement).

Definitions (notation of ``rovit_hip/laplace.py``: a_i = [relu(fc1 f_i + b1); 1], D = hid + 1 wide, padded to P = hid + 32 with exact
zeros; parameters class-major, index c P + a; W the fp32 table ``tables['whitening']`` / ``tables['whitening_mu']`` AS GIVEN):
  residual r (fp64, rounded to fp32 once)
    head 'cls', target 'loss'    r = softmax(l) - e_y, the cross-entropy gradient with respect to the logits; y the given label, or for
                                 a query without labels the first argmax of l ("the loss of the prediction made")
    head 'cls', target 'logit'   r = e_c, c given or the first argmax
    head 'mu',  target 'loss'    r = (mu - sev_true) exp(-log_var): the Gaussian NLL with fc_logvar held fixed, as ``HeadLaplace`` holds it
    head 'mu',  target 'mu'      r = 1
  whitened gradient  u = W g, g[c P + a] = r_c a_a, N = C P long; the padding's entries are exactly 0
  score              s(t, j) = u_t . u_j = g_t^T (H + tau I)^-1 g_j
  self-influence     |u_j|^2
  relative=True      s(t, j) / |u_j| (RelatIF, Barshan et al., AISTATS 2020): high-norm outliers stop being every query's top hit
Sign and scale: to first order, removing training row j changes the query's target (its loss, logit or mu) by + s(t, j).  For target
'loss' a PROPONENT has s > 0 (removing it raises the query's loss), an OPPONENT s < 0.  H is a sum over rows, not a mean, so the scale
means something: for a ridge problem at its exact minimiser with log_var = 0, s(t, j) / (1 - h_j), h_j = a_j^T (H + tau I)^-1 a_j, is the
exact leave-one-out change of mu_t (tests/test_influence_cpu.py).
Validity: a recorded row is never returned, and is counted, when a feature or logit is non-finite (``bad_rows``; for 'mu' also a
non-finite mu, log_var or severity, or an exp(-log_var) that is not finite in fp32), when its class label is outside [0, C)
(``bad_labels``), or when its stored row is all zeros; under ``relative`` also when its norm is 0.  A bad query row returns index -1 and
NaN scores in every slot.
Order: proponents by (score descending, index ascending), opponents by (score ascending, index ascending); the fp32 scores are compared
with -0 made +0, and only integer compares on (orderable score bits, index) decide membership.  The two lists are independent and may
overlap when fewer than 2 k valid rows exist; empty slots hold -1 / NaN.  ``exclude`` (B,) removes one index per query.

``HeadInfluence.update`` embeds a batch straight into the index at an offset the host knows (``rovit_influence_embed``, csrc/influence.hip,
one launch per head, no synchronisation); ``search`` is one embed launch for the queries and ``rovit_influence_search`` (no (B, n) matrix
exists; both ends in one pass); ``counts`` is the one device-to-host copy.  Every output is bit-identical from run to run, for every
``max_workgroups`` / ``max_splits`` and for every split of the rows into ``update`` calls.  On CPU tensors the same entry points run the
numpy fp64 statements below (``residual_reference``, ``embed_reference``, ``search_reference``; ``influence_reference`` is the brute force
with an explicit inverse), the kernels' oracle, as every other accumulator here does.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from . import native
from .laplace import HeadLaplace, _np, augmented_hidden
from .native import RovitHipError

HEADS = {'cls': native.INFLUENCE_CLS, 'mu': native.INFLUENCE_MU}
TARGETS = {'cls': {'loss': native.INFLUENCE_LOSS, 'logit': native.INFLUENCE_OUTPUT},
           'mu': {'loss': native.INFLUENCE_LOSS, 'mu': native.INFLUENCE_OUTPUT}}
OK, BAD_ROW, BAD_LABEL, ZERO_ROW = 0, 1, 2, 4          # a row's status (csrc/influence.hip)


def check_target(head: str, target: str) -> int:
    if head not in HEADS:
        raise RovitHipError(f"influence: head must be 'cls' or 'mu', got {head!r}")
    if target not in TARGETS[head]:
        raise RovitHipError(f"influence: the target of head {head!r} must be one of {sorted(TARGETS[head])}, got {target!r}")
    return TARGETS[head][target]


def check_k(k) -> None:
    if not (isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= native.INFLUENCE_MAX_K):
        raise RovitHipError(f'influence: k must be an integer in 1..{native.INFLUENCE_MAX_K}, got {k!r}')


# ---- host statements (fp64) ----------------------------------------------------------------------------------------------------------

def _f64(v) -> np.ndarray:
    """fp64 from the fp32 value of an input; an array that already is fp64 is taken as given (the brute-force tests stay in fp64)."""
    a = _np(v)
    return a if a.dtype == np.float64 else a.astype(np.float32).astype(np.float64)


def residual_reference(head: str, target: str, n: int, cls_logits=None, labels=None, mu=None, log_var=None, severity=None,
                       dtype=np.float32) -> Dict:
    """``residual`` (n, C) fp32 (fp64, rounded once; NaN for a row whose inputs are bad) and ``status`` (n): 0 good, 1 a non-finite input
    or a residual that is not finite in fp32, 2 a label outside [0, C).  The features are not looked at here.  ``dtype=np.float64`` keeps
    the residual unrounded (the same rows are bad)."""
    check_target(head, target)
    status = np.zeros(n, dtype=np.int64)
    with np.errstate(all='ignore'):
        if head == 'cls':
            l = _f64(cls_logits)
            C = l.shape[1]
            fin = np.isfinite(l).all(axis=1)
            ls = np.where(fin[:, None], l, 0.0)
            y = ls.argmax(axis=1) if labels is None else _np(labels).astype(np.int64).reshape(-1)
            status[~fin] = BAD_ROW
            status[fin & ((y < 0) | (y >= C))] = BAD_LABEL
            onehot = np.zeros((n, C))
            good = status == OK
            onehot[np.nonzero(good)[0], y[good]] = 1.0
            if target == 'loss':
                e = np.exp(ls - ls.max(axis=1, keepdims=True))
                s = np.zeros(n)
                for c in range(C):
                    s = s + e[:, c]
                r = e / s[:, None] - onehot
            else:
                r = onehot
        else:
            if target == 'loss':
                m, v, t = (_f64(z).reshape(-1) for z in (mu, log_var, severity))
                w = np.exp(-v)
                r = ((m - t) * w)[:, None]
                fin = np.isfinite(m) & np.isfinite(v) & np.isfinite(t) & np.isfinite(w.astype(np.float32)) & np.isfinite(r[:, 0].astype(np.float32))
                status[~fin] = BAD_ROW
            else:
                r = np.ones((n, 1))
        r32 = r.astype(dtype)
    r32[status != OK] = np.nan
    return {'residual': r32, 'status': status}


def embed_reference(features, fc1_weight, fc1_bias, whitening, num_classes: int, head: str = 'cls', target: str = 'loss', cls_logits=None,
                    labels=None, mu=None, log_var=None, severity=None, dtype=np.float32) -> Dict:
    """``rovit_influence_embed`` in numpy fp64 from the fp32 inputs and the whitening table as given: ``rows`` (n, N) fp64 (zeros for an
    invalid row), ``residual`` (n, C) fp32, ``norm2`` (n) fp64 = |u|^2 (0 for an invalid row), ``valid`` (n) bool, ``status`` and the counts
    ``n``, ``n_valid``, ``bad_rows``, ``bad_labels``.  ``dtype=np.float64`` keeps the residual unrounded."""
    x = _np(features, np.float32)
    W = np.asarray(_np(whitening), dtype=np.float64)
    C, n = num_classes, x.shape[0]
    res = residual_reference(head, target, n, cls_logits, labels, mu, log_var, severity, dtype)
    status = res['status'].copy()
    status[~np.isfinite(x).all(axis=1)] = BAD_ROW                  # a row that is both counts as a bad row
    a = augmented_hidden(np.where(np.isfinite(x), x, 0.0), fc1_weight, fc1_bias)
    D, P = a.shape[1], W.shape[0] // C
    if W.shape != (C * P, C * P) or P != D + 31 or res['residual'].shape[1] != C:
        raise RovitHipError(f'influence embed: the whitening table must be ({C * (D + 31)}, {C * (D + 31)}) for {C} outputs, got {W.shape}')
    good = status == OK
    r = np.where(good[:, None], res['residual'].astype(np.float64), 0.0)
    g = np.zeros((n, C, P))
    g[:, :, :D] = r[:, :, None] * np.where(good[:, None], a, 0.0)[:, None, :]
    with np.errstate(all='ignore'):
        u = g.reshape(n, C * P) @ W.T
        norm2 = (u * u).sum(axis=1)
        status[good & ~np.isfinite(norm2.astype(np.float32))] = BAD_ROW
    status[(status == OK) & ~(u != 0.0).any(axis=1)] = ZERO_ROW
    valid = status == OK
    u[~valid] = 0.0
    norm2[~valid] = 0.0
    residual = res['residual'].copy()
    residual[(status == BAD_ROW) | (status == BAD_LABEL)] = np.nan
    return {'rows': u, 'residual': residual, 'norm2': norm2, 'valid': valid, 'status': status, 'n': int(n), 'n_valid': int(valid.sum()),
            'bad_rows': int((status == BAD_ROW).sum()), 'bad_labels': int((status == BAD_LABEL).sum())}


def search_reference(queries, rows, norm2, valid, k: int = 10, relative: bool = False, exclude=None, query_valid=None, labels=None,
                     severity=None, chunk: int = 512) -> Dict[str, np.ndarray]:
    """``rovit_influence_search`` in numpy: fp64 scores from the fp32 rows (fp64 arrays are taken as given), s = q . r (divided by sqrt(norm2) under ``relative``), the
    candidates ordered by (score descending, index ascending) for ``pro_*`` and (score ascending, index ascending) for ``opp_*`` (stable
    sorts), ``*_indices`` int64 with -1 and ``*_scores`` NaN in the empty slots, ``*_labels`` (-1) and ``*_severities`` (NaN) when the
    columns are given."""
    check_k(k)
    q32, r32 = _f64(queries), _f64(rows)
    if q32.ndim != 2 or r32.ndim != 2 or q32.shape[1] != r32.shape[1] or q32.shape[0] < 1 or r32.shape[0] < 1:
        raise RovitHipError(f'search_reference: queries (B >= 1, N) and rows (n >= 1, N), got {q32.shape} and {r32.shape}')
    B, n = q32.shape[0], r32.shape[0]
    nrm = _f64(norm2).reshape(-1)
    ok = _np(valid).reshape(-1) != 0
    if relative:
        ok = ok & (nrm > 0.0)
    qok = np.ones(B, dtype=bool) if query_valid is None else _np(query_valid).reshape(-1) != 0
    ex = None if exclude is None else _np(exclude).astype(np.int64).reshape(-1)
    if ex is not None and ex.shape[0] != B:
        raise RovitHipError(f'search_reference: exclude must hold {B} indices, got {ex.shape[0]}')
    r64 = np.where(ok[:, None], r32, 0.0)
    div = np.sqrt(np.where(ok, nrm, 1.0)) if relative else None
    out = {'pro_scores': np.full((B, k), np.nan), 'pro_indices': np.full((B, k), -1, dtype=np.int64),
           'opp_scores': np.full((B, k), np.nan), 'opp_indices': np.full((B, k), -1, dtype=np.int64)}
    for r0 in range(0, B, chunk):
        qq = np.where(qok[r0:r0 + chunk, None], q32[r0:r0 + chunk], 0.0)
        with np.errstate(all='ignore'):
            s = qq @ r64.T
            if relative:
                s = s / div[None]
            s = s + 0.0
        cand = np.isfinite(s) & ok[None] & qok[r0:r0 + chunk, None]
        if ex is not None:
            e = ex[r0:r0 + chunk]
            hit = np.nonzero((e >= 0) & (e < n))[0]
            cand[hit, e[hit]] = False
        for name, key in (('pro', np.where(cand, -s, np.inf)), ('opp', np.where(cand, s, np.inf))):
            order = np.argsort(key, axis=1, kind='stable')[:, :k]
            real = np.take_along_axis(cand, order, axis=1)
            kk = order.shape[1]
            out[name + '_scores'][r0:r0 + chunk, :kk] = np.where(real, np.take_along_axis(s, order, axis=1), np.nan)
            out[name + '_indices'][r0:r0 + chunk, :kk] = np.where(real, order, -1)
    for name in ('pro', 'opp'):
        idx = out[name + '_indices']
        safe = np.maximum(idx, 0)
        if labels is not None:
            out[name + '_labels'] = np.where(idx >= 0, _np(labels).astype(np.int64).reshape(-1)[safe], -1)
        if severity is not None:
            out[name + '_severities'] = np.where(idx >= 0, _np(severity).astype(np.float32).reshape(-1).astype(np.float64)[safe], np.nan)
    return out


def influence_reference(a_query, a_train, theta, hessian, tau: float, head: str = 'cls', target: str = 'loss', out_query=None, out_train=None,
                        labels_query=None, labels_train=None, log_var_query=None, log_var_train=None, severity_query=None,
                        severity_train=None) -> np.ndarray:
    """The brute force, (B, n): g_t^T (H + tau I)^-1 g_j with an EXPLICIT inverse and autograd gradients with respect to theta =
    [weight, bias] (C, D), flattened class-major.  ``a_*`` are the augmented hidden rows (fp64); ``out_*`` the outputs as recorded (the
    logits (., C), or mu (.)): the value of the output is pinned to them while its dependence on theta stays the last layer's.  A training
    row's gradient is that of its loss (cross-entropy of ``labels_train``, or the Gaussian NLL with ``log_var_train`` held fixed); the
    query's is that of its loss, or of the logit ``labels_query`` / of mu for the targets 'logit' / 'mu'."""
    check_target(head, target)
    th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)

    def grads(a, out, y, lv, sv, tgt):
        rows = []
        a = torch.from_numpy(np.asarray(a, dtype=np.float64))
        for i in range(a.shape[0]):
            z = th @ a[i]
            z = z + (torch.from_numpy(np.asarray(out[i], dtype=np.float64).reshape(-1)) - z).detach()
            if head == 'cls':
                f = torch.nn.functional.cross_entropy(z[None], torch.tensor([int(y[i])])) if tgt == 'loss' else z[int(y[i])]
            else:
                f = 0.5 * torch.exp(-torch.tensor(float(lv[i]), dtype=torch.float64)) * (z[0] - float(sv[i])) ** 2 if tgt == 'loss' else z[0]
            rows.append(torch.autograd.grad(f, th)[0].reshape(-1).numpy().copy())
        return np.stack(rows)

    gq = grads(a_query, out_query, labels_query, log_var_query, severity_query, target)
    gt = grads(a_train, out_train, labels_train, log_var_train, severity_train, 'loss')
    H = np.asarray(hessian, dtype=np.float64)
    return gq @ np.linalg.inv(H + float(tau) * np.eye(H.shape[0])) @ gt.T


_OUT_DTYPES = {'pro_indices': np.int32, 'opp_indices': np.int32, 'pro_labels': np.int32, 'opp_labels': np.int32}


# ---- the index -------------------------------------------------------------------------------------------------------------------------

class HeadInfluence:
    """The whitened last-layer gradients of recorded training rows and the signed top-k search over them; see the module docstring.
    Built on a fitted ``HeadLaplace`` (its ``_tables_for`` is read at every call, so the stale-parameter refusal is inherited).  ``update``
    never synchronises; ``counts`` is the one device-to-host copy; ``search`` copies nothing.  There is no ``state_dict``: the index is
    rebuilt from a loader in one pass (``fit_model_influence``).  Memory: n N 4 bytes per head, N = C (hid + 32): 10 MB at 4 096 rows and
    168 MB at 65 536 for the default heads."""

    def __init__(self, laplace: HeadLaplace, capacity: int = 4096):
        if not isinstance(laplace, HeadLaplace):
            raise RovitHipError(f'HeadInfluence: a fitted HeadLaplace is needed, got {type(laplace).__name__}')
        if not laplace.fitted:
            raise RovitHipError('HeadInfluence: the HeadLaplace is not fitted; fit() (or load_state_dict) first')
        if not (isinstance(capacity, int) and 1 <= capacity <= native.KAN_STATS_MAX_ROWS):
            raise RovitHipError(f'HeadInfluence: capacity must be in 1..{native.KAN_STATS_MAX_ROWS}, got {capacity!r}')
        self.laplace, self._capacity0 = laplace, capacity
        self.embed_dim, self.num_classes = laplace.embed_dim, laplace.num_classes
        self.max_workgroups = 0                                    # > 0 caps every grid (tests); the results do not depend on it
        self.max_splits = 0                                        # > 0 caps the reference splits of a search (tests); likewise
        self.reset()

    def reset(self) -> None:
        self.n = 0
        self.device: Optional[torch.device] = None
        self.has_mu: Optional[bool] = None                         # fixed by the first update
        self._cap = 0
        self._store: Dict[str, torch.Tensor] = {}
        self._counts_dev: Optional[torch.Tensor] = None
        self._counts: Optional[Dict[str, int]] = None

    def _geometry(self, head: str):
        """(suffix of the Laplace tables, hidden width, outputs) of a head."""
        if head not in HEADS:
            raise RovitHipError(f"HeadInfluence: head must be 'cls' or 'mu', got {head!r}")
        if head == 'mu':
            if not self.laplace.has_gaussian:
                raise RovitHipError("HeadInfluence: head 'mu' needs a Laplace fit with a Gaussian part (log_var recorded, stage >= 3)")
            return '_mu', self.laplace.hid_mu, 1
        return '', self.laplace.hid, self.num_classes

    def dim(self, head: str = 'cls') -> int:
        _, hid, C = self._geometry(head)
        return C * (hid + 32)

    def _columns(self):
        cols = {'labels': ((), torch.int32), 'logits': ((self.num_classes,), torch.float32), 'rows': ((self.dim('cls'),), torch.float32),
                'residual': ((self.num_classes,), torch.float32), 'norm2': ((), torch.float32), 'valid': ((), torch.int32)}
        if self.has_mu:
            cols.update({'severity': ((), torch.float32), 'mu': ((), torch.float32), 'log_var': ((), torch.float32),
                         'rows_mu': ((self.dim('mu'),), torch.float32), 'residual_mu': ((1,), torch.float32), 'norm2_mu': ((), torch.float32),
                         'valid_mu': ((), torch.int32)})
        return cols

    def _reserve(self, rows: int) -> None:
        if rows <= self._cap:
            return
        if rows > native.KAN_STATS_MAX_ROWS:
            raise RovitHipError(f'HeadInfluence: {rows} rows exceed the limit of {native.KAN_STATS_MAX_ROWS}')
        new_cap = min(native.KAN_STATS_MAX_ROWS, max(rows, 2 * self._cap, self._capacity0))
        grown = {}
        for name, (shape, dtype) in self._columns().items():
            grown[name] = torch.empty((new_cap,) + shape, dtype=dtype, device=self.device)
            if name in self._store:
                grown[name][:self.n].copy_(self._store[name][:self.n])          # stream-ordered: no synchronisation
        self._store, self._cap = grown, new_cap

    def _embed(self, head: str, target: int, target_name: str, x, lg, y, mu, lv, sv, rows, residual, norm2, valid, counts) -> None:
        """One head's embed of a batch into the given (slices of) tensors; ``counts`` (4,) int64 is added to."""
        suffix, hid, C = self._geometry(head)
        t = self.laplace._tables_for(x.device)
        if not x.is_cuda:
            ref = embed_reference(x.numpy(), t['fc1_weight' + suffix], t['fc1_bias' + suffix], t['whitening' + suffix], C, head, target_name,
                                  None if lg is None else lg.numpy(), None if y is None else y.numpy(), None if mu is None else mu.numpy(),
                                  None if lv is None else lv.numpy(), None if sv is None else sv.numpy())
            rows.copy_(torch.from_numpy(ref['rows'].astype(np.float32)))
            residual.copy_(torch.from_numpy(ref['residual']))
            with np.errstate(all='ignore'):
                stored = ref['rows'].astype(np.float32).astype(np.float64)
                norm2.copy_(torch.from_numpy((stored * stored).sum(axis=1).astype(np.float32)))
            valid.copy_(torch.from_numpy(ref['valid'].astype(np.int32)))
            counts += torch.tensor([ref['n'], ref['n_valid'], ref['bad_rows'], ref['bad_labels']], dtype=torch.int64)
            return
        d = native.InfluenceRows()
        d.n, d.embed, d.hid, d.num_classes, d.head, d.target, d.max_workgroups = x.shape[0], self.embed_dim, hid, C, HEADS[head], target, self.max_workgroups
        d.features, d.cls_logits, d.labels = native.ptr(x), native.ptr(lg) if head == 'cls' else None, native.ptr(y) if head == 'cls' else None
        d.fc1_weight, d.fc1_bias, d.whitening = (native.ptr(t[k + suffix]) for k in ('fc1_weight', 'fc1_bias', 'whitening'))
        if head == 'mu' and target == native.INFLUENCE_LOSS:
            d.mu, d.log_var, d.severity = native.ptr(mu), native.ptr(lv), native.ptr(sv)
        d.rows, d.residual, d.norm2, d.valid, d.counts = (native.ptr(v) for v in (rows, residual, norm2, valid, counts))
        native.call('rovit_influence_embed', ctypes.byref(d), native.stream_ptr())

    @staticmethod
    def _column(v, B: int, dev, name: str, who: str, integer: bool = False):
        if v is None:
            return None
        v = v.detach().reshape(-1)
        if v.shape[0] != B or v.device != dev or (integer and (v.is_floating_point() or v.dtype == torch.bool)):
            raise RovitHipError(f"HeadInfluence.{who}: {name} must hold {B} {'integers' if integer else 'values'} on {dev}, got "
                                f'{tuple(v.shape)} of {v.dtype} on {v.device}')
        return v.to(torch.int32).contiguous() if integer else v.float().contiguous()

    def _check_batch(self, features, cls_logits, who: str):
        x = features.detach()
        E, C = self.embed_dim, self.num_classes
        if x.dim() != 2 or x.shape[1] != E or x.shape[0] < 1:
            raise RovitHipError(f'HeadInfluence.{who}: features must be (B >= 1, {E}), got {tuple(x.shape)}')
        if cls_logits is None or tuple(cls_logits.shape) != (x.shape[0], C) or cls_logits.device != x.device:
            raise RovitHipError(f'HeadInfluence.{who}: cls_logits must be ({x.shape[0]}, {C}) on {x.device}, got '
                                f'{None if cls_logits is None else (tuple(cls_logits.shape), cls_logits.device)}')
        return x.float().contiguous(), cls_logits.detach().float().contiguous()

    def update(self, features: torch.Tensor, cls_logits: torch.Tensor, class_labels: torch.Tensor, mu: Optional[torch.Tensor] = None,
               log_var: Optional[torch.Tensor] = None, severity: Optional[torch.Tensor] = None) -> None:
        """Record a batch: (B, E) feature rows, their (B, C) logits and (B,) integer class labels, embedded at once for the loss of the
        classification head; with ``mu``, ``log_var`` and ``severity`` (all three, (B,) or (B, 1)) and a Laplace fit with a Gaussian part
        also for the Gaussian NLL of the ``mu`` layer.  The first batch decides whether the 'mu' head is kept."""
        x, lg = self._check_batch(features, cls_logits, 'update')
        B, dev = x.shape[0], x.device
        if class_labels is None:
            raise RovitHipError('HeadInfluence.update: the class labels are needed (the gradient of the loss of a training row)')
        y = self._column(class_labels, B, dev, 'class_labels', 'update', integer=True)
        given = [v is not None for v in (mu, log_var, severity)]
        if any(given) and not all(given):
            raise RovitHipError("HeadInfluence.update: the 'mu' head needs mu, log_var and severity together; "
                                f"missing: {[k for k, g in zip(('mu', 'log_var', 'severity'), given) if not g]}")
        with_mu = all(given) and self.laplace.has_gaussian
        m, lv, sv = (self._column(v, B, dev, k, 'update') for k, v in (('mu', mu), ('log_var', log_var), ('severity', severity)))
        if self.device is None:
            self.device, self.has_mu = dev, with_mu
            self._counts_dev = torch.zeros((2, native.INFLUENCE_COUNT_WORDS), dtype=torch.int64, device=dev)
        elif dev != self.device:
            raise RovitHipError(f'HeadInfluence.update: batch on {dev}, earlier batches on {self.device}; reset() first')
        if with_mu != self.has_mu:
            raise RovitHipError(f"HeadInfluence.update: every batch carries the columns of the first one ('mu' head: {self.has_mu})")
        self.laplace._tables_for(dev)                              # unfitted or stale: refused before anything is stored
        self._reserve(self.n + B)
        st, lo, hi = self._store, self.n, self.n + B
        st['labels'][lo:hi].copy_(y)
        st['logits'][lo:hi].copy_(lg)
        self._embed('cls', native.INFLUENCE_LOSS, 'loss', x, lg, y, None, None, None, st['rows'][lo:hi], st['residual'][lo:hi],
                    st['norm2'][lo:hi], st['valid'][lo:hi], self._counts_dev[0])
        if with_mu:
            for name, v in (('mu', m), ('log_var', lv), ('severity', sv)):
                st[name][lo:hi].copy_(v)
            self._embed('mu', native.INFLUENCE_LOSS, 'loss', x, None, None, m, lv, sv, st['rows_mu'][lo:hi], st['residual_mu'][lo:hi],
                        st['norm2_mu'][lo:hi], st['valid_mu'][lo:hi], self._counts_dev[1])
        self.n = hi
        self._counts = None

    def _need_rows(self) -> None:
        if self.n < 1:
            raise RovitHipError('HeadInfluence: nothing recorded yet')

    def counts(self) -> Dict[str, int]:
        """``n``, ``n_valid``, ``bad_rows`` and ``bad_labels`` of the classification head's rows and, with the 'mu' head, ``n_valid_mu`` and
        ``bad_rows_mu``: the one device-to-host copy (kept until the next ``update``).  n - n_valid - bad_rows - bad_labels rows are
        all zeros."""
        self._need_rows()
        if self._counts is None:
            w = self._counts_dev.cpu().numpy()                     # the single device-to-host copy
            N, V, R, L = native.INFLUENCE_N, native.INFLUENCE_N_VALID, native.INFLUENCE_BAD_ROWS, native.INFLUENCE_BAD_LABELS
            self._counts = {'n': int(w[0, N]), 'n_valid': int(w[0, V]), 'bad_rows': int(w[0, R]), 'bad_labels': int(w[0, L])}
            if self.has_mu:
                self._counts.update({'n_valid_mu': int(w[1, V]), 'bad_rows_mu': int(w[1, R])})
        return self._counts

    def _head_store(self, head: str):
        self._geometry(head)
        self._need_rows()
        if head == 'mu' and not self.has_mu:
            raise RovitHipError("HeadInfluence: the 'mu' head was not recorded (update() needs mu, log_var and severity)")
        sfx = '_mu' if head == 'mu' else ''
        return tuple(self._store[k + sfx][:self.n] for k in ('rows', 'residual', 'norm2', 'valid'))

    def rows(self, head: str = 'cls') -> torch.Tensor:
        """The recorded (n, N) whitened gradients of a head, a view."""
        return self._head_store(head)[0]

    def self_influence(self, head: str = 'cls') -> torch.Tensor:
        """|u_j|^2 of every recorded row, (n,) on the device; NaN for an invalid row."""
        _, _, norm2, valid = self._head_store(head)
        return torch.where(valid != 0, norm2, torch.full_like(norm2, float('nan')))

    def search(self, features: torch.Tensor, cls_logits: torch.Tensor, labels: Optional[torch.Tensor] = None, mu: Optional[torch.Tensor] = None,
               log_var: Optional[torch.Tensor] = None, severity: Optional[torch.Tensor] = None, head: str = 'cls', target: str = 'loss',
               class_index=None, k: int = 10, relative: bool = False, exclude: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Proponents and opponents of every row of (B, E) ``features``: ``pro_scores`` / ``opp_scores`` (B, k) fp32, ``pro_indices`` /
        ``opp_indices`` (B, k) int32, ``pro_labels`` / ``opp_labels`` (B, k) int32 and, with the 'mu' head recorded, ``pro_severities`` /
        ``opp_severities`` (B, k) fp32 of the rows found; ``query_self_influence`` (B,) (NaN for a bad query) and the queries' ``residual``
        (B, C).  Head 'cls': target 'loss' (the cross-entropy of ``labels``, or of the prediction made) or 'logit' (of ``class_index``,
        an integer or (B,) integers, or the first argmax).  Head 'mu': target 'loss' (needs ``mu``, ``log_var`` and ``severity``) or 'mu'.
        Tensors on the features' device; nothing is copied to the host."""
        tcode = check_target(head, target)
        check_k(k)
        x, lg = self._check_batch(features, cls_logits, 'search')
        B, dev = x.shape[0], x.device
        rows, _, norm2, valid = self._head_store(head)
        if dev != self.device:
            raise RovitHipError(f'HeadInfluence.search: features on {dev}, the index on {self.device}')
        _, _, C = self._geometry(head)
        y = m = lv = sv = None
        if head == 'cls':
            if target == 'logit' and class_index is not None:
                labels = torch.full((B,), class_index, dtype=torch.int32, device=dev) if isinstance(class_index, int) else class_index
            elif target == 'logit':
                labels = None
            y = self._column(labels, B, dev, 'labels' if target == 'loss' else 'class_index', 'search', integer=True)
        elif target == 'loss':
            if mu is None or log_var is None or severity is None:
                raise RovitHipError("HeadInfluence.search: the loss of the 'mu' head needs mu, log_var and severity")
            m, lv, sv = (self._column(v, B, dev, name, 'search') for name, v in (('mu', mu), ('log_var', log_var), ('severity', severity)))
        ex = None
        if exclude is not None:
            if exclude.dim() != 1 or exclude.shape[0] != B or exclude.is_floating_point() or exclude.dtype == torch.bool:
                raise RovitHipError(f'HeadInfluence.search: exclude must be ({B},) integers, got {tuple(exclude.shape)} of {exclude.dtype}')
            ex = exclude.detach().to(device=dev, dtype=torch.int32).contiguous()
        N = rows.shape[1]
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        q, res, qn, qv = f32(B, N), f32(B, C), f32(B), i32(B)
        self._embed(head, tcode, target, x, lg, y, m, lv, sv, q, res, qn, qv, torch.zeros(native.INFLUENCE_COUNT_WORDS, dtype=torch.int64, device=dev))
        ref_labels = self._store['labels'][:self.n]
        ref_sev = self._store['severity'][:self.n] if self.has_mu else None
        if not x.is_cuda:
            ref = search_reference(q.numpy(), rows.numpy(), norm2.numpy(), valid.numpy(), k, relative, None if ex is None else ex.numpy(),
                                   qv.numpy(), ref_labels.numpy(), None if ref_sev is None else ref_sev.numpy())
            out = {name: torch.from_numpy(np.ascontiguousarray(v.astype(_OUT_DTYPES.get(name, np.float32)))) for name, v in ref.items()}
        else:
            out = {'pro_scores': f32(B, k), 'pro_indices': i32(B, k), 'opp_scores': f32(B, k), 'opp_indices': i32(B, k),
                   'pro_labels': i32(B, k), 'opp_labels': i32(B, k)}
            if ref_sev is not None:
                out['pro_severities'], out['opp_severities'] = f32(B, k), f32(B, k)
            lib = native.load()
            nbytes = lib.rovit_influence_workspace_bytes(B, self.n, N, k)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            d = native.InfluenceQuery()
            d.batch, d.n, d.dim, d.k, d.relative, d.max_workgroups, d.max_splits = B, self.n, N, k, int(bool(relative)), self.max_workgroups, self.max_splits
            d.queries, d.query_valid, d.rows, d.norm2, d.valid, d.exclude = (native.ptr(v) for v in (q, qv, rows, norm2, valid, ex))
            d.ref_labels, d.ref_severity = native.ptr(ref_labels), native.ptr(ref_sev)
            d.workspace, d.workspace_bytes = native.ptr(ws), nbytes
            for name, v in out.items():
                setattr(d, name, native.ptr(v))
            native.call('rovit_influence_search', ctypes.byref(d), native.stream_ptr())
        out['query_self_influence'] = torch.where(qv != 0, qn, torch.full_like(qn, float('nan')))
        out['residual'] = res
        return out

    def label_audit(self, top: int = 50, head: str = 'cls') -> Dict[str, torch.Tensor]:
        """The ``top`` valid recorded rows by self-influence, the standard audit score for label noise, found with ``torch.topk`` on the
        device: ``indices`` (int64, -1 in a slot beyond the valid rows), ``scores``, the given ``labels``, the ``predicted`` class and
        ``label_prob``, the probability of the given label (head 'mu': ``severity``, ``mu`` and ``log_var`` instead).  Nothing is copied
        to the host."""
        if not (isinstance(top, int) and top >= 1):
            raise RovitHipError(f'HeadInfluence.label_audit: top must be a positive integer, got {top!r}')
        s = self.self_influence(head)
        real = ~torch.isnan(s)
        score, idx = torch.topk(torch.where(real, s, torch.full_like(s, -1.0)), min(top, self.n))
        ok = score >= 0
        nan = torch.full_like(score, float('nan'))
        out = {'indices': torch.where(ok, idx, torch.full_like(idx, -1)), 'scores': torch.where(ok, score, nan)}
        if head == 'cls':
            y = self._store['labels'][:self.n][idx].long()
            p = torch.softmax(self._store['logits'][:self.n][idx].double(), dim=1)
            out['labels'] = torch.where(ok, y, torch.full_like(y, -1))
            out['predicted'] = torch.where(ok, p.argmax(dim=1), torch.full_like(y, -1))
            out['label_prob'] = torch.where(ok, p.gather(1, y.clamp(0, self.num_classes - 1)[:, None])[:, 0].float(), nan)
        else:
            for name in ('severity', 'mu', 'log_var'):
                out[name] = torch.where(ok, self._store[name][:self.n][idx], nan)
        return out


def fit_model_influence(model, x_or_loader, laplace: Optional[HeadLaplace] = None, chunk: int = 256) -> HeadInfluence:
    """``HeadInfluence`` of the model's own heads in ONE pass over an iterable of batches ``(images, class_labels, severity_labels, ...)``
    in eval mode under no_grad, ``chunk`` images at a time (host batches of a loader are copied to the model's device).  Without a fitted
    ``laplace`` the pass also records into a new ``HeadLaplace``, which is fitted before the rows are embedded; the features, logits and,
    from curriculum stage 3, ``mu`` and ``log_var`` of every row are kept on the device until then (E + C + 2 floats a row).  The index has
    no ``state_dict``: call this again to rebuild it."""
    if not (isinstance(chunk, int) and chunk >= 1):
        raise RovitHipError(f'fit_influence: chunk must be a positive integer, got {chunk!r}')
    if isinstance(x_or_loader, torch.Tensor):
        raise RovitHipError('fit_influence: influence needs the training labels; pass an iterable of (images, class_labels, severity_labels) batches')
    dev = next(model.parameters()).device
    la = laplace if laplace is not None else HeadLaplace(model)
    kept = []
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for batch in x_or_loader:
                if not isinstance(batch, (tuple, list)) or len(batch) < 2:
                    raise RovitHipError('fit_influence: every batch must be (images, class_labels[, severity_labels, ...])')
                images, y = batch[0].to(dev, non_blocking=True), batch[1].to(dev, non_blocking=True)
                s = batch[2].to(dev, non_blocking=True) if len(batch) > 2 else None
                for r0 in range(0, images.shape[0], chunk):
                    out = model(images[r0:r0 + chunk])
                    if laplace is None:
                        la.update(out['features'], out['cls_logits'], out.get('log_var'))
                    kept.append((out['features'], out['cls_logits'], y[r0:r0 + chunk], out.get('mu'), out.get('log_var'),
                                 None if s is None else s[r0:r0 + chunk]))
    finally:
        model.train(was_training)
    if laplace is None:
        la.fit()
    inf = HeadInfluence(la, capacity=max(1, min(native.KAN_STATS_MAX_ROWS, sum(b[0].shape[0] for b in kept))))
    for f, lg, y, mu, lv, s in kept:
        gaussian = la.has_gaussian and mu is not None and lv is not None and s is not None
        inf.update(f, lg, y, *((mu, lv, s) if gaussian else (None, None, None)))
    return inf
