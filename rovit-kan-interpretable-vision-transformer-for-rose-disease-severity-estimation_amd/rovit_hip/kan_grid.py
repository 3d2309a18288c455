"""KAN grid extension: refit the learned edge functions of the severity head to a new uniform knot vector by least squares on data.

The reference fixes every layer's knots at construction (``torch.linspace(-1, 1, num_knots + 6)``, models/kan.py:8-44) and truncates the
basis, so each edge spline is identically zero for ``tanh(x) >= knots[num_basis]`` (0.4 on the default grid).  This module
moves a trained head to another grid -- one whose live zone covers [-1, 1] (``layout='cover'``), or a finer one (pykan's
``update_grid_from_samples`` / ``refine``).  The definitions are this repository's own and are written out in DESIGN.md section 2:

    G_i = 1/N_i sum_n b'(v_n) b'(v_n)^T + (eps / L) int_D b' b'^T dv        M_i = 1/N_i sum_n b'(v_n) b(v_n)^T + (eps / L) int_D b' b^T dv
    T_i = (G_i + delta E_i)^-1 M_i      c'_ij = T_i c_ij                      delta = 2^-40 tr(G_i) / nb'
    E_i = diag[(G_i)_kk <= delta]: only the bases that neither the data nor D reach (they get coefficient 0)

with ``b`` / ``b'`` the truncated cubic bases of the old / new knots as ``kan_basis`` (csrc/kan_device.h) evaluates them, ``v = tanh(x)``
over the finite rows of input ``i``, ``D = [max(k'_0, -1), min(k'_nb', 1)]`` and ``L = |D|``: the L2 projection under "data + eps uniform".

``KANRegrid.update`` copies a batch of feature rows to a row offset the host already knows (no synchronisation).  ``fit`` runs, layer by
layer, ``rovit_kan_regrid_moments`` and ``rovit_kan_regrid_solve`` (csrc/kan_grid.hip: no (N, in, nb) tensor, fp64 sums in a fixed order),
pushes the rows through the refitted layer (``rovit_kan_layer_fwd``, ReLU) and copies ONE block, the diagnostics of all layers, to the
host.  ``RegridResult.apply`` installs the new knots and coefficients in the module.

On CPU tensors the same class runs ``regrid_reference``, the numpy fp64 statement of the definitions and the kernels' oracle.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import native
from .functions import ACT_RELU
from .native import RovitHipError

MIN_KNOTS, MAX_KNOTS = native.KAN_REGRID_MIN_KNOTS, native.KAN_MAX_KNOTS
_GL_X = np.array([-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526])
_GL_W = np.array([0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538])


# ---- grids -----------------------------------------------------------------------------------------------------------------------

def check_grid(knots, what: str = 'knots') -> np.ndarray:
    """The fp32 knots as a numpy array, or RovitHipError: 8..64 of them, finite, strictly increasing and uniform by the rule of
    ``KANSeverityModule._uniform_knots`` (the refit's moments and priors are those of the uniform cubic, the kernels' closed form; the
    forward kernels themselves follow any stored knots: kan_device.h)."""
    if isinstance(knots, torch.Tensor):
        knots = (knots.detach().cpu() if knots.is_cuda else knots.detach()).numpy()          # a host tensor costs no copy
    k = np.asarray(knots, dtype=np.float32).reshape(-1)
    if not MIN_KNOTS <= k.size <= MAX_KNOTS:
        raise RovitHipError(f'{what}: {k.size} knots (supported: {MIN_KNOTS}..{MAX_KNOTS})')
    if not np.isfinite(k).all() or not (np.diff(k) > 0).all():
        raise RovitHipError(f'{what}: the knots must be finite and strictly increasing')
    hstep = float(k[-1] - k[0]) / (k.size - 1)
    if not float(np.abs(np.diff(k) - np.float32(hstep)).max()) <= 1e-4 * abs(hstep):
        raise RovitHipError(f'{what}: non-uniform knots (the refit is defined for the uniform cubic basis)')
    return k


def make_grid(num_knots: int = 5, span=(-1.0, 1.0), layout: str = 'cover', margin: float = 2.0 ** -10) -> torch.Tensor:
    """``num_knots + 6`` fp32 knots.  ``layout='cover'``: in fp64, ``lo' = lo - margin``, ``hi' = hi + margin``,
    ``h = (hi' - lo') / (num_knots - 1)``, ``k_t = lo' + (t - 3) h``: the live zone ``[k_3, k_(G+2))`` of the truncated basis contains
    ``[lo, hi]``.  ``layout='reference'``: ``torch.linspace(lo, hi, num_knots + 6)``, the constructor's rule (cutoff inside the span)."""
    G = num_knots
    if not (isinstance(G, int) and 2 <= G <= MAX_KNOTS - 6):
        raise RovitHipError(f'make_grid: num_knots must be an integer in 2..{MAX_KNOTS - 6}, got {G!r}')
    lo, hi = float(span[0]), float(span[1])
    if not (np.isfinite([lo, hi]).all() and lo < hi):
        raise RovitHipError(f'make_grid: span must be finite and increasing, got {span!r}')
    if layout == 'reference':
        return torch.linspace(lo, hi, G + 6)
    if layout != 'cover':
        raise RovitHipError(f"make_grid: layout must be 'cover' or 'reference', got {layout!r}")
    if not (np.isfinite(margin) and margin >= 0):
        raise RovitHipError(f'make_grid: margin must be finite and non-negative, got {margin!r}')
    lo2, hi2 = lo - float(margin), hi + float(margin)
    h = (hi2 - lo2) / (G - 1)
    return torch.from_numpy((lo2 + (np.arange(G + 6, dtype=np.float64) - 3.0) * h).astype(np.float32))


# ---- the basis on the host (fp64; precision is a parameter so the tests can state the fp32 evaluation of the same formulas) --------

def intervals_v(v: np.ndarray, knots: np.ndarray) -> np.ndarray:
    """Interval of the normalised coordinate on the stored knots after the clamp: ``kan_basis``'s search."""
    k = np.asarray(knots)
    xc = np.clip(v, k[0], k[-1])
    return np.clip(np.searchsorted(k, xc, side='right') - 1, 0, k.size - 1).astype(np.int64)


def basis_v(v: np.ndarray, knots: np.ndarray, intervals: Optional[np.ndarray] = None, dtype=np.float64) -> np.ndarray:
    """(..., nb) truncated cubic basis of the NORMALISED coordinate ``v`` exactly as ``kan_basis`` (csrc/kan_device.h) states it: clamp to
    the end knots, interval ``j`` on the stored knots, zero for ``j >= nb``, else ``u = (v - k_j) / (k_(j+1) - k_j)`` and the four uniform
    cubic pieces for the bases ``j .. j - 3`` (those below 0 dropped).  ``intervals`` forces ``j`` (the kernel's own decisions)."""
    k = np.asarray(knots).astype(dtype)
    nk = k.size
    nb = nk - 4
    v = np.asarray(v).astype(dtype)
    xc = np.clip(v, k[0], k[-1])
    j = intervals_v(v, k) if intervals is None else np.asarray(intervals, dtype=np.int64)
    live = (j >= 0) & (j < nb)
    jj = np.where(live, j, 0)
    one, six = dtype(1), dtype(6)
    u = (xc - k[jj]) / (k[jj + 1] - k[jj])
    u2 = u * u
    u3 = u2 * u
    om = one - u
    vals = [u3 / six, (dtype(-3) * u3 + dtype(3) * u2 + dtype(3) * u + one) / six, (dtype(3) * u3 - six * u2 + dtype(4)) / six, om * om * om / six]
    out = np.zeros(v.shape + (nb,), dtype=dtype)
    for m in range(4):
        idx = jj - m
        ok = live & (idx >= 0)
        np.put_along_axis(out, np.where(ok, idx, 0)[..., None], np.where(ok, vals[m], out[..., 0])[..., None], axis=-1)
    return out


def quadrature(new_knots, old_knots):
    """Nodes and weights of the prior's integral over ``D = [max(k'_0, -1), min(k'_nb', 1)]``: 4-point Gauss-Legendre on every piece
    between the merged breakpoints of the two grids, exact for a product of two cubics.  Returns ``(v, w, L)``."""
    kn, ko = np.asarray(new_knots, dtype=np.float64), np.asarray(old_knots, dtype=np.float64)
    lo, hi = max(kn[0], -1.0), min(kn[kn.size - 4], 1.0)
    if not lo < hi:
        raise RovitHipError(f'regrid: the new grid does not meet [-1, 1] (its basis lives on [{kn[0]}, {kn[kn.size - 4]}))')
    pts = np.unique(np.concatenate([[lo, hi], kn[(kn > lo) & (kn < hi)], ko[(ko > lo) & (ko < hi)]]))
    a, b = pts[:-1], pts[1:]
    v = (0.5 * (a + b)[:, None] + 0.5 * (b - a)[:, None] * _GL_X[None]).reshape(-1)
    w = (0.5 * (b - a)[:, None] * _GL_W[None]).reshape(-1)
    return v, w, hi - lo


def prior_moments(new_knots, old_knots) -> Dict:
    """The host integrals ``G = int_D b' b'^T dv`` (nb', nb'), ``M = int_D b' b^T dv`` (nb', nb) in fp64, and ``L = |D|``."""
    v, w, L = quadrature(new_knots, old_knots)
    Bn, Bo = basis_v(v, new_knots), basis_v(v, old_knots)
    return {'G': (Bn * w[:, None]).T @ Bn, 'M': (Bn * w[:, None]).T @ Bo, 'L': L}


# ---- the reference ---------------------------------------------------------------------------------------------------------------

def data_moments(x, old_knots, new_knots, intervals_old=None, intervals_new=None, dtype=np.float64, chunk: int = 256) -> Dict:
    """The data sums per input over its finite rows: ``G`` (in, nb', nb'), ``M`` (in, nb', nb), ``O`` (in, nb, nb) as fp64 SUMS (not means),
    ``rows`` and ``nonfinite`` (in) int64.  ``dtype=np.float32`` evaluates tanh, the bases and the products in fp32 and adds at most 16 rows
    in fp32 before the fp64 sum, as the kernel does: the tests' yardstick for the kernel's distance from fp64."""
    x = np.asarray(x, dtype=np.float32)
    n, in_f = x.shape
    nbn, nb = len(new_knots) - 4, len(old_knots) - 4
    G, M, O = np.zeros((in_f, nbn, nbn)), np.zeros((in_f, nbn, nb)), np.zeros((in_f, nb, nb))
    fin = np.isfinite(x)
    step = 16 if dtype == np.float32 else chunk
    for r0 in range(0, n, step):
        xs, ok = x[r0:r0 + step], fin[r0:r0 + step]
        v = np.tanh(np.where(ok, xs, 0).astype(dtype))
        Bn = basis_v(v, new_knots, None if intervals_new is None else intervals_new[r0:r0 + step], dtype) * ok[..., None].astype(dtype)
        Bo = basis_v(v, old_knots, None if intervals_old is None else intervals_old[r0:r0 + step], dtype) * ok[..., None].astype(dtype)
        G += np.einsum('nia,nib->iab', Bn, Bn)
        M += np.einsum('nia,nib->iab', Bn, Bo)
        O += np.einsum('nia,nib->iab', Bo, Bo)
    return {'G': G, 'M': M, 'O': O, 'rows': fin.sum(0).astype(np.int64), 'nonfinite': (~fin).sum(0).astype(np.int64)}


def solve_moments(mom: Dict, spline_weights, new_knots, old_knots, prior_weight: float = 1e-2) -> Dict:
    """``T_i``, ``c'`` and the diagnostics from the data sums, in fp64: the statement of what ``rovit_kan_regrid_solve`` computes."""
    c = np.asarray(spline_weights, dtype=np.float64)
    in_f, out_f, nb = c.shape
    nbn = len(new_knots) - 4
    pri = prior_moments(new_knots, old_knots)
    Gp, Mp = pri['G'] * (prior_weight / pri['L']), pri['M'] * (prior_weight / pri['L'])
    cn = np.zeros((in_f, out_f, nbn))
    fit_ms, target_ms = np.zeros((in_f, out_f)), np.zeros((in_f, out_f))
    ratio, status = np.zeros(in_f), 0
    for i in range(in_f):
        N = int(mom['rows'][i])
        inv = 1.0 / N if N > 0 else 0.0
        Gd, Md, Od = mom['G'][i] * inv, mom['M'][i] * inv, mom['O'][i] * inv
        A = Gd + Gp
        delta = 2.0 ** -40 * np.trace(A) / nbn
        A = A + np.diag(np.where(np.diag(A) <= delta, delta, 0.0))
        try:
            Lc = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            status += 1
            continue
        piv = np.diag(Lc) ** 2
        ratio[i] = piv.min() / piv.max()
        T = np.linalg.solve(Lc.T, np.linalg.solve(Lc, Md + Mp))
        cn[i] = c[i] @ T.T
        target_ms[i] = np.einsum('ja,ab,jb->j', c[i], Od, c[i])
        fit_ms[i] = np.einsum('ja,ab,jb->j', cn[i], Gd, cn[i]) - 2.0 * np.einsum('ja,ab,jb->j', cn[i], Md, c[i]) + target_ms[i]
    return {'spline_weights': cn, 'fit_ms': fit_ms, 'target_ms': target_ms, 'pivot_ratio': ratio, 'status': status,
            'rows': np.asarray(mom['rows'], dtype=np.int64), 'nonfinite': np.asarray(mom['nonfinite'], dtype=np.int64)}


def regrid_reference(x, old_knots, new_knots, spline_weights, prior_weight: float = 1e-2, intervals_old=None, intervals_new=None,
                     moments: Optional[Dict] = None) -> Dict:
    """One layer's refit in numpy fp64 from its (N, in) inputs: the data sums (``G``, ``M``, ``O``, ``rows``, ``nonfinite``), then the
    new coefficients ``spline_weights`` (in, out, nb') as fp64 and the diagnostics.  ``intervals_old`` / ``intervals_new`` force the knot
    interval of every entry, as ``kan_stats.basis_rows(..., intervals=)`` does; ``moments`` replaces the data sums (the solve alone)."""
    mom = data_moments(x, old_knots, new_knots, intervals_old, intervals_new) if moments is None else moments
    return {**mom, **solve_moments(mom, spline_weights, new_knots, old_knots, prior_weight)}


def moments_from_block(blk: np.ndarray, in_f: int, n_knots_old: int, n_knots_new: int) -> Dict:
    """``rovit_kan_regrid_moments``' block (int64 words, fp64 part bit for bit) as the dense sums ``data_moments`` returns."""
    blk = np.asarray(blk, dtype=np.int64)
    o = native.kan_regrid_moment_offsets(in_f, n_knots_old, n_knots_new)
    nb, nbn = n_knots_old - 4, n_knots_new - 4
    f = blk.view(np.float64)

    def dense(band, n):
        out = np.zeros((in_f, n, n))
        for d in range(4):
            a = np.arange(d, n)
            out[:, a, a - d] = band[:, d:, d]
            out[:, a - d, a] = band[:, d:, d]
        return out
    return {'G': dense(f[:o['M']].reshape(in_f, nbn, 4), nbn), 'M': f[o['M']:o['O']].reshape(in_f, nbn, nb).copy(),
            'O': dense(f[o['O']:o['rows']].reshape(in_f, nb, 4), nb), 'rows': blk[o['rows']:o['nonfinite']].copy(),
            'nonfinite': blk[o['nonfinite']:o['words']].copy()}


def diagnostics_from_block(blk: np.ndarray, in_f: int, out_f: int) -> Dict:
    """One layer's diagnostics dict from ``rovit_kan_regrid_solve``'s block."""
    blk = np.asarray(blk, dtype=np.int64)
    o = native.kan_regrid_diag_offsets(in_f, out_f)
    f = blk.view(np.float64)
    return _diagnostics(f[:o['target_ms']].reshape(in_f, out_f), f[o['target_ms']:o['pivot_ratio']].reshape(in_f, out_f),
                        f[o['pivot_ratio']:o['rows']].copy(), blk[o['rows']:o['nonfinite']].copy(), blk[o['nonfinite']:o['status']].copy(),
                        int(blk[o['status']]))


def _diagnostics(fit_ms, target_ms, ratio, rows, nonfinite, status) -> Dict:
    return {'fit_rms': np.sqrt(np.maximum(fit_ms, 0.0)), 'target_rms': np.sqrt(np.maximum(target_ms, 0.0)), 'rows': rows,
            'nonfinite': nonfinite, 'pivot_ratio': ratio, 'status': status}


def _host_layer(a: np.ndarray, knots, w, lin_w, lin_b) -> np.ndarray:
    """ReLU(layer(a)) in fp64 from fp32 activations, as fp32: the rows the next layer sees."""
    z = np.einsum('nik,ijk->nj', basis_v(np.tanh(a.astype(np.float64)), knots), np.asarray(w, dtype=np.float64))
    z += a.astype(np.float64) @ np.asarray(lin_w, dtype=np.float64).T + np.asarray(lin_b, dtype=np.float64)
    return np.maximum(z, 0.0).astype(np.float32)


# ---- the accumulator -------------------------------------------------------------------------------------------------------------

def host_knots(layer, value: Optional[np.ndarray] = None) -> np.ndarray:
    """The layer's stored knots on the host, kept per (storage, version) of a buffer no optimizer touches: read from the device when
    ``KANRegrid`` is built, handed over by ``RegridResult.apply`` (``value``), so that ``fit`` itself copies nothing but its diagnostics."""
    key = (layer.knots.data_ptr(), layer.knots._version, str(layer.knots.device))
    hit = layer.__dict__.get('_regrid_knots_host')
    if value is not None:
        hit = (key, np.asarray(value, dtype=np.float32).copy())
    elif hit is None or hit[0] != key:
        hit = (key, layer.knots.detach().float().cpu().numpy())
    layer.__dict__['_regrid_knots_host'] = hit
    return hit[1]


class RegridResult:
    """What ``KANRegrid.fit`` returns: per refitted layer ``{'layer', 'knots', 'spline_weights', 'diagnostics'}`` with the tensors on the
    rows' device and the diagnostics (``fit_rms``, ``target_rms`` (in, out); ``rows``, ``nonfinite``, ``pivot_ratio`` (in); ``status``) on
    the host.  ``apply()`` installs it."""

    def __init__(self, kan_module, layers: List[Dict]):
        self.kan_module, self.layers = kan_module, layers

    @property
    def status(self) -> int:
        return sum(int(l['diagnostics']['status']) for l in self.layers)

    @torch.no_grad()
    def apply(self):
        """Install the new knots and coefficients in place: per layer ``num_knots``, ``num_basis``, the ``knots`` buffer and a new
        ``spline_weights`` Parameter (``requires_grad`` kept); the linear terms are untouched.  Optimizers built earlier hold the old
        storage: build a new one (``RoViTAdamW.step`` raises otherwise)."""
        mod = self.kan_module
        if self.status:
            raise RovitHipError(f'RegridResult.apply: {self.status} inputs met a non-positive pivot; nothing installed')
        for r in self.layers:
            layer = mod.kan_layers[r['layer']]
            knots = r['knots'].detach().to(device=layer.knots.device, dtype=layer.knots.dtype).clone()
            w = r['spline_weights'].detach().to(device=layer.spline_weights.device, dtype=layer.spline_weights.dtype).clone()
            layer.num_knots, layer.num_basis = knots.numel() - 2 * layer.degree, knots.numel() - layer.degree - 1
            layer.knots = knots
            host_knots(layer, r['knots'].detach().cpu().numpy() if 'knots_host' not in r else r['knots_host'])
            layer.spline_weights = torch.nn.Parameter(w, requires_grad=layer.spline_weights.requires_grad)
        mod._refresh_grid()
        return mod


class KANRegrid:
    """Streaming refit of a ``KANSeverityModule`` to a new grid over one pass of feature rows; see the module docstring.  ``update`` never
    synchronises; ``fit`` copies one buffer to the host."""

    def __init__(self, kan_module, capacity: int = 4096):
        if not (isinstance(capacity, int) and 1 <= capacity <= native.KAN_STATS_MAX_ROWS):
            raise RovitHipError(f'KANRegrid: capacity must be in 1..{native.KAN_STATS_MAX_ROWS}, got {capacity!r}')
        if not hasattr(kan_module, 'kan_layers') or len(kan_module.kan_layers) < 1:
            raise RovitHipError('KANRegrid: needs a KANSeverityModule')
        self.kan_module, self._capacity0 = kan_module, capacity
        self.in_features = kan_module.kan_layers[0].in_features
        for l in kan_module.kan_layers:
            host_knots(l)
        self.reset()

    def reset(self) -> None:
        self.n = 0
        self.device: Optional[torch.device] = None
        self._rows: Optional[torch.Tensor] = None
        self._cpu: List[torch.Tensor] = []

    def _reserve(self, rows: int) -> None:
        cap = self._rows.shape[0] if self._rows is not None else 0
        if rows <= cap:
            return
        if rows > native.KAN_STATS_MAX_ROWS:
            raise RovitHipError(f'KANRegrid: {rows} rows exceed the limit of {native.KAN_STATS_MAX_ROWS}')
        new = torch.empty((min(native.KAN_STATS_MAX_ROWS, max(rows, 2 * cap, self._capacity0)), self.in_features), dtype=torch.float32,
                          device=self.device)
        if self._rows is not None:
            new[:self.n].copy_(self._rows[:self.n])             # device-to-device, stream-ordered: no synchronisation
        self._rows = new

    def update(self, features: torch.Tensor) -> None:
        """Record a batch of (B, in) feature rows, the inputs of the head's first layer."""
        x = features.detach()
        if x.dim() != 2 or x.shape[1] != self.in_features or x.shape[0] < 1:
            raise RovitHipError(f'KANRegrid.update: features must be (B >= 1, {self.in_features}), got {tuple(x.shape)}')
        if self.device is None:
            self.device = x.device
        elif x.device != self.device:
            raise RovitHipError(f'KANRegrid.update: batch on {x.device}, earlier batches on {self.device}; reset() first')
        B = x.shape[0]
        if not x.is_cuda:
            self._cpu.append(x.float().clone())
        else:
            self._reserve(self.n + B)
            self._rows[self.n:self.n + B].copy_(x)
        self.n += B

    def _new_knots(self, num_knots, knots, span, layout, margin, layers) -> Dict[int, np.ndarray]:
        mod = self.kan_module
        L = len(mod.kan_layers)
        which = list(range(L)) if layers is None else sorted(set(int(l) for l in layers))
        if not which or which[0] < 0 or which[-1] >= L:
            raise RovitHipError(f'KANRegrid.fit: layers must name some of 0..{L - 1}, got {layers!r}')
        if knots is not None:
            per = [knots] * len(which) if isinstance(knots, (torch.Tensor, np.ndarray)) else list(knots)
            if len(per) != len(which):
                raise RovitHipError(f'KANRegrid.fit: {len(per)} knot vectors for {len(which)} layers')
            return {l: check_grid(k, f'KANRegrid.fit: knots of layer {l}') for l, k in zip(which, per)}
        out = {}
        for l in which:
            G = mod.kan_layers[l].knots.numel() - 6 if num_knots is None else num_knots
            out[l] = check_grid(make_grid(G, span, layout, margin), f'KANRegrid.fit: layer {l}')
        return out

    def fit(self, num_knots: Optional[int] = None, knots=None, span=(-1.0, 1.0), layout: str = 'cover', margin: float = 2.0 ** -10,
            prior_weight: float = 1e-2, layers: Optional[Sequence[int]] = None) -> RegridResult:
        """Refit the layers (all by default) in order on the recorded rows; see the module docstring.  ``knots``: one explicit knot
        vector for every refitted layer, or one per layer; else ``make_grid(num_knots or the layer's own, span, layout, margin)``."""
        if not (isinstance(prior_weight, (int, float)) and np.isfinite(prior_weight) and prior_weight > 0):
            raise RovitHipError(f'KANRegrid.fit: prior_weight must be positive, got {prior_weight!r}')
        new = self._new_knots(num_knots, knots, span, layout, margin, layers)
        if self.n < 1:
            raise RovitHipError('KANRegrid: nothing recorded yet')
        mod = self.kan_module
        for l in mod.kan_layers:
            check_grid(host_knots(l), 'KANRegrid.fit: the stored knots')
        dev = self.device
        if mod.kan_layers[0].spline_weights.device != dev:
            raise RovitHipError(f'KANRegrid: rows on {dev}, the module on {mod.kan_layers[0].spline_weights.device}')
        if dev.type != 'cuda':
            return self._fit_host(new, float(prior_weight))
        lib = native.load()
        n, sp = self.n, native.stream_ptr()
        shapes = {l: (mod.kan_layers[l].in_features, mod.kan_layers[l].out_features, mod.kan_layers[l].knots.numel(), new[l].size) for l in new}
        dwords = {l: lib.rovit_kan_regrid_diag_words(s[0], s[1]) for l, s in shapes.items()}
        diag = torch.empty(sum(dwords.values()), dtype=torch.int64, device=dev)
        wbytes = max(lib.rovit_kan_regrid_workspace_bytes(n, s[0], s[2], s[3]) for s in shapes.values())
        work = torch.empty((wbytes + 7) // 8, dtype=torch.float64, device=dev)
        out, at = [], 0
        a = self._rows[:n]
        last = max(new)
        for l, layer in enumerate(mod.kan_layers):
            if l > last:
                break
            w = layer.spline_weights.detach().float().contiguous()
            kn = layer.knots.detach().float().contiguous()
            if l in new:
                in_f, out_f, nko, nkn = shapes[l]
                kn_new = torch.from_numpy(new[l]).to(dev)
                pri = prior_moments(new[l], host_knots(layer))
                scale = prior_weight / pri['L']
                pg = torch.from_numpy(np.ascontiguousarray(pri['G'] * scale)).to(dev)
                pm = torch.from_numpy(np.ascontiguousarray(pri['M'] * scale)).to(dev)
                x = a.contiguous()
                mom = device_moments(x, kn, kn_new, work)
                w_new = device_solve(mom, pg, pm, w, nkn, diag[at:at + dwords[l]])
                at += dwords[l]
                out.append({'layer': l, 'knots': kn_new, 'knots_host': new[l], 'spline_weights': w_new, 'moments': mom})
                w, kn = w_new, kn_new
            if l < last:                                        # the rows the next layer will see: through the refitted layer, then ReLU
                lw, lb = layer.linear.weight.detach().float().contiguous(), layer.linear.bias.detach().float().contiguous()
                nxt = torch.empty(n, layer.out_features, dtype=torch.float32, device=dev)
                x = a.contiguous()
                native.call('rovit_kan_layer_fwd', native.ptr(x), native.ptr(w), native.ptr(kn), native.ptr(lw), native.ptr(lb), native.ptr(nxt), n,
                            layer.in_features, layer.out_features, kn.numel(), ACT_RELU, sp)
                a = nxt
        blk = diag.cpu().numpy()                                # the single device-to-host copy
        at = 0
        for r in out:
            in_f, out_f = shapes[r['layer']][:2]
            r['diagnostics'] = diagnostics_from_block(blk[at:at + dwords[r['layer']]], in_f, out_f)
            at += dwords[r['layer']]
        return RegridResult(mod, out)

    def _fit_host(self, new: Dict[int, np.ndarray], prior_weight: float) -> RegridResult:
        mod = self.kan_module
        a = torch.cat(self._cpu).numpy()
        out, last = [], max(new)
        for l, layer in enumerate(mod.kan_layers):
            if l > last:
                break
            w, kn = layer.spline_weights.detach().float().numpy(), layer.knots.detach().float().numpy()
            if l in new:
                r = regrid_reference(a, kn, new[l], w, prior_weight)
                w, kn = r['spline_weights'].astype(np.float32), new[l]
                out.append({'layer': l, 'knots': torch.from_numpy(kn.copy()), 'knots_host': kn, 'spline_weights': torch.from_numpy(w),
                            'diagnostics': _diagnostics(r['fit_ms'], r['target_ms'], r['pivot_ratio'], r['rows'], r['nonfinite'], r['status'])})
            if l < last:
                a = _host_layer(a, kn, w, layer.linear.weight.detach().numpy(), layer.linear.bias.detach().numpy())
        return RegridResult(mod, out)


def device_moments(x: torch.Tensor, knots_old: torch.Tensor, knots_new: torch.Tensor, work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``rovit_kan_regrid_moments`` on fp32 device tensors: the moment block (int64 words) of one layer's (N, in) inputs."""
    lib = native.load()
    n, in_f = x.shape
    nko, nkn = knots_old.numel(), knots_new.numel()
    need = lib.rovit_kan_regrid_workspace_bytes(n, in_f, nko, nkn)
    if work is None or work.numel() * 8 < need:
        work = torch.empty(max(1, (need + 7) // 8), dtype=torch.float64, device=x.device)
    mom = torch.empty(max(1, lib.rovit_kan_regrid_moment_words(in_f, nko, nkn)), dtype=torch.int64, device=x.device)
    d = native.KANRegridMoments()
    d.n, d.in_f, d.n_knots_old, d.n_knots_new = n, in_f, nko, nkn
    d.x, d.knots_old, d.knots_new = native.ptr(x), native.ptr(knots_old), native.ptr(knots_new)
    d.workspace, d.workspace_bytes, d.moments = native.ptr(work), work.numel() * 8, native.ptr(mom)
    native.call('rovit_kan_regrid_moments', ctypes.byref(d), native.stream_ptr())
    return mom


def device_solve(mom: torch.Tensor, prior_g: torch.Tensor, prior_m: torch.Tensor, spline_w: torch.Tensor, n_knots_new: int,
                 diag: torch.Tensor) -> torch.Tensor:
    """``rovit_kan_regrid_solve``: the new (in, out, nb') coefficients; ``diag`` (int64 words on the device) receives the diagnostics.
    ``prior_g`` / ``prior_m``: fp64 device tensors, already weighted by eps / L."""
    in_f, out_f, nb = spline_w.shape
    w_new = torch.empty(in_f, out_f, n_knots_new - 4, dtype=torch.float32, device=spline_w.device)
    f = native.KANRegridFit()
    f.in_f, f.out_f, f.n_knots_old, f.n_knots_new = in_f, out_f, nb + 4, n_knots_new
    f.moments, f.prior_g, f.prior_m, f.spline_w, f.spline_w_new = (native.ptr(t) for t in (mom, prior_g, prior_m, spline_w, w_new))
    f.diagnostics = native.ptr(diag)
    native.call('rovit_kan_regrid_solve', ctypes.byref(f), native.stream_ptr())
    return w_new


def model_regrid(model, x_or_loader, chunk: int = 256, **fit_kw) -> RegridResult:
    """``RoViTKAN.kan_regrid``: record ``model.backbone(images)`` over an image tensor or a loader, fit, apply; returns the result."""
    from .kan_stats import feed_model_features
    acc = feed_model_features(KANRegrid(model.kan_module), model, x_or_loader, chunk)
    res = acc.fit(**fit_kw)
    res.apply()
    if hasattr(model, '_head_grad_views'):
        model._head_grad_views = None
    return res
