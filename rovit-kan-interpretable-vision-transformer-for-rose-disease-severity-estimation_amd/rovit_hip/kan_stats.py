"""Per-edge activation statistics of the KAN severity head over a data set, and pykan-style feature attribution.

The reference can draw a learned edge function (``KANLayer.plot_activation``, models/kan.py:97-114; explainability/kan_viz.py) but not say
what the edges do ON DATA: how large each one is, how much of it is spline and how much the linear bypass, and which share of the inputs
sits in the dead zone of the truncated basis, where only the bypass acts.

``KANEdgeStats.update`` copies a batch of feature rows to a row offset the host already knows (no synchronisation).  ``compute`` runs the
head's own trajectory on the recorded rows, then ``rovit_kan_edge_stats`` once per layer (csrc/kan_stats.hip: no (N, in, out) intermediate,
fp64 sums in a fixed order) and copies the result buffer to the host: the only synchronisation.  Everything reported is derived from that
block on the host in fp64 (``stats_from_block``); ``kan_attribution`` propagates pykan's standard-deviation scores from the output back
to the input features.

On CPU tensors the same class runs the numpy fp64 restatement below (``edge_stats_block_from_arrays``), as ``EvalAccumulator`` and
``JointLoss._forward_tensor_ops`` do: the host logic is testable without a GPU.  The model's forward keeps having no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import native
from .native import RovitHipError

PARAM_KEYS = ('spline_weights', 'knots', 'linear.weight', 'linear.bias')
ATTRIBUTION_EPS = 1e-4          # pykan's attribute(): sqrt(var) / (sqrt(pre_var) + 1e-4)


# ---- host restatement (fp64) ---------------------------------------------------------------------------------------------------------

def knot_intervals(x: np.ndarray, knots: np.ndarray) -> np.ndarray:
    """Interval index of tanh(x) on the stored knots after the clamp (the search of ``kan_basis``, csrc/kan_device.h): ``knots[t] <= xc <
    knots[t + 1]``, ``t = nk - 1`` only for ``xc == knots[-1]``.  fp64 tanh of the fp32 inputs against the fp32 knots widened."""
    k = np.asarray(knots, dtype=np.float64)
    xc = np.clip(np.tanh(np.asarray(x, dtype=np.float64)), k[0], k[-1])
    return np.clip(np.searchsorted(k, xc, side='right') - 1, 0, len(k) - 1).astype(np.int64)


def basis_rows(x: np.ndarray, knots: np.ndarray, intervals: Optional[np.ndarray] = None) -> np.ndarray:
    """(..., nb) truncated cubic basis of tanh(x): the reference's Cox-de Boor recursion on the STORED knots (models/kan.py:8-44 as
    oracle.ref_cpu.truncated_bspline_basis restates it: nb degree-0 indicators, no right term for the last index), vectorised over the
    basis index in fp64.  Zero from interval ``nb`` on.  ``intervals`` forces the interval of every entry (a test's way to put an input
    within rounding of a knot on either side; the cubic pieces are then evaluated just outside their interval)."""
    k = np.asarray(knots, dtype=np.float64)
    nb = len(k) - 4
    xc = np.clip(np.tanh(np.asarray(x, dtype=np.float64)), k[0], k[-1])
    t = knot_intervals(x, knots) if intervals is None else np.asarray(intervals, dtype=np.int64)
    xe = xc[..., None]
    basis = (t[..., None] == np.arange(nb)).astype(np.float64)

    def ratio(num, den):
        return np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0)
    for d in range(1, 4):
        left = ratio(xe - k[:nb], k[d:d + nb] - k[:nb]) * basis
        shifted = np.concatenate([basis[..., 1:], np.zeros_like(basis[..., :1])], axis=-1)
        right = ratio(k[d + 1:d + 1 + nb] - xe, k[d + 1:d + 1 + nb] - k[1:nb + 1]) * shifted
        basis = left + right
    return basis


def _as_params(p) -> Dict[str, np.ndarray]:
    return {k: np.asarray(p[k].detach().cpu().numpy() if isinstance(p[k], torch.Tensor) else p[k]) for k in PARAM_KEYS}


def layer_section_from_arrays(x, params, intervals: Optional[np.ndarray] = None, chunk: int = 512) -> np.ndarray:
    """One layer's section of the result block (include/rovit_hip.h) from its (N, in) inputs, on the host."""
    p = _as_params(params)
    x = np.asarray(x)
    W = p['spline_weights'].astype(np.float64)
    lw, lb = p['linear.weight'].astype(np.float64), p['linear.bias'].astype(np.float64)
    n, (in_f, out_f, nb) = x.shape[0], W.shape
    nk = nb + 4
    o = native.kan_stats_offsets(in_f, out_f, nk)
    sec = np.zeros(o['words'], dtype=np.int64)
    f = sec.view(np.float64)
    e = in_f * out_f
    edge = np.zeros((4, in_f, out_f))
    pre = np.zeros((2, out_f))
    for r0 in range(0, n, chunk):
        xa = x[r0:r0 + chunk].astype(np.float64)
        B = basis_rows(x[r0:r0 + chunk], p['knots'], None if intervals is None else intervals[r0:r0 + chunk])
        s = np.matmul(B.transpose(1, 0, 2), W.transpose(0, 2, 1)).transpose(1, 0, 2)          # (n, in, out), one BLAS call per input
        phi = s + xa[:, :, None] * lw.T[None]
        edge[0] += phi.sum(0)
        edge[1] += (phi * phi).sum(0)
        edge[2] += np.abs(phi).sum(0)
        edge[3] += np.abs(s).sum(0)
        z = lb[None] + phi.sum(1)
        pre[0] += z.sum(0)
        pre[1] += (z * z).sum(0)
    f[:4 * e] = edge.reshape(-1)
    abs_in = np.abs(x.astype(np.float64)).sum(0)
    f[4 * e:5 * e] = (np.abs(lw).T * abs_in[:, None]).reshape(-1)
    f[o['pre']:o['pre'] + 2 * out_f] = pre.reshape(-1)
    f[o['abs_in']:o['abs_in'] + in_f] = abs_in
    t = knot_intervals(x, p['knots']) if intervals is None else np.asarray(intervals, dtype=np.int64)
    occ = np.zeros((in_f, nk), dtype=np.int64)
    for i in range(in_f):
        occ[i] = np.bincount(t[:, i], minlength=nk)
    sec[o['occupancy']:o['occupancy'] + in_f * nk] = occ.reshape(-1)
    sec[o['nonfinite']] = int((~np.isfinite(x)).sum())
    sec[o['n']] = n
    return sec


def edge_stats_block_from_arrays(layer_inputs: Sequence[np.ndarray], params: Sequence, intervals: Optional[Sequence[np.ndarray]] = None) -> np.ndarray:
    """The result buffer ``KANEdgeStats`` fills on the device -- the layers' sections one after the other, int64 words with the fp64 part
    stored bit for bit -- from each layer's (N, in_l) inputs and parameters (dicts with the state-dict keys ``spline_weights``, ``knots``,
    ``linear.weight``, ``linear.bias``).  Sums run over the whole arrays: the block cannot depend on how the rows arrived."""
    if len(layer_inputs) != len(params):
        raise RovitHipError(f'edge_stats_block_from_arrays: {len(layer_inputs)} layer inputs for {len(params)} layers')
    return np.concatenate([layer_section_from_arrays(x, p, None if intervals is None else intervals[l])
                           for l, (x, p) in enumerate(zip(layer_inputs, params))])


def host_trajectory(features, params: Sequence) -> List[np.ndarray]:
    """Inputs of every layer, then the head's output, as fp32 arrays: ReLU between layers and 3 sigmoid at the end
    (KANSeverityModule.get_activation_trajectory), each layer evaluated in fp64 from the fp32 activations before it."""
    a = np.asarray(features, dtype=np.float32)
    out = [a]
    for l, p in enumerate(params):
        p = _as_params(p)
        z = np.einsum('nik,ijk->nj', basis_rows(a, p['knots']), p['spline_weights'].astype(np.float64))
        z += a.astype(np.float64) @ p['linear.weight'].astype(np.float64).T + p['linear.bias'].astype(np.float64)
        a = (np.maximum(z, 0.0) if l < len(params) - 1 else 3.0 / (1.0 + np.exp(-z))).astype(np.float32)
        out.append(a)
    return out


def stats_from_block(blk: np.ndarray, shapes: Sequence) -> List[Dict]:
    """Per layer, from the result buffer: ``mean``, ``var`` (second central moment), ``l1`` = mean |phi|, ``spline_l1`` = mean |s| (in, out);
    ``pre_mean``, ``pre_var`` (out); ``occupancy`` (in, nk) int64, ``dead_share_per_input`` (in) and ``dead_share``: the share of inputs
    in knot intervals >= num_basis, where the truncated basis is zero; ``mean_abs_input`` (in); ``linear_l1`` = |w_ji| mean |a_i| and
    ``spline_share`` = spline_l1 / (spline_l1 + linear_l1) (in, out; 0 where both are 0); ``n``.  ``shapes``: (in, out, n_knots) per layer."""
    blk = np.asarray(blk, dtype=np.int64)
    out, at = [], 0
    for l, (in_f, out_f, nk) in enumerate(shapes):
        nb = nk - 4
        o = native.kan_stats_offsets(in_f, out_f, nk)
        sec = blk[at:at + o['words']]
        at += o['words']
        f = sec.view(np.float64)
        n = int(sec[o['n']])
        if n < 1:
            raise RovitHipError('KAN edge statistics: no rows recorded')
        if int(sec[o['nonfinite']]):
            raise RovitHipError(f"KAN edge statistics: {int(sec[o['nonfinite']])} non-finite inputs of layer {l}")
        e = in_f * out_f
        sums = f[:5 * e].reshape(5, in_f, out_f)
        mean = sums[native.KAN_STATS_SUM] / n
        pre = f[o['pre']:o['pre'] + 2 * out_f].reshape(2, out_f)
        pre_mean = pre[0] / n
        occ = sec[o['occupancy']:o['occupancy'] + in_f * nk].reshape(in_f, nk).copy()
        mean_abs = f[o['abs_in']:o['abs_in'] + in_f] / n
        spline_l1 = sums[native.KAN_STATS_SPLINE_ABS] / n
        lin_l1 = sums[native.KAN_STATS_LINEAR_ABS] / n
        with np.errstate(divide='ignore', invalid='ignore'):
            share = np.where(spline_l1 + lin_l1 > 0, spline_l1 / (spline_l1 + lin_l1), 0.0)
        out.append({'n': n, 'mean': mean, 'var': np.maximum(sums[native.KAN_STATS_SQ] / n - mean * mean, 0.0),
                    'l1': sums[native.KAN_STATS_ABS] / n, 'spline_l1': spline_l1, 'pre_mean': pre_mean,
                    'pre_var': np.maximum(pre[1] / n - pre_mean * pre_mean, 0.0), 'occupancy': occ,
                    'dead_share_per_input': occ[:, nb:].sum(1) / n, 'dead_share': float(occ[:, nb:].sum()) / (n * in_f),
                    'mean_abs_input': mean_abs, 'linear_l1': lin_l1, 'spline_share': share})
    return out


def kan_attribution(stats: Sequence[Dict]) -> Dict:
    """pykan's ``attribute()``: A^L = 1; edge_scores[l][i, j] = A^{l+1}_j sqrt(var_ij) / (sqrt(pre_var_j) + 1e-4); A^l_i = sum_j
    edge_scores[l][i, j], the activation between layers taken as the identity.  ``node_scores`` = [A^0, ..., A^L]; ``feature_scores`` = A^0:
    which backbone features drive the severity."""
    L = len(stats)
    a = np.ones(np.asarray(stats[-1]['pre_var']).shape[0], dtype=np.float64)
    nodes, edges = [a], [None] * L
    for l in range(L - 1, -1, -1):
        var, pre_var = np.asarray(stats[l]['var'], dtype=np.float64), np.asarray(stats[l]['pre_var'], dtype=np.float64)
        edges[l] = a[None, :] * np.sqrt(var) / (np.sqrt(pre_var)[None, :] + ATTRIBUTION_EPS)
        a = edges[l].sum(axis=1)
        nodes.insert(0, a)
    return {'edge_scores': edges, 'node_scores': nodes, 'feature_scores': a}


# ---- the accumulator -------------------------------------------------------------------------------------------------------------

class KANEdgeStats:
    """Streaming edge statistics of a ``KANSeverityModule`` over one pass of feature rows; see the module docstring.  ``update`` never
    synchronises; ``compute`` copies one buffer to the host."""

    def __init__(self, kan_module, capacity: int = 4096):
        if not (isinstance(capacity, int) and 1 <= capacity <= native.KAN_STATS_MAX_ROWS):
            raise RovitHipError(f'KANEdgeStats: capacity must be in 1..{native.KAN_STATS_MAX_ROWS}, got {capacity!r}')
        if not hasattr(kan_module, 'kan_layers') or len(kan_module.kan_layers) < 1:
            raise RovitHipError('KANEdgeStats: needs a KANSeverityModule')
        for l in kan_module.kan_layers:
            if l.knots.numel() > native.KAN_MAX_KNOTS:
                raise RovitHipError(f'KANEdgeStats: {l.knots.numel()} knots (at most {native.KAN_MAX_KNOTS})')
        self.kan_module, self._capacity0 = kan_module, capacity
        self.in_features = kan_module.kan_layers[0].in_features
        self.reset()

    def reset(self) -> None:
        self.n = 0
        self.device: Optional[torch.device] = None
        self._rows: Optional[torch.Tensor] = None
        self._cpu: List[torch.Tensor] = []
        self._block: Optional[np.ndarray] = None

    def _reserve(self, rows: int) -> None:
        cap = self._rows.shape[0] if self._rows is not None else 0
        if rows <= cap:
            return
        if rows > native.KAN_STATS_MAX_ROWS:
            raise RovitHipError(f'KANEdgeStats: {rows} rows exceed the limit of {native.KAN_STATS_MAX_ROWS}')
        new = torch.empty((min(native.KAN_STATS_MAX_ROWS, max(rows, 2 * cap, self._capacity0)), self.in_features), dtype=torch.float32,
                          device=self.device)
        if self._rows is not None:
            new[:self.n].copy_(self._rows[:self.n])             # device-to-device, stream-ordered: no synchronisation
        self._rows = new

    def update(self, features: torch.Tensor) -> None:
        """Record a batch of (B, in) feature rows, the inputs of the head's first layer."""
        x = features.detach()
        if x.dim() != 2 or x.shape[1] != self.in_features or x.shape[0] < 1:
            raise RovitHipError(f'KANEdgeStats.update: features must be (B >= 1, {self.in_features}), got {tuple(x.shape)}')
        if self.device is None:
            self.device = x.device
        elif x.device != self.device:
            raise RovitHipError(f'KANEdgeStats.update: batch on {x.device}, earlier batches on {self.device}; reset() first')
        self._block = None
        B = x.shape[0]
        if not x.is_cuda:
            self._cpu.append(x.float().clone())
        else:
            self._reserve(self.n + B)
            self._rows[self.n:self.n + B].copy_(x)
        self.n += B

    def _params(self):
        return [{'spline_weights': l.spline_weights.detach(), 'knots': l.knots.detach(), 'linear.weight': l.linear.weight.detach(),
                 'linear.bias': l.linear.bias.detach()} for l in self.kan_module.kan_layers]

    def result_block(self) -> np.ndarray:
        """The layers' sections one after the other as int64 words on the host (fp64 part bit for bit).  On the device this is the one
        synchronising call; the block is kept until the next ``update`` or ``reset``."""
        if self._block is not None:
            return self._block
        if self.n < 1:
            raise RovitHipError('KANEdgeStats: nothing recorded yet')
        params = self._params()
        if self.device.type != 'cuda':
            host = [_as_params(p) for p in params]
            self._block = edge_stats_block_from_arrays(host_trajectory(torch.cat(self._cpu).numpy(), host)[:-1], host)
            return self._block
        dev, mod = self.device, self.kan_module
        if params[0]['spline_weights'].device != dev:
            raise RovitHipError(f"KANEdgeStats: rows on {dev}, the module on {params[0]['spline_weights'].device}")
        was_training = mod.training
        mod.eval()
        try:
            with torch.no_grad():
                traj = mod._trajectory(self._rows[:self.n])
        finally:
            mod.train(was_training)
        lib = native.load()
        shapes = self.shapes()
        words = [lib.rovit_kan_stats_words(*s) for s in shapes]
        result = torch.empty(sum(words), dtype=torch.int64, device=dev)
        partials = torch.empty(max(lib.rovit_kan_stats_partials_doubles(self.n, *s) for s in shapes), dtype=torch.float64, device=dev)
        at = 0
        for l, (p, s) in enumerate(zip(params, shapes)):
            x = traj[l].detach().float().contiguous()
            t = {k: v.float().contiguous() for k, v in p.items()}
            d = native.KANStats()
            d.n, d.in_f, d.out_f, d.n_knots = self.n, *s
            d.x, d.spline_w, d.knots, d.lin_w, d.lin_b = (native.ptr(v) for v in (x, t['spline_weights'], t['knots'], t['linear.weight'],
                                                                                  t['linear.bias']))
            d.partials, d.result = native.ptr(partials), native.ptr(result[at:at + words[l]])
            native.call('rovit_kan_edge_stats', ctypes.byref(d), native.stream_ptr())
            at += words[l]
        self._block = result.cpu().numpy()               # the single device-to-host copy
        return self._block

    def shapes(self):
        return [(l.in_features, l.out_features, l.knots.numel()) for l in self.kan_module.kan_layers]

    def compute(self) -> List[Dict]:
        return stats_from_block(self.result_block(), self.shapes())


def feed_model_features(acc: KANEdgeStats, model, x_or_loader, chunk: int = 256) -> KANEdgeStats:
    """``acc.update(model.backbone(images))`` in eval mode under no_grad, ``chunk`` images at a time, for an image tensor or an iterable
    of batches whose first element is the images.  Images must be on the GPU (host batches of a loader are copied there)."""
    if not (isinstance(chunk, int) and chunk >= 1):
        raise RovitHipError(f'kan_edge_stats: chunk must be a positive integer, got {chunk!r}')
    dev = next(model.parameters()).device
    batches = [(x_or_loader,)] if isinstance(x_or_loader, torch.Tensor) else x_or_loader
    was_training = model.backbone.training
    model.backbone.eval()
    try:
        with torch.no_grad():
            for batch in batches:
                images = batch[0] if isinstance(batch, (tuple, list)) else batch
                if isinstance(x_or_loader, torch.Tensor):
                    native.ptr(images)                              # a CPU tensor raises: the backbone has no CPU path
                else:
                    images = images.to(dev, non_blocking=True)
                for r0 in range(0, images.shape[0], chunk):
                    acc.update(model.backbone(images[r0:r0 + chunk]))
    finally:
        model.backbone.train(was_training)
    return acc


def model_edge_stats(model, x_or_loader, chunk: int = 256) -> List[Dict]:
    return feed_model_features(KANEdgeStats(model.kan_module), model, x_or_loader, chunk).compute()
