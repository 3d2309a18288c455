"""Adversarial perturbations of a RoViTKAN input on the GPU: the worst change of a given size, where ``corrupt.py`` asks about the
average one.  Projected gradient ascent (Goodfellow et al., "Explaining and Harnessing Adversarial Examples", ICLR 2015, for the
one-step form; Madry et al., "Towards Deep Learning Models Resistant to Adversarial Attacks", ICLR 2018; the margin objective is the
one Croce & Hein, "Reliable Evaluation of Adversarial Robustness with an Ensemble of Diverse Parameter-free Attacks", ICML 2020,
recommend over cross-entropy) with the gradient route of ``input_grad.py`` -- training-mode fused forward, the head phase's own
backward, the dgrad chain alone down to the pixels -- and the step, the projection and the random start in csrc/attack.hip.

The step (specification of record; ``step_reference`` is its numpy statement)
-------------------------------------------------------------------------------
Images are NORMALISED, ``x = (z - mean_c) / std_c`` with ``z`` in [0, 1]; radii ``eps_b`` and step lengths ``alpha_b`` are per image and
in PIXEL units.  Constants: ``inv_s_c = fl32(1 / std_c)``, ``s_c = fl32(std_c)``, the box ``lo_c, hi_c`` = the fp32 normalisation of
``clip`` (``-inf, +inf`` for ``clip=None``); per image and channel ``r = fl32(eps_b inv_s_c)``, ``a = fl32(alpha_b inv_s_c)``.
``clamp(v, l, h)`` is ``l`` when ``v < l``, ``h`` when ``v > h``, else ``v`` itself: a zero keeps its sign and a NaN passes through
(``fminf`` / ``fmaxf`` leave both open, and the kernel has to equal numpy to the bit).

L-infinity, every operation rounded once to fp32::

    sg = +1, -1, 0 for g > 0, g < 0, and g == 0 or NaN
    d1 = delta + sg a;  d2 = clamp(d1, -r, r);  y = clamp(x + d2, lo, hi);  delta' = clamp(y - x, -r, r);  x_adv = clamp(x + delta', lo, hi)

``|delta'| <= r`` and ``lo <= x_adv <= hi`` hold exactly, and ``eps_b == 0`` leaves ``x_adv == x`` wherever ``x`` is inside the box.
``x_adv - x`` may differ from ``delta'`` by the one rounding of ``x + delta'``: half an ulp of ``x_adv``, at most 2^-23 for
``|x_adv|`` in [2, 4), against ``r >= 0.017`` at ``eps = 1/255``.

L2, the ball in pixel units (``u = delta s_c``), fp64 up to each ``fl32``::

    gh = g inv_s (0 where g is not finite);  G = |gh|_2 over the image;  d1 = delta + (alpha_b gh / G) inv_s   (G == 0: d1 = delta)
    db = fl32(clamp(d1, lo - x, hi - x));  U = |db s|_2;  delta' = fl32(db min(1, eps_b / U));  x_adv = clamp(fl32(x + delta'), lo, hi)

The box is applied to the perturbation (``delta`` in ``[lo - x, hi - x]``), not to ``x + delta``: the sum would round at the size of
``x``, about 2^-23, which is far above 2^-24 r.  The box is convex and holds ``x``, so the shrink to the ball stays inside it.  Both norms
are fp64 sums in a fixed order, so two runs give the same bits.

The start (``init_reference``): element ``e`` (its index in the (3, H, W) image) of the image with id ``ids[b]`` takes word ``e % 4`` of
Philox4x32-10(key = ``seed``, counter = ``(e / 4, ids[b], ATTACK_STREAM, restart)``), so a draw depends on ``(seed, ids[b], e, restart)``
and never on the batch split.  L-infinity: ``d1 = fl32((2 u - 1) r)`` with ``u = (word >> 8) 2^-24``, then ``d2 .. x_adv`` as above.  L2:
Box-Muller normals in fp64 -- words (x, y) of a call give ``z(4k) = R cos T``, ``z(4k + 1) = R sin T`` with ``R = sqrt(-2 ln(((x >> 8) + 1)
2^-24))``, ``T = 2 pi (y >> 8) 2^-24``; words (z, w) give ``z(4k + 2)``, ``z(4k + 3)`` the same way -- rounded once to fp32;
``d1 = (eps_b z / |z|_2) inv_s``, then ``db .. x_adv`` as above.

``PGD`` is the loop alone, for any ``value_and_grad``; on CPU tensors it runs the reference functions.  ``objective_gradient``,
``pgd_attack`` and ``robustness_radius`` are the model's side of it."""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Optional

import numpy as np
import torch

from . import native
from .native import RovitHipError, call, ptr, stream_ptr

NORMS = {'linf': native.ATTACK_LINF, 'l2': native.ATTACK_L2}
CLASS_OBJECTIVES = ('ce', 'margin')


def _mean_std():
    from data.transforms import IMAGENET_MEAN, IMAGENET_STD
    return IMAGENET_MEAN, IMAGENET_STD


def constants(mean=None, std=None, clip=(0., 1.)):
    """``(inv_s, s, lo, hi)``, four fp32 arrays of 3: the constants of the module docstring.  Raises on a bad mean / std / clip."""
    if mean is None or std is None:
        m0, s0 = _mean_std()
        mean, std = (m0 if mean is None else mean), (s0 if std is None else std)
    try:
        m, sd = np.asarray(mean, dtype=np.float64).reshape(-1), np.asarray(std, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise RovitHipError(f'attack: mean and std must be three numbers each, got {mean!r} and {std!r}') from None
    if m.shape != (3,) or sd.shape != (3,) or not (np.isfinite(m).all() and np.isfinite(sd).all() and (sd > 0).all()):
        raise RovitHipError(f'attack: mean and std must be three finite numbers each, std positive, got {mean!r} and {std!r}')
    s = sd.astype(np.float32)
    inv_s = (1.0 / sd).astype(np.float32)
    if clip is None:
        lo, hi = np.full(3, -np.inf, np.float32), np.full(3, np.inf, np.float32)
    else:
        try:
            c0, c1 = (float(v) for v in clip)
        except (TypeError, ValueError):
            raise RovitHipError(f'attack: clip must be None or a pair (low, high), got {clip!r}') from None
        if not (math.isfinite(c0) and math.isfinite(c1) and c0 <= c1):
            raise RovitHipError(f'attack: clip must be None or a finite pair low <= high, got {clip!r}')
        m32 = m.astype(np.float32)
        lo, hi = (np.float32(c0) - m32) / s, (np.float32(c1) - m32) / s          # the pipeline's own normalisation, fp32
    return inv_s, s, lo, hi


def _norm_id(norm) -> int:
    if norm not in NORMS:
        raise RovitHipError(f"attack: norm must be 'linf' or 'l2', got {norm!r}")
    return NORMS[norm]


# ------------------------------------------------------------------------------------------------------------
# The reference
# ------------------------------------------------------------------------------------------------------------
def _clamp(v, lo, hi):
    with np.errstate(invalid='ignore'):
        return np.where(v < lo, lo, np.where(v > hi, hi, v))


def _per_image(v, B: int) -> np.ndarray:
    """(B,) fp32 from a number or a (B,) array."""
    a = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float32).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, B)
    if a.shape != (B,):
        raise RovitHipError(f'attack: a per-image value must be a number or have shape ({B},), got {a.shape}')
    return a


def _as_np(t) -> np.ndarray:
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t), dtype=np.float32)


def _setup(x, eps, mean, std, clip, T):
    """x fp32 (B, 3, H, W) in T, and the constants broadcast to it in T (each computed in fp32 first, as the kernel receives them)."""
    x32 = _as_np(x)
    if x32.ndim != 4 or x32.shape[1] != 3 or x32.shape[0] < 1 or x32.shape[2] * x32.shape[3] < 1:
        raise RovitHipError(f'attack: expects (B, 3, H, W) images, got {x32.shape}')
    B = x32.shape[0]
    inv_s, s, lo, hi = constants(mean, std, clip)
    eps32 = _per_image(eps, B)
    shape = lambda v: v.reshape(1, 3, 1, 1)
    r32 = eps32.reshape(B, 1, 1, 1) * shape(inv_s)                                   # fp32: the kernel's r
    k = {'inv_s': shape(inv_s).astype(T), 's': shape(s).astype(T), 'lo': shape(lo).astype(T), 'hi': shape(hi).astype(T),
         'r': r32.astype(T), 'eps': eps32.astype(T).reshape(B, 1, 1, 1), 'inv_s32': shape(inv_s)}
    return x32.astype(T), k, B


def _project_linf(x, d1, k):
    d2 = _clamp(d1, -k['r'], k['r'])
    y = _clamp(x + d2, k['lo'], k['hi'])
    dn = _clamp(y - x, -k['r'], k['r'])
    return dn, _clamp(x + dn, k['lo'], k['hi'])


def _finish_l2(x, d1, k, T):
    """From the moved perturbation: box in delta space, shrink to the ball, x_adv."""
    db = _clamp(d1, k['lo'] - x, k['hi'] - x)
    U = np.sqrt(((db * k['s']).astype(np.float64) ** 2).sum(axis=(1, 2, 3), keepdims=True)).astype(T)
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.where(U > k['eps'], k['eps'] / U, T(1.0))
    dn = db * f
    return dn, _clamp(x + dn, k['lo'], k['hi'])


def step_reference(x, g, delta, eps, alpha, norm='linf', mean=None, std=None, clip=(0., 1.), dtype=np.float32):
    """One projected ascent step of the module docstring in numpy: ``(delta', x_adv)`` in ``dtype``.  ``x``, ``g``, ``delta``
    (B, 3, H, W) fp32 values (numpy or torch); ``eps``, ``alpha`` numbers or (B,) in pixel units.  ``dtype=np.float32`` repeats the
    L-infinity kernel's operations in its order, one rounding each, and equals it to the bit; ``np.float64`` is the oracle of the L2
    kernel (whose own arithmetic is fp64 with three roundings to fp32)."""
    _norm_id(norm)
    T = np.dtype(dtype).type
    xT, k, B = _setup(x, eps, mean, std, clip, T)
    gT, dT = _as_np(g), _as_np(delta).astype(T)
    if gT.shape != xT.shape or dT.shape != xT.shape:
        raise RovitHipError(f'attack: x, g and delta must have one shape, got {xT.shape}, {gT.shape}, {dT.shape}')
    al32 = _per_image(alpha, B).reshape(B, 1, 1, 1)
    with np.errstate(invalid='ignore', over='ignore'):
        if norm == 'linf':
            a = (al32 * k['inv_s32']).astype(T)                                  # fp32: the kernel's a
            sg = np.where(gT > 0, T(1.0), np.where(gT < 0, T(-1.0), T(0.0))).astype(T)
            return _project_linf(xT, dT + sg * a, k)
        gh = np.where(np.isfinite(gT), gT.astype(T) * k['inv_s'], T(0.0))
        G = np.sqrt((gh.astype(np.float64) ** 2).sum(axis=(1, 2, 3), keepdims=True)).astype(T)
        with np.errstate(divide='ignore'):
            t = np.where(G > 0, al32.astype(T) / G, T(0.0))
        return _finish_l2(xT, dT + gh * t * k['inv_s'], k, T)


def attack_calls(ids, count: int, seed: int, restart: int):
    """The four words of each element's Philox call: four (len(ids), count) uint64 arrays (element e reads call e / 4)."""
    from oracle.philox import philox4x32_10 as philox          # checker only, like corrupt._words
    ids = np.asarray(ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else ids, dtype=np.int64).reshape(-1)
    e = np.arange(count, dtype=np.uint64)
    out = [np.empty((ids.size, count), dtype=np.uint64) for _ in range(4)]
    for row, i in enumerate(ids):
        full = lambda v: np.full(count, v, dtype=np.uint64)
        w = philox([e >> np.uint64(2), full(int(i) & 0xFFFFFFFF), full(native.ATTACK_STREAM), full(int(restart) & 0xFFFFFFFF)],
                   [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
        for q in range(4):
            out[q][row] = w[q]
    return out


def attack_words(ids, count: int, seed: int, restart: int) -> np.ndarray:
    """(len(ids), count) uint64: the Philox word of elements 0 .. count - 1 of the images ``ids``, word e % 4 of call e / 4."""
    w = attack_calls(ids, count, seed, restart)
    return np.choose(np.arange(count) & 3, w)


def init_reference(x, ids, eps, norm='linf', seed: int = 0, restart: int = 0, mean=None, std=None, clip=(0., 1.), dtype=np.float32):
    """The random start of the module docstring in numpy: ``(delta, x_adv)`` in ``dtype``; ``ids`` (B,) integers."""
    _norm_id(norm)
    T = np.dtype(dtype).type
    xT, k, B = _setup(x, eps, mean, std, clip, T)
    count = xT[0].size
    w = attack_words(ids, count, int(seed), int(restart))
    if w.shape[0] != B:
        raise RovitHipError(f'attack: {w.shape[0]} ids for {B} images')
    if norm == 'linf':
        u = (w >> np.uint64(8)).astype(T) * T(1.0 / 16777216.0)
        t = (T(2.0) * u - T(1.0)).reshape(xT.shape)
        return _project_linf(xT, t * k['r'], k)
    # the pair (4k, 4k + 1) holds words (x, y) of call k, the pair (4k + 2, 4k + 3) words (z, w); the partner word comes from the call,
    # not from the neighbouring element, so a pair cut short by the image's end is no special case
    e = np.arange(count)
    words = attack_calls(ids, count, int(seed), int(restart))
    j = e & 3
    wa = np.where(j < 2, words[0], words[2])
    wb = np.where(j < 2, words[1], words[3])
    rad = np.sqrt(-2.0 * np.log(((wa >> np.uint64(8)) + np.uint64(1)).astype(np.float64) / 16777216.0))
    ang = 2.0 * math.pi * ((wb >> np.uint64(8)).astype(np.float64) / 16777216.0)
    z = (rad * np.where((j & 1) == 1, np.sin(ang), np.cos(ang))).astype(np.float32).astype(T).reshape(xT.shape)
    Z = np.sqrt((z.astype(np.float64) ** 2).sum(axis=(1, 2, 3), keepdims=True)).astype(T)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(Z > 0, k['eps'] / Z, T(0.0))
    return _finish_l2(xT, z * t * k['inv_s'], k, T)


# ------------------------------------------------------------------------------------------------------------
# The kernels
# ------------------------------------------------------------------------------------------------------------
class _Kernels:
    """The host side of csrc/attack.hip for one image shape: the constants as C arrays and the L2 scratch."""

    def __init__(self, norm: str, mean, std, clip, x: torch.Tensor):
        self.norm = norm
        self.B, _, self.H, self.W = x.shape
        self.consts = constants(mean, std, clip)
        self.c = [(C.c_float * 3)(*[float(v) for v in arr]) for arr in self.consts]
        self.scratch = None
        if norm == 'l2' and x.is_cuda:
            words = int(native.load().rovit_attack_scratch_doubles(self.B, self.H, self.W))
            if words == 0:
                raise RovitHipError(f'attack: {self.B} images of {self.H} x {self.W} are outside what the kernels take')
            self.scratch = torch.empty(words, dtype=torch.float64, device=x.device)
        self.mean, self.std, self.clip = mean, std, clip

    def step(self, x, g, delta, x_adv, best_delta, mask, eps, alpha):
        if not x.is_cuda:
            d, xa = step_reference(x, g, delta, eps, alpha, self.norm, self.mean, self.std, self.clip,
                                   np.float32 if self.norm == 'linf' else np.float64)
            if best_delta is not None:
                best_delta.copy_(torch.where(mask.view(-1, 1, 1, 1), delta, best_delta))
            delta.copy_(torch.from_numpy(d.astype(np.float32)))
            x_adv.copy_(torch.from_numpy(xa.astype(np.float32)))
            return
        inv_s, s, lo, hi = self.c
        m8 = mask.view(torch.uint8) if mask is not None else None
        if self.norm == 'linf':
            call('rovit_attack_step_linf', ptr(x), ptr(g), ptr(delta), ptr(x_adv), ptr(best_delta), ptr(m8), ptr(eps), ptr(alpha), inv_s, lo, hi,
                 self.B, self.H, self.W, stream_ptr())
        else:
            call('rovit_attack_step_l2', ptr(x), ptr(g), ptr(delta), ptr(x_adv), ptr(best_delta), ptr(m8), ptr(eps), ptr(alpha), inv_s, s, lo, hi,
                 ptr(self.scratch), self.B, self.H, self.W, stream_ptr())

    def init(self, x, delta, x_adv, ids, eps, seed: int, restart: int):
        if not x.is_cuda:
            d, xa = init_reference(x, ids, eps, self.norm, seed, restart, self.mean, self.std, self.clip,
                                   np.float32 if self.norm == 'linf' else np.float64)
            delta.copy_(torch.from_numpy(d.astype(np.float32)))
            x_adv.copy_(torch.from_numpy(xa.astype(np.float32)))
            return
        inv_s, s, lo, hi = self.c
        call('rovit_attack_init', ptr(x), ptr(delta), ptr(x_adv), ptr(ids), ptr(eps), NORMS[self.norm], int(seed) & 0xFFFFFFFFFFFFFFFF,
             int(restart) & 0xFFFFFFFF, inv_s, s, lo, hi, ptr(self.scratch), self.B, self.H, self.W, stream_ptr())

    def box(self, x):
        """clamp(x, lo, hi) per channel: the image the loop starts from without a random start, and x + delta of the final select."""
        lo, hi = (torch.from_numpy(v).to(x.device).view(1, 3, 1, 1) for v in self.consts[2:])
        return torch.where(x < lo, lo, torch.where(x > hi, hi, x))


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


class PGD:
    """The projected-gradient loop alone, for any ``value_and_grad(x_adv) -> (value (B,), grad like x_adv)`` that is to be MAXIMISED,
    as ``KernelShap`` is the estimator alone.  CUDA tensors drive the kernels of csrc/attack.hip; CPU tensors drive ``step_reference`` /
    ``init_reference``.

    ``norm``: ``'linf'`` or ``'l2'``; ``eps``: the radius in pixel units, a number or a (B,) tensor; ``steps`` >= 1;
    ``step_size``: a number, a (B,) tensor, or None for ``2.5 eps / steps`` (Madry et al.); ``random_start``; ``restarts`` >= 1, each
    with its own start (restart r draws Philox counter word 3 = r; without a random start every restart is the same run, so only one
    is made); ``seed``; ``mean`` / ``std``: the normalisation (default the ImageNet constants of ``data.transforms``);
    ``clip``: the pixel range, or None for no box.

    ``__call__(value_and_grad, x, ids=None, value=None)`` returns ``{'delta', 'x_adv', 'value'}``: per image the perturbation with the
    highest objective value seen -- every iterate of every restart, the clean image included when ``random_start=False``.  A NaN value
    never wins and a tie keeps the earlier perturbation; an image whose values are all NaN keeps ``delta = 0``.  ``ids`` (B,) integers
    name the images to the random start (default ``arange(B)``).  ``value(x_adv) -> (B,)``, when given, evaluates the last iterate
    without a gradient.  K steps cost K gradient calls, one value call and one select; the (B,) comparison that keeps the best is a torch
    operation on the device, and nothing is read back to the host inside the loop."""

    def __init__(self, norm: str = 'linf', eps=8 / 255, steps: int = 10, step_size=None, random_start: bool = True, restarts: int = 1,
                 seed: int = 0, mean=None, std=None, clip=(0., 1.)):
        _norm_id(norm)
        for name, v in (('eps', eps), ('step_size', step_size)):
            if v is None and name == 'step_size':
                continue
            if isinstance(v, torch.Tensor):
                if not v.dtype.is_floating_point or v.dim() != 1:
                    raise RovitHipError(f'PGD: {name} as a tensor must be a floating-point (B,) tensor, got {v.dtype} {tuple(v.shape)}')
            elif not _is_number(v) or not math.isfinite(v) or v < 0:
                raise RovitHipError(f'PGD: {name} must be a finite number >= 0 or a (B,) tensor, got {v!r}')
        if not _is_int(steps) or steps < 1:
            raise RovitHipError(f'PGD: steps must be an int >= 1, got {steps!r}')
        if not _is_int(restarts) or restarts < 1:
            raise RovitHipError(f'PGD: restarts must be an int >= 1, got {restarts!r}')
        if not _is_int(seed) or seed < 0:
            raise RovitHipError(f'PGD: seed must be an int >= 0, got {seed!r}')
        if not isinstance(random_start, (bool, np.bool_)):
            raise RovitHipError(f'PGD: random_start must be a bool, got {random_start!r}')
        constants(mean, std, clip)
        self.norm, self.eps, self.steps, self.step_size = norm, eps, int(steps), step_size
        self.random_start, self.restarts, self.seed = bool(random_start), int(restarts), int(seed)
        self.mean, self.std, self.clip = mean, std, clip

    @staticmethod
    def _vector(v, B, dev, name):
        if isinstance(v, torch.Tensor):
            if tuple(v.shape) != (B,):
                raise RovitHipError(f'PGD: {name} must have shape ({B},), got {tuple(v.shape)}')
            return v.detach().to(device=dev, dtype=torch.float32).contiguous()
        return torch.full((B,), float(v), dtype=torch.float32, device=dev)

    def check(self, x, ids=None):
        """The checks of a call that need the images: raises before anything runs."""
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1 or x.shape[2] * x.shape[3] < 1:
            raise RovitHipError(f'PGD: expects (B, 3, H, W) images, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}')
        if not x.dtype.is_floating_point:
            raise RovitHipError(f'PGD: the images must be floating point, got {x.dtype}')
        B = x.shape[0]
        for name, v in (('eps', self.eps), ('step_size', self.step_size)):
            if isinstance(v, torch.Tensor) and tuple(v.shape) != (B,):
                raise RovitHipError(f'PGD: {name} must have shape ({B},), got {tuple(v.shape)}')
        if ids is not None:
            if not isinstance(ids, torch.Tensor) or ids.dtype.is_floating_point or ids.dtype == torch.bool or tuple(ids.shape) != (B,):
                raise RovitHipError(f'PGD: ids must be an integer ({B},) tensor')

    def __call__(self, value_and_grad: Callable, x: torch.Tensor, ids: Optional[torch.Tensor] = None, value: Optional[Callable] = None):
        self.check(x, ids)
        with torch.no_grad():
            dev = x.device
            x = x.detach().float().contiguous()
            B = x.shape[0]
            eps = self._vector(self.eps, B, dev, 'eps')
            alpha = eps * (2.5 / self.steps) if self.step_size is None else self._vector(self.step_size, B, dev, 'step_size')
            ids = torch.arange(B, device=dev) if ids is None else ids.detach().to(device=dev, dtype=torch.int64).contiguous()
            k = _Kernels(self.norm, self.mean, self.std, self.clip, x)
            delta, x_adv, best_delta = torch.zeros_like(x), torch.empty_like(x), torch.zeros_like(x)
            best_value = torch.full((B,), -math.inf, dtype=torch.float32, device=dev)
            for restart in range(self.restarts if self.random_start else 1):
                if self.random_start:
                    k.init(x, delta, x_adv, ids, eps, self.seed, restart)
                else:
                    delta.zero_()
                    x_adv.copy_(k.box(x))
                for _ in range(self.steps):
                    v, g = value_and_grad(x_adv)
                    v = v.detach().float()
                    mask = v > best_value                               # NaN never improves; a tie keeps the earlier perturbation
                    best_value = torch.where(mask, v, best_value)
                    k.step(x, g.detach().float().contiguous(), delta, x_adv, best_delta, mask.contiguous(), eps, alpha)
                v = (value(x_adv) if value is not None else value_and_grad(x_adv)[0]).detach().float()
                mask = v > best_value
                best_value = torch.where(mask, v, best_value)
                best_delta = torch.where(mask.view(B, 1, 1, 1), delta, best_delta)          # the final select
            return {'delta': best_delta, 'x_adv': k.box(x + best_delta), 'value': best_value}


# ------------------------------------------------------------------------------------------------------------
# The model's side
# ------------------------------------------------------------------------------------------------------------
def _objective_names(stage: int):
    from .gradcam import TARGETS
    return CLASS_OBJECTIVES + tuple(n for n in TARGETS if n != 'class')


def _class_vector(v, B: int, classes: int, what: str, name: str, read_back: bool = True):
    """None, an int or a (B,) integer tensor -> None or a (B,) int64 tensor where it was given.  Raises before any launch.  A device
    tensor costs one host synchronisation for its range, unless ``read_back`` is False: then its values are clamped into range."""
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        if v.dtype.is_floating_point or v.dtype.is_complex or v.dtype == torch.bool:
            raise RovitHipError(f'{what}: {name} must be an integer tensor, got {v.dtype}')
        if tuple(v.shape) != (B,):
            raise RovitHipError(f'{what}: {name} must have shape ({B},), got {tuple(v.shape)}')
        if v.is_cuda and not read_back:
            return v.detach().long().clamp(0, classes - 1)
        lo, hi = int(v.min()), int(v.max())          # the one host synchronisation
        if lo < 0 or hi >= classes:
            raise RovitHipError(f'{what}: {name} values must be in [0, {classes}), got [{lo}, {hi}]')
        return v.detach().long()
    if not _is_int(v):
        raise RovitHipError(f'{what}: {name} must be None, an int or a (B,) integer tensor, got {type(v).__name__}')
    if not 0 <= v < classes:
        raise RovitHipError(f'{what}: {name} must be in [0, {classes}), got {v}')
    return torch.full((B,), int(v), dtype=torch.int64)


def _check_objective(model, x, labels, objective, target_class, direction, chunk, what, read_back: bool = True):
    """The checks objective_gradient, pgd_attack and robustness_radius share, in _check_args' order; the CUDA check comes last.
    Returns (labels, target_class) as (B,) int64 tensors on x's device, or None."""
    from .gradcam import TARGETS, _check_coverage
    from .input_grad import _check_phase
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or tuple(x.shape[1:]) != (3, 224, 224):
        raise RovitHipError(f'{what}: expects (B,3,224,224) images, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}')
    if x.shape[0] < 1:
        raise RovitHipError(f'{what}: empty batch')
    if not x.dtype.is_floating_point:
        raise RovitHipError(f'{what}: the images must be floating point, got {x.dtype}')
    names = _objective_names(model.curriculum_stage)
    if not isinstance(objective, str) or objective not in names:
        raise RovitHipError(f'{what}: objective must be one of {list(names)}, got {objective!r}')
    is_class = objective in CLASS_OBJECTIVES
    if not is_class and model.curriculum_stage < TARGETS[objective][1]:
        raise RovitHipError(f'{what}: objective {objective!r} needs curriculum stage {TARGETS[objective][1]}; at stage '
                            f'{model.curriculum_stage} forward() returns None for it')
    if direction not in (1, -1) or isinstance(direction, bool):
        raise RovitHipError(f'{what}: direction must be +1 or -1, got {direction!r}')
    if is_class and direction != 1:
        raise RovitHipError(f'{what}: direction belongs to the severity objectives; {objective!r} is always maximised')
    if not is_class and (labels is not None or target_class is not None):
        raise RovitHipError(f'{what}: labels / target_class belong to the class objectives, not to {objective!r}')
    if not _is_int(chunk) or chunk < 1:
        raise RovitHipError(f'{what}: chunk must be an int >= 1, got {chunk!r}')
    classes = model.classification_head.fc2.out_features
    B = x.shape[0]
    y = _class_vector(labels, B, classes, what, 'labels', read_back)
    t = _class_vector(target_class, B, classes, what, 'target_class', read_back)
    _check_coverage(model, [] if is_class else [objective])
    _check_phase(model, what)
    if not x.is_cuda:
        raise RovitHipError(f'{what}: the images must be on the GPU (there is no CPU fallback)')
    return (y.to(x.device) if y is not None else None), (t.to(x.device) if t is not None else None)


def objective_value(objective: str, outs, labels=None, target_class=None, direction: int = 1) -> torch.Tensor:
    """(B,) value of an attack objective on the head outputs ``(cls, ordinal, mu, log_var, kan)``; every objective is MAXIMISED.
    ``'ce'``: ``-log_softmax(z)[y]``, targeted ``+log_softmax(z)[t]``; ``'margin'``: ``max_{j != y} z_j - z_y``, targeted
    ``z_t - max_{j != t} z_j``; a severity output: ``direction`` times its value as ``input_grad._target_value`` defines it."""
    from .input_grad import _target_value
    if objective not in CLASS_OBJECTIVES:
        return float(direction) * _target_value(objective, outs, None)
    z = outs[0]
    c = (target_class if target_class is not None else labels).view(-1, 1)
    sign = 1.0 if target_class is not None else -1.0
    if objective == 'ce':
        return sign * torch.log_softmax(z, dim=1).gather(1, c).squeeze(1)
    own = z.gather(1, c).squeeze(1)
    other = z.masked_fill(torch.zeros_like(z, dtype=torch.bool).scatter_(1, c, True), -math.inf).max(dim=1).values
    return sign * (own - other)


class _Route:
    """The gradient route of one attack: the backbone calls of input_grad._Backbone, the head phase and the objective."""

    def __init__(self, model, dev, objective, labels, target_class, direction, chunk):
        from .input_grad import _Backbone
        self.model, self.bb = model, _Backbone(model, dev)
        self.objective, self.y, self.t, self.direction, self.chunk = objective, labels, target_class, direction, chunk

    def _value(self, outs, b0, b1):
        y = self.y[b0:b1] if self.y is not None else None
        t = self.t[b0:b1] if self.t is not None else None
        return objective_value(self.objective, outs, y, t, self.direction)

    def outputs(self, x):
        """The head outputs of an inference forward, chunked: what forward() in eval mode returns for x."""
        from .input_grad import _head_outputs
        parts = []
        with torch.no_grad():
            for b0 in range(0, x.shape[0], self.chunk):
                feats, _ = self.bb.features(x[b0:b0 + self.chunk], False)
                parts.append(_head_outputs(self.model, feats))
        return tuple(torch.cat([p[i] for p in parts]) if parts[0][i] is not None else None for i in range(len(parts[0])))

    def value(self, x):
        """(B,) objective value from the same training-mode forward as value_and_grad, so that the two compare bit for bit."""
        from .input_grad import _head_outputs
        out = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
        with torch.no_grad():
            for b0 in range(0, x.shape[0], self.chunk):
                b1 = min(x.shape[0], b0 + self.chunk)
                feats, ws = self.bb.features(x[b0:b1], True)
                self.bb.eng.give_ws(b1 - b0, True, ws)
                out[b0:b1] = self._value(_head_outputs(self.model, feats), b0, b1)
        return out

    def value_and_grad(self, x):
        from .input_grad import _head_outputs
        B = x.shape[0]
        val = torch.empty(B, device=x.device, dtype=torch.float32)
        grad = torch.empty(B, 3, 224, 224, device=x.device, dtype=torch.float32)
        for b0 in range(0, B, self.chunk):
            b1 = min(B, b0 + self.chunk)
            with torch.no_grad():
                feats, ws = self.bb.features(x[b0:b1], True)
            with torch.enable_grad():
                f = feats.detach().requires_grad_(True)
                v = self._value(_head_outputs(self.model, f), b0, b1)
                g, = torch.autograd.grad(v.sum(), f)
            with torch.no_grad():
                val[b0:b1] = v.detach()
                self.bb.pixels(x[b0:b1], ws, g.contiguous(), grad[b0:b1], 1, 1.0, 0)
        return val, grad


def objective_gradient(model, x: torch.Tensor, labels=None, objective: str = 'ce', target_class=None, direction: int = 1, chunk: int = 256):
    """``(value (B,), grad (B,3,224,224))`` of an attack objective (``objective_value``) with respect to the normalised images: the
    fused forward that keeps the activations, the head phase, the objective in torch on the head outputs, autograd down to the
    features, the dgrad chain alone down to the pixels.  ``labels=None`` uses the model's own prediction at ``x``; ``target_class``
    (an int or a (B,) tensor) makes a class objective targeted.  Eval semantics and the side-effect contract of ``input_gradients``: no
    ``.grad`` written, flags untouched, workspaces of its own; the same models.  Refuses every bad argument before any launch."""
    y, t = _check_objective(model, x, labels, objective, target_class, direction, chunk, 'objective_gradient')
    x32 = x.detach().float().contiguous()
    route = _Route(model, x.device, objective, y, t, direction, chunk)
    if objective in CLASS_OBJECTIVES and y is None and t is None:
        route.y = route.outputs(x32)[0].argmax(dim=1)
    return route.value_and_grad(x32)


def _attack_args(what, norm, eps, steps, step_size, random_start, restarts, seed, mean, std, clip):
    try:
        return PGD(norm, eps, steps, step_size, random_start, restarts, seed, mean, std, clip)
    except RovitHipError as e:
        raise RovitHipError(f'{what}: {e}') from None


def _outputs_dict(outs):
    return {k: v for k, v in zip(('cls_logits', 'ordinal_logits', 'mu', 'log_var', 'kan_severity'), outs) if v is not None}


def pgd_attack(model, x: torch.Tensor, labels=None, *, objective: str = 'ce', target_class=None, direction: int = 1, norm: str = 'linf',
               eps=8 / 255, steps: int = 10, step_size=None, random_start: bool = True, restarts: int = 1, seed: int = 0, ids=None,
               mean=None, std=None, clip=(0., 1.), chunk: int = 256, return_info: bool = False, check_labels: bool = True):
    """Adversarial images of ``x`` (B,3,224,224, normalised) inside the ``norm`` ball of radius ``eps`` (pixel units) and the pixel
    range ``clip``: ``PGD`` on ``objective_gradient``.  ``labels=None`` attacks the model's own prediction at ``x``.  Returns
    ``x_adv``; with ``return_info`` also a dict: ``delta`` (normalised units; ``x_adv - x`` up to one rounding of ``x``),
    ``value_clean`` and ``value`` (the objective at ``x`` and at ``x_adv``, the best value seen: both from the training-mode forward
    the loop itself runs, so ``value >= value_clean`` holds exactly without a random start), ``outputs`` (the head outputs of an
    inference forward of ``x_adv``: what ``forward()`` in eval mode and ``predict()`` see; the training-mode forward is not assumed to
    give the same bits, so this is one more forward) and, for the class objectives, ``labels`` and ``success`` (untargeted: argmax !=
    label; targeted: argmax == target).  K steps cost K gradient calls and three forwards.  ``check_labels=False``: labels on the
    device are not read back for their range check but clamped into range (the score card's loop, which reads nothing back).  The side-effect contract of
    ``input_gradients``; every bad argument is refused (RovitHipError) before anything is launched."""
    what = 'pgd_attack'
    pgd = _attack_args(what, norm, eps, steps, step_size, random_start, restarts, seed, mean, std, clip)
    _check_images_only(x, what)
    try:
        pgd.check(x, ids)
    except RovitHipError as e:
        raise RovitHipError(f'{what}: {e}') from None
    y, t = _check_objective(model, x, labels, objective, target_class, direction, chunk, what, bool(check_labels))
    with torch.no_grad():
        x32 = x.detach().float().contiguous()
        route = _Route(model, x.device, objective, y, t, direction, chunk)
        is_class = objective in CLASS_OBJECTIVES
        if is_class and y is None and t is None:
            route.y = route.outputs(x32)[0].argmax(dim=1)
        res = pgd(route.value_and_grad, x32, ids, route.value)
        if not return_info:
            return res['x_adv']
        outs = route.outputs(res['x_adv'])
        info = {'delta': res['delta'], 'value_clean': route.value(x32), 'value': res['value'], 'outputs': _outputs_dict(outs)}
        if is_class:
            pred = outs[0].argmax(dim=1)
            info['labels'] = route.y if route.t is None else route.t
            info['success'] = (pred == route.t) if route.t is not None else (pred != route.y)
        return res['x_adv'], info


def _check_images_only(x, what):
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or tuple(x.shape[1:]) != (3, 224, 224):
        raise RovitHipError(f'{what}: expects (B,3,224,224) images, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}')
    if x.shape[0] < 1:
        raise RovitHipError(f'{what}: empty batch')


def robustness_radius(model, x: torch.Tensor, labels, norm: str = 'linf', eps_max: float = 8 / 255, search_steps: int = 8, steps: int = 10,
                      *, objective: str = 'margin', step_size=None, random_start: bool = False, restarts: int = 1, seed: int = 0, ids=None,
                      mean=None, std=None, clip=(0., 1.), chunk: int = 256):
    """Per image, the smallest radius (pixel units) at which ``pgd_attack`` changes the class away from ``labels``: a bisection over
    eps for all images at once, each with its own ``eps_b`` in one batch.  An image whose clean prediction differs from its label has
    radius 0.  One attack at ``eps_max`` comes first; an image it does not break gets ``radius = inf``, meaning "> eps_max as far as this
    attack can tell".  Then ``search_steps`` halvings of ``[lower, radius]``; finished images ride along with ``eps_b = 0``.  All
    bookkeeping is ``torch.where`` on the device.  Returns ``{'radius', 'lower', 'broken', 'x_adv'}``: ``broken`` marks the images the
    search ran on (correct when clean, broken at ``eps_max``); ``lower`` is the largest radius tried that did not break the image
    (``eps_max`` for unbroken ones, 0 for misclassified ones); ``x_adv`` is the adversarial image found at ``radius`` (``x`` itself where
    none was found or needed).

    ``radius`` is an UPPER bound on the true minimal adversarial radius: a stronger attack may break the image closer in, and PGD is not
    monotone in eps, so ``lower`` is not a certificate either."""
    what = 'robustness_radius'
    if not _is_number(eps_max) or not math.isfinite(eps_max) or eps_max <= 0:
        raise RovitHipError(f'{what}: eps_max must be a finite number > 0, got {eps_max!r}')
    if not _is_int(search_steps) or search_steps < 0:
        raise RovitHipError(f'{what}: search_steps must be an int >= 0, got {search_steps!r}')
    pgd = _attack_args(what, norm, float(eps_max), steps, step_size, random_start, restarts, seed, mean, std, clip)
    if objective not in CLASS_OBJECTIVES:
        raise RovitHipError(f'{what}: objective must be one of {list(CLASS_OBJECTIVES)}, got {objective!r}')
    if labels is None:
        raise RovitHipError(f'{what}: needs the true labels (an int or a (B,) integer tensor)')
    _check_images_only(x, what)
    try:
        pgd.check(x, ids)
    except RovitHipError as e:
        raise RovitHipError(f'{what}: {e}') from None
    y, _ = _check_objective(model, x, labels, objective, None, 1, chunk, what)
    with torch.no_grad():
        dev, B = x.device, x.shape[0]
        x32 = x.detach().float().contiguous()
        route = _Route(model, dev, objective, y, None, 1, chunk)
        correct = route.outputs(x32)[0].argmax(dim=1) == y
        f32 = lambda v: torch.full((B,), v, dtype=torch.float32, device=dev)
        zero, top, inf = f32(0.0), f32(float(eps_max)), f32(math.inf)

        def attack(eps_b):
            pgd.eps = eps_b
            xa = pgd(route.value_and_grad, x32, ids, route.value)['x_adv']
            return xa, route.outputs(xa)[0].argmax(dim=1) != y

        xa, hit = attack(torch.where(correct, top, zero))
        broken = correct & hit
        high, low = top.clone(), zero.clone()
        x_best = torch.where(broken.view(B, 1, 1, 1), xa, x32)
        for _ in range(search_steps):
            mid = (low + high) * 0.5
            xa, hit = attack(torch.where(broken, mid, zero))
            hit = hit & broken
            high = torch.where(hit, mid, high)
            low = torch.where(broken & ~hit, mid, low)
            x_best = torch.where(hit.view(B, 1, 1, 1), xa, x_best)
        radius = torch.where(broken, high, torch.where(correct, inf, zero))
        lower = torch.where(broken, low, torch.where(correct, top, zero))
        return {'radius': radius, 'lower': lower, 'broken': broken, 'x_adv': x_best}
