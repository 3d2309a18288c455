"""Image corruptions of a device-resident uint8 image store (csrc/corrupt.hip): the corruption step of a corruption-robustness
benchmark -- fixed corruptions at five severities, one score card per cell (Hendrycks & Dietterich, "Benchmarking Neural Network
Robustness to Common Corruptions and Perturbations", ICLR 2019, "ImageNet-C") -- as ONE launch per batch from the uint8 store
(``contrast`` needs a second one, the integer plane sums).  The output is at the store's own resolution: nothing is resampled.

The severity tables are ImageNet-C's where the operation has a parameter of the same meaning (``gaussian_noise``, ``shot_noise``,
``impulse_noise``, ``gaussian_blur``, ``brightness``, ``contrast``, ``jpeg``) and otherwise this repository's own; ImageNet-C's
generator also works at its own resolution and with skimage / PIL / wand, so no number here is comparable with a published one --
"parity unpinned", like ``augment.py``.  An explicit ``param=`` overrides the table.

The corruptions (specification of record)
-----------------------------------------
``src[idx[n]]`` (3, H, W) uint8 gives ``out[n]`` (3, H, W) fp32, any H, W >= 8.  All arithmetic is on ``v = u8 / 255`` per channel
unless stated otherwise; the result is ``z = clamp(., 0, 1)``, then ``out = (z - mean_c) / std_c`` with the ImageNet constants.  The fp32
output is NOT quantised to 8 bits; ``out_u8``, when asked for, is ``floor(255 z + 0.5)``.  ``id`` is the name's position in
``CORRUPTIONS``; the parameter is rounded to fp32 once (the value the C struct carries) before anything is computed from it.

===============  ==========================================================================================  =========================
name (id)        definition                                                                                  severity 1..5
===============  ==========================================================================================  =========================
gaussian_noise   v + sigma n, n standard normal                                                              sigma = .08 .12 .18 .26 .38
shot_noise       v + sqrt(v / c) n: the NORMAL APPROXIMATION of Poisson(c v) / c, not a Poisson draw         c = 60 25 12 5 3
impulse_noise    per pixel and channel: u < p/2 -> 0;  u >= 1 - p/2 -> 1;  else v                            p = .03 .06 .09 .17 .27
gaussian_blur    2-D product of normalised 1-D weights ~ exp(-k^2 / 2 sigma^2), k in [-R, R],                sigma = 1 2 3 4 6
                 R = ceil(3 sigma); edges replicate
defocus_blur     equal weights on dx^2 + dy^2 <= r^2, normalised; edges replicate                            r = 3 4 6 8 10
motion_blur      mean of 2R + 1 BILINEAR samples at (x + k cos theta, y + k sin theta), k = -R..R;           R = 3 5 7 10 14
                 theta = 2 pi u, one draw per image
brightness       v + c                                                                                       c = .1 .2 .3 .4 .5
contrast         m_c + c (v - m_c), m_c the channel mean over the image = integer sum / (255 H W)            c = .4 .3 .2 .1 .05
saturate         g + s (v - g), g = .299 R + .587 G + .114 B                                                 s = .6 .4 .2 .1 0
pixelate         every pixel takes the mean of its b x b cell (cells start at 0 and are clipped at the       b = 2 3 4 6 8
                 image edge): integer sum / (255 count)
jpeg             baseline JPEG round trip, 4:4:4, in integers (below)                                        quality = 25 18 15 10 7
===============  ==========================================================================================  =========================

``contrast`` and ``saturate`` are evaluated as ``v + (1 - c)(m - v)`` and ``v + (1 - s)(g - v)``, so that c = 1 and s = 1 are the
identity to the bit.  A motion-blur sample's coordinates are clamped like the augmentation's taps: ``sx`` to [0, W - 1], ``sy`` to
[0, H - 1], the four taps at ``floor`` and ``floor + 1`` (the upper one clamped to the last row / column).  The Gaussian and the motion
blur are evaluated as the centre value plus the weighted differences to it (the weights sum to one) and the disk as an integer sum over
``255 count``, so that every blur leaves a constant image unchanged to the bit.  Limits: ceil(3 sigma) <= 18,
r <= 18, R <= 17, 1 <= b <= 64, 1 <= quality <= 100 (R, b and quality integers).

Draws.  Philox4x32-10 (``oracle.philox``), key = ``seed``.  One call per pixel, counter = ``(y W + x, index in the STORE, id, 0)``;
``u = (word >> 8) 2^-24``.  The normals are Box-Muller with ``u1 = ((word >> 8) + 1) 2^-24`` in the logarithm: ``n_R = sqrt(-2 ln
u1(x)) cos(2 pi u(y))``, ``n_G`` the sine branch of the same pair, ``n_B = sqrt(-2 ln u1(z)) cos(2 pi u(w))``.  Impulse noise: words x,
y, z serve R, G, B, and the two thresholds ``p/2`` and ``1 - p/2`` are fp32 values compared with the exact ``u``, so the mask is exact.
The motion blur's ``theta = 2 pi u(x)`` comes from the counter ``(index in the STORE, 0, id, 1)``.  The counter holds the image's index
in the STORE, not its position in the batch, and a pixel's arithmetic depends on nothing else: a corrupted image has the same bits for
every batch size, order and split.  The plane sums of ``contrast`` are the one cross-thread reduction, and they are integer sums: there
is no floating-point atomic in the kernels, so every output is also bit-identical from run to run.

``jpeg`` -- integers end to end, so kernel and oracle agree bit for bit:

1. RGB -> YCbCr with libjpeg's 16-bit fixed point: ``Y = (19595 R + 38470 G + 7471 B + 32768) >> 16``, ``Cb = (-11059 R - 21709 G +
   32768 B + (128 << 16) + 32767) >> 16``, ``Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16``; level shift by -128.
2. ``M[u][x] = rint(8192 a(u) cos((2x + 1) u pi / 16))``, a(0) = sqrt(1/8), a(u) = 1/2.  Forward transform of each 8 x 8 block:
   ``t = M block`` (along y), ``t <- (t + 512) >> 10``, ``c = t M^T`` (along x; scale 2^16).
3. ``q = sign(c) ((|c| + (Q << 15)) / (Q << 16))`` (integer division), ``d = q Q``.  Q is the Annex-K luminance table for Y and the
   chrominance table for Cb, Cr, scaled by libjpeg's quality rule: ``s = 5000 / quality`` below 50, else ``200 - 2 quality``;
   ``Q = clamp((base s + 50) / 100, 1, 255)``.
4. Inverse transform in the same two passes with the same descale: ``w = M^T d`` (along u), ``(w + 512) >> 10``, ``r = w M`` (along v);
   ``level = clamp(((r + 32768) >> 16) + 128, 0, 255)``.
5. ``R = Y + ((91881 (Cr - 128) + 32768) >> 16)``, ``G = Y + ((-22554 (Cb - 128) - 46802 (Cr - 128) + 32768) >> 16)``,
   ``B = Y + ((116130 (Cb - 128) + 32768) >> 16)``, clamped to 0..255; ``z = level / 255``.

Every shift is arithmetic (floor); every intermediate fits int32.  Sides that are no multiple of 8 are edge-replicated up to the next
multiple and cropped afterwards; there is no entropy coding (it is lossless).  tests/test_corrupt_cpu.py pins this rule to PIL's encoder
(``quality=q, subsampling=0``): the mean absolute difference is below one level where the codec's own distortion is 5 to 60.

Store indices.  The kernels never dereference an index outside [0, N): such a sample's output is NaN.  Index lists that come from the
host are checked on the host when they are uploaded; a device tensor is not read back.

``corrupt_reference`` is the numpy statement of all of the above (fp64 for the float corruptions, int64 for ``jpeg`` and the integer
sums): the oracle of the tests, and what a store on the CPU runs through the same entry point.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import native
from .augment import IMAGENET_MEAN, IMAGENET_STD, DeviceImageStore
from .native import RovitHipError, call, ptr, stream_ptr

CORRUPTIONS = ('gaussian_noise', 'shot_noise', 'impulse_noise', 'gaussian_blur', 'defocus_blur', 'motion_blur', 'brightness', 'contrast',
               'saturate', 'pixelate', 'jpeg')
SEVERITY_TABLE = {
    'gaussian_noise': (.08, .12, .18, .26, .38),
    'shot_noise': (60., 25., 12., 5., 3.),
    'impulse_noise': (.03, .06, .09, .17, .27),
    'gaussian_blur': (1., 2., 3., 4., 6.),
    'defocus_blur': (3., 4., 6., 8., 10.),
    'motion_blur': (3., 5., 7., 10., 14.),
    'brightness': (.1, .2, .3, .4, .5),
    'contrast': (.4, .3, .2, .1, .05),
    'saturate': (.6, .4, .2, .1, 0.),
    'pixelate': (2., 3., 4., 6., 8.),
    'jpeg': (25., 18., 15., 10., 7.),
}
MAX_RADIUS = native.CORRUPT_MAX_RADIUS
JPEG_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
JPEG_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, dtype=np.int64).reshape(8, 8)


def corruption_id(name: str) -> int:
    if name not in CORRUPTIONS:
        raise RovitHipError(f'unknown corruption {name!r}: one of {", ".join(CORRUPTIONS)}')
    return CORRUPTIONS.index(name)


def corruption_param(name: str, severity: int) -> float:
    """The table's parameter of ``name`` at ``severity`` 1..5."""
    corruption_id(name)
    if isinstance(severity, bool) or not isinstance(severity, (int, np.integer)) or not 1 <= int(severity) <= 5:
        raise RovitHipError(f'severity must be an integer in 1..5, got {severity!r}')
    return float(SEVERITY_TABLE[name][int(severity) - 1])


def _resolve(name: str, severity: int, param) -> float:
    """The fp32 parameter value (as a Python float) after the range checks the C entry point repeats."""
    p = corruption_param(name, severity) if param is None else float(param)
    corruption_id(name)
    p = float(np.float32(p))
    whole = p == math.floor(p) if math.isfinite(p) else False
    ok = {'gaussian_noise': p >= 0, 'shot_noise': p > 0, 'impulse_noise': 0 <= p <= 1,
          'gaussian_blur': p > 0 and math.ceil(3.0 * p) <= MAX_RADIUS, 'defocus_blur': 0 <= p <= MAX_RADIUS,
          'motion_blur': whole and 0 <= p <= MAX_RADIUS - 1, 'brightness': True, 'contrast': True, 'saturate': True,
          'pixelate': whole and 1 <= p <= 64, 'jpeg': whole and 1 <= p <= 100}[name]
    if not (math.isfinite(p) and ok):
        raise RovitHipError(f'{name}: parameter {p!r} outside its range (see the module docstring)')
    return p


# ------------------------------------------------------------------------------------------------------------
# The reference
# ------------------------------------------------------------------------------------------------------------
def jpeg_tables(quality: int):
    """The two quantisation tables (8, 8) int64 at ``quality``: Annex K scaled by libjpeg's rule."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (JPEG_LUMA, JPEG_CHROMA))


def dct_matrix() -> np.ndarray:
    u, x = np.arange(8, dtype=np.float64).reshape(8, 1), np.arange(8, dtype=np.float64).reshape(1, 8)
    a = np.where(u == 0, math.sqrt(0.125), 0.5)
    return np.rint(8192.0 * a * np.cos((2 * x + 1) * u * math.pi / 16.0)).astype(np.int64)


def jpeg_levels(images_u8: np.ndarray, quality: int, dtype=np.int64) -> np.ndarray:
    """The integer codec of the module docstring on (B, 3, H, W) uint8: the decoded levels, same shape and dtype.  ``dtype``: the integer
    type of every intermediate (int32 is what the kernel uses; numpy wraps silently, so equal results show that nothing overflows)."""
    B, _, H, W = images_u8.shape
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    rgb = np.pad(images_u8.astype(dtype), ((0, 0), (0, 0), (0, Hp - H), (0, Wp - W)), mode='edge')
    R, G, Bl = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    ycc = np.stack([(19595 * R + 38470 * G + 7471 * Bl + 32768) >> 16,
                    (-11059 * R - 21709 * G + 32768 * Bl + (128 << 16) + 32767) >> 16,
                    (32768 * R - 27439 * G - 5329 * Bl + (128 << 16) + 32767) >> 16], axis=1) - 128
    blocks = ycc.reshape(B, 3, Hp // 8, 8, Wp // 8, 8).transpose(0, 1, 2, 4, 3, 5)          # (B, 3, by, bx, y, x)
    M = dct_matrix().astype(dtype)
    luma, chroma = jpeg_tables(quality)
    Q = np.stack([luma, chroma, chroma]).astype(dtype).reshape(1, 3, 1, 1, 8, 8)
    t = (M @ blocks + 512) >> 10
    c = t @ M.T
    q = np.sign(c) * ((np.abs(c) + (Q << 15)) // (Q << 16))
    d = q * Q
    w = (M.T @ d + 512) >> 10
    r = w @ M
    lev = np.clip(((r + 32768) >> 16) + 128, 0, 255)
    lev = lev.transpose(0, 1, 2, 4, 3, 5).reshape(B, 3, Hp, Wp)[:, :, :H, :W]
    Y, Cb, Cr = lev[:, 0], lev[:, 1] - 128, lev[:, 2] - 128
    out = np.stack([Y + ((91881 * Cr + 32768) >> 16), Y + ((-22554 * Cb - 46802 * Cr + 32768) >> 16), Y + ((116130 * Cb + 32768) >> 16)], axis=1)
    return np.clip(out, 0, 255).astype(np.uint8)


def _words(c0, c1, c2, c3, seed: int):
    from oracle.philox import philox4x32_10 as philox          # checker only, like draw_params_reference
    n = np.broadcast(c0, c1).size
    full = lambda v: np.broadcast_to(np.asarray(v, dtype=np.uint64), (n,)).copy()
    return philox([full(c0), full(c1), full(c2), full(c3)], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])


def motion_theta(indices, seed: int, dtype=np.float64) -> np.ndarray:
    """``theta`` of ``motion_blur`` for store indices ``indices``, in ``dtype``."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    w = _words((idx & 0xFFFFFFFF).astype(np.uint64), 0, corruption_id('motion_blur'), 1, seed)
    return dtype(2.0 * math.pi) * ((w[0] >> np.uint64(8)).astype(dtype) * dtype(1.0 / 16777216.0))


def _shifted_sum(v: np.ndarray, taps, halo: int) -> np.ndarray:
    """sum over (dy, dx, weight) of weight * (v shifted - v), with replicated edges; v (3, H, W)."""
    H, W = v.shape[-2:]
    pad = np.pad(v, ((0, 0), (halo, halo), (halo, halo)), mode='edge')
    acc = np.zeros_like(v)
    for dy, dx, wgt in taps:
        acc += wgt * (pad[:, halo + dy:halo + dy + H, halo + dx:halo + dx + W] - v)
    return acc


def _corrupt_one(u8: np.ndarray, image: int, name: str, p: float, seed: int, T) -> np.ndarray:
    """z (3, H, W) in dtype ``T`` before the clamp, of one image (3, H, W) uint8 with store index ``image``."""
    kind = corruption_id(name)
    _, H, W = u8.shape
    v = u8.astype(T) / T(255.0)
    p = T(p)
    one = T(1.0)
    if name in ('gaussian_noise', 'shot_noise', 'impulse_noise'):
        w = _words(np.arange(H * W, dtype=np.uint64), image & 0xFFFFFFFF, kind, 0, seed)
        scale = T(1.0 / 16777216.0)
        u = [(x >> np.uint64(8)).astype(T).reshape(H, W) * scale for x in w]
        if name == 'impulse_noise':
            lo = np.float32(p) * np.float32(0.5)
            hi = np.float32(1.0) - lo
            z = v.copy()
            for c in range(3):
                uc = (w[c] >> np.uint64(8)).astype(np.float64).reshape(H, W) / 16777216.0          # exact
                z[c] = np.where(uc < np.float64(lo), T(0.0), np.where(uc >= np.float64(hi), one, v[c]))
            return z
        u1 = [((x >> np.uint64(8)) + np.uint64(1)).astype(T).reshape(H, W) * scale for x in w]
        two_pi = T(2.0 * math.pi)
        r0, r1 = np.sqrt(T(-2.0) * np.log(u1[0])), np.sqrt(T(-2.0) * np.log(u1[2]))
        n = np.stack([r0 * np.cos(two_pi * u[1]), r0 * np.sin(two_pi * u[1]), r1 * np.cos(two_pi * u[3])]).astype(T)
        return v + p * n if name == 'gaussian_noise' else v + np.sqrt(v / p) * n
    if name == 'brightness':
        return v + p
    if name == 'contrast':
        m = (u8.astype(np.int64).sum(axis=(1, 2)).astype(T) / T(255.0 * H * W)).reshape(3, 1, 1)
        return v + (one - p) * (m - v)
    if name == 'saturate':
        g = T(0.299) * v[0] + T(0.587) * v[1] + T(0.114) * v[2]
        return v + (one - p) * (g[None] - v)
    if name == 'pixelate':
        b = int(p)
        ys, xs = np.arange(0, H, b), np.arange(0, W, b)
        sums = np.add.reduceat(np.add.reduceat(u8.astype(np.int64), ys, axis=1), xs, axis=2)
        count = np.add.reduceat(np.add.reduceat(np.ones((H, W), np.int64), ys, axis=0), xs, axis=1)
        cell = sums.astype(T) / (T(255.0) * count.astype(T))
        return cell[:, np.arange(H)[:, None] // b, np.arange(W)[None, :] // b]
    if name == 'gaussian_blur':
        R = int(math.ceil(3.0 * float(p)))
        k = np.arange(-R, R + 1).astype(T)
        w1 = np.exp(-(k * k) / (T(2.0) * p * p))
        w1 = w1 / w1.sum()
        rows = v + _shifted_sum(v, [(0, dx, w1[dx + R]) for dx in range(-R, R + 1)], R)          # the 2-D product, one axis at a time
        return rows + _shifted_sum(rows, [(dy, 0, w1[dy + R]) for dy in range(-R, R + 1)], R)
    if name == 'defocus_blur':
        R = int(math.floor(float(p)))
        r2 = float(p) * float(p)
        taps = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if dx * dx + dy * dy <= r2]
        pad = np.pad(u8.astype(np.int64), ((0, 0), (R, R), (R, R)), mode='edge')
        total = sum(pad[:, R + dy:R + dy + H, R + dx:R + dx + W] for dy, dx in taps)          # equal weights: an integer sum
        return total.astype(T) / T(255.0 * len(taps))
    if name == 'motion_blur':
        R = int(p)
        theta = motion_theta([image], seed, T)[0]
        cs, sn = np.cos(theta), np.sin(theta)
        xs, ys = np.arange(W).astype(T)[None, :], np.arange(H).astype(T)[:, None]
        flat = v.reshape(3, H * W)
        acc = np.zeros_like(v)
        for k in range(-R, R + 1):
            sx = np.clip(xs + T(k) * cs, T(0.0), T(W - 1)) + np.zeros((H, 1), T)
            sy = np.clip(ys + T(k) * sn, T(0.0), T(H - 1)) + np.zeros((1, W), T)
            x0f, y0f = np.floor(sx), np.floor(sy)
            fx, fy = sx - x0f, sy - y0f
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
            x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
            tap = lambda yy, xx: flat[:, (yy * W + xx).reshape(-1)].reshape(3, H, W)
            top = tap(y0, x0) + fx * (tap(y0, x1) - tap(y0, x0))
            bot = tap(y1, x0) + fx * (tap(y1, x1) - tap(y1, x0))
            acc += (top + fy * (bot - top)) - v
        return v + acc / T(2 * R + 1)
    raise RovitHipError(f'unknown corruption {name!r}')


def corrupt_reference(images_u8, indices, corruption: str, severity: int = 3, seed: int = 0, param=None, *, dtype=np.float64,
                      return_u8: bool = False):
    """The module docstring in numpy: (B, 3, H, W) ``dtype`` (fp64; fp32 restates the same formulas in the kernel's precision, which is
    how the tests' bounds are set) for store indices ``indices`` of ``images_u8`` (N, 3, H, W) uint8 (numpy or torch, any device).
    ``return_u8``: also ``floor(255 z + 0.5)`` as uint8."""
    p = _resolve(corruption, severity, param)
    src = images_u8.detach().cpu().numpy() if isinstance(images_u8, torch.Tensor) else np.asarray(images_u8)
    if src.dtype != np.uint8 or src.ndim != 4 or src.shape[1] != 3 or min(src.shape[2:]) < 8:
        raise RovitHipError(f'corrupt_reference expects uint8 (N, 3, H >= 8, W >= 8), got {src.dtype} {src.shape}')
    idx = np.asarray(indices.detach().cpu().numpy() if isinstance(indices, torch.Tensor) else indices, dtype=np.int64).reshape(-1)
    if idx.size == 0 or idx.min() < 0 or idx.max() >= src.shape[0]:
        raise RovitHipError(f'corrupt_reference: empty index list, or an index outside [0, {src.shape[0]})')
    T = np.dtype(dtype).type
    if corruption == 'jpeg':
        z = jpeg_levels(src[idx], int(p)).astype(T) / T(255.0)
    else:
        z = np.stack([_corrupt_one(src[i], int(i), corruption, p, int(seed), T) for i in idx]).astype(T)
    z = np.clip(z, T(0.0), T(1.0))
    mean, std = (np.array(t, dtype=T).reshape(1, 3, 1, 1) for t in (IMAGENET_MEAN, IMAGENET_STD))
    out = (z - mean) / std
    return (out, np.floor(T(255.0) * z + T(0.5)).astype(np.uint8)) if return_u8 else out


# ------------------------------------------------------------------------------------------------------------
# The entry point
# ------------------------------------------------------------------------------------------------------------
def corrupt(store: DeviceImageStore, indices, corruption: str, severity: int = 3, seed: int = 0, param=None,
            out: Optional[torch.Tensor] = None, return_u8: bool = False):
    """fp32 (B, 3, H, W) at the store's resolution: images ``indices`` (sequence, CPU or device int64 tensor) of ``store`` under
    ``corruption`` at ``severity`` 1..5 (or with the explicit ``param``), normalised with the ImageNet constants.  One launch (two for
    ``contrast``).  ``out``: an fp32 tensor to write into; ``return_u8``: also the quantised uint8 image.  A store on the CPU runs
    ``corrupt_reference``."""
    p = _resolve(corruption, severity, param)
    kind = corruption_id(corruption)
    N, _, H, W = store.images.shape
    if H < 8 or W < 8:
        raise RovitHipError(f'corrupt: the store\'s images are {H} x {W}; both sides must be >= 8')
    idx = store.upload_indices(indices)
    B = int(idx.numel())
    if B == 0:
        raise RovitHipError('empty batch')
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != (B, 3, H, W) or out.device != store.device):
        raise RovitHipError(f'out must be fp32 ({B}, 3, {H}, {W}) on the store\'s device')
    if not store.images.is_cuda:
        ref, u8 = corrupt_reference(store.images, idx, corruption, seed=seed, param=p, return_u8=True)
        res = torch.from_numpy(ref).to(torch.float32)
        if out is not None:
            res = out.copy_(res)
        return (res, torch.from_numpy(u8)) if return_u8 else res
    if out is None:
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=store.device)
    u8 = torch.empty(B, 3, H, W, dtype=torch.uint8, device=store.device) if return_u8 else None
    sums = None
    if corruption == 'contrast':
        sums = torch.empty(B, 3, dtype=torch.int64, device=store.device)
        call('rovit_corrupt_stats', ptr(store.images), N, H, W, ptr(idx), B, ptr(sums), stream_ptr())
    desc = native.CorruptionC(kind, p, int(seed) & 0xFFFFFFFFFFFFFFFF)
    call('rovit_corrupt_batch', ptr(store.images), N, H, W, ptr(idx), B, C.addressof(desc), ptr(sums), ptr(out), ptr(u8), stream_ptr())
    return (out, u8) if return_u8 else out
