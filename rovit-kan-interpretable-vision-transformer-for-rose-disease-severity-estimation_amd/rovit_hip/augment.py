"""Device-resident uint8 image store and the fused per-sample augmentation kernel (csrc/augment_batch.hip).

The data set is decoded ONCE, kept on the device as uint8 (20 000 images at 224 x 224 are 3.0 GB), and one launch per batch does the
rest: gather by index, draw each sample's augmentation, resample, colour-transform, normalise, write the fp32 NCHW batch the backbone
reads.  The reference's ``data/transforms.py`` is not part of its checkout (its README promises "color jitter, random flips"), so WHAT
is augmented is this repository's own definition -- "parity unpinned", like ``cutmix_or_mixup`` in data/transforms.py.  The colour
part is the DALI "ColorTwist" form, NOT torchvision's ColorJitter: the order of the four operations is fixed and contrast pivots on
0.5, not on the image's grey mean, so no per-image reduction is needed and the kernel stays single-pass.

The transform (specification of record)
---------------------------------------
Sample ``n`` of a batch has a row of 12 floats ``[flip_h, flip_v, area, log_ratio, ux, uy, theta, brightness, contrast, saturation,
hue, 0]`` and produces ``out[n]`` (3, Ho, Wo) fp32 from ``src[idx[n]]`` (3, Hs, Ws) uint8.

Geometry -- a crop in the spirit of RandomResizedCrop (no retry loop), a rotation and flips as ONE affine map::

    r = exp(log_ratio);   w = min(Ws, Ws sqrt(area r));   h = min(Hs, Hs sqrt(area / r))
    cx = ux (Ws - w) + w / 2;   cy = uy (Hs - h) + h / 2
    dx = ((j + 0.5) / Wo - 0.5) w (1 - 2 flip_h);   dy = ((i + 0.5) / Ho - 0.5) h (1 - 2 flip_v)
    sx = cx + cos(theta) dx - sin(theta) dy - 0.5;   sy = cy + sin(theta) dx + cos(theta) dy - 0.5

``sx`` is clamped to [0, Ws - 1] and ``sy`` to [0, Hs - 1]; the four taps are at ``floor`` and ``floor + 1`` (the upper one clamped to
the last row / column) with the fractional parts as weights, on pixel values ``u8 / 255``; no antialiasing.  This is
``F.grid_sample(mode='bilinear', padding_mode='border', align_corners=False)`` on the same grid.  With rows down and columns to the
right, ``theta = +pi/2`` on a square source at ``area = 1`` is ``torch.rot90(image, 1, (-2, -1))``: the displayed image turns a
quarter COUNTER-clockwise.

Colour -- one affine transform and one clamp per pixel::

    T = [[0.299, 0.587, 0.114], [0.5959, -0.2746, -0.3213], [0.2115, -0.5227, 0.3112]]        (NTSC RGB -> YIQ)
    A = inv(T) diag(1, saturation Rot(2 pi hue)) T,    Rot(a) = [[cos a, -sin a], [sin a, cos a]]
    z = clamp(brightness (0.5 + contrast (A v - 0.5)), 0, 1);    out = (z - mean_c) / std_c         (ImageNet constants)

Draws -- without explicit rows the kernel draws them from Philox4x32-10, key = ``seed``, counter = ``(index in the store, r,
epoch lo, epoch hi)`` for r = 0, 1, 2, ``u = (word >> 8) 2^-24`` in fp32::

    r = 0:  x -> flip_h = u < p_hflip    y -> flip_v = u < p_vflip    z -> area = s0 + u (s1 - s0)    w -> log_ratio = l0 + u (l1 - l0)
    r = 1:  x -> ux    y -> uy    z -> theta = (2u - 1) theta_max     w -> brightness = 1 + (2u - 1) jb
    r = 2:  x -> contrast = 1 + (2u - 1) jc    y -> saturation = 1 + (2u - 1) js    z -> hue = (2u - 1) jh

The counter's first word is the image's index in the STORE, not its position in the batch: an image in a given epoch gets the same
augmentation -- and, because a pixel's arithmetic depends on its row alone, the same output bits -- for every batch size, order and split.

Store indices.  The kernel never dereferences an index outside [0, N): such a sample's output (and reported row) is NaN, which the loss
turns into a non-finite value the training loop already watches for.  Index lists that come from the host (a Python sequence, a CPU tensor,
the loader's subset) are checked on the host when they are uploaded, at no synchronisation cost; a device tensor is not read back.

There is no CPU path: ``DeviceImageStore.batch`` on CPU tensors raises ``RovitHipError``.  ``augment_reference`` (the explicit torch
recipe above, on any device, fp64 by default) and ``draw_params_reference`` (numpy, on ``oracle.philox``) are the oracles
of the tests and one arm of tools/time_augment.py, not fall-backs.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import native
from .native import RovitHipError, call, ptr, stream_ptr

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
RGB_TO_YIQ = ((0.299, 0.587, 0.114), (0.5959, -0.2746, -0.3213), (0.2115, -0.5227, 0.3112))
PARAM_NAMES = ('flip_h', 'flip_v', 'area', 'log_ratio', 'ux', 'uy', 'theta', 'brightness', 'contrast', 'saturation', 'hue', 'pad')
ROW = len(PARAM_NAMES)


@dataclass(frozen=True)
class AugmentConfig:
    """Ranges the per-sample rows are drawn from.  The defaults equal ``augmented_transforms()``: horizontal flip + normalise."""
    hflip: float = 0.5
    vflip: float = 0.0
    scale: Tuple[float, float] = (1.0, 1.0)          # crop area as a fraction of the source
    ratio: Tuple[float, float] = (1.0, 1.0)          # crop aspect ratio (drawn log-uniformly)
    rotate_deg: float = 0.0                          # theta uniform in [-rotate_deg, rotate_deg]
    brightness: float = 0.0                          # factors uniform in [1 - j, 1 + j]
    contrast: float = 0.0
    saturation: float = 0.0
    hue: float = 0.0                                 # fraction of a full turn, uniform in [-hue, hue]

    @classmethod
    def identity(cls) -> 'AugmentConfig':
        """No augmentation (validation and test batches): normalisation only."""
        return cls(hflip=0.0)

    def validate(self) -> None:
        s0, s1 = self.scale
        r0, r1 = self.ratio
        if not (0.0 <= self.hflip <= 1.0 and 0.0 <= self.vflip <= 1.0):
            raise RovitHipError(f'AugmentConfig: flip probabilities ({self.hflip}, {self.vflip}) outside [0, 1]')
        if not (0.0 < s0 <= s1 <= 1.0):
            raise RovitHipError(f'AugmentConfig: scale range {self.scale} must satisfy 0 < lo <= hi <= 1')
        if not (0.0 < r0 <= r1 and math.isfinite(r1)):
            raise RovitHipError(f'AugmentConfig: ratio range {self.ratio} must satisfy 0 < lo <= hi')
        for k in ('rotate_deg', 'brightness', 'contrast', 'saturation', 'hue'):
            v = getattr(self, k)
            if not (v >= 0.0 and math.isfinite(v)):
                raise RovitHipError(f'AugmentConfig: {k} = {v} must be finite and >= 0')

    def ranges(self) -> Tuple[float, ...]:
        """The eleven fp32 fields of ``rovit_augment_config``, in its order."""
        return (self.hflip, self.vflip, self.scale[0], self.scale[1], math.log(self.ratio[0]), math.log(self.ratio[1]),
                math.radians(self.rotate_deg), self.brightness, self.contrast, self.saturation, self.hue)

    def to_c(self) -> native.AugmentConfigC:
        return native.AugmentConfigC(*self.ranges())


# ------------------------------------------------------------------------------------------------------------
# References (any device; the oracles of the tests)
# ------------------------------------------------------------------------------------------------------------
def colour_matrix(saturation: torch.Tensor, hue: torch.Tensor) -> torch.Tensor:
    """A = inv(T) diag(1, s Rot(2 pi hue)) T for vectors of s and hue: (B, 3, 3) in their dtype."""
    dt, dev = saturation.dtype, saturation.device
    T = torch.tensor(RGB_TO_YIQ, dtype=torch.float64).to(device=dev, dtype=dt)
    Tinv = torch.linalg.inv(torch.tensor(RGB_TO_YIQ, dtype=torch.float64)).to(device=dev, dtype=dt)
    a = 2.0 * math.pi * hue
    c, s = saturation * torch.cos(a), saturation * torch.sin(a)
    D = torch.zeros(saturation.shape[0], 3, 3, dtype=dt, device=dev)
    D[:, 0, 0] = 1.0
    D[:, 1, 1], D[:, 1, 2], D[:, 2, 1], D[:, 2, 2] = c, -s, s, c
    return Tinv @ D @ T


def sample_grid(params: torch.Tensor, src_size: Tuple[int, int], out_size: Tuple[int, int]):
    """The UNclamped source coordinates (sx, sy), each (B, Ho, Wo), of the rows' affine maps."""
    Hs, Ws = src_size
    Ho, Wo = out_size
    p = params
    fh, fv = (p[:, 0] > 0.5).to(p.dtype), (p[:, 1] > 0.5).to(p.dtype)
    r = torch.exp(p[:, 3])
    w = torch.clamp(Ws * torch.sqrt(p[:, 2] * r), max=float(Ws))
    h = torch.clamp(Hs * torch.sqrt(p[:, 2] / r), max=float(Hs))
    cx, cy = p[:, 4] * (Ws - w) + w / 2, p[:, 5] * (Hs - h) + h / 2
    j = torch.arange(Wo, dtype=p.dtype, device=p.device)
    i = torch.arange(Ho, dtype=p.dtype, device=p.device)
    dx = ((j + 0.5) / Wo - 0.5).view(1, 1, Wo) * (w * (1 - 2 * fh)).view(-1, 1, 1)
    dy = ((i + 0.5) / Ho - 0.5).view(1, Ho, 1) * (h * (1 - 2 * fv)).view(-1, 1, 1)
    cs, sn = torch.cos(p[:, 6]).view(-1, 1, 1), torch.sin(p[:, 6]).view(-1, 1, 1)
    sx = cx.view(-1, 1, 1) + cs * dx - sn * dy - 0.5
    sy = cy.view(-1, 1, 1) + sn * dx + cs * dy - 0.5
    return sx, sy


def augment_reference(src_u8: torch.Tensor, indices, params: torch.Tensor, out_size: Tuple[int, int] = (224, 224),
                      dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """The transform of the module docstring as explicit torch operations, on ``src_u8``'s device: (B, 3, Ho, Wo) in ``dtype``."""
    dev = src_u8.device
    idx = torch.as_tensor(indices, dtype=torch.long).to(dev)
    p = torch.as_tensor(params).to(device=dev, dtype=dtype).reshape(-1, ROW)
    B, (Hs, Ws), (Ho, Wo) = idx.numel(), src_u8.shape[-2:], out_size
    img = src_u8.index_select(0, idx).to(dtype).div_(255.0).reshape(B, 3, Hs * Ws)
    sx, sy = sample_grid(p, (Hs, Ws), (Ho, Wo))
    sx, sy = sx.clamp(0, Ws - 1), sy.clamp(0, Hs - 1)
    x0f, y0f = torch.floor(sx), torch.floor(sy)
    fx, fy = (sx - x0f).view(B, 1, -1), (sy - y0f).view(B, 1, -1)
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = (x0 + 1).clamp(max=Ws - 1), (y0 + 1).clamp(max=Hs - 1)

    def tap(y, x):
        return img.gather(2, (y * Ws + x).view(B, 1, -1).expand(B, 3, -1))

    top = tap(y0, x0) * (1 - fx) + tap(y0, x1) * fx
    bot = tap(y1, x0) * (1 - fx) + tap(y1, x1) * fx
    v = top * (1 - fy) + bot * fy                                                  # (B, 3, Ho*Wo)
    z = colour_matrix(p[:, 9], p[:, 10]) @ v
    z = p[:, 7].view(B, 1, 1) * (0.5 + p[:, 8].view(B, 1, 1) * (z - 0.5))
    z = z.clamp(0.0, 1.0)
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float64).to(device=dev, dtype=dtype).view(1, 3, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float64).to(device=dev, dtype=dtype).view(1, 3, 1)
    return ((z - mean) / std).view(B, 3, Ho, Wo)


def draw_params_reference(indices, config: AugmentConfig, seed: int, epoch: int) -> np.ndarray:
    """The rows the kernel draws for store indices ``indices``: (B, 12) float32, from the repository's numpy restatement of
    Philox4x32-10 (oracle/philox.py, known-answer tested).  ``u`` is exact; every derived entry is evaluated in fp64 and rounded once
    (the kernel's fp32 evaluation differs by one or two roundings)."""
    from oracle.philox import philox4x32_10 as philox          # checker only, like the head-phase masks
    idx = np.asarray(torch.as_tensor(indices).cpu().numpy() if isinstance(indices, torch.Tensor) else indices, dtype=np.int64).reshape(-1)
    n = idx.size
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    lo, hi = np.full(n, epoch & 0xFFFFFFFF, np.uint64), np.full(n, (epoch >> 32) & 0xFFFFFFFF, np.uint64)
    c0 = (idx & 0xFFFFFFFF).astype(np.uint64)
    u = [[(w >> np.uint64(8)).astype(np.float64) / 16777216.0 for w in philox([c0, np.full(n, r, np.uint64), lo, hi], key)] for r in range(3)]
    f = [np.float64(np.float32(v)) for v in config.ranges()]       # the fp32 values the C struct carries
    p_h, p_v, s0, s1, l0, l1, tmax, jb, jc, js, jh = f
    rows = np.zeros((n, ROW), np.float64)
    rows[:, 0] = u[0][0] < p_h
    rows[:, 1] = u[0][1] < p_v
    rows[:, 2] = s0 + u[0][2] * (s1 - s0)
    rows[:, 3] = l0 + u[0][3] * (l1 - l0)
    rows[:, 4], rows[:, 5] = u[1][0], u[1][1]
    rows[:, 6] = (2 * u[1][2] - 1) * tmax
    rows[:, 7] = 1 + (2 * u[1][3] - 1) * jb
    rows[:, 8] = 1 + (2 * u[2][0] - 1) * jc
    rows[:, 9] = 1 + (2 * u[2][1] - 1) * js
    rows[:, 10] = (2 * u[2][2] - 1) * jh
    return rows.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------
# The store
# ------------------------------------------------------------------------------------------------------------
class DeviceImageStore:
    """``images_u8`` (N, 3, Hs, Ws) uint8 with ``labels`` and ``severities`` (N), resident on one device.

    ``dataset``: the ``RoseLeafDataset`` the store was decoded from (``DeviceAugmentLoader.dataset.dataset``).  The constructor accepts
    tensors of any device so that loader logic can be built and tested without one; ``batch`` is the kernel and needs the HIP device."""

    def __init__(self, images_u8: torch.Tensor, labels: torch.Tensor, severities: torch.Tensor, dataset=None):
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[1] != 3:
            raise RovitHipError(f'DeviceImageStore expects uint8 (N, 3, H, W), got {images_u8.dtype} {tuple(images_u8.shape)}')
        if images_u8.shape[0] == 0 or labels.shape[0] != images_u8.shape[0] or severities.shape[0] != images_u8.shape[0]:
            raise RovitHipError('DeviceImageStore: empty store, or labels / severities do not match the images')
        self.images = images_u8.contiguous()
        self.labels = labels.to(self.images.device, torch.long)
        self.severities = severities.to(self.images.device, torch.long)
        self.dataset = dataset

    def __len__(self) -> int:
        return int(self.images.shape[0])

    @property
    def device(self) -> torch.device:
        return self.images.device

    @property
    def nbytes(self) -> int:
        """Resident bytes: the images and the two label vectors."""
        return sum(int(t.numel()) * t.element_size() for t in (self.images, self.labels, self.severities))

    @classmethod
    def synthetic(cls, labels: torch.Tensor, severities: torch.Tensor, device, size: Tuple[int, int] = (224, 224), seed: int = 0,
                  dataset=None) -> 'DeviceImageStore':
        """Seeded uniform uint8 noise images, one per label, generated on ``device``."""
        device = torch.device(device)
        g = torch.Generator(device=device).manual_seed(seed)
        imgs = torch.randint(0, 256, (int(labels.shape[0]), 3, int(size[0]), int(size[1])), dtype=torch.uint8, device=device, generator=g)
        return cls(imgs, labels, severities, dataset)

    @classmethod
    def from_dataset(cls, dataset, device, size: Tuple[int, int] = (224, 224), threads: int = 16, seed: int = 0) -> 'DeviceImageStore':
        """Decode an image-folder ``RoseLeafDataset`` once on the host (PIL, at most 16 threads), resize every image to ``size`` =
        (Hs, Ws) with PIL's default filter, upload once.  A synthetic dataset (no files) gets a synthetic store seeded with ``seed``."""
        device = torch.device(device)
        if not dataset.samples:
            return cls.synthetic(dataset.labels, dataset.severities, device, size, seed=seed, dataset=dataset)
        from concurrent.futures import ThreadPoolExecutor
        from PIL import Image
        Hs, Ws = int(size[0]), int(size[1])
        host = torch.empty(len(dataset.samples), 3, Hs, Ws, dtype=torch.uint8)
        if device.type == 'cuda':
            host = host.pin_memory()

        def load(k: int) -> None:
            with Image.open(dataset.samples[k][0]) as im:
                host[k] = torch.from_numpy(np.asarray(im.convert('RGB').resize((Ws, Hs))).copy()).permute(2, 0, 1)

        with ThreadPoolExecutor(max_workers=max(1, min(16, int(threads)))) as pool:
            list(pool.map(load, range(len(dataset.samples))))
        return cls(host.to(device), dataset.labels, dataset.severities, dataset)

    def upload_indices(self, indices) -> torch.Tensor:
        """int64 device vector of store indices.  Host-side lists and tensors are range-checked here; a device tensor is taken as is
        (the kernel writes NaN for an index it must not read)."""
        if isinstance(indices, torch.Tensor) and indices.is_cuda:
            return indices.to(torch.long).contiguous()
        idx = torch.as_tensor(indices, dtype=torch.long).reshape(-1)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise RovitHipError(f'store index outside [0, {len(self)})')
        return idx.to(self.device, non_blocking=True)

    def batch(self, indices, config: Optional[AugmentConfig] = None, seed: int = 0, epoch: int = 0,
              params: Optional[torch.Tensor] = None, return_params: bool = False, out_size: Tuple[int, int] = (224, 224),
              out: Optional[torch.Tensor] = None):
        """One launch: fp32 (B, 3, Ho, Wo) of ``indices`` (sequence, CPU or device int64 tensor), drawn from ``config`` at
        ``(seed, epoch)`` or computed from explicit rows ``params`` (B, 12).  ``return_params``: also the (B, 12) rows used.
        ``out``: an fp32 device tensor to write into instead of a new one."""
        if not self.images.is_cuda:
            raise RovitHipError('DeviceImageStore.batch runs on the HIP device only (the store is on the CPU); there is no CPU path')
        config = config if config is not None else AugmentConfig()
        config.validate()
        Ho, Wo = int(out_size[0]), int(out_size[1])
        if Ho <= 0 or Wo <= 0 or Wo % 4:
            raise RovitHipError(f'out_size {tuple(out_size)}: the width must be a positive multiple of 4')
        idx = self.upload_indices(indices)
        B = int(idx.numel())
        if B == 0:
            raise RovitHipError('empty batch')
        if params is not None:
            params = params.to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(params.shape) != (B, ROW):
                raise RovitHipError(f'params must be ({B}, {ROW}), got {tuple(params.shape)}')
        if out is None:
            out = torch.empty(B, 3, Ho, Wo, dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (B, 3, Ho, Wo):
            raise RovitHipError(f'out must be fp32 ({B}, 3, {Ho}, {Wo})')
        rows = torch.empty(B, ROW, dtype=torch.float32, device=self.device) if return_params else None
        cfg = config.to_c()
        N, _, Hs, Ws = self.images.shape
        call('rovit_augment_batch', ptr(self.images), N, Hs, Ws, ptr(idx), B, ptr(params), ptr(rows), C.addressof(cfg),
             int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFFFFFFFFFF, ptr(out), Ho, Wo, stream_ptr())
        return (out, rows) if return_params else out

    def corrupt(self, indices, corruption: str, severity: int = 3, seed: int = 0, param=None, out: Optional[torch.Tensor] = None,
                return_u8: bool = False):
        """``rovit_hip.corrupt.corrupt(self, ...)``: the images under one of its ``CORRUPTIONS`` at the store's own resolution."""
        from .corrupt import corrupt
        return corrupt(self, indices, corruption, severity, seed, param, out, return_u8)
