"""Shared cases of the corruption tests (tests/test_corrupt_cpu.py, tests/test_gpu_corrupt.py): store shapes, index lists, seeds, the
cached fp64 reference and the error bounds of the kernel-vs-reference comparison.

The stores are uniform uint8 noise drawn on the HOST from a numpy seed, so that the reference, the fp32 restatement the bounds come from
and the kernel all see the same bytes on every machine.  Uniform noise makes a wrong tap, channel, table entry or draw an error of order 1.

Bounds (max-abs on the normalised output, no pixel excluded).  ``corrupt_reference(..., dtype=np.float32)`` evaluates the reference's
formulas in fp32 numpy; its largest deviation from the fp64 reference over ALL the cases below (three shapes x severities 1, 3, 5), per
family, was

    noise        (gaussian_noise, shot_noise)                    3.6e-6  (shot_noise, severity 5, 224 x 224)
    photometric  (impulse_noise, brightness, contrast, saturate) 8.6e-7  (saturate, severity 5)
    stencil      (gaussian_blur, defocus_blur, motion_blur)      1.5e-5  (motion_blur, severity 1, 224 x 224)
    cell         (pixelate)                                      4.5e-7  (severity 1, 37 x 53)

(figures rounded up) and the bound of a family is 4x that (the precedent of tests/test_gpu_augment_batch.py).  The stencil figure is the
motion blur's at 224 x 224: one ulp of an fp32 sample coordinate near 224 is 1.5e-5 of a pixel, times a slope of up to 1 / 0.224 per
pixel on noise, averaged over the 2R + 1 samples; the Gaussian and the disk alone stay below 1.7e-6 and 5.8e-6.
``jpeg`` is integer arithmetic: its uint8 output is compared exactly and its fp32 output within 1e-6 (set by the task, about four
ulp of the largest normalised value)."""
import functools

import numpy as np

SHAPES = ((5, 37, 53), (3, 64, 64), (2, 224, 224))          # odd sides below one stencil tile; one tile exactly; several tiles
INDICES = {(5, 37, 53): (4, 0, 2, 2, 1, 3), (3, 64, 64): (2, 0, 2, 1), (2, 224, 224): (1, 0, 1)}          # repeated and out of order
SEVERITIES = (1, 3, 5)
SEED = 0x5EED0C0DE5

FAMILY = {'gaussian_noise': 'noise', 'shot_noise': 'noise', 'impulse_noise': 'photometric', 'brightness': 'photometric',
          'contrast': 'photometric', 'saturate': 'photometric', 'gaussian_blur': 'stencil', 'defocus_blur': 'stencil',
          'motion_blur': 'stencil', 'pixelate': 'cell'}
FP32_RESTATEMENT = {'noise': 3.6e-6, 'photometric': 8.6e-7, 'stencil': 1.5e-5, 'cell': 4.5e-7}
BOUND = {k: 4.0 * v for k, v in FP32_RESTATEMENT.items()}
JPEG_FP32_BOUND = 1e-6


def shape_id(shape) -> str:
    return f'{shape[0]}x{shape[1]}x{shape[2]}'


@functools.lru_cache(maxsize=None)
def store_images(shape) -> np.ndarray:
    n, h, w = shape
    images = np.random.default_rng(1000 * h + w).integers(0, 256, (n, 3, h, w), dtype=np.uint8)
    images.setflags(write=False)
    return images


@functools.lru_cache(maxsize=None)
def reference(shape, name: str, severity: int):
    """(fp64 (B, 3, H, W), uint8 (B, 3, H, W)) of ``INDICES[shape]``; computed once, shared, read-only."""
    from rovit_hip.corrupt import corrupt_reference
    out, u8 = corrupt_reference(store_images(shape), INDICES[shape], name, severity, seed=SEED, return_u8=True)
    out.setflags(write=False)
    u8.setflags(write=False)
    return out, u8
