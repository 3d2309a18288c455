"""Shared cases of the attack tests (tests/test_attack_cpu.py, tests/test_gpu_attack.py): plain numpy builders of the images, gradients,
perturbations, radii and masks the step and start kernels of csrc/attack.hip are held to, and the L2 tolerance.

What a case holds.  Images of every shape in ``SHAPES`` (one pixel; 3 and 5 pixels; 255 = 3 x 85, odd; 256, a multiple of 4: the 16-byte path inside
one slab; 257, odd again; 224 x 224, 49 slabs per plane) for B in ``BATCHES``.  The gradient carries exact zeros, -0.0, NaN and
+-inf at fixed positions; the perturbation carries values whose step lands exactly on +-r, one ulp inside and one ulp outside it (built
by search: the delta with fl32(delta + a) == the target); the images sit on the box edge (pixel 0 and 1) at fixed positions, and with
``clip=None`` also outside [0, 1].  Radii differ per image: 4/255, 0, a denormal, 8/255, 1/255 in that order.

L2 tolerance (derived): every element within ``8 * 2^-24 * max(r_bc, |reference|) + 2^-149`` of
``step_reference(dtype=float64)``.  The first term is the contract's: both norms are fp64 sums (error of order n 2^-53), the kernel rounds to
fp32 three times (the boxed perturbation, the scale factors' product, and for the start the normal), each half an ulp = 2^-24 relative.
The second term is one fp32 denormal step: with a denormal radius the first term is below the spacing of the fp32 numbers themselves
(2^-149), which no fp32 output can meet; for every normal radius it changes nothing."""
import numpy as np

SHAPES = [(1, 1), (1, 3), (1, 5), (3, 85), (16, 16), (1, 257), (224, 224)]
BATCHES = [1, 2, 5]
MISALIGNED_SHAPE = (16, 16)          # n % 4 == 0: the shape that also runs from a storage offset of one float
EPS = np.array([4 / 255, 0.0, 1e-40, 8 / 255, 1 / 255], dtype=np.float32)
ALPHA = np.array([1 / 255, 1 / 255, 1e-41, 2 / 255, 0.5 / 255], dtype=np.float32)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
L2_FACTOR = 8.0 * 2.0 ** -24
DENORMAL_STEP = 2.0 ** -149
SEED = 20260


def shape_id(shape):
    return f'{shape[0]}x{shape[1]}'


def _landing(a, target):
    """fp32 delta with fl32(delta + a) == target, elementwise (a, target fp32 arrays); found among the neighbours of fl32(target - a)."""
    a, target = np.asarray(a, np.float32), np.asarray(target, np.float32)
    d = (target - a).astype(np.float32)
    best = d.copy()
    found = (d + a).astype(np.float32) == target
    for direction in (np.float32(-np.inf), np.float32(np.inf)):
        c = d.copy()
        for _ in range(3):
            c = np.nextafter(c, direction)
            hit = ((c + a).astype(np.float32) == target) & ~found
            best = np.where(hit, c, best)
            found |= hit
    return best.astype(np.float32), found


def build(shape, B, clip=(0., 1.), seed=0, dead_image=False):
    """One case: dict of x, g, delta (B, 3, H, W) fp32, eps, alpha (B,) fp32, copy_mask (B,) bool, best (the buffer best_delta starts
    from), delta_l2 (the perturbation of the L2 tests).  ``dead_image``: the last image's gradient is all zeros and NaN (an L2 step must not move it)."""
    H, W = shape
    n = H * W
    rng = np.random.default_rng([SEED, H, W, B, seed, 0 if clip is None else 1])
    mean, std = np.array(MEAN, np.float32).reshape(1, 3, 1, 1), np.array(STD, np.float32).reshape(1, 3, 1, 1)
    z = rng.random((B, 3, H, W), dtype=np.float32)
    if clip is None:
        z = z * np.float32(1.4) - np.float32(0.2)          # some pixels outside [0, 1]
    flat = z.reshape(B, 3, n)
    flat[:, :, 0::11] = 0.0                                 # the box edge: pixel 0 and pixel 1
    flat[:, :, 5 % n::13] = 1.0
    x = ((z - mean) / std).astype(np.float32)
    eps, alpha = EPS[np.arange(B) % 5].copy(), ALPHA[np.arange(B) % 5].copy()
    inv_s = (1.0 / np.array(STD, np.float64)).astype(np.float32).reshape(1, 3, 1, 1)
    r = (eps.reshape(B, 1, 1, 1) * inv_s).astype(np.float32)
    a = (alpha.reshape(B, 1, 1, 1) * inv_s).astype(np.float32)
    g = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    delta = ((rng.random((B, 3, H, W), dtype=np.float32) * np.float32(2.0) - np.float32(1.0)) * r).astype(np.float32)
    gf, df = g.reshape(B, 3 * n), delta.reshape(B, 3 * n)
    rf, af = np.broadcast_to(r, x.shape).reshape(B, 3 * n), np.broadcast_to(a, x.shape).reshape(B, 3 * n)
    count = 3 * n
    # landings: positions 17 k + 1 (k = 0..5): +r, one ulp inside, one ulp outside, and the same three on the negative side
    for k in range(6):
        p = (17 * k + 1) % count
        sign = np.float32(1.0 if k < 3 else -1.0)
        edge = rf[:, p]
        target = [edge, np.nextafter(edge, np.float32(0.0)), np.nextafter(edge, np.float32(np.inf))][k % 3] * sign
        d, ok = _landing(sign * af[:, p], target)
        ok &= (rf[:, p] > af[:, p]) & (af[:, p] > np.float32(1e-30))
        df[:, p] = np.where(ok, d, df[:, p])
        gf[:, p] = np.where(ok, sign * np.float32(0.5), gf[:, p])
    df[:, 2 % count] = rf[:, 2 % count]                     # delta exactly on the ball
    df[:, 4 % count] = -rf[:, 4 % count]
    # specials of the gradient at positions 7 k + 3
    for k, v in enumerate([0.0, -0.0, np.nan, np.inf, -np.inf]):
        gf[:, (7 * k + 3) % count] = np.float32(v)
    if dead_image:
        gf[B - 1, 0::2] = 0.0
        gf[B - 1, 1::2] = np.nan
    # the L2 tests' perturbation: the same pattern scaled to 0.5 .. 1.7 times the L2 radius, so that some images start inside their ball
    # and some outside it (uniform values in [-r, r] have a pixel norm of about eps sqrt(n))
    ratio = np.array([1.5, 3.0, 1.2, 2.4, 0.9], np.float32)[np.arange(B) % 5].reshape(B, 1, 1, 1) / np.float32(np.sqrt(3.0 * n))
    delta_l2 = (delta * ratio).astype(np.float32)
    copy_mask = (np.arange(B) % 2 == 0) if B > 1 else np.array([True])
    best = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    return {'x': x, 'g': g, 'delta': delta, 'eps': eps, 'alpha': alpha, 'copy_mask': copy_mask, 'best': best, 'clip': clip, 'r': r, 'a': a,
            'delta_l2': delta_l2}


def l2_tolerance(case, reference):
    """(B, 3, H, W) fp64 bound of the module docstring on |kernel - reference|."""
    return L2_FACTOR * np.maximum(case['r'].astype(np.float64), np.abs(reference)) + DENORMAL_STEP


def l2_norm_bound(eps, count):
    """(B,) fp64 bound on the pixel norm of a returned perturbation of ``count`` elements: ``eps_b (1 + 2^-20)``, the contract's, plus the
    norm of ``count`` half steps of the fp32 denormals (each element is rounded to fp32 once; only a denormal radius can see it)."""
    return np.asarray(eps, np.float64) * (1.0 + 2.0 ** -20) + np.sqrt(count) * 2.0 ** -150


def pixel_norm(delta):
    """(B,) fp64 L2 norm of a normalised perturbation in pixel units."""
    s = np.array(STD, np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    return np.sqrt(((np.asarray(delta, np.float64) * s) ** 2).sum(axis=(1, 2, 3)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """Bit equality of two fp32 arrays, any NaN equal to any NaN (a NaN's payload is not part of the specification)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))
