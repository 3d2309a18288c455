"""Cases, fp64 truth and error bounds for the KAN spline kernels (csrc/kan_heads.hip, csrc/kan_stack.hip, csrc/kan_device.h and the KAN half
of head_phase_dw_kernel).  CPU only: numpy, no kernel code.  tests/test_kan_cases_cpu.py checks this module, tests/test_gpu_kan_rows.py
and tools/kan_rows_error.py use it against the exported entry points.

THE TRUTH R (fp64).  `basis` restates the reference's truncated Cox-de Boor recursion (models/kan.py:8-44 of the reference) on the STORED
fp32 knots taken as fp64: degree-0 indicators on [knots[i], knots[i+1]) for i < nb = nk - 4 only, the zero-denominator guards, the right
term dropped at i = nb - 1.  It is the recursion itself, not the closed form the kernels evaluate, and it carries the first and second
derivative along by differentiating every recursion step.  `layer_truth` puts KANLayer.forward (tanh, clamp, spline contraction + Linear)
and one of ACT_NONE / ACT_RELU / ACT_SIGMOID3 on top and, given the gradient of the output, the analytic backward: dL/dz through the
activation's derivative AT z (the reference's way, not through an fp32 y), dx, dW, dlin_w, dlin_b.  `stack_truth` and `backward_truth(gz_given=...)`
go LAYER BY LAYER ON GIVEN LAYER INPUTS: the GPU test feeds each layer the GPU's own previous output (and, backwards, the GPU's own dL/dz
of the layer above), so each layer is judged alone and no bound has to absorb cascade amplification.

THE BOUNDS, per output element, from fp64 quantities only (never from a GPU result).  u = 2^-24, gamma(n) = n u / (1 - n u).
  basis value    The kernels compute t = tanhf(x), the interval j by an exact search on the stored knots, u_ = (t - k_j) / (k_j+1 - k_j)
                 (three roundings: |d u_| <= 3u, i.e. 3 u h in t) and four cubics in u_ whose terms sum to at most 13/6 in magnitude over at
                 most six roundings each: 16 u.  With dt = TAU ulp32(t) + 3 u h the error of the coordinate,
                     eB = 16 u [B != 0] + |B'(t)| dt + |B''(t)| dt^2 / 2 + 8 dt^3 / hmin^3
                 (the last term bounds the Taylor remainder, max |B'''| <= 6 / hmin^3, and is what a kernel that picks the neighbouring
                 interval within dt of an INTERIOR knot leaves in a position where R has an exact zero: the spline is C2 there).
                 rovit_kan_basis takes the normalised coordinate itself: dt = 3 u h.
                 THE STORED KNOTS.  The kernels' cubics in u_ are the recursion on the grid v_m = k_j + (m - j) (k_j+1 - k_j); the stored
                 fp32 knots of linspace(-1, 1, nk) are that grid only up to their own rounding (spacings differ by up to 3.5e-6 of h at 64
                 knots, and knots[5] = -1.49e-8 on the default grid).  On an interval whose five surrounding spans agree within ROUNDING_TOL
                 (local_spans: what the rounding of stored knots explains, NOT the kernels' looser criterion for the closed form) the gap gB = |basis(t; k) - basis(t; v)|, both by
                 the recursion in fp64, is added to eB (gD to eD); it reaches 8e-7 at 64 knots.  Elsewhere it is NOT added.
  basis slope    the same with one derivative more: eD = 24 u / h + |B''(t)| dt + 3 dt^2 / hmin^3 (quadratics with terms <= 3 in sum, / h).
  forward        z = lin_b + sum_i (x lin_w + sum_k B W):  bz = sum eB |W| + gamma(5 in + 72) (|lin_b| + sum |x lin_w| + sum B |W|).
                 5 in + 72 covers every path: one thread's five FMAs per feature, the nsplit partial sums added serially (nsplit <= 64
                 for the widths that split), the chunk-by-chunk accumulation of the fused stack and the matrix-core order (its structural
                 zeros add exactly).  y: NONE and RELU are 1-Lipschitz, by = bz; SIGMOID3 y = 3 / (1 + __expf(-z)):
                 by = y (1 - y / 3) (bz + EPS_EXP + 2 u |z|) + 4 u y   (the exponent product z log2 e is rounded: 2 u |z|).
  dL/dz          NONE: exact.  RELU: the kernels gate on y > 0, R on z > 0: an element with |z| <= bz may fall on either side and gets
                 |g|.  SIGMOID3 act_grad = g y (1 - y c), c = fl(1/3), through the fp32 y:
                 |g| (|1 - 2 y / 3| by + 2 u y y / 3 + 3 u y (1 - y / 3)): y c is off y / 3 by the rounding of c and of the product, and that
                 ABSOLUTE error stays when 1 - y c cancels near y = 3; three more roundings act on the product.  A gradient
                 that itself carries an error e_g (the stack's chain) adds e_g |act'|, and one u |g| where two gradients are added.
  dx             r = fmaf(spl, 1 - t^2, lin): sum_o |gz| sum_k |W| eD (1 - t^2) + |spl| (2 |t| TAU ulp32(t) + 3 u)
                 + gamma(out + 16) (sum_o |gz| |sum_k W B'| (1 - t^2) + sum_o |gz lin_w|) + the bound of dL/dz pushed through the same
                 linear map (+ u |dx_prev + r| with accumulate).  out + 16: a lane's out / 4 outputs, four FMAs inside, two shuffles.
  dW, dlin_w,    sums over the batch: sum_b |gz| eB + gamma(B + 256) sum_b |gz B| + the bound of dL/dz through the map (dlin_w: x for B,
  dlin_b         dlin_b: 1).  B + 256 covers the batch chunks, the sample slices of a split item and their serial partial sums.
TAU (ulps of t = tanhf(x)) and EPS_EXP (relative error of __expf) are measured, not guessed: no document shipped with the toolchain states
an ulp bound for either, so they are the smallest powers of two for which every ratio of profiles/kan_rows_error.jsonl is at most 0.5 on
the unchanged kernels; the record names the ratios that fixed them.  Three tensors stay above 0.5 whatever they are: the accumulating dx
and the dL/dz of a layer that also receives an outside gradient are ONE fp32 addition against its exact half-ulp bound u |sum| (0.89, 0.80),
and the dL/dz of a SIGMOID3 output near y = 3 is the rounding of y c against twice its half-ulp bound (0.52).
Every bound also gets UNDERFLOW = 2^-120: a product or sum below the smallest normal (a subnormal input times a gradient) may be flushed.
NON-UNIFORM STORED KNOTS (nonuniform_knots()) are judged like any other: the truth is the recursion on them.  The kernels follow them:
where the five spans around interval j differ by more than UNIFORM_RTOL = 1e-4 of the span (the package's rule for a uniform grid) they run the local form of the recursion itself (about twice
the operations, on spans of unequal size: 32 u for the values, 48 u over the smallest local span for the slopes, 3 u of the largest
local span more in dt); where they agree, the closed form; its gap gB is forgiven only at the rounding level above, so spans that differ by more
than rounding and less than 1e-4 would show as errors of up to 1e-4 (no case here has such knots: the package's contract calls them uniform).

THE ONE DISCONTINUITY.  The truncated basis jumps to zero at t >= knots[nb].  guard = 2 TAU ulp32(knots[nb]); ulp32 is never smaller than
2^-126 (a flushed subnormal).  An input is DECIDED when |tanh64(x) - knots[nb]| > guard, and x = +-0 is decided always (tanhf(+-0) = +-0
exactly); otherwise it is EITHER-SIDE and R returns both candidates ('on': the basis continued from the left, 'off': zero); the GPU row
must lie within the bound of one of them and its backward must match the same choice (its dt is 3 TAU ulp: the 'on' candidate is evaluated
just left of the knot).  Either-side inputs exist only where a case constructs them, at most one a row, in layer-0 inputs; a hidden row whose
(GPU-made) input is within the guard may be skipped, at most 1 row in 1000.  INTERIOR knots need nothing of the kind: the cubic spline is
C2 there -- in R the left and right limits of value and first derivative agree to 1e-12 (test_kan_cases_cpu.py) -- so a coordinate that lands
on the other side of an interior knot moves the result by the third-order term above.

INPUT FAMILIES: knot_probe, random, relu_zeros, selector (see each)."""
import math
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
TAU = 2.0                       # ulps of t = tanhf(x): measured, see profiles/kan_rows_error.jsonl
EPS_EXP = 2.0 ** -24            # relative error of __expf: measured, see the same record
ACT_NONE, ACT_RELU, ACT_SIGMOID3 = 0, 1, 2
ACTS = (ACT_NONE, ACT_RELU, ACT_SIGMOID3)
PROBE_M = (0, 1, -1, 2, -2, 4, -4, 16, -16, 64, -64)
MIN_NORMAL = 2.0 ** -126
UNDERFLOW = 2.0 ** -120         # added to every bound: up to 64 products or sums of a result that fp32 flushes or rounds as a subnormal


def gamma(n):
    return n * U / (1.0 - n * U)


def ulp32(v):
    """Spacing of fp32 at |v| as fp64, never below the smallest normal (a flushed subnormal counts as that)."""
    return np.maximum(np.spacing(np.abs(np.asarray(v, dtype=np.float32))).astype(np.float64), MIN_NORMAL)


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------------------------------
# knot vectors
# ------------------------------------------------------------------------------------------------------------------------------------
def uniform_knots(nk):
    """The reference's knots: torch.linspace(-1, 1, nk) in fp32 (kan.py:59), its rounding artefacts included."""
    import torch
    return torch.linspace(-1, 1, nk).numpy().copy()


def nonuniform_knots():
    """name -> fp32 knots.  geometric: dense near 0; first_gap: knots[1] - knots[0] is ten times the median spacing, so the guess from
    inv_h0 is far off; cut_zero: knots[nb] == 0.0 exactly (every ReLU zero of a hidden layer sits on the jump, on its off side)."""
    g = [2.0 ** -e for e in range(8)]
    geo = [-v for v in g] + g[::-1]
    s = 2.0 / 22.0
    gap = [-1.0] + [-1.0 + 10 * s + i * s for i in range(13)]
    cz = [-1.0, -0.8, -0.65, -0.5, -0.4, -0.3, -0.2, -0.1, 0.0, 0.2, 0.5, 1.0]
    out = {'geometric': f32(geo), 'first_gap': f32(gap), 'cut_zero': f32(cz)}
    assert out['cut_zero'][len(cz) - 4] == 0.0
    return out


def uniform_cut_zero(nk=12, h=0.25):
    """A UNIFORM grid with knots[nb] == 0.0 exactly: what KANRegrid accepts of the cut_zero idea.  h = 0.25 is exact in fp32; with h = 0.13 and 11 knots
    the fp32 knots make 1 / (knots[1] - knots[0]) fall short, and the kernels' arithmetic guess puts t = 0.0 into interval nb - 1."""
    nb = nk - 4
    return f32([(i - nb) * h for i in range(nk)])


# ------------------------------------------------------------------------------------------------------------------------------------
# the truth
# ------------------------------------------------------------------------------------------------------------------------------------
def basis(t, knots, force_on=None, force_off=None):
    """(B, B', B'') of the truncated cubic basis at the fp64 coordinates t (any shape) -> three arrays of shape t.shape + (nb,).
    force_on: boolean mask of inputs evaluated just LEFT of the cutoff knot; force_off: inputs whose basis is zero (the two candidates of
    an either-side input)."""
    k = np.asarray(knots, dtype=np.float64)
    nk, nb = k.size, k.size - 4
    t = np.asarray(t, dtype=np.float64)
    inside = ((t >= k[0]) & (t <= k[-1]))[..., None]
    tc = np.clip(t, k[0], k[-1])
    if force_on is not None:
        tc = np.where(force_on, np.minimum(tc, np.nextafter(k[nb], -np.inf)), tc)
    tc = tc[..., None]
    B = ((tc >= k[:nb]) & (tc < k[1:nb + 1])).astype(np.float64)
    dB, d2B = np.zeros_like(B), np.zeros_like(B)
    zero = np.zeros_like(B[..., :1])

    def up(A):                                              # A[i + 1]; absent for i = nb - 1 (the dropped right term)
        return np.concatenate([A[..., 1:], zero], axis=-1)

    for d in (1, 2, 3):
        dl = k[d:d + nb] - k[:nb]
        il = np.where(dl != 0, 1.0 / np.where(dl != 0, dl, 1.0), 0.0)
        dr = k[d + 1:d + 1 + nb] - k[1:nb + 1]
        ir = np.where(dr != 0, 1.0 / np.where(dr != 0, dr, 1.0), 0.0)
        L = (tc - k[:nb]) * il
        R = (k[d + 1:d + 1 + nb] - tc) * ir
        Bu, dBu, d2Bu = up(B), up(dB), up(d2B)
        B, dB, d2B = (L * B + R * Bu,
                      il * B + L * dB - ir * Bu + R * dBu,
                      2 * il * dB + L * d2B - 2 * ir * dBu + R * d2Bu)
    dB, d2B = dB * inside, d2B * inside                     # the clamp's derivative
    if force_off is not None:
        keep = ~force_off[..., None]
        B, dB, d2B = B * keep, dB * keep, d2B * keep
    return B, dB, d2B


def interval(t, knots):
    """Knot interval of the clamped coordinate on the stored knots (fp64 comparison of fp32-exact values is exact)."""
    k = np.asarray(knots, dtype=np.float64)
    return np.clip(np.searchsorted(k, np.clip(t, k[0], k[-1]), side='right') - 1, 0, k.size - 1)


def cutoff(knots):
    return float(np.asarray(knots, dtype=np.float64)[len(knots) - 4])


def guard(knots):
    return float(2 * TAU * ulp32(cutoff(knots)))


def classify(x, knots):
    """'decided' mask of fp32 layer inputs x: |tanh64(x) - knots[nb]| > guard, or x == 0."""
    x = np.asarray(x, dtype=np.float64)
    return (np.abs(np.tanh(x) - cutoff(knots)) > guard(knots)) | (x == 0.0)


def act_apply(z, act):
    if act == ACT_RELU:
        return np.maximum(z, 0.0)
    if act == ACT_SIGMOID3:
        return 3.0 / (1.0 + np.exp(-z))
    return z


def act_slope(z, act):
    if act == ACT_RELU:
        return (z > 0).astype(np.float64)
    if act == ACT_SIGMOID3:
        y = 3.0 / (1.0 + np.exp(-z))
        return y * (1.0 - y / 3.0)
    return np.ones_like(z)


Params = namedtuple('Params', 'W knots lw lb in_f out_f nk')


def _bo(A, W):
    """einsum('bik,iok->bo') through one matrix product."""
    return A.reshape(A.shape[0], -1) @ np.ascontiguousarray(W.transpose(0, 2, 1)).reshape(-1, W.shape[1])


def _bio(A, W):
    """einsum('bik,iok->bio') as a batched matrix product over i."""
    return np.matmul(A.transpose(1, 0, 2), W.transpose(0, 2, 1)).transpose(1, 0, 2)


def _iok(gz, A):
    """einsum('bo,bik->iok') as a batched matrix product over i."""
    return np.matmul(A.transpose(1, 2, 0), gz).transpose(0, 2, 1)


def make_layer(in_f, out_f, nk, seed, knots=None):
    """The reference's initial distributions (kan.py:63-68) in fp32."""
    rng = np.random.default_rng(seed)
    kn = f32(uniform_knots(nk) if knots is None else knots)
    nk = kn.size
    bound = 1.0 / math.sqrt(in_f)
    return Params(f32(rng.standard_normal((in_f, out_f, nk - 4)) * 0.1), kn, f32(rng.uniform(-bound, bound, (out_f, in_f))),
                  f32(rng.uniform(-bound, bound, out_f)), in_f, out_f, nk)


def make_stack(dims, nks, seed, knots=None):
    if isinstance(nks, int):
        nks = [nks] * (len(dims) - 1)
    return [make_layer(a, b, nk, seed * 16 + l, knots) for l, (a, b, nk) in enumerate(zip(dims[:-1], dims[1:], nks))]


def stack_acts(n):
    return [ACT_RELU] * (n - 1) + [ACT_SIGMOID3]


def layer_truth(x, p, act, choice=None, tanh=True):
    """Forward of one layer in fp64.  x: (B, in) fp32.  choice: None, or a (B, in) int8 array, 0 where the input is decided, +1 / -1 for the
    'on' / 'off' candidate of an either-side input.  Returns a dict with everything the bounds and the backward need."""
    x64 = np.asarray(x, dtype=np.float64)
    t = np.tanh(x64) if tanh else x64
    on = off = None
    if choice is not None:
        on, off = choice > 0, choice < 0
    B, dB, d2B = basis(t, p.knots, on, off)
    W, lw, lb = (np.asarray(a, dtype=np.float64) for a in (p.W, p.lw, p.lb))
    z = _bo(B, W) + x64 @ lw.T + lb
    return {'x': x64, 't': t, 'B': B, 'dB': dB, 'd2B': d2B, 'z': z, 'y': act_apply(z, act), 'act': act, 'p': p,
            'wide': None if choice is None else choice != 0}


UNIFORM_RTOL = 1e-4             # kan_device.h KAN_UNIFORM_RTOL: spans within this fraction of each other are one uniform step to the kernels
ROUNDING_TOL = 16 * U           # spans of a uniform grid on [-1, 1] stored in fp32 differ by less (linspace: 4 u); scaled by max |knot| beyond 1


def storage_uniform(knots):
    """True when every spacing of the stored knots is within 8 u of the mean one: a grid that is uniform but for the rounding of its
    fp32 values (linspace(-1, 1, nk): each knot is start + i step with both rounded, at most 3 u off, so a spacing at most 6 u)."""
    d = np.diff(np.asarray(knots, dtype=np.float64))
    return bool(np.max(np.abs(d - d.mean())) <= 8 * U)


def local_spans(knots):
    """Per interval j, of the five spans j-2 .. j+2 the cubics alive on j depend on (spans off the left end count as span j; off the
    right end they belong to dead intervals and are clipped): (closed, rounding, smallest, largest).  closed: the kernels' criterion for
    taking the closed form, |d - h| <= UNIFORM_RTOL h in fp32.  rounding: the spans differ by no more than the rounding of the stored
    knots explains -- the only deviation whose effect the bounds forgive (knot_gap), whatever the kernels' criterion is."""
    k = f32(knots)
    d = (k[1:] - k[:-1]).astype(np.float32)
    n = d.size
    scale = max(1.0, float(np.abs(k).max()))
    closed, rnd, lo, hi = np.zeros(n + 1, dtype=bool), np.zeros(n + 1, dtype=bool), np.ones(n + 1), np.ones(n + 1)
    for j in range(n):
        loc = np.array([d[j + m] if 0 <= j + m < n else d[j] for m in (-2, -1, 0, 1, 2)], dtype=np.float32)
        dev = np.abs(loc - d[j]).max()
        closed[j] = dev <= np.float32(UNIFORM_RTOL) * d[j]
        rnd[j] = dev <= ROUNDING_TOL * scale
        lo[j], hi[j] = loc.min(), loc.max()
    return closed, rnd, lo, hi


def knot_gap(tr):
    """(|B - Bv|, |B' - Bv'|): what the recursion on the stored knots and the recursion on the grid v_m = k_j + (m - j) (k_j+1 - k_j) the
    kernels' u = (t - k_j) / (k_j+1 - k_j) stands for differ by, per element, both by `basis` in fp64.  Zero for a grid that is not
    storage_uniform: there the kernels have to follow the stored knots."""
    p, t = tr['p'], tr['t']
    gB, gD = np.zeros_like(tr['B']), np.zeros_like(tr['B'])
    uni = local_spans(p.knots)[1]
    k = np.asarray(p.knots, dtype=np.float64)
    nk, nb = k.size, k.size - 4
    wide = tr['wide']
    tt = t if wide is None else np.where(wide, np.minimum(t, np.nextafter(k[nb], -np.inf)), t)
    j = interval(tt, k)
    for jj in np.unique(j):
        if jj >= nb or not uni[jj]:
            continue
        sel = j == jj
        v = k[jj] + (np.arange(nk) - jj) * (k[jj + 1] - k[jj])
        Bv, dBv, _ = basis(tt[sel], v)
        live = (tr['B'][sel] != 0).any(-1, keepdims=True) | (tr['dB'][sel] != 0).any(-1, keepdims=True)     # not an 'off' candidate
        gB[sel] = np.abs(tr['B'][sel] - Bv) * live
        gD[sel] = np.abs(tr['dB'][sel] - dBv) * live
    return gB, gD


def basis_bounds(tr, tanh=True):
    """(eB, eD): error bounds of the kernels' basis values and slopes, shape (B, in, nb)."""
    if ('_bb', tanh) in tr:
        return tr['_bb', tanh]
    tr['_bb', tanh] = out = _basis_bounds(tr, tanh)
    return out


def _basis_bounds(tr, tanh):
    p, t = tr['p'], tr['t']
    k = np.asarray(p.knots, dtype=np.float64)
    j = np.clip(interval(t, k), 0, k.size - 2)
    h = (k[j + 1] - k[j])[..., None]
    hmin = float(np.min(np.diff(k)))
    dt = 3 * U * h
    if tanh:
        tau = TAU * (np.where(tr['wide'], 3.0, 1.0) if tr['wide'] is not None else 1.0)
        dt = dt + (tau * ulp32(t))[..., None]
    B, dB, d2B = tr['B'], np.abs(tr['dB']), np.abs(tr['d2B'])
    gB, gD = knot_gap(tr)
    uni, _, lo, hi = local_spans(p.knots)
    gen = ~uni[j][..., None]                                # the recursion itself: about twice the operations, on spans of unequal size
    c = np.where(gen, 2.0, 1.0)
    dt = dt + np.where(gen, 3 * U * hi[j][..., None], 0.0)
    hd = np.where(gen, lo[j][..., None], h)
    eB = 16 * U * c * (B != 0) + dB * dt + d2B * dt * dt / 2 + 8 * dt ** 3 / hmin ** 3 + gB
    eD = 24 * U * c / hd * ((B != 0) | (dB != 0)) + d2B * dt + 3 * dt * dt / hmin ** 3 + gD
    return eB, eD


def forward_bounds(tr, tanh=True):
    """(bz, by): bounds of the pre-activation and of the layer output, shape (B, out)."""
    p = tr['p']
    eB, _ = basis_bounds(tr, tanh)
    aW, alw, alb = (np.abs(np.asarray(a, dtype=np.float64)) for a in (p.W, p.lw, p.lb))
    mag = alb + np.abs(tr['x']) @ alw.T + _bo(tr['B'], aW)
    bz = _bo(eB, aW) + gamma(5 * p.in_f + 72) * mag
    if tr['act'] == ACT_SIGMOID3:
        y = tr['y']
        return bz, y * (1 - y / 3) * (bz + EPS_EXP + 2 * U * np.abs(tr['z'])) + 4 * U * y
    return bz, bz


def backward_truth(tr, g, g_err=None, y_err=None, dx_prev=None, gz_given=None, need_dx=True):
    """Backward of one layer in fp64 with its bounds.  g: (B, out) gradient of the layer output (fp32 values); g_err: its own error bound
    (the stack's chain) or None; y_err: bound of the y the kernel's act_grad reads (default: this layer's forward bound); dx_prev: what
    dx held before an accumulating call; gz_given: take dL/dz as given exactly (the GPU's own, when a layer below the top of a stack is
    judged alone) instead of deriving it from g.  Returns (values, bounds), dicts over gz, dx, dW, dlw, dlb."""
    p, act = tr['p'], tr['act']
    W, lw = np.asarray(p.W, dtype=np.float64), np.asarray(p.lw, dtype=np.float64)
    bz, by = forward_bounds(tr)
    if y_err is None:
        y_err = by
    if gz_given is not None:
        gz, bgz = np.asarray(gz_given, dtype=np.float64), np.zeros_like(tr['z'])
    else:
        g = np.asarray(g, dtype=np.float64)
        ag = np.abs(g)
        gz = g * act_slope(tr['z'], act)
        if act == ACT_RELU:
            bgz = np.where(np.abs(tr['z']) <= bz, ag, 0.0)
        elif act == ACT_SIGMOID3:
            y = tr['y']
            bgz = ag * (np.abs(1 - 2 * y / 3) * y_err + 2 * U * y * y / 3 + 3 * U * y * (1 - y / 3))
        else:
            bgz = np.zeros_like(gz)
        if g_err is not None:
            bgz = bgz + (g_err + U * ag) * np.abs(act_slope(tr['z'], act))
    agz = np.abs(gz)
    eB, eD = basis_bounds(tr)
    t, x = tr['t'], tr['x']
    dx = bdx = None
    if need_dx:
        s = 1 - t * t
        bi = lambda a, m: np.matmul(m, a[:, :, None])[:, :, 0]              # einsum('bo,bio->bi')
        M = _bio(tr['dB'], W)                                  # d spline_o / d t_i
        spl = bi(gz, M)
        dx = spl * s + gz @ lw
        bdx = (bi(agz, _bio(eD, np.abs(W))) * s
               + np.abs(spl) * (2 * np.abs(t) * TAU * ulp32(t) + 3 * U)
               + gamma(p.out_f + 16) * (bi(agz, np.abs(M)) * s + agz @ np.abs(lw))
               + bi(bgz, np.abs(M)) * s + bgz @ np.abs(lw))
        if dx_prev is not None:
            dx = dx + np.asarray(dx_prev, dtype=np.float64)
            bdx = bdx + U * np.abs(dx)
    n = gamma(x.shape[0] + 256)
    dW = _iok(gz, tr['B'])
    bdW = _iok(agz, eB) + n * _iok(agz, tr['B']) + _iok(bgz, tr['B'])
    dlw = gz.T @ x
    bdlw = n * (agz.T @ np.abs(x)) + bgz.T @ np.abs(x)
    dlb = gz.sum(0)
    bdlb = n * agz.sum(0) + bgz.sum(0)
    return ({'gz': gz, 'dx': dx, 'dW': dW, 'dlw': dlw, 'dlb': dlb},
            {'gz': bgz, 'dx': bdx, 'dW': bdW, 'dlw': bdlw, 'dlb': bdlb})


def ratio(got, want, bound):
    """|got - want| / bound per element (0 where they agree exactly, inf where got is not finite)."""
    got = np.asarray(got, dtype=np.float64)
    d = np.abs(got - want)
    r = np.where(d == 0, 0.0, d / (bound + UNDERFLOW))
    return np.where(np.isfinite(got), r, np.inf)


def worst(r):
    """(largest ratio, its index) of a ratio array."""
    if r.size == 0:
        return 0.0, ()
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), tuple(int(v) for v in i)


def choose(x, p, act, y_gpu, either):
    """The candidate each either-side row took, read off the layer output: a (B, in) int8 choice array (0 where decided) and the per-row
    ratio of the chosen candidate.  either: (B, in) mask with at most one True a row.  The two candidates of a row must differ by more than
    their bounds together (the spline weights that the cutoff's three bases meet are not zero), or the output could not tell them apart."""
    assert int(either.sum(1).max(initial=0)) <= 1
    rows = either.any(1)
    trs = [layer_truth(x[rows], p, act, (either[rows] * sign).astype(np.int8)) for sign in (1, -1)]
    bys = [forward_bounds(tr)[1] for tr in trs]
    apart = (np.abs(trs[0]['y'] - trs[1]['y']) > bys[0] + bys[1]).any(1)
    dead = (trs[0]['y'] == 0).all(1) & (trs[1]['y'] == 0).all(1)          # a ReLU that is off either way: no gradient passes, no choice matters
    assert (apart | dead).all(), 'an either-side input whose two candidates give the same output'
    r = [ratio(y_gpu[rows], tr['y'], by).max(1) for tr, by in zip(trs, bys)]
    sign = np.where(r[1] < r[0], -1, 1)
    choice = np.zeros(either.shape, dtype=np.int8)
    choice[rows] = either[rows] * sign[:, None]
    best = np.zeros(either.shape[0])
    best[rows] = np.minimum(r[0], r[1])
    return choice, best


def stack_truth(inputs, params, acts):
    """Layer by layer on GIVEN layer inputs (inputs[l]: what layer l read): the list of layer_truth dicts."""
    return [layer_truth(x, p, a) for x, p, a in zip(inputs, params, acts)]


def hidden_skip(x, knots):
    """Rows of a hidden layer's (GPU-made) input that hold a value within the guard of the cutoff."""
    return ~classify(x, knots).all(1)


# ------------------------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels' closed form (for the CPU test: the bounds must be satisfiable before a GPU sees them)
# ------------------------------------------------------------------------------------------------------------------------------------
def emulate_basis(t32, knots, deriv=False):
    """kan_basis of csrc/kan_device.h in numpy fp32: dense (.., nb) values (and slopes)."""
    one = np.float32(1)
    k = f32(knots)
    nk, nb = k.size, k.size - 4
    xc = np.minimum(np.maximum(f32(t32), k[0]), k[-1])
    j = np.clip(np.searchsorted(k, xc, side='right') - 1, 0, nk - 1)
    live = j < nb
    jc = np.minimum(j, nk - 2)
    tj = k[jc]
    h = (k[jc + 1] - tj).astype(np.float32)
    u = ((xc - tj) / h).astype(np.float32)
    u2 = u * u
    u3 = u2 * u
    om = one - u
    s6 = np.float32(1.0 / 6.0)
    v = [u3 * s6, (np.float32(-3) * u3 + np.float32(3) * u2 + np.float32(3) * u + one) * s6,
         (np.float32(3) * u3 - np.float32(6) * u2 + np.float32(4)) * s6, om * om * om * s6]
    ih = one / h
    dv = [np.float32(0.5) * u2 * ih, (np.float32(-9) * u2 + np.float32(6) * u + np.float32(3)) * s6 * ih,
          (np.float32(9) * u2 - np.float32(12) * u) * s6 * ih, np.float32(-0.5) * om * om * ih]
    # where the spans around j differ: the local Cox-de Boor recursion (kan_basis_general)
    gen = ~local_spans(k)[0][jc]
    if gen.any():
        kk = lambda q: k[np.clip(jc + q, 0, nk - 1)]
        l1, l2, l3 = xc - kk(0), xc - kk(-1), xc - kk(-2)
        r1, r2, r3 = kk(1) - xc, kk(2) - xc, kk(3) - xc
        a = one / (r1 + l1)
        n10, n11 = r1 * a, l1 * a
        b0, b1 = n10 / (r1 + l2), n11 / (r2 + l1)
        q0, q1, q2 = r1 * b0, l2 * b0 + r2 * b1, l1 * b1
        c0, c1, c2 = q0 / (r1 + l3), q1 / (r2 + l2), q2 / (r3 + l1)
        three = np.float32(3)
        gv = [l1 * c2, l2 * c1 + r3 * c2, l3 * c0 + r2 * c1, r1 * c0]
        gd = [three * c2, three * (c1 - c2), three * (c0 - c1), -three * c0]
        v = [np.where(gen, g_, v_).astype(np.float32) for g_, v_ in zip(gv, v)]
        dv = [np.where(gen, g_, v_).astype(np.float32) for g_, v_ in zip(gd, dv)]
    out = np.zeros(xc.shape + (nb,), dtype=np.float32)
    dout = np.zeros_like(out)
    idx = np.indices(xc.shape)
    for m in range(4):
        ok = live & (j - m >= 0)
        sel = tuple(a[ok] for a in idx) + ((j - m)[ok],)
        out[sel] = v[m][ok]
        dout[sel] = dv[m][ok]
    return (out, dout) if deriv else out


def emulate_layer(x, p, act, g=None):
    """The per-layer kernels' arithmetic in numpy fp32 (numpy's own summation order): y, and with g the backward dict."""
    x = f32(x)
    t = np.tanh(x).astype(np.float32)
    B, dB = emulate_basis(t, p.knots, deriv=True)
    z = (np.einsum('bik,iok->bo', B, p.W) + x @ p.lw.T + p.lb).astype(np.float32)
    if act == ACT_RELU:
        y = np.maximum(z, np.float32(0))
    elif act == ACT_SIGMOID3:
        y = (np.float32(3) / (np.float32(1) + np.exp(-z).astype(np.float32))).astype(np.float32)
    else:
        y = z
    if g is None:
        return y
    g = f32(g)
    if act == ACT_RELU:
        gz = np.where(y > 0, g, np.float32(0))
    elif act == ACT_SIGMOID3:
        gz = g * y * (np.float32(1) - y * np.float32(1.0 / 3.0))
    else:
        gz = g
    gz = gz.astype(np.float32)
    spl = np.einsum('bo,bik,iok->bi', gz, dB, p.W).astype(np.float32)
    dx = (spl * (np.float32(1) - t * t) + gz @ p.lw).astype(np.float32)
    return y, {'gz': gz, 'dx': dx, 'dW': np.einsum('bo,bik->iok', gz, B).astype(np.float32), 'dlw': (gz.T @ x).astype(np.float32),
               'dlb': gz.sum(0).astype(np.float32)}


# ------------------------------------------------------------------------------------------------------------------------------------
# input families
# ------------------------------------------------------------------------------------------------------------------------------------
Probe = namedtuple('Probe', 'name knots t32 x either n_constructed')


def knot_probe(nk=None, knots=None, name=None):
    """Every knot k = 1 .. nk-2 approached from both sides.
    t32: normalised coordinates for rovit_kan_basis: fl32(knots[k] + m ulp32(knots[k])) for m in PROBE_M, the end knots, interval midpoints.
    x:   layer inputs fl32(atanh(knots[k] + m ulp32(knots[k]))) for the same m, each classified (`either`: the either-side ones, which can
         only arise at the cutoff knot k = nb); plus 0.0 and -0.0, +-30, +-9, the smallest normal of both signs and a subnormal, the
         interval midpoints and one value below atanh(knots[1]) in each of the first three intervals (the left-edge terms that drop; the
         first of them is the first interval's midpoint region)."""
    kn = f32(uniform_knots(nk) if knots is None else knots)
    nk = kn.size
    k = kn.astype(np.float64)
    tt = np.array([k[q] + m * float(ulp32(k[q])) for q in range(1, nk - 1) for m in PROBE_M])
    origin = np.repeat(np.arange(1, nk - 1), len(PROBE_M))[np.abs(tt) < 1.0]             # the knot each probe is aimed at
    tt = tt[np.abs(tt) < 1.0]
    mids = (k[:-1] + k[1:]) / 2
    mids = mids[np.abs(mids) < 1.0]
    left = np.array([k[q] + f * (k[q + 1] - k[q]) for q in range(3) for f in (0.25, 0.9)])
    left = left[np.abs(left) < 1.0]
    t32 = f32(np.concatenate([tt, mids, left, [k[0], k[-1], 0.0, -1.5, 1.5]]))
    x = f32(np.concatenate([np.arctanh(tt), np.arctanh(mids), np.arctanh(left),
                            [0.0, -0.0, 30.0, -30.0, 9.0, -9.0, MIN_NORMAL, -MIN_NORMAL, 2.0 ** -140]]))
    either = ~classify(x, kn)
    # what the construction aims at the cutoff: the probes of knot nb, and the three tiny values when the cutoff is 0.0
    aimed = np.zeros(x.size, dtype=bool)
    aimed[:tt.size] = origin == nk - 4
    if cutoff(kn) == 0.0:
        aimed[-3:] = True
    return Probe(name or f'uniform{nk}', kn, t32, x, either, int((aimed & either).sum()))


def all_probes():
    out = [knot_probe(nk) for nk in range(8, 65)]
    out += [knot_probe(knots=v, name=n) for n, v in nonuniform_knots().items()]
    out.append(knot_probe(knots=uniform_cut_zero(), name='uniform_cut_zero'))
    out.append(knot_probe(knots=uniform_cut_zero(11, 0.13), name='zero_cut_guess'))
    return out


def decided_random(shape, knots_list, seed, scale=1.5, margin=100.0):
    """randn * scale in fp32 with every value further than margin * guard from the cutoff of every knot vector given."""
    rng = np.random.default_rng(seed)
    x = f32(rng.standard_normal(shape) * scale)
    for _ in range(8):
        bad = np.zeros(x.shape, dtype=bool)
        for kn in knots_list:
            bad |= np.abs(np.tanh(x.astype(np.float64)) - cutoff(kn)) <= margin * guard(kn)
        if not bad.any():
            break
        x[bad] = f32(rng.standard_normal(int(bad.sum())) * scale)
    return x


def random(batch, in_f, seed, scale=1.5, knots=None):
    return decided_random((batch, in_f), [] if knots is None else [knots], seed, scale)


def probe_rows(probe, in_f, seed, scale=1.5):
    """Layer-0 rows holding the probe inputs, one a row at column (row % in_f), the rest decided random values: (x, either)."""
    n = probe.x.size
    x = decided_random((n, in_f), [probe.knots], seed, scale)
    either = np.zeros((n, in_f), dtype=bool)
    r = np.arange(n)
    x[r, r % in_f] = probe.x
    either[r, r % in_f] = probe.either
    return x, either


def relu_zeros(batch, in_f, seed, knots=None):
    """Layer inputs as a ReLU leaves them: about half exact zeros, some of them -0.0, the rest positive."""
    rng = np.random.default_rng(seed)
    x = np.abs(decided_random((batch, in_f), [] if knots is None else [knots], seed + 1, 1.0))
    kind = rng.integers(0, 8, size=x.shape)
    x[kind < 4] = 0.0
    x[kind == 0] = -0.0
    return f32(x)


def selector(in_f, out_f, nk, i, o, k, knots=None):
    """W one-hot in a single (i, o, k), lin_w = 0, lin_b = 0: the forward returns one basis value, dW that value per sample, dx one slope."""
    kn = f32(uniform_knots(nk) if knots is None else knots)
    W = np.zeros((in_f, out_f, kn.size - 4), dtype=np.float32)
    W[i, o, k] = 1.0
    return Params(W, kn, np.zeros((out_f, in_f), dtype=np.float32), np.zeros(out_f, dtype=np.float32), in_f, out_f, kn.size)


def dw_bc(out_f, nk):
    """Batch rows per LDS chunk of the parameter-gradient kernels (rovit_kan_layer_bwd / rovit_kan_stack_bwd)."""
    return (24 * 1024) // (nk - 4 + 1 + out_f)


def kan_tb(out_f):
    return max(1, min(16, 64 // out_f))
