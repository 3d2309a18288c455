"""Shared cases of the KAN grid-extension tests (tests/test_kan_grid_cpu.py, tests/test_gpu_kan_grid.py): heads, grids, conditioned
inputs, the brute-force least-squares statement and the fp32 yardstick of the moment kernel.

Float bound of the moments (the rule of tests/test_gpu_corrupt.py): per transition and per quantity (G, M, O as MEANS over the finite
rows, max-abs over every entry), four times the largest deviation from fp64 of an fp32 numpy evaluation of the same formulas -- fp32 tanh,
the closed-form bases and the products in fp32, at most 16 rows added in fp32 before the fp64 sum -- over every shape, layer and row
count the tests use.  The deviations are computed here, once per transition, from the reference alone; nothing in them comes from the
kernel.  The kernels' measured distances are in DESIGN.md section 2."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_cpu  # noqa: E402  (checker only)

SHAPES = ((7, 3, 1), (192, 64, 16, 1))
ROWS = (1, 255, 257, 1000)          # the 16-row fold and the 256-row chunks (the row partition is made of whole chunks) on either side
KEYS = ('spline_weights', 'knots', 'linear.weight', 'linear.bias')
CUTOFF_GAP = 1e-4
HALVED = (-1.0 + 0.1 * np.arange(18, dtype=np.float64)).astype(np.float32)      # the default grid's step halved, same origin and cutoff
# name -> (the head's num_knots before, fit keywords)
TRANSITIONS = {'5_to_5_cover': (5, {'num_knots': 5}), '5_to_halved': (5, {'knots': torch.from_numpy(HALVED)}),
               '32_to_16': (32, {'num_knots': 16}), '5_to_58': (5, {'num_knots': 58})}


def new_knots(name: str) -> np.ndarray:
    from rovit_hip import kan_grid
    kw = TRANSITIONS[name][1]
    return kw['knots'].numpy() if 'knots' in kw else kan_grid.make_grid(kw['num_knots']).numpy()


def old_knots(name: str) -> np.ndarray:
    return ref_cpu.make_knots(TRANSITIONS[name][0], 3).numpy()


def head_state(layers, num_knots, seed):
    g = torch.Generator().manual_seed(seed)
    return ref_cpu.init_kan_state(list(layers), num_knots, 3, g), g


def cutoff(knots) -> float:
    k = np.asarray(knots, dtype=np.float64)
    return float(k[k.size - 4])


def condition(x: torch.Tensor, grids) -> torch.Tensor:
    """Move (not drop) every entry whose tanh lies within CUTOFF_GAP of a grid's cutoff ``knots[nb]``, the basis' one discontinuity, to
    3 gaps below it; asserted afterwards.  Cutoffs at or beyond 1 cannot be reached by tanh and are left alone."""
    x = x.clone()
    for k in grids:
        c = cutoff(k)
        if c >= 1.0 - 4 * CUTOFF_GAP:
            continue
        near = (torch.tanh(x.double()) - c).abs() < CUTOFF_GAP
        x[near] = float(np.arctanh(c - 3 * CUTOFF_GAP))
        assert not bool(((torch.tanh(x.double()) - c).abs() < CUTOFF_GAP).any())
    return x


def layer_inputs(n: int, width: int, layer: int, seed: int, grids) -> torch.Tensor:
    """(n, width) fp32 inputs of a layer: N(0, 1.5^2) for the first, ReLU of it for the later ones (half the rows exactly 0)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, width, generator=g) * 1.5
    if layer > 0:
        x = torch.relu(x)
    return condition(x, grids)


def lstsq_refit(x, old, new, c, prior_weight=1e-2):
    """Brute force: per input, ``np.linalg.lstsq`` on the stacked system -- the finite data rows weighted by sqrt(1 / N_i), then the
    quadrature rows weighted by sqrt(eps w / L) -- with the old splines' values as right-hand sides.  (in, out, nb') fp64."""
    from rovit_hip import kan_grid as kg
    x = np.asarray(x, dtype=np.float32)
    c = np.asarray(c, dtype=np.float64)
    vq, wq, L = kg.quadrature(new, old)
    Aq = kg.basis_v(vq, new) * np.sqrt(prior_weight * wq / L)[:, None]
    Bq = kg.basis_v(vq, old) * np.sqrt(prior_weight * wq / L)[:, None]
    out = np.zeros((c.shape[0], c.shape[1], len(new) - 4))
    for i in range(c.shape[0]):
        ok = np.isfinite(x[:, i])
        v = np.tanh(x[ok, i].astype(np.float64))
        s = 1.0 / np.sqrt(max(1, int(ok.sum())))
        A = np.concatenate([kg.basis_v(v, new) * s, Aq])
        rhs = np.concatenate([kg.basis_v(v, old) * s, Bq]) @ c[i].T
        out[i] = np.linalg.lstsq(A, rhs, rcond=None)[0].T
    return out


def mean_moments(mom):
    n = np.maximum(mom['rows'], 1).astype(np.float64)[:, None, None]
    return {k: mom[k] / n for k in ('G', 'M', 'O')}


def moment_layers():
    """(shape index, layer index, in_f) of every layer the moment tests run."""
    return [(s, l, shape[l]) for s, shape in enumerate(SHAPES) for l in range(len(shape) - 1)]


@functools.lru_cache(maxsize=None)
def moment_case(name: str, n: int, s: int, l: int):
    """Inputs and the fp64 reference means of one case; computed once and shared."""
    from rovit_hip import kan_grid as kg
    old, new = old_knots(name), new_knots(name)
    x = layer_inputs(n, SHAPES[s][l], l, 7919 * n + 31 * s + l, (old, new))
    want = mean_moments(kg.data_moments(x.numpy(), old, new))
    return x, want


@functools.lru_cache(maxsize=None)
def moment_bounds(name: str):
    """4 x the largest fp32-numpy deviation per quantity over every case of the transition (module docstring)."""
    from rovit_hip import kan_grid as kg
    old, new = old_knots(name), new_knots(name)
    worst = {'G': 0.0, 'M': 0.0, 'O': 0.0}
    for n in ROWS:
        for s, l, _ in moment_layers():
            x, want = moment_case(name, n, s, l)
            x64 = np.tanh(x.numpy().astype(np.float64))
            got = mean_moments(kg.data_moments(x.numpy(), old, new, kg.intervals_v(x64, old.astype(np.float64)),
                                               kg.intervals_v(x64, new.astype(np.float64)), dtype=np.float32))
            for k in worst:
                worst[k] = max(worst[k], float(np.abs(got[k] - want[k]).max()))
    return {k: 4.0 * v for k, v in worst.items()}
