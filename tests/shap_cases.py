"""Cases shared by the CPU and GPU tests of KernelSHAP (rovit_hip/shap.py, csrc/shap.hip): the (players, budget) grid, the games and
the references, computed once per process and never modified."""
import functools

import numpy as np

# (P, M) of the estimator alone.  Exact mode: M = 2^P - 2.
EXACT = [(2, 2), (3, 6), (8, 254)]
# none of these budgets enumerates a class (the share rule of the plan); (8, 100) and (196, 2600) enumerate the singletons and sample the
# rest, the mixed path
SAMPLED = [(8, 32), (13, 52), (49, 256), (196, 784)]
MIXED = [(8, 100), (196, 2600)]
SEEDS = [0, 7, (1 << 40) + 12345]                 # the last: a 64-bit seed above 2^32 (both key words used)

UNEQUAL5 = np.array([0] * 50 + [1] * 7 + [2] * 90 + [3] * 1 + [4] * 48, dtype=np.int32)    # an unequal 5-player patch map
UNEQUAL5_M = 20                                                                            # min(2^5 - 2, 4 * 5)


def patch_map_for(P: int) -> np.ndarray:
    """A (196,) patch -> player map with P players: the g x g block grid where P = g^2 divides the patch grid, interleaved ids otherwise
    (unequal counts when P does not divide 196)."""
    from rovit_hip.shap import player_map
    for g in (2, 7, 14):
        if g * g == P:
            return player_map(g)
    return (np.arange(196) % P).astype(np.int32)


@functools.lru_cache(maxsize=None)
def reference(P: int, M: int, seed: int):
    """(Z, w) of coalitions_reference, read-only."""
    from rovit_hip.shap import coalitions_reference
    Z, w = coalitions_reference(P, M, seed)
    Z.setflags(write=False)
    w.setflags(write=False)
    return Z, w


def rank_deficient_design():
    """(Z (8, 3), w): players 0 and 1 always together, unit weights.  A = [[4, 4, 0], [4, 4, 0], [0, 0, 4]]: the first pivot is 4, its
    root 2 and the second pivot 4 - 2 * 2 = 0 exactly, with or without a fused multiply-add."""
    Z = np.array([[1, 1, 0], [0, 0, 1]] * 4, dtype=bool)
    return Z, np.ones(8)


def random_game(P: int, seed: int):
    """A random non-additive game as a table over the 2^P coalitions (bit i of the index: player i); returns (table, value_fn)."""
    tab = np.random.default_rng(seed).standard_normal(2 ** P)
    weights = 1 << np.arange(P)
    return tab, lambda mask: tab[int((np.asarray(mask, dtype=np.int64) * weights).sum())]


def synthetic_values(Z: np.ndarray, B: int, T: int, seed: int):
    """fp32 values (M, B, T), v_empty and v_full (B, T) of a noisy additive game per (image, target): a_i of order 1 plus an interaction
    term, so the fit has a residual.  Exact in fp64 (they are fp32 numbers)."""
    rng = np.random.default_rng(seed)
    M, P = Z.shape
    a = rng.standard_normal((B, T, P))
    c = rng.standard_normal((B, T))
    inter = rng.standard_normal((B, T)) * 0.3
    size = Z.sum(axis=1).astype(np.float64)
    vals = c[None] + np.einsum('mp,btp->mbt', Z.astype(np.float64), a) + inter[None] * np.sin(size)[:, None, None]
    v0 = c + inter * np.sin(0.0)
    v1 = c + a.sum(axis=2) + inter * np.sin(float(P))
    return vals.astype(np.float32), v0.astype(np.float32), v1.astype(np.float32)
