"""Shared inputs of the per-head attention statistics tests (tests/test_head_stats_cpu.py, tests/test_gpu_head_stats.py): synthetic
probability matrices with known statistics, rows for the finalise kernel, the tolerance rule and the stated summation order of
csrc/head_stats.hip in fp32.  No GPU needed to import."""
import numpy as np

T, PATCHES, GRID = 197, 196, 14
LN197 = float(np.log(197.0))

# ---- tolerance rule ----------------------------------------------------------------------------------------------------------------
# Sums of at most 197 non-negative fp32 terms are off by at most 197 x 2^-24 relative; the cap allows 8 of them (the softmax bits are the
# oracle's inputs, so only the reductions and the device logarithm / square root differ).  A test asserts min(4 x measured, CAP) of the
# statistic's scale; MEASURED holds the largest error seen on the MI355X per class of statistic (None: not measured yet, the cap alone).
CAP = 8 * 197 * 2.0 ** -24
SCALES = {'entropy': LN197, 'distance': 16.0 * np.sqrt(338.0), 'mass': 1.0}
STAT_CLASS = ('entropy', 'distance', 'mass', 'mass', 'entropy', 'mass', 'mass', 'mass')       # of summary[..., k]
TOKEN_CLASS = ('entropy', 'distance', 'mass', 'mass')                                        # of per_token[..., k]


def tolerance(measured):
    return CAP if measured is None else min(4.0 * measured, CAP)


# ---- probability matrices with known statistics ------------------------------------------------------------------------------------

def uniform_probs(B=1, H=3):
    return np.full((B, H, T, T), 1.0 / T)


def identity_probs(B=1, H=3):
    return np.broadcast_to(np.eye(T), (B, H, T, T)).copy()


def right_neighbour_probs(B=1, H=3):
    """Every patch query attends to the patch on its right (the last column and the class token to themselves)."""
    P = np.zeros((T, T))
    P[0, 0] = 1.0
    for t in range(1, T):
        c = (t - 1) % GRID
        P[t, t + 1 if c < GRID - 1 else t] = 1.0
    return np.broadcast_to(P, (B, H, T, T)).copy()


def uniform_expected():
    """Analytic summary of the uniform matrix: mean distance to all 196 patches per patch query, 3x3 neighbourhood sizes."""
    r, c = np.divmod(np.arange(PATCHES), GRID)
    d = 16.0 * np.sqrt((r[:, None] - r[None]) ** 2.0 + (c[:, None] - c[None]) ** 2.0)
    per_query = d.mean(1)
    nb = ((np.minimum(r + 1, GRID - 1) - np.maximum(r - 1, 0) + 1) * (np.minimum(c + 1, GRID - 1) - np.maximum(c - 1, 0) + 1))
    return {'distance_per_query': per_query, 'distance': per_query.mean(), 'neighbours': nb, 'locality': nb.mean() / T,
            'summary': np.array([LN197, per_query.mean(), 1.0 / T, 1.0 / T, LN197, 1.0 / T, 1.0 / T, nb.mean() / T])}


# ---- rows for the finalise kernel ---------------------------------------------------------------------------------------------------

FINALIZE_N = (1, 5, 67, 300)
FINALIZE_CLASSES = 4
FINALIZE_EMPTY_CLASS = 2


def finalize_rows(n, depth=2, seed=0):
    """(summary (n, depth, 3, 8), cls_attention (n, depth, 3, 196), labels (n)) fp32 / int32: positive values of the statistics'
    magnitudes; class FINALIZE_EMPTY_CLASS of the FINALIZE_CLASSES never occurs."""
    rng = np.random.default_rng(1000 * seed + n)
    summary = (rng.random((n, depth, 3, 8)) * np.array([LN197, 294.2, 1, 1, LN197, 1, 1, 1])).astype(np.float32)
    cls = rng.random((n, depth, 3, PATCHES)).astype(np.float32)
    cls /= cls.sum(-1, keepdims=True)
    labels = rng.choice([c for c in range(FINALIZE_CLASSES) if c != FINALIZE_EMPTY_CLASS], size=n).astype(np.int32)
    return summary, cls.astype(np.float32), labels


def finalize_splits(n):
    """The ways the n rows arrive: at once, one row then the rest, batches of 7."""
    out = [[n]]
    if n > 1:
        out.append([1, n - 1])
    out.append([7] * (n // 7) + ([n % 7] if n % 7 else []))
    return out


# ---- the stated summation order of head_stats_step_kernel / head_stats_combine_kernel, in fp32 ---------------------------------------

def stated_order_mean(v, patch_only):
    """fp32 mean of v (..., 197) over the query rows as the kernels add it: 13 slices of 16 rows; in a slice 4 waves of 4 rows, each
    added in row order from 0; the waves ((w0 + w1) + w2) + w3; the slices in order from 0; times the fp32 constant 1/197 (1/196 with
    ``patch_only``, where row 0 is not added).  Padding rows add nothing."""
    v = np.asarray(v, dtype=np.float32)
    pad = np.zeros(v.shape[:-1] + (208,), dtype=np.float32)
    pad[..., :T] = v
    if patch_only:
        pad[..., 0] = 0.0
    g = pad.reshape(v.shape[:-1] + (13, 4, 4))
    wave = np.zeros(g.shape[:-1], dtype=np.float32)
    for r in range(4):
        wave = (wave + g[..., r]).astype(np.float32)
    wg = (((wave[..., 0] + wave[..., 1]).astype(np.float32) + wave[..., 2]).astype(np.float32) + wave[..., 3]).astype(np.float32)
    s = np.zeros(wg.shape[:-1], dtype=np.float32)
    for k in range(13):
        s = (s + wg[..., k]).astype(np.float32)
    scale = np.float32(1.0) / np.float32(196.0 if patch_only else 197.0)
    return (s * scale).astype(np.float32)
