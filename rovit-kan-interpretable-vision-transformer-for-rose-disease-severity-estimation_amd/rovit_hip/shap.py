"""Patch Shapley values of a RoViTKAN output on the GPU: KernelSHAP (Lundberg & Lee, NeurIPS 2017; the paired sampling of Covert & Lee,
AISTATS 2021) over the 196 patches or any grouping of them into players, with the value function evaluated by token gather.

A coalition S of players is an image in which the patches of the players outside S are perturbed: ``'replace'`` takes their token rows
from the baseline's table, ``'drop'`` removes their tokens from the sequence (the baseline-free missingness of Covert, Kim & Lee, ICLR
2023).  Both are sequences of rovit_vit_forward_tokens (csrc/perturb.hip), so an explanation costs one embedding of the image and M
gathered forwards, no pixel tensor.  Definitions:

  size weights   p(s) ~ (P - 1) / (s (P - s)), s = 1..P-1, normalised to 1
  pairs          every coalition is followed by its complement; a pair of class s has sizes s and P - s, s = 1..floor(P / 2)
  the plan       a pure function of (P, M): classes are enumerated from s = 1 while their full pair count fits their share of the
                 remaining budget (weight p(s) / C(P, s) per sample), the other pairs draw their class by systematic sampling and
                 their members with Philox (one weight for all of them); M = 2^P - 2 enumerates everything (exact mode)
  the fit        A = sum_m w_m z_m z_m^T, b = sum_m w_m z_m (v(S_m) - v(0)), phi = A^-1 (b - lambda 1) with lambda chosen so that
                 sum(phi) = v(all) - v(0)

``plan``, ``coalitions_reference``, ``solve_reference`` and ``shapley_exact`` are the numpy fp64 statement of all this and the oracle of
the kernels of csrc/shap.hip (rovit_shap_coalitions, rovit_shap_gram, rovit_shap_solve); on CPU tensors KernelShap runs them."""
import ctypes
import itertools
import math

import numpy as np
import torch

from . import native
from .native import MLP_AUTO, MLP_FUSED_MIN_ROWS, MLP_ONE_LAUNCH, MLP_TWO_LAUNCH, RovitHipError

NP = 196                      # patches of a 224x224 image (14 x 14)
WORDS = 7                     # 32-bit words of one packed coalition (ROVIT_SHAP_WORDS)
GRIDS = (1, 2, 7, 14)         # ``players=g``: the patch grid cut into g x g blocks
MAX_SAMPLES = native.SHAP_MAX_SAMPLES


def _philox():
    from oracle.philox import philox4x32_10
    return philox4x32_10


# ---- the plan ----------------------------------------------------------------------------------------------------------------------

def size_mass(P: int) -> np.ndarray:
    """p(s), s = 0..P (p(0) = p(P) = 0): the Shapley kernel's mass of the coalitions of size s, normalised to 1."""
    s = np.arange(1, P, dtype=np.float64)
    p = np.zeros(P + 1)
    p[1:P] = (P - 1) / (s * (P - s))
    return p / p.sum()


def min_samples(P: int) -> int:
    """The smallest budget accepted: min(2^P - 2, 4 P) (below it the system can be singular: P = 4, M = 8 is)."""
    return min(2 ** P - 2, 4 * P)


def plan(P: int, M: int) -> dict:
    """The sampling plan of (P, M), in integers and fp64 on the host.  M is made even (rounded down) and clipped to 2^P - 2.

    Returns ``P``, ``M`` (the samples actually used), ``exact`` (every class enumerated: the result is the exact Shapley value), and per
    pair k (samples 2k and 2k + 1): ``pair_class`` s, ``pair_exact`` (1: enumerated), ``pair_rank`` (enumerated: the rank of the coalition
    among the s-subsets in the order of itertools.combinations; sampled: r, the Philox counter word), ``pair_weight`` (of each of its two
    samples); per sample ``sizes`` (M,)."""
    if isinstance(P, bool) or not isinstance(P, (int, np.integer)) or not 2 <= P <= NP:
        raise RovitHipError(f'shap.plan: the number of players must be an int in [2, {NP}], got {P!r}')
    if isinstance(M, bool) or not isinstance(M, (int, np.integer)) or M < 2:
        raise RovitHipError(f'shap.plan: num_samples must be an int >= 2, got {M!r}')
    P, M = int(P), int(M)
    full_budget = 2 ** P - 2
    M = min(M - M % 2, full_budget)
    if M < min_samples(P):
        raise RovitHipError(f'shap.plan: num_samples = {M} is below min(2^P - 2, 4 P) = {min_samples(P)} for {P} players')
    if M > MAX_SAMPLES:
        raise RovitHipError(f'shap.plan: num_samples = {M} is above the limit of {MAX_SAMPLES}')
    p = size_mass(P)
    classes = list(range(1, P // 2 + 1))
    q = np.array([p[s] if 2 * s == P else 2 * p[s] for s in classes])
    full = [math.comb(P, s) // 2 if 2 * s == P else math.comb(P, s) for s in classes]
    R = M // 2
    cls, ex, rank, wt = [], [], [], []
    first = 0                                             # classes[first:] are sampled
    for k, s in enumerate(classes):
        share = R * q[k] / q[k:].sum()
        if M != full_budget and not full[k] <= share:
            break
        n = full[k]
        cls.append(np.full(n, s, np.int32))
        ex.append(np.ones(n, np.int32))
        rank.append(np.arange(n, dtype=np.int32))
        wt.append(np.full(n, p[s] / math.comb(P, s)))
        R -= n
        first = k + 1
    if R > 0:
        rem = q[first:]
        mass = rem.sum()
        cdf = np.cumsum(rem) / mass
        u = (np.arange(R, dtype=np.float64) + 0.5) / R
        pick = np.minimum(np.searchsorted(cdf, u, side='left'), len(rem) - 1)
        cls.append(np.asarray(classes[first:], np.int32)[pick])
        ex.append(np.zeros(R, np.int32))
        rank.append(np.arange(R, dtype=np.int32))
        wt.append(np.full(R, mass / (2 * R)))
    pair_class = np.concatenate(cls)
    sizes = np.stack([pair_class, P - pair_class], axis=1).reshape(-1).astype(np.int32)
    return {'P': P, 'M': M, 'exact': M == full_budget, 'pair_class': pair_class, 'pair_exact': np.concatenate(ex),
            'pair_rank': np.concatenate(rank), 'pair_weight': np.concatenate(wt), 'sizes': sizes}


def coalitions_reference(P: int, M: int, seed: int = 0):
    """(Z (M', P) bool, w (M',) float64) of plan(P, M), M' = its M.  Sampled pair r of class s: player i has the 64-bit key
    (word << 32) | i, word = word i % 4 of Philox4x32-10 with key = seed and counter (i // 4, r, SHAP_STREAM, 0); the coalition is the
    s players with the smallest keys.  A function of (P, M, seed) alone."""
    pl = plan(P, M)
    P, M = pl['P'], pl['M']
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    Z = np.zeros((M // 2, P), dtype=bool)
    k = 0
    exact = pl['pair_exact'].astype(bool)
    while k < len(exact) and exact[k]:
        s = int(pl['pair_class'][k])
        n = int((pl['pair_class'][exact] == s).sum())
        for r, c in enumerate(itertools.islice(itertools.combinations(range(P), s), n)):
            Z[k + r, list(c)] = True
        k += n
    R = M // 2 - k
    if R > 0:
        i = np.arange(P, dtype=np.uint64)
        r = np.arange(R, dtype=np.uint64)
        c0 = np.broadcast_to(i // np.uint64(4), (R, P))
        c1 = np.broadcast_to(r[:, None], (R, P))
        words = _philox()([c0, c1, np.full((R, P), native.SHAP_STREAM, np.uint64), np.zeros((R, P), np.uint64)],
                          [seed & 0xFFFFFFFF, seed >> 32])
        word = np.choose(np.broadcast_to(i % np.uint64(4), (R, P)).astype(np.int64), words)
        key = (word << np.uint64(32)) | i
        order = np.argsort(key, axis=1, kind='stable')
        pos = np.empty_like(order)
        np.put_along_axis(pos, order, np.broadcast_to(np.arange(P), (R, P)), axis=1)
        Z[k:] = pos < pl['pair_class'][k:, None]
    Zall = np.stack([Z, ~Z], axis=1).reshape(M, P)
    return Zall, np.repeat(pl['pair_weight'], 2)


def solve_reference(Z, w, y, v0, v1) -> dict:
    """The constrained weighted least-squares fit in numpy fp64.  Z (M, P) in {0, 1}, w (M,), y (M, ...) the VALUES v(S_m), v0 and v1
    (...) the values of the empty and the full coalition.  A and b are summed over m in ascending order, as the kernels do.
    Returns ``phi`` (..., P), ``fit_rmse`` (...) = sqrt(sum_m w_m (z_m . phi - (y_m - v0))^2 / sum_m w_m), ``A``, ``cond`` (of A, 2-norm),
    ``min_pivot`` (the smallest Cholesky pivot, before the square root) and ``ok``; a non-positive pivot gives NaN phi and ok = False."""
    Z = np.asarray(Z, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    v0, v1 = np.asarray(v0, dtype=np.float64), np.asarray(v1, dtype=np.float64)
    M, P = Z.shape
    tail = y.shape[1:]
    d = (y - v0).reshape(M, -1)                                         # (M, n)
    n = d.shape[1]
    A = np.zeros((P, P))
    b = np.zeros((P, n))
    for m in range(M):
        A += w[m] * np.outer(Z[m], Z[m])
        b += Z[m][:, None] * (w[m] * d[m])[None, :]
    piv, L = _cholesky(A)
    ok = bool(piv > 0.0)
    cond = float(np.linalg.cond(A)) if np.all(np.isfinite(A)) else float('inf')
    if ok:
        xu = _cholesky_solve(L, np.concatenate([b, np.ones((P, 1))], axis=1))
        x, u = xu[:, :n], xu[:, n]
        lam = (x.sum(axis=0) - (v1 - v0).reshape(-1)) / u.sum()
        phi = x - u[:, None] * lam[None, :]
        res = Z @ phi - d
        rmse = np.sqrt((w[:, None] * res * res).sum(axis=0) / w.sum())
    else:
        phi = np.full((P, n), np.nan)
        rmse = np.full(n, np.nan)
    return {'phi': np.moveaxis(phi, 0, -1).reshape(tail + (P,)), 'fit_rmse': rmse.reshape(tail), 'A': A, 'cond': cond, 'min_pivot': piv,
            'ok': ok}


def _cholesky(A):
    """(the smallest pivot met, L or None): right-looking Cholesky that stops at the first non-positive pivot."""
    L = np.array(A, dtype=np.float64)
    P = L.shape[0]
    piv = np.inf
    for k in range(P):
        piv = min(piv, L[k, k])
        if not L[k, k] > 0.0:
            return float(L[k, k]) if L[k, k] == L[k, k] else float('nan'), None
        L[k, k] = math.sqrt(L[k, k])
        L[k + 1:, k] /= L[k, k]
        L[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    return float(piv), np.tril(L)


def _cholesky_solve(L, rhs):
    """(L L^T)^-1 rhs by the two triangular solves, column-oriented."""
    x = np.array(rhs, dtype=np.float64)
    P = L.shape[0]
    for k in range(P):
        x[k] /= L[k, k]
        x[k + 1:] -= np.outer(L[k + 1:, k], x[k])
    for k in range(P - 1, -1, -1):
        x[k] /= L[k, k]
        x[:k] -= np.outer(L[k, :k], x[k])
    return x


def shapley_exact(value_fn, P: int) -> np.ndarray:
    """The Shapley values by their subset-sum definition, brute force over the 2^P coalitions: phi_i = sum over S without i of
    |S|! (P - |S| - 1)! / P! (v(S + i) - v(S)).  value_fn: bool mask (P,) -> a float or an array (...); returns (..., P) float64."""
    if not 1 <= P <= 20:
        raise RovitHipError(f'shapley_exact: brute force over 2^P coalitions, P in [1, 20], got {P}')
    vals = [np.asarray(value_fn(np.array([(c >> i) & 1 for i in range(P)], dtype=bool)), dtype=np.float64) for c in range(2 ** P)]
    wt = [math.factorial(s) * math.factorial(P - s - 1) / math.factorial(P) for s in range(P)]
    phi = np.zeros(vals[0].shape + (P,))
    for c in range(2 ** P):
        s = bin(c).count('1')
        for i in range(P):
            if not (c >> i) & 1:
                phi[..., i] += wt[s] * (vals[c | (1 << i)] - vals[c])
    return phi


# ---- players -----------------------------------------------------------------------------------------------------------------------

def player_map(players, what='KernelShap') -> np.ndarray:
    """(196,) int32 patch -> player id from ``players``: an int g out of (1, 2, 7, 14) cuts the 14 x 14 patch grid into g x g equal
    blocks (P = g^2; g = 1 leaves one player and is refused), a (196,) integer map is taken as it is (ids 0..P-1, every id used)."""
    if isinstance(players, bool):
        raise RovitHipError(f'{what}: players must be an int out of {list(GRIDS)} or a (196,) integer map, got {players!r}')
    if isinstance(players, (int, np.integer)):
        g = int(players)
        if g not in GRIDS:
            raise RovitHipError(f'{what}: players must be an int out of {list(GRIDS)} or a (196,) integer map, got {players!r}')
        if g == 1:
            raise RovitHipError(f'{what}: players = 1 leaves one player; Shapley values need 2 <= P <= {NP}')
        r = np.arange(14) // (14 // g)
        return (r[:, None] * g + r[None, :]).reshape(NP).astype(np.int32)
    if isinstance(players, torch.Tensor):
        if players.dtype.is_floating_point or players.dtype.is_complex or players.dtype == torch.bool:
            raise RovitHipError(f'{what}: a players map must hold integers, got {players.dtype}')
        arr = players.detach().cpu().numpy()
    else:
        try:
            arr = np.asarray(players)
        except Exception:
            arr = None
        if arr is None or arr.dtype.kind not in 'iu':
            raise RovitHipError(f'{what}: players must be an int out of {list(GRIDS)} or a (196,) integer map, got {type(players).__name__}')
    if arr.size != NP or arr.shape not in ((NP,), (14, 14)):
        raise RovitHipError(f'{what}: a players map must have shape (196,) or (14, 14), got {tuple(arr.shape)}')
    arr = arr.reshape(NP).astype(np.int64)
    P = int(arr.max()) + 1
    if arr.min() < 0 or not 2 <= P <= NP or len(np.unique(arr)) != P:
        raise RovitHipError(f'{what}: a players map must use every id of 0..P-1 with 2 <= P <= {NP}; got ids in [{int(arr.min())}, '
                            f'{int(arr.max())}], {len(np.unique(arr))} of them distinct')
    return arr.astype(np.int32)


def pack_bits(Z: np.ndarray) -> np.ndarray:
    """(M, 7) uint32 of (M, P) bool: player i is bit i % 32 of word i // 32."""
    M, P = Z.shape
    full = np.zeros((M, WORDS * 32), dtype=np.uint64)
    full[:, :P] = Z
    sh = np.arange(32, dtype=np.uint64)
    return (full.reshape(M, WORDS, 32) << sh).sum(axis=2).astype(np.uint32)


def unpack_bits(bits: torch.Tensor, P: int) -> torch.Tensor:
    """(M, P) bool of packed coalitions (M, 7) int32 / uint32, on the tensor's device."""
    b = bits.view(torch.int32) if bits.dtype != torch.int32 else bits
    i = torch.arange(P, device=b.device)
    return ((b[:, i // 32] >> (i % 32)) & 1).bool()


def _drop_layout(kept: np.ndarray):
    """Sequences of equal length packed together.  kept (M,): kept patches per sample.  Returns (offsets (M,) int64 into one flat int32
    buffer, total words, groups [(tokens, sample indices ascending, first word)]) with the groups in ascending token count."""
    tokens = kept.astype(np.int64) + 1
    off = np.zeros(len(kept), dtype=np.int64)
    groups, at = [], 0
    for t in np.unique(tokens):
        idx = np.nonzero(tokens == t)[0]
        off[idx] = at + np.arange(len(idx), dtype=np.int64) * int(t)
        groups.append((int(t), idx, at))
        at += len(idx) * int(t)
    return off, at, groups


class KernelShap:
    """The KernelSHAP estimator of one (players, num_samples, seed): its coalitions and the fit, for any value function.

    ``players``: an int g out of (2, 7, 14) or a (196,) patch -> player map (``player_map``); the coalitions then come with the ``src``
    rows of rovit_vit_forward_tokens.  ``num_players=P`` instead names an abstract game of P players without patches.
    ``num_samples`` is made even and clipped to 2^P - 2; below min(2^P - 2, 4 P) it is refused.
    ``max_workgroups`` > 0 caps every grid (tests); no result depends on it."""

    def __init__(self, players=None, num_samples: int = 2048, seed: int = 0, *, num_players=None):
        what = 'KernelShap'
        if (players is None) == (num_players is None):
            raise RovitHipError(f'{what}: give players (a grid size or a patch map) or num_players, not both')
        self.players = None if players is None else player_map(players, what)
        P = int(self.players.max()) + 1 if self.players is not None else num_players
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise RovitHipError(f'{what}: seed must be an int in [0, 2^64), got {seed!r}')
        self.plan = plan(P, num_samples)
        self.P, self.M, self.exact, self.seed = self.plan['P'], self.plan['M'], self.plan['exact'], int(seed)
        self.max_workgroups = 0
        self._design = None                    # from_design: (Z, w) given by hand
        self._cache = {}

    @classmethod
    def from_design(cls, Z, w, players=None):
        """An estimator over a hand-made design: Z (M, P) in {0, 1} and weights w (M,) instead of the plan's (any M >= 1)."""
        Z = np.asarray(Z).astype(bool)
        w = np.asarray(w, dtype=np.float64)
        if Z.ndim != 2 or not 2 <= Z.shape[1] <= NP or w.shape != (Z.shape[0],) or not 1 <= Z.shape[0] <= MAX_SAMPLES:
            raise RovitHipError(f'KernelShap.from_design: Z must be (M, P) with 2 <= P <= {NP} and w (M,), got {Z.shape} and {w.shape}')
        self = cls.__new__(cls)
        self.players = None if players is None else player_map(players, 'KernelShap.from_design')
        if self.players is not None and int(self.players.max()) + 1 != Z.shape[1]:
            raise RovitHipError(f'KernelShap.from_design: the players map names {int(self.players.max()) + 1} players, Z has {Z.shape[1]}')
        self.plan, self.P, self.M, self.exact, self.seed = None, Z.shape[1], Z.shape[0], False, 0
        self.max_workgroups = 0
        self._design = (Z, w)
        self._cache = {}
        return self

    # -- coalitions ----------------------------------------------------------------------------------------------------------------

    def kept_patches(self) -> np.ndarray:
        """(M,) patches each sample keeps.  Players of equal patch count: from the plan's sizes; otherwise from the host reference."""
        counts = np.bincount(self.players, minlength=self.P)
        if self._design is None and np.all(counts == counts[0]):
            return self.plan['sizes'].astype(np.int64) * int(counts[0])
        Z = self._design[0] if self._design is not None else coalitions_reference(self.P, self.M, self.seed)[0]
        return Z.astype(np.int64) @ counts.astype(np.int64)

    def coalitions(self, device='cuda') -> dict:
        """The coalitions on ``device``: ``bits`` (M, 7) int32 packed (player i: bit i % 32 of word i // 32), ``weights`` (M,) float64 and,
        with a patch map, ``src_replace`` (M, 197) int32 and ``src_drop``: a list of (tokens, sample indices (n,) int64, src (n, tokens)
        int32), one entry per sequence length in ascending order -- the rows perturbation.source_rows builds from the same masks.
        Sample 2k + 1 is the complement of sample 2k.  On a CPU device the numpy reference builds them."""
        dev = torch.device(device)
        key = (str(dev), self.max_workgroups)
        if key in self._cache:
            return self._cache[key]
        out = self._coalitions_cpu() if dev.type != 'cuda' else self._coalitions_gpu(dev)
        self._cache[key] = out
        return out

    def _coalitions_cpu(self) -> dict:
        from .perturbation import source_rows
        Z, w = self._design if self._design is not None else coalitions_reference(self.P, self.M, self.seed)
        out = {'bits': torch.from_numpy(pack_bits(Z).view(np.int32).copy()), 'weights': torch.from_numpy(np.array(w, dtype=np.float64))}
        if self.players is not None:
            absent = torch.from_numpy(~Z[:, self.players])
            out['src_replace'] = source_rows(absent, 'replace')
            _, _, groups = _drop_layout(self.kept_patches())
            out['src_drop'] = [(t, torch.from_numpy(idx), source_rows(absent[torch.from_numpy(idx)], 'drop', t)) for t, idx, _ in groups]
        return out

    def _coalitions_gpu(self, dev) -> dict:
        if self._design is not None:
            Z, w = self._design
            out = {'bits': torch.from_numpy(pack_bits(Z).view(np.int32).copy()).to(dev), 'weights': torch.from_numpy(np.array(w)).to(dev)}
            if self.players is not None:
                cpu = self._coalitions_cpu()
                out['src_replace'] = cpu['src_replace'].to(dev)
                out['src_drop'] = [(t, i.to(dev), s.to(dev)) for t, i, s in cpu['src_drop']]
            return out
        pl, M = self.plan, self.M
        tab = np.stack([pl['pair_class'], pl['pair_exact'], pl['pair_rank'], np.zeros(M // 2, np.int32)], axis=1).astype(np.int32)
        with torch.cuda.device(dev):
            pairs = torch.from_numpy(tab).pin_memory().to(dev, non_blocking=True)
            pair_w = torch.from_numpy(pl['pair_weight']).pin_memory().to(dev, non_blocking=True)
            bits = torch.empty(M, WORDS, dtype=torch.int32, device=dev)
            weights = torch.empty(M, dtype=torch.float64, device=dev)
            a = native.ShapCoalitionArgs()
            a.num_players, a.num_samples, a.max_workgroups, a.seed = self.P, M, self.max_workgroups, self.seed
            a.pairs, a.pair_weights, a.bits, a.weights = native.ptr(pairs), native.ptr(pair_w), native.ptr(bits), native.ptr(weights)
            out = {'bits': bits, 'weights': weights}
            if self.players is not None:
                off, words, groups = _drop_layout(self.kept_patches())
                pmap = torch.from_numpy(self.players).pin_memory().to(dev, non_blocking=True)
                offs = torch.from_numpy(off).pin_memory().to(dev, non_blocking=True)
                src_rep = torch.empty(M, NP + 1, dtype=torch.int32, device=dev)
                src_drop = torch.empty(words, dtype=torch.int32, device=dev)
                a.players, a.src_replace, a.src_drop = native.ptr(pmap), native.ptr(src_rep), native.ptr(src_drop)
                a.drop_offsets, a.drop_words = native.ptr(offs), words
                out['src_replace'] = src_rep
                out['src_drop'] = [(t, torch.from_numpy(idx).to(dev, non_blocking=True), src_drop[at:at + len(idx) * t].view(len(idx), t))
                                   for t, idx, at in groups]
            native.call('rovit_shap_coalitions', ctypes.byref(a), native.stream_ptr())
        return out

    # -- the fit -------------------------------------------------------------------------------------------------------------------

    def solve(self, values: torch.Tensor, v_empty: torch.Tensor, v_full: torch.Tensor) -> dict:
        """The fit for values (M, B, T) or (M, B) of ANY value function on this estimator's coalitions, with v_empty and v_full (B, T) or
        (B,).  Returns ``phi`` (B, T, P) float64, ``phi32`` the same in fp32, ``fit_rmse`` (B, T) float64, ``ok`` (B, T) bool,
        ``min_pivot`` () float64 and, with a patch map, ``patch_map`` (B, T, 196) fp32: a player's value divided evenly over its patches.
        (Without the T axis in, without it out.)  A non-positive Cholesky pivot gives NaN phi and ok = False as device values; nothing is
        read back.  On CPU tensors the numpy reference runs."""
        what = 'KernelShap.solve'
        if not isinstance(values, torch.Tensor) or values.dim() not in (2, 3) or values.shape[0] != self.M or not values.dtype.is_floating_point:
            raise RovitHipError(f'{what}: values must be a floating (M, B) or (M, B, T) tensor with M = {self.M}, got '
                                f'{tuple(values.shape) if isinstance(values, torch.Tensor) else type(values).__name__}')
        flat = values.dim() == 2
        B, T = values.shape[1], 1 if flat else values.shape[2]
        if B < 1 or T < 1:
            raise RovitHipError(f'{what}: empty values {tuple(values.shape)}')
        for name, v in (('v_empty', v_empty), ('v_full', v_full)):
            if not isinstance(v, torch.Tensor) or tuple(v.shape) != tuple(values.shape[1:]) or v.device != values.device:
                raise RovitHipError(f'{what}: {name} must be a {tuple(values.shape[1:])} tensor on {values.device}')
        dev = values.device
        if not values.is_cuda:
            out = self._solve_cpu(values, v_empty, v_full, B, T)
        else:
            out = self._solve_gpu(values.detach().float().reshape(self.M, B, T).contiguous(), v_empty.detach().float().reshape(B, T).contiguous(),
                                  v_full.detach().float().reshape(B, T).contiguous(), B, T, dev)
        if flat:
            out = {k: (v.squeeze(1) if k != 'min_pivot' else v) for k, v in out.items()}
        return out

    def _solve_cpu(self, values, v_empty, v_full, B, T) -> dict:
        Z, w = self._design if self._design is not None else coalitions_reference(self.P, self.M, self.seed)
        r = solve_reference(Z, w, values.float().reshape(self.M, B, T).numpy(), v_empty.float().reshape(B, T).numpy(),
                            v_full.float().reshape(B, T).numpy())
        phi = torch.from_numpy(r['phi'])
        out = {'phi': phi, 'phi32': phi.float(), 'fit_rmse': torch.from_numpy(np.asarray(r['fit_rmse'])),
               'ok': torch.full((B, T), r['ok'], dtype=torch.bool), 'min_pivot': torch.tensor(r['min_pivot'], dtype=torch.float64)}
        if self.players is not None:
            counts = np.bincount(self.players, minlength=self.P).astype(np.float64)
            out['patch_map'] = torch.from_numpy((r['phi'] / counts)[..., self.players]).float()
        return out

    def factor(self, device) -> dict:
        """A = sum_m w_m z_m z_m^T and its Cholesky factor on ``device`` (rovit_shap_gram), once per estimator and device: ``gram`` (P, P)
        float64 and the block ``factor`` the solve reads (native.shap_factor_offsets)."""
        dev = torch.device(device)
        key = ('factor', str(dev), self.max_workgroups)
        if key not in self._cache:
            co = self.coalitions(dev)
            P = self.P
            with torch.cuda.device(dev):
                gram = torch.empty(P, P, dtype=torch.float64, device=dev)
                fac = torch.empty(native.shap_factor_offsets(P)['words'], dtype=torch.float64, device=dev)
                a = native.ShapGramArgs()
                a.num_players, a.num_samples, a.max_workgroups = P, self.M, self.max_workgroups
                a.bits, a.weights, a.gram, a.factor = native.ptr(co['bits']), native.ptr(co['weights']), native.ptr(gram), native.ptr(fac)
                native.call('rovit_shap_gram', ctypes.byref(a), native.stream_ptr())
            self._cache[key] = {'gram': gram, 'factor': fac}
        return self._cache[key]

    def _solve_gpu(self, values, v_empty, v_full, B, T, dev) -> dict:
        co, fa = self.coalitions(dev), self.factor(dev)
        P = self.P
        with torch.cuda.device(dev):
            phi = torch.empty(B, T, P, dtype=torch.float64, device=dev)
            phi32 = torch.empty(B, T, P, dtype=torch.float32, device=dev)
            rmse = torch.empty(B, T, dtype=torch.float64, device=dev)
            ok = torch.empty(B, T, dtype=torch.int32, device=dev)
            pmap = pm = None
            if self.players is not None:
                pmap = torch.from_numpy(self.players).pin_memory().to(dev, non_blocking=True)
                pm = torch.empty(B, T, NP, dtype=torch.float32, device=dev)
            a = native.ShapSolveArgs()
            a.num_players, a.num_samples, a.batch, a.num_targets, a.max_workgroups = P, self.M, B, T, self.max_workgroups
            a.bits, a.weights, a.factor = native.ptr(co['bits']), native.ptr(co['weights']), native.ptr(fa['factor'])
            a.values, a.v_empty, a.v_full, a.players = native.ptr(values), native.ptr(v_empty), native.ptr(v_full), native.ptr(pmap)
            a.phi, a.phi32, a.patch_map, a.fit_rmse, a.ok = native.ptr(phi), native.ptr(phi32), native.ptr(pm), native.ptr(rmse), native.ptr(ok)
            native.call('rovit_shap_solve', ctypes.byref(a), native.stream_ptr())
        out = {'phi': phi, 'phi32': phi32, 'fit_rmse': rmse, 'ok': ok.bool(),
               'min_pivot': fa['factor'][native.shap_factor_offsets(P)['min_pivot']]}
        if pm is not None:
            out['patch_map'] = pm
        return out


# ---- the model call ------------------------------------------------------------------------------------------------------------------

def _check(model, x, target, class_idx, num_samples, players, perturbation, baseline, seed, chunk, upsample, return_values, ragged=False):
    from .gradcam import _target_names
    from .input_grad import _check_args
    from .perturbation import PERTURBATIONS
    what = 'patch_shap'
    if perturbation not in PERTURBATIONS:
        raise RovitHipError(f'{what}: perturbation must be one of {list(PERTURBATIONS)}, got {perturbation!r}')
    if perturbation == 'drop' and baseline is not None:
        raise RovitHipError(f"{what}: perturbation='drop' removes patches from the sequence and takes no baseline")
    pmap = player_map(players, what)
    counts = np.bincount(pmap)
    if perturbation == 'drop' and not np.all(counts == counts[0]):
        raise RovitHipError(f"{what}: perturbation='drop' needs players of equal patch count (the sequence lengths are then known without "
                            f"reading the coalitions back); got between {int(counts.min())} and {int(counts.max())} patches per player")
    try:
        ks = KernelShap(pmap, num_samples, seed)
    except RovitHipError as e:
        raise RovitHipError(f'{what}: {e}') from None
    for name, flag in (('upsample', upsample), ('return_values', return_values), ('ragged', ragged)):
        if not isinstance(flag, bool):
            raise RovitHipError(f'{what}: {name} must be a bool, got {flag!r}')
    stage = getattr(model, 'curriculum_stage', None)
    if not isinstance(stage, int):
        raise RovitHipError(f'{what}: expects a RoViTKAN, got {type(model).__name__}')
    names, several = _target_names(target, class_idx, stage)
    targets = None
    for n in names:      # the images, class_idx, baseline (broadcast to x, x's device), chunk and head shapes as input_gradients checks them
        t = _check_args(model, x, n, class_idx if n == 'class' else None, 1, baseline, chunk, what)
        targets = t if n == 'class' else targets
    return names, several, targets, ks


def patch_shap(model, x: torch.Tensor, target='class', class_idx=None, num_samples: int = 2048, players=14, perturbation: str = 'drop',
               baseline=None, seed: int = 0, chunk: int = 256, upsample: bool = True, return_values: bool = False, ragged: bool = False):
    """KernelSHAP values of the players of every image for one RoViTKAN output (or several: a list / tuple of targets is explained from
    the same forwards and returns a dict name -> result).

    ``target``, ``class_idx``, ``baseline`` and ``chunk`` as perturbation_curves: ``'class'`` is the softmax probability of c_b
    (``class_idx`` None: each image's argmax at the unperturbed image), the others as input_gradients.
    ``players``: g out of (2, 7, 14) -- the patch grid in g x g blocks, P = g^2 -- or a (196,) patch -> player map (superpixels, lesion
    segments).  ``num_samples`` M is made even and clipped to 2^P - 2, where the result is the exact Shapley value; below
    min(2^P - 2, 4 P) it is refused.  The coalitions depend on (P, M, seed) only, never on the image or the batch.
    ``perturbation='drop'`` (default): the patches of absent players leave the sequence; needs players of equal patch count and takes no
    baseline.  ``'replace'``: they are ``baseline``'s (default zeros).

    Returns ``{'shap': (B,224,224) -- each pixel 1/256 of its patch's value, so the map sums to value - base_value -- or (B,14,14) with
    upsample=False, a player's value divided evenly over its patches; 'player_values': (B,P); 'base_value': (B,) v(nothing); 'value': (B,)
    v(image); 'fit_rmse': (B,) the weighted residual RMS of the fit; 'ok': (B,) bool (False with NaN values when A is not positive
    definite); 'exact': bool; 'num_samples': M; 'class_idx': (B,) for 'class'}``, fp32 on x's device; ``return_values=True`` adds
    ``'values'`` (M, B), the value of every coalition, and ``'coalitions'`` (M, P) bool.  player_values.sum(1) = value - base_value by
    construction.

    Eval semantics, as input_gradients: the bf16 engine whatever ``precision`` says, no dropout, no ``.grad`` written, flags untouched.
    Sequences of equal length are packed into backbone calls of ``chunk``; the MLP path is the engine's override or is chosen from
    ``chunk`` x tokens, never from a call's size, so an image's values do not depend on the others of the batch.  ``ragged=True`` with
    ``'drop'``: the sequences of ALL lengths are packed, longest first, into calls of ``chunk`` x 197 rows (rovit_hip.ragged,
    rovit_vit_forward_ragged) -- sampled coalitions of 196 players come in about 197 lengths, and this makes a handful of backbone calls
    of them; the MLP path is then the engine's override or chosen from ``chunk`` x 197 alone, so a short sequence may take the other
    path than with ``ragged=False`` (the two agree to bf16 rounding, not bit for bit: the default stays False).  With ``'replace'`` the
    flag changes nothing.  Every bad argument is refused (RovitHipError) before anything is launched."""
    from .functions import VitEngine
    from .input_grad import _Backbone, _head_outputs, _target_value
    from .perturbation import source_rows
    names, several, targets, ks = _check(model, x, target, class_idx, num_samples, players, perturbation, baseline, seed, chunk, upsample,
                                         return_values, ragged)
    dev = x.device
    B, M, P = x.shape[0], ks.M, ks.P
    with torch.no_grad():
        x32 = x.detach().float().contiguous()
        bb = _Backbone(model, dev)
        img_t = torch.empty(B, 197, 192, device=dev, dtype=torch.float32)
        for b0 in range(0, B, chunk):
            bb.embed(x32[b0:b0 + chunk], img_t[b0:b0 + chunk])
        base_shared = 0
        base_t = img_t                       # 'drop' reads no baseline row
        if perturbation == 'replace':
            xb = torch.zeros(1, 3, 224, 224, device=dev) if baseline is None else baseline.detach().float()
            base_shared = int(xb.dim() < 4 or xb.shape[0] == 1)
            xb = xb.expand(1 if base_shared else B, 3, 224, 224).contiguous()
            base_t = torch.empty(xb.shape[0], 197, 192, device=dev, dtype=torch.float32)
            for b0 in range(0, xb.shape[0], chunk):
                bb.embed(xb[b0:b0 + chunk], base_t[b0:b0 + chunk])
        co = ks.coalitions(dev)
        # rows of raw: the M coalitions, then the full image (M) and the empty coalition (M + 1), each computed once per image
        ends = torch.tensor([[False] * NP, [True] * NP], device=dev)
        groups = {}                           # tokens -> [(raw rows (n,), src (n, tokens))]
        if perturbation == 'replace':
            groups[197] = [(torch.arange(M, device=dev), co['src_replace']), (torch.tensor([M, M + 1], device=dev), source_rows(ends, 'replace'))]
        else:
            for t, idx, src in co['src_drop']:
                groups[t] = [(idx, src)]
            groups.setdefault(197, []).append((torch.tensor([M], device=dev), source_rows(ends[:1], 'drop', 197)))
            groups.setdefault(1, []).append((torch.tensor([M + 1], device=dev), source_rows(ends[1:], 'drop', 1)))
        override = bb.eng.mlp_path if bb.eng.mlp_path is not None else VitEngine.default_mlp_path
        C_ = model.classification_head.fc2.out_features
        others = [n for n in names if n != 'class']
        raw_cls = torch.empty(M + 2, B, C_, device=dev, dtype=torch.float32) if 'class' in names else None
        raw_oth = torch.empty(M + 2, B, len(others), device=dev, dtype=torch.float32) if others else None
        if ragged and perturbation == 'drop':
            from . import ragged as rg
            max_rows = chunk * 197
            mlp = override if override != MLP_AUTO else (MLP_ONE_LAUNCH if max_rows >= MLP_FUSED_MIN_ROWS else MLP_TWO_LAUNCH)
            # every coalition's rows in one flat buffer: the groups in ascending length (_drop_layout's offsets), the full image, nothing
            kept = ks.kept_patches()
            woff, words, _ = _drop_layout(kept)
            flat = torch.cat([s_.reshape(-1) for _, _, s_ in co['src_drop']]
                             + [source_rows(ends[:1], 'drop', 197).reshape(-1), source_rows(ends[1:], 'drop', 1).reshape(-1)])
            woff_d = torch.from_numpy(np.concatenate([woff, [words, words + 197]])).to(dev)
            lengths = np.repeat(np.concatenate([kept + 1, [197, 1]]), B)                    # sequences coalition-major, images inside
            calls, _ = rg.ragged_layout(lengths, max_rows)
            ws = rg.take_ws(bb.eng, max_rows, dev)
            for seq, off in calls:
                j = torch.from_numpy(seq).to(dev)
                ci, b = j // B, j % B
                off_d, seq_of_row, pos = rg.packed_rows(off, dev)
                src = flat[woff_d[ci][seq_of_row] + pos].contiguous()
                feats = bb.forward_ragged(img_t, base_t, 0, b.int(), src, off_d, off, ws, mlp)
                outs = _head_outputs(model, feats)
                if raw_cls is not None:
                    raw_cls[ci, b] = outs[0].float()
                for k, n in enumerate(others):
                    raw_oth[ci, b, k] = _target_value(n, outs, None).float()
            bb.eng.give_ws(max_rows, 'ragged', ws)
        else:
            cap = min(chunk, max(sum(len(r) for r, _ in g) for g in groups.values()) * B)
            ws = bb.eng.take_ws(cap, False, dev)
            for tokens, parts in groups.items():
                mlp = override if override != MLP_AUTO else (MLP_ONE_LAUNCH if chunk * tokens >= MLP_FUSED_MIN_ROWS else MLP_TWO_LAUNCH)
                rows = torch.cat([r for r, _ in parts])
                src_g = torch.cat([s for _, s in parts]) if len(parts) > 1 else parts[0][1]
                total = rows.shape[0] * B
                for j0 in range(0, total, chunk):
                    j = torch.arange(j0, min(total, j0 + chunk), device=dev)
                    ci, b = j // B, j % B                                  # sequences coalition-major, images inside
                    feats = bb.forward_tokens(img_t, base_t, base_shared, b.int(), src_g[ci].contiguous(), ws, mlp)
                    outs = _head_outputs(model, feats)
                    if raw_cls is not None:
                        raw_cls[rows[ci], b] = outs[0].float()
                    for k, n in enumerate(others):
                        raw_oth[rows[ci], b, k] = _target_value(n, outs, None).float()
            bb.eng.give_ws(cap, False, ws)
        cols = []
        cls = None
        for n in names:
            if n == 'class':
                cls = targets.long() if targets is not None else raw_cls[M].argmax(dim=1)
                cols.append(torch.softmax(raw_cls, dim=2).gather(2, cls.view(1, B, 1).expand(M + 2, B, 1)).squeeze(2))
            else:
                cols.append(raw_oth[:, :, others.index(n)])
        vals = torch.stack(cols, dim=2).contiguous()                   # (M + 2, B, T)
        fit = ks.solve(vals[:M], vals[M + 1], vals[M])
        Z = unpack_bits(co['bits'], P) if return_values else None
        results = {}
        for k, n in enumerate(names):
            pm = fit['patch_map'][:, k].reshape(B, 14, 14)
            if upsample:
                pm = (pm * (1.0 / 256.0)).view(B, 14, 1, 14, 1).expand(B, 14, 16, 14, 16).reshape(B, 224, 224)
            r = {'shap': pm.contiguous(), 'player_values': fit['phi32'][:, k].contiguous(), 'base_value': vals[M + 1, :, k].contiguous(),
                 'value': vals[M, :, k].contiguous(), 'fit_rmse': fit['fit_rmse'][:, k].float(), 'ok': fit['ok'][:, k].contiguous(),
                 'exact': ks.exact, 'num_samples': M}
            if n == 'class':
                r['class_idx'] = cls
            if return_values:
                r['values'] = vals[:M, :, k].contiguous()
                r['coalitions'] = Z
            results[n] = r
    return results if several else results[names[0]]
