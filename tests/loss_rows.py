"""Shared by tests/test_gpu_loss_rows.py and tests/test_loss_rows_cpu.py (no test in here): the edge grid of the fused joint loss
(csrc/joint_loss_row.h), a closed-form fp64 reference of every row of it, the per-row comparator, and an fp32 emulation of
joint_loss::row that stands in the kernel's place where there is no GPU.

The grid is built from named families, so a failure names its family and its row.  A `case` is one launch: a batch of rows (numpy
arrays, fp32 head outputs, int64 labels, int64 or fp32 severities) with the launch's scalars (C, gamma, alpha, lam, stage):
    focal        rows [off + gap, fillers in (off - gap, off], off - gap]: the softmax from a tie to p_t -> 1 and p_t -> 0, the logits
                 around 0, around +-30 and around +-1000; the target at the largest logit, at a filler and at the smallest
    ordinal      logits from 0 to the point where 1 + exp(-|x|) rounds to 1 and to +-100, severities on both sides of every threshold,
                 int64 and fp32 (fractional, and exactly on a threshold)
    uncertainty  log_var from clamp to clamp of the heads (+-10), residuals from 0 to 20
    kan          predictions on, next to and away from the label
    batch        all four grids cycled to batch sizes on either side of a wave and of the kernel's 256-thread loop, stages 1 to 4
In every family the heads that are not its subject hold mild values, so that a failure there points at the subject.

Everything is compared as the per-sample gradient G = B * d(total)/d(output): the kernels' gradients carry a factor 1/B, and a bound
taken over the whole tensor, 1e-5 max(1, max |g|), lets every entry of a batch of 1000 be 1 % wrong.  Per row and per head the bound is
the project's own, 1e-5 max(1, max_j |G_ref[row]|)."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from training_fp64 import HEADS, LOSSES

FAMILIES = ('focal', 'ordinal', 'uncertainty', 'kan', 'batch')
GAPS = (0.0, 2.0 ** -10, 1.0, 5.0, 10.0, 15.0, 16.5, 17.0, 20.0, 30.0, 40.0, 80.0, 88.0, 100.0, 120.0)
OFFS = (0.0, 30.0, -30.0, 1000.0, -1000.0)
CS = (2, 4, 16)                                  # 16 is joint_loss::MAXC
GAMMAS = (0.0, 0.5, 1.0, 2.0, 5.0)
LAMS = (0.0, 0.3, 1.0)
ORD_X = (0.0, 2.0 ** -20, -2.0 ** -20, 1.0, -1.0, 10.0, -10.0, 16.6, -16.6, 17.0, -17.0, 30.0, -30.0, 88.0, -88.0, 100.0, -100.0)
LOG_VARS = (-10.0, -9.999, -1.0, 0.0, 1.0, 10.0)          # the uncertainty head clamps log_var to +-10
RESIDUALS = (0.0, 2.0 ** -12, -2.0 ** -12, 1.0, -1.0, 3.0, -3.0, 20.0, -20.0)          # y - mu
KAN_KINDS = ('y', 'y+', 'y-', '0', '1.5', '3')
BATCH_SIZES = (1, 63, 64, 65, 255, 256, 257, 511, 513)
LAMBDA_ORD, MU_UNC, NU_KAN = 1.0, 0.5, 0.5
GRAD_TOL = LOSS_TOL = 1e-5
DIRECT_BELOW = 4.0          # joint_loss::DIRECT_BELOW; test_loss_rows_cpu.py reads the header and holds the two together
GATE = {'cls_logits': 1, 'ordinal_logits': 2, 'mu': 3, 'log_var': 3, 'kan_severity': 4}
F32 = np.float32


def alpha_of(C):
    """focal_alpha with unequal entries: a wrong alpha[t] moves a row by at least a fifth."""
    return (0.5 + 0.25 * ((3 * np.arange(C)) % 5)).astype(F32)


# ---- the heads' grids, one row per index ---------------------------------------------------------------------------------------------------

def _target_positions(C):
    """(name, column): the largest logit, a filler, the smallest.  C = 2 has no filler."""
    return (('max', 0), ('min', 1)) if C == 2 else (('max', 0), ('filler', C // 2), ('min', C - 1))


_FILL_U = np.random.default_rng(20240).random((len(GAPS), 14))          # the only random numbers of the grid: where the fillers sit


def focal_pool(C):
    """Every (gap, off, target) of the focal family -> logits (R, C) fp32, labels a and b, the rows' names, offsets and gaps.  The
    fillers of a gap sit at the same fractions of it at every offset, so the rows of one gap are shifts of one another.  Label b
    equals label a in the even rows and is the next target position in the odd ones."""
    pos = _target_positions(C)
    z, ta, tb, names, offs, gaps = [], [], [], [], [], []
    for gi, gap in enumerate(GAPS):
        for off in OFFS:
            row = np.empty(C)
            row[0], row[C - 1] = off + gap, off - gap
            row[1:C - 1] = off - gap * _FILL_U[gi, :C - 2]
            for pi, (pname, col) in enumerate(pos):
                r = len(z)
                z.append(row)
                ta.append(col)
                tb.append(col if r % 2 == 0 else pos[(pi + 1) % len(pos)][1])
                names.append(f'gap {gap:g} off {off:g} target {pname}')
                offs.append(off)
                gaps.append(gap)
    return SimpleNamespace(cls=np.asarray(z).astype(F32), ta=np.asarray(ta, dtype=np.int64), tb=np.asarray(tb, dtype=np.int64), names=names,
                           off=np.asarray(offs), gap=np.asarray(gaps))


def ordinal_severities(C, as_float):
    if as_float:          # fractional, exactly on a threshold (1.0 > 1 is false), below and above every threshold
        s = [0.0, 0.5, 1.0, 2.999, float(C - 1)] + ([7.0, 14.5] if C == 16 else [])
        return np.asarray(s, dtype=F32)
    return np.asarray(sorted({0, 1, C - 1} | ({8} if C == 16 else set())), dtype=np.int64)


def ordinal_head(idx, K1):
    """Threshold k of row i holds ORD_X[(i + k) % 17]: every value meets every severity at k = 0."""
    x = np.asarray(ORD_X)
    return x[(np.asarray(idx).reshape(-1, 1) + np.arange(K1).reshape(1, -1)) % len(x)].astype(F32)


def uncertainty_head(y, idx):
    """mu = y - RESIDUALS[i % 9] (exact in fp32 for the small integer labels used), log_var = LOG_VARS[(i // 9) % 6]."""
    idx = np.asarray(idx)
    r, lv = np.asarray(RESIDUALS)[idx % 9], np.asarray(LOG_VARS)[(idx // 9) % 6]
    return (y.astype(np.float64) - r).astype(F32).reshape(-1, 1), lv.astype(F32).reshape(-1, 1)


def kan_head(y, idx):
    y = y.astype(np.float64)
    kinds = np.stack([y, y + 2.0 ** -20, y - 2.0 ** -20, np.zeros_like(y), np.full_like(y, 1.5), np.full_like(y, 3.0)], axis=1)
    return kinds[np.arange(len(y)), np.asarray(idx) % 6].astype(F32).reshape(-1, 1)


def _mild(B, C, y):
    """Mild values for the heads that are not a family's subject: logits within +-1, residual 1, log_var 0, prediction 1.5."""
    i = np.arange(B)
    cls = np.tile((((np.arange(C) * 7) % 5 - 2) * 0.5).astype(F32), (B, 1))
    ordl = np.tile(np.where(np.arange(C - 1) % 2 == 0, 1.0, -1.0).astype(F32), (B, 1))
    return dict(cls=cls, ta=(i % C).astype(np.int64), tb=((i + 1) % C).astype(np.int64), ord=ordl,
                mu=(y.astype(np.float64) - 1.0).astype(F32).reshape(-1, 1), lv=np.zeros((B, 1), F32), kan=np.full((B, 1), 1.5, F32))


def make_case(family, name, C, sev, rows, names, gamma=2.0, alpha=True, lam=None, stage=4, off=None, gap=None):
    B = len(sev)
    d = _mild(B, C, sev)
    d.update(rows)
    return SimpleNamespace(family=family, name=name, B=B, C=C, sev=sev, names=list(names), gamma=float(gamma),
                           alpha=alpha_of(C) if alpha else None, lam=lam, stage=stage,
                           off=np.full(B, np.nan) if off is None else off, gap=np.full(B, np.nan) if gap is None else gap, **d)


def family_cases(family):
    """The launches of one family.  lam None is the unmixed loss (rovit_joint_loss, and rovit_joint_loss_mixed without a second label
    column); a float is rovit_joint_loss_mixed with label column b."""
    out = []
    if family == 'focal':
        for C in CS:
            p = focal_pool(C)
            sev = (np.arange(len(p.ta)) % C).astype(np.int64)
            rows = dict(cls=p.cls, ta=p.ta, tb=p.tb)
            for gamma in GAMMAS:
                for alpha in (False, True):
                    for lam in (None,) + LAMS:
                        out.append(make_case(family, f'C {C} gamma {gamma:g} alpha {alpha} lam {lam}', C, sev, rows, p.names, gamma, alpha, lam,
                                         off=p.off, gap=p.gap))
    elif family == 'ordinal':
        for C in CS:
            for as_float in (False, True):
                sevs = ordinal_severities(C, as_float)
                xi, si = np.meshgrid(np.arange(len(ORD_X)), np.arange(len(sevs)), indexing='ij')
                xi, sev = xi.reshape(-1), sevs[si.reshape(-1)]
                names = [f'x[0] {ORD_X[i]:g} severity {s:g}' for i, s in zip(xi, sev)]
                for lam in (None, 0.3):
                    out.append(make_case(family, f'C {C} severity {sev.dtype} lam {lam}', C, sev, dict(ord=ordinal_head(xi, C - 1)), names, lam=lam))
    elif family == 'uncertainty':
        for C in CS:
            idx = np.arange(len(LOG_VARS) * len(RESIDUALS))
            sev = np.ones(len(idx), dtype=np.int64)
            mu, lv = uncertainty_head(sev, idx)
            names = [f'log_var {LOG_VARS[i // 9]:g} y-mu {RESIDUALS[i % 9]:g}' for i in idx]
            for lam in (None, 0.3):
                out.append(make_case(family, f'C {C} lam {lam}', C, sev, dict(mu=mu, lv=lv), names, lam=lam))
    elif family == 'kan':
        for C in CS:
            ys = np.asarray(sorted({0, 1, C - 1}), dtype=np.int64)
            sev = np.repeat(ys, len(KAN_KINDS))
            idx = np.arange(len(sev))
            names = [f'y {y} prediction {KAN_KINDS[i % 6]}' for y, i in zip(sev, idx)]
            for lam in (None, 0.3):
                out.append(make_case(family, f'C {C} lam {lam}', C, sev, dict(kan=kan_head(sev, idx)), names, lam=lam))
    elif family == 'batch':
        C = 4
        p = focal_pool(C)
        for B in BATCH_SIZES:
            i = np.arange(B)
            sev = (i % C).astype(np.int64)
            f = i % len(p.ta)
            mu, lv = uncertainty_head(sev, i)
            rows = dict(cls=p.cls[f], ta=p.ta[f], tb=p.tb[f], ord=ordinal_head(i, C - 1), mu=mu, lv=lv, kan=kan_head(sev, i))
            names = [f'row {k}: {p.names[j]}' for k, j in zip(i, f)]
            for stage in (1, 2, 3, 4):
                for lam in (None, 0.3):
                    out.append(make_case(family, f'B {B} stage {stage} lam {lam}', C, sev, rows, names, lam=lam, stage=stage, off=p.off[f], gap=p.gap[f]))
    else:
        raise KeyError(family)
    return out


def switch_cases():
    """Rows on either side of the point where joint_loss::softmax_shift changes form: the offset-0 rows of the focal family moved so that
    their largest logit is the last fp32 below 4, 4, -4 and the first fp32 above -4."""
    out = []
    edges = (float(np.nextafter(F32(4.0), F32(0.0))), 4.0, -4.0, float(np.nextafter(F32(-4.0), F32(0.0))))
    for C in CS:
        p = focal_pool(C)
        keep = np.nonzero(p.off == 0.0)[0]
        base = p.cls[keep].astype(np.float64)
        base = base - base.max(axis=1, keepdims=True)
        cls = np.concatenate([base + e for e in edges]).astype(F32)
        idx = np.tile(keep, len(edges))
        names = [f'zmax {e!r}: {p.names[k]}' for e in edges for k in keep]
        sev = (np.arange(len(idx)) % C).astype(np.int64)
        for gamma in (0.5, 2.0):
            for lam in (None, 0.3):
                out.append(make_case('switch', f'C {C} gamma {gamma:g} lam {lam}', C, sev, dict(cls=cls, ta=p.ta[idx], tb=p.tb[idx]), names, gamma, True, lam,
                                     off=np.repeat(edges, len(keep)), gap=p.gap[idx]))
    return out


_CASES = {}


def cases(family):
    """family_cases(family), built once; the closed-form reference of a case is computed once too (reference())."""
    if family not in _CASES:
        _CASES[family] = switch_cases() if family == 'switch' else family_cases(family)
    return _CASES[family]


def head_arrays(case):
    """The five head outputs in HEADS order."""
    return {'cls_logits': case.cls, 'ordinal_logits': case.ord, 'mu': case.mu, 'log_var': case.lv, 'kan_severity': case.kan}


def torch_case(case, device='cpu', dtype=torch.float32):
    """-> (head outputs as tensors of ``dtype``, labels a, labels b, severities, alpha or None) on ``device``."""
    out = {k: torch.from_numpy(v).to(device=device, dtype=dtype) for k, v in head_arrays(case).items()}
    alpha = None if case.alpha is None else torch.from_numpy(case.alpha).to(device)
    return out, torch.from_numpy(case.ta).to(device), torch.from_numpy(case.tb).to(device), torch.from_numpy(case.sev).to(device), alpha


# ---- closed-form fp64 reference ------------------------------------------------------------------------------------------------------------

def _focal_fp64(z, t, gamma, alpha):
    """One label column -> (per-row loss, per-row gradient (B, C) of it), finite wherever the logits are.  1 - p_t is the sum of the other
    classes' probabilities, never a subtraction, and log p_t is -log1p(that sum's numerator) where the target holds the maximum: the
    autograd form (1 - p_t)^gamma * CE gives 0 * inf for gamma < 1 once p_t rounds to 1, which fp64 does from a gap of about 37.
        d/dz_j = alpha_t [gamma om^(gamma-1) p_t log p_t - om^gamma] (delta_jt - p_j),   om = 1 - p_t,
    the first term absent at gamma = 0, and delta_tt - p_t = om."""
    B, C = z.shape
    r = np.arange(B)
    m = z.max(axis=1)
    e = np.exp(z - m[:, None])
    S = e.sum(axis=1)
    p = e / S[:, None]
    hot = np.zeros((B, C))
    hot[r, t] = 1.0
    rest = (e * (1.0 - hot)).sum(axis=1)
    om = rest / S
    et = e[r, t]
    with np.errstate(divide='ignore'):
        logpt = np.where(et == 1.0, -np.log1p(rest), (z[r, t] - m) - np.log(S))
    pt = et / S
    fg = om ** gamma
    first = 0.0 if gamma == 0.0 else gamma * om ** (gamma - 1.0) * pt * logpt
    al = 1.0 if alpha is None else alpha.astype(np.float64)[t]
    d = hot - p
    d[r, t] = om
    return al * fg * (-logpt), (al * (first - fg))[:, None] * d


def reference(case):
    """-> (the five losses, the per-sample gradients G = B * d(total)/d(output) of the five heads), fp64, for an upstream gradient of 1.
    Heads that the stage leaves out have G = 0 and loss 0.  Cached on the case."""
    if getattr(case, '_ref', None) is not None:
        return case._ref
    f8 = lambda a: a.astype(np.float64)
    z, y = f8(case.cls), f8(case.sev).reshape(-1, 1)
    val, g = _focal_fp64(z, case.ta, case.gamma, case.alpha)
    if case.lam is not None:
        vb, gb = _focal_fp64(z, case.tb, case.gamma, case.alpha)
        val, g = case.lam * val + (1.0 - case.lam) * vb, case.lam * g + (1.0 - case.lam) * gb
    L = dict.fromkeys(LOSSES, 0.0)
    G = {k: np.zeros(v.shape) for k, v in head_arrays(case).items()}
    L['cls_loss'], G['cls_logits'] = math.fsum(val) / case.B, g
    total = L['cls_loss']
    if case.stage >= 2:
        x, K1 = f8(case.ord), case.C - 1
        yt = (y > np.arange(K1).reshape(1, -1)).astype(np.float64)
        ex = np.exp(-np.abs(x))
        bce = np.maximum(x, 0.0) - x * yt + np.log1p(ex)
        sig = np.where(x >= 0, 1.0 / (1.0 + ex), ex / (1.0 + ex))                    # sigmoid(x)
        nsig = np.where(x >= 0, ex / (1.0 + ex), 1.0 / (1.0 + ex))                   # sigmoid(-x) = 1 - sigmoid(x), without the subtraction
        L['ord_loss'] = math.fsum(bce.mean(axis=1)) / case.B
        G['ordinal_logits'] = LAMBDA_ORD / K1 * np.where(yt == 1.0, -nsig, sig)
        total += LAMBDA_ORD * L['ord_loss']
    if case.stage >= 3:
        r, s = y - f8(case.mu), f8(case.lv)
        prec = np.exp(-s)
        L['unc_loss'] = math.fsum((0.5 * (r * r * prec + s)).reshape(-1)) / case.B
        G['mu'], G['log_var'] = -MU_UNC * r * prec, MU_UNC * 0.5 * (1.0 - r * r * prec)
        total += MU_UNC * L['unc_loss']
    if case.stage >= 4:
        r = f8(case.kan) - y
        L['kan_loss'] = math.fsum((r * r).reshape(-1)) / case.B
        G['kan_severity'] = NU_KAN * 2.0 * r
        total += NU_KAN * L['kan_loss']
    L['total_loss'] = total
    case._ref = (L, G)
    return case._ref


# ---- comparator -----------------------------------------------------------------------------------------------------------------------------

def grad_ratios(G_got, G_ref):
    """Per head, per row: max_j |G_got - G_ref| / (1e-5 max(1, max_j |G_ref[row]|)).  A non-finite entry of G_got gives inf; a non-finite
    reference is an error of the test."""
    out = {}
    for k in HEADS:
        ref = np.asarray(G_ref[k], dtype=np.float64)
        assert np.isfinite(ref).all(), f'the reference of {k} is not finite'
        got = np.asarray(G_got[k], dtype=np.float64).reshape(ref.shape)
        err = np.abs(got - ref).max(axis=1)
        bound = GRAD_TOL * np.maximum(1.0, np.abs(ref).max(axis=1))
        out[k] = np.where(np.isfinite(got).all(axis=1), err / bound, np.inf)
    return out


def loss_ratios(L_got, L_ref):
    """Per loss: |v - v_ref| / (1e-5 max(1, |v_ref|)).  At most 513 fp32 terms, each good to a few 1e-6 of its size, are added three to a
    thread and then in a fixed tree: under 4e-6 of the sum in all."""
    out = {}
    for k in LOSSES:
        ref, got = float(L_ref[k]), float(L_got[k])
        assert math.isfinite(ref), f'the reference of {k} is not finite'
        out[k] = abs(got - ref) / (LOSS_TOL * max(1.0, abs(ref))) if math.isfinite(got) else math.inf
    return out


def compare(case, L_got, G_got, upstream=1.0, what=''):
    """Asserts every row of every head and every loss of one launch against the closed form; the message names (family, row, head).
    ``G_got`` is the per-sample gradient B * grad.  -> (worst gradient ratio, worst loss ratio) in units of the bounds."""
    L_ref, G_ref = reference(case)
    gr = grad_ratios(G_got, {k: upstream * v for k, v in G_ref.items()})
    worst_g = 0.0
    for k in HEADS:
        i = int(np.argmax(gr[k]))
        worst_g = max(worst_g, float(gr[k][i]))
        assert gr[k][i] <= 1.0, (f'{what} family {case.family} [{case.name}] row {i} ({case.names[i]}) head {k}: {gr[k][i]:.3g} bounds; '
                                 f'got {np.asarray(G_got[k]).reshape(case.B, -1)[i]}, want {upstream * G_ref[k][i]}')
    worst_l = 0.0
    if L_got is not None:
        lr = loss_ratios(L_got, L_ref)
        for k in LOSSES:
            worst_l = max(worst_l, lr[k])
            assert lr[k] <= 1.0, f'{what} family {case.family} [{case.name}] {k}: {lr[k]:.3g} bounds; got {float(L_got[k])!r}, want {L_ref[k]!r}'
    return worst_g, worst_l


def failing_rows(case, G_got):
    """The rows of a launch with any head above its bound (sorted indices)."""
    gr = grad_ratios(G_got, reference(case)[1])
    return np.nonzero(np.max(np.stack([gr[k] for k in HEADS]), axis=0) > 1.0)[0]


def per_sample(grads, case, scale=None):
    """Gradient tensors or arrays (None for a head the stage leaves out) -> {head: B * grad as fp64 numpy}."""
    out = {}
    for k, ref in head_arrays(case).items():
        g = grads[k] if isinstance(grads, dict) else grads[HEADS.index(k)]
        if g is None:
            out[k] = np.zeros(ref.shape)
        else:
            g = g.detach().cpu().double().numpy() if isinstance(g, torch.Tensor) else np.asarray(g, dtype=np.float64)
            out[k] = case.B * g.reshape(ref.shape)
    return out


# ---- fp32 emulation of joint_loss::row and joint_loss::reduce ---------------------------------------------------------------------------------

def _block_sum(vals, B):
    """joint_loss_kernel's sum of per-row values: thread b % 256 adds its rows in order, then the 64 lanes of a wave in a butterfly tree, then
    the four waves in order."""
    acc = np.zeros(256, F32)
    for s in range(0, B, 256):
        chunk = vals[s:s + 256]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    v = acc.reshape(4, 64)
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    v = v.reshape(4)
    return ((v[0] + v[1]) + v[2]) + v[3]


def emulate(case, form):
    """joint_loss::row in numpy float32, operation by operation (libm exp / log / pow in place of the device's), with the log-softmax as
    'lse':       lse = zmax + log(se), log p_j = z_j - lse            the sum is rounded at the size of zmax: every log-probability of the
                                                                      row carries up to ulp(zmax) / 2, and a common shift changes the result
    'reordered': log p_j = (z_j - zmax) - log(se)                     the shift leaves with the first, exact-to-an-ulp subtraction
    'kernel':    'lse' in the rows with |zmax| < DIRECT_BELOW,        joint_loss::softmax_shift: the sum is rounded by at most 2^-22 there, and
                 'reordered' in the others                            the kernel keeps the operations it has always had for such rows
    -> (five losses, per-sample gradients)."""
    assert form in ('lse', 'reordered', 'kernel')
    B, C, K1 = case.B, case.C, case.C - 1
    r = np.arange(B)
    one, zero = F32(1.0), F32(0.0)
    invB = one / F32(B)
    gamma = F32(case.gamma)
    with np.errstate(all='ignore'):
        z = case.cls
        zmax = z.max(axis=1)
        se = np.zeros(B, F32)
        for j in range(C):
            se = se + np.exp(z[:, j] - zmax)
        direct = {'lse': np.ones(B, bool), 'reordered': np.zeros(B, bool), 'kernel': np.abs(zmax) < F32(DIRECT_BELOW)}[form]
        lgse = np.log(se)
        shift, rest = np.where(direct, zmax + lgse, zmax), np.where(direct, zero, lgse)
        logp = (z - shift[:, None]) - rest[:, None]
        p = np.exp(logp)
        hot = lambda t: (np.arange(C).reshape(1, -1) == t.reshape(-1, 1)).astype(F32)

        def focal(t):
            logpt, pt = logp[r, t], p[r, t]
            al = one if case.alpha is None else case.alpha[t]
            om = one - pt
            fg = np.power(np.maximum(om, zero), gamma)
            fgm1 = np.zeros(B, F32) if case.gamma == 0.0 else gamma * np.power(np.maximum(om, F32(1e-30)), gamma - one)
            return al * fg * (-logpt), al * (fgm1 * pt * logpt - fg) * invB
        val, coef = focal(case.ta)
        if case.lam is None:
            d_cls = coef[:, None] * (hot(case.ta) - p)
        else:
            vb, cb = focal(case.tb)
            lam = F32(case.lam)
            oml = one - lam
            val = lam * val + oml * vb
            d_cls = lam * (coef[:, None] * (hot(case.ta) - p)) + oml * (cb[:, None] * (hot(case.tb) - p))
        y = case.sev.astype(F32)
        grads = {'cls_logits': d_cls, 'ordinal_logits': None, 'mu': None, 'log_var': None, 'kan_severity': None}
        s_cls = _block_sum(val, B) * invB
        s_ord = s_unc = s_kan = zero
        total = s_cls
        if case.stage >= 2:
            w = F32(LAMBDA_ORD) * invB / F32(K1)
            acc = np.zeros(B, F32)
            d_ord = np.empty((B, K1), F32)
            for k in range(K1):
                x = case.ord[:, k]
                yt = (y > F32(k)).astype(F32)
                acc = acc + (np.maximum(x, zero) - x * yt + np.log(one + np.exp(-np.abs(x))))
                d_ord[:, k] = w * (one / (one + np.exp(-x)) - yt)
            grads['ordinal_logits'] = d_ord
            s_ord = _block_sum(acc / F32(K1), B) * invB
            total = total + F32(LAMBDA_ORD) * s_ord
        if case.stage >= 3:
            m, s = case.mu[:, 0], case.lv[:, 0]
            prec, res = np.exp(-s), y - m
            s_unc = _block_sum(F32(0.5) * (res * res * prec + s), B) * invB
            grads['mu'] = (-F32(MU_UNC) * invB * res * prec).reshape(B, 1)
            grads['log_var'] = (F32(MU_UNC) * invB * F32(0.5) * (one - res * res * prec)).reshape(B, 1)
            total = total + F32(MU_UNC) * s_unc
        if case.stage >= 4:
            res = case.kan[:, 0] - y
            s_kan = _block_sum(res * res, B) * invB
            grads['kan_severity'] = (F32(NU_KAN) * invB * F32(2.0) * res).reshape(B, 1)
            total = total + F32(NU_KAN) * s_kan
    return dict(zip(LOSSES, (s_cls, s_ord, s_unc, s_kan, total))), per_sample(grads, case)
