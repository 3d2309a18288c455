"""Cases, fp64 truth, error bounds and an fp32 restatement for the optimizer kernels of csrc/optim.hip: rovit_sq_norm_clip, rovit_sq_norm_accum,
rovit_clip_coef, rovit_adamw_flat, rovit_adamw_flat_multi and rovit_adamw_ema_flat_multi.  CPU only: numpy, no kernel code.
tests/test_optim_cases_cpu.py checks this module, tests/test_gpu_optim_rows.py and tools/optim_rows_error.py use it against the exported entries.

THE TRUTH R (fp64), torch's semantics with the hyperparameters rounded to fp32 first, as the kernels receive them:
    norm = sqrt(sum g^2) over all buffers          coef = min(1, max_norm / (norm + 1e-6))     (NaN norm -> NaN coef: torch clamps)
    gr = g coef     m' = b1 m + (1 - b1) gr     v' = b2 v + (1 - b2) gr^2
    p' = p (1 - lr wd) - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)       e' = rovit_hip.optim.ema_reference(e, p', decay)
AdamW is judged on a GIVEN coefficient (the fp32 value the kernel reads); the norm and the coefficient are judged in cases of their own.
fp32's range is part of the semantics: a sum of squares or a second moment beyond FLT_MAX is +inf (no case sits within a factor 2 of it).

THE BOUNDS, per element, from fp64 quantities only (never from a GPU result).  u = 2^-24; every rounding is at most u of its result.
  m'     A = b1 m, B = (1 - b1) gr.  gr, fl(1 - b1) and their product: 3u B; b1 m where it is not fused: u A; the sum: u |m'| <= u (|A| + |B|).
         em = 4u (|A| + |B|): it does not shrink with m' where A and B cancel.
  v'     C = b2 v, D = (1 - b2) gr^2 (both >= 0).  gr twice, fl(1 - b2), two products: 5u D; b2 v: u C; the sum: u (C + D).  ev = 6u (C + D).
  p'     s = sqrt(v'): es = min(ev / s, sqrt(ev)) + u s (the propagated ev, then sqrtf's rounding).  denom = s / sqrt(bc2) + eps:
         ed = es / sqrt(bc2) + 3u denom (the fp32 1 / sqrt(bc2), the product where it is not fused, the sum).  q = m' / denom:
         eq = (em + |q| ed) / (denom - ed) + u |q|.  upd = step q, step = fl(lr fl(1 / bc1)): eu = step eq + 3u |upd|.  decay = fl(1 - lr wd): 2u.
         p' = decay p - upd, fused or not: ep = 4u (|p| + |upd|) + eu.
  e'     e + omd (p' - e): omd (ep + u (|p'| + |e|)) + u |e'|.
  TINY = 2^-124 is added to every bound: a result below the smallest normal may be flushed or rounded as a subnormal.
  squared norm   every term is >= 0, so the relative error is at most gamma(d) = d u / (1 - d u), d the longest chain of roundings a term
         passes through: clip_depth / accum_depth count it from the kernels' loops and state it per case.  Exact cases have bound 0.
  norm   norm (gamma / (2 (1 - gamma)) + u): half the squared norm's, and sqrtf's rounding.
  coef   c = max_norm / (norm + 1e-6): the sum's rounding u (norm + 1e-6) on top of the norm's, then c (e_den / (den - e_den) + u); min(., 1) is
         1-Lipschitz, and where c - ec >= 1 the coefficient must be exactly 1.
REQUIRED OUTCOMES that no tolerance decides have bound 0: g coef = 0 with m = v = 0 leaves m' = v' = 0 and p' = fl(fl(decay) p); a second moment
that overflows is +inf and p' = fl(fl(decay) p) (the update term m' / inf is 0); norm 0 -> coef 1; an overflowing sum -> norm +inf, coef 0;
a NaN gradient -> norm NaN, coef NaN.
SAFETY = 2 multiplies every derived bound, once, in `ratio`.  It is not fitted to any GPU result: it pays for what the derivations leave
out at second order (products of two u terms, the fp64 rounding of R itself)."""
import math
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
SAFETY = 2.0
TINY = 2.0 ** -124
FLT_MAX = float(np.finfo(np.float32).max)
f32, f64 = np.float32, np.float64

# restated from csrc/optim.hip; tests/test_optim_cases_cpu.py reads them out of the source so the two cannot drift apart
ADAM_PIECE4 = 512               # float4 per block of the multi-segment AdamW kernels
ADAM_THREADS = 256
FLAT_MAX_BLOCKS = 2048          # rovit_adamw_flat: grid stride above this many 256-thread blocks
NORM_PIECE4 = 4096              # float4 per piece of rovit_sq_norm_clip
NORM_THREADS = 1024
NORM_MAX_BLOCKS = 256
ACCUM_MAX_BLOCKS = 512          # rovit_sq_norm_accum: grid stride above this many 256-thread blocks
ACCUM_THREADS = 256
NORM_PIECE = NORM_PIECE4 * 4    # floats
ADAM_PIECE = ADAM_PIECE4 * 4


def gamma(d):
    return d * U / (1.0 - d * U)


def arr32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=f32))


def ratio(got, want, bound):
    """Elementwise |got - want| / (SAFETY bound); 0 where both agree exactly (inf == inf, NaN with NaN), inf where a bound-0 element differs."""
    got, want, bound = (np.atleast_1d(np.asarray(x, dtype=f64)) for x in (got, want, bound))
    with np.errstate(all='ignore'):
        same = (got == want) | (np.isnan(got) & np.isnan(want))
        r = np.abs(got - want) / (SAFETY * bound)
    r = np.where(same, 0.0, r)
    return np.where(np.isnan(r), np.inf, r)


def worst(rec, key, r, where):
    """Keep the largest ratio per tensor in rec: {tensor: (ratio, where)}; `where` is a function of the flat index."""
    i = int(np.argmax(r))
    if key not in rec or not float(r[i]) <= rec[key][0]:
        rec[key] = (float(r[i]), where(i))


# =====================================================================================================================================
# the norm kernels
# =====================================================================================================================================
def clip_layout(counts):
    """rovit_sq_norm_clip's walk: (first piece of every buffer + [total], total pieces P, grid, [(p0, p1) per block])."""
    first, P = [], 0
    for c in counts:
        first.append(P)
        P += (c // 4 + NORM_PIECE4 - 1) // NORM_PIECE4
    grid = min(P, NORM_MAX_BLOCKS)
    return first + [P], P, grid, [(b * P // grid, (b + 1) * P // grid) for b in range(grid)]


def piece_span(counts, pc):
    """(buffer, first float, one past the last float) of piece pc, clipped to the buffer's count."""
    first = clip_layout(counts)[0]
    k = max(q for q in range(len(counts)) if pc >= first[q] and counts[q] > 0 and pc < first[q + 1])
    lo = (pc - first[k]) * NORM_PIECE
    return k, lo, min(lo + NORM_PIECE, counts[k])


def clip_depth(counts):
    """Longest chain of roundings a term of rovit_sq_norm_clip's sum passes through: the square (1), the float4 pair sums (2), four adds a
    piece onto the thread's accumulator, the wave butterfly (6), the 16 wave partials in order (16), then the last block: its first add
    (1), the butterfly (6) and the 16 partials again."""
    ppb = max(p1 - p0 for p0, p1 in clip_layout(counts)[3])
    return 1 + 2 + 4 * ppb + 6 + 16 + 1 + 6 + 16


def accum_layout(n):
    n4 = n // 4
    blocks = min(max((n4 + ACCUM_THREADS - 1) // ACCUM_THREADS, 1), ACCUM_MAX_BLOCKS)
    stride = blocks * ACCUM_THREADS
    return n4, blocks, (n4 + stride - 1) // stride


def accum_depth(n, scratch):
    """rovit_sq_norm_accum: the square (1), the float4 chain (3), one add per grid-stride trip, the tail's add (1), the butterfly (6), the four
    wave partials (3); with scratch the last block's two adds a thread, butterfly, partials and the add onto *out_sq (2 + 6 + 3 + 1),
    without it one atomic add per block, in any order."""
    _, blocks, trips = accum_layout(n)
    return 1 + 3 + trips + 1 + 6 + 3 + (12 if scratch else blocks)


def _butterfly(v):
    """wave_sum64 on the last axis (64 lanes): every lane ends with the same sum; lane 0 is returned."""
    lanes = np.arange(64)
    for s in (1, 2, 4, 8, 16, 32):
        v = v + v[..., lanes ^ s]
    return v[..., 0]


def _serial(s):
    t = np.zeros(s.shape[:-1], dtype=f32)
    for w in range(s.shape[-1]):
        t = t + s[..., w]
    return t


def clip_coefficient32(norm, max_norm):
    """The kernels' coefficient in fp32 (clip_coefficient of optim.hip)."""
    with np.errstate(all='ignore'):
        return f32(norm) if np.isnan(norm) else np.minimum(f32(1), f32(max_norm) / (f32(norm) + f32(1e-6)))


def emulate_clip(bufs, max_norm):
    """sq_norm_clip_kernel in numpy fp32, in its own order -> (squared norm, norm, coef), all fp32."""
    counts = [b.size for b in bufs]
    first, P, grid, blocks = clip_layout(counts)
    with np.errstate(all='ignore'):
        S = []
        for k, b in enumerate(bufs):
            np_ = first[k + 1] - first[k]
            if np_ == 0:
                continue
            pad = np.zeros(np_ * NORM_PIECE, dtype=f32)
            pad[:b.size] = b
            sq = pad.reshape(np_, 4, NORM_THREADS, 4)
            sq = sq * sq
            S.append((sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3]))
        S = np.concatenate(S)                                          # (P, 4, 1024): piece, load, thread
        p0 = np.array([b[0] for b in blocks])
        cnt = np.array([b[1] - b[0] for b in blocks])
        acc = np.zeros((grid, NORM_THREADS), dtype=f32)
        for j in range(int(cnt.max())):
            on = cnt > j
            for u in range(4):
                acc[on] = acc[on] + S[p0[on] + j, u]
        part = _serial(_butterfly(acc.reshape(grid, NORM_THREADS // 64, 64)))
        t = np.zeros(NORM_THREADS, dtype=f32)
        t[:grid] = t[:grid] + part
        sq = _serial(_butterfly(t.reshape(NORM_THREADS // 64, 64)))
        norm = np.sqrt(f32(sq))
        return f32(sq), f32(norm), f32(clip_coefficient32(norm, max_norm))


def emulate_accum(g, out, scratch):
    """sq_norm_kernel in numpy fp32 -> out + sum g^2 (fp32).  Without scratch the atomic adds are taken in block order."""
    n = g.size
    n4, blocks, trips = accum_layout(n)
    with np.errstate(all='ignore'):
        pad = np.zeros(max(trips, 1) * blocks * ACCUM_THREADS * 4, dtype=f32)
        pad[:n4 * 4] = g[:n4 * 4]
        sq = pad.reshape(max(trips, 1), blocks, ACCUM_THREADS, 4)
        sq = sq * sq
        acc = np.zeros((blocks, ACCUM_THREADS), dtype=f32)
        for it in range(trips):
            acc = acc + (((sq[it, ..., 0] + sq[it, ..., 1]) + sq[it, ..., 2]) + sq[it, ..., 3])
        tail = g[n4 * 4:]
        acc[0, :tail.size] = acc[0, :tail.size] + tail * tail
        s = _butterfly(acc.reshape(blocks, 4, 64))                     # (blocks, 4)
        out = f32(out)
        if not scratch:
            for b in range(blocks):
                out = out + (((s[b, 0] + s[b, 1]) + s[b, 2]) + s[b, 3])
            return f32(out)
        part = np.zeros(2 * ACCUM_THREADS, dtype=f32)
        part[:blocks] = (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
        t = (np.zeros(ACCUM_THREADS, dtype=f32) + part[:ACCUM_THREADS]) + part[ACCUM_THREADS:]
        w = _butterfly(t.reshape(4, 64))
        return f32(out + ((w[0] + w[1]) + (w[2] + w[3])))


def sq_truth(bufs):
    """fp64 sum of squares with fp32's range: beyond FLT_MAX it is +inf, a NaN stays a NaN."""
    with np.errstate(all='ignore'):
        sq = float(sum(np.sum(np.asarray(b, dtype=f64) ** 2) for b in bufs))
    if not math.isnan(sq):
        assert not FLT_MAX / 2 < sq <= 2 * FLT_MAX, 'a case within a factor 2 of the fp32 range decides nothing'
        if sq > FLT_MAX:
            sq = math.inf
    return sq


def coef_truth(sq, max_norm, rel_sq):
    """(norm, coef) and their bounds from a squared norm known to the relative error rel_sq (0: exactly)."""
    if math.isnan(sq):
        return (math.nan, 0.0), (math.nan, 0.0)
    if math.isinf(sq):
        return (math.inf, 0.0), (0.0, 0.0)
    norm = math.sqrt(sq)
    bnorm = norm * (rel_sq / (2 * (1 - rel_sq)) + U)
    den = norm + float(f32(1e-6))
    eden = bnorm + U * den
    c = float(f32(max_norm)) / den
    ec = c * (eden / (den - eden) + U)
    if c - SAFETY * ec >= 1.0:
        return (norm, bnorm), (1.0, 0.0)
    return (norm, bnorm), (min(1.0, c), ec)


ClipCase = namedtuple('ClipCase', 'name bufs max_norm exact probes classes')
# probes: [(buffer, float index, value, class)]: the elements an exact sparse case is sensitive to; classes: what the case is there for


def _dense(n, rng):
    return arr32(rng.choice([-1.0, 1.0], size=n))


def _sparse(counts, positions):
    """Zeros except 2^k at the k-th position: the squares 4^k occupy disjoint base-4 digits of the sum."""
    assert len(positions) <= 10, 'ten probes: beyond that a lost 1 hides behind the square root (see sensitivity)'
    bufs = [np.zeros(c, dtype=f32) for c in counts]
    probes = []
    for j, (k, i, cls) in enumerate(positions):
        assert bufs[k][i] == 0, 'two probes on one element'
        bufs[k][i] = 2.0 ** j
        probes.append((k, i, 2.0 ** j, cls))
    return bufs, probes


def block_edge_positions(counts, blocks):
    """First and last float4 (element 0 of the first, element 3 of the last) of the first and the last piece of each given block."""
    layout = clip_layout(counts)[3]
    pos = []
    for b in blocks:
        p0, p1 = layout[b]
        for which, pc in (('first', p0), ('last', p1 - 1)):
            k, lo, hi = piece_span(counts, pc)
            for i, end in ((lo, 'first4'), (hi - 1, 'last4')):
                if (k, i) not in [(a, c) for a, c, _ in pos]:
                    pos.append((k, i, f'{which}_piece_{end}'))
    return pos


PIECE_TOTALS = (1, 2, 255, 256, 257, 511, 513)
SINGLE_SIZES = (4, NORM_PIECE - 4, NORM_PIECE, NORM_PIECE + 4)


def clip_piece_cases():
    """Sparse probes at every total piece count: `ends` the first and the last block (whole last piece), `mid` the first block that has
    the most pieces and the first that has the fewest (last piece of the buffer half full)."""
    for P in PIECE_TOTALS:
        for variant in ('ends', 'mid'):
            n = P * NORM_PIECE if variant == 'ends' else P * NORM_PIECE - NORM_PIECE // 2
            layout = clip_layout([n])[3]
            cnt = [p1 - p0 for p0, p1 in layout]
            blocks = [0, len(layout) - 1] if variant == 'ends' else [cnt.index(max(cnt)), cnt.index(min(cnt))]
            blocks = list(dict.fromkeys(blocks))
            bufs, probes = _sparse([n], block_edge_positions([n], blocks)[:10])
            yield ClipCase(f'pieces{P}_{variant}', bufs, f32(1.0), True, probes, {f'pieces{P}'})


MULTI_COUNTS = ((NORM_PIECE + 4, 20000), (4, NORM_PIECE - 4, 2 * NORM_PIECE + 4), (NORM_PIECE + 8, 12, 40004, NORM_PIECE + 4))
ZERO_COUNTS = {'zero_first': (0, NORM_PIECE + 4, 20), 'zero_middle': (NORM_PIECE + 4, 0, 20), 'zero_last': (NORM_PIECE + 4, 20, 0)}


def clip_small_cases():
    rng = np.random.default_rng(5)
    for n in SINGLE_SIZES:
        yield ClipCase(f'single{n}_dense', [_dense(n, rng)], f32(1.0), True, [], {f'single{n}'})
        pos = [(0, 0, 'first'), (0, n - 1, 'last')] + ([(0, NORM_PIECE - 1, 'piece_end'), (0, NORM_PIECE, 'piece_start')] if n > NORM_PIECE else [])
        bufs, probes = _sparse([n], pos)
        yield ClipCase(f'single{n}_probes', bufs, f32(1.0), True, probes, {f'single{n}'})
    for counts in MULTI_COUNTS:
        k = len(counts)
        yield ClipCase(f'bufs{k}_dense', [_dense(c, rng) for c in counts], f32(100.0), True, [], {f'bufs{k}'})
        pos = [x for q in range(k - 1) for x in ((q, counts[q] - 1, 'buffer_last'), (q + 1, 0, 'buffer_first'))]
        pos = list(dict.fromkeys(pos)) + [(k - 1, counts[k - 1] - 1, 'buffer_last')]
        bufs, probes = _sparse(counts, [p for j, p in enumerate(pos) if p[:2] not in [q[:2] for q in pos[:j]]])
        yield ClipCase(f'bufs{k}_probes', bufs, f32(1.0), True, probes, {f'bufs{k}'})
    for name, counts in ZERO_COUNTS.items():
        yield ClipCase(f'{name}_dense', [_dense(c, rng) for c in counts], f32(50.0), True, [], {name})
        pos = [(q, i, 'buffer_edge') for q, c in enumerate(counts) if c for i in (0, c - 1)]
        bufs, probes = _sparse(counts, pos)
        yield ClipCase(f'{name}_probes', bufs, f32(1.0), True, probes, {name})


def clip_coef_cases():
    """The coefficient: norm exactly max_norm, one fp32 below and above it, 0, an overflowing sum, a NaN, and sums that are not exact."""
    five = [arr32([3, 4, 0, 0])]
    yield ClipCase('norm_equals_max', five, f32(5.0), True, [], {'norm_equals_max'})
    yield ClipCase('norm_just_above_max', five, np.nextafter(f32(5.0), f32(0)), True, [], {'norm_just_above_max'})
    yield ClipCase('norm_just_below_max', five, np.nextafter(f32(5.0), f32(9)), True, [], {'norm_just_below_max'})
    yield ClipCase('norm_far_below_max', five, f32(64.0), True, [], {'coef_one'})
    yield ClipCase('norm_zero', [np.zeros(NORM_PIECE + 4, dtype=f32), np.zeros(8, dtype=f32)], f32(1.0), True, [], {'norm_zero'})
    big = np.zeros(NORM_PIECE + 4, dtype=f32)
    big[[0, NORM_PIECE + 3]] = 2.0 ** 100
    yield ClipCase('sum_overflows', [big], f32(1.0), True, [], {'overflow'})
    for where in ('first', 'last'):
        x = [np.ones(NORM_PIECE + 4, dtype=f32), np.ones(8, dtype=f32)]
        x[0 if where == 'first' else 1][0 if where == 'first' else -1] = np.nan
        yield ClipCase(f'nan_{where}', x, f32(1.0), True, [], {'nan'})
    rng = np.random.default_rng(6)
    for name, counts, mx in (('random1', (NORM_PIECE + 4,), 1.0), ('random3', (50000, 4, 33000), 1.0), ('random300', (300 * NORM_PIECE - 8,), 1.0),
                             ('random_small_norm', (2 * NORM_PIECE,), 1.0)):
        scale = 1e-3 if name == 'random_small_norm' else 1.0
        yield ClipCase(name, [arr32(rng.standard_normal(c) * scale) for c in counts], f32(mx), False, [], {'random'})


def clip_cases():
    yield from clip_small_cases()
    yield from clip_coef_cases()
    yield from clip_piece_cases()


def clip_truth(case):
    """((norm, bound), (coef, bound), d)."""
    d = clip_depth([b.size for b in case.bufs])
    n, c = coef_truth(sq_truth(case.bufs), case.max_norm, 0.0 if case.exact else gamma(d))
    return n, c, d


def judge_clip(case, run, rec):
    """run(bufs, max_norm) -> (norm, coef) as fp32.  Adds the case's ratios to rec."""
    (norm, bnorm), (coef, bcoef), _ = clip_truth(case)
    g_norm, g_coef = run(case.bufs, case.max_norm)
    worst(rec, 'norm', ratio(g_norm, norm, bnorm), lambda i: case.name)
    worst(rec, 'coef', ratio(g_coef, coef, bcoef), lambda i: case.name)


def clip_sensitivity(case):
    """For an exact case: (the allowance of the norm, the smallest move of the expected norm when one probe / one element of a dense fill
    is dropped or counted twice).  The test requires move > 2 allowance: the allowance on either side of a wrong sum cannot reach R."""
    sq = sq_truth(case.bufs)
    norm = math.sqrt(sq)
    allowance = SAFETY * U * norm
    terms = [v * v for _, _, v, _ in case.probes] if case.probes else [1.0]
    move = min(min(abs(math.sqrt(sq + s * t) - norm) for s in (1, -1)) for t in terms)
    return allowance, move


AccumCase = namedtuple('AccumCase', 'name bufs exact')
ACCUM_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, ACCUM_MAX_BLOCKS * 1024 - 4, ACCUM_MAX_BLOCKS * 1024, ACCUM_MAX_BLOCKS * 1024 + 5)


def accum_cases():
    rng = np.random.default_rng(7)
    for n in ACCUM_SIZES:
        yield AccumCase(f'n{n}_dense', [_dense(n, rng)], True)
        # the first and the last element, the last float4's first element and the first tail element carry distinct base-4 digits
        pos = sorted({0, n - 1, max(n // 4 * 4 - 4, 0), min(n // 4 * 4, n - 1)})
        bufs, _ = _sparse([n], [(0, i, 'edge') for i in pos])
        yield AccumCase(f'n{n}_probes', bufs, True)
        yield AccumCase(f'n{n}_random', [arr32(rng.standard_normal(n))], False)
    three = (1025, 3, ACCUM_MAX_BLOCKS * 1024 + 5)
    yield AccumCase('three_buffers_dense', [_dense(n, rng) for n in three], True)
    yield AccumCase('three_buffers_random', [arr32(rng.standard_normal(n)) for n in three], False)


def accum_truth(case, scratch):
    """(squared norm, bound): buffer by buffer, each with its own depth and one more add onto the running *out_sq."""
    sqs = [sq_truth([b]) for b in case.bufs]
    if case.exact:
        return sum(sqs), 0.0
    return sum(sqs), sum(gamma(accum_depth(b.size, scratch) + len(case.bufs)) * s for b, s in zip(case.bufs, sqs))


def judge_accum(case, run, rec, scratch):
    """run(bufs, scratch) -> the accumulated squared norm (fp32).  Without scratch only exact cases are order-independent; the others get the
    bound that counts one atomic add per block."""
    sq, b = accum_truth(case, scratch)
    worst(rec, 'sq' if scratch else 'sq_atomic', ratio(run(case.bufs, scratch), sq, b), lambda i: case.name)


# =====================================================================================================================================
# AdamW
# =====================================================================================================================================
Hyper = namedtuple('Hyper', 'b1 b2 eps wd')
HYPER = Hyper(f32(0.9), f32(0.999), f32(1e-8), f32(1e-2))
HYPER_BACKBONE = Hyper(f32(0.9), f32(0.999), f32(1e-8), f32(1e-4))       # with lr 1e-5: lr wd = 1e-9 < 2^-24, decay rounds to 1
TS = (1, 2, 10, 1000000)
COEFS = (None, f32(1.0), f32(0.5), f32(0.0))
LRS = (f32(1e-3), f32(3e-4), f32(1e-2), f32(1e-5))
DECAYS = (0.5, 0.9, 0.999, 2.0 / 11.0)
RECIPES = ('body', 'zero_moments', 'zero_grad', 'cancel', 'denom_below_eps', 'denom_near_eps', 'denom_above_eps', 'gr_subnormal',
           'gr2_underflows', 'gr2_overflows', 'large_p')
K = len(RECIPES)


def decay32(lr, wd):
    """fl(1 - lr wd) as one fused operation; the CPU test checks that the two-rounding form gives the same value for every case."""
    return f32(1.0 - float(lr) * float(wd))


def host_corrections(hyper, t):
    """(inv_bc1, inv_sqrt_bc2) as the entry points compute them: in double, rounded to float."""
    bc1, bc2 = 1.0 - float(hyper.b1) ** t, 1.0 - float(hyper.b2) ** t
    return f32(1.0 / bc1), f32(1.0 / math.sqrt(bc2))


def lay_recipes(n, shift, rng, lr, t, coef, hyper):
    """p, g, m, v, e and the recipe index of every element: element i gets recipe (i + shift) mod K, so K shifts put every recipe on every
    position.  The recipes aim at the gradient after scaling, gr = g coef (coef 0 makes every gradient 0: that is its own case)."""
    c = 1.0 if coef is None or float(coef) == 0.0 else float(coef)
    b1, b2, eps = float(hyper.b1), float(hyper.b2), float(hyper.eps)
    bc2 = 1.0 - b2 ** t
    rec = (np.arange(n) + shift) % K
    p, g = rng.standard_normal(n), rng.standard_normal(n)
    m, v = 0.1 * rng.standard_normal(n), 1e-2 * rng.random(n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)

    def put(name, **kw):
        on = rec == RECIPES.index(name)
        for key, val in kw.items():
            a = {'p': p, 'g': g, 'm': m, 'v': v}[key]
            a[on] = val[on] if isinstance(val, np.ndarray) else val
    put('zero_moments', m=0.0, v=0.0)
    put('zero_grad', g=0.0, m=0.0, v=0.0)
    put('cancel', m=-(1.0 - b1) * (g.astype(f32).astype(f64) * c) / b1)
    put('denom_below_eps', g=1e-12 * sign / c, m=0.0, v=0.0)
    put('denom_near_eps', g=eps * math.sqrt(bc2) / math.sqrt(1.0 - b2) / c * sign * (0.5 + 1.5 * rng.random(n)), m=0.0, v=0.0)
    put('denom_above_eps', m=0.5 * sign, v=1.0)
    put('gr_subnormal', g=1e-40 * sign, m=0.0, v=0.0)
    put('gr2_underflows', g=1e-25 * sign, m=0.0, v=0.0)
    put('gr2_overflows', g=2.0 ** 75 * sign, m=0.0, v=0.0)
    put('large_p', p=1e4 * p, g=1e-6 * g, m=1e-7 * sign, v=1e-13)
    return {'p': arr32(p), 'g': arr32(g), 'm': arr32(m), 'v': arr32(v), 'e': arr32(rng.standard_normal(n)), 'recipe': rec}


def adam_truth(s, g, lr, t, decay, coef, hyper):
    """One AdamW step of one segment in fp64 from the fp32 state s = {p, m, v, e} -> (want, bound): dicts over p, m, v, e."""
    b1, b2, eps, wd = (f64(x) for x in hyper)
    lr = f64(f32(lr))
    p, m, v, e, g = (np.asarray(x, dtype=f64) for x in (s['p'], s['m'], s['v'], s['e'], g))
    c = 1.0 if coef is None else f64(f32(coef))
    with np.errstate(all='ignore'):
        gr = g * c
        A, B = b1 * m, (1.0 - b1) * gr
        m1, em = A + B, 4 * U * (np.abs(A) + np.abs(B)) + TINY
        Cc, D = b2 * v, (1.0 - b2) * gr * gr
        v1 = Cc + D
        assert not np.any((v1 > FLT_MAX / 2) & (v1 <= 2 * FLT_MAX)), 'a second moment within a factor 2 of the fp32 range decides nothing'
        over = v1 > FLT_MAX
        ev = np.where(over, 0.0, 6 * U * v1 + TINY)
        v1 = np.where(over, np.inf, v1)
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        sq = np.sqrt(np.where(over, 1.0, v1))
        es = np.minimum(np.where(sq > 0, ev / np.where(sq > 0, sq, 1.0), np.inf), np.sqrt(ev)) + U * sq
        isb2 = 1.0 / math.sqrt(bc2)
        denom = sq * isb2 + eps
        ed = es * isb2 + 3 * U * denom
        q = m1 / denom
        eq = (em + np.abs(q) * ed) / (denom - ed) + U * np.abs(q) + TINY
        step = lr / bc1
        upd, dec = step * q, 1.0 - lr * wd
        eu = step * eq + 3 * U * np.abs(upd)
        p1 = p * dec - upd
        ep = 4 * U * (np.abs(p) + np.abs(upd)) + eu + TINY
        # required outcomes: nothing to move the element, or a second moment beyond fp32 -> p' = fl(fl(decay) p), no tolerance
        still = (gr == 0) & (m == 0) & (v == 0)
        exact = still | over
        p_exact = (decay32(lr, wd) * np.asarray(s['p'], dtype=f32)).astype(f64)
        p1, ep = np.where(exact, p_exact, p1), np.where(exact, 0.0, ep)
        em, ev = np.where(still, 0.0, em), np.where(still, 0.0, ev)
        omd = f64(f32(1.0 - f64(f32(decay))))
        e1 = e + omd * (p1 - e)                                       # rovit_hip.optim.ema_reference, on R's own p'
        ee = omd * (ep + U * (np.abs(p1) + np.abs(e))) + U * np.abs(e1) + TINY
    return {'p': p1, 'm': m1, 'v': v1, 'e': e1}, {'p': ep, 'm': em, 'v': ev, 'e': ee}


def _fma32(a, b, c):
    """fmaf in numpy: the product of two fp32 is exact in fp64; the sum rounds to fp64 and then to fp32 (a double rounding that can move
    the last bit once in 2^29 times: inside every bound here, and the reason `emulate` is held to the bounds and not to the GPU's bits)."""
    return (np.asarray(a, dtype=f64) * np.asarray(b, dtype=f64) + np.asarray(c, dtype=f64)).astype(f32)


def adam_emulate(s, g, lr, t, decay, coef, hyper):
    """adamw_element and ema_element of optim.hip in numpy fp32 -> {p, m, v, e}."""
    b1, b2, eps, wd = hyper
    lr = f32(lr)
    gs = f32(1.0) if coef is None else f32(coef)
    inv_bc1, isb2 = host_corrections(hyper, t)
    with np.errstate(all='ignore'):
        dec, step = decay32(lr, wd), lr * inv_bc1
        gr = g * gs
        M = _fma32(b1, s['m'], (f32(1) - b1) * gr)
        V = _fma32(gr, (f32(1) - b2) * gr, b2 * s['v'])
        denom = _fma32(np.sqrt(V), isb2, eps)
        P = _fma32(dec, s['p'], -(step * (M / denom)))
        omd = f32(1.0 - f64(f32(decay)))
        E = _fma32(omd, P - s['e'], s['e'])
    return {'p': P, 'm': M, 'v': V, 'e': E}


AdamCase = namedtuple('AdamCase', 'name segs coef hyper steps')
# segs: [{p, g, m, v, e, recipe, lr, t, decay}]; steps: None, or [(gradients per segment, coef)] of a run that continues from its own state


def _seg(n, shift, rng, lr, t, decay, coef, hyper):
    s = lay_recipes(n, shift, rng, lr, t, coef, hyper)
    s.update(lr=f32(lr), t=int(t), decay=decay)
    return s


SINGLE_N = (1, 3, 4, 5, ADAM_PIECE - 4, ADAM_PIECE - 1, ADAM_PIECE, ADAM_PIECE + 1, ADAM_PIECE + 4, 2 * ADAM_PIECE + 3)
FLAT_LARGE_N = FLAT_MAX_BLOCKS * 1024 + 4 * 1024 + 3
MULTI_SIZES = ((2 * ADAM_PIECE + 3, 5), (ADAM_PIECE + 1, ADAM_PIECE - 1, 3), (ADAM_PIECE + 4, 1, 2 * ADAM_PIECE + 3), (5, ADAM_PIECE, 4, ADAM_PIECE - 4),
               (3, 2 * ADAM_PIECE + 3, 1, ADAM_PIECE + 1), (ADAM_PIECE, 0, 7), (0, 9, ADAM_PIECE + 1, 0))


def adam_single_cases(n):
    """One segment of n floats, K shifts: every recipe on every position; t and coef cycle so that each size sees each of them."""
    rng = np.random.default_rng(1000 + n)
    backbone = n in (5, ADAM_PIECE + 1)
    for shift in range(K):
        t, coef = TS[shift % 4], COEFS[(shift + shift // 4) % 4]
        hyper, lr = (HYPER_BACKBONE, LRS[3]) if backbone and shift % 2 else (HYPER, LRS[shift % 3])
        yield AdamCase(f'n{n}_shift{shift}_t{t}_coef{coef}', [_seg(n, shift, rng, lr, t, DECAYS[shift % 4], coef, hyper)], coef, hyper, None)


def adam_product_cases():
    """Every t with every coef, at a size with two whole pieces and a tail."""
    n = 2 * ADAM_PIECE + 3
    rng = np.random.default_rng(77)
    for i, (t, coef) in enumerate((t, c) for t in TS for c in COEFS):
        yield AdamCase(f'product_t{t}_coef{coef}', [_seg(n, i % K, rng, LRS[0], t, 0.9, coef, HYPER)], coef, HYPER, None)


def adam_multi_cases(sizes):
    rng = np.random.default_rng(2000 + sum(sizes) + len(sizes))
    for shift in range(K):
        coef = COEFS[shift % 4]
        hyper = HYPER_BACKBONE if shift == 5 else HYPER
        segs = [_seg(n, shift + 3 * k, rng, LRS[(k + shift) % 4], TS[(k + shift) % 4], DECAYS[k], coef, hyper) for k, n in enumerate(sizes)]
        yield AdamCase(f'sizes{"_".join(map(str, sizes))}_shift{shift}_coef{coef}', segs, coef, hyper, None)


def adam_flat_large_cases(shifts=range(K)):
    """rovit_adamw_flat above its block cap: one grid-stride trip more for the first 1 024 float4, and a tail of 3."""
    for shift in shifts:
        rng = np.random.default_rng(3000 + shift)
        t, coef = TS[shift % 4], COEFS[(shift + 1) % 4]
        yield AdamCase(f'flat_large_shift{shift}_t{t}_coef{coef}', [_seg(FLAT_LARGE_N, shift, rng, LRS[0], t, 0.9, coef, HYPER)], coef, HYPER, None)


STEP_COEFS = (f32(1.0), f32(0.5), f32(0.25), f32(0.125), f32(0.9), f32(0.1), None, f32(0.7))


def adam_steps_case():
    """Eight steps from non-trivial moments, a fresh gradient and another coefficient every step; t counts on per segment."""
    rng = np.random.default_rng(4000)
    sizes, t0 = (ADAM_PIECE + 7, 5), (1, 5)
    segs = [_seg(n, k, rng, LRS[k], t0[k], DECAYS[k + 1], STEP_COEFS[0], HYPER) for k, n in enumerate(sizes)]
    for s in segs:                                                    # no overflow here: the run is about the scale of ordinary elements
        s['g'][np.abs(s['g']) > 1e10] = 1.0
    steps = [([arr32(rng.standard_normal(n)) if j else s['g'] for n, s in zip(sizes, segs)], c) for j, c in enumerate(STEP_COEFS)]
    return AdamCase('eight_steps', segs, STEP_COEFS[0], HYPER, steps)


def adam_classes(n, entry):
    """Position class of every element for an entry point ('flat', 'multi', 'ema'): what the kernels' index arithmetic distinguishes."""
    i = np.arange(n)
    i4, n4 = i // 4, n // 4
    cls = np.full(n, 'body', dtype=object)
    if entry == 'flat':
        stride = min(max((n4 + 255) // 256, 1), FLAT_MAX_BLOCKS) * 256
        cls[i4 >= stride] = 'second_trip'
        cls[i4 == stride - 1] = 'last4_of_first_trip'
        cls[i4 == stride] = 'first4_of_second_trip'
    else:
        cls[(i4 % ADAM_PIECE4 == ADAM_PIECE4 - 1)] = 'last4_of_piece'
        cls[(i4 % ADAM_PIECE4 == 0) & (i4 > 0)] = 'first4_of_next_piece'
    cls[i >= n4 * 4] = 'tail'
    return cls


def judge_adam(case, run, rec, ema):
    """run(segs, gs, ts, coef, hyper, ema) -> the new [{p, m, v, e}] (fp32) after one call from the state in segs with gradients gs.
    Every step is judged alone: R continues from the state `run` itself returned.  Adds the worst ratios to rec."""
    state = [{k: s[k] for k in 'pmve'} for s in case.segs]
    steps = case.steps or [([s['g'] for s in case.segs], case.coef)]
    for j, (gs, coef) in enumerate(steps):
        ts = [s['t'] + j for s in case.segs]
        new = run([dict(s, **st) for s, st in zip(case.segs, state)], gs, ts, coef, case.hyper, ema)
        for k, (s, st, nw) in enumerate(zip(case.segs, state, new)):
            if s['p'].size == 0:
                continue
            want, bound = adam_truth(st, gs[k], s['lr'], ts[k], s['decay'], coef, case.hyper)
            for x in ('pmve' if ema else 'pmv'):
                worst(rec, x, ratio(nw[x], want[x], bound[x]),
                      lambda i, k=k, s=s, j=j: f'{case.name} step {j} seg {k} elem {i} ({RECIPES[s["recipe"][i]]})')
        state = [{k: nw[k] if k in nw else st[k] for k in 'pmve'} for st, nw in zip(state, new)]
    return state


def emulate_run(segs, gs, ts, coef, hyper, ema):
    return [adam_emulate(s, g, s['lr'], t, s['decay'], coef, hyper) for s, g, t in zip(segs, gs, ts)]
