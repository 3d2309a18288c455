"""Shared by tests/test_attention_cases_cpu.py, tests/test_gpu_attention_rows.py and tools/attention_rows_error.py (no test in here): the
inputs, the fp64 references, the per-element bounds and the comparators of the attention kernels of csrc/attention.hip, per (image, head).

A `result` is what the kernels leave (or what stand_in() makes on the CPU): a dict of fp64 CPU tensors
    out (B,H,T,64), lse2 (B,H,T), dq, dk, dv (B,H,T,64)
Two references, both fp64:
  R  truth(): softmax(scale Q K^T) V, lse2 = log2 sum exp(scale q.k), and the closed forms dP = dO V^T, delta = rowsum(dO o O),
     dS = P o (dP - delta), dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO.  Nothing is rounded.
  E  the emulation: the same with the kernels' roundings, read from attention.hip:
       attn_fwd_kernel      m = the row maximum of the raw scores, p = exp2(fma(s, c2, -m c2)) in fp32 with c2 = scale log2 e; l = the fp32 sum
                            of the UNROUNDED p; bf16(p), unnormalised, is the operand of the P V product; out = bf16(sum / l);
                            lse2 = m c2 + log2 l in fp32
       attn_bwd_kernel      item A4 of backward_rows.py (attention_bwd_heads, imported): delta from the stored bf16 out, P / 8 and dS / 8
                            rounded to bf16 as the operands of the dV, dK and dQ products
       attn_cls_*_kernel    the class token's query alone; P and dS stay fp32 (attention_cls_bwd_heads, imported)

The bounds are per element and are sums of the terms those rounding points give, in the constants of backward_rows.py (HALF_ULP = ULP / 2, U32, FLOOR);
no factor in them was fitted to what a kernel returns.  With T keys, a = sum_d |q_d| |k_d| and smax = max_j |s_ij|:
  eta     the relative error of an fp32 probability of row i: ln 2 times the error of its exponent -- (64 + 4) roundings of the score sum
          ((64 + 4) U32 a c2), the roundings of c2, of m c2 and of the fma (4 U32 c2 smax) -- plus 2 U32 for exp2 itself
  acc     (T + 2) U32: an fp32 sum of T terms (the MFMA accumulation of a product over the keys or the queries, or l)
  out     with A = sum_j P_j |v_jd|:  (HALF_ULP + eta + acc) A from the numerator (the rounding of P, its fp32 error, the accumulation),
          (eta + acc + U32) A from l and the division; everything times (1 + 2^-6) for the second-order terms (every relative error here is
          below 2^-7); then HALF_ULP (|R| + that) for the output's own rounding
  lse2    log2 e (eta + acc) (1 + 2^-6) from l, 2 U32 (log2 T + 1) for log2f, U32 |lse2| for the last sum
  the backward reads the kernel's own out and lse2, so their bounds enter: delta errs by sum_d |dO_d| bound(out_d) + (64 + 2) U32 sum |dO o O|,
  the exponent by bound(lse2) + U32 (|lse2| + 3).  With eta' the relative error of P / 8, D = dP - delta and
  eD = err(delta) + (64 + 2) U32 (sum_d |dO_d v_jd| + |delta|):
  dS      errs by P ((HALF_ULP + eta' + U32)(1 + 2^-6) |D| + (1 + that) eD)       (the class-token kernels: no HALF_ULP, P and dS stay fp32)
  dQ, dK  scale (err(dS) |K| + acc |dS| |K|) summed over the keys (dK: |Q|, over the queries), + 2 U32 |R|; then HALF_ULP (|R| + that)
  dV      ((HALF_ULP + eta')(1 + 2^-6) + acc) sum_i P_ij |dO_id| + 2 U32 |R|; then HALF_ULP (|R| + that)
  floor   out, dQ, dK and dV: + HALF_ULP FLOOR max |R| of the (image, head) -- 2^-28 of the tensor's largest element, below which the
          subnormal range of bf16 and a flushed exp2 are not modelled.  No fault hides under it; what the truth makes exactly zero is
          asserted to be zero by the tests themselves
Comparators are per row and per tensor: dQ, dK and dV never share a scale."""
import math

import torch

from backward_rows import FLOOR, HALF_ULP, LOG2E, U32, attention_bwd_heads, attention_cls_bwd_heads, bf

HD = 64
LN2 = math.log(2.0)
SECOND = 1.0 + 2.0 ** -6          # second-order terms of products of relative errors that are each below 2^-7
UNDERFLOW_LOG2 = 150.0            # a probability 2^-150 away from the row's largest is zero in fp32 (the smallest subnormal is 2^-149)
TENSORS = ('out', 'lse2', 'dq', 'dk', 'dv')

EDGE_T = sorted({t for k in range(0, 7) for t in (32 * k - 1, 32 * k, 32 * k + 1, 32 * k + 15, 32 * k + 16, 32 * k + 17) if 1 <= t <= 208}
                | {1, 2, 197, 207, 208})
ALL_T = list(range(1, 209))
CLS_T = list(range(1, 225))
GENERATORS = ('random', 'peaked', 'selector', 'pair_selector', 'uniform')


class Case:
    """qkv (B*T, 3*H*64) and dout (B*T, H*64): fp64 tensors of bf16 values, in the kernels' layout.  info: what the generator knows."""

    def __init__(self, name, B, T, H, scale, qkv, dout, info=None):
        self.name, self.B, self.T, self.H, self.scale, self.qkv, self.dout, self.info = name, B, T, H, scale, qkv, dout, info or {}

    def heads(self):
        """q, k, v (B,H,T,64)."""
        return self.qkv.view(self.B, self.T, 3, self.H, HD).permute(2, 0, 3, 1, 4)

    def dout_heads(self):
        return self.dout.view(self.B, self.T, self.H, HD).transpose(1, 2)


def to_rows(t):
    """(B,H,T,64) -> (B*T, H*64)."""
    B, H, T, _ = t.shape
    return t.transpose(1, 2).reshape(B * T, H * HD)


def from_rows(t, B, T, H):
    return t.view(B, T, H, HD).transpose(1, 2)


# ---- generators ---------------------------------------------------------------------------------------------------------------------

def random(B, T, H, seed, gain=1.3, scale=0.125, name='random'):
    g = torch.Generator().manual_seed(seed * 1000 + T)
    qkv = bf(torch.randn(B * T, 3 * H * HD, generator=g, dtype=torch.float64) * gain)
    dout = bf(torch.randn(B * T, H * HD, generator=g, dtype=torch.float64))
    return Case(name, B, T, H, scale, qkv, dout)


def peaked(B, T, H, seed):
    """gain 3: the scores have a standard deviation of 9, most softmax rows are nearly one-hot."""
    return random(B, T, H, seed + 7919, gain=3.0, name='peaked')


def uniform(B, T, H, seed):
    """Q = 0: P = 1 / T, lse2 = log2 T, out = the column mean of V.  Padded keys have score 0 too."""
    c = random(B, T, H, seed + 104729, name='uniform')
    c.qkv.view(B, T, 3, H * HD)[:, :, 0] = 0.0
    return c


def _codebook():
    """256 codes in {+-1}^64 whose pairwise dot products are 0, +-8 or -64: family 0 = +- the rows of the 64 x 64 Sylvester-Hadamard
    matrix, family 1 = the same times the bent sequence (-1)^(x0 x1 + x2 x3 + x4 x5), whose Walsh spectrum is +-8 everywhere.  Code c's
    negative is code c ^ 64; c >> 7 is its family.  (Independent random codes have dots with a standard deviation of 8, and the pair condition
    needs 64 + c_a.c_b - c_a.c_j - c_b.c_j >= 48 for every other key j: a randomly drawn second key misses it.  Here two keys of one family
    that are not each other's negative give 64 + 0 - 8 - 8 at worst, whichever keys are drawn.)"""
    x = torch.arange(64)
    bits = (x[:, None] >> torch.arange(6)) & 1
    had = 1 - 2 * ((bits @ bits.t()) % 2)
    bent = 1 - 2 * ((bits[:, 0] * bits[:, 1] + bits[:, 2] * bits[:, 3] + bits[:, 4] * bits[:, 5]) % 2)
    return torch.cat([had, -had, had * bent, -had * bent]).double()


def _structureless(pi):
    """Not the identity and not a rotation (so: no shift by a multiple of 16 either)."""
    T = len(pi)
    return T < 3 or len({(int(p) - i) % T for i, p in enumerate(pi)}) > 2


def _draw_codes(T, pair, g):
    """Key codes, the permutation pi and (pair) every query's second key, or None if this draw does not meet the conditions."""
    book = _codebook()
    cols = torch.randperm(64, generator=g)
    signs = (torch.randint(0, 2, (64,), generator=g) * 2 - 1).double()
    ids = torch.randperm(256, generator=g)[:T]
    codes = book[ids][:, cols] * signs               # column permutation and sign flips keep every dot product
    pi = torch.randperm(T, generator=g)
    if not _structureless(pi):
        return None
    second = pi.clone()
    if pair and T > 1:                               # a second key of the first one's family that is neither it nor its negative
        a = ids[pi]
        ok = ((ids[None, :] >> 7) == (a[:, None] >> 7)) & (ids[None, :] != a[:, None]) & (ids[None, :] != (a[:, None] ^ 64))
        if not bool(ok.any(1).all()):
            return None
        second = torch.multinomial(ok.double(), 1, generator=g).squeeze(1)
    return codes, pi, second


def _small_ints(B, T, H):
    """V in [-125, 125] and dO in [-6, 6]: integers that differ per key (an odd multiplier modulo the prime 251 > 224), per column, head and
    image.  Exact in bf16, and so is every half of a sum of two of V's."""
    b, h, j, d = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(T), torch.arange(HD), indexing='ij')
    v = ((j + 31 * h + 57 * b) * (2 * d + 1) + 5 * d) % 251 - 125
    g = (j * (2 * d + 3) + 11 * d + 7 * h + 3 * b) % 13 - 6
    return v.double(), g.double()


def _selector(B, T, H, seed, pair):
    q, k = torch.empty(B, H, T, HD, dtype=torch.float64), torch.empty(B, H, T, HD, dtype=torch.float64)
    targets = torch.empty(B, H, T, 2, dtype=torch.long)
    for item in range(B * H):
        for attempt in range(256):                     # the seed search: the first draw that meets the conditions, deterministically
            g = torch.Generator().manual_seed((seed * 256 + attempt) * 4096 + item * 256 + T)
            drawn = _draw_codes(T, pair, g)
            if drawn is not None:
                break
        else:
            raise ValueError(f'selector: no draw meets the conditions at T = {T}')
        codes, pi, second = drawn
        k[item // H, item % H] = 6.0 * codes
        q[item // H, item % H] = 3.0 * (codes[pi] + codes[second])          # selector: second = pi, so 6 c_pi
        targets[item // H, item % H] = torch.stack([pi, second], 1)
    v, dout = _small_ints(B, T, H)
    qkv = torch.stack([q, k, v]).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * H * HD)
    c = Case('pair_selector' if pair else 'selector', B, T, H, 0.125, qkv, to_rows(dout), {'targets': targets})
    assert torch.equal(bf(c.qkv), c.qkv) and torch.equal(bf(c.dout), c.dout)
    c.info['gap_log2'] = selector_gap(c)
    return c


def selector(T, H, seed, B=1):
    """Keys 6 c_j, query i = 6 c_pi(i): out[i] = v[pi(i)], P one-hot to far below fp32 resolution; dQ = dK = 0, dV[pi(i)] = dO[i]."""
    return _selector(B, T, H, seed, False)


def pair_selector(T, H, seed, B=1):
    """Queries 3 (c_a + c_b): the softmax is exactly 1/2, 1/2 on keys a and b (T = 1: the one key)."""
    return _selector(B, T, H, seed + 15485863, True)


def selector_gap(case):
    """The condition of the selector cases, not a measurement: the target keys of a row tie exactly for the largest scaled score and every other
    key lies so far below that its probability underflows in fp32.  Returns the smallest gap times log2 e; raises if it is not above 150."""
    q, k, _ = case.heads()
    s = (q @ k.transpose(-2, -1)) * case.scale
    tgt = case.info['targets']
    on = torch.zeros_like(s, dtype=torch.bool).scatter_(-1, tgt, True)
    top = s.gather(-1, tgt)
    if not torch.equal(top[..., 0], top[..., 1]) or not torch.equal(top[..., 0], s.amax(-1)):
        raise ValueError(f'{case.name}: the target keys do not tie for the largest score at T = {case.T}')
    gap = float((top[..., :1] - s.masked_fill(on, -math.inf)).min()) * LOG2E
    if not gap > UNDERFLOW_LOG2:
        raise ValueError(f'{case.name}: off-target gap {gap:.1f} in log2 units at T = {case.T}, needs > {UNDERFLOW_LOG2}')
    return gap


def make(generator, T, H=1, B=1, seed=0):
    if generator in ('selector', 'pair_selector'):
        return globals()[generator](T, H, seed, B=B)
    return globals()[generator](B, T, H, seed)


# ---- R ----------------------------------------------------------------------------------------------------------------------------------

def selector_probabilities(case):
    """P of the selector cases without a softmax: 1/2 on each target key (1 where the two coincide), zero elsewhere."""
    tgt = case.info['targets']
    P = torch.zeros(case.B, case.H, case.T, case.T, dtype=torch.float64)
    return P.scatter_add_(-1, tgt, torch.full(tgt.shape, 0.5, dtype=torch.float64))


def truth(case, cls=False, softmax=False):
    """R and what the bounds need of it.  cls: only the class token's row of dO carries gradient (the class-token kernels).  The selector
    cases take their closed-form P (softmax=True: the fp64 softmax all the same, which differs from it by less than 2^-150 per element and
    makes gradients of 1e-40 out of exact zeros); lse2 needs no such care."""
    q, k, v = case.heads()
    s = (q @ k.transpose(-2, -1)) * case.scale
    P = torch.softmax(s, -1) if softmax or 'targets' not in case.info else selector_probabilities(case)
    g = case.dout_heads().clone()
    if cls:
        g[:, :, 1:] = 0.0
    o = P @ v
    D = g @ v.transpose(-2, -1) - (g * o).sum(-1, keepdim=True)
    dS = P * D
    return {'out': o, 'lse2': torch.logsumexp(s, -1) * LOG2E, 'P': P, 'D': D, 'dS': dS, 'g': g,
            'dq': case.scale * (dS @ k), 'dk': case.scale * (dS.transpose(-2, -1) @ q), 'dv': P.transpose(-2, -1) @ g}


def closed_form(case):
    """The selector cases without a softmax: P = 1/2 on each target (1 where they coincide)."""
    q, k, v = case.heads()
    tgt, P = case.info['targets'], selector_probabilities(case)
    g = case.dout_heads()
    o = 0.5 * (torch.gather(v, 2, tgt[..., :1].expand(-1, -1, -1, HD)) + torch.gather(v, 2, tgt[..., 1:].expand(-1, -1, -1, HD)))
    top = ((q * torch.gather(k, 2, tgt[..., :1].expand(-1, -1, -1, HD))).sum(-1)) * case.scale
    dS = P * (g @ v.transpose(-2, -1) - (g * o).sum(-1, keepdim=True))
    return {'out': o, 'lse2': top * LOG2E + torch.log2((tgt[..., 0] != tgt[..., 1]).double() + 1.0),
            'dq': case.scale * (dS @ k), 'dk': case.scale * (dS.transpose(-2, -1) @ q), 'dv': P.transpose(-2, -1) @ g}


# ---- E ----------------------------------------------------------------------------------------------------------------------------------

def emulate_fwd(case, cls=False, drop_last_key=False, extra_padded_key=False, swap=None, no_log2l=False):
    """attn_fwd_kernel (cls: attn_cls_fwd_kernel, fp32 probabilities, valid in row 0) as out (bf16) and lse2 (fp32).  The keywords inject
    the forward faults of stand_in()."""
    q, k, v = case.heads()
    c2 = case.scale * LOG2E
    s = q @ k.transpose(-2, -1)
    if drop_last_key:
        s[..., -1] = -math.inf
    m = s.amax(-1, keepdim=True)
    if extra_padded_key:                                # a zero K row with a zero V row: only the statistics see it
        m = m.clamp_min(0.0)
    p = torch.exp2(s * c2 - m * c2).float()
    l = p.sum(-1, keepdim=True).double()
    if extra_padded_key:
        l = l + torch.exp2(-m * c2).float().double()
    pv = p.double() if cls else bf(p.double())
    if swap is not None:
        pv = pv.clone()
        pv[..., list(swap)] = pv[..., list(swap[::-1])]
    lse2 = m.squeeze(-1) * c2 + (0.0 if no_log2l else torch.log2(l.squeeze(-1)))
    return bf((pv @ v) / l), lse2.float().double()


def emulate_bwd(case, out, lse2, cls=False):
    """attn_bwd_kernel (cls: attn_cls_bwd_kernel) on the forward's saved out and lse2: dq, dk, dv before their bf16 rounding."""
    q, k, v = case.heads()
    g = case.dout_heads()
    if cls:
        delta = (g[:, :, 0] * out[:, :, 0]).sum(-1)
        return attention_cls_bwd_heads(q[:, :, 0], k, v, g[:, :, 0], delta, lse2[:, :, 0], case.scale)
    return attention_bwd_heads(q, k, v, g, (g * out).sum(-1), lse2, case.scale)


FAULTS = ('last_key_dropped', 'padded_key_unmasked', 'second_subtile_unwritten', 'keys_exchanged', 'lse2_without_log2_l', 'tail_dv_without_x8',
          'last_subtile_dk_zero', 'dq_dk_times_eighth_over_scale')


def stand_in(case, fault=None, cls=False):
    """E in the kernels' place: a result as the GPU test would capture it, with at most one fault.
      last_key_dropped               the forward masks key >= T - 1 instead of key >= T
      padded_key_unmasked            one zero-padded key (score 0, value 0) takes part in the forward's maximum and sum
      second_subtile_unwritten       rows 32 w + 16 .. of the last wave w that has any there keep their NaN poison in out, lse2 and dQ
      keys_exchanged                 the probabilities of keys 1 and 17 (two slots of one 32-key group) meet each other's V rows
      lse2_without_log2_l            lse2 = m c2
      tail_dv_without_x8             dV of the keys of the last 32-key block is not multiplied by 8
      last_subtile_dk_zero           dK of the last 16-key sub-tile is zero
      dq_dk_times_eighth_over_scale  what attn_bwd_kernel does at scale != 1/8 (2^-3 folded in for the factor, the argument in the exponent);
                                     the case itself must carry that scale
    The backward reads the faulty forward's out and lse2, as it does on the GPU."""
    T = case.T
    kw = {'last_key_dropped': {'drop_last_key': True}, 'padded_key_unmasked': {'extra_padded_key': True},
          'keys_exchanged': {'swap': (1, min(17, T - 1))}, 'lse2_without_log2_l': {'no_log2l': True}}.get(fault, {})
    out, lse2 = emulate_fwd(case, cls=cls, **kw)
    dq, dk, dv = emulate_bwd(case, out, lse2, cls=cls)
    if fault == 'dq_dk_times_eighth_over_scale':
        assert case.scale != 0.125 and not cls     # attention_bwd_heads already is that kernel: nothing to inject
    elif not cls and case.scale != 0.125:
        dq, dk = dq * (case.scale / 0.125), dk * (case.scale / 0.125)          # E of a backward that honours its scale
    if fault == 'tail_dv_without_x8':
        dv = dv.clone()
        dv[:, :, 32 * ((T - 1) >> 5):] /= 8.0
    if fault == 'last_subtile_dk_zero':
        dk = dk.clone()
        dk[:, :, 16 * ((T - 1) >> 4):] = 0.0
    res = {'out': out, 'lse2': lse2, 'dq': bf(dq), 'dk': bf(dk), 'dv': bf(dv)}
    if fault == 'second_subtile_unwritten':
        lo = 32 * ((T - 17) >> 5) + 16
        for n in ('out', 'lse2', 'dq'):
            res[n] = res[n].clone()
            res[n][:, :, lo:lo + 16] = math.nan
    return res


# ---- bounds -----------------------------------------------------------------------------------------------------------------------------

def bounds(case, R, cls=False):
    """Per-element bounds of |result - R| for out, lse2, dq, dk, dv (the module docstring derives them)."""
    q, k, v = case.heads()
    T, scale = case.T, case.scale
    c2 = scale * LOG2E
    acc = (T + 2) * U32
    a = q.abs() @ k.abs().transpose(-2, -1)
    smax = (q @ k.transpose(-2, -1)).abs().amax(-1)
    eta = LN2 * c2 * ((HD + 4) * U32 * a.amax(-1) + 4 * U32 * smax) + 2 * U32                     # (B,H,T)
    P, D, dS, g = R['P'], R['D'], R['dS'], R['g']
    half = 0.0 if cls else HALF_ULP
    e = eta.unsqueeze(-1)
    pre = ((half + e + half * e + acc) + (e + acc + U32)) * SECOND * (P @ v.abs())
    b_out = pre + HALF_ULP * (R['out'].abs() + pre)
    b_lse = LOG2E * (eta + acc) * SECOND + 2 * U32 * (math.log2(T) + 1.0) + U32 * R['lse2'].abs()
    # the backward, fed with the kernel's own out and lse2
    delta = (g * R['out']).sum(-1)
    e_delta = (g.abs() * b_out).sum(-1) + (HD + 2) * U32 * (g * R['out']).abs().sum(-1)
    eta2 = (eta + LN2 * (b_lse + U32 * (R['lse2'].abs() + 3.0))).unsqueeze(-1)
    eD = e_delta.unsqueeze(-1) + (HD + 2) * U32 * (g.abs() @ v.abs().transpose(-2, -1) + delta.abs().unsqueeze(-1))
    relS = (half + eta2 + (U32 if not cls else 2 * U32)) * SECOND
    e_dS = P * (relS * D.abs() + (1.0 + relS) * eD)
    e_P = (half + eta2) * SECOND * P

    def close(pre, ref):
        pre = pre + 2 * U32 * ref.abs()
        return pre + HALF_ULP * (ref.abs() + pre) + floor(ref)

    def floor(ref):
        return HALF_ULP * FLOOR * ref.abs().amax((-2, -1), keepdim=True)

    b_out = b_out + floor(R['out'])

    return {'out': b_out, 'lse2': b_lse,
            'dq': close(scale * (e_dS @ k.abs() + acc * (dS.abs() @ k.abs())), R['dq']),
            'dk': close(scale * (e_dS.transpose(-2, -1) @ q.abs() + acc * (dS.abs().transpose(-2, -1) @ q.abs())), R['dk']),
            'dv': close(e_P.transpose(-2, -1) @ g.abs() + acc * (P.transpose(-2, -1) @ g.abs()), R['dv'])}


# ---- comparators ------------------------------------------------------------------------------------------------------------------------

def ratio(got, ref, bound):
    """|got - ref| / bound per element.  A bound of zero demands equality; anything not finite is infinitely wrong."""
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return torch.where(torch.isfinite(got), r, math.inf)


def worst(r):
    """The largest ratio and its (image, head, row)."""
    per_row = r.reshape(r.shape[0], r.shape[1], r.shape[2], -1).amax(-1)
    i = int(per_row.argmax())
    H, T = per_row.shape[1], per_row.shape[2]
    return float(per_row.flatten()[i]), (i // (H * T), (i // T) % H, i % T)


def compare(result, R, B, rows=None, tensors=TENSORS):
    """{tensor: (worst ratio to its own bound, (image, head, row))} -- out, lse2, dQ, dK and dV each per row on its own bound.  rows: a slice
    of the query rows of out, lse2 and dq that are compared (the class-token kernels write row 0 of out and lse2 only)."""
    rep = {}
    for n in tensors:
        got, ref, bound = result[n], R[n], B[n]
        if rows is not None and n in ('out', 'lse2'):
            got, ref, bound = got[:, :, rows], ref[:, :, rows], bound[:, :, rows]
        rep[n] = worst(ratio(got, ref, bound))
    return rep


def failures(rep):
    return {n: v for n, v in rep.items() if not v[0] <= 1.0}


def old_criteria(result, R):
    """What test_attention_fwd_bwd asserts, on a result: one max-norm number per tensor, dQ, dK and dV together."""
    grad = torch.cat([R['dq'], R['dk'], R['dv']], -1)
    got = torch.cat([result['dq'], result['dk'], result['dv']], -1)
    return (float((result['out'] - R['out']).abs().max()) < 2e-2 and float((result['lse2'] - R['lse2']).abs().max()) < 1e-3
            and float((got - grad).abs().max()) < 3e-2 * float(grad.abs().max()))


def mutation_table(Ts=(197, 33, 49, 64), seed=0):
    """{fault: {'caught': {T: the generators whose faulty result fails the new comparator}, 'slipped': the (generator, T) at which the new
    comparator fails the faulty result and old_criteria passes it}}.  A fault that cannot show in a generator (two exchanged keys under
    uniform probabilities, a padded key next to a one-hot row) is not caught there; every fault must be caught at every T.  The scale fault
    runs at scale 0.25 on random, peaked and uniform (the selectors' conditions are stated for 1/8)."""
    table = {}
    for fault in FAULTS:
        caught, slipped = {T: [] for T in Ts}, []
        for gen in GENERATORS:
            for T in Ts:
                case = make(gen, T, H=1, B=1, seed=seed)
                if fault == 'dq_dk_times_eighth_over_scale':
                    if gen not in ('random', 'peaked', 'uniform'):
                        continue
                    case.scale = 0.25
                R = truth(case)
                res = stand_in(case, fault)
                if failures(compare(res, R, bounds(case, R))):
                    caught[T].append(gen)
                    if old_criteria(res, R):
                        slipped.append((gen, T))
        table[fault] = {'caught': caught, 'slipped': slipped}
    return table
