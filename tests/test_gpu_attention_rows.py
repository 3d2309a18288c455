"""The attention kernels of csrc/attention.hip against the fp64 truth R of tests/attention_cases.py, per row and per tensor, within the
bounds derived there: every token count 1 .. 208 (1 .. 224 for the class-token kernels), heads and item counts off the kernels' grouping,
the structured cases at every edge token count, the scale rule and determinism.  Everything goes through the exported C entry points.

Every call: outputs pre-filled with NaN, every buffer followed by guard rows whose sentinel must survive, and after the backward qkv, out,
lse2 and dout bit-identical to what went in.  No shape here is outside what the entry points accept; the refusals are checked on the CPU
(test_attention_cases_cpu.py)."""
import math

import pytest
import torch

import attention_cases as ac

pytestmark = pytest.mark.gpu

GUARD = 4                      # rows behind every buffer
SENTINEL = -12288.0            # exact in bf16 and fp32
SCALES = (0.0625, 0.125, 0.25, 0.1)


def _native():
    from rovit_hip import native
    native.load()
    return native


def dev():
    return torch.device('cuda:0')


class Buf:
    """rows x cols on the device with GUARD sentinel rows behind it; `t` is the part the kernels are given."""

    def __init__(self, rows, cols, dtype, init):
        self.full = torch.full((rows + GUARD, cols), SENTINEL, dtype=dtype, device=dev())
        self.t = self.full[:rows]
        if isinstance(init, float):
            self.t.fill_(init)
        else:
            self.t.copy_(init.reshape(rows, cols).to(dtype))

    def guard_intact(self):
        return bool((self.full[self.t.shape[0]:] == SENTINEL).all())

    def bits(self):
        return self.t.contiguous().view(torch.int16 if self.t.dtype == torch.bfloat16 else torch.int32).clone()


def _result(case, out, lse2, dqkv):
    B, T, H = case.B, case.T, case.H
    dq, dk, dv = dqkv.t.double().cpu().view(B, T, 3, H, ac.HD).permute(2, 0, 3, 1, 4)
    return {'out': ac.from_rows(out.t.double().cpu(), B, T, H), 'lse2': lse2.t.double().cpu().view(B, H, T), 'dq': dq, 'dk': dk, 'dv': dv}


def run(case, cls=False, refusals=None):
    """Forward and backward of `case` through rovit_attention_fwd / _bwd (cls: the class-token entries): (result, raw) with raw the device
    bits of out, lse2 and dqkv.  refusals: a list that receives the entries that raised RovitHipError instead of running (the scale test);
    without it a refusal is an error like any other."""
    from rovit_hip import RovitHipError
    native = _native()
    p, sp = native.ptr, native.stream_ptr()
    B, T, H = case.B, case.T, case.H
    qkv = Buf(B * T, 3 * H * ac.HD, torch.bfloat16, case.qkv)
    dout = Buf(B * T, H * ac.HD, torch.bfloat16, case.dout)
    out = Buf(B * T, H * ac.HD, torch.bfloat16, math.nan)
    lse2 = Buf(B * H, T, torch.float32, math.nan)
    dqkv = Buf(B * T, 3 * H * ac.HD, torch.bfloat16, math.nan)
    qkv0, dout0 = qkv.bits(), dout.bits()
    names = ('rovit_attention_cls_fwd', 'rovit_attention_cls_bwd') if cls else ('rovit_attention_fwd', 'rovit_attention_bwd')

    def call(name, *args):
        try:
            native.call(name, *args)
            return True
        except RovitHipError:
            if refusals is None:
                raise
            refusals.append(name)
            return False

    ran_fwd = call(names[0], p(qkv.t), p(out.t), p(lse2.t), B, T, H, ac.HD, case.scale, sp)
    torch.cuda.synchronize()
    if not ran_fwd:                                    # the backward needs a forward's out and lse2: E's (the refused entry wrote nothing)
        assert bool(torch.isnan(out.t).all()) and bool(torch.isnan(lse2.t).all())
        o, l = ac.emulate_fwd(case, cls=cls)
        out.t.copy_(ac.to_rows(o).to(torch.bfloat16))
        lse2.t.copy_(l.reshape(B * H, T).float())
    out0, lse0 = out.bits(), lse2.bits()
    ran_bwd = call(names[1], p(qkv.t), p(out.t), p(lse2.t), p(dout.t), p(dqkv.t), B, T, H, ac.HD, case.scale, sp)
    torch.cuda.synchronize()
    for b in (qkv, dout, out, lse2, dqkv):
        assert b.guard_intact(), f'{case.name} T = {T}: a guard row was written'
    assert torch.equal(qkv.bits(), qkv0) and torch.equal(dout.bits(), dout0), 'an input was written'
    assert torch.equal(out.bits(), out0) and torch.equal(lse2.bits(), lse0), 'the backward wrote out or lse2'
    if not ran_bwd:
        assert bool(torch.isnan(dqkv.t).all())
    res = _result(case, out, lse2, dqkv)
    if cls and ran_fwd:                                # the class-token forward writes row 0 of out and lse2 and nothing else
        assert T == 1 or (bool(torch.isnan(res['out'][:, :, 1:]).all()) and bool(torch.isnan(res['lse2'][:, :, 1:]).all()))
    return res, (out0, lse0, dqkv.bits())


def check(case, cls=False, label=''):
    """Run, compare per row against R, print each figure; returns (failures, result, R, bounds)."""
    R = ac.truth(case, cls=cls)
    Bd = ac.bounds(case, R, cls=cls)
    res, _ = run(case, cls=cls)
    rep = ac.compare(res, R, Bd, rows=slice(0, 1) if cls else None)
    print(f'{label or case.name} B {case.B} T {case.T} H {case.H} scale {case.scale}' + (' cls' if cls else '') + ': '
          + '  '.join(f'{n} {v[0]:.3f} @ {v[1]}' for n, v in rep.items()))
    if cls and case.T > 1:
        assert float(res['dq'][:, :, 1:].abs().max()) == 0.0, 'class-token backward: dQ of a patch query is not exactly zero'
    return ac.failures(rep), res, R, Bd


@pytest.mark.parametrize('group', range(13))
def test_every_token_count(group):
    """B = 2 images of different data (a wrong batch stride shows), H = 3, random inputs, 16 consecutive token counts a test."""
    bad = {}
    for T in ac.ALL_T[16 * group:16 * group + 16]:
        f = check(ac.random(2, T, 3, seed=1))[0]
        if f:
            bad[T] = f
    assert not bad, bad


@pytest.mark.parametrize('B,H', [(1, 1), (5, 1), (7, 1), (3, 2), (1, 4), (3, 4)])
@pytest.mark.parametrize('T', [17, 64, 197])
def test_heads_and_items(B, H, T):
    """H in {1, 2, 4}; B H = 1, 5, 7 and 6 items are no multiple of the four items a workgroup of the class-token kernels takes."""
    case = ac.random(B, T, H, seed=2)
    bad = {cls: f for cls in (False, True) for f in [check(case, cls=cls)[0]] if f}
    assert not bad, bad


@pytest.mark.parametrize('gen', ['selector', 'pair_selector', 'uniform', 'peaked'])
def test_structured_cases(gen):
    """Every edge token count, B = 1, H = 2.  Beyond the bounds:
      selector, pair_selector  out and dV are asserted BIT FOR BIT against bf16(R).  Every operand is an exactly representable integer or half
                               integer; the unnormalised probability of a target key is 1 + O(2^-16) in fp32 and exactly 1 after its bf16
                               rounding (P / 8 in the backward: exactly 2^-3 or 2^-4), every other one underflows to zero, the sums are exact
                               in fp32, and the division by l = 1 (or 2) times 1 + O(2^-16) moves an exactly representable quotient by far
                               less than the half ulp its rounding forgives.
                               lse2 = m c2 + log2 l rounds m c2 and log2f in fp32: bound only.
      selector                 dQ and dK are asserted EXACTLY ZERO: on the target key dP - delta cancels in integers, elsewhere P is zero.
      pair_selector            dS = P / 8 (dP - delta) is a true bf16 rounding of a product with an fp32 P / 8: dQ and dK by the bounds.
      uniform                  Q = 0: dK = sum bf16(dS / 8) q is asserted EXACTLY ZERO.  Padded keys have the valid keys' score here."""
    bad = {}
    for T in ac.EDGE_T:
        case = ac.make(gen, T, H=2, B=1, seed=4)
        f, res, R, _ = check(case)
        if gen in ('selector', 'pair_selector'):
            for n in ('out', 'dv'):
                if not torch.equal(res[n], ac.bf(R[n])):
                    f[n + ' bits'] = ac.worst((res[n] - ac.bf(R[n])).abs())
        zero = {'selector': ('dq', 'dk'), 'uniform': ('dk',)}.get(gen, ())
        for n in zero:
            if not float(res[n].abs().max()) == 0.0:
                f[n + ' not zero'] = ac.worst(res[n].abs())
        if f:
            bad[T] = f
    assert not bad, bad


@pytest.mark.parametrize('group', range(14))
def test_class_token_kernels(group):
    """rovit_attention_cls_fwd / _bwd at 16 consecutive token counts of 1 .. 224 against R's row 0 (dQ rows >= 1 exactly zero: check()); up to
    208 also against the dense kernels given the same gradient (zero off the class token's row), within the two kernels' bounds together."""
    bad = {}
    for T in ac.CLS_T[16 * group:16 * group + 16]:
        case = ac.random(2, T, 3, seed=3)
        f, res, R, Bc = check(case, cls=True)
        if T <= 208:
            dense = ac.Case('random, dO of the class token only', case.B, T, case.H, case.scale, case.qkv, ac.to_rows(R['g']))
            Bd = ac.bounds(dense, R)
            res_d, _ = run(dense)
            both = {n: Bc[n] + Bd[n] for n in ac.TENSORS}
            rep = ac.compare(res, res_d, both, rows=slice(0, 1))
            f.update({n + ' vs dense': v for n, v in ac.failures(rep).items()})
            f.update({n + ' dense': v for n, v in ac.failures(ac.compare(res_d, R, Bd)).items()})
        if f:
            bad[T] = f
    assert not bad, bad


@pytest.mark.parametrize('T', [33, 197])
@pytest.mark.parametrize('scale', SCALES)
def test_scale(scale, T):
    """Each entry either matches R at that scale or raises RovitHipError; at 1/8 nothing is refused.  (Before the entry checks
    rovit_attention_bwd ran at any scale and returned dQ and dK multiplied by 0.125 / scale.)"""
    bad = {}
    for cls in (False, True):
        case = ac.random(2, T, 3, seed=5, scale=scale)
        refused = []
        R = ac.truth(case, cls=cls)
        res, _ = run(case, cls=cls, refusals=refused)
        ran = [n for n in ac.TENSORS if not any(r.endswith('_fwd') for r in refused) or n not in ('out', 'lse2')]
        ran = [n for n in ran if not any(r.endswith('_bwd') for r in refused) or n not in ('dq', 'dk', 'dv')]
        rep = ac.compare(res, R, ac.bounds(case, R, cls=cls), rows=slice(0, 1) if cls else None, tensors=ran)
        print(f'scale {scale} T {T}' + (' cls' if cls else '') + f': refused {refused}  '
              + '  '.join(f'{n} {v[0]:.3f} @ {v[1]}' for n, v in rep.items()))
        if scale == 0.125 and refused:
            bad[(cls, 'refused')] = refused
        if ac.failures(rep):
            bad[cls] = ac.failures(rep)
    assert not bad, bad


def test_two_runs_give_the_same_bytes():
    for T in ac.EDGE_T:
        case = ac.random(2, T, 3, seed=1)
        a, b = run(case)[1], run(case)[1]
        assert all(torch.equal(x, y) for x, y in zip(a, b)), T
