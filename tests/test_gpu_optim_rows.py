"""The optimizer kernels (csrc/optim.hip) against the fp64 truth R of tests/optim_cases.py, per element, within the bounds derived there:
rovit_sq_norm_clip and rovit_sq_norm_accum at every piece, block and buffer edge (exact sums bit for bit, the others within gamma(d)),
rovit_clip_coef as the same function as rovit_sq_norm_clip's last step, and rovit_adamw_flat, rovit_adamw_flat_multi and
rovit_adamw_ema_flat_multi with every per-element recipe on every position class.  Everything goes through the exported C entry points.

Every call: every buffer lies between GUARD sentinel floats that must survive (NaN around the gradient buffers of the norm kernels: a read
past a buffer's end poisons the norm), inputs are bit-identical afterwards, a second identical call gives bit-identical outputs, and the
scratch ticket word is 0 after every call.  No test builds a model.

Each `sweep_*` function runs one group of cases and returns {tensor: (largest |gpu - R| / bound, where)}; the tests assert ratio <= 1,
tools/optim_rows_error.py writes the same figures to profiles/optim_rows_error.jsonl."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import optim_cases as oc

pytestmark = pytest.mark.gpu

GUARD = 64                       # floats either side of every buffer (keeps the 16-byte alignment)
SENTINEL = 12345.0
UNWRITTEN = -7.0                 # what outputs hold before a call


def _native():
    from rovit_hip import native
    native.load()
    return native


def dev():
    return torch.device('cuda:0')


class Guarded:
    """n floats between GUARD floats of `fill` on each side; `.t` is the 16-byte aligned view a kernel gets (a valid pointer for n = 0 too)."""

    def __init__(self, values, fill=SENTINEL):
        values = np.atleast_1d(np.asarray(values, dtype=np.float32))
        self.n = values.size
        self.full = torch.full((self.n + 2 * GUARD,), fill, dtype=torch.float32, device=dev())
        self.t = self.full[GUARD:GUARD + self.n]
        if self.n:
            self.t.copy_(torch.from_numpy(values))
        assert (self.full.data_ptr() + 4 * GUARD) % 16 == 0
        self.bits0 = self.bits()

    def ptr(self):
        return self.full.data_ptr() + 4 * GUARD

    def bits(self):
        return self.full.view(torch.int32).clone()

    def intact(self):
        b = self.bits()
        return torch.equal(b[:GUARD], self.bits0[:GUARD]) and torch.equal(b[GUARD + self.n:], self.bits0[GUARD + self.n:])

    def unchanged(self):
        return torch.equal(self.bits(), self.bits0)

    def np(self):
        return self.t.detach().cpu().numpy().copy()


def _ptrs(bufs):
    return (C.c_void_p * len(bufs))(*[None if b is None else b.ptr() for b in bufs])


def _settle(inputs, outputs, scratch=None):
    torch.cuda.synchronize()
    for b in outputs:
        assert b.intact(), 'a sentinel was written'
    for b in inputs:
        assert b.unchanged(), 'an input or its sentinels were written'
    if scratch is not None:
        assert scratch.intact(), 'a sentinel of the scratch was written'
        assert int(scratch.t[:1].view(torch.int32)) == 0, 'the ticket was not re-armed'


_SCRATCH = {}


def scratch(floats):
    """One scratch per size for the whole module, zeroed once: every call must leave its ticket at 0 for the next."""
    if floats not in _SCRATCH:
        _SCRATCH[floats] = Guarded(np.zeros(floats, dtype=np.float32))
    return _SCRATCH[floats]


# ---- the norm kernels --------------------------------------------------------------------------------------------------------------------

def gpu_clip(bufs, max_norm):
    """rovit_sq_norm_clip -> (norm, coef) as fp32."""
    n = _native()
    g = [Guarded(b, fill=math.nan) for b in bufs]
    coef, norm, sc = Guarded([UNWRITTEN]), Guarded([UNWRITTEN]), scratch(264)
    counts = (C.c_size_t * len(g))(*[b.n for b in g])

    def call():
        n.call('rovit_sq_norm_clip', _ptrs(g), counts, len(g), float(max_norm), coef.ptr(), norm.ptr(), sc.ptr(), 264, n.stream_ptr())
        _settle(g, [coef, norm], sc)
        return norm.np()[0], coef.np()[0]
    first = call()
    coef.t.fill_(UNWRITTEN); norm.t.fill_(UNWRITTEN)
    second = call()
    assert np.array_equal(np.array(first).view(np.int32), np.array(second).view(np.int32)), 'a second identical call gave different bits'
    return first


def gpu_clip_coef(sq, max_norm):
    """rovit_clip_coef on a squared norm -> (norm, coef) as fp32."""
    n = _native()
    s, coef, norm = Guarded([sq]), Guarded([UNWRITTEN]), Guarded([UNWRITTEN])
    n.call('rovit_clip_coef', s.ptr(), float(max_norm), coef.ptr(), norm.ptr(), n.stream_ptr())
    _settle([s], [coef, norm])
    return norm.np()[0], coef.np()[0]


def gpu_accum(bufs, with_scratch, exact=True):
    """rovit_sq_norm_accum of every buffer into one zeroed *out_sq -> its fp32 value."""
    n = _native()
    g = [Guarded(b, fill=math.nan) for b in bufs]
    out, sc = Guarded([0.0]), scratch(520) if with_scratch else None

    def call():
        for b in g:
            n.call('rovit_sq_norm_accum', b.ptr(), b.n, out.ptr(), None if sc is None else sc.ptr(), n.stream_ptr())
            _settle(g, [out], sc)
        return out.np()[0]
    first = call()
    out.t.zero_()
    second = call()
    if with_scratch or exact:                                          # the atomic path promises an order only where none matters
        assert np.float32(first).view(np.int32) == np.float32(second).view(np.int32), 'a second identical call gave different bits'
    return first


def sweep_clip(cases):
    """rovit_sq_norm_clip against R, and rovit_clip_coef on the same squared norm (known exactly for the exact cases): the same bits."""
    rec = {}
    for case in cases:
        got = {}

        def run(bufs, max_norm):
            got['norm'], got['coef'] = gpu_clip(bufs, max_norm)
            return got['norm'], got['coef']
        oc.judge_clip(case, run, rec)
        if case.exact:
            sq = oc.sq_truth(case.bufs)
            norm2, coef2 = gpu_clip_coef(sq, case.max_norm)
            (norm, bn), (coef, bc), _ = oc.clip_truth(case)
            oc.worst(rec, 'clip_coef norm', oc.ratio(norm2, norm, bn), lambda i: case.name)
            oc.worst(rec, 'clip_coef coef', oc.ratio(coef2, coef, bc), lambda i: case.name)
            a, b = np.array([norm2, coef2]), np.array([got['norm'], got['coef']])
            same = ((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all()       # a NaN's payload is not part of the rule
            assert same,(case.name, 'rovit_clip_coef and rovit_sq_norm_clip disagree', norm2, coef2, got)
    return rec


def sweep_accum(cases):
    rec = {}
    for case in cases:
        for with_scratch in (True, False):
            oc.judge_accum(case, lambda bufs, s: gpu_accum(bufs, s, case.exact), rec, with_scratch)
    return rec


def test_clip_at_every_buffer_edge_and_the_coefficient_at_every_special_norm():
    rec = sweep_clip(list(oc.clip_small_cases()) + list(oc.clip_coef_cases()))
    print(rec)
    assert all(v[0] <= 1 for v in rec.values()), rec


@pytest.mark.parametrize('pieces', oc.PIECE_TOTALS)
def test_clip_at_every_piece_count(pieces):
    rec = sweep_clip([c for c in oc.clip_piece_cases() if c.name.startswith(f'pieces{pieces}_')])
    print(rec)
    assert all(v[0] <= 1 for v in rec.values()), rec


def test_the_ticket_is_rearmed_across_grids_of_1_256_and_3_on_one_scratch():
    rng = np.random.default_rng(8)
    cases = [oc.ClipCase(f'grid{p}', [oc._dense(p * oc.NORM_PIECE - 8, rng)], np.float32(1.0), True, [], set()) for p in (1, 256, 3, 1)]
    assert [oc.clip_layout([c.bufs[0].size])[2] for c in cases] == [1, 256, 3, 1]
    rec = sweep_clip(cases)                                           # _settle checks the ticket word after every one of the calls
    print(rec)
    assert all(v[0] <= 1 for v in rec.values()), rec


def test_accum_at_every_size_with_and_without_scratch():
    rec = sweep_accum(oc.accum_cases())
    print(rec)
    assert rec['sq'][0] <= 1 and rec['sq_atomic'][0] <= 1, rec


# ---- AdamW -----------------------------------------------------------------------------------------------------------------------------

def gpu_adam(entry):
    """-> run(segs, gs, ts, coef, hyper, ema) for optim_cases.judge_adam through one entry point ('flat', 'multi', 'ema')."""
    n = _native()

    def once(segs, gs, ts, coef, hyper):
        k = len(segs)
        b = [{x: Guarded(s[x]) for x in 'pmve'} for s in segs]
        for d, g in zip(b, gs):
            d['g'] = Guarded(g)
        cf = None if coef is None else Guarded([coef])
        sizes = (C.c_size_t * k)(*[s['p'].size for s in segs])
        lrs, tt = (C.c_float * k)(*[float(s['lr']) for s in segs]), (C.c_int * k)(*ts)
        hy = [float(x) for x in hyper]
        if entry == 'flat':
            assert k == 1
            d = b[0]
            n.call('rovit_adamw_flat', d['p'].ptr(), d['g'].ptr(), d['m'].ptr(), d['v'].ptr(), d['p'].n, None if cf is None else cf.ptr(),
                   float(segs[0]['lr']), *hy, ts[0], n.stream_ptr())
        elif entry == 'multi':
            n.call('rovit_adamw_flat_multi', *(_ptrs([d[x] for d in b]) for x in 'pgmv'), sizes, lrs, tt, k, None if cf is None else cf.ptr(), *hy,
                   n.stream_ptr())
        else:
            decays = (C.c_float * k)(*[float(s['decay']) for s in segs])
            n.call('rovit_adamw_ema_flat_multi', *(_ptrs([d[x] for d in b]) for x in 'pgmve'), sizes, lrs, tt, decays, k,
                   None if cf is None else cf.ptr(), *hy, n.stream_ptr())
        _settle([d['g'] for d in b] + ([] if cf is None else [cf]) + ([] if entry == 'ema' else [d['e'] for d in b]),
                [d[x] for d in b for x in ('pmve' if entry == 'ema' else 'pmv')])
        return [{x: d[x].np() for x in 'pmve'} for d in b]

    def run(segs, gs, ts, coef, hyper, ema):
        first = once(segs, gs, ts, coef, hyper)
        second = once(segs, gs, ts, coef, hyper)
        for a, c in zip(first, second):
            for x in 'pmve':
                assert np.array_equal(a[x].view(np.int32), c[x].view(np.int32)), 'a second identical call gave different bits'
        return first
    return run


def sweep_adam(cases, entries=('flat', 'multi', 'ema')):
    """Every case through every entry that takes it (rovit_adamw_flat: one segment).  Keys are 'entry tensor'.  p, m, v of
    rovit_adamw_flat_multi and rovit_adamw_ema_flat_multi must agree bit for bit: their existing contract."""
    out = {}
    for case in cases:
        final = {}
        for entry in entries:
            if entry == 'flat' and len(case.segs) != 1:
                continue
            rec = {}
            final[entry] = oc.judge_adam(case, gpu_adam(entry), rec, entry == 'ema')
            for x, v in rec.items():
                if f'{entry} {x}' not in out or not v[0] <= out[f'{entry} {x}'][0]:
                    out[f'{entry} {x}'] = v
        if 'multi' in final and 'ema' in final:
            for k, (a, b) in enumerate(zip(final['multi'], final['ema'])):
                for x in 'pmv':
                    assert np.array_equal(a[x].view(np.int32), b[x].view(np.int32)), (case.name, k, x, 'the plain and the EMA kernel disagree')
    return out


def _assert_rec(rec):
    print(rec)
    assert rec and all(v[0] <= 1 for v in rec.values()), {k: v for k, v in rec.items() if not v[0] <= 1}


@pytest.mark.parametrize('n', oc.SINGLE_N)
def test_adamw_one_segment_every_recipe_on_every_position(n):
    _assert_rec(sweep_adam(oc.adam_single_cases(n)))


def test_adamw_every_step_count_with_every_coefficient():
    _assert_rec(sweep_adam(oc.adam_product_cases()))


@pytest.mark.parametrize('sizes', oc.MULTI_SIZES, ids=lambda s: '_'.join(map(str, s)))
def test_adamw_segments_of_unlike_sizes_with_their_own_lr_and_t(sizes):
    _assert_rec(sweep_adam(oc.adam_multi_cases(sizes), ('multi', 'ema')))


@pytest.mark.parametrize('shift', range(oc.K))
def test_adamw_flat_above_its_block_cap(shift):
    _assert_rec(sweep_adam(oc.adam_flat_large_cases([shift]), ('flat',)))


def test_adamw_eight_steps_from_nontrivial_moments_each_judged_alone():
    _assert_rec(sweep_adam([oc.adam_steps_case()], ('multi', 'ema')))


def test_adamw_flat_accepts_an_empty_buffer_and_touches_nothing():
    n = _native()
    b = [Guarded([]) for _ in range(4)]
    n.call('rovit_adamw_flat', *(x.ptr() for x in b), 0, None, 1e-3, *[float(x) for x in oc.HYPER], 1, n.stream_ptr())
    _settle(b, [])


def body_tail_record():
    """The same element values in a body slot and in a tail slot, through the three entries.  -> {'multi_equals_ema': ..., 'flat_equals_multi':
    ..., 'tail_equals_body': {entry: ...}}: only the first is promised."""
    rng = np.random.default_rng(9)
    body = 4 * oc.K
    res = {'multi_equals_ema': True, 'flat_equals_multi': True, 'tail_equals_body': {e: True for e in ('flat', 'multi', 'ema')}}
    for j in range(0, body - 2, 3):
        coef, t = oc.COEFS[(j // 3) % 4], oc.TS[(j // 3) % 4]
        s = oc._seg(body, 0, rng, oc.LRS[0], t, 0.9, coef, oc.HYPER)
        for x in 'pgmve':
            s[x] = np.concatenate([s[x], s[x][j:j + 3]])
        s['recipe'] = np.concatenate([s['recipe'], s['recipe'][j:j + 3]])
        got = {e: gpu_adam(e)([s], [s['g']], [t], coef, oc.HYPER, e == 'ema')[0] for e in ('flat', 'multi', 'ema')}
        bits = lambda a: a.view(np.int32)
        for x in 'pmv':
            res['multi_equals_ema'] &= bool(np.array_equal(bits(got['multi'][x]), bits(got['ema'][x])))
            res['flat_equals_multi'] &= bool(np.array_equal(bits(got['flat'][x]), bits(got['multi'][x])))
            for e in got:
                res['tail_equals_body'][e] &= bool(np.array_equal(bits(got[e][x][body:]), bits(got[e][x][j:j + 3])))
    return res


def test_body_and_tail_slots_through_the_three_entries():
    res = body_tail_record()
    print(res)
    assert res['multi_equals_ema']
