"""The KAN spline kernels (csrc/kan_heads.hip, csrc/kan_stack.hip, csrc/kan_device.h) against the fp64 truth R of tests/kan_cases.py, per row
and per element, within the bounds derived there: every knot of every knot count 8 .. 64 from both sides, the launch-shape branches of the
per-layer kernels, the fused stack (vector and matrix-core form) and the stack backward.  Everything goes through the exported C entry
points (native.call).

Every call: outputs pre-filled with NaN, every buffer followed by GUARD sentinel rows that must survive, inputs bit-identical afterwards,
and a second identical call gives bit-identical outputs.  Each layer of a stack is judged alone: R is given the GPU's own previous-layer
output (and the GPU's own dL/dz of the layer above).  No shape here is outside what the entry points accept; the refusals are checked
without a device in test_kan_cases_cpu.py.

Each `sweep_*` function runs one group of cases and returns {tensor: (largest |gpu - R| / bound, where)}; the tests assert ratio <= 1,
tools/kan_rows_error.py writes the same figures to profiles/kan_rows_error.jsonl."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import kan_cases as kc

pytestmark = pytest.mark.gpu

GUARD = 4
SENTINEL = -12288.0
PROBES = {p.name: p for p in kc.all_probes()}
NONUNIFORM = tuple(kc.nonuniform_knots())


def _native():
    from rovit_hip import native
    native.load()
    return native


def dev():
    return torch.device('cuda:0')


class Buf:
    """An fp32 array on the device with GUARD sentinel rows (of its last dimension) behind it; `t` is what the kernels are given."""

    def __init__(self, shape, init):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        cols = shape[-1]
        rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
        self.full = torch.full((rows + GUARD, cols), SENTINEL, dtype=torch.float32, device=dev())
        self.t = self.full[:rows].view(shape)
        if isinstance(init, float):
            self.t.fill_(init)
        else:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32)).view(shape))
        self.rows = rows
        self.bits0 = self.bits()

    def guard_intact(self):
        return bool((self.full[self.rows:] == SENTINEL).all())

    def bits(self):
        return self.t.contiguous().view(torch.int32).clone()

    def unchanged(self):
        return torch.equal(self.bits(), self.bits0)

    def np(self):
        return self.t.detach().cpu().numpy().astype(np.float64)


def nan_buf(shape):
    return Buf(shape, math.nan)


def ints(xs):
    return (C.c_int * len(xs))(*[int(v) for v in xs])


def settle(inputs, outputs):
    torch.cuda.synchronize()
    for b in list(inputs) + list(outputs):
        assert b.guard_intact(), 'a guard row was written'
    for b in inputs:
        assert b.unchanged(), 'an input was written'


def twice(fn, inputs, outputs):
    """Run fn, check guards and inputs, run it again on re-NaN'd outputs and require bit-identical results."""
    for b in inputs:
        b.bits0 = b.bits()
    fn()
    settle(inputs, outputs)
    first = [b.bits() for b in outputs]
    for b in outputs:
        if getattr(b, 'prefill', None) is not None:
            b.t.copy_(b.prefill)
        else:
            b.t.fill_(math.nan)
    fn()
    settle(inputs, outputs)
    for b, f in zip(outputs, first):
        assert torch.equal(b.bits(), f), 'a second identical call gave different bits'


class DevLayer:
    def __init__(self, p):
        self.p = p
        self.W, self.knots, self.lw, self.lb = Buf(p.W.shape, p.W), Buf(p.knots.shape, p.knots), Buf(p.lw.shape, p.lw), Buf(p.lb.shape, p.lb)

    def bufs(self):
        return [self.W, self.knots, self.lw, self.lb]


# ------------------------------------------------------------------------------------------------------------------------------------
# entry-point wrappers
# ------------------------------------------------------------------------------------------------------------------------------------
def gpu_basis(t32, knots):
    n = _native()
    x, k = Buf((t32.size,), t32), Buf((knots.size,), knots)
    out = nan_buf((t32.size, knots.size - 4))
    twice(lambda: n.call('rovit_kan_basis', n.ptr(x.t), n.ptr(k.t), n.ptr(out.t), t32.size, knots.size, n.stream_ptr()), [x, k], [out])
    return out.np()


def gpu_layer_fwd(x, d, act):
    """x: a Buf (batch, in).  Returns the output Buf."""
    n, p = _native(), d.p
    batch = x.t.shape[0]
    out = nan_buf((batch, p.out_f))
    twice(lambda: n.call('rovit_kan_layer_fwd', n.ptr(x.t), n.ptr(d.W.t), n.ptr(d.knots.t), n.ptr(d.lw.t), n.ptr(d.lb.t), n.ptr(out.t), batch,
                         p.in_f, p.out_f, p.nk, act, n.stream_ptr()), [x] + d.bufs(), [out])
    return out


def gpu_layer_bwd(x, d, act, y, g, want_dx=True, want_dw=True, prefill=None):
    """rovit_kan_layer_bwd; prefill: dx's content before an accumulating call.  Returns {name: Buf}."""
    n, p = _native(), d.p
    batch = x.t.shape[0]
    out = {}
    if want_dx:
        out['dx'] = nan_buf((batch, p.in_f))
        if prefill is not None:
            out['dx'].t.copy_(torch.from_numpy(prefill))
            out['dx'].prefill = out['dx'].t.clone()
    if want_dw:
        out.update(dW=nan_buf(p.W.shape), dlw=nan_buf(p.lw.shape), dlb=nan_buf(p.lb.shape))
    pt = lambda name: n.ptr(out[name].t) if name in out else None
    twice(lambda: n.call('rovit_kan_layer_bwd', n.ptr(x.t), n.ptr(d.W.t), n.ptr(d.knots.t), n.ptr(d.lw.t), n.ptr(y.t), n.ptr(g.t), pt('dx'), pt('dW'),
                         pt('dlw'), pt('dlb'), batch, p.in_f, p.out_f, p.nk, act, int(prefill is not None), n.stream_ptr()),
          [x, y, g] + d.bufs(), list(out.values()))
    return out


def gpu_stack_fwd(x, ds, acts, mfma=False):
    n = _native()
    batch = x.t.shape[0]
    dims = [ds[0].p.in_f] + [d.p.out_f for d in ds]
    nks = [d.p.nk for d in ds]
    outs = [nan_buf((batch, d.p.out_f)) for d in ds]
    prep, scratch = [], []
    for d in ds:
        p = d.p
        if mfma:
            nm = n.load().rovit_kan_mfma_prepared_floats(p.in_f, p.out_f, p.nk - 4)
            assert nm > 0
            wm = nan_buf((nm,))
            twice(lambda: n.call('rovit_kan_prepare_mfma', n.ptr(d.W.t), n.ptr(d.lw.t), n.ptr(wm.t), p.in_f, p.out_f, p.nk - 4, n.stream_ptr()),
                  [d.W, d.lw], [wm])
            prep.append((wm,))
        else:
            wt, lwt = nan_buf((p.in_f, p.nk - 4, p.out_f)), nan_buf((p.in_f, p.out_f))
            twice(lambda: n.call('rovit_kan_prepare', n.ptr(d.W.t), n.ptr(d.lw.t), n.ptr(wt.t), n.ptr(lwt.t), p.in_f, p.out_f, p.nk - 4, n.stream_ptr()),
                  [d.W, d.lw], [wt, lwt])
            assert torch.equal(wt.t, d.W.t.permute(0, 2, 1)) and torch.equal(lwt.t, d.lw.t.t()), 'rovit_kan_prepare is not the transposition'
            prep.append((wt, lwt))
        scratch += list(prep[-1])
    for b in scratch:
        b.bits0 = b.bits()
    inputs = [x] + [b for d in ds for b in d.bufs()] + scratch
    if mfma:
        fn = lambda: n.call('rovit_kan_stack_fwd_mfma', n.ptr(x.t), n.ptr_array([q[0].t for q in prep]), n.ptr_array([d.knots.t for d in ds]),
                            n.ptr_array([d.lb.t for d in ds]), n.ptr_array([o.t for o in outs]), batch, ints(dims), ints(nks), ints(acts), len(ds),
                            n.stream_ptr())
    else:
        fn = lambda: n.call('rovit_kan_stack_fwd', n.ptr(x.t), n.ptr_array([q[0].t for q in prep]), n.ptr_array([d.knots.t for d in ds]),
                            n.ptr_array([q[1].t for q in prep]), n.ptr_array([d.lb.t for d in ds]), n.ptr_array([o.t for o in outs]), batch,
                            ints(dims), ints(nks), ints(acts), len(ds), n.stream_ptr())
    twice(fn, inputs, outs)
    return outs


def gpu_stack_bwd(x, ds, acts, outs, gys, want_dx=True, want_dw=True):
    """gys: per layer a Buf or None.  Returns (gz list, dx or None, dW / dlw / dlb lists or None)."""
    n = _native()
    batch = x.t.shape[0]
    dims = [ds[0].p.in_f] + [d.p.out_f for d in ds]
    gz = [nan_buf((batch, d.p.out_f)) for d in ds]
    dx = nan_buf((batch, dims[0])) if want_dx else None
    dW = [nan_buf(d.p.W.shape) for d in ds] if want_dw else None
    dlw = [nan_buf(d.p.lw.shape) for d in ds] if want_dw else None
    dlb = [nan_buf(d.p.lb.shape) for d in ds] if want_dw else None
    arr = lambda bs: n.ptr_array([b.t for b in bs]) if bs is not None else None
    fn = lambda: n.call('rovit_kan_stack_bwd', n.ptr(x.t), arr([d.W for d in ds]), arr([d.knots for d in ds]), arr([d.lw for d in ds]), arr(outs),
                        n.ptr_array([g.t if g is not None else None for g in gys]), arr(gz), n.ptr(dx.t) if dx is not None else None, arr(dW), arr(dlw),
                        arr(dlb), batch, ints(dims), ints([d.p.nk for d in ds]), ints(acts), len(ds), n.stream_ptr())
    outputs = gz + ([dx] if want_dx else []) + ((dW + dlw + dlb) if want_dw else [])
    twice(fn, [x] + outs + [g for g in gys if g is not None] + [b for d in ds for b in d.bufs()], outputs)
    return gz, dx, (dW, dlw, dlb) if want_dw else None


# ------------------------------------------------------------------------------------------------------------------------------------
# bookkeeping
# ------------------------------------------------------------------------------------------------------------------------------------
class Report(dict):
    """tensor -> (largest ratio, where); `skipped` / `rows` count the hidden rows left out / judged."""

    def __init__(self):
        super().__init__()
        self.skipped = self.rows = 0

    def note(self, name, r, label):
        v, where = kc.worst(np.asarray(r))
        if name not in self or not v <= self[name][0]:
            self[name] = (v, f'{label} @ {where}')

    def bad(self):
        return {n: v for n, v in self.items() if not v[0] <= 1.0}

    def check(self):
        print('  '.join(f'{n} {v[0]:.3f} [{v[1]}]' for n, v in self.items()), f'skipped {self.skipped} of {self.rows}')
        assert self.skipped * 1000 <= max(self.rows, 1000), f'{self.skipped} of {self.rows} hidden rows skipped'
        assert not self.bad(), self.bad()


def g_for(shape, seed):
    return kc.f32(np.random.default_rng(seed).standard_normal(shape))


# ------------------------------------------------------------------------------------------------------------------------------------
# rovit_kan_basis
# ------------------------------------------------------------------------------------------------------------------------------------
def basis_case(pr, t32, rep, label):
    p = kc.selector(1, 1, pr.knots.size, 0, 0, 0, pr.knots)
    tr = kc.layer_truth(t32[:, None], p, kc.ACT_NONE, tanh=False)
    got = gpu_basis(t32, pr.knots)
    eB, _ = kc.basis_bounds(tr, tanh=False)
    rep.note('basis', kc.ratio(got, tr['B'][:, 0], eB[:, 0]), label)
    j = kc.interval(t32.astype(np.float64), pr.knots)[:, None]
    col = np.arange(pr.knots.size - 4)[None, :]
    structural_zero = (col > j) | (col < j - 3) | (j >= pr.knots.size - 4)
    return got, tr['B'][:, 0], structural_zero, eB[:, 0]


def sweep_basis_positions(name):
    """Non-zero positions: exactly zero wherever R is structurally zero (outside j-3 .. j of R's own interval j, or beyond the cutoff),
    non-zero wherever R exceeds its bound (a (1 - u)^3 of 1e-23 one ulp left of a knot is a zero in fp32)."""
    pr = PROBES[name]
    got, R, sz, eB = basis_case(pr, pr.t32, Report(), name)
    wrong = (sz & (got != 0)) | ((R > eB) & (got == 0))
    return np.argwhere(wrong)


def sweep_basis(name):
    rep = Report()
    pr = PROBES[name]
    basis_case(pr, pr.t32, rep, name)
    if name == 'uniform64':
        for n in (1, 255, 256, 257):
            basis_case(pr, pr.t32[-n:], rep, f'{name} n={n}')
    return rep


@pytest.mark.parametrize('name', list(PROBES))
def test_basis_positions(name):
    wrong = sweep_basis_positions(name)
    assert wrong.size == 0, wrong[:8]


@pytest.mark.parametrize('name', list(PROBES))
def test_basis_values(name):
    sweep_basis(name).check()


# ------------------------------------------------------------------------------------------------------------------------------------
# per-layer kernels
# ------------------------------------------------------------------------------------------------------------------------------------
LAYERS = [(8, 1, 8), (8, 3, 11), (33, 5, 16), (32, 5, 17), (192, 64, 11), (192, 64, 64), (8, 300, 11), (7, 65, 38)]


def capped_probe_rows(pr, in_f, seed, cap):
    """probe_rows cut to about `cap` rows: every probe of the cutoff knot and the special values, a stride of the rest."""
    x, either = kc.probe_rows(pr, in_f, seed)
    near = np.abs(np.tanh(pr.x.astype(np.float64)) - kc.cutoff(pr.knots)) < 200 * kc.guard(pr.knots)
    keep = near.copy()
    keep[-9:] = True
    rest = np.flatnonzero(~keep)
    keep[rest[::max(1, rest.size // max(1, cap - int(keep.sum())))]] = True
    return x[keep], either[keep]


def judge_layer(rep, label, x_np, either, d, act, y, grads=None, g_np=None, prefill=None):
    """Forward (and backward) of one layer launch against R with the either-side choice read off the forward."""
    p = d.p
    choice = None
    if either is not None and either.any():
        choice, _ = kc.choose(x_np, p, act, y.np(), either)
    tr = kc.layer_truth(x_np, p, act, choice)
    rep.note('y', kc.ratio(y.np(), tr['y'], kc.forward_bounds(tr)[1]), label)
    if grads:
        v, b = kc.backward_truth(tr, g_np, dx_prev=prefill, need_dx='dx' in grads)
        for name, buf in grads.items():
            rep.note(name + ('+' if prefill is not None and name == 'dx' else ''), kc.ratio(buf.np(), v[name], b[name]), label)
    return tr


def sweep_layer(in_f, out_f, nk, act):
    rep = Report()
    p = kc.make_layer(in_f, out_f, nk, 7)
    d = DevLayer(p)
    tb = kc.kan_tb(out_f)
    xa, ea = capped_probe_rows(PROBES[f'uniform{nk}'], in_f, 11, 96 if in_f * out_f > 4096 else 160)
    batches = [1, tb, tb + 1, xa.shape[0]] + ([1025] if (in_f, nk) == (33, 16) else [])
    for batch in batches:
        if batch <= xa.shape[0]:
            x_np, either = xa[-batch:], ea[-batch:]
        else:
            x_np = np.concatenate([xa, kc.random(batch - xa.shape[0], in_f, 13, 1.5, p.knots)])
            either = np.concatenate([ea, np.zeros((batch - xa.shape[0], in_f), dtype=bool)])
        label = f'{in_f}->{out_f} nk {nk} act {act} B {batch}'
        x = Buf(x_np.shape, x_np)
        y = gpu_layer_fwd(x, d, act)
        g_np = g_for((batch, out_f), 17)
        g = Buf(g_np.shape, g_np)
        both = gpu_layer_bwd(x, d, act, y, g)
        judge_layer(rep, label, x_np, either, d, act, y, both, g_np)
        pre = g_for((batch, in_f), 19)
        acc = gpu_layer_bwd(x, d, act, y, g, want_dw=False, prefill=pre)
        judge_layer(rep, label, x_np, either, d, act, y, acc, g_np, prefill=pre)
        only_dx = gpu_layer_bwd(x, d, act, y, g, want_dw=False)
        only_dw = gpu_layer_bwd(x, d, act, y, g, want_dx=False)
        assert torch.equal(only_dx['dx'].bits(), both['dx'].bits()), f'{label}: dx alone differs from dx with the parameter gradients'
        for name in ('dW', 'dlw', 'dlb'):
            assert torch.equal(only_dw[name].bits(), both[name].bits()), f'{label}: {name} alone differs'
    return rep


@pytest.mark.parametrize('act', kc.ACTS)
@pytest.mark.parametrize('in_f,out_f,nk', LAYERS)
def test_layer(in_f, out_f, nk, act):
    """Forward, dx (plain, accumulating, alone) and the parameter gradients (with dx, alone) at batch 1, tb, tb + 1 and over the probe rows
    (more rows than one workgroup's tile; 33 -> 5 also at 1025, beyond the 1024-thread launch)."""
    sweep_layer(in_f, out_f, nk, act).check()


def sweep_dw_chunks(in_f, out_f, nk, batches, act=kc.ACT_SIGMOID3):
    rep = Report()
    p = kc.make_layer(in_f, out_f, nk, 23)
    d = DevLayer(p)
    xa = kc.random(max(batches), in_f, 29, 1.5, p.knots)
    ga = g_for((max(batches), out_f), 31)
    for batch in batches:
        x_np, g_np = xa[:batch], ga[:batch]
        x, g = Buf(x_np.shape, x_np), Buf(g_np.shape, g_np)
        y = gpu_layer_fwd(x, d, act)
        grads = gpu_layer_bwd(x, d, act, y, g, want_dx=False)
        judge_layer(rep, f'{in_f}->{out_f} nk {nk} B {batch}', x_np, None, d, act, y, grads, g_np)
    return rep


@pytest.mark.parametrize('in_f,out_f,nk', [(192, 64, 64), (7, 65, 38)])
def test_layer_dw_batch_chunks(in_f, out_f, nk):
    """Parameter gradients at B = 1, 2, bc - 1, bc, bc + 1, 2 bc + 1 (bc = 196 and 245: the two smallest of LAYERS)."""
    bc = kc.dw_bc(out_f, nk)
    assert bc == {64: 196, 65: 245}[out_f]
    sweep_dw_chunks(in_f, out_f, nk, [1, 2, bc - 1, bc, bc + 1, 2 * bc + 1]).check()


def test_layer_dw_empty_slices():
    """8 -> 1 with 8 knots has 6 items for 256 threads: at B = 3 most sample slices of an item are empty."""
    for act in kc.ACTS:
        sweep_dw_chunks(8, 1, 8, [3], act).check()


def sweep_selector():
    """W one-hot: y is one basis value, dW that value per sample summed, dx one slope: indexing without summation."""
    rep = Report()
    for nk in (8, 11, 38, 64):
        pr = PROBES[f'uniform{nk}']
        in_f, out_f = 5, 3
        xa, ea = kc.probe_rows(pr, in_f, 37)
        xa, ea = xa[~ea.any(1)], None                   # decided rows only: a one-hot weight cannot show which side an either-side input took
        for (i, o, k) in [(0, 0, 0), (4, 2, nk - 5), (2, 1, (nk - 4) // 2), (3, 0, nk - 7)]:
            p = kc.selector(in_f, out_f, nk, i, o, k)
            d = DevLayer(p)
            x = Buf(xa.shape, xa)
            y = gpu_layer_fwd(x, d, kc.ACT_NONE)
            g_np = np.ones((xa.shape[0], out_f), dtype=np.float32)
            g = Buf(g_np.shape, g_np)
            grads = gpu_layer_bwd(x, d, kc.ACT_NONE, y, g)
            tr = judge_layer(rep, f'selector nk {nk} ({i},{o},{k})', xa, ea, d, kc.ACT_NONE, y, grads, g_np)
            eB, _ = kc.basis_bounds(tr)
            rep.note('y basis bound', kc.ratio(y.np()[:, o], tr['B'][:, i, k], eB[:, i, k]), f'selector nk {nk} ({i},{o},{k})')
            other = np.delete(y.np(), o, axis=1)
            assert not other.any(), 'an output the one-hot weight does not reach is not exactly zero'
    return rep


def test_selector():
    sweep_selector().check()


# ------------------------------------------------------------------------------------------------------------------------------------
# fused stack forward
# ------------------------------------------------------------------------------------------------------------------------------------
STACKS = {
    'default11': ([192, 64, 16, 1], 11, None), 'default38': ([192, 64, 16, 1], 38, None), 'default64': ([192, 64, 16, 1], 64, None),
    '10-1': ([10, 1], 11, None), '18-3-1': ([18, 3, 1], 11, None), '192-6-1': ([192, 6, 1], 11, None),
    '40-60-12-4': ([40, 60, 12, 4], 11, None), '17-36-20-1': ([17, 36, 20, 1], 16, None), '64x4': ([64, 64, 64, 64], 11, None),
    'mixed': ([24, 8, 64, 4], [8, 64, 11], None),
    'geometric': ([18, 8, 1], None, 'geometric'), 'first_gap': ([18, 8, 1], None, 'first_gap'), 'cut_zero': ([18, 8, 1], None, 'cut_zero'),
    'uniform_cut_zero': ([18, 8, 1], None, 'uniform_cut_zero'),
    # step 0.13, 11 knots: knots[nb] == 0.0 and the guess from inv_h0 lands in interval nb - 1 for t == 0.0, so only the walk on the stored
    # knots (ks_basis) or the comparison with the stored cutoff (km_basis) turns the basis off for an exact zero
    'zero_cut_guess': ([8, 8, 1], None, 'zero_cut_guess'),
    '8-40-8-4': ([8, 40, 8, 4], 11, None),                    # matrix-core shapes: two output tiles, the second with 8 live outputs
    '8-40-8-4 nk9': ([8, 40, 8, 4], 9, None),                 # 5 basis functions in the 8-slot instantiation: two dead slots
}


def stack_params(name, seed=41):
    dims, nks, kv = STACKS[name]
    knots = None
    if kv is not None:
        knots = kc.uniform_cut_zero() if kv == 'uniform_cut_zero' else (kc.uniform_cut_zero(11, 0.13) if kv == 'zero_cut_guess' else kc.nonuniform_knots()[kv])
        nks = knots.size
    ps = kc.make_stack(dims, nks, seed, knots)
    return ps, kc.stack_acts(len(ps))


def build_stack(name, seed=41):
    ps, acts = stack_params(name, seed)
    return ps, [DevLayer(p) for p in ps], acts


def input_seed(name):
    """The seed of a stack's layer-0 rows: the first from 43 up for which R's own fp64 trajectory has no hidden input within 100 guards of
    a cutoff (test_kan_cases_cpu.py checks it)."""
    return 44 if name == 'default38' else 43


def stack_inputs(ps, rows, seed):
    """Layer-0 rows: the probe rows of the first layer's knot vector, then random rows at scales 0.3, 1.5 and 4, then relu_zeros."""
    kn = ps[0].knots
    pr = kc.knot_probe(knots=kn)
    xa, ea = capped_probe_rows(pr, ps[0].in_f, seed, 128)
    parts = [xa] + [kc.random(24, ps[0].in_f, seed + q, s, kn) for q, s in enumerate((0.3, 1.5, 4.0))] + [kc.relu_zeros(24, ps[0].in_f, seed + 5, kn)]
    x = np.concatenate(parts)
    either = np.concatenate([ea, np.zeros((x.shape[0] - ea.shape[0], ps[0].in_f), dtype=bool)])
    if rows > x.shape[0]:
        extra = kc.f32(np.random.default_rng(seed + 9).standard_normal((rows - x.shape[0], ps[0].in_f), dtype=np.float32) * 1.5)
        fix = slice(0, 128) if extra.shape[0] > 128 else slice(None)       # the rows that end up first and last: decided, like the rest of
        extra[fix] = kc.random(extra[fix].shape[0], ps[0].in_f, seed + 10, 1.5, kn)   # what R judges (the others meet only another kernel)
        x, either = np.concatenate([extra, x]), np.concatenate([np.zeros(extra.shape, dtype=bool), either])
    return x[-rows:] if rows < x.shape[0] else x, either[-rows:] if rows < either.shape[0] else either


def judge_stack_fwd(rep, label, x_np, either, ds, acts, outs, rows=None):
    """Every layer's HBM output against R on the GPU's own previous output.  rows: an index array to restrict R to (edge rows)."""
    sel = np.arange(x_np.shape[0]) if rows is None else rows
    trs, inp, ei = [], x_np[sel], (either[sel] if either is not None else None)
    for l, d in enumerate(ds):
        y = outs[l].np()[sel]
        if l == 0:
            choice = kc.choose(inp, d.p, acts[l], y, ei)[0] if ei is not None and ei.any() else None
            tr = kc.layer_truth(inp, d.p, acts[l], choice)
            r = kc.ratio(y, tr['y'], kc.forward_bounds(tr)[1])
        else:
            skip = kc.hidden_skip(inp, d.p.knots)
            rep.skipped += int(skip.sum())
            rep.rows += int(skip.size)
            tr = kc.layer_truth(inp, d.p, acts[l])
            r = kc.ratio(y, tr['y'], kc.forward_bounds(tr)[1])[~skip]
        rep.note(f'y{l}', r, label)
        trs.append(tr)
        inp = kc.f32(y)
    return trs


def sweep_stack_fwd(name, mfma=False, batches=(1, 15, 16, 17)):
    rep = Report()
    ps, ds, acts = build_stack(name)
    xa, ea = stack_inputs(ps, 0, input_seed(name))
    for batch in list(batches) + [xa.shape[0]]:
        x_np, either = (xa[-batch:], ea[-batch:]) if batch < xa.shape[0] else (xa, ea)
        x = Buf(x_np.shape, x_np)
        outs = gpu_stack_fwd(x, ds, acts, mfma)
        judge_stack_fwd(rep, f'{name} B {x_np.shape[0]}', x_np, either, ds, acts, outs)
    return rep


@pytest.mark.parametrize('name', list(STACKS))
def test_stack_fwd(name):
    """rovit_kan_prepare + rovit_kan_stack_fwd at batch 1, 15, 16, 17 and over the probe / random / relu_zeros rows (a partial last tile)."""
    sweep_stack_fwd(name).check()


def coarse_rows_check(rep, label, ds, acts, outs, x, edge):
    """Rows R is not computed for: every layer's output against rovit_kan_layer_fwd on the same (GPU-made) input, within twice the largest
    bound R gives that output column on the edge rows (both kernels are within their bound of R there; the inputs are of one family)."""
    inp = x
    for l, d in enumerate(ds):
        ref = gpu_layer_fwd(inp, d, acts[l])
        col = 2 * edge[l].max(0)
        rep.note(f'y{l} vs layer kernel', np.abs(outs[l].np() - ref.np()) / col, label)
        inp = outs[l]


def sweep_stack_fwd_large(name, batch, mfma=False):
    rep = Report()
    ps, ds, acts = build_stack(name)
    x_np, either = stack_inputs(ps, batch, input_seed(name))
    x = Buf(x_np.shape, x_np)
    outs = gpu_stack_fwd(x, ds, acts, mfma)
    rows = np.concatenate([np.arange(64), np.arange(batch - 64, batch)])
    label = f'{name} B {batch}' + (' mfma' if mfma else '')
    trs = judge_stack_fwd(rep, label, x_np, either, ds, acts, outs, rows)
    coarse_rows_check(rep, label, ds, acts, outs, x, [kc.forward_bounds(tr)[1] for tr in trs])
    return rep


@pytest.mark.parametrize('batch', [4096, 4097])
def test_stack_fwd_large(batch):
    """The 16-sample tiles at their largest batch and the 32-sample tiles with a one-sample last tile: R on the first and last 64 rows."""
    sweep_stack_fwd_large('default11', batch).check()


# ------------------------------------------------------------------------------------------------------------------------------------
# matrix-core stack
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['default11', '8-40-8-4', '8-40-8-4 nk9', 'default38', 'zero_cut_guess'])
def test_stack_fwd_mfma(name):
    """rovit_kan_prepare_mfma + rovit_kan_stack_fwd_mfma at batch 1, 31, 32, 33, 65 and over the probe rows: the kernel without an exact
    search has to decide every decided input the reference's way."""
    sweep_stack_fwd(name, mfma=True, batches=(1, 31, 32, 33, 65)).check()


@pytest.mark.parametrize('batch', [49152, 49153])
def test_stack_fwd_mfma_two_tiles(batch):
    """38 knots from 49152 samples up: two sample tiles a wave, and its one-sample tail."""
    sweep_stack_fwd_large('default38', batch, mfma=True).check()


# ------------------------------------------------------------------------------------------------------------------------------------
# stack backward
# ------------------------------------------------------------------------------------------------------------------------------------
def judge_stack_bwd(rep, label, x_np, ds, acts, outs, gys_np, gz, dx, dws, rows=None):
    """gz[l], dx and the parameter gradients against R layer by layer: the top dL/dz from its gradient, every other from R's dx of the layer
    above GIVEN THE GPU's dL/dz there; dx and the parameter gradients of a layer from the GPU's own dL/dz.  rows: edge rows only (then the
    parameter gradients, sums over every row, are left to the bit-identity with rovit_kan_layer_bwd)."""
    L = len(ds)
    sel = np.arange(x_np.shape[0]) if rows is None else rows
    g_in, g_err = None, None
    for l in range(L - 1, -1, -1):
        inp = x_np[sel] if l == 0 else kc.f32(outs[l - 1].np()[sel])
        tr = kc.layer_truth(inp, ds[l].p, acts[l])
        skip = np.zeros(sel.size, dtype=bool) if l == 0 else kc.hidden_skip(inp, ds[l].p.knots)
        rep.skipped += int(skip.sum())
        rep.rows += int(skip.size)
        g = gys_np[l][sel] if gys_np[l] is not None else None
        if g_in is not None:
            g = g_in if g is None else g_in + g
        v, b = kc.backward_truth(tr, g, g_err=g_err, need_dx=False)         # act_grad reads the forward kernel's y: within the forward bound of R's
        rep.note(f'gz{l}', kc.ratio(gz[l].np()[sel], v['gz'], b['gz'])[~skip], label)
        v2, b2 = kc.backward_truth(tr, None, gz_given=gz[l].np()[sel], need_dx=l > 0 or dx is not None)
        if l == 0:
            if dx is not None:
                rep.note('dx', kc.ratio(dx.np()[sel], v2['dx'], b2['dx']), label)
        else:
            g_in, g_err = v2['dx'], b2['dx']
        if dws is not None and rows is None and not skip.any():
            for name, bufs in zip(('dW', 'dlw', 'dlb'), dws):
                rep.note(f'{name}{l}', kc.ratio(bufs[l].np(), v2[name], b2[name]), label)


def equal_to_layer_bwd(label, x, ds, acts, outs, gz, dx, dws):
    """Documented bit-identity: per layer, rovit_kan_layer_bwd given dL/dz (activation NONE) returns the stack's gradients bit for bit."""
    for l, d in enumerate(ds):
        inp = x if l == 0 else outs[l - 1]
        ref = gpu_layer_bwd(inp, d, kc.ACT_NONE, outs[l], gz[l], want_dx=(l == 0 and dx is not None), want_dw=dws is not None)
        if l == 0 and dx is not None:
            assert torch.equal(ref['dx'].bits(), dx.bits()), f'{label}: dx differs from rovit_kan_layer_bwd'
        if dws is not None:
            for name, bufs in zip(('dW', 'dlw', 'dlb'), dws):
                assert torch.equal(ref[name].bits(), bufs[l].bits()), f'{label}: {name} of layer {l} differs from rovit_kan_layer_bwd'


def sweep_stack_bwd(name, batch, variant='last', edge=False):
    rep = Report()
    ps, ds, acts = build_stack(name)
    x_np, _ = stack_inputs(ps, batch, input_seed(name))
    x_np = np.where(kc.classify(x_np, ps[0].knots), x_np, np.float32(0.25)).astype(np.float32)      # decided rows only: the cutoff is the forward's
    x = Buf(x_np.shape, x_np)
    outs = [None] * len(ds)
    inp = x
    for l, d in enumerate(ds):
        outs[l] = inp = gpu_layer_fwd(inp, d, acts[l])
    for o in outs:
        o.bits0 = o.bits()
    L = len(ds)
    gys_np = [g_for((batch, d.p.out_f), 59 + l) if (variant == 'all' or l == L - 1) else None for l, d in enumerate(ds)]
    gys = [Buf(g.shape, g) if g is not None else None for g in gys_np]
    gz, dx, dws = gpu_stack_bwd(x, ds, acts, outs, gys, want_dx=variant != 'no_dx', want_dw=variant != 'no_dw')
    label = f'{name} B {batch} {variant}'
    rows = np.concatenate([np.arange(min(64, batch)), np.arange(max(64, batch - 64), batch)]) if edge else None
    judge_stack_bwd(rep, label, x_np, ds, acts, outs, gys_np, gz, dx, dws, rows)
    equal_to_layer_bwd(label, x, ds, acts, outs, gz, dx, dws)
    if L > 1 and variant != 'all':
        # hidden dL/dz through the ReLU: exactly the per-layer kernel's dx where the output is positive, exactly zero elsewhere
        for l in range(1, L):
            ref = gpu_layer_bwd(outs[l - 1], ds[l], kc.ACT_NONE, outs[l], gz[l], want_dw=False)['dx']
            want = torch.where(outs[l - 1].t > 0, ref.t, torch.zeros_like(ref.t))
            assert torch.equal(want, gz[l - 1].t), f'{label}: dL/dz of layer {l - 1} is not the layer kernel dx through the ReLU'
    return rep


@pytest.mark.parametrize('variant', ['last', 'all', 'no_dx', 'no_dw'])
@pytest.mark.parametrize('name', list(STACKS))
def test_stack_bwd(name, variant):
    """rovit_kan_stack_bwd at 33 rows: one sample a workgroup; every grad_outs[l] given / only the last / dx NULL / d_spline_w NULL."""
    sweep_stack_bwd(name, 33, variant).check()


@pytest.mark.parametrize('batch', [1, 1024, 1025, 4096, 4097])
def test_stack_bwd_tiles(batch):
    """tb = 1, 4 and 16 with full and partial last tiles: R on the first and last 64 rows, bit-identity with the layer kernels everywhere."""
    sweep_stack_bwd('default11', batch, 'last', edge=True).check()


def test_stack_bwd_batch_chunks():
    """B = 2 bc + 1 = 393 for the 192 -> 64 layer at 64 knots (bc = 196): three chunks in kan_dw_body, the last of one row."""
    assert kc.dw_bc(64, 64) == 196
    sweep_stack_bwd('default64', 393, 'all').check()


# ------------------------------------------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------------------------------------------
def test_model_paths_after_a_regrid_to_a_cutoff_at_zero():
    """KANSeverityModule forward and backward on relu_zeros and random rows after a regrid to the uniform grid with knots[nb] == 0.0 (every
    zero, +0.0 or -0.0, sits on the jump, on its off side; so does every output of a hidden ReLU), through the per-layer path, the fused
    stack and with the matrix-core stack asked for -- which the module must decline: the 12-knot grid has no instantiation.  KANRegrid
    refuses the non-uniform cut_zero vector outright.  Every layer is judged against R on the GPU's own trajectory; the backward chain
    carries R's bound of the gradient it hands down."""
    from models.kan import KANSeverityModule
    from rovit_hip import RovitHipError
    torch.manual_seed(5)
    m = KANSeverityModule([24, 8, 1], num_knots=5).to(dev())
    kn = kc.uniform_cut_zero()
    x_np = np.concatenate([kc.relu_zeros(40, 24, 71, kn), kc.random(40, 24, 73, 1.5, kn)])
    xd = torch.from_numpy(x_np).to(dev())
    with pytest.raises(RovitHipError):
        m.regrid(xd, knots=torch.from_numpy(kc.nonuniform_knots()['cut_zero']))
    assert m.kan_layers[0].knots.numel() == 11
    res = m.regrid(xd, knots=torch.from_numpy(kn))
    assert res.status == 0 and all(torch.equal(l.knots.cpu(), torch.from_numpy(kn)) for l in m.kan_layers)
    ps = [kc.Params(kc.f32(l.spline_weights.detach().cpu().numpy()), kn, kc.f32(l.linear.weight.detach().cpu().numpy()),
                    kc.f32(l.linear.bias.detach().cpu().numpy()), l.in_features, l.out_features, kn.size) for l in m.kan_layers]
    acts = kc.stack_acts(2)
    g_np = g_for((80, 1), 79)
    rep = Report()
    for path in ('per-layer', 'stack', 'matrix cores asked'):
        m.fused_min_batch, m.mfma_min_batch = (1 << 30, 1 << 30) if path == 'per-layer' else (1, 1 << 30 if path == 'stack' else 1)
        if path == 'matrix cores asked':
            assert not all(p[2] is not None for p in m._prepared()), 'the matrix-core stack was not declined for a 12-knot grid'
        m.zero_grad(set_to_none=True)
        xin = xd.clone().requires_grad_(True)
        traj = m.get_activation_trajectory(xin)
        traj[-1].backward(torch.from_numpy(g_np).to(dev()))
        g, g_err = g_np, None
        for l in (1, 0):
            inp = x_np if l == 0 else kc.f32(traj[1].detach().cpu().numpy())
            tr = kc.layer_truth(inp, ps[l], acts[l])
            rep.note(f'y{l}', kc.ratio(traj[l + 1].detach().cpu().numpy(), tr['y'], kc.forward_bounds(tr)[1]), path)
            v, b = kc.backward_truth(tr, g, g_err=g_err)
            layer = m.kan_layers[l]
            for name, t in (('dW', layer.spline_weights.grad), ('dlw', layer.linear.weight.grad), ('dlb', layer.linear.bias.grad)):
                rep.note(f'{name}{l}', kc.ratio(t.cpu().numpy(), v[name], b[name]), path)
            g, g_err = v['dx'], b['dx']
        rep.note('dx', kc.ratio(xin.grad.cpu().numpy(), g, g_err), path)
    rep.check()


# ------------------------------------------------------------------------------------------------------------------------------------
# the head phase: head_phase_dw_kernel runs kan_dw_body with its own, smaller batch chunk
# ------------------------------------------------------------------------------------------------------------------------------------
def sweep_head_phase(B):
    """The KAN parameter gradients of HeadPhaseFn (rovit_head_phase_bwd -> head_phase_dw_kernel) on a 64-knot [192, 64, 16, 1] head, and
    those of rovit_kan_stack_bwd on the same activations, both against R's chain on those activations."""
    import test_gpu_head_phase as HP
    dims = (192, 64, 16, 1)
    sd, _ = HP._state(192, 128, 4, dims, 58, seed=7)
    kn = sd['kan_module.kan_layers.0.knots'].numpy()
    assert kn.size == 64 and np.array_equal(kn, kc.uniform_knots(64))
    x_np = kc.random(B, 192, 83, 1.5, kn)
    f, params, keys, outs = HP._fused(torch.from_numpy(x_np), sd, 4, dims)
    kouts = [t.detach().clone() for t in outs[4].grad_fn.saved_tensors[-3:]]
    assert [tuple(t.shape) for t in kouts] == [(B, 64), (B, 16), (B, 1)] and torch.equal(kouts[2], outs[4].detach())
    g_np = g_for((B, 1), 89)
    HP._weighted(outs, [torch.zeros_like(o) for o in outs[:4]] + [torch.from_numpy(g_np).to(dev())]).backward()
    grads = {k: p.grad for k, p in zip(keys, params)}
    ps = [kc.Params(kc.f32(sd[f'kan_module.kan_layers.{l}.spline_weights'].numpy()), kn, kc.f32(sd[f'kan_module.kan_layers.{l}.linear.weight'].numpy()),
                    kc.f32(sd[f'kan_module.kan_layers.{l}.linear.bias'].numpy()), dims[l], dims[l + 1], 64) for l in range(3)]
    ds, acts = [DevLayer(p) for p in ps], kc.stack_acts(3)
    x = Buf(x_np.shape, x_np)
    obufs = [Buf(t.shape, t.cpu().numpy()) for t in kouts]
    gz, dx, dws = gpu_stack_bwd(x, ds, acts, obufs, [None, None, Buf(g_np.shape, g_np)], want_dx=False)
    rep = Report()
    g, g_err = g_np, None
    for l in (2, 1, 0):
        inp = x_np if l == 0 else kc.f32(kouts[l - 1].cpu().numpy())
        assert l == 0 or not kc.hidden_skip(inp, kn).any()
        tr = kc.layer_truth(inp, ps[l], acts[l])
        v, b = kc.backward_truth(tr, g, g_err=g_err, need_dx=l > 0)
        names = {'dW': 'spline_weights', 'dlw': 'linear.weight', 'dlb': 'linear.bias'}
        for q, (n, key) in enumerate(names.items()):
            hp = grads[f'kan_module.kan_layers.{l}.{key}']
            rep.note(f'head phase {n}{l}', kc.ratio(hp.cpu().numpy(), v[n], b[n]), f'B {B}')
            rep.note(f'stack bwd {n}{l}', kc.ratio(dws[q][l].np(), v[n], b[n]), f'B {B}')
        if l > 0:
            g, g_err = v['dx'], b['dx']
    return rep


def test_head_phase_kan_parameter_gradients():
    """Batch bc + 1 = 58 for the widest layer (192 -> 64, 64 knots: the head phase chunks its batch by bc = 7168 / 125 = 57 rows, so
    `*p = c0 == 0 ? acc : *p + acc` takes its second branch), and batch bc = 57 (one chunk): the head phase's KAN parameter gradients and
    those of rovit_kan_stack_bwd on the same activations, each against R.  They are not compared bit for bit: the head phase derives
    dL/dz in its own per-sample kernel and keeps it in its scratch, and beyond one chunk it adds the rows 57.. as a rounded partial sum
    where the stack backward (bc = 196) continues one FMA chain."""
    assert (7 * 1024) // (60 + 1 + 64) == 57
    for B in (58, 57):
        sweep_head_phase(B).check()
