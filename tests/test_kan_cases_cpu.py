"""Everything about tests/kan_cases.py that needs no GPU: the fp64 recursion R against the fp32 oracles of oracle/ref_cpu.py, an fp32 emulation
of the kernels' basis (closed form on uniform spans, the recursion elsewhere) inside R's bounds for every input family (the bounds must be
satisfiable before a GPU sees them), the continuity statement at interior knots, the seed conditions of the stacks the GPU test runs, the
either-side bookkeeping of the probes, and the shape refusals of the entry points (they return before any launch, so the library is enough)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import kan_cases as kc
from oracle import ref_cpu

PROBES = {p.name: p for p in kc.all_probes()}
NONUNIFORM = tuple(kc.nonuniform_knots())


def _truth_basis(t32, knots):
    p = kc.selector(1, 1, knots.size, 0, 0, 0, knots)
    tr = kc.layer_truth(np.asarray(t32)[:, None], p, kc.ACT_NONE, tanh=False)
    return tr, tr['B'][:, 0]


@pytest.mark.parametrize('name', list(PROBES))
def test_recursion_against_the_fp32_oracles(name):
    """R against ref_cpu.truncated_bspline_basis (the reference's recursion in fp32) on every probe coordinate: fp32 accuracy.  The
    coordinates are fp32 values compared with fp32 knots, so every one is decided.  On the uniform grids also against closed_form_basis."""
    pr = PROBES[name]
    _, B = _truth_basis(pr.t32, pr.knots)
    ref = ref_cpu.truncated_bspline_basis(torch.from_numpy(pr.t32), torch.from_numpy(pr.knots)).numpy()
    assert np.abs(B - ref).max() < 4e-7
    assert ((B == 0) == (ref == 0)).all() or np.abs(B - ref)[(B == 0) != (ref == 0)].max() < 1e-20
    if name not in NONUNIFORM:
        j, vals = ref_cpu.closed_form_basis(torch.from_numpy(pr.t32), torch.from_numpy(pr.knots))
        dense = np.zeros_like(B)
        for m in range(4):
            ok = (j.numpy() - m >= 0) & (j.numpy() - m < B.shape[1])
            dense[np.flatnonzero(ok), (j.numpy() - m)[ok]] = vals.numpy()[ok, m]
        assert np.abs(B - dense).max() < 2e-6            # 8e-7 of it is the gap between the stored fp32 knots and a uniform grid (64 knots)


def test_storage_uniform_is_what_linspace_gives():
    for nk in range(8, 65):
        assert kc.storage_uniform(kc.uniform_knots(nk)), nk
    assert kc.storage_uniform(kc.uniform_cut_zero())
    for name, kn in kc.nonuniform_knots().items():
        assert not kc.storage_uniform(kn), name
    kn = kc.uniform_knots(11)
    assert kn[5] != 0.0 and abs(kn[5]) < 2e-8            # the linspace artefact next to every ReLU zero


@pytest.mark.parametrize('name', list(PROBES))
def test_emulation_of_the_closed_form_inside_the_bounds(name):
    """kan_basis in numpy fp32 on every probe coordinate, and a small layer (forward, dx, parameter gradients, all three activations) on the
    probe rows: inside R's bounds."""
    pr = PROBES[name]
    tr, B = _truth_basis(pr.t32, pr.knots)
    eB, _ = kc.basis_bounds(tr, tanh=False)
    bad = {}
    r = kc.worst(kc.ratio(kc.emulate_basis(pr.t32, pr.knots), B, eB[:, 0]))
    if r[0] > 1:
        bad['basis'] = r
    if name in ('uniform8', 'uniform11', 'uniform38', 'uniform64', 'uniform_cut_zero') + NONUNIFORM:
        p = kc.make_layer(6, 3, pr.knots.size, 3, pr.knots)
        x, either = kc.probe_rows(pr, 6, 5)
        g = kc.f32(np.random.default_rng(7).standard_normal((x.shape[0], 3)))
        for act in kc.ACTS:
            y, bw = kc.emulate_layer(x, p, act, g)
            choice = kc.choose(x, p, act, y, either)[0]
            t = kc.layer_truth(x, p, act, choice)
            v, b = kc.backward_truth(t, g)
            for n, got, want, bound in [('y', y, t['y'], kc.forward_bounds(t)[1])] + [(n, bw[n], v[n], b[n]) for n in v]:
                r = kc.worst(kc.ratio(got, want, bound))
                if r[0] > 1:
                    bad[f'{n} act {act}'] = r
    assert not bad, bad


@pytest.mark.parametrize('family', ['random 0.3', 'random 1.5', 'random 4', 'relu_zeros', 'selector'])
@pytest.mark.parametrize('in_f,out_f,nk', [(8, 3, 11), (33, 5, 16), (7, 65, 38), (24, 64, 64)])
def test_emulated_layer_inside_the_bounds(family, in_f, out_f, nk):
    p = kc.make_layer(in_f, out_f, nk, 11)
    if family.startswith('random'):
        x = kc.random(37, in_f, 13, float(family.split()[1]), p.knots)
    elif family == 'relu_zeros':
        x = kc.relu_zeros(37, in_f, 17, p.knots)
        assert (x == 0).mean() > 0.35 and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    else:
        p = kc.selector(in_f, out_f, nk, in_f - 1, out_f - 1, nk - 6)
        x = kc.random(37, in_f, 19, 1.5, p.knots)
    g = kc.f32(np.random.default_rng(23).standard_normal((37, out_f)))
    for act in kc.ACTS:
        y, bw = kc.emulate_layer(x, p, act, g)
        t = kc.layer_truth(x, p, act)
        v, b = kc.backward_truth(t, g)
        assert kc.worst(kc.ratio(y, t['y'], kc.forward_bounds(t)[1]))[0] <= 1
        for n in v:
            assert kc.worst(kc.ratio(bw[n], v[n], b[n]))[0] <= 1, (n, act)
    if family == 'selector':
        t = kc.layer_truth(x, p, kc.ACT_NONE)
        assert np.array_equal(t['z'][:, -1], t['B'][:, in_f - 1, nk - 6]) and not t['z'][:, :-1].any()


def test_a_wrong_closed_form_leaves_the_bounds():
    """The bounds are worth something: 5 u for 6 u in the slope of basis j - 1, a dropped d tanh, 0.3 for 1/3 in the sigmoid's slope, one
    sample missing from a parameter gradient -- each is outside the bound of the tensor it touches."""
    p = kc.make_layer(8, 3, 11, 29)
    x = kc.random(64, 8, 31, 1.5, p.knots)
    g = kc.f32(np.random.default_rng(37).standard_normal((64, 3)))
    t = kc.layer_truth(x, p, kc.ACT_SIGMOID3)
    v, b = kc.backward_truth(t, g)
    s = 1 - t['t'] ** 2
    no_dtanh = (v['dx'] - v['gz'] @ p.lw.astype(np.float64)) / np.where(s > 0, s, 1) + v['gz'] @ p.lw.astype(np.float64)
    assert kc.worst(kc.ratio(no_dtanh, v['dx'], b['dx']))[0] > 100
    y = t['y']
    assert kc.worst(kc.ratio(g * y * (1 - y * 0.3), v['gz'], b['gz']))[0] > 100
    one_less = kc.backward_truth(kc.layer_truth(x[:-1], p, kc.ACT_SIGMOID3), g[:-1])[0]['dW']
    assert kc.worst(kc.ratio(one_less, v['dW'], b['dW']))[0] > 100
    k = p.knots.astype(np.float64)
    j = kc.interval(t['t'], k)
    u = (t['t'] - k[np.minimum(j, 9)]) / (k[np.minimum(j, 9) + 1] - k[np.minimum(j, 9)])
    wrong = t['dB'].copy()
    for bb, ii in zip(*np.nonzero((j >= 1) & (j < 7))):
        wrong[bb, ii, j[bb, ii] - 1] = (-9 * u[bb, ii] ** 2 + 5 * u[bb, ii] + 3) / 6 / (k[j[bb, ii] + 1] - k[j[bb, ii]])
    _, eD = kc.basis_bounds(t)
    assert kc.worst(kc.ratio(wrong, t['dB'], eD))[0] > 100


@pytest.mark.parametrize('name', list(PROBES))
def test_continuity_at_interior_knots(name):
    """In R the left and right limits of value and first derivative agree to 1e-12 at every interior knot (the spline is C2 there); at
    the cutoff knots[nb] the value jumps (to zero)."""
    pr = PROBES[name]
    k = pr.knots.astype(np.float64)
    nb = k.size - 4
    for q in range(1, k.size - 1):
        lo, hi = np.nextafter(k[q], -np.inf), k[q]
        (Bl, dl, _), (Bh, dh, _) = kc.basis(np.array([lo]), k), kc.basis(np.array([hi]), k)
        if q == nb:
            assert np.abs(Bl - Bh).max() > 0.1 and not Bh.any()
        elif q < nb:
            scale = 1.0 / np.min(np.diff(k)) ** 2
            assert np.abs(Bl - Bh).max() <= 1e-12 and np.abs(dl - dh).max() <= 1e-12 * max(1.0, scale * 1e-3), q
        else:
            assert not Bl.any() and not Bh.any()


@pytest.mark.parametrize('name', list(PROBES))
def test_probes_decided_on_both_sides_and_either_side_count(name):
    pr = PROBES[name]
    t = np.tanh(pr.x.astype(np.float64))
    dec = ~pr.either
    cut = kc.cutoff(pr.knots)
    assert (dec & (t < cut)).sum() >= 8 and (dec & (t >= cut)).sum() >= 8
    assert int(pr.either.sum()) == pr.n_constructed            # no either-side input but the ones aimed at the cutoff
    assert 1 <= pr.n_constructed <= 11
    x, either = kc.probe_rows(pr, 5, 3)
    assert int(either.sum()) == pr.n_constructed and int(either.sum(1).max()) == 1
    # with knots[nb] == 0.0 the input 0.0 is decided, on the off side
    if cut == 0.0:
        zero = pr.x == 0
        assert zero.sum() >= 2 and dec[zero].all()
        assert not kc.basis(np.array([0.0]), pr.knots)[0].any()


def _gpu_module():
    import test_gpu_kan_rows as G
    return G


def test_seed_conditions_of_the_gpu_stacks():
    """R's own fp64 trajectory of every stack of the GPU test has no hidden input within 100 guards of its layer's cutoff, and the only
    either-side layer-0 inputs are the constructed ones."""
    G = _gpu_module()
    for name in G.STACKS:
        ps, acts = G.stack_params(name)
        for seed in (G.input_seed(name),):
            x, either = G.stack_inputs(ps, 0, seed)
            pr = kc.knot_probe(knots=ps[0].knots)
            assert int(either.sum()) <= pr.n_constructed and int((~kc.classify(x, ps[0].knots)).sum()) == int(either.sum())
            inp = np.where(either, np.float32(0.25), x).astype(np.float32)
            for l, (p, a) in enumerate(zip(ps[:-1], acts[:-1])):
                inp = kc.f32(kc.layer_truth(inp, p, a)['y'])
                nxt = ps[l + 1]
                dist = np.abs(np.tanh(inp.astype(np.float64)) - kc.cutoff(nxt.knots))
                near = (dist <= 100 * kc.guard(nxt.knots)) & (inp != 0)
                assert not near.any(), (name, seed, int(near.sum()))


# ------------------------------------------------------------------------------------------------------------------------------------
# shape refusals: every check returns before a launch, so no device is needed (the library loads without one)
# ------------------------------------------------------------------------------------------------------------------------------------
def _lib():
    """The library, built first where a fresh checkout has none; a library that does not load is a failure like any other."""
    from rovit_hip import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    native.load()
    return native


P = 0x10000          # a non-null, 16-byte aligned address no refused call may touch


def _arr(n):
    a = (C.c_void_p * n)()
    for i in range(n):
        a[i] = P
    return a


def _ints(xs):
    return (C.c_int * len(xs))(*xs)


def _refused(native, name, *args):
    from rovit_hip import RovitHipError
    with pytest.raises(RovitHipError):
        native.call(name, *args)


@pytest.mark.parametrize('nk', [7, 65])
def test_knot_counts_outside_8_64_are_refused(nk):
    n = _lib()
    _refused(n, 'rovit_kan_basis', P, P, P, 4, nk, None)
    _refused(n, 'rovit_kan_layer_fwd', P, P, P, P, P, P, 4, 8, 3, nk, 0, None)
    _refused(n, 'rovit_kan_layer_bwd', P, P, P, P, P, P, P, P, P, P, 4, 8, 3, nk, 0, 0, None)
    _refused(n, 'rovit_kan_stack_fwd', P, _arr(1), _arr(1), _arr(1), _arr(1), _arr(1), 4, _ints([8, 4]), _ints([nk]), _ints([0]), 1, None)
    _refused(n, 'rovit_kan_stack_bwd', P, _arr(1), _arr(1), _arr(1), _arr(1), _arr(1), _arr(1), P, _arr(1), _arr(1), _arr(1), 4, _ints([8, 4]),
             _ints([nk]), _ints([0]), 1, None)


def test_stack_shapes_that_are_refused():
    n = _lib()
    fwd = lambda dims, nks: _refused(n, 'rovit_kan_stack_fwd', P, _arr(len(nks)), _arr(len(nks)), _arr(len(nks)), _arr(len(nks)), _arr(len(nks)), 4,
                                     _ints(dims), _ints(nks), _ints([0] * len(nks)), len(nks), None)
    bwd = lambda dims, nks: _refused(n, 'rovit_kan_stack_bwd', P, *[_arr(len(nks))] * 6, P, *[_arr(len(nks))] * 3, 4, _ints(dims), _ints(nks),
                                     _ints([0] * len(nks)), len(nks), None)
    for f in (fwd, bwd):
        f([64, 64, 64, 64, 64, 1], [11] * 5)                 # 5 layers
        f([192, 65, 1], [11, 11])                            # hidden width 65
    fwd([192, 10, 1], [11, 11])                              # 10 outputs over KS_G = 8 threads: neither a multiple of 4 nor below 8
    fwd([192, 14, 1], [11, 11])
    fwd([192, 64, 9], [11, 11])


def test_matrix_core_shapes_that_are_refused():
    n = _lib()
    lib = n.load()
    assert lib.rovit_kan_mfma_prepared_floats(192, 64, 7) == 192 * 4 * 2 * 64 and lib.rovit_kan_mfma_prepared_floats(192, 16, 34) == 192 * 18 * 64
    # the two instantiated slot counts, 8 and 36, hold 4 .. 7 and 32 .. 35 basis functions plus the linear term: 8 .. 11 and 36 .. 39 knots
    for nb in range(4, 61):
        assert (lib.rovit_kan_mfma_prepared_floats(192, 64, nb) != 0) == (nb in (4, 5, 6, 7, 32, 33, 34, 35)), nb
    assert lib.rovit_kan_mfma_prepared_floats(12, 64, 7) == 0 and lib.rovit_kan_mfma_prepared_floats(8, 65, 7) == 0
    _refused(n, 'rovit_kan_prepare_mfma', P, P, P, 12, 64, 7, None)          # a width that is no multiple of 8
    _refused(n, 'rovit_kan_prepare_mfma', P, P, P, 192, 64, 12, None)        # 16 knots
    _refused(n, 'rovit_kan_stack_fwd_mfma', P, _arr(1), _arr(1), _arr(1), _arr(1), 4, _ints([12, 4]), _ints([11]), _ints([0]), 1, None)
    _refused(n, 'rovit_kan_stack_fwd_mfma', P, _arr(1), _arr(1), _arr(1), _arr(1), 4, _ints([8, 4]), _ints([16]), _ints([0]), 1, None)
    _refused(n, 'rovit_kan_stack_fwd_mfma', P, _arr(2), _arr(2), _arr(2), _arr(2), 4, _ints([8, 8, 4]), _ints([11, 38]), _ints([0, 0]), 2, None)
