"""CPU tests of the KAN edge statistics (rovit_hip/kan_stats.py, explainability/kan_viz.py): the fp64 host restatement against a brute-force
double loop over edges on the reference-pinned basis (oracle.ref_cpu.truncated_bspline_basis), the identities the statistics obey, pykan's
attribution rule on hand-made statistics, ``KANEdgeStats`` on CPU tensors, the descriptor checks of rovit_kan_edge_stats, and the drop-in
``KANVisualizer``.

Bound of the float comparisons, 1e-12 relative to the edge's scale: both sides are fp64 sums of at most 64 terms (2^-52 * 64 ~ 1.4e-14 of
the terms' magnitudes); the closed form and the Cox-de Boor recursion differ by a few ulp of fp64 per basis value."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu

TOL = 1e-12


@pytest.fixture(scope='module')
def native():
    from rovit_hip import native as n
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    n.load()
    return n


def _state(layers, num_knots, seed):
    g = torch.Generator().manual_seed(seed)
    sd = ref_cpu.init_kan_state(layers, num_knots, 3, g)
    params = [{k: sd[f'kan_layers.{l}.{k}'].numpy() for k in ('spline_weights', 'knots', 'linear.weight', 'linear.bias')}
              for l in range(len(layers) - 1)]
    x = torch.randn(64, layers[0], generator=g) * 1.5
    x[0, :min(4, layers[0])] = torch.tensor([30.0, -30.0, 0.0, ref_cpu.kan_cutoff(sd['kan_layers.0.knots'])])[:min(4, layers[0])]
    return sd, params, x


def _brute_force_section(x, p):
    """Double loop over the edges, fp64, the reference's own (truncated Cox-de Boor) basis."""
    x64 = torch.from_numpy(np.asarray(x)).double()
    knots = torch.from_numpy(p['knots']).double()
    B = ref_cpu.truncated_bspline_basis(torch.tanh(x64), knots).numpy()           # (N, in, nb)
    W, lw, lb = p['spline_weights'].astype(np.float64), p['linear.weight'].astype(np.float64), p['linear.bias'].astype(np.float64)
    in_f, out_f, _ = W.shape
    n = x64.shape[0]
    sums = np.zeros((5, in_f, out_f))
    z = np.tile(lb, (n, 1))
    xa = x64.numpy()
    for i in range(in_f):
        for j in range(out_f):
            s = B[:, i, :] @ W[i, j]
            phi = lw[j, i] * xa[:, i] + s
            sums[:, i, j] = [phi.sum(), (phi * phi).sum(), np.abs(phi).sum(), np.abs(s).sum(), abs(lw[j, i]) * np.abs(xa[:, i]).sum()]
            z[:, j] += phi
    k = knots.numpy()
    xc = np.clip(np.tanh(xa), k[0], k[-1])
    occ = np.zeros((in_f, len(k)), dtype=np.int64)
    for t in range(len(k)):
        hi = k[t + 1] if t + 1 < len(k) else np.inf
        occ[:, t] = ((xc >= k[t]) & (xc < hi)).sum(0)
    return sums, z.sum(0), (z * z).sum(0), np.abs(xa).sum(0), occ


@pytest.mark.parametrize('layers,num_knots', [([7, 3, 1], 5), ([7, 3, 1], 32), ([192, 64, 16, 1], 5), ([192, 64, 16, 1], 32)])
def test_restatement_against_brute_force(native, layers, num_knots):
    from rovit_hip import kan_stats as ks
    sd, params, x = _state(layers, num_knots, seed=len(layers) * 100 + num_knots)
    inputs = [t.numpy() for t in ref_cpu.kan_module_layer_inputs(x, sd)]
    blk = ks.edge_stats_block_from_arrays(inputs, params)
    at = 0
    for l, (a, p) in enumerate(zip(inputs, params)):
        in_f, out_f, nb = p['spline_weights'].shape
        o = native.kan_stats_offsets(in_f, out_f, nb + 4)
        assert o['words'] == native.load().rovit_kan_stats_words(in_f, out_f, nb + 4)
        sec = blk[at:at + o['words']]
        at += o['words']
        f = sec.view(np.float64)
        sums, sz, szz, sabs, occ = _brute_force_section(a, p)
        scale = np.abs(p['spline_weights']).sum(2).astype(np.float64) + np.abs(p['linear.weight'].T).astype(np.float64) * np.abs(a).max(0)[:, None]
        got = f[:5 * in_f * out_f].reshape(5, in_f, out_f)
        n = a.shape[0]
        for q, pw in enumerate((1, 2, 1, 1, 1)):
            err = float((np.abs(got[q] - sums[q]) / (n * scale ** pw)).max())
            assert err <= TOL, (l, q, err)
        tot = scale.sum(0)
        assert float((np.abs(f[o['pre']:o['pre'] + out_f] - sz) / (n * tot)).max()) <= TOL
        assert float((np.abs(f[o['pre'] + out_f:o['pre'] + 2 * out_f] - szz) / (n * tot ** 2)).max()) <= TOL
        assert float(np.abs(f[o['abs_in']:o['abs_in'] + in_f] - sabs).max()) <= TOL * n * max(1.0, float(np.abs(a).max()))
        assert np.array_equal(sec[o['occupancy']:o['occupancy'] + in_f * (nb + 4)].reshape(in_f, nb + 4), occ)
        assert int(sec[o['nonfinite']]) == 0 and int(sec[o['n']]) == n
    assert at == len(blk)


@pytest.mark.parametrize('num_knots', [5, 32])
def test_identities(native, num_knots):
    from rovit_hip import kan_stats as ks
    layers = [7, 3, 1]
    sd, params, x = _state(layers, num_knots, seed=3)
    x[1, 0], x[1, 1] = 30.0, -30.0
    inputs = [t.numpy() for t in ref_cpu.kan_module_layer_inputs(x, sd)]
    shapes = [(p['spline_weights'].shape[0], p['spline_weights'].shape[1], len(p['knots'])) for p in params]
    stats = ks.stats_from_block(ks.edge_stats_block_from_arrays(inputs, params), shapes)
    for l, (a, p, s) in enumerate(zip(inputs, params, stats)):
        n, nk = a.shape[0], len(p['knots'])
        assert s['n'] == n
        assert np.abs(p['linear.bias'].astype(np.float64) + s['mean'].sum(0) - s['pre_mean']).max() <= TOL * max(1.0, np.abs(s['pre_mean']).max())
        assert np.array_equal(s['occupancy'].sum(1), np.full(a.shape[1], n))
        cut = ref_cpu.kan_cutoff(torch.from_numpy(p['knots']))
        assert np.array_equal(s['dead_share_per_input'], (a.astype(np.float64) >= cut).mean(0))
        assert s['dead_share'] == float((a.astype(np.float64) >= cut).mean())
        assert (s['var'] >= 0).all() and (s['l1'] >= np.abs(s['mean']) - 1e-15).all()
        assert ((s['spline_share'] >= 0) & (s['spline_share'] <= 1)).all()
    # a column of +30 only / -30 only: last / first interval; the spline is dead at +30, and at -30 basis 0 is at its zero end (u = 0)
    a = np.zeros((5, 7), dtype=np.float32)
    a[:, 0], a[:, 1] = 30.0, -30.0
    s = ks.stats_from_block(ks.layer_section_from_arrays(a, params[0]), shapes[:1])[0]
    nk = shapes[0][2]
    assert s['occupancy'][0, nk - 1] == 5 and s['occupancy'][0].sum() == 5
    assert s['occupancy'][1, 0] == 5 and s['occupancy'][1].sum() == 5
    assert (s['spline_l1'][0] == 0).all() and (s['spline_l1'][1] == 0).all() and s['dead_share_per_input'][0] == 1.0 and s['dead_share_per_input'][1] == 0.0
    assert (s['spline_share'][0] == 0).all()


def test_forced_intervals_evaluate_the_neighbouring_piece():
    """``basis_rows(..., intervals=)`` is what the GPU parity test builds its envelope from.  Against the uniform cubic B-spline pieces
    written out by hand: forcing an entry into the interval below evaluates that interval's four polynomials at u > 1, the interval above
    at u < 0; at an interior knot both agree with the natural piece (the spline is C2), forcing into the dead zone gives zero, and
    forcing the first dead interval's entry down revives the last live piece.  On exactly uniform fp64 knots, so that the hand-written
    uniform pieces are the same function: 1e-12."""
    from rovit_hip.kan_stats import basis_rows, knot_intervals
    knots = np.linspace(-1.0, 1.0, 11)
    nk, nb = len(knots), len(knots) - 4
    k = knots
    h = (k[-1] - k[0]) / (nk - 1)

    def by_hand(xn, t):
        out = np.zeros(nb)
        if t >= nb:
            return out
        u = (xn - (k[0] + t * h)) / h
        vals = [u ** 3 / 6, (-3 * u ** 3 + 3 * u ** 2 + 3 * u + 1) / 6, (3 * u ** 3 - 6 * u ** 2 + 4) / 6, (1 - u) ** 3 / 6]
        for m, v in enumerate(vals):
            if 0 <= t - m < nb:
                out[t - m] = v
        return out
    xn = np.array([k[3] + 1e-7, k[4] - 1e-7, 0.13, k[nb] + 1e-7, k[nb] - 1e-7, k[nb + 1] + 0.01])
    x = np.arctanh(xn)
    nat = knot_intervals(x, knots)
    assert list(nat) == [3, 3, 5, nb, nb - 1, nb + 1]
    for forced in (nat, nat - 1, nat + 1):
        got = basis_rows(x, knots, intervals=forced)
        for e in range(len(x)):
            assert np.abs(got[e] - by_hand(xn[e], int(forced[e]))).max() <= 1e-12, (e, forced[e])
    assert np.array_equal(basis_rows(x, knots), basis_rows(x, knots, intervals=nat))
    # an interior knot: the neighbouring piece continues the natural one; the cutoff: it does not
    assert np.abs(basis_rows(x[:1], knots, intervals=nat[:1] - 1) - basis_rows(x[:1], knots)).max() <= 1e-6
    assert basis_rows(x[3:4], knots).max() == 0.0 and basis_rows(x[3:4], knots, intervals=np.array([nb - 1])).max() > 0.1
    assert basis_rows(x[4:5], knots, intervals=np.array([nb])).max() == 0.0
    # the plain path is the reference's recursion
    ref = ref_cpu.truncated_bspline_basis(torch.from_numpy(xn), torch.from_numpy(k)).numpy()
    assert np.abs(basis_rows(x, knots) - ref).max() <= 1e-12


def test_attribution_rule_on_hand_made_statistics():
    from rovit_hip.kan_stats import kan_attribution
    # two layers 3 -> 2 -> 1.  Only the path input 1 -> hidden 0 -> output carries variance.
    l0 = {'var': np.array([[0., 0.], [4., 0.], [0., 0.]]), 'pre_var': np.array([4., 0.])}
    l1 = {'var': np.array([[9.], [0.]]), 'pre_var': np.array([9.])}
    a = kan_attribution([l0, l1])
    e1 = 3.0 / (3.0 + 1e-4)
    e0 = e1 * 2.0 / (2.0 + 1e-4)
    assert np.allclose(a['edge_scores'][1], [[e1], [0.0]], rtol=0, atol=1e-15)
    assert np.allclose(a['edge_scores'][0], [[0, 0], [e0, 0], [0, 0]], rtol=0, atol=1e-15)
    assert np.allclose(a['feature_scores'], [0, e0, 0], rtol=0, atol=1e-15)
    assert [tuple(n.shape) for n in a['node_scores']] == [(3,), (2,), (1,)] and a['node_scores'][2][0] == 1.0
    assert a['node_scores'][1][1] == 0.0                       # the zero-variance edge passes nothing on
    # a zero-variance OUTPUT (pre_var 0): the 1e-4 keeps the score finite and zero
    dead = kan_attribution([{'var': np.zeros((2, 1)), 'pre_var': np.zeros(1)}])
    assert np.array_equal(dead['feature_scores'], np.zeros(2))
    # two equal edges into one output share the score: each sqrt(var) / (sqrt(pre_var) + eps)
    two = kan_attribution([{'var': np.array([[1.], [1.]]), 'pre_var': np.array([2.])}])
    assert np.allclose(two['feature_scores'], 1.0 / (np.sqrt(2.0) + 1e-4), rtol=0, atol=1e-15)


def _module(layers, num_knots, sd):
    from models.kan import KANSeverityModule
    m = KANSeverityModule(layers, num_knots, 3)
    m.load_state_dict(sd)
    return m


def test_kan_edge_stats_on_cpu_tensors(native):
    from rovit_hip import RovitHipError
    from rovit_hip.kan_stats import KANEdgeStats, kan_attribution
    layers = [12, 5, 1]
    g = torch.Generator().manual_seed(8)
    sd = ref_cpu.init_kan_state(layers, 5, 3, g)
    m = _module(layers, 5, sd)
    x = torch.randn(700, 12, generator=g) * 1.5
    blocks = []
    for sizes in ((700,), (1, 7, 13, 100), (256,)):
        acc = KANEdgeStats(m, capacity=16)
        i, k = 0, 0
        while i < 700:
            acc.update(x[i:i + sizes[k % len(sizes)]])
            i += sizes[k % len(sizes)]
            k += 1
        assert acc.n == 700
        blocks.append(acc.result_block().tobytes())
    assert blocks[0] == blocks[1] == blocks[2]
    stats = acc.compute()
    assert [s['mean'].shape for s in stats] == [(12, 5), (5, 1)] and stats[0]['n'] == 700
    # the layer inputs are the oracle's trajectory
    want = ref_cpu.kan_module_layer_inputs(x, sd)
    cut = ref_cpu.kan_cutoff(sd['kan_layers.1.knots'])
    assert abs(stats[1]['dead_share'] - float((want[1] >= cut).double().mean())) <= 2.0 / want[1].numel()
    att = kan_attribution(stats)
    assert att['feature_scores'].shape == (12,) and np.isfinite(att['feature_scores']).all() and (att['feature_scores'] >= 0).all()
    acc.reset()
    assert acc.n == 0
    with pytest.raises(RovitHipError):
        acc.compute()
    acc.update(x[:3])
    assert acc.compute()[0]['n'] == 3
    bad = x[:5].clone()
    bad[2, 4] = float('nan')
    acc.reset()
    acc.update(bad)
    with pytest.raises(RovitHipError, match='non-finite'):
        acc.compute()
    with pytest.raises(RovitHipError):
        acc.update(torch.randn(3, 11))
    with pytest.raises(RovitHipError):
        KANEdgeStats(m, capacity=0)


def test_descriptor_is_checked_before_any_launch(native):
    lib = native.load()

    def desc(**kw):
        d = native.KANStats()
        d.n, d.in_f, d.out_f, d.n_knots = 64, 8, 4, 11
        for f in ('x', 'spline_w', 'knots', 'lin_w', 'lin_b', 'partials', 'result'):
            setattr(d, f, 64)           # dummy non-null aligned addresses: every call here is refused before a launch
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for kw in ({'n': 0}, {'in_f': 0}, {'out_f': 0}, {'n_knots': 65}, {'n_knots': 4}, {'x': None}, {'result': None}, {'partials': 4},
               {'n': native.KAN_STATS_MAX_ROWS + 1}):
        assert lib.rovit_kan_edge_stats(ctypes.byref(desc(**kw)), None) < 0, kw
        assert lib.rovit_last_error_string()
    assert lib.rovit_kan_edge_stats(None, None) < 0
    assert lib.rovit_kan_stats_words(192, 64, 11) == 5 * 192 * 64 + 2 * 64 + 192 + 192 * 11 + 2
    assert lib.rovit_kan_stats_words(192, 64, 65) == 0
    assert lib.rovit_kan_stats_partials_doubles(65536, 192, 64, 11) * 8 < 64 << 20       # the workspace stays small: no N x in x out
    assert lib.rovit_kan_curves(None, None, None, None, None, 4, 4, 11, 10, None) < 0


def test_kan_visualizer_drop_in(native):
    import explainability
    from explainability.kan_viz import KANVisualizer
    assert explainability.KANVisualizer is KANVisualizer
    layers = [12, 5, 1]
    sd = ref_cpu.init_kan_state(layers, 5, 3, torch.Generator().manual_seed(1))
    m = _module(layers, 5, sd)
    v = KANVisualizer()
    for name, args in (('plot_spline_activations', (m,)), ('plot_severity_trajectory', (m, None, None, [])),
                       ('plot_severity_distribution', (None, None, [])), ('plot_spline_weights_heatmap', (m,))):
        with pytest.raises(NotImplementedError):
            getattr(v, name)(*args)
    maps = v.spline_weights_heatmap(m)
    assert [h.shape for h in maps] == [(12, 5), (5, 1)]
    assert np.allclose(maps[0], sd['kan_layers.0.spline_weights'].mean(dim=2).numpy())
    out = v.edge_attribution(m, [torch.randn(40, 12), torch.randn(24, 12)])
    assert out['stats'][0]['n'] == 64 and out['feature_scores'].shape == (12,)
