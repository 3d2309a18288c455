"""CPU tests of the KAN grid extension (rovit_hip/kan_grid.py): the grids, the numpy fp64 statement of the refit (the kernels' oracle)
against exactness cases and a brute-force least squares, ``RegridResult.apply`` / ``resize_grid_like`` on a CPU module, the refusals and
the C entry points' descriptor validation (no launch).  Bounds: exactness 1e-10 max|c| (fp64 at a condition of about 1e3); the brute
force solves the same normal equations by QR, so the two agree to cond * 2^-52 * max|c'| -- 1e-7 max|c'| at the stated condition of at
most 4e6 with a factor 100 to spare."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kan_grid_cases as cases  # noqa: E402
from kan_grid_cases import ref_cpu  # noqa: E402


@pytest.fixture(scope='module')
def native():
    from rovit_hip import native as n
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return n


def _module(layers, num_knots, seed):
    from models.kan import KANSeverityModule
    sd, g = cases.head_state(layers, num_knots, seed)
    m = KANSeverityModule(list(layers), num_knots, 3)
    m.load_state_dict(sd)
    return m, sd, g


def _curve(c, knots, v):
    from rovit_hip import kan_grid as kg
    return np.einsum('pk,ijk->ijp', kg.basis_v(v, knots), np.asarray(c, dtype=np.float64))


@pytest.mark.parametrize('G', [2, 5, 12, 32, 58])
def test_make_grid_is_uniform_and_has_no_dead_row(G):
    from models.kan import KANSeverityModule
    from rovit_hip import kan_grid as kg
    from rovit_hip.kan_stats import knot_intervals
    k = kg.make_grid(G)
    assert k.dtype == torch.float32 and k.numel() == G + 6
    kg.check_grid(k)

    class L:
        knots = k
    assert KANSeverityModule._uniform_knots(KANSeverityModule.__new__(KANSeverityModule), L)
    x = np.concatenate([[0.0, 30.0, -30.0, 9.5, -9.5], torch.randn(4096, generator=torch.Generator().manual_seed(G)).numpy()]).astype(np.float32)
    assert np.tanh(np.float32(30.0)) == np.float32(1.0)
    t = knot_intervals(x, k.numpy())
    assert t.min() >= 3 and t.max() <= G + 1                         # live: below num_basis = G + 2
    # the device's coordinate is fp32: tanh rounded to fp32 lands in the same zone
    t32 = kg.intervals_v(np.tanh(x.astype(np.float64)).astype(np.float32), k.numpy())
    assert t32.min() >= 3 and t32.max() <= G + 1
    assert torch.equal(kg.make_grid(G, layout='reference'), ref_cpu.make_knots(G, 3))


@pytest.mark.parametrize('layers', cases.SHAPES)
def test_reference_is_exact_where_the_spaces_nest(layers):
    from rovit_hip import kan_grid as kg
    sd, g = cases.head_state(layers, 5, 3)
    x = torch.randn(300, layers[0], generator=g).numpy()
    c = sd['kan_layers.0.spline_weights'].numpy()
    old = -1.0 + 0.2 * np.arange(11, dtype=np.float64)                # the default grid and its halved step as exact fp64 multiples
    half = -1.0 + 0.1 * np.arange(18, dtype=np.float64)
    tol = 1e-10 * float(np.abs(c).max())
    same = kg.regrid_reference(x, old, old, c)
    print('same knots: max |c\' - c| =', float(np.abs(same['spline_weights'] - c).max()))
    assert same['status'] == 0 and float(np.abs(same['spline_weights'] - c).max()) <= tol
    fine = kg.regrid_reference(x, old, half, c)
    assert fine['spline_weights'].shape == (layers[0], layers[1], 14) and fine['status'] == 0
    v = np.linspace(-1.0, 1.0, 2001)
    v = v[np.abs(v - 0.4) > 1e-9]                                     # the cutoff itself is a jump
    err = float(np.abs(_curve(fine['spline_weights'], half, v) - _curve(c, old, v)).max())
    print('halved step: max curve distance =', err, 'condition proxy: pivot ratio', float(fine['pivot_ratio'].min()))
    assert err <= tol
    assert float(fine['fit_ms'].max()) <= tol and np.all(same['rows'] == 300) and np.all(same['nonfinite'] == 0)


def test_cover_refit_removes_the_dead_share():
    from rovit_hip import kan_grid as kg
    from rovit_hip.kan_stats import KANEdgeStats
    m, sd, g = _module((192, 64, 16, 1), 5, 11)
    x = torch.randn(4096, 192, generator=g)
    acc = KANEdgeStats(m)
    acc.update(x)
    before = acc.compute()
    assert 0.30 <= before[0]['dead_share'] <= 0.37, before[0]['dead_share']
    res = m.regrid(x)
    assert res.status == 0 and [r['layer'] for r in res.layers] == [0, 1, 2]
    acc = KANEdgeStats(m)
    acc.update(x)
    after = acc.compute()
    for s in after:
        nb = s['occupancy'].shape[1] - 4
        assert int(s['occupancy'][:, nb:].sum()) == 0 and int(s['occupancy'].sum()) == 4096 * s['occupancy'].shape[0]
    for r in res.layers:
        d = r['diagnostics']
        assert np.isfinite(d['fit_rms']).all() and np.isfinite(d['target_rms']).all() and (d['pivot_ratio'] > 0).all()
        assert (d['rows'] == 4096).all() and (d['nonfinite'] == 0).all()


@pytest.mark.parametrize('case', ['relu', 'one_row', 'nan_column'])
def test_reference_equals_brute_force_least_squares(case):
    from rovit_hip import kan_grid as kg
    sd, g = cases.head_state((7, 3, 1), 5, 5)
    c = sd['kan_layers.0.spline_weights'].numpy()
    old, new = ref_cpu.make_knots(5, 3).numpy(), kg.make_grid(12).numpy()
    x = torch.randn(400, 7, generator=g)
    if case == 'relu':
        x = torch.relu(x)
        assert float((x == 0).float().mean()) > 0.4
    elif case == 'one_row':
        x = x[:1]
    else:
        x[:, 2] = float('nan')
        x[5, 4] = float('inf')
    r = kg.regrid_reference(x.numpy(), old, new, c)
    assert r['status'] == 0 and np.isfinite(r['spline_weights']).all()
    want = cases.lstsq_refit(x.numpy(), old, new, c)
    scale = float(np.abs(want).max())
    err = float(np.abs(r['spline_weights'] - want).max())
    print(case, 'max |c\'| =', scale, 'distance from lstsq =', err, 'smallest pivot ratio =', float(r['pivot_ratio'].min()))
    assert scale <= 10.0 * float(np.abs(c).max())                    # bounded where the data leave bases unexcited
    assert err <= 1e-7 * scale
    if case == 'nan_column':
        assert r['rows'].tolist() == [400, 400, 0, 400, 399, 400, 400] and r['nonfinite'].tolist() == [0, 0, 400, 0, 1, 0, 0]
        pri = kg.prior_moments(new, old)                              # N_i = 0: the prior alone, whatever its weight
        T = np.linalg.solve(pri['G'], pri['M'])
        assert float(np.abs(r['spline_weights'][2] - c[2] @ T.T).max()) <= 1e-7 * scale


def test_apply_resize_and_checkpoint_round_trip(tmp_path):
    from evaluation.evaluator import load_model_for_evaluation
    from models.kan import KANSeverityModule
    from models.rovit_kan import RoViTKAN
    m, sd, g = _module((7, 3, 1), 5, 9)
    keys = list(m.state_dict().keys())
    old_w = m.kan_layers[0].spline_weights
    m.kan_layers[1].spline_weights.requires_grad_(False)
    lin = [l.linear.weight.clone() for l in m.kan_layers]
    res = m.regrid(torch.randn(64, 7, generator=g), num_knots=12)
    assert m.num_knots == 12 and m.__dict__['_regrid_count'] == 1 and m.fused_min_batch == 2048 and m.mfma_min_batch == 32768
    for l, layer in enumerate(m.kan_layers):
        assert layer.num_knots == 12 and layer.num_basis == 14 and layer.knots.numel() == 18
        assert tuple(layer.spline_weights.shape) == (layer.in_features, layer.out_features, 14)
        assert isinstance(layer.spline_weights, torch.nn.Parameter) and layer.spline_weights.requires_grad == (l == 0)
        assert torch.equal(layer.linear.weight, lin[l]) and torch.equal(layer.knots, res.layers[l]['knots'])
    assert m.kan_layers[0].spline_weights is not old_w and list(m.state_dict().keys()) == keys
    part = m.regrid(torch.randn(64, 7, generator=g), num_knots=20, layers=[1])
    assert [r['layer'] for r in part.layers] == [1] and m.num_knots == 12 and m.kan_layers[1].num_knots == 20
    fresh = KANSeverityModule([7, 3, 1], 5, 3)
    with pytest.raises(RuntimeError):
        fresh.load_state_dict(m.state_dict())
    fresh.resize_grid_like(m.state_dict()).load_state_dict(m.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), m.state_dict().values()))
    assert [l.num_knots for l in fresh.kan_layers] == [12, 20]
    # a whole model: regrid its head on the CPU, save, load through the evaluator's loader built from the ORIGINAL config
    model = RoViTKAN(pretrained=False)
    model._head_grad_views = {1: None}
    model.kan_module.regrid(torch.randn(32, 192, generator=g), num_knots=8, layout='cover')
    assert model._head_grad_views is None
    path = tmp_path / 'regridded.pt'
    torch.save({'model_state_dict': model.state_dict(), 'epoch': 0}, path)

    class Cfg:
        class model:
            embed_dim, hidden_dim, kan_layers, kan_num_knots, kan_degree, dropout, pretrained = 192, 128, [192, 64, 16, 1], 5, 3, 0.3, False

        class data:
            num_classes = 4
    loaded = load_model_for_evaluation(path, Cfg, torch.device('cpu'))
    assert loaded.kan_module.num_knots == 8
    assert all(torch.equal(a, b) for a, b in zip(loaded.state_dict().values(), model.state_dict().values()))


def test_refusals():
    from rovit_hip import RovitHipError
    from rovit_hip import kan_grid as kg
    m, sd, g = _module((7, 3, 1), 5, 1)
    x = torch.randn(16, 7, generator=g)
    acc = kg.KANRegrid(m)
    with pytest.raises(RovitHipError, match='nothing recorded'):
        acc.fit()
    acc.update(x)
    bent = kg.make_grid(5).clone()
    bent[4] += 0.05
    down = kg.make_grid(5).flip(0)
    for kw in ({'knots': bent}, {'knots': down}, {'num_knots': 1}, {'num_knots': 59}, {'knots': torch.linspace(-1, 1, 65)},
               {'knots': torch.linspace(-1, 1, 7)}, {'prior_weight': 0.0}, {'prior_weight': -1.0}, {'layout': 'quantile'}, {'layers': [3]},
               {'knots': [kg.make_grid(5)]}):
        with pytest.raises(RovitHipError):
            acc.fit(**kw)
    with pytest.raises(RovitHipError):
        acc.update(torch.randn(3, 11))
    with pytest.raises(RovitHipError):
        kg.KANRegrid(m, capacity=0)
    assert m.__dict__.get('_regrid_count', 0) == 0                   # nothing was installed


def test_descriptors_are_checked_before_any_launch(native):
    lib = native.load()

    def moments(**kw):
        d = native.KANRegridMoments()
        d.n, d.in_f, d.n_knots_old, d.n_knots_new = 64, 8, 11, 18
        for f in ('x', 'knots_old', 'knots_new', 'workspace', 'moments'):
            setattr(d, f, 64)           # dummy non-null aligned addresses: every call here is refused before a launch
        d.workspace_bytes = 1 << 30
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def fit(**kw):
        d = native.KANRegridFit()
        d.in_f, d.out_f, d.n_knots_old, d.n_knots_new = 8, 4, 11, 18
        for f in ('moments', 'prior_g', 'prior_m', 'spline_w', 'spline_w_new', 'diagnostics'):
            setattr(d, f, 64)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for kw in ({'n': 0}, {'in_f': 0}, {'n_knots_old': 7}, {'n_knots_old': 65}, {'n_knots_new': 7}, {'n_knots_new': 65}, {'x': None},
               {'knots_old': None}, {'knots_new': None}, {'workspace': None}, {'moments': None}, {'workspace_bytes': 8},
               {'n': native.KAN_STATS_MAX_ROWS + 1}):
        assert lib.rovit_kan_regrid_moments(ctypes.byref(moments(**kw)), None) < 0, kw
        assert lib.rovit_last_error_string()
    for kw in ({'in_f': 0}, {'out_f': 0}, {'n_knots_old': 7}, {'n_knots_new': 65}, {'moments': None}, {'prior_g': None}, {'prior_m': None},
               {'spline_w': None}, {'spline_w_new': None}, {'diagnostics': None}):
        assert lib.rovit_kan_regrid_solve(ctypes.byref(fit(**kw)), None) < 0, kw
    assert lib.rovit_kan_regrid_moments(None, None) < 0 and lib.rovit_kan_regrid_solve(None, None) < 0
    assert lib.rovit_kan_regrid_moment_words(192, 11, 18) == 192 * (4 * 14 + 14 * 7 + 4 * 7 + 2)
    assert lib.rovit_kan_regrid_moment_words(192, 11, 65) == 0 and lib.rovit_kan_regrid_workspace_bytes(0, 192, 11, 18) == 0
    assert lib.rovit_kan_regrid_diag_words(192, 64) == 2 * 192 * 64 + 3 * 192 + 1
    for n in (1, 4096, 1 << 22):                                      # the workspace is bounded whatever n is
        assert 0 < lib.rovit_kan_regrid_workspace_bytes(n, 192, 64, 64) <= (1024 + 192) * 30592
    o = native.kan_regrid_moment_offsets(192, 11, 18)
    assert o['words'] == lib.rovit_kan_regrid_moment_words(192, 11, 18)
    assert native.kan_regrid_diag_offsets(192, 64)['words'] == lib.rovit_kan_regrid_diag_words(192, 64)
