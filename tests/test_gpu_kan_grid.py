"""GPU tests of the KAN grid extension (csrc/kan_grid.hip, rovit_hip/kan_grid.py).  Oracle: ``regrid_reference`` (numpy fp64, pinned on
the CPU in tests/test_kan_grid_cpu.py).  Cases, conditioned inputs and the moment bounds with their derivation: tests/kan_grid_cases.py.

Inputs are generated on the CPU with no tanh(x) within 1e-4 of either grid's cutoff ``knots[nb]`` (offenders moved, not dropped); at the
interior knots the neighbouring cubic pieces agree to rounding, so the kernel's interval decisions are those of the fp64 tanh up to
rounding and no row is left out of any comparison.

Bounds.  Moments: 4x the fp32-numpy deviation (kan_grid_cases.moment_bounds).  Solve, from the kernel's own moments: c' within 2^-22
max|c'| (fp32 storage; the fp64 solve error at a condition of at most 1e8 is about 1e-8); fit_ms / target_ms within 1e-6 of the largest
target_ms (a 1e-8 relative move of c' changes the quadratic forms by at most 4e-8 of it).  Forward paths after ``apply``: the tolerances
of tests/test_gpu_round2.py for each path (1e-4 per-layer / VALU stack / matrix-core stack against the oracle, 1e-3 head phase, 5e-4
relative for the backward).  The measured maxima are printed (DESIGN.md records them)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kan_grid_cases as cases  # noqa: E402
from kan_grid_cases import ref_cpu  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def _module(layers, num_knots, seed):
    from models.kan import KANSeverityModule
    sd, g = cases.head_state(layers, num_knots, seed)
    m = KANSeverityModule(list(layers), num_knots, 3)
    m.load_state_dict(sd)
    return m.to(dev()).eval(), sd, g


def _priors(new, old, eps=1e-2):
    from rovit_hip import kan_grid as kg
    pri = kg.prior_moments(new, old)
    s = eps / pri['L']
    return torch.from_numpy(np.ascontiguousarray(pri['G'] * s)).to(dev()), torch.from_numpy(np.ascontiguousarray(pri['M'] * s)).to(dev())


@pytest.mark.parametrize('n', cases.ROWS)
@pytest.mark.parametrize('name', list(cases.TRANSITIONS))
def test_moments_and_solve_against_the_reference(name, n):
    from rovit_hip import kan_grid as kg
    from rovit_hip import native as N
    old, new = cases.old_knots(name), cases.new_knots(name)
    bounds = cases.moment_bounds(name)
    kn_old, kn_new = torch.from_numpy(old).to(dev()), torch.from_numpy(new).to(dev())
    pg, pm = _priors(new, old)
    worst = {'G': 0.0, 'M': 0.0, 'O': 0.0, 'c': 0.0, 'ms': 0.0}
    for s, l, in_f in cases.moment_layers():
        out_f = cases.SHAPES[s][l + 1]
        x, want = cases.moment_case(name, n, s, l)
        blk = kg.device_moments(x.to(dev()), kn_old, kn_new)
        mom = kg.moments_from_block(blk.cpu().numpy(), in_f, old.size, new.size)
        assert np.array_equal(mom['rows'], np.full(in_f, n)) and not mom['nonfinite'].any()
        got = cases.mean_moments(mom)
        for k in ('G', 'M', 'O'):
            err = float(np.abs(got[k] - want[k]).max())
            worst[k] = max(worst[k], err)
            assert err <= bounds[k], (name, n, s, l, k, err, bounds[k])
        # the solve, from the kernel's own moments
        c = (torch.randn(in_f, out_f, old.size - 4, generator=torch.Generator().manual_seed(n + l)) * 0.1)
        diag = torch.empty(N.kan_regrid_diag_offsets(in_f, out_f)['words'], dtype=torch.int64, device=dev())
        w_new = kg.device_solve(blk, pg, pm, c.to(dev()), new.size, diag)
        ref = kg.solve_moments(mom, c.numpy(), new, old)
        d = kg.diagnostics_from_block(diag.cpu().numpy(), in_f, out_f)
        assert ref['status'] == 0 and d['status'] == 0
        scale = float(np.abs(ref['spline_weights']).max())
        err = float(np.abs(w_new.double().cpu().numpy() - ref['spline_weights']).max()) / scale
        worst['c'] = max(worst['c'], err)
        assert err <= 2.0 ** -22, (name, n, s, l, err)
        tscale = float(ref['target_ms'].max())
        blkd = diag.cpu().numpy().view(np.float64)
        e = in_f * out_f
        ms_err = max(float(np.abs(blkd[:e].reshape(in_f, out_f) - ref['fit_ms']).max()), float(np.abs(blkd[e:2 * e].reshape(in_f, out_f) - ref['target_ms']).max()))
        worst['ms'] = max(worst['ms'], ms_err / tscale)
        assert ms_err <= 1e-6 * tscale, (name, n, s, l, ms_err, tscale)
        assert np.array_equal(d['rows'], mom['rows']) and np.array_equal(d['nonfinite'], mom['nonfinite'])
        assert np.abs(d['pivot_ratio'] - ref['pivot_ratio']).max() <= 1e-6 * ref['pivot_ratio'].max()
    print(f'{name} N={n}: moments max-abs distance G {worst["G"]:.3e} (bound {bounds["G"]:.3e}), M {worst["M"]:.3e} ({bounds["M"]:.3e}), '
          f'O {worst["O"]:.3e} ({bounds["O"]:.3e}); c\' {worst["c"]:.3e} of max|c\'| (bound {2.0 ** -22:.3e}); ms {worst["ms"]:.3e} of max target_ms')


@pytest.mark.parametrize('layers', cases.SHAPES)
def test_halved_step_reproduces_the_curves_on_the_device(layers):
    from rovit_hip import kan_grid as kg
    m, sd, g = _module(layers, 5, 17)
    old, new = cases.old_knots('5_to_halved'), cases.HALVED
    x = cases.layer_inputs(1000, layers[0], 0, 23, (old, new))
    xs, before = m.kan_layers[0].activation_curves()
    res = m.regrid(x.to(dev()), knots=torch.from_numpy(new), layers=[0])
    assert res.status == 0 and m.kan_layers[0].knots.numel() == 18
    _, after = m.kan_layers[0].activation_curves()
    # the yardstick: the same chain in fp32 numpy (fp32 moments, c' stored as fp32, the curve evaluated in fp32) against the fp64 old curve
    c = sd['kan_layers.0.spline_weights'].numpy()
    x64 = np.tanh(x.numpy().astype(np.float64))
    m32 = kg.data_moments(x.numpy(), old, new, kg.intervals_v(x64, old.astype(np.float64)), kg.intervals_v(x64, new.astype(np.float64)), dtype=np.float32)
    c32 = kg.solve_moments(m32, c, new, old)['spline_weights'].astype(np.float32)
    curve32 = np.einsum('pk,ijk->ijp', kg.basis_v(xs, new, dtype=np.float32), c32)
    curve64 = np.einsum('pk,ijk->ijp', kg.basis_v(xs.astype(np.float64), old), c.astype(np.float64))
    bound = 4.0 * float(np.abs(curve32.astype(np.float64) - curve64).max())
    err = float(np.abs(after.astype(np.float64) - before.astype(np.float64)).max())
    print(f'{layers}: halved step, max curve distance {err:.3e} (bound {bound:.3e}); largest fit_rms {float(res.layers[0]["diagnostics"]["fit_rms"].max()):.3e}')
    assert err <= bound


@pytest.mark.parametrize('name', list(cases.TRANSITIONS))
@pytest.mark.parametrize('layers', cases.SHAPES)
def test_every_forward_path_agrees_with_the_oracle_after_apply(layers, name):
    from rovit_hip import native as N
    G, kw = cases.TRANSITIONS[name]
    m, sd, g = _module(layers, G, 29)
    x = cases.layer_inputs(1000, layers[0], 0, 31, (cases.old_knots(name), cases.new_knots(name)))
    x[0, :3] = torch.tensor([30.0, -30.0, 0.0])
    res = m.regrid(x.to(dev()), **kw)
    assert res.status == 0
    new_sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    assert all(new_sd[f'kan_layers.{l}.knots'].numel() == cases.new_knots(name).size for l in range(len(layers) - 1))
    want = ref_cpu.kan_module_forward(x, new_sd)
    xd = x.to(dev())
    with torch.no_grad():
        m.fused_min_batch, m.mfma_min_batch = 1 << 30, 1 << 30
        per_layer = m(xd)
        m.fused_min_batch = 1
        valu = m(xd)
        paths = {'per-layer': per_layer, 'VALU stack': valu}
        if all(p[2] is not None for p in m._prepared()):
            m.mfma_min_batch = 1
            paths['matrix-core stack'] = m(xd)
        else:
            # the matrix-core stack is instantiated for 7 and 34 basis functions and input widths that are multiples of 8 only
            # (rovit_kan_mfma_prepared_floats is 0 otherwise, whatever the grid): the module then keeps to the VALU stack
            lib = N.load()
            assert any(lib.rovit_kan_mfma_prepared_floats(l.in_features, l.out_features, l.num_basis) == 0 for l in m.kan_layers)
            assert name != '5_to_5_cover' or layers[0] % 8
    for k, y in paths.items():
        err = float((y.cpu() - want).abs().max())
        print(f'{layers} {name} {k}: max distance from the oracle {err:.3e} (bound 1e-4)')
        assert torch.isfinite(y).all() and err < 1e-4, (k, err)


def test_backward_after_a_regrid_against_fp64_autograd():
    m, sd, g = _module((7, 3, 1), 5, 37)
    x = cases.layer_inputs(64, 7, 0, 41, (cases.old_knots('5_to_58'), cases.new_knots('5_to_58')))
    m.regrid(x.to(dev()), num_knots=12)
    m.train()
    xd = x.to(dev()).requires_grad_(True)
    m(xd).sum().backward()
    rp = {k: (v.detach().cpu().double().requires_grad_('knots' not in k)) for k, v in m.state_dict().items()}
    xr = x.double().requires_grad_(True)
    ref_cpu.kan_module_forward(xr, rp).sum().backward()
    for k, p in m.named_parameters():
        rel = float((p.grad.cpu().double() - rp[k].grad).abs().max()) / float(rp[k].grad.abs().max() + 1e-6)
        print(f'backward after regrid {k}: {rel:.3e} of the largest gradient (bound 5e-4)')
        assert rel < 5e-4, (k, rel)
    assert float((xd.grad.cpu().double() - xr.grad).abs().max()) < 5e-4 * float(xr.grad.abs().max())


def _full_model(seed):
    from models.rovit_kan import RoViTKAN
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(ref_cpu.init_rovit_state(seed=seed), strict=True)
    return m.to(dev()).eval()


@pytest.mark.parametrize('num_knots', [5, 58])
def test_head_phase_path_after_a_model_regrid(num_knots):
    model = _full_model(43)
    images = torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(47)).to(dev())
    res = model.kan_regrid(images, chunk=4, num_knots=num_knots)
    assert res.status == 0 and model.kan_module.num_knots == num_knots and (res.layers[0]['diagnostics']['rows'] == 8).all()
    with torch.no_grad():
        out = model(images)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    err = float((out['kan_severity'].cpu() - ref_cpu.kan_module_forward(out['features'].cpu(), sd, 'kan_module.')).abs().max())
    print(f'head phase after a regrid to {num_knots} knots: max distance from the oracle {err:.3e} (bound 1e-3)')
    assert err < 1e-3


def test_no_dead_interval_after_a_cover_regrid():
    from rovit_hip.kan_stats import KANEdgeStats
    m, sd, g = _module((192, 64, 16, 1), 5, 53)
    x = torch.randn(1000, 192, generator=g) * 1.5
    x[0, :3] = torch.tensor([30.0, -30.0, 0.0])
    xd = x.to(dev())
    acc = KANEdgeStats(m)
    acc.update(xd)
    assert acc.compute()[0]['dead_share'] > 0.25
    m.regrid(xd)
    acc = KANEdgeStats(m)
    acc.update(xd)
    for s in acc.compute():
        nb = s['occupancy'].shape[1] - 4
        assert int(s['occupancy'][:, nb:].sum()) == 0 and int(s['occupancy'].sum()) == 1000 * s['occupancy'].shape[0]


def test_results_are_bit_identical_across_runs_and_update_splits():
    from rovit_hip.kan_grid import KANRegrid
    for layers, G, kw in (((192, 64, 16, 1), 5, {'num_knots': 12}), ((7, 3, 1), 32, {'num_knots': 16})):
        m, sd, g = _module(layers, G, 59)
        x = (torch.randn(1000, layers[0], generator=g) * 1.5).to(dev())
        runs = []
        for sizes in ((1000,), (1, 7, 256, 300, 100, 255, 81), (1000,)):
            acc = KANRegrid(m, capacity=16)
            i = 0
            for b in sizes:
                acc.update(x[i:i + b])
                i += b
            assert i == 1000 and acc.n == 1000
            res = acc.fit(**kw)
            runs.append(b''.join(r['moments'].cpu().numpy().tobytes() + r['spline_weights'].cpu().numpy().tobytes() +
                                 b''.join(np.ascontiguousarray(r['diagnostics'][k]).tobytes() for k in ('fit_rms', 'target_rms', 'pivot_ratio', 'rows'))
                                 for r in res.layers))
        assert runs[0] == runs[2], 'two runs of the same rows differ'
        assert runs[0] == runs[1], 'the result depends on how the rows were split into update() calls'


def test_update_never_synchronises_and_fit_copies_once(monkeypatch):
    from rovit_hip import native as N
    from rovit_hip.kan_grid import KANRegrid
    m, sd, g = _module((192, 64, 16, 1), 5, 83)
    x = (torch.randn(3000, 192, generator=g) * 1.5).to(dev())
    acc = KANRegrid(m, capacity=32)
    acc.update(x)                                          # warm: allocator pools, code objects
    acc.fit(num_knots=12)
    acc.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        i = 0
        for b in (64, 1, 300, 2635):                       # growth by doubling inside
            acc.update(x[i:i + b])
            i += b
    finally:
        torch.cuda.set_sync_debug_mode('default')
    copies = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: (copies.append(tuple(self.shape)), real(self, *a, **k))[1])
    res = acc.fit(num_knots=12)
    monkeypatch.undo()
    words = sum(N.kan_regrid_diag_offsets(l.in_features, l.out_features)['words'] for l in m.kan_layers)
    assert copies == [(words,)], copies                    # one device-to-host copy: the diagnostics of all layers
    assert res.status == 0 and (res.layers[0]['diagnostics']['rows'] == 3000).all()


def test_edge_inputs_nonfinite_rows_and_the_empty_column():
    from rovit_hip import RovitHipError
    from rovit_hip import kan_grid as kg
    from rovit_hip.kan_stats import KANEdgeStats
    m, sd, g = _module((7, 3, 1), 5, 61)
    old, new = cases.old_knots('5_to_5_cover'), kg.make_grid(12).numpy()
    x = torch.randn(300, 7, generator=g)
    x[0, :3] = torch.tensor([30.0, -30.0, 0.0])
    x[1, :] = torch.from_numpy(np.arctanh(np.clip(new[3:10].astype(np.float64), -0.999999, 0.999999)).astype(np.float32))   # tanh on (or within rounding of) new knots
    x[2, :] = torch.from_numpy(np.arctanh(old[2:9].astype(np.float64).clip(-0.999999, 0.999999)).astype(np.float32))       # ... and old ones
    bad = x.clone()
    bad[:, 2] = float('nan')
    bad[5, 4], bad[6, 4], bad[7, 0] = float('inf'), float('-inf'), float('nan')
    with pytest.raises(RovitHipError, match='different|on cuda|rows on'):
        acc = kg.KANRegrid(m)
        acc.update(bad)                                               # rows on the CPU, the module on the GPU
        acc.fit(num_knots=12)
    acc = kg.KANRegrid(m)
    acc.update(bad.to(dev()))
    res = acc.fit(num_knots=12, layers=[0])
    d = res.layers[0]['diagnostics']
    assert d['rows'].tolist() == [299, 300, 0, 300, 298, 300, 300] and d['nonfinite'].tolist() == [1, 0, 300, 0, 2, 0, 0] and d['status'] == 0
    w = res.layers[0]['spline_weights'].double().cpu().numpy()
    assert np.isfinite(w).all() and np.isfinite(d['fit_rms']).all() and (d['fit_rms'][2] == 0).all() and (d['target_rms'][2] == 0).all()
    c = sd['kan_layers.0.spline_weights'].numpy().astype(np.float64)
    pri = kg.prior_moments(new, old)
    T = np.linalg.solve(pri['G'], pri['M'])                            # the empty column: the prior alone
    assert float(np.abs(w[2] - c[2] @ T.T).max()) <= 2.0 ** -22 * float(np.abs(w).max())
    # finite and live: the edge rows alone, refitted and pushed through every layer
    edge = x[:3].to(dev())
    m.regrid(x.to(dev()), num_knots=12)
    with torch.no_grad():
        assert torch.isfinite(m(edge)).all()
    st = KANEdgeStats(m)
    st.update(edge)
    for s in st.compute():
        nb = s['occupancy'].shape[1] - 4
        assert int(s['occupancy'][:, nb:].sum()) == 0


def test_training_after_a_regrid_needs_a_fresh_optimizer():
    from rovit_hip import RovitHipError
    from rovit_hip.losses import JointLoss
    from rovit_hip.optim import RoViTAdamW
    torch.manual_seed(67)
    model = _full_model(71).train()
    model.curriculum_stage = 4
    stale = RoViTAdamW(model, lr=1e-3)
    images = torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(73)).to(dev())
    cls_t, sev_t = torch.randint(0, 4, (8,), device=dev()), torch.randint(0, 4, (8,), device=dev())
    model.kan_regrid(images, num_knots=12)
    assert model.training and getattr(model, '_head_grad_views', None) is None
    opt = RoViTAdamW(model, lr=1e-3)
    before = [l.spline_weights.detach().clone() for l in model.kan_module.kan_layers]
    assert all(tuple(b.shape)[2] == 14 for b in before)
    loss_fn = JointLoss(1.0, 0.5, 0.5, 2.0)
    opt.zero_grad()
    loss = loss_fn(model(images), cls_t, sev_t, 4)['total_loss']
    loss.backward()
    opt.step()
    assert np.isfinite(float(loss.detach()))
    for l, b in zip(model.kan_module.kan_layers, before):
        assert tuple(l.spline_weights.shape) == tuple(b.shape) and not torch.equal(l.spline_weights.detach(), b)
    with pytest.raises(RovitHipError, match='regridded'):
        stale.step()
