"""GPU tests of the KAN edge statistics (csrc/kan_stats.hip, rovit_hip/kan_stats.py): per-layer parity with the fp64 host restatement on the
kernel's own inputs, bit-reproducibility, the absence of hidden synchronisation, ``KANLayer.activation_curves`` and the model methods.

Parity.  The oracle block is built in fp64 from the GPU's own trajectory (``get_activation_trajectory``, fp32), so every layer is compared on
the very rows the kernel read.  The spline jumps at the cutoff and an input whose tanh is within rounding of a knot can land in the
neighbouring interval: an entry is AMBIGUOUS when the interval of fp32(tanh64(x)) moved down 4 ulp differs from that moved up 4 ulp.  The
oracle is evaluated with the ambiguous entries in the lower and in the upper interval; the GPU value must lie inside that envelope widened
by the float bound.  Interval counts must be equal, except that for input i they may differ by at most twice its ambiguous rows in total.
Condition, asserted: ambiguous entries are at most 1e-4 of a layer's entries -- counted over the random rows.  Row 0 is planted: 30, -30,
0 and the cutoff sit on knots on purpose (tanh(+-30) = +-1 = the end knots, the cutoff is knots[num_basis]) and are ambiguous by
construction, and what the 30s feed into the later layers saturates there too (tanh == 1: intervals nk - 2 and nk - 1, both dead).  Row 0
takes part in every other check: the envelope, the interval counts, the bounds.  At N = 1 the planted row is the only one, so the share
has nothing to count there and is not asserted; every other check runs.  Only at the cutoff does the spline jump, so only there
could a mixed assignment leave an all-low / all-high envelope: the entries ambiguous AT THE CUTOFF (at most 6, asserted) are therefore
evaluated in every combination of sides, the others all low and all high.

Float bounds (derived, the same at every N): tanhf within 2 ulp moves the interval coordinate u by at most 2.4e-7 / h (4.4e-6 at the
32-knot spacing h = 2 / 37); basis values have slope at most 3/4; the four-term fp32 sum adds about 6 * 2^-24 of its terms' magnitudes;
fp32 partial sums of at most 16 rows add 16 * 2^-24 ~ 1e-6.  With scale_ij = sum_k |spline_weights[i,j,k]| + |w_ji| max_n |a_ni| that is
about 4e-6 scale_ij per value: mean, l1, spline_l1 within 2e-5 scale_ij; var within 4e-5 scale_ij^2; pre_mean within 2e-5 sum_i scale_ij;
pre_var within 4e-5 (sum_i scale_ij)^2.  The measured maxima are printed (DESIGN.md records them)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_cpu  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu

CLASS_NAMES = ["Healthy Leaf", "Leaf Holes", "Black Spot", "Dry Leaf"]
SEVERITY = {n: i for i, n in enumerate(CLASS_NAMES)}
KEYS = ('spline_weights', 'knots', 'linear.weight', 'linear.bias')


def dev():
    return torch.device('cuda:0')


def _kan(layers, num_knots, seed):
    from models.kan import KANSeverityModule
    g = torch.Generator().manual_seed(seed)
    sd = ref_cpu.init_kan_state(layers, num_knots, 3, g)
    m = KANSeverityModule(layers, num_knots, 3)
    m.load_state_dict(sd)
    params = [{k: sd[f'kan_layers.{l}.{k}'].numpy() for k in KEYS} for l in range(len(layers) - 1)]
    return m.to(dev()).eval(), sd, params, g


def _features(n, width, sd, g):
    x = torch.randn(n, width, generator=g) * 1.5
    x[0, :4] = torch.tensor([30.0, -30.0, 0.0, ref_cpu.kan_cutoff(sd['kan_layers.0.knots'])])
    return x


def _feed(acc, x, sizes):
    i, k = 0, 0
    while i < x.shape[0]:
        acc.update(x[i:i + sizes[k % len(sizes)]])
        i += sizes[k % len(sizes)]
        k += 1


def _interval_of_fp32(xn32, knots):
    k = knots.astype(np.float64)
    xc = np.clip(xn32.astype(np.float64), k[0], k[-1])
    return np.clip(np.searchsorted(k, xc, side='right') - 1, 0, len(k) - 1)


def _shift_ulps(v32, ulps):
    out = v32.copy()
    for _ in range(abs(ulps)):
        out = np.nextafter(out, np.float32(np.inf if ulps > 0 else -np.inf), dtype=np.float32)
    return out


@pytest.mark.parametrize('n', [1, 37, 4096, 16384])
@pytest.mark.parametrize('layers,num_knots', [([192, 64, 16, 1], 5), ([384, 64, 16, 1], 5), ([192, 64, 16, 1], 32), ([7, 3, 1], 5)])
def test_parity_per_layer_on_identical_inputs(layers, num_knots, n):
    from rovit_hip import kan_stats as ks
    from rovit_hip import native as N
    m, sd, params, g = _kan(layers, num_knots, seed=1000 * len(layers) + num_knots + layers[0])
    x = _features(n, layers[0], sd, g).to(dev())
    acc = ks.KANEdgeStats(m, capacity=64)
    _feed(acc, x, (4096,))
    got = acc.compute()
    with torch.no_grad():
        traj = [t.cpu().numpy() for t in m.get_activation_trajectory(x)]
    shapes = acc.shapes()
    worst = {}
    for l, (a, p, s) in enumerate(zip(traj[:-1], params, got)):
        in_f, out_f, nk = shapes[l]
        assert a.shape == (n, in_f) and s['n'] == n
        xn32 = np.tanh(a.astype(np.float64)).astype(np.float32)
        t_lo, t_hi = _interval_of_fp32(_shift_ulps(xn32, -4), p['knots']), _interval_of_fp32(_shift_ulps(xn32, 4), p['knots'])
        amb = t_lo != t_hi
        random_amb = int(amb[1:].sum())                      # row 0 is the planted one, in every layer
        print(f'{layers} G={num_knots} N={n} layer {l}: {int(amb.sum())} ambiguous entries ({random_amb} in the random rows), '
              f'at most {int(amb.sum(0).max())} per input')
        if n > 1:
            share = random_amb / amb[1:].size
            print(f'  layer {l}: ambiguous share of the random rows {share:.2e} (condition 1e-4)')
            assert share <= 1e-4
        else:                                                # N = 1 is the planted row alone: the condition has no random entry to count
            assert amb[1:].size == 0
        # Envelope.  At an interior knot the two neighbouring cubic pieces agree to rounding, so for those entries all-low and all-high
        # span every mixed assignment up to rounding.  At the cutoff knot (intervals nb - 1 | nb) the spline JUMPS: every combination of
        # sides of the cutoff-ambiguous entries is evaluated.  The sums are additive over rows, so the rows without an ambiguous entry
        # are evaluated once and only the few ambiguous rows per combination.
        nb = nk - 4
        at_cut = amb & (t_lo < nb) & (t_hi >= nb)
        cut_idx = np.argwhere(at_cut)
        print(f'  layer {l}: {len(cut_idx)} ambiguous entries at the cutoff, {int(at_cut[1:].sum())} of them in the random rows')
        assert len(cut_idx) <= 6
        base = ks.knot_intervals(a, p['knots'])
        assert np.array_equal(base[~amb], t_lo[~amb])
        amb_rows = amb.any(1)
        o = N.kan_stats_offsets(*shapes[l])
        rest = ks.layer_section_from_arrays(a[~amb_rows], p) if (~amb_rows).any() else np.zeros(o['words'], dtype=np.int64)
        env = []
        for side in (t_lo, t_hi):
            for combo in range(1 << len(cut_idx)):
                t = np.where(amb, side, base)
                for b, (r, c) in enumerate(cut_idx):
                    t[r, c] = t_hi[r, c] if (combo >> b) & 1 else t_lo[r, c]
                sec = ks.layer_section_from_arrays(a[amb_rows], p, t[amb_rows]) if amb_rows.any() else np.zeros(o['words'], dtype=np.int64)
                tot_sec = rest + sec                               # the integer words add as integers ...
                tot_sec[:o['occupancy']] = (rest[:o['occupancy']].view(np.float64) + sec[:o['occupancy']].view(np.float64)).view(np.int64)   # ... the fp64 ones as fp64
                env.append(ks.stats_from_block(tot_sec, [shapes[l]])[0])
        # interval counts
        occ_base = np.stack([np.bincount(base[:, i], minlength=nk) for i in range(in_f)])
        assert np.array_equal(s['occupancy'].sum(1), np.full(in_f, n))
        diff = np.abs(s['occupancy'] - occ_base).sum(1)
        assert (diff <= 2 * amb.sum(0)).all(), (l, diff.max())
        # floats inside the envelope widened by the derived bounds
        scale = np.abs(p['spline_weights']).sum(2).astype(np.float64) + np.abs(p['linear.weight'].T).astype(np.float64) * np.abs(a).max(0)[:, None].astype(np.float64)
        tot = scale.sum(0)
        for key, unit, bound in (('mean', scale, 2e-5), ('l1', scale, 2e-5), ('spline_l1', scale, 2e-5), ('var', scale ** 2, 4e-5),
                                 ('pre_mean', tot, 2e-5), ('pre_var', tot ** 2, 4e-5)):
            lo, hi = np.min([e[key] for e in env], axis=0), np.max([e[key] for e in env], axis=0)
            out = np.maximum(np.maximum(lo - s[key], s[key] - hi), 0.0) / unit
            worst[key] = max(worst.get(key, 0.0), float(out.max()))
            print(f'  layer {l} {key}: max distance from the envelope {float(out.max()):.3e} of its unit (bound {bound:.0e})')
            assert float(out.max()) <= bound, (l, key, float(out.max()))
        # the linear term's share is exact arithmetic on sum |a_i|: fp64 sums of fp32 values in another order
        assert np.abs(s['linear_l1'] - env[0]['linear_l1']).max() <= 1e-12 * max(1.0, float(np.abs(env[0]['linear_l1']).max()))
        assert np.abs(s['mean_abs_input'] - env[0]['mean_abs_input']).max() <= 1e-12 * max(1.0, float(np.abs(a).max()))
    print(f'{layers} G={num_knots} N={n} worst: ' + ', '.join(f'{k} {v:.3e}' for k, v in worst.items()))


def test_result_buffer_is_bit_reproducible_and_independent_of_the_update_split():
    from rovit_hip.kan_stats import KANEdgeStats
    for layers, num_knots, n in (([192, 64, 16, 1], 5, 5003), ([192, 64, 16, 1], 32, 2500), ([7, 3, 1], 5, 300)):
        m, sd, _, g = _kan(layers, num_knots, seed=5)
        x = _features(n, layers[0], sd, g).to(dev())
        blocks = []
        for sizes, cap in (((n,), 8192), ((n,), 8192), ((n,), 8192), ((1, 7, 256, 1000), 16), ((32,), 4096)):
            acc = KANEdgeStats(m, capacity=cap)
            _feed(acc, x, sizes)
            blocks.append(acc.result_block().tobytes())
        assert blocks[0] == blocks[1] == blocks[2], 'three runs of the same rows differ'
        assert blocks[0] == blocks[3] == blocks[4], 'the result buffer depends on how the rows were split into update() calls'


def test_update_never_synchronises_and_compute_copies_once(monkeypatch):
    from rovit_hip import native as N
    from rovit_hip.kan_stats import KANEdgeStats
    m, sd, _, g = _kan([192, 64, 16, 1], 5, seed=2)
    x = _features(6000, 192, sd, g).to(dev())
    acc = KANEdgeStats(m, capacity=32)
    _feed(acc, x, (3000,))                                 # warm: allocator pools, code objects, the module's prepared weights
    acc.result_block()
    acc.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        _feed(acc, x, (64, 1, 300))                        # growth by doubling inside
        with pytest.raises(RuntimeError):                  # compute() is where the pass synchronises
            acc.compute()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    copies = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: (copies.append(tuple(self.shape)), real(self, *a, **k))[1])
    stats = acc.compute()
    monkeypatch.undo()
    words = sum(N.kan_stats_offsets(*s)['words'] for s in acc.shapes())
    assert copies == [(words,)], copies                    # one device-to-host copy: the result buffer
    assert stats[0]['n'] == 6000 and np.isfinite(stats[0]['mean']).all()


@pytest.mark.parametrize('num_knots', [5, 32])
def test_activation_curves_equal_plot_activation(num_knots):
    m, sd, _, g = _kan([192, 64, 16, 1], num_knots, seed=11)
    layer = m.kan_layers[0]
    xs, ys = layer.activation_curves()
    assert xs.shape == (100,) and ys.shape == (192, 64, 100) and ys.dtype == np.float32
    rng = np.random.default_rng(0)
    for i, j in zip(rng.integers(0, 192, 20), rng.integers(0, 64, 20)):
        px, py = layer.plot_activation(int(i), int(j))
        assert np.array_equal(px, xs) and np.abs(py - ys[i, j]).max() <= 1e-6, (i, j)
    xs2, ys2 = layer.activation_curves(num_points=33, include_linear=True)
    _, ys0 = layer.activation_curves(num_points=33)
    assert ys2.shape == (192, 64, 33)
    lw = sd['kan_layers.0.linear.weight'].numpy()
    assert np.abs(ys2 - (ys0 + lw.T[:, :, None] * xs2[None, None, :])).max() <= 1e-6
    xs3, ys3 = m.kan_layers[2].activation_curves(num_points=7)
    assert ys3.shape == (16, 1, 7) and np.abs(ys3[5, 0] - m.kan_layers[2].plot_activation(5, 0, 7)[1]).max() <= 1e-6


def _full_model(seed):
    from models.rovit_kan import RoViTKAN
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(ref_cpu.init_rovit_state(seed=seed), strict=True)
    return m.to(dev()).eval()


def test_model_methods_end_to_end():
    from data.dataset import DeviceBatchLoader, create_dataloaders
    from data.transforms import original_transforms
    from explainability import KANVisualizer
    from rovit_hip import RovitHipError
    from rovit_hip.kan_stats import KANEdgeStats
    model = _full_model(23)
    images = torch.randn(40, 3, 224, 224, generator=torch.Generator().manual_seed(4)).to(dev())
    got = model.kan_edge_stats(images, chunk=16)
    acc = KANEdgeStats(model.kan_module)
    with torch.no_grad():
        for r0 in range(0, 40, 16):
            acc.update(model.backbone(images[r0:r0 + 16]))
    want = acc.compute()
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), k           # bit for bit
    att = model.kan_attribution(images, chunk=16)
    assert [tuple(v.shape) for v in att['node_scores'][:3]] == [(192,), (64,), (16,)] and att['feature_scores'].shape == (192,)
    for v in att['node_scores'] + att['edge_scores']:
        assert np.isfinite(v).all() and (v >= 0).all()
    assert [tuple(v.shape) for v in att['edge_scores']] == [(192, 64), (64, 16), (16, 1)]
    assert att['stats'][0]['n'] == 40 and 0.0 <= att['stats'][0]['dead_share'] <= 1.0
    # a loader of (images, class labels, severity labels) batches
    _, _, test_loader = create_dataloaders('data/Augmented Image', 'data/Original Image', CLASS_NAMES, SEVERITY,
                                           original_transform=original_transforms(), batch_size=8, synthetic=96, seed=7, device=dev())
    assert isinstance(test_loader, DeviceBatchLoader)
    from_loader = model.kan_edge_stats(test_loader)
    assert from_loader[0]['n'] == sum(b[0].shape[0] for b in test_loader) and np.isfinite(from_loader[0]['var']).all()
    viz = KANVisualizer().edge_attribution(model, test_loader)
    assert np.array_equal(viz['feature_scores'], model.kan_attribution(test_loader)['feature_scores'])
    for fn in (model.kan_edge_stats, model.kan_attribution):
        with pytest.raises(RovitHipError):
            fn(torch.randn(2, 3, 224, 224))


def test_visualizer_data_methods():
    from explainability import KANVisualizer
    m, sd, _, g = _kan([192, 64, 16, 1], 5, seed=3)
    v = KANVisualizer()
    curves = v.spline_activations(m, num_samples=5)
    assert [c['y'].shape for c in curves] == [(5, 100), (5, 100), (1, 100)] and curves[0]['edges'] == [(i, i) for i in range(5)]
    assert np.abs(curves[1]['y'][3] - m.kan_layers[1].plot_activation(3, 3)[1]).max() <= 1e-6
    x = _features(50, 192, sd, g).to(dev())
    tr = v.severity_trajectory(m, x, torch.arange(50) % 4)
    assert len(tr['mean_activations']) == 4 and tr['mean_activations'][0].shape == (50,) and tr['labels'].shape == (50,)
    assert np.allclose(tr['mean_activations'][0], x.mean(dim=1).cpu().numpy(), atol=1e-6)
    assert [h.shape for h in v.spline_weights_heatmap(m)] == [(192, 64), (64, 16), (16, 1)]
