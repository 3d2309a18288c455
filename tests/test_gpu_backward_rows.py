"""GPU tests of every token row of every block of the bf16 backbone BACKWARD, inside the schedule training uses (rovit_vit_backward with its
two streams, rotating buffers, merged weight-gradient launches and class-token forms), against fp64 on the CPU.

The backward is cut into single-block ranges (engine.backward_ranges) and a range hook clones the block's backward buffers through
rovit_hip.taps.workspace_view (include/rovit_hip.h: rovit_vit_workspace_field) before a later block reuses them.  Every stage of every block
is then recomputed in fp64 from the engine's own inputs to that stage -- its saved forward fields and its incoming gradient buffer -- twice:
R on the fp32 master weights, E with the kernels' roundings (tests/backward_rows.py lists them and holds the references, the bounds and the
comparators; tests/test_backward_rows_cpu.py shows that the comparators reject what they should).  Checked per row: gelu' and lse (saved by
the forward, read only by the backward), dpre, dx_mid, dO, the three thirds of dqkv, dx_out, the last block's class-token forms and the
final-norm backward; per element: every parameter gradient and the image gradient, as exact sums of the engine's own bf16 buffers with a
derived fp32 accumulation bound.  Every case also requires the cut run's gradients to equal an uncut run's bit for bit.

Depth 6 reaches every code form: block 5 is the class-token form, blocks 4 and 3 wait for the weight-gradient stream in front of the MLP
launch, blocks 2, 1 and 0 in front of the attention backward (both parities), block 0 takes the unfused qkv dgrad.  Batch 1 (197 rows) is less
than one 240-row workgroup, 3 (591 rows) no multiple of 16, 17 (3 349 rows) uses both half-batch forward chains.

The schedule tests at the end need no CPU reference: depth 12, the uncut two-stream backward against twelve single-block ranges, bit for
bit, up to batches at which the two streams overlap.

Measured on MI355X, worst ratio to the bound over CASES (DESIGN.md section 2 has the rows): dact 0.95; lse 5.1e-6 absolute; against E / R:
dpre 0.41 / 0.35, dx_mid 0.59 / 0.54, dO 0.66 / 0.54, dx_out 0.57 / 0.35, the last block's dx_in 0.62; dqkv against R 0.49 / 0.50 / 0.49 (q / k / v),
with E-to-R row distances of 3.5e-3 / 2.1e-2 / 3.9e-3 (peaked softmax: 1.0e-1 / 5.8e-1 / 1.1e-2); parameter gradients at most 0.21 (the last
block's class-token fc1 weight), x.grad 5.6e-3."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import backward_rows as br  # noqa: E402

DEPTH = 6
FWD = ('xhat1', 'rstd1', 'qkv', 'lse', 'attn_o', 'xhat2', 'rstd2', 'act', 'dact')
BWD = ('dx_in', 'dx_mid', 'dO', 'dx_out', 'dpre', 'dqkv')


def dev():
    return torch.device('cuda:0')


def _mlp(path):
    from rovit_hip import native
    return {None: None, 'one': native.MLP_ONE_LAUNCH, 'two': native.MLP_TWO_LAUNCH}[path]


def _backbone(sd, depth):
    from models.backbone import DeiTTiny
    m = DeiTTiny(depth=depth)
    m.load_state_dict(sd, strict=True)
    return m.to(dev())


def _field_ids():
    from rovit_hip import taps
    return {'xhat1': taps.WS_XHAT1, 'rstd1': taps.WS_RSTD1, 'qkv': taps.WS_QKV, 'lse': taps.WS_LSE, 'attn_o': taps.WS_ATTN_O,
            'xhat2': taps.WS_XHAT2, 'rstd2': taps.WS_RSTD2, 'act': taps.WS_ACT, 'dact': taps.WS_DACT, 'dx_in': taps.WS_DX_IN,
            'dx_mid': taps.WS_DX_MID, 'dO': taps.WS_DO, 'dx_out': taps.WS_DX_OUT, 'dpre': taps.WS_DPRE, 'dqkv': taps.WS_DQKV}


def _host(name, t):
    t = t.double().cpu()
    return t.reshape(-1) if name in ('rstd1', 'rstd2') else t


def _step(m, x, w, path, ranges, want_dx, capture=None):
    """One forward + backward of (features * w).sum() with fresh gradients.  capture: a dict that receives every block's forward fields
    (cloned before the backward) and, through a range hook, its backward fields (cloned right behind the block's range).  Returns
    ({parameter name: gradient}, the image gradient or None), clones."""
    from rovit_hip import taps
    eng = m.engine
    depth = eng.depth
    ids = _field_ids()
    saved = (eng.mlp_path, eng.backward_ranges, eng.range_hook)

    def hook(engine, first, last, ordered):
        assert first == last and not ordered
        ws, B, p = engine.last_ws
        capture['bwd'][first] = {n: taps.workspace_view(ws, B, depth, ids[n], first, p).clone() for n in BWD}

    try:
        eng.mlp_path, eng.backward_ranges, eng.range_hook = path, ranges, (hook if capture is not None else None)
        for prm in m.parameters():
            prm.grad = None                                   # the hook runs on the "fresh" path only
        xi = x.to(dev()).requires_grad_(want_dx)
        feats = m(xi)
        if capture is not None:
            ws, B, p = eng.last_ws
            capture['fwd'] = [{n: _host(n, taps.workspace_view(ws, B, depth, ids[n], i, p)) for n in FWD} for i in range(depth)]
            capture['xhat_cls'] = taps.workspace_view(ws, B, depth, taps.WS_XHAT_CLS, 0, p).double().cpu()
            capture['rstd_cls'] = taps.workspace_view(ws, B, depth, taps.WS_RSTD_CLS, 0, p).double().cpu().reshape(-1)
            capture['bwd'] = [None] * depth
        (feats * w.to(dev())).sum().backward()
        torch.cuda.synchronize()
        grads = {n: prm.grad.detach().clone() for n, prm in m.named_parameters()}
        dx = xi.grad.detach().clone() if want_dx else None
    finally:
        eng.mlp_path, eng.backward_ranges, eng.range_hook = saved
    return grads, dx


@functools.lru_cache(maxsize=1)
def _case(B, path, peaked, want_dx):
    """The engine's cut run of one case as a `run` of backward_rows, and the gradients of the uncut run of the same inputs; shared by the
    tests, never modified (one case is kept: a batch-17 run is 0.7 GB of fp64 rows on the host)."""
    sd = br.vit_sd(DEPTH, seed=100 + B, peaked=peaked)
    x, w = br.images(B, seed=B), br.loss_weights(B, seed=7 + B)
    m = _backbone(sd, DEPTH)
    cap = {}
    cut = [(i, i) for i in range(DEPTH - 1, -1, -1)]
    g_cut, dx_cut = _step(m, x, w, _mlp(path), cut, want_dx, cap)
    assert all(b is not None for b in cap['bwd']), 'the range hook did not run for every block'
    g_whole, dx_whole = _step(m, x, w, _mlp(path), None, want_dx)
    run = {'depth': DEPTH, 'B': B, 'fwd': cap['fwd'], 'bwd': [{n: _host(n, t) for n, t in b.items()} for b in cap['bwd']],
           'xhat_cls': cap['xhat_cls'], 'rstd_cls': cap['rstd_cls'], 'dfeat': w.double(),
           'grads': {n: g.double().cpu() for n, g in g_cut.items()}, 'xgrad': dx_cut.double().cpu() if want_dx else None}
    return sd, x, run, (g_cut, dx_cut), (g_whole, dx_whole)


CASES = [  # batch, mlp path, peaked weights, images require grad
    (1, 'two', False, False), (1, 'one', False, False),
    (3, 'two', False, True), (3, 'one', False, True),
    (17, 'two', False, False), (17, 'one', False, False),
    (3, 'two', True, False), (3, 'one', True, False),
]


@pytest.mark.parametrize('B,path,peaked,want_dx', CASES,
                         ids=[f'b{b}-{p}{"-peaked" if k else ""}{"-dx" if d else ""}' for b, p, k, d in CASES])
def test_backward_every_row_of_every_block(B, path, peaked, want_dx):
    sd, x, run, (g_cut, dx_cut), (g_whole, dx_whole) = _case(B, path, peaked, want_dx)
    report, fails = br.check_run(run, sd, x, f'backward d{DEPTH} b{B} {path}{" peaked" if peaked else ""}')      # (prints every figure)
    if peaked:
        med = float(torch.cat([br.attention(f['qkv'], B)[2] for f in run['fwd']]).median())
        print(f'median softmax row max {med:.3f}')
        assert med >= 0.3, med
    # the tie to the path training uses: the cut run IS the uncut run
    for n in g_cut:
        assert bool(torch.isfinite(g_cut[n]).all()), n
        assert torch.equal(g_cut[n], g_whole[n]), n
    if want_dx:
        assert bool(torch.isfinite(dx_cut).all()) and float(dx_cut.abs().max()) > 0
        assert torch.equal(dx_cut, dx_whole)
    assert not fails, fails
    assert sum(k.endswith(' vs R') for k in report) == 8 and sum(k.endswith(' vs E') for k in report) == 5
    assert sum(k.startswith('grad ') for k in report) == 12 + 6 + int(want_dx)


def test_comparators_reject_one_bad_row_of_the_engines_own_output():
    """Every dgrad tensor of every block, gelu' and lse, as the engine wrote them, with one element of one patch row (class-token rows: one
    image's) moved by 5 % of that row's scale; a weight gradient and the pos_embed gradient with one token row's share changed."""
    B = 3
    sd, x, run, _, _ = _case(B, 'one', False, True)
    for i in range(DEPTH):
        for st in br.block_stages(run, sd, i):
            r = br.ROWS + 100 if st.got.shape[0] > B else 1
            bad = st.got.clone()
            bad[r, bad.shape[1] // 2] += 0.05 * float(br.row_scale(st.R)[r])
            rE, rR, _ = br.stage_ratios(st, bad)
            assert float(rR[r]) > 1.0 and (rE is None or float(rE[r]) > 1.0), (st.name, i, float(rR[r]))
        f = run['fwd'][i]
        r = br.ROWS + 100 if f['dact'].shape[0] > B else 1
        bad = f['dact'].clone()
        bad[r, 384] += 0.05 * float(f['dact'][r].abs().max())
        assert float(br.dact_ratio(run, sd, i, bad)[r].max()) > 1.0, i
        bad = f['lse'].clone()
        bad[1, 1, 0] *= 1.05
        assert float(br.lse_error(run, i, bad).max()) > br.LSE_TOL, i
    refs = br.grad_refs(run, sd, x)
    r = br.ROWS + 100
    b2 = run['bwd'][2]
    for key, dy, a in (('blocks.2.mlp.fc2.weight', b2['dx_in'], run['fwd'][2]['act']), ('blocks.2.attn.proj.weight', b2['dx_mid'], run['fwd'][2]['attn_o'])):
        ref, bound = refs[key]
        assert br.worst_of(br.grad_ratio(run['grads'][key], ref, bound))[0] <= 1.0, key
        assert br.worst_of(br.grad_ratio(run['grads'][key] - torch.outer(dy[r], a[r]), ref, bound))[0] > 1.0, key
    ref, bound = refs['pos_embed']
    bad = run['grads']['pos_embed'].clone()
    bad[0, [17, 18]] = bad[0, [18, 17]]
    assert br.worst_of(br.grad_ratio(bad, ref, bound))[0] > 1.0


# ---- the schedule, without a CPU reference ----------------------------------------------------------------------------------------

def _schedule_inputs(B, depth=12):
    sd = br.vit_sd(depth, seed=900 + B)
    g = torch.Generator(device=dev()).manual_seed(B)
    x = torch.randn(B, 3, 224, 224, device=dev(), generator=g)
    w = torch.randn(B, br.D, device=dev(), generator=g)
    return _backbone(sd, depth), x, w


def _same_bits(a, b):
    for n in a:
        assert bool(torch.isfinite(a[n]).all()), n
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize('B,path', [(32, 'two'), (32, 'one'), (172, None), (173, None)], ids=['b32-two', 'b32-one', 'b172-auto', 'b173-auto'])
def test_depth_12_uncut_backward_equals_twelve_single_block_ranges(B, path):
    """Depth 12: blocks 10 and 9 wait early, blocks 8 .. 0 late; batch 172 / 173 are the two sides of MLP_AUTO's one-launch switch, with
    launches long enough for the dgrad and the weight-gradient stream to overlap."""
    m, x, w = _schedule_inputs(B)
    whole, _ = _step(m, x, w, _mlp(path), None, False)
    cut, _ = _step(m, x, w, _mlp(path), [(i, i) for i in range(11, -1, -1)], False)
    _same_bits(whole, cut)


def test_depth_12_uncut_backward_repeats_its_bits_at_batch_173():
    m, x, w = _schedule_inputs(173)
    first, _ = _step(m, x, w, None, None, False)
    second, _ = _step(m, x, w, None, None, False)
    _same_bits(first, second)
