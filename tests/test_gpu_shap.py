"""GPU tests of KernelSHAP (csrc/shap.hip, rovit_hip/shap.py): rovit_shap_coalitions bit for bit against the numpy reference and
perturbation.source_rows; the Gram matrix and the fit against solve_reference within the rounding bound of the solve; run-to-run and
grid-cap bit-identity; a rank-deficient design; RoViTKAN.patch_shap against the pixel recipe, the subset-sum definition, the torch
source_rows path, and its independence of the batch and of the other targets."""
import functools

import numpy as np
import pytest
import torch

import shap_cases as cases

pytestmark = pytest.mark.gpu

from oracle import ref_cpu  # noqa: E402  (checker only)

PROB_TOL = 1.5e-2                     # softmax probability against another forward path: tests/test_gpu_perturbation.py's bound
ESTIMATOR_CASES = cases.EXACT + cases.SAMPLED + cases.MIXED + [(5, cases.UNEQUAL5_M)]


def dev():
    return torch.device('cuda:0')


def _shap():
    from rovit_hip import shap
    return shap


def _map_of(P, M):
    return cases.UNEQUAL5 if (P, M) == (5, cases.UNEQUAL5_M) else cases.patch_map_for(P)


@functools.lru_cache(maxsize=None)
def _model(seed=0):
    from models.rovit_kan import RoViTKAN
    sd = ref_cpu.init_rovit_state(seed=seed)
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(sd, strict=True)
    return m.to(dev()).eval()


def _images(B, seed):
    return torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(seed))


# ---- 1. the coalitions ---------------------------------------------------------------------------------------------------------------

def _check_coalitions(co, Z, w, pmap):
    from rovit_hip.perturbation import source_rows
    s = _shap()
    M, P = Z.shape
    assert co['bits'].dtype == torch.int32 and tuple(co['bits'].shape) == (M, 7)
    assert np.array_equal(co['bits'].cpu().numpy().view(np.uint32), s.pack_bits(Z))                # the padding bits are zero too
    assert np.array_equal(co['weights'].cpu().numpy(), w)
    absent = torch.from_numpy(~Z[:, pmap])
    assert torch.equal(co['src_replace'].cpu(), source_rows(absent, 'replace'))
    seen = []
    for tokens, idx, src in co['src_drop']:
        assert tuple(src.shape) == (len(idx), tokens) and src.dtype == torch.int32
        assert torch.equal(src.cpu(), source_rows(absent[idx.cpu()], 'drop', tokens))
        seen.append(idx.cpu().numpy())
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(M))


@pytest.mark.parametrize('P,M', ESTIMATOR_CASES)
def test_coalitions_equal_the_reference_bit_for_bit(P, M):
    s = _shap()
    pmap = _map_of(P, M)
    for seed in cases.SEEDS:
        Z, w = cases.reference(P, M, seed)
        ks = s.KernelShap(pmap, M, seed)
        _check_coalitions(ks.coalitions(dev()), Z, w, pmap)
        if seed == cases.SEEDS[1]:            # one workgroup walks every pair: the same bits
            capped = s.KernelShap(pmap, M, seed)
            capped.max_workgroups = 1
            a, b = ks.coalitions(dev()), capped.coalitions(dev())
            assert torch.equal(a['bits'], b['bits']) and torch.equal(a['weights'], b['weights']) and torch.equal(a['src_replace'], b['src_replace'])
            assert all(torch.equal(x[2], y[2]) for x, y in zip(a['src_drop'], b['src_drop']))
    if (P, M) in cases.SAMPLED:
        assert not np.array_equal(cases.reference(P, M, cases.SEEDS[0])[0], cases.reference(P, M, cases.SEEDS[1])[0])
    # an abstract game of P players has the same coalitions and no src rows
    abstract = s.KernelShap(num_players=P, num_samples=M, seed=cases.SEEDS[2]).coalitions(dev())
    assert torch.equal(abstract['bits'], ks.coalitions(dev())['bits']) and 'src_replace' not in abstract


# ---- 2. the fit --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('P,M', ESTIMATOR_CASES)
def test_solve_against_the_reference(P, M):
    """Synthetic fp32 values (B = 3, T = 2), exact in fp64: A and b are summed in the reference's own order, so the only error is the
    order of the fp64 operations of the factorisation and the solves.  Bound: 64 cond(A) 2^-53 max|y| with cond(A) < 1e7 asserted first
    (DESIGN.md section 2 records the measured distances: at most 2 % of the bound)."""
    s = _shap()
    seed = 11
    B, T = 3, 2
    Z, w = cases.reference(P, M, seed)
    vals, v0, v1 = cases.synthetic_values(Z, B, T, 1000 + P)
    ref = s.solve_reference(Z, w, vals, v0, v1)
    assert ref['cond'] < 1e7 and ref['ok']
    y = vals.astype(np.float64) - v0.astype(np.float64)
    bound = 64.0 * ref['cond'] * 2.0 ** -53 * float(np.abs(y).max())
    pmap = _map_of(P, M)
    ks = s.KernelShap(pmap, M, seed)
    tv, t0, t1 = (torch.from_numpy(a).to(dev()) for a in (vals, v0, v1))
    out = ks.solve(tv, t0, t1)
    assert torch.equal(ks.factor(dev())['gram'].cpu(), torch.from_numpy(ref['A']))                  # the same sums in the same order
    phi = out['phi'].cpu().numpy()
    err = float(np.abs(phi - ref['phi']).max())
    delta = v1.astype(np.float64) - v0.astype(np.float64)
    eff = float(np.abs(phi.sum(-1) - delta).max())
    print(f'P={P} M={M}: cond(A) {ref["cond"]:.3e}  bound {bound:.2e}  |phi - ref| {err:.2e}  |sum phi - delta| {eff:.2e}  '
          f'min pivot {float(out["min_pivot"]):.3e} (ref {ref["min_pivot"]:.3e})')
    assert err <= bound
    assert eff <= bound
    assert bool(out['ok'].all()) and out['ok'].dtype == torch.bool
    assert torch.equal(out['phi32'], out['phi'].float())
    rm = out['fit_rmse'].cpu().numpy()
    assert np.allclose(rm, ref['fit_rmse'], rtol=1e-9, atol=bound)
    assert abs(float(out['min_pivot']) - ref['min_pivot']) <= 64.0 * 2.0 ** -53 * ref['cond'] * np.abs(ref['A']).max()
    counts = np.bincount(pmap, minlength=P).astype(np.float64)
    assert np.array_equal(out['patch_map'].cpu().numpy(), (phi / counts)[..., pmap].astype(np.float32))
    # a second run, and every grid capped at one workgroup: the same bits
    again = ks.solve(tv, t0, t1)
    capped = s.KernelShap(pmap, M, seed)
    capped.max_workgroups = 1
    one = capped.solve(tv, t0, t1)
    for k in ('phi', 'phi32', 'fit_rmse', 'ok', 'patch_map', 'min_pivot'):
        assert torch.equal(out[k], again[k]) and torch.equal(out[k], one[k]), k
    assert torch.equal(ks.factor(dev())['factor'], capped.factor(dev())['factor'])
    # (M, B) values: the same numbers without the target axis
    flat = ks.solve(tv[:, :, 1].contiguous(), t0[:, 1].contiguous(), t1[:, 1].contiguous())
    assert tuple(flat['phi'].shape) == (B, P) and torch.equal(flat['phi'], out['phi'][:, 1])


def test_rank_deficient_design_gives_nan_and_not_ok_without_raising():
    s = _shap()
    Z, w = cases.rank_deficient_design()
    ks = s.KernelShap.from_design(Z, w)
    vals = torch.randn(8, 3, 2, generator=torch.Generator().manual_seed(1)).to(dev())
    out = ks.solve(vals, torch.zeros(3, 2, device=dev()), torch.ones(3, 2, device=dev()))
    assert out['ok'].is_cuda and not bool(out['ok'].any())
    assert bool(torch.isnan(out['phi']).all()) and bool(torch.isnan(out['phi32']).all()) and bool(torch.isnan(out['fit_rmse']).all())
    assert float(out['min_pivot']) <= 0.0
    # the same design made regular by one sample that separates players 0 and 1
    Z2 = np.concatenate([Z, np.array([[1, 0, 0]], dtype=bool)])
    ks2 = s.KernelShap.from_design(Z2, np.ones(9))
    vals2 = torch.cat([vals, vals[:1]])
    out2 = ks2.solve(vals2, torch.zeros(3, 2, device=dev()), torch.ones(3, 2, device=dev()))
    ref = s.solve_reference(Z2, np.ones(9), vals2.cpu().numpy(), np.zeros((3, 2)), np.ones((3, 2)))
    assert bool(out2['ok'].all()) and np.abs(out2['phi'].cpu().numpy() - ref['phi']).max() < 1e-12


# ---- 3. the model ------------------------------------------------------------------------------------------------------------------------

def _vit_forward(bb, imgs, mlp):
    from rovit_hip.native import call, ptr, stream_ptr
    n = imgs.shape[0]
    ws = bb.eng.take_ws(n, False, dev())
    f = torch.empty(n, 192, device=dev())
    call('rovit_vit_forward', ptr(imgs), bb.pa, ptr(bb.eng.prep), ptr(ws), ptr(f), n, bb.vit.depth, 0, mlp, stream_ptr())
    bb.eng.give_ws(n, False, ws)
    return f


def _exact_from_values(res, b):
    """shapley_exact of image b on the values patch_shap returned (every coalition of P players is among them in exact mode)."""
    s = _shap()
    Z = res['coalitions'].cpu().numpy()
    P = Z.shape[1]
    table = {bytes(np.packbits(z)): float(v) for z, v in zip(Z, res['values'][:, b].cpu().double().numpy())}
    table[bytes(np.packbits(np.zeros(P, bool)))] = float(res['base_value'][b].double())
    table[bytes(np.packbits(np.ones(P, bool)))] = float(res['value'][b].double())
    assert len(table) == 2 ** P
    return s.shapley_exact(lambda mask: table[bytes(np.packbits(mask))], P)


def _efficiency(res):
    """value - base_value against the sum of the fp32 player values, both taken in fp64: the fp32 rounding of each phi_i (2^-24 |phi_i|)
    plus the fp64 solve's own 1e-12."""
    pv = res['player_values'].double()
    gap = (res['value'].double() - res['base_value'].double() - pv.sum(1)).abs()
    tol = 2.0 ** -24 * pv.abs().sum(1) + 1e-12
    print('efficiency gap', gap.cpu().numpy(), 'tol', tol.cpu().numpy())
    assert bool((gap <= tol).all())


def test_patch_shap_replace_against_the_pixel_recipe_and_the_definition():
    from rovit_hip.input_grad import _Backbone, _head_outputs
    from rovit_hip.native import MLP_ONE_LAUNCH
    m = _model()
    B = 2
    x = _images(B, 21).to(dev())
    base = (_images(B, 22) * 0.5).to(dev())
    res = m.patch_shap(x, players=2, num_samples=14, perturbation='replace', baseline=base, return_values=True)
    assert res['exact'] and res['num_samples'] == 14 and bool(res['ok'].all())
    assert tuple(res['values'].shape) == (14, B) and tuple(res['coalitions'].shape) == (14, 4) and tuple(res['player_values'].shape) == (B, 4)
    cls = res['class_idx']
    pmap = torch.from_numpy(_shap().player_map(2)).to(dev()).long()
    present = res['coalitions'][:, pmap]                                                              # (14, 196)
    pix = present.view(14, 1, 1, 14, 1, 14, 1).expand(14, B, 3, 14, 16, 14, 16).reshape(14, B, 3, 224, 224)
    imgs = torch.where(pix, x.unsqueeze(0), base.unsqueeze(0)).reshape(14 * B, 3, 224, 224).contiguous()
    with torch.no_grad():
        # the engine's own forward on the pixel images, the MLP path patch_shap resolves for chunk 256 x 197 rows: bit for bit
        bb = _Backbone(m, dev())
        logits = _head_outputs(m, _vit_forward(bb, imgs, MLP_ONE_LAUNCH))[0]
        want = torch.softmax(logits, 1).view(14, B, -1).gather(2, cls.view(1, B, 1).expand(14, B, 1)).squeeze(2)
        assert torch.equal(res['values'], want)
        # the model's inference forward (predict()'s): another MLP path may be taken, so within the probability tolerance
        pred = torch.softmax(m(imgs)['cls_logits'].float(), 1).view(14, B, -1).gather(2, cls.view(1, B, 1).expand(14, B, 1)).squeeze(2)
        err = float((res['values'] - pred).abs().max())
        print(f'values against the inference forward: max-abs {err:.2e}')
        assert err < PROB_TOL
        full = torch.softmax(m(x)['cls_logits'].float(), 1).gather(1, cls.view(-1, 1))[:, 0]
        assert float((res['value'] - full).abs().max()) < PROB_TOL
    for b in range(B):
        y = (res['values'][:, b].double() - res['base_value'][b].double()).abs().max()
        want = _exact_from_values(res, b)
        err = float(np.abs(res['player_values'][b].cpu().double().numpy() - want).max())
        print(f'image {b}: |phi - exact| {err:.2e}, max|y| {float(y):.2e}, fit_rmse {float(res["fit_rmse"][b]):.2e}')
        assert err <= 1e-6 * float(y)
    _efficiency(res)
    assert tuple(res['shap'].shape) == (B, 224, 224)
    small = m.patch_shap(x, players=2, num_samples=14, perturbation='replace', baseline=base, upsample=False)
    assert tuple(small['shap'].shape) == (B, 14, 14) and torch.equal(small['player_values'], res['player_values'])
    # a player's value over its 49 patches: the kernel divides the fp64 value and rounds once, this divides the fp32 one (2 ulp)
    torch.testing.assert_close(small['shap'].view(B, 196), (res['player_values'].double() / 49.0)[:, pmap].float(), rtol=2.0 ** -22, atol=0)
    assert torch.equal(res['shap'], (small['shap'] / 256.0).view(B, 14, 1, 14, 1).expand(B, 14, 16, 14, 16).reshape(B, 224, 224))


def test_patch_shap_drop_against_the_torch_rows_and_its_independence():
    from rovit_hip.input_grad import _Backbone, _head_outputs
    from rovit_hip.native import MLP_ONE_LAUNCH, MLP_TWO_LAUNCH, MLP_FUSED_MIN_ROWS
    from rovit_hip.perturbation import source_rows
    m = _model()
    B = 2
    x = _images(B, 31).to(dev())
    res = m.patch_shap(x, players=2, num_samples=14, perturbation='drop', return_values=True)
    assert res['exact'] and bool(res['ok'].all())
    cls = res['class_idx']
    pmap = torch.from_numpy(_shap().player_map(2)).to(dev()).long()
    absent = ~res['coalitions'][:, pmap]
    kept = (~absent).sum(1)
    with torch.no_grad():
        bb = _Backbone(m, dev())
        img_t = torch.empty(B, 197, 192, device=dev())
        bb.embed(x, img_t)
        want = torch.empty(14, B, device=dev())
        for k in kept.unique().tolist():
            idx = (kept == k).nonzero()[:, 0]
            src = source_rows(absent[idx], 'drop', k + 1).repeat_interleave(B, dim=0).contiguous()
            seq_img = torch.arange(B, device=dev()).repeat(len(idx)).int()
            ws = bb.eng.take_ws(src.shape[0], False, dev())
            mlp = MLP_ONE_LAUNCH if 256 * (k + 1) >= MLP_FUSED_MIN_ROWS else MLP_TWO_LAUNCH
            feats = bb.forward_tokens(img_t, img_t, 0, seq_img, src, ws, mlp)
            bb.eng.give_ws(src.shape[0], False, ws)
            p = torch.softmax(_head_outputs(m, feats)[0], 1).view(len(idx), B, -1)
            want[idx] = p.gather(2, cls.view(1, B, 1).expand(len(idx), B, 1)).squeeze(2)
    assert torch.equal(res['values'], want)
    for b in range(B):
        y = float((res['values'][:, b].double() - res['base_value'][b].double()).abs().max())
        assert float(np.abs(res['player_values'][b].cpu().double().numpy() - _exact_from_values(res, b)).max()) <= 1e-6 * y
    _efficiency(res)
    # an image alone: the same bits as its row of the batch
    alone = m.patch_shap(x[1:2], players=2, num_samples=14, perturbation='drop', return_values=True)
    for k in ('shap', 'player_values', 'base_value', 'value', 'fit_rmse', 'ok', 'class_idx'):
        assert torch.equal(alone[k][0], res[k][1]), k
    assert torch.equal(alone['values'][:, 0], res['values'][:, 1])
    # a list of two targets: a dict whose entries equal the single-target calls
    both = m.patch_shap(x, target=['mu', 'class'], players=2, num_samples=14, perturbation='drop', return_values=True)
    assert list(both) == ['mu', 'class'] and 'class_idx' not in both['mu']
    mu = m.patch_shap(x, target='mu', players=2, num_samples=14, perturbation='drop', return_values=True)
    for name, single in (('mu', mu), ('class', res)):
        for k in ('shap', 'player_values', 'base_value', 'value', 'fit_rmse', 'ok', 'values', 'coalitions'):
            assert torch.equal(both[name][k], single[k]), (name, k)
    _efficiency(mu)
    # the explainer class of the explainability package
    from explainability import PatchSHAP
    got = PatchSHAP(m, device=dev()).explain(x.cpu(), players=2, num_samples=14)
    assert got.shape == (224, 224) and np.array_equal(got, res['shap'][0].cpu().numpy())


def test_patch_shap_of_all_196_patches():
    m = _model()
    x = _images(1, 41).to(dev())
    res = m.patch_shap(x, players=14, num_samples=784, perturbation='drop')
    assert bool(res['ok'].all()) and not res['exact'] and res['num_samples'] == 784
    assert tuple(res['shap'].shape) == (1, 224, 224) and tuple(res['player_values'].shape) == (1, 196)
    small = m.patch_shap(x, players=14, num_samples=784, perturbation='drop', upsample=False)
    assert tuple(small['shap'].shape) == (1, 14, 14) and torch.equal(small['shap'].view(1, 196), res['player_values'])
    assert bool(torch.isfinite(res['player_values']).all()) and float(res['fit_rmse']) >= 0.0
    _efficiency(res)
    curves = m.perturbation_curves(x, res['shap'], steps=4, perturbation='drop', class_idx=res['class_idx'])
    assert tuple(curves['deletion'].shape) == (1, 5)
    assert torch.equal(curves['deletion'][:, 0], res['value']) and torch.equal(curves['deletion'][:, -1], res['base_value'])
    # the ranking the curves take from the upsampled map is the ranking of the player values
    from rovit_hip.perturbation import patch_order
    assert torch.equal(patch_order(res['shap']), patch_order(small['shap']))
