"""CPU tests of KernelSHAP's host side (rovit_hip/shap.py): the numpy fp64 references against the subset-sum definition, the plan's
invariants, the structural properties of the Shapley value, KernelShap on CPU tensors and every refusal of patch_shap."""
import itertools
import math

import numpy as np
import pytest
import torch

import shap_cases as cases


def _shap():
    from rovit_hip import shap
    return shap


# ---- exact mode against the definition -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('P', [2, 3, 4, 7, 8])
def test_exact_mode_equals_the_subset_sum_definition(P):
    """M = 2^P - 2 enumerates every coalition with the Shapley kernel's weights; the constrained fit is then the Shapley value.
    Bound 1e-12 (a numpy prototype measured <= 4.9e-15), efficiency within 1e-13."""
    s = _shap()
    M = 2 ** P - 2
    pl = s.plan(P, M)
    assert pl['exact'] and pl['M'] == M and pl['pair_exact'].all()
    Z, w = cases.reference(P, M, 0)
    tab, f = cases.random_game(P, 100 + P)
    y = np.array([f(z) for z in Z])
    r = s.solve_reference(Z, w, y, tab[0], tab[-1])
    want = s.shapley_exact(f, P)
    err = float(np.abs(r['phi'] - want).max())
    print(f'P={P}: |phi - exact| {err:.2e}, efficiency {abs(r["phi"].sum() - (tab[-1] - tab[0])):.2e}, fit_rmse {float(r["fit_rmse"]):.2e}')
    assert err < 1e-12
    assert abs(r['phi'].sum() - (tab[-1] - tab[0])) < 1e-13
    assert r['ok'] and r['min_pivot'] > 0


def test_dummy_and_symmetric_players_in_exact_mode():
    s = _shap()
    P = 6
    rng = np.random.default_rng(5)
    g = rng.standard_normal(2 ** 4)

    def f(mask):          # player 5 is a dummy; players 0 and 1 enter only through their count: symmetric
        m = np.asarray(mask, dtype=np.int64)
        return g[(m[0] + m[1]) + 3 * m[2] + 6 * m[3]] * (1.0 + 0.5 * m[4])
    Z, w = cases.reference(P, 2 ** P - 2, 0)
    y = np.array([f(z) for z in Z])
    r = s.solve_reference(Z, w, y, f(np.zeros(P, bool)), f(np.ones(P, bool)))
    assert abs(r['phi'][5]) < 1e-13
    assert abs(r['phi'][0] - r['phi'][1]) < 1e-13
    ex = s.shapley_exact(f, P)
    assert abs(ex[5]) < 1e-13 and abs(ex[0] - ex[1]) < 1e-13


# ---- additive games ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('P,M', [(196, 784), (196, 2048), (49, 256), (16, 64)])
def test_additive_game_is_recovered(P, M):
    """v(S) = c + sum_{i in S} a_i lies in the model's span, so any non-singular design recovers a.  Bound 1e-9; cond(A) < 1e7 is asserted
    first as the condition that makes it meaningful (a prototype measured <= 2.6e-12 at cond(A) <= 2.4e5)."""
    s = _shap()
    Z, w = cases.reference(P, M, 3)
    rng = np.random.default_rng(P + M)
    a, c = rng.standard_normal(P), 0.3
    r = s.solve_reference(Z, w, c + Z @ a, c, c + a.sum())
    print(f'P={P} M={M}: cond(A) {r["cond"]:.3e}, |phi - a| {np.abs(r["phi"] - a).max():.2e}, min pivot {r["min_pivot"]:.2e}')
    assert r['cond'] < 1e7
    assert np.abs(r['phi'] - a).max() < 1e-9
    assert float(r['fit_rmse']) < 1e-9


# ---- the plan --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('P,M', cases.EXACT + cases.SAMPLED + cases.MIXED + [(4, 14), (5, 30), (16, 600)])
def test_plan_invariants(P, M):
    s = _shap()
    pl = s.plan(P, M)
    Z, w = cases.reference(P, M, 1)
    assert Z.shape == (pl['M'], P) and pl['M'] == M
    assert abs(w.sum() - 1.0) < 1e-14
    assert np.array_equal(Z[0::2], ~Z[1::2])                                  # every coalition is followed by its complement
    sizes = Z.sum(axis=1)
    assert np.array_equal(sizes, pl['sizes'])
    assert sizes.min() >= 1 and sizes.max() <= P - 1
    ex = np.repeat(pl['pair_exact'].astype(bool), 2)
    p = s.size_mass(P)
    rows = [bytes(z) for z in np.packbits(Z, axis=1)]
    for c in sorted(set(pl['pair_class'][pl['pair_exact'].astype(bool)])):     # an enumerated class holds each subset once, sizes s and P - s
        for size in {c, P - c}:
            sel = [rows[m] for m in np.nonzero(ex & (sizes == size))[0]]
            assert len(sel) == math.comb(P, size) and len(set(sel)) == len(sel)
            assert np.allclose(w[ex & (sizes == size)], p[size] / math.comb(P, size), rtol=1e-15, atol=0)
    if pl['exact']:
        assert len(set(rows)) == 2 ** P - 2
    else:
        assert len(set(w[~ex])) == 1                                          # the sampled pairs carry one weight
        assert not set(pl['pair_class'][~pl['pair_exact'].astype(bool)]) & set(pl['pair_class'][pl['pair_exact'].astype(bool)])
    # enumerated coalitions come in the order of itertools.combinations
    k = 0
    for c in sorted(set(pl['pair_class'][pl['pair_exact'].astype(bool)])):
        n = int((pl['pair_class'][pl['pair_exact'].astype(bool)] == c).sum())
        for comb in itertools.islice(itertools.combinations(range(P), int(c)), n):
            assert np.array_equal(np.nonzero(Z[2 * k])[0], comb)
            k += 1


def test_mixed_plans_enumerate_the_singletons():
    s = _shap()
    for P, M in cases.MIXED:
        pl = s.plan(P, M)
        assert not pl['exact'] and int(pl['pair_exact'].sum()) == P and set(pl['pair_class'][:P]) == {1}
    for P, M in cases.SAMPLED:
        assert not s.plan(P, M)['pair_exact'].any()


def test_budget_is_made_even_clipped_and_refused_when_too_small():
    from rovit_hip import RovitHipError
    s = _shap()
    assert s.plan(8, 33)['M'] == 32
    assert s.plan(8, 10 ** 6)['M'] == 254 and s.plan(8, 10 ** 6)['exact']
    assert s.plan(3, 7)['M'] == 6
    assert s.plan(196, 785)['M'] == 784
    for P, M in [(4, 8), (4, 13), (8, 31), (196, 783), (2, 1), (49, 195)]:
        with pytest.raises(RovitHipError, match='num_samples'):
            s.plan(P, M)
    for P in (1, 197, 0, True, 2.0):
        with pytest.raises(RovitHipError, match='players'):
            s.plan(P, 64)


def test_coalitions_depend_on_the_seed_alone():
    s = _shap()
    P, M = 13, 52
    a, wa = s.coalitions_reference(P, M, 5)
    b, wb = s.coalitions_reference(P, M, 5)
    c, _ = s.coalitions_reference(P, M, 6)
    d, _ = s.coalitions_reference(P, M, 5 + (1 << 32))
    assert np.array_equal(a, b) and np.array_equal(wa, wb)
    assert not np.array_equal(a, c) and not np.array_equal(a, d)             # the high key word matters too
    # a KernelShap's coalitions are the reference's whatever patch map carries the players
    k1 = s.KernelShap(cases.patch_map_for(P), M, 5).coalitions('cpu')
    k2 = s.KernelShap(num_players=P, num_samples=M, seed=5).coalitions('cpu')
    assert torch.equal(k1['bits'], k2['bits']) and torch.equal(k1['weights'], k2['weights'])
    assert np.array_equal(s.unpack_bits(k1['bits'], P).numpy(), a)
    # the draw: the stream word is its own
    from rovit_hip import native
    assert native.SHAP_STREAM not in (native.EVAL_BOOT_STREAM, native.EVAL_CONF_STREAM) and native.SHAP_STREAM == 0x53686170


def test_the_draw_rule_by_hand():
    """Sampled pair r of class s: the s smallest keys (word << 32) | i, word = word i % 4 of Philox(key = seed, counter (i // 4, r,
    SHAP_STREAM, 0)) -- restated here with scalar calls."""
    from oracle.philox import philox4x32_10
    from rovit_hip import native
    s = _shap()
    P, M, seed = 13, 52, (1 << 40) + 12345
    pl = s.plan(P, M)
    Z, _ = s.coalitions_reference(P, M, seed)
    for r in (0, 7, 25):
        keys = []
        for i in range(P):
            w = philox4x32_10([i // 4, r, native.SHAP_STREAM, 0], [seed & 0xFFFFFFFF, seed >> 32])[i % 4]
            keys.append((int(w) << 32) | i)
        members = sorted(np.argsort(np.array(keys, dtype=np.uint64))[:int(pl['pair_class'][r])])
        assert list(np.nonzero(Z[2 * r])[0]) == members


# ---- KernelShap on CPU tensors ---------------------------------------------------------------------------------------------------------

def test_kernel_shap_on_cpu_tensors_runs_the_references():
    from rovit_hip.perturbation import source_rows
    s = _shap()
    P, M = 49, 256
    ks = s.KernelShap(7, M, seed=2)
    assert ks.P == P and ks.M == M and not ks.exact
    co = ks.coalitions('cpu')
    Z, w = cases.reference(P, M, 2)
    assert np.array_equal(s.unpack_bits(co['bits'], P).numpy(), Z) and np.array_equal(co['weights'].numpy(), w)
    absent = torch.from_numpy(~Z[:, ks.players])
    assert torch.equal(co['src_replace'], source_rows(absent, 'replace'))
    seen = 0
    for tokens, idx, src in co['src_drop']:
        assert torch.equal(src, source_rows(absent[idx], 'drop', tokens)) and src.shape == (len(idx), tokens)
        seen += len(idx)
    assert seen == M
    vals, v0, v1 = cases.synthetic_values(Z, 3, 2, 9)
    out = ks.solve(torch.from_numpy(vals), torch.from_numpy(v0), torch.from_numpy(v1))
    ref = s.solve_reference(Z, w, vals, v0, v1)
    assert np.array_equal(out['phi'].numpy(), ref['phi']) and out['phi32'].dtype == torch.float32
    assert tuple(out['patch_map'].shape) == (3, 2, 196) and bool(out['ok'].all())
    # 196 fp32 roundings of values below 1: 196 * 2^-24 < 1.2e-5
    assert np.allclose(out['patch_map'].double().sum(-1).numpy(), ref['phi'].sum(-1), rtol=0, atol=1.2e-5)
    flat = ks.solve(torch.from_numpy(vals[:, :, 0].copy()), torch.from_numpy(v0[:, 0].copy()), torch.from_numpy(v1[:, 0].copy()))
    assert tuple(flat['phi'].shape) == (3, P) and np.array_equal(flat['phi'].numpy(), ref['phi'][:, 0])


def test_rank_deficient_design_is_flagged_on_cpu():
    s = _shap()
    Z, w = cases.rank_deficient_design()
    ks = s.KernelShap.from_design(Z, w)
    out = ks.solve(torch.ones(8, 2), torch.zeros(2), torch.ones(2))
    assert not bool(out['ok'].any()) and bool(torch.isnan(out['phi']).all())


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------

def test_patch_shap_refuses_bad_arguments_before_anything_runs():
    from rovit_hip import RovitHipError
    from models.rovit_kan import RoViTKAN
    m = RoViTKAN(pretrained=False).eval()
    x = torch.zeros(2, 3, 224, 224)
    bad = [
        (dict(perturbation='blur'), 'perturbation must be one of'),
        (dict(perturbation='drop', baseline=torch.zeros(1, 3, 224, 224)), 'takes no baseline'),
        (dict(players=1), 'one player'),
        (dict(players=3), 'players must be an int out of'),
        (dict(players=True), 'players must be an int out of'),
        (dict(players=torch.zeros(196)), 'must hold integers'),
        (dict(players=torch.zeros(195, dtype=torch.long)), r'shape \(196,\)'),
        (dict(players=torch.zeros(196, dtype=torch.long)), 'every id of 0..P-1'),
        (dict(players=torch.arange(196) % 5 * 2), 'every id of 0..P-1'),
        (dict(players=torch.from_numpy(cases.UNEQUAL5)), 'equal patch count'),
        (dict(players=2, num_samples=8), r'below min\(2\^P - 2, 4 P\)'),
        (dict(players=14, num_samples=700), r'below min\(2\^P - 2, 4 P\)'),
        (dict(num_samples=2.5), 'num_samples must be an int'),
        (dict(num_samples=1 << 21), 'above the limit'),
        (dict(seed=-1), 'seed must be an int'),
        (dict(seed=1.5), 'seed must be an int'),
        (dict(upsample=1), 'upsample must be a bool'),
        (dict(return_values=None), 'return_values must be a bool'),
        (dict(target='nope'), 'unknown target'),
        (dict(target=[]), 'target must be a name'),
        (dict(target=['mu', 'mu']), 'more than once'),
        (dict(target='mu', class_idx=1), "does not contain 'class'"),
        (dict(class_idx=9), 'class_idx must be in'),
        (dict(chunk=0), 'chunk must be an int >= 1'),
        (dict(perturbation='replace', baseline=torch.zeros(3, 3, 224, 224)), 'does not broadcast'),
        (dict(perturbation='replace', baseline=3.0), 'baseline must be a floating-point tensor'),
    ]
    for kw, msg in bad:
        with pytest.raises(RovitHipError, match=msg):
            m.patch_shap(x, **kw)
    with pytest.raises(RovitHipError, match=r'expects \(B,3,224,224\) images'):
        m.patch_shap(torch.zeros(2, 3, 32, 32))
    with pytest.raises(RovitHipError, match='GPU'):                           # a CPU model: no fallback, as predict_mc
        m.patch_shap(x)
    with pytest.raises(RovitHipError, match='GPU'):
        m.patch_shap(x, target=['class', 'mu'], perturbation='replace', players=7, num_samples=256)
    from explainability import PatchSHAP
    with pytest.raises(RovitHipError, match='one player'):
        PatchSHAP(m, device='cpu').explain(x, players=1)


def test_kernel_shap_refuses_bad_arguments():
    from rovit_hip import RovitHipError
    s = _shap()
    with pytest.raises(RovitHipError, match='not both'):
        s.KernelShap()
    with pytest.raises(RovitHipError, match='not both'):
        s.KernelShap(7, 256, num_players=49)
    ks = s.KernelShap(num_players=8, num_samples=32)
    with pytest.raises(RovitHipError, match='values must be'):
        ks.solve(torch.zeros(31, 2), torch.zeros(2), torch.zeros(2))
    with pytest.raises(RovitHipError, match='v_full must be'):
        ks.solve(torch.zeros(32, 2), torch.zeros(2), torch.zeros(3))
    with pytest.raises(RovitHipError, match='brute force'):
        s.shapley_exact(lambda m: 0.0, 21)
    with pytest.raises(RovitHipError, match='from_design'):
        s.KernelShap.from_design(np.zeros((4, 1)), np.ones(4))
