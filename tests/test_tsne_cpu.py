"""CPU tests of rovit_hip.embedding: the numpy fp64 statements that are the oracle of csrc/tsne.hip (the gradient against a finite
difference of the KL divergence, the affinities' invariants, the duplicate rows), every refusal, the 'random' init against
oracle/philox.py, the CPU path of the public methods and the binding."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsne_cases as cases  # noqa: E402
from oracle import philox  # noqa: E402

from rovit_hip import embedding as EM  # noqa: E402
from rovit_hip import native  # noqa: E402
from rovit_hip.native import RovitHipError  # noqa: E402


def test_reference_gradient_is_the_finite_difference_of_the_reference_kl():
    rng = np.random.default_rng(3)
    n = 7
    P = rng.random((n, n))
    P = P + P.T
    np.fill_diagonal(P, 0.0)
    P /= P.sum()
    Y = rng.standard_normal((n, 2))
    ref = EM.step_reference(P, Y, np.zeros((n, 2)), np.ones((n, 2)), 1.0, 0.5, 1.0)
    assert abs(ref['kl'] - EM.kl_reference(P, Y)) < 1e-13
    h = 1e-6
    for i in range(n):
        for c in range(2):
            up, dn = Y.copy(), Y.copy()
            up[i, c] += h
            dn[i, c] -= h
            fd = (EM.kl_reference(P, up) - EM.kl_reference(P, dn)) / (2 * h)
            assert abs(fd - ref['grad'][i, c]) < 1e-8, (i, c, fd, ref['grad'][i, c])


@pytest.mark.parametrize('n,perplexity', [(5, 2.0), (65, 5.0), (65, 15.0), (257, 80.0)])
def test_reference_affinities_symmetric_normalised_and_at_their_perplexity(n, perplexity):
    x = cases.float_rows(n, 32)
    cond = EM.affinities_reference(x, perplexity, symmetrize=False)
    C = cond['P']
    assert np.all(np.diag(C) == 0) and np.allclose(C.sum(axis=1), 1.0, rtol=0, atol=1e-13)
    with np.errstate(divide='ignore', invalid='ignore'):
        H = -np.where(C > 0, C * np.log(np.where(C > 0, C, 1.0)), 0.0).sum(axis=1)
    assert np.abs(np.exp(H) / perplexity - 1.0).max() <= 1e-12
    assert np.abs(H - cond['entropy']).max() <= 1e-12
    sym = EM.affinities_reference(x, perplexity)
    P = sym['P']
    assert np.array_equal(P, P.T) and np.all(np.diag(P) == 0)
    assert abs(P.sum() - 1.0) <= n * n * EM.P_FLOOR + 1e-12
    assert sym['status'] == dict(cond['status']) and sym['status']['unconverged'] == 0 and sym['status']['n_valid'] == n
    D, ok = EM.distances_reference(x)
    again = EM.affinities_reference(perplexity=perplexity, D=D, valid=ok)
    assert np.array_equal(again['P'], P)


def test_reference_duplicates_are_unconverged_and_uniform():
    x = cases.duplicate_rows()
    out = EM.affinities_reference(x, 5.0, symmetrize=False)
    C = out['P']
    assert out['status']['unconverged'] == 40 and np.isfinite(C).all() and np.isfinite(out['beta']).all() and np.isfinite(out['entropy']).all()
    for i in range(40):
        others = [j for j in range(40) if j != i]
        assert np.all(C[i, others] == 1.0 / 39.0) and C[i, i] == 0 and np.all(C[i, 40:] == 0)
        assert out['beta'][i] == 2.0 ** 64
    assert np.isfinite(EM.affinities_reference(x, 5.0)['P']).all()


def test_reference_treats_a_bad_row_as_absent():
    x = np.array(cases.float_rows(65, 32))
    bad = np.insert(x, 7, np.nan, axis=0)
    a, b = EM.affinities_reference(x, 5.0), EM.affinities_reference(bad, 5.0)
    keep = np.arange(66) != 7
    assert b['status']['n_valid'] == 65 and b['status']['bad_rows'] == 1
    assert np.all(b['P'][7] == 0) and np.all(b['P'][:, 7] == 0)
    assert np.array_equal(b['P'][keep][:, keep], a['P'])


def test_reference_step_decides_every_gain_of_the_gpu_cases():
    """The GPU test compares the new gains wherever |g| exceeds the gradient's bound: the reference leaves none undecided."""
    for n, s, alpha, m in cases.STEP_CASES:
        ref = cases.step_reference(n, s, alpha, m)
        assert np.all(np.abs(ref['grad']) > cases.gradient_bound(ref, n, alpha)), (n, s, alpha)


def test_steps_on_cpu_tensors_are_the_run_reference():
    P, Y, _, G = (torch.from_numpy(np.array(a)).double() for a in cases.step_case(65, 1e-4))
    V, Y0 = torch.zeros_like(Y), Y.numpy().copy()
    t = EM.TSNE(perplexity=5.0)
    kls = []
    for it in range(4):
        out = t.step(P, Y, V, G, 12.0 if it < 2 else 1.0, 0.5 if it < 2 else 0.8, 50.0)
        kls.append(float(out['kl']))
    run = EM.run_reference(P.numpy(), Y0, 4, 12.0, 2, 50.0, 1)
    assert np.allclose(Y.numpy() - Y.numpy().mean(axis=0), run['map'], rtol=0, atol=1e-15)
    assert np.allclose(kls, run['kl_trace'], rtol=1e-13, atol=0)


def test_fit_transform_on_cpu_tensors():
    x = torch.from_numpy(np.insert(np.array(cases.float_rows(65, 32)), 3, np.inf, axis=0))
    t = EM.TSNE(perplexity=5.0, n_iter=60, exaggeration_iter=20, kl_every=10)
    Y = t.fit_transform(x)
    assert Y.shape == (66, 2) and Y.dtype == torch.float32 and torch.isnan(Y[3]).all()
    keep = np.arange(66) != 3
    assert np.isfinite(Y.numpy()[keep]).all() and np.abs(Y.numpy()[keep].astype(np.float64).mean(axis=0)).max() < 1e-5
    assert t.status_ == {'n': 66, 'n_valid': 65, 'bad_rows': 1, 'unconverged': 0, 'min_beta': t.status_['min_beta'],
                         'max_beta': t.status_['max_beta'], 'iterations': 60, 'nonfinite': 0}
    assert len(t.kl_trace_) == len(EM.kl_slots(60, 10)) == 7 and t.kl_divergence_ == pytest.approx(float(t.kl_trace_[-1]), rel=1e-6)
    assert t.kl_divergence_ < float(t.kl_trace_[2])
    aff = t.affinities(x)
    assert aff['status']['n_valid'] == 65 and aff['P'].shape == (66, 66)
    assert EM.TSNE(perplexity=5.0).distances(x).shape == (66, 66)


def test_random_init_is_the_philox_stream():
    n, seed = 9, 0x1234567890
    got = EM.random_init_reference(n, seed)
    for e in range(2 * n):
        w = philox.philox4x32_10([e, 0, native.TSNE_STREAM, 0], [seed & 0xFFFFFFFF, seed >> 32])
        u1, u2 = ((int(w[0]) >> 8) + 1) / 2.0 ** 24, (int(w[1]) >> 8) / 2.0 ** 24
        assert got[e // 2, e % 2] == 1e-4 * np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    t = EM.TSNE(perplexity=2.0, init='random', seed=seed)
    assert np.array_equal(t._initial(torch.zeros(n, 32)).numpy(), got.astype(np.float32))
    big = EM.random_init_reference(4096, 1)
    assert abs(big.mean()) < 5e-6 and abs(big.std() / 1e-4 - 1.0) < 0.05


def test_pca_init():
    x = np.array(cases.float_rows(65, 32))
    Y = EM.pca_init(torch.from_numpy(x)).numpy().astype(np.float64)
    xc = x.astype(np.float64) - x.astype(np.float64).mean(axis=0)
    val, vec = np.linalg.eigh(xc.T @ xc / 65)
    for c, k in ((0, -1), (1, -2)):
        v = vec[:, k] * np.sign(vec[np.argmax(np.abs(vec[:, k])), k])
        proj = xc @ v
        assert np.allclose(Y[:, c], proj * (Y[:, 0].std() / (xc @ vec[:, -1]).std()), rtol=1e-5, atol=1e-10)
    assert abs(Y[:, 0].std() - 1e-4) < 1e-10
    bad = EM.pca_init(torch.from_numpy(np.insert(x, 0, np.nan, axis=0)))
    assert torch.isnan(bad[0]).all() and np.allclose(bad[1:].numpy(), Y, rtol=1e-4, atol=1e-9)


def test_every_refusal():
    ok = torch.zeros(40, 32)
    for kw in ({'perplexity': 1.0}, {'perplexity': 'thirty'}, {'n_iter': 0}, {'metric': 'manhattan'}, {'init': 'spectral'}, {'learning_rate': 0},
               {'learning_rate': 'fast'}, {'early_exaggeration': 0}, {'kl_every': -1}, {'exaggeration_iter': 1.5}):
        with pytest.raises(RovitHipError):
            EM.TSNE(**kw)
    t = EM.TSNE(perplexity=30.0)
    for x in (torch.zeros(3, 32), torch.zeros(native.TSNE_MAX_ROWS + 1, 32), torch.zeros(40, 48), torch.zeros(40, 288), torch.zeros(40),
              torch.zeros(30, 32), torch.zeros(31, 32)):                       # the last two: perplexity 30 is not below n - 1
        for method in (t.fit_transform, t.affinities, t.distances):
            with pytest.raises(RovitHipError):
                method(x)
    t.affinities(torch.randn(32, 32, generator=torch.Generator().manual_seed(0)))      # perplexity 30 < 31: accepted
    with pytest.raises(RovitHipError, match='16384'):
        t.fit_transform(torch.zeros(native.TSNE_MAX_ROWS + 1, 32))
    with pytest.raises(RovitHipError):
        EM.TSNE(perplexity=5.0, init=torch.zeros(39, 2)).fit_transform(ok)
    with pytest.raises(RovitHipError):
        EM.TSNE(perplexity=5.0, init=torch.zeros(40, 2, device='meta')).fit_transform(ok)
    with pytest.raises(RovitHipError):
        t.step(torch.zeros(5, 5), torch.zeros(6, 2), torch.zeros(6, 2), torch.zeros(6, 2), 12.0, 0.5, 50.0)
    with pytest.raises(RovitHipError):
        t.step(torch.zeros(5, 5), torch.zeros(5, 2), torch.zeros(5, 2), torch.zeros(5, 2), 12.0, 1.0, 50.0)
    with pytest.raises(RovitHipError):
        EM.knn_preservation(ok, torch.zeros(39, 2))
    with pytest.raises(RovitHipError):
        EM.knn_preservation(ok, torch.zeros(40, 2), k=33)
    with pytest.raises(RovitHipError):
        EM.TSNE().kl_divergence_


def test_knn_preservation_on_cpu_tensors_is_the_numpy_count():
    x = np.array(cases.float_rows(65, 32))
    Y = np.random.default_rng(5).standard_normal((65, 2)).astype(np.float32)
    got = EM.knn_preservation(torch.from_numpy(x), torch.from_numpy(Y), k=10)
    assert got == cases.knn_overlap(x, Y, 10)
    assert EM.knn_preservation(torch.from_numpy(x), torch.from_numpy(x[:, :2].copy()), k=5) > got


def test_binding_and_limits():
    lib = native.load()
    for name in ('rovit_tsne_workspace_bytes', 'rovit_tsne_affinities', 'rovit_tsne_run', 'rovit_tsne_random_init'):
        assert name in native.SIGNATURES and hasattr(lib, name)
    assert native.ABI_VERSION == lib.rovit_version()
    assert lib.rovit_tsne_workspace_bytes(3, 32) == 0 and lib.rovit_tsne_workspace_bytes(native.TSNE_MAX_ROWS + 1, 32) == 0
    assert lib.rovit_tsne_workspace_bytes(64, 48) == 0 and lib.rovit_tsne_workspace_bytes(64, 288) == 0
    small, big = lib.rovit_tsne_workspace_bytes(4, 32), lib.rovit_tsne_workspace_bytes(native.TSNE_MAX_ROWS, 256)
    assert 0 < small < big and small % 16 == 0 and big >= native.TSNE_MAX_ROWS * (256 + 8 + 2) * 4
    # a bad descriptor is refused before any launch: these calls need no device
    d = native.TsneAffinity()
    d.n, d.embed, d.metric, d.perplexity = 3, 32, native.KNN_L2, 2.0
    assert lib.rovit_tsne_affinities(ctypes.byref(d), None) != 0 and b'rows' in lib.rovit_last_error_string()
    d.n, d.perplexity = 64, 63.0
    assert lib.rovit_tsne_affinities(ctypes.byref(d), None) != 0 and b'perplexity' in lib.rovit_last_error_string()
    d.perplexity, d.embed = 5.0, 48
    assert lib.rovit_tsne_affinities(ctypes.byref(d), None) != 0 and b'embed' in lib.rovit_last_error_string()
    r = native.TsneDescent()
    r.n, r.n_iter = native.TSNE_MAX_ROWS + 1, 10
    assert lib.rovit_tsne_run(ctypes.byref(r), None) != 0 and b'rows' in lib.rovit_last_error_string()
    r.n, r.n_iter = 64, 0
    assert lib.rovit_tsne_run(ctypes.byref(r), None) != 0 and b'iterations' in lib.rovit_last_error_string()
    assert ctypes.sizeof(native.TsneAffinity) == 88 and ctypes.sizeof(native.TsneDescent) == 128
