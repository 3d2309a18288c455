"""GPU tests of csrc/tsne.hip through rovit_hip.embedding: the distances, the perplexity search, the duplicate rows, the symmetrised P,
one iteration and the whole descent against the numpy fp64 statements (bit for bit where fp32 is exact, within derived bounds
elsewhere), their determinism, a row that is not valid, kNN preservation and the model entry point.

Measured on the MI355X over the cases below (printed by the tests before they assert; u = 2^-24):
  distances    max |D - D_ref| / ((E + 2) u D_ref) = 1.458e-01 with l2 (n = 65, E = 32; 6.4e-02 .. 1.5e-01 over the cases), 7.116e-02 of the
               cosine bound below (n = 65, E = 32; 3.2e-02 .. 7.1e-02)
  perplexity   max |exp(H) / perplexity - 1| of the device rows, H recomputed in fp64 = 3.238e-07 (n = 257, perplexity 15)
               max relative error of beta against the fp64 oracle on the device's own D = 4.985e-06, of p_j|i >= 1e-6 = 6.497e-05 (both at
               n = 257, perplexity 2: H(beta) is flattest there, and the error of p is that of beta times beta d, about 13 at p = 1e-6);
               at perplexity >= 5 they are below 2.2e-07 and 2.6e-06
  one step     Z error / bound <= 1.9e-02, gradient error / bound <= 6.4e-02 over the twelve cases, no gain undecided
  whole run    final KL 0.8975 against the oracle's 0.8826: ratio 1.0169 (the fp32 numpy restatement of the oracle gives 1.015); purity
               1.0000 (oracle 1.0000, the features themselves 0.9829); kNN preservation at k = 10: 0.419455, the numpy count exactly
The asserted tolerances are 4 x these (a margin for data the tests do not cover), capped at 1e-3; a None would mean not measured yet,
and the cap alone would hold.

Cosine bound.  The unit rows carry a relative error of at most (E/2 + 3) u each (the fma chain of the squared norm: E u / 2 on its root,
the root and the division: 1 u each, one more for the chain's final rounding), so every difference x^_ik - x^_jk is off by at most
(E/2 + 3) u (|x^_ik| + |x^_jk|); squared and summed over k that moves D by at most 2 (E/2 + 3) u sqrt(D) (|x^_i| + |x^_j|)
= 4 (E/2 + 3) u sqrt(D) (Cauchy-Schwarz, unit rows), on top of the (E + 2) u D of the chain itself:
  |D - D_ref| <= (E + 2) u D_ref + (2 E + 12) u sqrt(D_ref).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsne_cases as cases  # noqa: E402
from oracle import ref_cpu  # noqa: E402  (checker only)

from rovit_hip import embedding as EM  # noqa: E402

pytestmark = pytest.mark.gpu

U = cases.U32
CAP = 1e-3
MEASURED_DISTANCE_RATIO = 1.458e-01
MEASURED_COSINE_RATIO = 7.116e-02
MEASURED_PERPLEXITY = 3.238e-07
MEASURED_BETA = 4.985e-06
MEASURED_P = 6.497e-05
MEASURED_KL_RATIO = 1.0169


def tolerance(measured):
    return CAP if measured is None else min(4.0 * measured, CAP)


def dev():
    return torch.device('cuda:0')


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def tsne(**kw):
    kw.setdefault('perplexity', 2.0)
    return EM.TSNE(**kw)


# ---- 1. distances ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('E', [32, 192])
@pytest.mark.parametrize('n', [4, 63, 64, 65, 257])
def test_integer_rows_bit_equal(n, E):
    x = cases.integer_rows(n, E, seed=n + E)
    D = tsne(perplexity=1.5).distances(cuda(x)).cpu().numpy()
    ref = EM.distances_reference(x)[0]
    assert D.dtype == np.float32 and np.array_equal(D.astype(np.float64), ref)
    capped = tsne(perplexity=1.5)
    capped.max_workgroups = 3
    assert np.array_equal(capped.distances(cuda(x)).cpu().numpy(), D)


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
@pytest.mark.parametrize('n,E', [(65, 32), (257, 192), (257, 256)])
def test_float_rows_within_the_derived_bound(n, E, metric):
    x = cases.float_rows(n, E)
    D = tsne(metric=metric).distances(cuda(x)).cpu().numpy().astype(np.float64)
    ref = EM.distances_reference(x, metric)[0]
    bound = (E + 2) * U * ref + ((2 * E + 12) * U * np.sqrt(ref) if metric == 'cosine' else 0.0)
    off = ~np.eye(n, dtype=bool)
    print(f'tsne distances n={n} E={E} {metric}: max error / bound = {(np.abs(D - ref)[off] / bound[off]).max():.3e}')
    assert np.all(np.diag(D) == 0) and np.array_equal(D, D.T)
    assert np.all(np.abs(D - ref) <= bound)


# ---- 2. perplexity ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,perplexity', cases.PERPLEXITY_CASES)
def test_conditional_rows_reach_their_perplexity(n, perplexity):
    x = cases.float_rows(n, 32)
    t = tsne(perplexity=perplexity)
    out = t.affinities(cuda(x), symmetrize=False)
    C, beta = out['P'].cpu().numpy().astype(np.float64), out['beta'].cpu().numpy().astype(np.float64)
    status = EM.decode_status(out['status'])
    assert status['n'] == n and status['n_valid'] == n and status['bad_rows'] == 0 and status['unconverged'] == 0
    assert status['min_beta'] == beta.min() and status['max_beta'] == beta.max()
    assert np.all(np.diag(C) == 0) and np.abs(C.sum(axis=1) - 1.0).max() <= (n + 16) * U
    with np.errstate(divide='ignore', invalid='ignore'):
        H = -np.where(C > 0, C * np.log(np.where(C > 0, C, 1.0)), 0.0).sum(axis=1)
    ratio = np.abs(np.exp(H) / perplexity - 1.0).max()
    D = t.distances(cuda(x)).cpu().numpy().astype(np.float64)      # the oracle runs on the device's own D
    ref = EM.affinities_reference(perplexity=perplexity, symmetrize=False, D=D)
    beta_err = np.abs(beta / ref['beta'] - 1.0).max()
    big = ref['P'] >= 1e-6                                         # below that the relative error of exp(-beta d) in fp32 is of order beta d u
    p_err = np.abs(C[big] / ref['P'][big] - 1.0).max()
    h_err = np.abs(out['entropy'].cpu().numpy() - ref['entropy']).max()
    print(f'tsne perplexity n={n} perplexity={perplexity}: |exp(H)/perplexity - 1| = {ratio:.3e}, beta rel = {beta_err:.3e}, '
          f'p rel (p >= 1e-6) = {p_err:.3e}, entropy abs = {h_err:.3e}')
    assert ratio <= tolerance(MEASURED_PERPLEXITY)
    assert beta_err <= tolerance(MEASURED_BETA)
    assert p_err <= tolerance(MEASURED_P)


# ---- 3. duplicates ---------------------------------------------------------------------------------------------------------------------

def test_duplicate_rows_are_unconverged_uniform_and_finite():
    x = cases.duplicate_rows()
    for symmetrize in (False, True):
        out = tsne(perplexity=5.0).affinities(cuda(x), symmetrize=symmetrize)
        P = out['P'].cpu().numpy()
        assert EM.decode_status(out['status'])['unconverged'] == 40
        assert np.isfinite(P).all() and torch.isfinite(out['beta']).all() and torch.isfinite(out['entropy']).all()
        if not symmetrize:
            want = np.zeros((40, 65), dtype=np.float32)
            want[:, :40] = np.float32(1.0 / 39.0)
            want[np.arange(40), np.arange(40)] = 0
            assert np.array_equal(P[:40], want)
            assert np.all(out['beta'].cpu().numpy()[:40] == np.float32(2.0 ** 64))


# ---- 4. symmetrise ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,perplexity', [(5, 2.0), (65, 5.0), (257, 15.0), (257, 80.0)])
def test_symmetric_p(n, perplexity):
    x = cases.float_rows(n, 32)
    t = tsne(perplexity=perplexity)
    out = t.affinities(cuda(x))
    P = out['P'].cpu().numpy()
    assert np.array_equal(P, P.T) and np.all(np.diag(P) == 0)
    assert abs(P.astype(np.float64).sum() - 1.0) <= (n + 16) * U * n
    D = t.distances(cuda(x)).cpu().numpy().astype(np.float64)
    ref = EM.affinities_reference(perplexity=perplexity, D=D)['P']
    floor = ref == EM.P_FLOOR
    assert np.all(P[floor] == np.float32(EM.P_FLOOR))
    print(f'tsne symmetrise n={n} perplexity={perplexity}: {int(floor.sum())} entries at the floor, sum P - 1 = {P.astype(np.float64).sum() - 1.0:.3e}')
    big = ref >= 1e-6 / n
    err = np.abs(P[big] / ref[big] - 1.0).max()
    print(f'tsne symmetrise n={n} perplexity={perplexity}: P rel (P >= 1e-6 / n) = {err:.3e}')
    assert err <= tolerance(MEASURED_P) + 4 * U
    capped = tsne(perplexity=perplexity)
    capped.max_workgroups = 2
    again = capped.affinities(cuda(x))
    assert torch.equal(again['P'], out['P']) and torch.equal(again['beta'], out['beta']) and torch.equal(again['status'], out['status'])


def test_a_nan_row_is_absent_from_p():
    x = np.array(cases.float_rows(65, 32))
    bad = np.insert(x, 7, np.nan, axis=0)
    keep = np.arange(66) != 7
    for metric in ('l2', 'cosine'):
        t = tsne(perplexity=5.0, metric=metric)
        out = t.affinities(cuda(bad))
        P = out['P'].cpu().numpy()
        status = EM.decode_status(out['status'])
        assert status['n'] == 66 and status['n_valid'] == 65 and status['bad_rows'] == 1 and status['unconverged'] == 0
        assert np.all(P[7] == 0) and np.all(P[:, 7] == 0) and np.isfinite(P).all()
        rest = P[keep][:, keep]                                     # against the oracle run WITHOUT that row, on the device's own D
        D = t.distances(cuda(x)).cpu().numpy().astype(np.float64)
        ref = EM.affinities_reference(perplexity=5.0, D=D)['P']
        big = ref >= 1e-6 / 65
        err = np.abs(rest[big] / ref[big] - 1.0).max()
        print(f'tsne nan row {metric}: P rel = {err:.3e}')
        assert np.array_equal(rest, rest.T) and np.all(rest[ref == EM.P_FLOOR] == np.float32(EM.P_FLOOR))
        assert err <= tolerance(MEASURED_P) + 4 * U
    zero = np.array(x)
    zero[3] = 0                                                     # a zero row: valid with l2, not valid with cosine
    assert EM.decode_status(tsne(perplexity=5.0).affinities(cuda(zero))['status'])['n_valid'] == 65
    assert EM.decode_status(tsne(perplexity=5.0, metric='cosine').affinities(cuda(zero))['status'])['n_valid'] == 64


# ---- 5. one step -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,s,alpha,m', cases.STEP_CASES)
def test_one_step_within_the_propagated_bounds(n, s, alpha, m):
    P, Y0, V0, G0 = cases.step_case(n, s)
    ref = cases.step_reference(n, s, alpha, m)
    eta = cases.STEP_ETA
    Y, V, G = cuda(Y0).clone(), cuda(V0).clone(), cuda(G0).clone()
    out = tsne().step(cuda(P), Y, V, G, alpha, m, eta)
    Z, g = float(out['Z']), out['grad'].cpu().numpy().astype(np.float64)
    bg = cases.gradient_bound(ref, n, alpha)
    print(f'tsne step n={n} s={s} alpha={alpha}: Z error / bound = {abs(Z - ref["Z"]) / ((n * n + 16) * U * ref["Z"]):.3e}, '
          f'gradient error / bound = {(np.abs(g - ref["grad"]) / bg).max():.3e}, kl = {float(out["kl"]):.6f} (oracle {ref["kl"]:.6f})')
    assert abs(Z - ref['Z']) <= (n * n + 16) * U * ref['Z']
    assert np.all(np.abs(g - ref['grad']) <= bg)
    decided = np.abs(ref['grad']) > bg
    assert (~decided).mean() <= 0.01
    Gd, Vd, Yd = (t.cpu().numpy().astype(np.float64) for t in (G, V, Y))
    assert np.array_equal(Gd[decided], ref['G'].astype(np.float32).astype(np.float64)[decided])
    mv, step = np.abs(m * V0.astype(np.float64)), np.abs(eta * ref['G'] * ref['grad'])
    bv = eta * ref['G'] * bg + 4 * U * (mv + step)                  # the gradient's error through eta gain, and the roundings of m v - eta gain g
    by = bv + 2 * U * (np.abs(Y0.astype(np.float64)) + np.abs(ref['V']))
    assert np.all(np.abs(Vd - ref['V'])[decided] <= bv[decided]) and np.all(np.abs(Yd - ref['Y'])[decided] <= by[decided])
    # KL: its fp32 sums over n terms per row and n rows, its logarithms (2 u each) and log Z, against the sum of the terms' absolute values
    d2 = ((Y0.astype(np.float64)[:, None, :] - Y0.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    Pd = P.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        abs_terms = np.where(Pd > 0, Pd * (np.abs(np.log(np.where(Pd > 0, Pd, 1.0))) + np.log1p(d2)), 0.0).sum() + abs(np.log(ref['Z'])) * Pd.sum()
    assert abs(float(out['kl']) - ref['kl']) <= (n + 16) * U * abs_terms


# ---- 6. the whole run ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def device_run(max_workgroups: int = 0):
    x, y, P, Y0, run = cases.whole_run()
    t = EM.TSNE(perplexity=15.0, n_iter=300, exaggeration_iter=100, init=cuda(Y0), kl_every=50)
    t.max_workgroups = max_workgroups
    Y = t.fit_transform(cuda(x))
    return t, Y.clone()


def test_whole_run_is_deterministic():
    (a, Ya), (b, Yb) = device_run(), device_run(5)
    _, Yc = device_run.__wrapped__()
    assert torch.equal(Ya, Yc) and torch.equal(Ya, Yb) and torch.equal(a.kl_trace_, b.kl_trace_)
    assert a.status_ == b.status_ == {'n': 257, 'n_valid': 257, 'bad_rows': 0, 'unconverged': 0, 'min_beta': a.status_['min_beta'],
                                      'max_beta': a.status_['max_beta'], 'iterations': 300, 'nonfinite': 0}


def test_whole_run_against_the_oracle():
    x, y, P, Y0, run = cases.whole_run()
    t, Y = device_run()
    Yh = Y.cpu().numpy()
    assert np.isfinite(Yh).all() and Yh.shape == (257, 2)
    pur, pur_ref, pur_x = cases.purity(Yh, y), cases.purity(run['map'], y), float((y[cases.knn_sets(x, 10)] == y[:, None]).mean())
    trace = t.kl_trace_.cpu().numpy().astype(np.float64)
    slots = EM.kl_slots(300, 50)
    final, final_ref = EM.kl_reference(P, Yh), EM.kl_reference(P, run['map'])
    print(f'tsne run: purity {pur:.4f} (oracle {pur_ref:.4f}, features {pur_x:.4f}); trace {np.round(trace, 4).tolist()} (oracle '
          f'{np.round(run["kl_trace"], 4).tolist()}); final KL {final:.4f}, oracle {final_ref:.4f}, ratio {final / final_ref:.4f}')
    assert len(trace) == len(slots) == 7 and slots[2] == 100
    assert pur >= 0.98
    assert final < trace[2]
    assert final <= 1.05 * final_ref
    assert t.kl_divergence_ == float(trace[-1])
    assert np.abs(Yh.astype(np.float64).mean(axis=0)).max() <= (257 + 16) * U * np.abs(Yh).max()


def test_knn_preservation_equals_the_numpy_count():
    x, y, P, Y0, run = cases.whole_run()
    _, Y = device_run()
    got = EM.knn_preservation(cuda(x), Y, k=10)
    want = cases.knn_overlap(x, Y.cpu().numpy(), 10)
    print(f'tsne knn_preservation at k = 10: {got:.6f} (numpy count {want:.6f})')
    assert got == want


# ---- 7. a row that is not valid, in a run ----------------------------------------------------------------------------------------------

def test_an_invalid_row_in_a_run():
    x = np.insert(np.array(cases.float_rows(65, 32)), 7, np.nan, axis=0)
    Y0 = EM.pca_init(torch.from_numpy(x))
    t = EM.TSNE(perplexity=5.0, n_iter=60, exaggeration_iter=20, init=Y0.to(dev()), kl_every=20)
    Y = t.fit_transform(cuda(x)).cpu().numpy()
    keep = np.arange(66) != 7
    assert np.isnan(Y[7]).all() and np.isfinite(Y[keep]).all()
    assert np.abs(Y[keep].astype(np.float64).mean(axis=0)).max() <= (65 + 16) * U * np.abs(Y[keep]).max()
    assert t.status_['n_valid'] == 65 and t.status_['bad_rows'] == 1 and t.status_['nonfinite'] == 0
    assert np.isfinite(t.kl_trace_.cpu().numpy()).all() and t.kl_divergence_ < float(t.kl_trace_[1])
    r = EM.TSNE(perplexity=5.0, n_iter=3, init='random', seed=5)
    r.fit_transform(cuda(x))
    first = EM.TSNE(perplexity=5.0, init='random', seed=5)._initial(cuda(x)).cpu().numpy()
    assert np.abs(first - EM.random_init_reference(66, 5)).max() <= 1e-4 * 64 * U * 8      # Box-Muller in fp32: a few ulp of a draw below 8 sigma


# ---- 8. the model entry ----------------------------------------------------------------------------------------------------------------

def test_model_feature_map():
    from models.rovit_kan import RoViTKAN
    model = RoViTKAN(pretrained=False)
    model.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    model = model.to(dev()).train()
    g = torch.Generator().manual_seed(0)
    images = torch.nn.functional.interpolate(torch.randn(48, 3, 7, 7, generator=g), size=224, mode='bilinear', align_corners=False).to(dev())
    out = model.feature_map(images, perplexity=10.0, n_iter=50)
    assert model.training and all(p.grad is None for p in model.parameters())
    assert out['map'].shape == (48, 2) and out['features'].shape == (48, 192) and out['kl_divergence'].shape == ()
    assert out['map'].is_cuda and torch.isfinite(out['map']).all() and torch.isfinite(out['kl_divergence'])
    t = EM.TSNE(perplexity=10.0, n_iter=50)
    assert torch.equal(t.fit_transform(out['features']), out['map']) and t.kl_divergence_ == float(out['kl_divergence'])
    loader = [(images[i:i + 16].cpu(),) for i in range(0, 48, 16)]
    assert torch.equal(model.feature_map(loader, perplexity=10.0, n_iter=50)['map'], out['map'])
