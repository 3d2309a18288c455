"""The case lists of tests/wgrad_cases.py must reach every step count, tail and split edge of the weight-gradient loop (csrc/gemm.hip,
wgrad_kernel).  Everything here is computed from ``geometry()`` on the CPU: trimming a list so that an edge is lost fails here, before a
GPU run silently covers less."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_cases as cases  # noqa: E402

# every kernel form of tests/test_gpu_wgrad_edges.py whose case list is free: (M, S) pairs.  The single-problem <96, 96> launch, the merged
# <192, 192> launch (all its layouts and problem counts), the affine un-fold and the lone flush run cases.CASES; the class-token launch
# runs cases.CLS_CASES.
FORMS = {
    'single_and_merged': cases.CASES,
    'class_token': [(M, S) for M, S, _ in cases.CLS_CASES],
}


def _splits(form):
    return [(M, S, cases.geometry(M, S)) for M, S in FORMS[form]]


def test_geometry_restates_the_issue_table():
    steps = lambda M, S: [g[2] for g in cases.geometry(M, S)]
    rows = lambda M, S: [g[1] - g[0] for g in cases.geometry(M, S)]
    assert [steps(M, 1) for M in (1, 64, 65, 129)] == [[1], [1], [2], [3]]
    assert steps(192, 2) == [2, 1]
    assert steps(193, 2) == [2, 2] and rows(193, 2)[-1] == 65
    assert steps(320, 2) == [3, 2]
    assert steps(321, 2) == [3, 3] and rows(321, 2)[-1] == 129
    assert steps(449, 2) == [4, 4] and rows(449, 2)[-1] == 193
    assert steps(448, 1) == [7]
    assert steps(833, 2) == [7, 7] and rows(833, 2)[-1] == 385
    assert steps(130, 4) == [1, 1, 1, 0] and rows(130, 4) == [64, 64, 2, 0]
    assert [steps(M, 1) for M in (257, 320, 321, 384)] == [[5], [5], [6], [6]]
    # the engine's own launches (S_MERGE): what the fp64 backward parity reaches, and training at batch 32
    assert steps(197, 4) == [1, 1, 1, 1]
    assert steps(591, 10) == [1] * 10
    assert steps(3349, 16) == [4] * 13 + [1, 0, 0]
    assert steps(6304, 16) == [7] * 14 + [1, 0]
    # rows_per_split is a multiple of 64, the splits tile [0, M) in order, and only trailing splits are empty
    for M, S in cases.CASES + [(M, S) for M, S, _ in cases.CLS_CASES]:
        geo = cases.geometry(M, S)
        assert len(geo) == S
        live = [g for g in geo if g[2]]
        assert geo[:len(live)] == live and live[0][0] == 0 and live[-1][1] == M
        assert all(a[1] == b[0] for a, b in zip(live, live[1:]))
        assert all((e - b) % 64 == 0 for b, e, _, _ in live[:-1])
        assert all(0 < t <= 64 and (e - b) == (n - 1) * 64 + t for b, e, n, t in live)


@pytest.mark.parametrize('form', sorted(FORMS))
def test_cases_reach_every_step_count_tail_and_split_edge(form):
    launches = _splits(form)
    live = [g for _, _, geo in launches for g in geo if g[2]]
    assert {n for _, _, n, _ in live} >= {1, 2, 3, 4, 5, 6, 7}
    tails = {t % 64 for _, _, _, t in live}
    assert 0 in tails                                    # full last step
    assert tails >= {1, 31, 33, 63}                      # partial last steps
    assert any(M == 1 for M, _, _ in launches)           # a one-row problem
    assert any(len({g[2] % 2 for g in geo if g[2]}) == 2 for _, _, geo in launches)       # both step parities in one grid
    assert any(geo[-1][2] == 0 for _, _, geo in launches)                                 # an empty trailing split
    assert any(S == 1 for _, S, _ in launches)
    # the stale-register-set and odd-last-step paths in a launch of several splits, not only with S == 1
    assert any(S > 1 and max(g[2] for g in geo) >= 5 for _, S, geo in launches)
    assert any(S > 1 and any(g[2] >= 3 and g[2] % 2 for g in geo) for _, S, geo in launches)


# every case of the list with what it is there for: steps per split, rows of the last step of the last live split
EXPECTED = {
    (1, 1): ([1], 1), (63, 1): ([1], 63), (64, 1): ([1], 64), (65, 1): ([2], 1), (129, 1): ([3], 1), (287, 1): ([5], 31),
    (353, 1): ([6], 33), (448, 1): ([7], 64), (191, 2): ([2, 1], 63), (192, 2): ([2, 1], 64), (193, 2): ([2, 2], 1),
    (320, 2): ([3, 2], 64), (321, 2): ([3, 3], 1), (449, 2): ([4, 4], 1), (833, 2): ([7, 7], 1), (895, 3): ([5, 5, 4], 63),
    (130, 4): ([1, 1, 1, 0], 2), (257, 4): ([2, 2, 1, 0], 1),
}


def test_no_case_has_left_the_list():
    """A case that is removed from (or changed in) the list fails here by name, whether or not the matrix above still holds."""
    assert len(cases.CASES) == len(set(cases.CASES))
    missing = sorted(set(EXPECTED) - set(cases.CASES))
    assert not missing, f'cases removed from wgrad_cases.CASES: {missing}'
    for (M, S), (steps, tail) in EXPECTED.items():
        geo = cases.geometry(M, S)
        assert [g[2] for g in geo] == steps, (M, S)
        assert [g for g in geo if g[2]][-1][3] == tail, (M, S)
    for M, S in cases.CASES:
        assert (M, S, 3) in cases.CLS_CASES or M <= 65          # the class-token launch runs the larger ones too


def test_class_token_and_patch_lists_are_the_stated_ones():
    small = [(M, S) for M, S, r in cases.CLS_CASES if r == cases.TOKENS]
    assert small == [(1, 1), (2, 1), (63, 1), (64, 1), (65, 1), (65, 2), (65, 4)]
    assert [g[2] for g in cases.geometry(65, 4)] == [1, 1, 0, 0]                          # two empty splits
    assert {(M, S) for M, S, r in cases.CLS_CASES if r == 3} >= {(173, 1), (173, 3), (256, 1), (256, 4)}
    assert all(M * r * 768 * 2 <= 20 * 2 ** 20 for M, _, r in cases.CLS_CASES)            # at most 20 MB per operand
    # PatchEmbed rows: M = batch * 196, so the last step holds 4, 8 or 12 rows and the tails of the matrix above cannot occur;
    # the step counts are the ones the list was chosen for
    steps = {(b, S): [g[2] for g in cases.geometry(b * 196, S)] for b, S in cases.PATCH_CASES}
    assert steps == {(1, 1): [4], (2, 1): [7], (2, 2): [4, 3], (3, 4): [3, 3, 3, 1], (1, 8): [1, 1, 1, 1, 0, 0, 0, 0]}
    assert {b * 196 % 64 for b, _ in cases.PATCH_CASES} == {4, 8, 12}


def test_integer_cases_are_exact_in_fp32():
    Ms = [M for M, _ in cases.CASES] + [M for M, _, _ in cases.CLS_CASES] + [b * 196 for b, _ in cases.PATCH_CASES]
    assert max(Ms) <= 896
    assert all(M * 2 * 3 < 2 ** 24 for M in Ms)
    # the affine un-fold (|gamma|, |beta| <= 2, |W| <= 1, N <= 768): |gamma G + beta db| <= 2 * 6 M + 2 * 2 M, |sum_n W G| <= 768 * 6 M
    assert all(2 * 6 * M + 2 * 2 * M < 2 ** 24 and 768 * 6 * M < 2 ** 24 for M in Ms)
    dY, A = cases.int_operands(65, 96, 192, 0)
    assert dY.dtype == A.dtype == torch.bfloat16
    assert int(dY.float().abs().max()) == 2 and int(A.float().abs().max()) == 3
    assert torch.equal(dY.float(), dY.float().round()) and torch.equal(A.float(), A.float().round())


def test_operand_makers_and_reference():
    dY, A = cases.int_operands(130, 96, 192, 1)
    p = cases.padded(dY)
    assert p.shape == (130 + 6 * 64, 96) and torch.equal(p[:130], dY) and bool(p[130:].isnan().all())
    s = cases.strided(A, 3)
    assert s.shape == (390, 192) and torch.equal(s[::3], A) and bool(s[1::3].isnan().all()) and bool(s[2::3].isnan().all())
    c = cases._chunks(A)
    assert torch.equal(cases._rows(c, 130), A)
    assert torch.equal(c.view(6, 130, 32)[4, 77], A[77, 128:160])
    slabs, colsums, G, cs = cases.reference(dY, A, 4)
    assert torch.equal(G, dY.double().t() @ A.double()) and torch.equal(cs, dY.double().sum(0))
    assert torch.equal(slabs[2], dY[128:130].double().t() @ A[128:130].double()) and not slabs[3].any() and not colsums[3].any()
    assert not torch.equal(G[:, :96], G[:, :96].t())                                      # asymmetric: a transposition shows
    dX, dy, images, col = cases.patch_operands(2, 96, 5)
    assert dX.shape == (2 * 197, 96) and bool(dX[0].isnan().all()) and bool(dX[197].isnan().all())
    assert torch.equal(dX.view(2, 197, 96)[:, 1:].reshape(392, 96), dy)
    assert col.shape == (392, 768) and float(images.abs().max()) == 3.0
