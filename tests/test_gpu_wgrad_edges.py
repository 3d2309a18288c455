"""Exact tests of the weight-gradient kernels (csrc/gemm.hip: wgrad_kernel, wgrad_reduce_batch_kernel) at every step count, tail and split
edge of the main loop, through the C ABI.

The loop is unrolled by two over 64-row steps with two register sets and a prefetch of up to four steps, clamps its loads to the last row
and zeroes the rows past a split's end in a partial-step branch.  With the engine's split counts the other kernel-level tests run ONE step per
workgroup; here the (M, S) cases of tests/wgrad_cases.py (proved by tests/test_wgrad_cases_cpu.py to reach 1..7 steps, full and partial
tails, mixed parities, empty splits) run through every instantiation the engine launches.  Operands are small integers in bf16, so every
partial sum is an integer below 2^24 and fp32 is exact in any order: all comparisons are ``torch.equal`` against an fp64 CPU reference,
per slab and after the reduce.  Workspaces start as NaN with a canary behind them, row-major operands have NaN rows behind them, strided
ones NaN rows between: an unwritten slab, a write past the workspace or a read past a split's rows shows.  The one tolerance in this file
is the randn bound of ``_assert_within_fp32_sum_bound``."""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_cases as cases  # noqa: E402

CANARY = 256
CANARY_BITS = 0x5CA1AB1E
ERR_SHAPE, ERR_ALIGN = -1, -2
U = 2.0 ** -24
NAN = float('nan')


def _native():
    from rovit_hip import native
    native.load()
    return native


def dev():
    return torch.device('cuda:0')


def arr(xs):
    return (C.c_int * len(xs))(*xs)


def _ids(cs):
    return ['-'.join(str(v) for v in c) for c in cs]


# ------------------------------------------------------------------ workspace, canary, checks ----------------
def _workspace(lib, N, K, S):
    n = lib.rovit_wgrad_workspace_bytes(N, K, S) // 4
    assert n == S * N * K + S * N
    ws = torch.full((n + CANARY,), NAN, device=dev())
    ws[n:].view(torch.int32).fill_(CANARY_BITS)
    return ws


def _slabs(ws, N, K, S):
    return ws[:S * N * K].view(S, N, K), ws[S * N * K:S * N * K + S * N].view(S, N)


def _assert_written_inside(ws, what):
    assert bool(torch.isfinite(ws[:-CANARY]).all()), f'{what}: a slab or colsum element was never written'
    assert bool((ws[-CANARY:].view(torch.int32) == CANARY_BITS).all()), f'{what}: write past the workspace'


def _assert_untouched(ws, what):
    assert bool(torch.isnan(ws[:-CANARY]).all()), f'{what}: the workspace was written'
    assert bool((ws[-CANARY:].view(torch.int32) == CANARY_BITS).all()), f'{what}: write past the workspace'


def _reduce(native, ws, N, K, S):
    dW, db = torch.full((N, K), NAN, device=dev()), torch.full((N,), NAN, device=dev())
    native.call('rovit_wgrad_reduce', native.ptr(ws), S, N, K, None, None, None, native.ptr(dW), native.ptr(db), None, None, None,
                native.stream_ptr())
    return dW.cpu(), db.cpu()


def _assert_exact(native, ws, N, K, S, ref, what):
    """(a) every slab and colsum row equals its split's reference (empty splits: zeros), (b) the reduce gives the totals"""
    _assert_written_inside(ws, what)
    slabs, colsums = _slabs(ws, N, K, S)
    r_slabs, r_colsums, r_G, r_cs = ref
    got_s, got_c = slabs.cpu(), colsums.cpu()
    for s in range(S):
        assert torch.equal(got_s[s], r_slabs[s].float()), f'{what}: slab {s}'
        assert torch.equal(got_c[s], r_colsums[s].float()), f'{what}: colsum {s}'
    dW, db = _reduce(native, ws, N, K, S)
    assert torch.equal(dW, r_G.float()), f'{what}: dW'
    assert torch.equal(db, r_cs.float()), f'{what}: db'


def _assert_same_bits(a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{what}: two launches differ'


def _assert_within_fp32_sum_bound(got, ref, absb, n_terms, what, factor=2.0):
    """The one tolerance of this file.  A sum of n products in fp32, in ANY order, with round-to-nearest adds, is within
    (n - 1) u sum|terms| of the exact sum to first order, u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2);
    the bf16 x bf16 products themselves are exact in fp32.  Here n = M + S (M rows, then S slabs), the bound is elementwise with
    |dY|^T |A| in fp64, and it is DOUBLED (factor 2) for the one thing not derived: whether the matrix core's internal adds round to
    nearest or truncate (u = 2^-23).  Measured figures: docstring of test_randn_operands_stay_within_the_fp32_sum_bound."""
    bound = n_terms * U * absb
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f'{what}: worst |err| / ((M + S) u |dY|^T|A|) = {ratio:.4f} (allowed {factor})')
    assert bool((err <= factor * bound).all()), f'{what}: ratio {ratio}'


# ------------------------------------------------------------------ operand placement ------------------------
def _place(t, how):
    """CPU operand -> (device allocation whose first element is the operand's, ld): 'row' = row-major with NaN rows behind, 'blk' =
    chunk-major (no pad possible: the chunk stride is M * 32), an int r = every r-th row of a NaN-filled allocation"""
    if how == 'row':
        return cases.padded(t).to(dev()), t.shape[1]
    if how == 'blk':
        return cases._chunks(t).to(dev()), t.shape[1]
    return cases.strided(t, how).to(dev()), t.shape[1] * how


def _launch_single(native, dY, A, M, N, K, S, patch_tokens=0):
    ws = _workspace(native.load(), N, K, S)
    native.call('rovit_wgrad', native.ptr(dY), N, native.ptr(A), K, M, N, K, S, patch_tokens, native.ptr(ws), native.stream_ptr())
    return ws


def _launch_multi(native, shapes, dys, ldys, As, ldas, M, S, a_blk=None, y_blk=None):
    lib = native.load()
    wss = [_workspace(lib, n, k, S) for n, k in shapes]
    args = (native.ptr_array(dys), arr(ldys), native.ptr_array(As), arr(ldas), arr([n for n, _ in shapes]), arr([k for _, k in shapes]),
            native.ptr_array(wss))
    if a_blk is None:
        native.call('rovit_wgrad_multi', *args, len(shapes), M, S, native.stream_ptr())
    else:
        native.call('rovit_wgrad_multi_ex', *args, arr(a_blk), arr(y_blk), len(shapes), M, S, native.stream_ptr())
    return wss


def _multi_operands(shapes, M, y_how, a_how, maker=cases.int_operands):
    """problem j of a launch: seed j, dY placed as y_how[j], A as a_how[j]"""
    dys, ldys, As, ldas = [], [], [], []
    for j, (N, K) in enumerate(shapes):
        dY, A = maker(M, N, K, j)
        y, ldy = _place(dY, y_how[j])
        a, lda = _place(A, a_how[j])
        dys.append(y), ldys.append(ldy), As.append(a), ldas.append(lda)
    return dys, ldys, As, ldas


def _blk(how):
    return [int(h == 'blk') for h in how]


def _run_multi_exact(native, shapes, M, S, y_how, a_how, ex, what):
    ops = _multi_operands(shapes, M, y_how, a_how)
    blk = (_blk(a_how), _blk(y_how)) if ex else (None, None)
    first = _launch_multi(native, shapes, *ops, M, S, *blk)
    again = _launch_multi(native, shapes, *ops, M, S, *blk)
    for j, (N, K) in enumerate(shapes):
        _assert_exact(native, first[j], N, K, S, cases.int_reference(M, N, K, S, j), f'{what} problem {j} ({N}, {K})')
        _assert_same_bits(first[j], again[j], f'{what} problem {j}')          # (c)
    return first


# ------------------------------------------------------------------ 1. single problem, <96, 96> --------------
@pytest.mark.parametrize('M,S', cases.CASES, ids=_ids(cases.CASES))
def test_single_problem_every_slab_and_total_is_exact(M, S):
    """rovit_wgrad, wgrad_kernel<96, 96>: 1 to 8 k-tiles (colsum ownership), 1 to 6 n-tiles"""
    native = _native()
    for N, K in cases.SINGLE_SHAPES:
        dY, A = cases.int_operands(M, N, K, 0)
        (y, _), (a, _) = _place(dY, 'row'), _place(A, 'row')
        ref = cases.int_reference(M, N, K, S, 0)
        first = _launch_single(native, y, a, M, N, K, S)
        _assert_exact(native, first, N, K, S, ref, f'wgrad ({N}, {K})')
        _assert_same_bits(first, _launch_single(native, y, a, M, N, K, S), f'wgrad ({N}, {K})')


# ------------------------------------------------------------------ 2. merged launch, <192, 192, WN = 4> -----
ROW4 = ['row'] * 4
MERGED = {                      # name: (problems, dY layouts, A layouts, through rovit_wgrad_multi_ex)
    'n4_row_major': (cases.BLOCK_PROBLEMS, ROW4, ROW4, True),
    'n4_mlp_chunk_major': (cases.BLOCK_PROBLEMS, ['row', 'blk', 'row', 'row'], ['blk', 'row', 'row', 'row'], True),     # a_blk fc2, y_blk fc1
    'n3_row_major': (cases.BLOCK_PROBLEMS[:3], ROW4[:3], ROW4[:3], False),
    'n2_mlp_chunk_major': (cases.BLOCK_PROBLEMS[:2], ['row', 'blk'], ['blk', 'row'], True),
}


@pytest.mark.parametrize('layout', sorted(MERGED))
@pytest.mark.parametrize('M,S', cases.CASES, ids=_ids(cases.CASES))
def test_merged_launch_every_problem_slab_and_total_is_exact(M, S, layout):
    """The per-block launch of rovit_vit_backward (fc2, fc1, proj, qkv in one grid of eight-wave workgroups), row-major and in the
    one-launch MLP layout (act and dpre chunk-major: a row taken from the neighbouring chunk is a wrong integer), and with 2 and 3 problems"""
    shapes, y_how, a_how, ex = MERGED[layout]
    _run_multi_exact(_native(), shapes, M, S, y_how, a_how, ex, f'merged {layout}')


@pytest.mark.parametrize('M,S', cases.CASES, ids=_ids(cases.CASES))
def test_lone_qkv_flush_equals_its_slabs_in_the_merged_launch(M, S):
    """rovit_wgrad_multi with n = 1 (96 x 96 tiles) is documented as bit-identical to the same problem inside the merged launch"""
    native = _native()
    merged = _launch_multi(native, cases.BLOCK_PROBLEMS, *_multi_operands(cases.BLOCK_PROBLEMS, M, ROW4, ROW4), M, S, [0] * 4, [0] * 4)
    N, K = cases.QKV
    dY, A = cases.int_operands(M, N, K, 3)
    (y, _), (a, _) = _place(dY, 'row'), _place(A, 'row')
    lone, = _launch_multi(native, [cases.QKV], [y], [N], [a], [K], M, S)
    _assert_exact(native, lone, N, K, S, cases.int_reference(M, N, K, S, 3), 'lone qkv')
    _assert_written_inside(merged[3], 'merged qkv')
    _assert_same_bits(lone, merged[3], 'lone qkv against merged')


# ------------------------------------------------------------------ 3. class-token launch --------------------
@pytest.mark.parametrize('M,S,stride', cases.CLS_CASES, ids=_ids(cases.CLS_CASES))
def test_class_token_launch_with_strided_rows_is_exact(M, S, stride):
    """fc2, fc1 and proj of the class-token block: M = the batch, operand row m is row m * stride of the token matrix; every row between
    holds NaN"""
    shapes = cases.BLOCK_PROBLEMS[:3]
    _run_multi_exact(_native(), shapes, M, S, [stride] * 3, [stride] * 3, False, f'class-token stride {stride}')


# ------------------------------------------------------------------ 4. patch rows ----------------------------
def _images_on_device(images):
    buf = torch.full((images.shape[0] + 1,) + tuple(images.shape[1:]), NAN)       # one NaN image behind the batch
    buf[:-1] = images
    return buf.to(dev())


def _launch_patch_pair(native, dX, images, col, batch, N, S):
    lib = native.load()
    M = batch * (cases.TOKENS - 1)
    x, _ = _place(dX, 'row')
    c, _ = _place(col, 'row')
    img = _images_on_device(images)
    ws_col = _launch_single(native, x, c, M, N, 768, S, patch_tokens=cases.TOKENS)
    ws_img = _workspace(lib, N, 768, S)
    native.call('rovit_patch_embed_wgrad', native.ptr(x), N, native.ptr(img), batch, cases.TOKENS, N, S, native.ptr(ws_img),
                native.stream_ptr())
    return ws_col, ws_img


_PATCH_REF = {}


@pytest.mark.parametrize('N', [192, 96])
@pytest.mark.parametrize('batch,S', cases.PATCH_CASES, ids=_ids(cases.PATCH_CASES))
def test_patch_rows_column_buffer_and_image_gather_are_exact_and_identical(batch, S, N):
    """rovit_wgrad(patch_tokens = 197) on an im2col buffer (<96, 96, PATCH>) and rovit_patch_embed_wgrad on the fp32 images
    (<192, 96, PATCH, IMG> at N = 192, <96, 96, PATCH, IMG> at N = 96): dY row of patch row m is m + m / 196 + 1, the class-token rows
    between hold NaN"""
    native = _native()
    dX, dy, images, col = cases.patch_operands(batch, N, 7)
    if (batch, N, S) not in _PATCH_REF:
        _PATCH_REF[batch, N, S] = cases.reference(dy, col, S)
    ref = _PATCH_REF[batch, N, S]
    ws_col, ws_img = _launch_patch_pair(native, dX, images, col, batch, N, S)
    _assert_exact(native, ws_col, N, 768, S, ref, 'patch rows, column buffer')
    _assert_exact(native, ws_img, N, 768, S, ref, 'patch rows, image gather')
    _assert_same_bits(ws_col, ws_img, 'image gather against column buffer')
    again = _launch_patch_pair(native, dX, images, col, batch, N, S)
    _assert_same_bits(ws_col, again[0], 'patch rows, column buffer')
    _assert_same_bits(ws_img, again[1], 'patch rows, image gather')


# ------------------------------------------------------------------ 5. affine un-fold in the reduce ----------
@pytest.mark.parametrize('N,K', [cases.FC1, cases.QKV], ids=['fc1', 'qkv'])
@pytest.mark.parametrize('M,S', [(448, 1), (320, 2), (130, 4)], ids=['one_split', 'mixed_parity', 'empty_split'])
def test_reduce_unfolds_the_layernorm_affine_exactly(M, S, N, K):
    """W_f = W gamma, b_f = b + W beta  =>  dW = gamma G + db (x) beta, dgamma = sum_n W G, dbeta = sum_n W db.  Integer gamma, beta in
    [-2, 2] and W in {-1, 0, 1}: every intermediate is an integer below 2^24 (tests/test_wgrad_cases_cpu.py), so fp32 and its fmaf are exact"""
    native = _native()
    assert (M, S) in cases.CASES
    dY, A = cases.int_operands(M, N, K, 0)
    (y, _), (a, _) = _place(dY, 'row'), _place(A, 'row')
    ws = _launch_single(native, y, a, M, N, K, S)
    g = torch.Generator(device='cpu').manual_seed(11)
    gamma, beta = (torch.randint(-2, 3, (K,), generator=g).float() for _ in range(2))
    W = torch.randint(-1, 2, (N, K), generator=g).float()
    out = {k: torch.full(s, NAN, device=dev()) for k, s in (('dW', (N, K)), ('db', (N,)), ('dgamma', (K,)), ('dbeta', (K,)), ('gs', (N, K)))}
    d = lambda t: t.to(dev())
    gam_d, bet_d, W_d = d(gamma), d(beta), d(W)
    native.call('rovit_wgrad_reduce', native.ptr(ws), S, N, K, native.ptr(gam_d), native.ptr(bet_d), native.ptr(W_d), native.ptr(out['dW']),
                native.ptr(out['db']), native.ptr(out['dgamma']), native.ptr(out['dbeta']), native.ptr(out['gs']), native.stream_ptr())
    _assert_written_inside(ws, 'un-fold')
    _, _, G, cs = cases.int_reference(M, N, K, S, 0)
    Wd, gd, bd = W.double(), gamma.double(), beta.double()
    assert torch.equal(out['db'].cpu(), cs.float())
    assert torch.equal(out['dW'].cpu(), (gd * G + cs[:, None] * bd).float())
    assert torch.equal(out['dgamma'].cpu(), (Wd * G).sum(0).float())
    assert torch.equal(out['dbeta'].cpu(), (Wd * cs[:, None]).sum(0).float())


# ------------------------------------------------------------------ 6. precision ------------------------------
def _randn_multi(native, shapes, y_how, a_how, ex, what):
    M, S = cases.RANDN_CASE
    ops = _multi_operands(shapes, M, y_how, a_how, maker=cases.randn_operands)
    wss = _launch_multi(native, shapes, *ops, M, S, *((_blk(a_how), _blk(y_how)) if ex else (None, None)))
    for j, (N, K) in enumerate(shapes):
        _check_randn(native, wss[j], *cases.randn_operands(M, N, K, j), S, f'{what} problem {j} ({N}, {K})')


def _check_randn(native, ws, dY, A, S, what):
    _assert_written_inside(ws, what)
    (M, N), K = dY.shape, A.shape[1]
    _, _, G, cs = cases.reference(dY, A, S)
    absG, abscs = cases.abs_bound(dY, A)
    dW, db = _reduce(native, ws, N, K, S)
    _assert_within_fp32_sum_bound(dW, G, absG, M + S, what + ' dW')
    _assert_within_fp32_sum_bound(db, cs, abscs, M + S, what + ' db')


@pytest.mark.parametrize('form', ['single', 'merged_row_major', 'merged_mlp_chunk_major', 'class_token', 'patch'])
def test_randn_operands_stay_within_the_fp32_sum_bound(form):
    """Integer operands cannot show an accumulator that is lossy but still exact on small integers: normal operands at (M, S) = (833, 2)
    (7 and 7 steps; the patch kernels at batch 4, M = 784: 7 and 6 steps), dW and db after the reduce against fp64, elementwise within
    2 (M + S) 2^-24 |dY|^T |A| (_assert_within_fp32_sum_bound).  Measured on the MI355X, worst ratio to the UNDOUBLED bound: dW 0.0016
    (merged and class-token launches, proj), 0.0010 to 0.0013 for every other problem and form, db 0.0001: rounding errors of random
    signs grow like sqrt(n), the bound like n.  The constant used is the derived 2; nothing was fitted to these figures."""
    native = _native()
    M, S = cases.RANDN_CASE
    if form == 'single':
        for N, K in cases.SINGLE_SHAPES:
            dY, A = cases.randn_operands(M, N, K, 0)
            ws = _launch_single(native, _place(dY, 'row')[0], _place(A, 'row')[0], M, N, K, S)
            _check_randn(native, ws, dY, A, S, f'wgrad ({N}, {K})')
    elif form == 'merged_row_major':
        _randn_multi(native, *MERGED['n4_row_major'], 'merged row-major')
    elif form == 'merged_mlp_chunk_major':
        _randn_multi(native, *MERGED['n4_mlp_chunk_major'], 'merged chunk-major')
    elif form == 'class_token':
        _randn_multi(native, cases.BLOCK_PROBLEMS[:3], [3] * 3, [3] * 3, False, 'class-token')
    else:
        batch, S = cases.RANDN_PATCH_CASE
        for N in (192, 96):
            dX, dy, images, col = cases.patch_operands(batch, N, 9, integer=False)
            ws_col, ws_img = _launch_patch_pair(native, dX, images, col, batch, N, S)
            _assert_same_bits(ws_col, ws_img, 'image gather against column buffer')
            _check_randn(native, ws_col, dy, col, S, f'patch rows N = {N}, column buffer')
            _check_randn(native, ws_img, dy, col, S, f'patch rows N = {N}, image gather')


# ------------------------------------------------------------------ 7. arguments ------------------------------
def test_bad_arguments_return_their_error_code_without_a_launch():
    native = _native()
    lib = native.load()
    M, S = 130, 2
    sp = native.stream_ptr()
    ops = _multi_operands(cases.BLOCK_PROBLEMS, M, ROW4, ROW4)
    dys, ldys, As, ldas = ops

    def multi(shapes, ldys_, n, splits):
        k = len(shapes)
        wss = [_workspace(lib, N, K, max(splits, 1)) for N, K in shapes]
        rc = lib.rovit_wgrad_multi(native.ptr_array((dys * 2)[:k]), arr(ldys_), native.ptr_array((As * 2)[:k]), arr([K for _, K in shapes]),
                                   arr([N for N, _ in shapes]), arr([K for _, K in shapes]), native.ptr_array(wss), n, M, splits, sp)
        torch.cuda.synchronize()
        for ws in wss:
            _assert_untouched(ws, f'wgrad_multi n = {n}, splits = {splits}')
        return rc

    # a two-problem launch needs 192-wide tiles: N = 96 has none (operands of (192, 768) and (768, 192) hold more than (96, 192) reads)
    assert multi([(96, 192), (96, 192)], [96, 96], 2, S) == ERR_SHAPE
    assert multi([(192, 192), (192, 192)], [192 + 4, 192], 2, S) == ERR_ALIGN
    assert multi([(192, 192), (192, 192)], [192, 192], 2, 0) == ERR_SHAPE
    assert multi([(192, 192)] * 5, [192] * 5, 5, S) < 0
    # the single-problem entry points
    N, K = 192, 192
    for fn_args, want in (((N + 4, K, S), ERR_ALIGN), ((N, K + 4, S), ERR_ALIGN), ((N, K, 0), ERR_SHAPE)):
        ldy, lda, splits = fn_args
        ws = _workspace(lib, N, K, max(splits, 1))
        assert lib.rovit_wgrad(native.ptr(dys[2]), ldy, native.ptr(As[2]), lda, M, N, K, splits, 0, native.ptr(ws), sp) == want
        torch.cuda.synchronize()
        _assert_untouched(ws, f'wgrad ldy = {ldy}, lda = {lda}, splits = {splits}')
    dX, dy, images, col = cases.patch_operands(1, 96, 7)
    x, img = _place(dX, 'row')[0], _images_on_device(images)
    for ldy, splits, want in ((96 + 4, S, ERR_ALIGN), (96, 0, ERR_SHAPE)):
        ws = _workspace(lib, 96, 768, max(splits, 1))
        assert lib.rovit_patch_embed_wgrad(native.ptr(x), ldy, native.ptr(img), 1, cases.TOKENS, 96, splits, native.ptr(ws), sp) == want
        torch.cuda.synchronize()
        _assert_untouched(ws, f'patch_embed_wgrad ldy = {ldy}, splits = {splits}')
