"""Round-3 GPU tests: the fused MLP half of a block (mlp_fused.hip) against the two-launch path it replaces and against a plain
PyTorch fp32 reference of the same op, called through the C ABI; the fused path inside the backbone forward."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu  # noqa: E402  (checker only)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wgrad_cases import _chunks, _rows  # noqa: E402  (chunk-major [24][M][32] <-> row-major (M,768))


def _native():
    from rovit_hip import native
    native.load()
    return native


def dev():
    return torch.device('cuda:0')


def bf(x):
    return x.to(torch.bfloat16)


def _mlp_problem(M, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    xhat2 = bf(r(M, 192)).to(dev())
    w1 = bf(r(768, 192) * 0.08).to(dev())          # fc1 weight, LayerNorm affine already folded in
    w2 = bf(r(192, 768) * 0.05).to(dev())
    b1 = (r(768) * 0.3).to(dev())
    b2 = (r(192) * 0.3).to(dev())
    X0 = (r(M, 192) * 2).to(dev())
    return xhat2, w1, w2, b1, b2, X0


def _two_launch(native, xhat2, w1, w2, b1, b2, X0, keep=True):
    M = xhat2.shape[0]
    act = torch.empty(M, 768, device=dev(), dtype=torch.bfloat16)
    dact = torch.empty_like(act)
    native.call('rovit_gemm_nt', native.ptr(xhat2), 192, native.ptr(w1), 192, M, 768, 192, native.ptr(b1), 1, native.ptr(act), 768,
                native.ptr(dact), None, 0, None, 0, None, 0, native.stream_ptr())
    X = X0.clone()
    xhat = torch.empty(M, 192, device=dev(), dtype=torch.bfloat16)
    rstd = torch.empty(M, device=dev())
    native.call('rovit_gemm_resid_ln', native.ptr(act), 768, native.ptr(w2), 768, M, 768, native.ptr(b2), native.ptr(X), native.ptr(xhat),
                native.ptr(rstd), 1e-6, native.stream_ptr())
    return act, dact, X, xhat, rstd


KNOB_MLP_SCHEDULE = 8          # csrc/common.h RovitKnob: the schedules that lost live in the developer library only


def _set_schedule(native, waves):
    """10 = the product's schedule (nothing to set); 4 / 8 / 9 need the developer library (ROVIT_HIP_LIB=.../librovit_hip_dev.so)."""
    lib = native.load()
    if hasattr(lib, 'rovit_dev_set_knob'):
        lib.rovit_dev_set_knob(KNOB_MLP_SCHEDULE, waves, 0)
    elif waves != 10:
        pytest.skip('schedule %d is compiled into the developer library only' % waves)


def _fused(native, xhat2, w1, w2, b1, b2, X0, mode=2, ln=True, waves=None):
    M = xhat2.shape[0]
    if waves is not None:
        _set_schedule(native, waves)
    ws = torch.empty(native.load().rovit_mlp_stream_bytes(), dtype=torch.uint8, device=dev())
    native.call('rovit_mlp_prepare_stream', native.ptr(w1), native.ptr(w2), native.ptr(ws), native.stream_ptr())
    # poisoned outputs: a row or column the kernel fails to write shows up as NaN
    act = torch.full((M, 768), float('nan'), device=dev(), dtype=torch.bfloat16) if mode >= 1 else None
    dact = torch.full((M, 768), float('nan'), device=dev(), dtype=torch.bfloat16) if mode == 2 else None
    X = X0.clone()
    xhat = torch.full((M, 192), float('nan'), device=dev(), dtype=torch.bfloat16) if ln else None
    rstd = torch.full((M,), float('nan'), device=dev()) if ln else None
    native.call('rovit_mlp_fused_fwd', native.ptr(xhat2), native.ptr(ws), native.ptr(b1), native.ptr(b2), native.ptr(act), native.ptr(dact),
                native.ptr(X), native.ptr(xhat), native.ptr(rstd), 1e-6, M, M, native.stream_ptr())
    # the kept activations are chunk-major: back to rows for the comparisons (a chunk the kernel failed to write stays NaN)
    return (_rows(act, M) if act is not None else None), (_rows(dact, M) if dact is not None else None), X, xhat, rstd


@pytest.mark.parametrize('waves', [4, 8, 9, 10])   # 8 = lockstep, 9 = waves 4-7 staggered by half a chunk, 10 = in-wave pipeline + GELU table
@pytest.mark.parametrize('M', [1, 5, 129, 197, 256, 257, 591, 1000, 3 * 197 * 4, 256 * 197])
def test_fused_mlp_half_equals_the_two_launch_path_and_a_torch_reference(M, waves):
    """rovit_mlp_fused_fwd = rovit_gemm_nt(EPI_GELU) + rovit_gemm_resid_ln in one launch.  act and gelu' must be BIT-IDENTICAL to the
    two-launch path (same MFMA, same k order, same bf16-staged pre-activation); X and the LayerNorm outputs agree to the
    fp32 summation order of fc2 (one chain over the 768 hidden units here, two half-sums in the K = 768 kernel), i.e. to an
    occasional neighbouring-bf16 rounding of the branch output.  Ragged M: rows beyond M are neither read nor written."""
    native = _native()
    prob = _mlp_problem(M, 100 + M)
    a0, d0, X0, h0, r0 = _two_launch(native, *prob)
    a1, d1, X1, h1, r1 = _fused(native, *prob, waves=waves)
    _set_schedule(native, 10)     # the library default
    assert torch.equal(a0.view(torch.int16), a1.view(torch.int16))
    assert torch.equal(d0.view(torch.int16), d1.view(torch.int16))
    xhat2, w1, w2, b1, b2, Xin = prob
    branch = bf(a1.float() @ w2.float().t() + b2).float()              # the staged (bf16) branch output
    ref_x = Xin + branch
    scale = float(branch.abs().max())
    assert float((X1 - ref_x).abs().max()) < 2 ** -7 * max(scale, 1.0)           # one bf16 ulp of the branch output
    assert float((X1 - X0).abs().max()) < 2 ** -7 * max(scale, 1.0) and float((X1 - X0).abs().mean()) < 1e-4
    ref_h = torch.nn.functional.layer_norm(X1, (192,), eps=1e-6)        # statistics of the rows the kernel wrote
    assert float((h1.float() - ref_h).abs().max()) < 2e-2
    assert float(((r1 - 1 / torch.sqrt(X1.var(1, unbiased=False) + 1e-6)).abs() / r1.abs()).max()) < 1e-5
    # against torch's own GELU (the kernels use the A&S 7.1.26 erf): the existing stated tolerances
    pre = (xhat2.float() @ w1.float().t() + b1).requires_grad_(True)
    ref_act = torch.nn.functional.gelu(pre)
    ref_act.sum().backward()
    assert float((a1.float() - ref_act.detach()).abs().max()) < 3e-2
    assert float((d1.float() - pre.grad).abs().max()) < 1e-2


@pytest.mark.parametrize('M', [64, 700])
def test_pipelined_mlp_half_gelu_table_and_its_fallback_on_special_inputs(M):
    """The pipelined forward looks gelu / gelu' up in a table of the bf16 input patterns 2^-24 <= |x| < 16 and falls back to the
    formula (wave-uniform branch) elsewhere.  Drive pre-activations onto the table's edges and beyond: zero weights with biases
    set to exact zeros, +-2^-24 (first entry), values below it, +-16 (first value above), huge values, and ordinary ones -- act and
    gelu' must stay BIT-IDENTICAL to the two-launch kernels, which evaluate the formula for every element."""
    native = _native()
    xhat2, w1, w2, b1, b2, X0 = _mlp_problem(M, 900 + M)
    w1 = torch.zeros_like(w1)                    # pre-activation = bias exactly
    special = torch.tensor([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -30, 1e-38, 15.9375, -15.9375, 16.0, -16.0, 40.0, -40.0, 3e4,
                            -3e4, 1.0, -1.0, 0.5, 2.0 ** -23, 2.0 ** -10, -2.0 ** -10, 7.96875, 1e-45, -1e-45], device=dev())
    b1 = special[torch.arange(768, device=dev()) % special.numel()].clone()
    b1[400:] = (torch.randn(368, device=dev()) * 3)          # and a block of ordinary values
    prob = (xhat2, w1, w2, b1, b2, X0)
    a0, d0, Xr, h0, r0 = _two_launch(native, *prob)
    a1, d1, X1, h1, r1 = _fused(native, *prob, waves=10)
    _set_schedule(native, 10)
    assert torch.equal(a0.view(torch.int16), a1.view(torch.int16))
    assert torch.equal(d0.view(torch.int16), d1.view(torch.int16))
    assert bool(torch.isfinite(X1).all())
    # mixed case: real weights, a few bias columns special (most waves take the table, some the fallback)
    xhat2, w1, w2, b1, b2, X0 = _mlp_problem(M, 901 + M)
    w1[::7] = 0
    b1[::7] = special[torch.arange(0, 768, 7, device=dev()) % special.numel()]
    prob = (xhat2, w1, w2, b1, b2, X0)
    a0, d0, Xr, h0, r0 = _two_launch(native, *prob)
    a1, d1, X1, h1, r1 = _fused(native, *prob, waves=10)
    _set_schedule(native, 10)
    assert torch.equal(a0.view(torch.int16), a1.view(torch.int16))
    assert torch.equal(d0.view(torch.int16), d1.view(torch.int16))
    assert float((X1 - Xr).abs().max()) < 2 ** -7 * max(float((X1 - X0).abs().max()), 1.0)


@pytest.mark.parametrize('M', [1, 77, 256, 257, 1000, 197 * 20, 256 * 197])
@pytest.mark.parametrize('train', [True, False])
def test_block_tail_equals_proj_plus_mlp_half_and_a_torch_reference(M, train):
    """rovit_block_tail_fwd = proj + residual + norm2 + MLP + residual + next norm1 in ONE launch, the residual stream held in fp32
    registers between the halves.  Against the chain rovit_gemm_resid_ln (proj) -> rovit_mlp_fused_fwd it differs only by what those
    stage through bf16 (the two branch outputs), i.e. X agrees to about one bf16 ulp of a branch output, and the LayerNorm outputs to a
    neighbouring bf16 value; against a plain fp32 torch computation on the same bf16 operands it is the CLOSER of the two."""
    native = _native()
    g = torch.Generator(device='cpu').manual_seed(7000 + M)
    r = lambda *s: torch.randn(*s, generator=g)
    o = bf(r(M, 192)).to(dev())
    wp = bf(r(192, 192) * 0.07).to(dev())
    bp_ = (r(192) * 0.2).to(dev())
    _, w1, w2, b1, b2, X0 = _mlp_problem(M, 7100 + M)
    p, sp = native.ptr, native.stream_ptr()
    lib = native.load()
    # chain of the two existing launches
    Xa = X0.clone()
    xh2a = torch.empty(M, 192, device=dev(), dtype=torch.bfloat16)
    r2a = torch.empty(M, device=dev())
    native.call('rovit_gemm_resid_ln', p(o), 192, p(wp), 192, M, 192, p(bp_), p(Xa), p(xh2a), p(r2a), 1e-6, sp)
    acta, dacta, Xa2, xh1a, r1a = _fused(native, xh2a, w1, w2, b1, b2, Xa)
    # one launch
    nanb2 = lambda *s: torch.full(s, float('nan'), device=dev(), dtype=torch.bfloat16)
    ws = torch.empty(lib.rovit_mlp_stream_bytes(), dtype=torch.uint8, device=dev())
    wq = bf(r(576, 192) * 0.07).to(dev())              # the NEXT block's qkv weight (norm1 affine folded in) and bias
    bq = (r(576) * 0.2).to(dev())
    native.call('rovit_mlp_prepare_stream_tail', p(w1), p(w2), p(wp), p(wq), p(ws), sp)
    qkv = nanb2(M, 576)
    nanb = nanb2
    X = X0.clone()
    xh2, r2 = (nanb(M, 192), torch.full((M,), float('nan'), device=dev())) if train else (None, None)
    act, dact = (nanb(M, 768), nanb(M, 768)) if train else (None, None)
    xh1, r1 = nanb(M, 192), torch.full((M,), float('nan'), device=dev())
    native.call('rovit_block_tail_fwd', p(o), p(ws), p(bp_), p(b1), p(b2), p(X), p(xh2), p(r2), p(act), p(dact), p(xh1), p(r1), p(bq), p(qkv),
                1e-6, M, M, sp)
    # the next block's qkv projection of the normalised rows: bit-identical to the library GEMM on this launch's own xhat_out
    qkv_chk = torch.empty(M, 576, device=dev(), dtype=torch.bfloat16)
    native.call('rovit_gemm_nt', p(xh1), 192, p(wq), 192, M, 576, 192, p(bq), 0, p(qkv_chk), 576, None, None, 0, None, 0, None, 0, sp)
    assert torch.equal(qkv.view(torch.int16), qkv_chk.view(torch.int16))
    # and without the qkv phase (qkv_next = NULL) everything else is unchanged
    Xn, xh1n, r1n = X0.clone(), nanb(M, 192), torch.full((M,), float('nan'), device=dev())
    native.call('rovit_block_tail_fwd', p(o), p(ws), p(bp_), p(b1), p(b2), p(Xn), None, None, None, None, p(xh1n), p(r1n), None, None, 1e-6, M, M, sp)
    assert torch.equal(Xn, X) and torch.equal(xh1n.view(torch.int16), xh1.view(torch.int16)) and torch.equal(r1n, r1)
    # fp32 reference on the same bf16 operands (xhat2 rounded to bf16 where the kernels round it)
    Xm = X0 + o.float() @ wp.float().t() + bp_
    ln = lambda t: torch.nn.functional.layer_norm(t, (192,), eps=1e-6)
    xh2_ref = bf(ln(Xm))
    pre = bf(xh2_ref.float() @ w1.float().t() + b1).float()
    act_ref = torch.nn.functional.gelu(pre)
    Xf = Xm + bf(act_ref).float() @ w2.float().t() + b2
    br = float((Xf - X0).abs().max())
    assert bool(torch.isfinite(X).all()) and bool(torch.isfinite(xh1.float()).all())
    e_new, e_old = float((X - Xf).abs().max()), float((Xa2 - Xf).abs().max())
    print('block tail: max |X - fp32 reference|', e_new, 'two launches', e_old, 'branch scale', br)
    assert e_new < 2 ** -7 * max(br, 1.0)                       # a bf16 ulp of the branch sum: GELU rounding flips of single hidden units
    assert float((X - Xa2).abs().max()) < 2 ** -6 * max(br, 1.0)
    assert float((xh1.float() - ln(X)).abs().max()) < 2e-2
    assert float(((r1 - 1 / torch.sqrt(X.var(1, unbiased=False) + 1e-6)).abs() / r1.abs()).max()) < 1e-5
    if train:
        assert float((xh2.float() - ln(Xm)).abs().max()) < 2e-2 and float((xh2.float() - xh2a.float()).abs().max()) < 4e-2
        assert float(((r2 - 1 / torch.sqrt(Xm.var(1, unbiased=False) + 1e-6)).abs() / r2.abs()).max()) < 1e-4
        a_rows, d_rows = _rows(act, M), _rows(dact, M)
        # the kept activations are those of the xhat2 THIS launch normalised: recompute them from its own xhat2 with the two-launch GELU kernel
        a_chk = torch.empty(M, 768, device=dev(), dtype=torch.bfloat16)
        d_chk = torch.empty_like(a_chk)
        native.call('rovit_gemm_nt', p(xh2), 192, p(w1), 192, M, 768, 192, p(b1), 1, p(a_chk), 768, p(d_chk), None, 0, None, 0, None, 0, sp)
        assert torch.equal(a_rows.view(torch.int16), a_chk.view(torch.int16)) and torch.equal(d_rows.view(torch.int16), d_chk.view(torch.int16))


def test_fused_mlp_half_on_row_ranges_of_one_chunk_major_tensor():
    """rovit_vit_forward runs the two half-batches as two launches that write row ranges of ONE chunk-major act / gelu' pair
    (pointers advanced by first_row x 32 elements, act_rows = rows of the whole): together they must equal one whole-batch launch."""
    native = _native()
    M, M0 = 700, 353
    xhat2, w1, w2, b1, b2, X0 = _mlp_problem(M, 4242)
    a_ref, d_ref, X_ref, h_ref, r_ref = _fused(native, xhat2, w1, w2, b1, b2, X0)
    ws = torch.empty(native.load().rovit_mlp_stream_bytes(), dtype=torch.uint8, device=dev())
    p, sp = native.ptr, native.stream_ptr()
    native.call('rovit_mlp_prepare_stream', p(w1), p(w2), p(ws), sp)
    act = torch.full((M, 768), float('nan'), device=dev(), dtype=torch.bfloat16)
    dact = torch.full((M, 768), float('nan'), device=dev(), dtype=torch.bfloat16)
    X, xhat, rstd = X0.clone(), torch.empty(M, 192, device=dev(), dtype=torch.bfloat16), torch.empty(M, device=dev())
    for r0, n in ((0, M0), (M0, M - M0)):
        native.call('rovit_mlp_fused_fwd', p(xhat2[r0:]), p(ws), p(b1), p(b2), act.data_ptr() + r0 * 64, dact.data_ptr() + r0 * 64,
                    p(X[r0:]), p(xhat[r0:]), p(rstd[r0:]), 1e-6, n, M, sp)
    assert torch.equal(_rows(act, M).view(torch.int16), a_ref.view(torch.int16))
    assert torch.equal(_rows(dact, M).view(torch.int16), d_ref.view(torch.int16))
    assert torch.equal(X, X_ref) and torch.equal(xhat.view(torch.int16), h_ref.view(torch.int16)) and torch.equal(rstd, r_ref)


@pytest.mark.parametrize('M', [300, 197 * 16])
def test_fused_mlp_half_modes_keep_only_what_is_asked_for(M):
    """Inference keeps neither act nor gelu' (MODE 0), the gelu'-recompute memory mode keeps act alone (MODE 1), no LayerNorm
    requested = plain residual add: X is bit-identical in every mode (same arithmetic, only the stores differ)."""
    native = _native()
    prob = _mlp_problem(M, 7 + M)
    a2, d2, X2, h2, r2 = _fused(native, *prob, mode=2)
    a1, d1, X1, h1, r1 = _fused(native, *prob, mode=1)
    a0, d0, Xi, h0, r0 = _fused(native, *prob, mode=0)
    assert d1 is None and a0 is None and d0 is None
    assert torch.equal(a1.view(torch.int16), a2.view(torch.int16))
    assert torch.equal(X1, X2) and torch.equal(Xi, X2)
    assert torch.equal(h1.view(torch.int16), h2.view(torch.int16)) and torch.equal(h0.view(torch.int16), h2.view(torch.int16))
    assert torch.equal(r0, r2)
    _, _, Xn, hn, rn = _fused(native, *prob, mode=0, ln=False)
    assert hn is None and torch.equal(Xn, X2)


def test_fused_mlp_half_is_run_to_run_identical_at_full_size():
    """Hand-counted vmcnt / one barrier per chunk: a mis-count shows up as rare wrong tiles that come and go.  Twenty launches on
    the benchmark's shape must give bit-identical outputs, and agree with the two-launch path on act / gelu'."""
    native = _native()
    M = 256 * 197
    prob = _mlp_problem(M, 3)
    a0, d0, _, _, _ = _two_launch(native, *prob)
    ref = None
    for it in range(20):
        a, d, X, h, r = _fused(native, *prob)
        assert torch.equal(a.view(torch.int16), a0.view(torch.int16)) and torch.equal(d.view(torch.int16), d0.view(torch.int16)), it
        if ref is None:
            ref = (X.clone(), h.clone(), r.clone())
        else:
            assert torch.equal(X, ref[0]) and torch.equal(h.view(torch.int16), ref[1].view(torch.int16)) and torch.equal(r, ref[2]), it


@pytest.mark.parametrize('M', [1, 37, 256, 257, 1000, 197 * 12, 256 * 197])
def test_fused_mlp_backward_equals_the_two_launch_dgrad_chain_and_a_torch_reference(M):
    """rovit_mlp_fused_bwd = rovit_gemm_nt(EPI_MUL) + rovit_gemm_ln_bwd in one launch: dpre bit-identical (same MFMA chain, the
    bf16-staged dgrad times the bf16 mask in fp32), dX to the fp32 summation order of the second GEMM (one chain over the 768
    hidden units here, two half-sums in the K = 768 kernel), dXb = bf16(dX) exactly."""
    native = _native()
    g = torch.Generator(device='cpu').manual_seed(900 + M)
    r = lambda *s: torch.randn(*s, generator=g)
    dY = bf(r(M, 192)).to(dev())
    w2t = bf(r(768, 192) * 0.05).to(dev())             # fc2 weight transposed (768,192)
    w1t = bf(r(192, 768) * 0.05).to(dev())             # fc1 weight (affine folded) transposed (192,768)
    dact = bf(torch.rand(M, 768, generator=g) * 1.2 - 0.1).to(dev())
    xh = bf(r(M, 192)).to(dev())
    rstd = (torch.rand(M, generator=g) + 0.5).to(dev())
    dX0 = r(M, 192).to(dev())
    p, sp = native.ptr, native.stream_ptr()
    # two launches
    dpre0 = torch.empty(M, 768, device=dev(), dtype=torch.bfloat16)
    native.call('rovit_gemm_nt', p(dY), 192, p(w2t), 192, M, 768, 192, None, 3, p(dpre0), 768, None, None, 0, p(dact), 768, None, 0, sp)
    dXa = dX0.clone()
    dXba = torch.empty(M, 192, device=dev(), dtype=torch.bfloat16)
    native.call('rovit_gemm_ln_bwd', p(dpre0), 768, p(w1t), 768, M, 768, p(xh), p(rstd), p(dXa), None, p(dXba), sp)
    # one launch
    ws = torch.empty(native.load().rovit_mlp_stream_bytes(), dtype=torch.uint8, device=dev())
    native.call('rovit_mlp_prepare_stream', p(w2t), p(w1t), p(ws), sp)
    dpre1 = torch.full((M, 768), float('nan'), device=dev(), dtype=torch.bfloat16)
    dXb1 = torch.full((M, 192), float('nan'), device=dev(), dtype=torch.bfloat16)
    dX1 = dX0.clone()
    dact_c = _chunks(dact)                                             # the one-launch kernels read gelu' and write dpre chunk-major
    native.call('rovit_mlp_fused_bwd', p(dY), p(ws), p(dact_c), p(dpre1), p(xh), p(rstd), p(dX1), p(dXb1), M, sp)
    dpre1_c = dpre1
    dpre1 = _rows(dpre1, M)
    assert torch.equal(dpre0.view(torch.int16), dpre1.view(torch.int16))
    # the weight-gradient launch reads the chunk-major operands in place (rovit_wgrad_multi_ex): dW1 = dpre^T xhat2 from the
    # chunk-major dpre (dY operand) and dW2 = dY^T act with a chunk-major A operand must equal the row-major launch bit for bit
    if M >= 64:
        import ctypes as C
        lib = native.load()
        S = 2
        arr = lambda xs: (C.c_int * len(xs))(*xs)
        shapes = [(768, 192), (192, 768)]                              # (N, K): fc1 (dY = dpre, A = xhat2), fc2 (dY = dY, A = "act" := dact)
        outs = []
        for blocked in (0, 1):
            # NaN, not zeros: a slab element that a launch never writes must not compare equal
            wsl = [torch.full((lib.rovit_wgrad_workspace_bytes(n, k, S) // 4,), float('nan'), device=dev()) for n, k in shapes]
            dys = [dpre1_c if blocked else dpre1, dY]
            As = [xh, dact_c if blocked else dact]
            native.call('rovit_wgrad_multi_ex', native.ptr_array(dys), arr([768, 192]), native.ptr_array(As), arr([192, 768]), arr([768, 192]),
                        arr([192, 768]), native.ptr_array(wsl), arr([0, blocked]), arr([blocked, 0]), 2, M, S, sp)
            outs.append([w.clone() for w in wsl])
        for a, b in zip(*outs):
            assert torch.equal(a, b)
    assert torch.equal(dXb1.view(torch.int16), bf(dX1).view(torch.int16))
    gq = bf(dpre1.float() @ w1t.float().t()).float()                  # the second dgrad, rounded as the kernel stages it
    h = xh.float()
    ref = dX0 + rstd[:, None] * (gq - gq.mean(1, keepdim=True) - h * (gq * h).mean(1, keepdim=True))
    ulp = 2 ** -7 * float(gq.abs().max() * rstd.max())                # one bf16 ulp of the staged dgrad, through the LayerNorm backward
    assert float((dX1 - ref).abs().max()) < 2e-3 * float(ref.abs().max()) + ulp
    assert float((dX1 - dXa).abs().max()) < 2 * ulp and float((dX1 - dXa).abs().mean()) < 2e-4
    # plain fp32 reference of the first product
    ref_dpre = (dY.float() @ w2t.float().t()) * dact.float()
    assert float((dpre1.float() - ref_dpre).abs().max()) < 2e-2 * float(ref_dpre.abs().max())


@pytest.mark.parametrize('M', [1, 37, 256, 257, 1000, 197 * 12, 256 * 197])
def test_block_tail_backward_equals_the_dgrad_launches_and_a_torch_reference(M):
    """rovit_block_tail_bwd = rovit_mlp_fused_bwd with the norm2 backward in registers (fp32 dxhat2 instead of a bf16-staged one) and the
    proj dgrad dO = dXb Wproj behind it in the same launch: dpre bit-identical, dX / dXb to the bf16 staging the other path has,
    dO against rovit_gemm_nt on this launch's own dXb (bit-identical: same MFMA chain) and all of it against fp32 torch."""
    native = _native()
    if not hasattr(native.load(), 'rovit_block_tail_bwd'):
        pytest.skip("round 3's backward block tail lives in the developer library only since round 4 (it lost in the step: 4.87 against 4.78 ms)")
    g = torch.Generator(device='cpu').manual_seed(1900 + M)
    r = lambda *s: torch.randn(*s, generator=g)
    dY = bf(r(M, 192)).to(dev())
    w2t = bf(r(768, 192) * 0.05).to(dev())
    w1t = bf(r(192, 768) * 0.05).to(dev())
    wpT = bf(r(192, 192) * 0.07).to(dev())             # WprojT: row d = weights of attention-output column d
    dact = bf(torch.rand(M, 768, generator=g) * 1.2 - 0.1).to(dev())
    xh = bf(r(M, 192)).to(dev())
    rstd = (torch.rand(M, generator=g) + 0.5).to(dev())
    dX0 = r(M, 192).to(dev())
    p, sp = native.ptr, native.stream_ptr()
    lib = native.load()
    dact_c = _chunks(dact)
    # the existing one-launch dgrad kernel + the proj dgrad GEMM
    ws0 = torch.empty(lib.rovit_mlp_stream_bytes(), dtype=torch.uint8, device=dev())
    native.call('rovit_mlp_prepare_stream', p(w2t), p(w1t), p(ws0), sp)
    dpre0 = torch.empty(M, 768, device=dev(), dtype=torch.bfloat16)
    dXa, dXba = dX0.clone(), torch.empty(M, 192, device=dev(), dtype=torch.bfloat16)
    native.call('rovit_mlp_fused_bwd', p(dY), p(ws0), p(dact_c), p(dpre0), p(xh), p(rstd), p(dXa), p(dXba), M, sp)
    # one launch
    ws = torch.empty(lib.rovit_mlp_stream_bytes(), dtype=torch.uint8, device=dev())
    native.call('rovit_mlp_prepare_stream_tail_bwd', p(w2t), p(w1t), p(wpT), p(ws), sp)
    nanb = lambda *s: torch.full(s, float('nan'), device=dev(), dtype=torch.bfloat16)
    dpre1, dXb1, dO1, dX1 = nanb(M, 768), nanb(M, 192), nanb(M, 192), dX0.clone()
    native.call('rovit_block_tail_bwd', p(dY), p(ws), p(dact_c), p(dpre1), p(xh), p(rstd), p(dX1), p(dXb1), p(dO1), M, sp)
    assert torch.equal(dpre0.view(torch.int16), dpre1.view(torch.int16))
    assert torch.equal(dXb1.view(torch.int16), bf(dX1).view(torch.int16))
    dpre_r = _rows(dpre1, M)
    gq = dpre_r.float() @ w1t.float().t()                               # the second dgrad in fp32 (this launch does not stage it through bf16)
    h = xh.float()
    ref = dX0 + rstd[:, None] * (gq - gq.mean(1, keepdim=True) - h * (gq * h).mean(1, keepdim=True))
    ulp = 2 ** -7 * float(gq.abs().max() * rstd.max())
    e_new, e_old = float((dX1 - ref).abs().max()), float((dXa - ref).abs().max())
    print('backward block tail: max |dX - fp32 reference|', e_new, 'staged path', e_old, 'bf16 ulp of the dgrad', ulp)
    assert e_new < 1e-3 * float(ref.abs().max()) + 0.1 * ulp and e_new <= e_old + 1e-6
    assert float((dX1 - dXa).abs().max()) < 2 * ulp
    # proj dgrad: against the library GEMM on the same dXb (same MFMA chain: bit-identical) and against fp32
    dO_chk = torch.empty(M, 192, device=dev(), dtype=torch.bfloat16)
    native.call('rovit_gemm_nt', p(dXb1), 192, p(wpT), 192, M, 192, 192, None, 0, p(dO_chk), 192, None, None, 0, None, 0, None, 0, sp)
    assert torch.equal(dO1.view(torch.int16), dO_chk.view(torch.int16))
    ref_dO = dXb1.float() @ wpT.float().t()
    assert float((dO1.float() - ref_dO).abs().max()) < 2 ** -7 * float(ref_dO.abs().max()) + 1e-6
    # dO = NULL: no proj phase, same dX
    dX2, dXb2, dpre2 = dX0.clone(), nanb(M, 192), nanb(M, 768)
    native.call('rovit_block_tail_bwd', p(dY), p(ws), p(dact_c), p(dpre2), p(xh), p(rstd), p(dX2), p(dXb2), None, M, sp)
    assert torch.equal(dX2, dX1) and torch.equal(dXb2.view(torch.int16), dXb1.view(torch.int16))


def test_fused_mlp_backward_is_run_to_run_identical_at_full_size():
    native = _native()
    M = 256 * 197
    g = torch.Generator(device='cpu').manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=g)
    dY, w2t, w1t = bf(r(M, 192)).to(dev()), bf(r(768, 192) * 0.05).to(dev()), bf(r(192, 768) * 0.05).to(dev())
    dact, xh = bf(torch.rand(M, 768, generator=g)).to(dev()), bf(r(M, 192)).to(dev())      # (read as chunk-major: any values do)
    rstd, dX0 = (torch.rand(M, generator=g) + 0.5).to(dev()), r(M, 192).to(dev())
    p, sp = native.ptr, native.stream_ptr()
    ws = torch.empty(native.load().rovit_mlp_stream_bytes(), dtype=torch.uint8, device=dev())
    native.call('rovit_mlp_prepare_stream', p(w2t), p(w1t), p(ws), sp)
    ref = None
    for it in range(20):
        dpre = torch.empty(M, 768, device=dev(), dtype=torch.bfloat16)
        dXb = torch.empty(M, 192, device=dev(), dtype=torch.bfloat16)
        dX = dX0.clone()
        native.call('rovit_mlp_fused_bwd', p(dY), p(ws), p(dact), p(dpre), p(xh), p(rstd), p(dX), p(dXb), M, sp)
        if ref is None:
            ref = (dpre.clone(), dX.clone(), dXb.clone())
        else:
            assert torch.equal(dpre.view(torch.int16), ref[0].view(torch.int16)) and torch.equal(dX, ref[1]), it
            assert torch.equal(dXb.view(torch.int16), ref[2].view(torch.int16)), it



@pytest.mark.parametrize('layers,G,B', [([192, 64, 16, 1], 5, 256), ([192, 64, 16, 1], 32, 512), ([16, 8, 1], 5, 33), ([192, 64, 16, 1], 5, 1),
                                        ([24, 8, 1], 32, 1500), ([192, 64, 16, 1], 5, 5000), ([10, 1], 5, 7)])
def test_kan_stack_backward_in_two_launches_is_bit_identical_to_the_per_layer_kernels(layers, G, B):
    """rovit_kan_stack_bwd (the per-sample dx chain of all layers in one launch + the parameter gradients of all layers in one
    launch) against rovit_kan_layer_bwd layer by layer: same arithmetic, same summation order, so every gradient is equal bit
    for bit; and through the module (autograd) against the CPU oracle."""
    import ctypes as C
    from models.kan import KANSeverityModule
    from rovit_hip.functions import ACT_RELU, ACT_SIGMOID3
    native = _native()
    p, sp = native.ptr, native.stream_ptr()
    g = torch.Generator().manual_seed(B + G)
    sd = ref_cpu.init_kan_state(layers, G, 3, g)
    m = KANSeverityModule(layers, G, 3)
    m.load_state_dict(sd)
    m = m.to(dev())
    n = len(layers) - 1
    x = (torch.randn(B, layers[0], generator=g) * 1.5).to(dev())
    acts = [ACT_RELU] * (n - 1) + [ACT_SIGMOID3]
    outs = []
    h = x
    for i, l in enumerate(m.kan_layers):
        h = l._run(h, acts[i]).detach()
        outs.append(h)
    gout = torch.randn(B, layers[-1], generator=g).to(dev())
    # per layer
    ref_dw, gcur, ref_dx = [], gout, None
    for i in range(n - 1, -1, -1):
        l = m.kan_layers[i]
        xin = x if i == 0 else outs[i - 1]
        dx = torch.empty_like(xin)
        dws, dlw, dlb = torch.empty_like(l.spline_weights), torch.empty_like(l.linear.weight), torch.empty_like(l.linear.bias)
        native.call('rovit_kan_layer_bwd', p(xin), p(l.spline_weights), p(l.knots), p(l.linear.weight), p(outs[i]), p(gcur), p(dx), p(dws), p(dlw),
                    p(dlb), B, l.in_features, l.out_features, l.knots.numel(), acts[i], 0, sp)
        ref_dw.insert(0, (dws, dlw, dlb))
        gcur = dx
    ref_dx = gcur
    # whole stack
    arr = lambda xs: (C.c_int * len(xs))(*xs)
    gz = [torch.empty(B, layers[i + 1], device=dev()) for i in range(n)]
    dx = torch.full_like(x, float('nan'))
    dws = [torch.full_like(l.spline_weights, float('nan')) for l in m.kan_layers]
    dlw = [torch.full_like(l.linear.weight, float('nan')) for l in m.kan_layers]
    dlb = [torch.full_like(l.linear.bias, float('nan')) for l in m.kan_layers]
    pa = native.ptr_array
    native.call('rovit_kan_stack_bwd', p(x), pa([l.spline_weights for l in m.kan_layers]), pa([l.knots for l in m.kan_layers]),
                pa([l.linear.weight for l in m.kan_layers]), pa(outs), pa([None] * (n - 1) + [gout]), pa(gz), p(dx), pa(dws), pa(dlw), pa(dlb),
                B, arr(layers), arr([l.knots.numel() for l in m.kan_layers]), arr(acts), n, sp)
    assert torch.equal(dx, ref_dx)
    for i in range(n):
        assert torch.equal(dws[i], ref_dw[i][0]) and torch.equal(dlw[i], ref_dw[i][1]) and torch.equal(dlb[i], ref_dw[i][2]), i
    # through the module: ONE autograd node for the stack, gradients vs the CPU oracle
    xd = x.clone().requires_grad_(True)
    y = m(xd)
    assert y.grad_fn is not None and 'KANStackFn' in type(y.grad_fn).__name__
    (y * gout).sum().backward()
    rp = {k: (v.clone().requires_grad_(True) if 'knots' not in k else v) for k, v in sd.items()}
    xr = x.cpu().clone().requires_grad_(True)
    (ref_cpu.kan_module_forward(xr, rp) * gout.cpu()).sum().backward()
    for k, prm in m.named_parameters():
        assert float((prm.grad.cpu() - rp[k].grad).abs().max()) < 5e-4 * float(rp[k].grad.abs().max() + 1e-6), k
    assert float((xd.grad.cpu() - xr.grad).abs().max()) < 5e-4 * float(xr.grad.abs().max() + 1e-9)


def test_backbone_forward_with_the_fused_mlp_half_matches_the_two_launch_build_of_the_same_forward():
    """mlp_path (an argument of rovit_vit_forward / _backward since round 4; rounds 2-3: a process-wide environment switch and two child
    processes) selects the MLP-half kernels: run both on the same seeded weights and images, training workspaces, and compare features
    and every gradient."""
    from oracle import ref_cpu
    from models.backbone import DeiTTiny
    from rovit_hip import native
    m = DeiTTiny(12)
    m.load_state_dict(ref_cpu.init_vit_state(12, torch.Generator().manual_seed(5)))
    m = m.cuda().train()
    torch.manual_seed(1)
    x = torch.randn(24, 3, 224, 224, device='cuda')
    res = {}
    for mode, path in (('1', native.MLP_ONE_LAUNCH), ('0', native.MLP_TWO_LAUNCH)):
        m.engine.mlp_path = path
        for prm in m.parameters():
            prm.grad = None
        f = m(x)
        (f.float().square().mean()).backward()
        res[mode] = {'f': f.detach().cpu(), 'g': torch.cat([prm.grad.flatten() for prm in m.parameters()]).cpu()}
    m.engine.mlp_path = None
    f1, f0 = res['1']['f'], res['0']['f']
    g1, g0 = res['1']['g'], res['0']['g']
    # the two builds differ only by fp32 summation order inside fc2 (an occasional neighbouring-bf16 rounding of a branch output)
    # (bf16 rounding flips propagate through 12 blocks: the two builds differ like either differs from the fp32 oracle)
    # (the one-launch build also keeps the residual stream in fp32 where the other stages two branch outputs through bf16: 6.1e-3 RMS
    # between the builds after 12 blocks, each within the 8e-3 the tests allow against the fp32 oracle)
    assert float((f1 - f0).abs().max()) < 3e-2 and float((f1 - f0).pow(2).mean().sqrt()) < 8e-3
    assert float(torch.nn.functional.cosine_similarity(g1, g0, dim=0)) > 0.9995
    assert float((g1 - g0).abs().max()) < 3e-2 * float(g0.abs().max())
