"""GPU tests of rovit_block_bwd_fused (mlp_fused.hip): the qkv dgrad + norm1 backward of block i in front of the MLP dgrad chain of block
i-1 in one launch, against the two launches it replaces (rovit_gemm_ln_bwd at K = 576, rovit_mlp_fused_bwd), against an fp32 torch
reference of the staged arithmetic, in its partial modes, and inside rovit_vit_backward (whole and cut into block ranges).

Row counts: 1 and 37 are one partial row tile; 240 is exactly one workgroup (240 token rows per workgroup while the launch fits one round
of workgroups), 241 adds a workgroup that holds one row; 394 = 2 x 197 and 591 = 3 x 197 are no multiple of 16."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 37, 240, 241, 394, 591]
PAD = 16                      # rows behind M of every output: pre-filled with NaN, must stay NaN


def _native():
    from rovit_hip import native
    native.load()
    return native


def dev():
    return torch.device('cuda:0')


def bf(x):
    return x.to(torch.bfloat16)


def _rows(t, M):
    """chunk-major [24][M][32] -> row-major (M,768)"""
    return t.view(24, M, 32).permute(1, 0, 2).reshape(M, 768).contiguous()


def _chunks(t):
    """row-major (M,768) -> chunk-major [24][M][32], flat"""
    M = t.shape[0]
    return t.view(M, 24, 32).permute(1, 0, 2).contiguous().view(M, 768)


def _bits(t):
    return t.view(torch.int16)


def _nan(*shape):
    return torch.full(shape, float('nan'), device=dev(), dtype=torch.bfloat16)


def _all_nan(t):
    return bool(t.float().isnan().all())


@functools.lru_cache(maxsize=None)
def _case(M):
    """Seeded CPU inputs of one row count, the fused launch on them, and the launches it replaces; shared by the tests, never modified."""
    native = _native()
    g = torch.Generator(device='cpu').manual_seed(5100 + M)
    r = lambda *s: torch.randn(*s, generator=g)
    c = {'M': M}
    c['dqkv'] = bf(r(M, 576)).to(dev())
    c['wqT'] = bf(r(192, 576) * 0.05).to(dev())            # qkv weight (norm1 affine folded) transposed (192,576)
    c['xh1'] = bf(r(M, 192)).to(dev())
    c['rstd1'] = (torch.rand(M, generator=g) + 0.5).to(dev())
    c['xmid_in'] = bf(r(M, 192)).to(dev())
    c['w2t'] = bf(r(768, 192) * 0.05).to(dev())
    c['w1t'] = bf(r(192, 768) * 0.05).to(dev())
    c['dact'] = bf(torch.rand(M, 768, generator=g) * 1.2 - 0.1).to(dev())
    c['dact_c'] = _chunks(c['dact'])
    c['xh2'] = bf(r(M, 192)).to(dev())
    c['rstd2'] = (torch.rand(M, generator=g) + 0.5).to(dev())
    p, sp = native.ptr, native.stream_ptr()
    ws = torch.empty(native.load().rovit_mlp_stream_bytes(), dtype=torch.uint8, device=dev())
    native.call('rovit_mlp_prepare_stream_bwd', p(c['w2t']), p(c['w1t']), p(c['wqT']), p(ws), sp)
    c['ws'] = ws
    c['fused'] = _launch(c)
    # the two launches it replaces, on the same inputs
    xout0 = _nan(M, 192)
    native.call('rovit_gemm_ln_bwd', p(c['dqkv']), 576, p(c['wqT']), 576, M, 576, p(c['xh1']), p(c['rstd1']), None, p(c['xmid_in']), p(xout0), sp)
    c['xout_gemm'] = xout0
    torch.cuda.synchronize()
    return c


def _launch(c, front=True, mlp=True, xout_in=None):
    """rovit_block_bwd_fused with NaN-filled outputs of M + PAD rows -> (xout, dpre flat chunk-major + PAD rows of tail, xmid)."""
    native = _native()
    M = c['M']
    p, sp = native.ptr, native.stream_ptr()
    xout = _nan(M + PAD, 192)
    if xout_in is not None:
        xout[:M] = xout_in
    dpre = _nan(24 * M * 32 + PAD * 768)
    xmid = _nan(M + PAD, 192)
    native.call('rovit_block_bwd_fused', p(c['dqkv']) if front else None, p(c['xh1']), p(c['rstd1']), p(c['xmid_in']), p(xout), p(c['ws']),
                p(c['dact_c']) if mlp else None, p(dpre) if mlp else None, p(c['xh2']) if mlp else None, p(c['rstd2']) if mlp else None,
                p(xmid) if mlp else None, M, sp)
    torch.cuda.synchronize()
    return xout, dpre, xmid


def _mlp_alone(c, dY):
    native = _native()
    M = c['M']
    p, sp = native.ptr, native.stream_ptr()
    dpre, xmid = _nan(24 * M * 32), _nan(M, 192)
    native.call('rovit_mlp_fused_bwd', p(dY), p(c['ws']), p(c['dact_c']), p(dpre), p(c['xh2']), p(c['rstd2']), None, p(xmid), M, sp)
    torch.cuda.synchronize()
    return dpre, xmid


@pytest.mark.parametrize('M', SIZES)
def test_front_phase_equals_the_qkv_dgrad_launch_and_a_torch_reference(M):
    """xout of the fused launch against rovit_gemm_ln_bwd(dqkv, K = 576, ..., xmid, xout) and against fp32 torch on the staged dgrad; the
    bound is the one the same epilogue has in test_gpu_round3 (2 bf16 ulps of the staged dgrad through the LayerNorm backward, mean 2e-4;
    2e-3 relative plus one ulp against torch)."""
    c = _case(M)
    xout = c['fused'][0][:M].float()
    x0 = c['xout_gemm'].float()
    gq = bf(c['dqkv'].float() @ c['wqT'].float().t()).float()            # the dgrad, rounded as the kernel stages it
    h = c['xh1'].float()
    ref = c['xmid_in'].float() + c['rstd1'][:, None] * (gq - gq.mean(1, keepdim=True) - h * (gq * h).mean(1, keepdim=True))
    ulp = 2 ** -7 * float(gq.abs().max() * c['rstd1'].max())
    d_gemm, d_ref = (xout - x0).abs(), (xout - ref).abs()
    print('M', M, 'max |fused - gemm_ln_bwd|', float(d_gemm.max()), 'mean', float(d_gemm.mean()), 'bit-identical',
          torch.equal(_bits(c['fused'][0][:M]), _bits(c['xout_gemm'])), 'max |fused - torch|', float(d_ref.max()), 'ulp', ulp,
          'max |ref|', float(ref.abs().max()))
    assert not bool(xout.isnan().any())
    assert float(d_gemm.max()) < 2 * ulp and float(d_gemm.mean()) < 2e-4
    assert float(d_ref.max()) < 2e-3 * float(ref.abs().max()) + ulp


@pytest.mark.parametrize('M', SIZES)
def test_mlp_phase_is_the_arithmetic_of_the_mlp_launch_on_the_fused_xout(M):
    """rovit_mlp_fused_bwd fed with the fused launch's own xout gives its dpre (chunk-major) and xmid bit for bit."""
    c = _case(M)
    xout, dpre, xmid = c['fused']
    dpre0, xmid0 = _mlp_alone(c, xout[:M].contiguous())
    assert not _all_nan(dpre0) and not bool(xmid0.float().isnan().any())
    assert torch.equal(_bits(dpre[:24 * M * 32]), _bits(dpre0))
    assert torch.equal(_bits(xmid[:M]), _bits(xmid0))
    # and a plain fp32 reference of the first product, from the rows the front phase wrote
    ref_dpre = (xout[:M].float() @ c['w2t'].float().t()) * c['dact'].float()
    got = _rows(dpre[:24 * M * 32].view(M, 768), M).float()
    assert float((got - ref_dpre).abs().max()) < 2e-2 * float(ref_dpre.abs().max())


@pytest.mark.parametrize('M', SIZES)
def test_partial_modes(M):
    """Front pointer NULL: the launch is rovit_mlp_fused_bwd bit for bit.  MLP pointers NULL: xout equals the full launch's bit for bit."""
    c = _case(M)
    xout, dpre, xmid = c['fused']
    dY = xout[:M].contiguous()
    x1, dpre1, xmid1 = _launch(c, front=False, xout_in=dY)
    dpre0, xmid0 = _mlp_alone(c, dY)
    assert torch.equal(_bits(dpre1[:24 * M * 32]), _bits(dpre0)) and torch.equal(_bits(xmid1[:M]), _bits(xmid0))
    assert torch.equal(_bits(x1[:M]), _bits(dY)) and _all_nan(x1[M:])          # xout is an input in this mode
    assert _all_nan(dpre1[24 * M * 32:]) and _all_nan(xmid1[M:])
    x2, dpre2, xmid2 = _launch(c, mlp=False)
    assert torch.equal(_bits(x2[:M]), _bits(xout[:M]))
    assert _all_nan(x2[M:]) and _all_nan(dpre2) and _all_nan(xmid2)


@pytest.mark.parametrize('M', SIZES)
def test_rows_beyond_M_keep_their_fill(M):
    c = _case(M)
    xout, dpre, xmid = c['fused']
    assert _all_nan(xout[M:]) and _all_nan(xmid[M:]) and _all_nan(dpre[24 * M * 32:])
    assert not bool(xout[:M].float().isnan().any()) and not bool(xmid[:M].float().isnan().any())
    assert not bool(dpre[:24 * M * 32].float().isnan().any())


def test_two_launches_on_the_same_inputs_give_equal_bits():
    c = _case(591)
    a, b = c['fused'], _launch(c)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


def test_argument_checks():
    native = _native()
    c = _case(37)
    p, sp = native.ptr, native.stream_ptr()
    lib = native.load()
    o = _nan(37, 192)
    # the front part without its operands, a misaligned buffer, the MLP part without dpre
    assert lib.rovit_block_bwd_fused(p(c['dqkv']), None, p(c['rstd1']), p(c['xmid_in']), p(o), p(c['ws']), None, None, None, None, None, 37, sp) != 0
    assert lib.rovit_block_bwd_fused(p(c['dqkv']) + 2, p(c['xh1']), p(c['rstd1']), p(c['xmid_in']), p(o), p(c['ws']), None, None, None, None, None,
                                     37, sp) != 0
    assert lib.rovit_block_bwd_fused(p(c['dqkv']), p(c['xh1']), p(c['rstd1']), p(c['xmid_in']), p(o), p(c['ws']), p(c['dact_c']), None, p(c['xh2']),
                                     p(c['rstd2']), p(o), 37, sp) != 0
    assert lib.rovit_block_bwd_fused(p(c['dqkv']), p(c['xh1']), p(c['rstd1']), p(c['xmid_in']), p(o), p(c['ws']), None, None, None, None, None, 0, sp) != 0
    torch.cuda.synchronize()
    assert _all_nan(o)


def test_whole_backward_with_the_fused_launch_small():
    """Depth 3, batch 2, one-launch MLP path: every parameter gradient against the two-launch path of the same inputs (the bound of the
    existing one-launch / two-launch comparison in test_gpu_round3, applied to every tensor), and the call cut into the block ranges
    [2,2] [1,1] [0,0] -- the fused launch then runs as its front-only and MLP-only halves -- bit-identical to the uncut call, parameter
    gradients and the image gradient of rovit_vit_backward_input alike."""
    from oracle import ref_cpu
    from models.backbone import DeiTTiny
    from rovit_hip import native
    depth = 3
    m = DeiTTiny(depth)
    m.load_state_dict(ref_cpu.init_vit_state(depth, torch.Generator().manual_seed(5)))
    m = m.cuda().train()
    torch.manual_seed(1)
    x = torch.randn(2, 3, 224, 224, device='cuda')

    def run(path, ranges, want_dx):
        m.engine.mlp_path, m.engine.backward_ranges = path, ranges
        for prm in m.parameters():
            prm.grad = None
        xi = x.clone().requires_grad_(want_dx)
        f = m(xi)
        (f.float().square().mean()).backward()
        torch.cuda.synchronize()
        return [prm.grad.detach().clone() for prm in m.parameters()], (xi.grad.detach().clone() if want_dx else None)

    try:
        cut = [(2, 2), (1, 1), (0, 0)]
        g_one, _ = run(native.MLP_ONE_LAUNCH, None, False)
        g_two, _ = run(native.MLP_TWO_LAUNCH, None, False)
        g_cut, _ = run(native.MLP_ONE_LAUNCH, cut, False)
        gi_one, dx_one = run(native.MLP_ONE_LAUNCH, None, True)
        gi_cut, dx_cut = run(native.MLP_ONE_LAUNCH, cut, True)
    finally:
        m.engine.mlp_path, m.engine.backward_ranges = None, None
    names = [n for n, _ in m.named_parameters()]
    f1, f0 = torch.cat([t.flatten() for t in g_one]), torch.cat([t.flatten() for t in g_two])
    top = float(f0.abs().max())
    cos = float(torch.nn.functional.cosine_similarity(f1, f0, dim=0))
    print('one-launch against two-launch: cosine', cos, 'max |g0|', top)
    for n, a, b in zip(names, g_one, g_two):
        d = float((a - b).abs().max())
        print('  %-40s max diff %.3e  (tensor max %.3e)' % (n, d, float(b.abs().max())))
        assert bool(torch.isfinite(a).all()), n
        assert d < 3e-2 * top, n
    assert cos > 0.9995
    for n, a, b in zip(names, g_one, g_cut):
        assert torch.equal(a, b), n
    for n, a, b in zip(names, gi_one, gi_cut):
        assert torch.equal(a, b), n
    assert dx_one is not None and bool(torch.isfinite(dx_one).all()) and float(dx_one.abs().max()) > 0
    assert torch.equal(dx_one, dx_cut)
