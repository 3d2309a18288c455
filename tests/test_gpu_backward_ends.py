"""GPU tests of the two ends of the backward's dgrad chain.

Top: rovit_block_bwd_fused_cls (mlp_fused.hip) -- the class-token block's qkv dgrad + norm1 backward in front of the MLP dgrad of the
block below, against the launch it replaces (rovit_gemm_ln_bwd_cls) and rovit_mlp_fused_bwd, bit for bit, and with NaN in every row of
the incoming mid-block gradient that carries none (the select).  Bottom: the qkv weight gradient of a range's last block is handed to the
side stream behind the attention backward.  Both inside rovit_vit_backward: the uncut backward against backwards cut into block ranges
(which run the launches unfused and flush at every range end), bit for bit.

Row counts: 1 and 37 are one partial row tile; 197 is exactly one image; 240 is exactly one workgroup, 241 adds a workgroup that holds one
row; 394 = 2 x 197 and 591 = 3 x 197 put an incoming row into the interior of a tile (rows 197, 394)."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 37, 197, 240, 241, 394, 591]
PAD = 16                      # rows behind M of every output: pre-filled with NaN, must stay NaN
STEP = 197


def _native():
    from rovit_hip import native
    native.load()
    return native


def dev():
    return torch.device('cuda:0')


def bf(x):
    return x.to(torch.bfloat16)


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


def _finite(t):
    return bool(torch.isfinite(t.float()).all())


def _launch(c, step, front=True, mlp=True, xout_in=None, xmid_in=None, plain=False):
    """rovit_block_bwd_fused_cls (plain: rovit_block_bwd_fused) with NaN-filled outputs of M + PAD rows -> (xout, dpre flat chunk-major +
    PAD rows of tail, xmid)."""
    native = _native()
    M = c['M']
    p, sp = native.ptr, native.stream_ptr()
    xout = _nan(M + PAD, 192)
    if xout_in is not None:
        xout[:M] = xout_in
    dpre = _nan(24 * M * 32 + PAD * 768)
    xmid = _nan(M + PAD, 192)
    xm = c['xmid_in'] if xmid_in is None else xmid_in
    head = [p(c['dqkv']) if front else None, p(c['xh1']), p(c['rstd1']), p(xm)]
    tail = [p(xout), p(c['ws']), p(c['dact_c']) if mlp else None, p(dpre) if mlp else None, p(c['xh2']) if mlp else None,
            p(c['rstd2']) if mlp else None, p(xmid) if mlp else None, M, sp]
    if plain:
        native.call('rovit_block_bwd_fused', *head, *tail)
    else:
        native.call('rovit_block_bwd_fused_cls', *head, step, *tail)
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


@functools.lru_cache(maxsize=None)
def _case(M):
    """Seeded CPU inputs of one row count, the class-token launch on them, and the launches it replaces; shared by the tests, never
    modified."""
    native = _native()
    g = torch.Generator(device='cpu').manual_seed(6100 + M)
    r = lambda *s: torch.randn(*s, generator=g)
    c = {'M': M}
    c['dqkv'] = bf(r(M, 576)).to(dev())
    c['wqT'] = bf(r(192, 576) * 0.05).to(dev())
    c['xh1'] = bf(r(M, 192)).to(dev())
    c['rstd1'] = (torch.rand(M, generator=g) + 0.5).to(dev())
    c['xmid_in'] = bf(r(M, 192)).to(dev())
    c['w2t'] = bf(r(768, 192) * 0.05).to(dev())
    c['w1t'] = bf(r(192, 768) * 0.05).to(dev())
    c['dact_c'] = _chunks(bf(torch.rand(M, 768, generator=g) * 1.2 - 0.1).to(dev()))
    c['xh2'] = bf(r(M, 192)).to(dev())
    c['rstd2'] = (torch.rand(M, generator=g) + 0.5).to(dev())
    # the same incoming gradient with NaN in every row that carries none
    xm = c['xmid_in'].clone()
    rows = torch.arange(M, device=dev())
    xm[rows % STEP != 0] = float('nan')
    c['xmid_nan'] = xm
    p, sp = native.ptr, native.stream_ptr()
    ws = torch.empty(native.load().rovit_mlp_stream_bytes(), dtype=torch.uint8, device=dev())
    native.call('rovit_mlp_prepare_stream_bwd', p(c['w2t']), p(c['w1t']), p(c['wqT']), p(ws), sp)
    c['ws'] = ws
    c['fused'] = _launch(c, STEP)
    xout0 = _nan(M + PAD, 192)
    native.call('rovit_gemm_ln_bwd_cls', p(c['dqkv']), 576, p(c['wqT']), 576, M, 576, p(c['xh1']), p(c['rstd1']), p(c['xmid_in']), STEP,
                p(xout0), sp)
    torch.cuda.synchronize()
    c['xout_gemm'] = xout0
    return c


@pytest.mark.parametrize('M', SIZES)
def test_cls_form_equals_the_launches_it_replaces(M):
    """xout against rovit_gemm_ln_bwd_cls, dpre / dXb against rovit_mlp_fused_bwd on that xout, bit for bit; pad rows keep their NaN."""
    c = _case(M)
    xout, dpre, xmid = c['fused']
    assert _all_nan(c['xout_gemm'][M:]) and _finite(c['xout_gemm'][:M])
    d = (xout[:M].float() - c['xout_gemm'][:M].float()).abs()
    print('M', M, 'max |fused cls - gemm_ln_bwd_cls|', float(d.max()))
    assert torch.equal(_bits(xout[:M]), _bits(c['xout_gemm'][:M]))
    dpre0, xmid0 = _mlp_alone(c, c['xout_gemm'][:M].contiguous())
    assert _finite(dpre0) and _finite(xmid0)
    assert torch.equal(_bits(dpre[:24 * M * 32]), _bits(dpre0))
    assert torch.equal(_bits(xmid[:M]), _bits(xmid0))
    assert _all_nan(xout[M:]) and _all_nan(xmid[M:]) and _all_nan(dpre[24 * M * 32:])
    # the rows without an incoming gradient are the LayerNorm-backward term alone: not what the plain launch gives on the same buffer
    if M > 1:
        plain = _launch(c, 0, plain=True)
        assert not torch.equal(_bits(plain[0][:M]), _bits(xout[:M]))
        assert torch.equal(_bits(plain[0][0]), _bits(xout[0]))          # row 0 carries its gradient in both


@pytest.mark.parametrize('M', SIZES)
def test_rows_without_gradient_are_zeros_by_a_select(M):
    """NaN in every row of xmid_in that is no multiple of 197: every output unchanged bit for bit, and finite."""
    c = _case(M)
    a = c['fused']
    b = _launch(c, STEP, xmid_in=c['xmid_nan'])
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))
    assert _finite(b[0][:M]) and _finite(b[1][:24 * M * 32]) and _finite(b[2][:M])
    # ... and in the front-only mode
    x2, dpre2, xmid2 = _launch(c, STEP, mlp=False, xmid_in=c['xmid_nan'])
    assert torch.equal(_bits(x2), _bits(a[0])) and _all_nan(dpre2) and _all_nan(xmid2)


@pytest.mark.parametrize('M', SIZES)
def test_step_zero_is_the_plain_launch(M):
    c = _case(M)
    a, b = _launch(c, 0), _launch(c, 0, plain=True)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))
    assert _finite(a[0][:M]) and _all_nan(a[0][M:])


@pytest.mark.parametrize('M', SIZES)
def test_partial_modes_of_the_cls_form(M):
    """Front pointer NULL: the launch is rovit_mlp_fused_bwd bit for bit (xmid_step plays no part).  MLP pointers NULL: xout equals the
    full launch's bit for bit."""
    c = _case(M)
    xout, dpre, xmid = c['fused']
    dY = xout[:M].contiguous()
    x1, dpre1, xmid1 = _launch(c, STEP, front=False, xout_in=dY)
    dpre0, xmid0 = _mlp_alone(c, dY)
    assert torch.equal(_bits(dpre1[:24 * M * 32]), _bits(dpre0)) and torch.equal(_bits(xmid1[:M]), _bits(xmid0))
    assert torch.equal(_bits(x1[:M]), _bits(dY)) and _all_nan(x1[M:])          # xout is an input in this mode
    assert _all_nan(dpre1[24 * M * 32:]) and _all_nan(xmid1[M:])
    x2, dpre2, xmid2 = _launch(c, STEP, mlp=False)
    assert torch.equal(_bits(x2[:M]), _bits(xout[:M]))
    assert _all_nan(x2[M:]) and _all_nan(dpre2) and _all_nan(xmid2)


def test_two_cls_launches_on_the_same_inputs_give_equal_bits():
    c = _case(591)
    for x, y in zip(c['fused'], _launch(c, STEP)):
        assert torch.equal(_bits(x), _bits(y))


def test_argument_checks():
    native = _native()
    c = _case(37)
    p, sp = native.ptr, native.stream_ptr()
    lib = native.load()
    o, dpre, xmid = _nan(37, 192), _nan(37 * 768), _nan(37, 192)
    full = lambda step, M=37, dq=None: lib.rovit_block_bwd_fused_cls(p(c['dqkv']) if dq is None else dq, p(c['xh1']), p(c['rstd1']),
                                                                      p(c['xmid_in']), step, p(o), p(c['ws']), p(c['dact_c']), p(dpre),
                                                                      p(c['xh2']), p(c['rstd2']), p(xmid), M, sp)
    assert full(-1) != 0 and full(-197) != 0
    # a negative step is refused in the partial modes too
    assert lib.rovit_block_bwd_fused_cls(p(c['dqkv']), p(c['xh1']), p(c['rstd1']), p(c['xmid_in']), -1, p(o), p(c['ws']), None, None, None, None,
                                         None, 37, sp) != 0
    assert lib.rovit_block_bwd_fused_cls(None, None, None, None, -1, p(o), p(c['ws']), p(c['dact_c']), p(dpre), p(c['xh2']), p(c['rstd2']),
                                         p(xmid), 37, sp) != 0
    assert full(STEP, M=0) != 0 and full(STEP, dq=p(c['dqkv']) + 2) != 0
    assert lib.rovit_block_bwd_fused_cls(p(c['dqkv']), p(c['xh1']), p(c['rstd1']), None, STEP, p(o), p(c['ws']), None, None, None, None, None, 37,
                                         sp) != 0
    torch.cuda.synchronize()
    assert _all_nan(o) and _all_nan(dpre) and _all_nan(xmid)


# ---- inside rovit_vit_backward -------------------------------------------------------------------------------------------------

def _model(depth, seed=5):
    from oracle import ref_cpu
    from models.backbone import DeiTTiny
    m = DeiTTiny(depth)
    m.load_state_dict(ref_cpu.init_vit_state(depth, torch.Generator().manual_seed(seed)))
    return m.cuda().train()


def _run(m, x, path, ranges, want_dx=False):
    """One forward + backward of the backbone on the given MLP path and block ranges -> (parameter gradients, image gradient)."""
    m.engine.mlp_path, m.engine.backward_ranges = path, ranges
    try:
        for prm in m.parameters():
            prm.grad = None
        xi = x.clone().requires_grad_(want_dx)
        f = m(xi)
        (f.float().square().mean()).backward()
        torch.cuda.synchronize()
        return [prm.grad.detach().clone() for prm in m.parameters()], (xi.grad.detach().clone() if want_dx else None)
    finally:
        m.engine.mlp_path, m.engine.backward_ranges = None, None


def _cuts(depth):
    cuts = [[(i, i) for i in range(depth - 1, -1, -1)]]
    if depth >= 3:
        cuts.append([(depth - 1, depth - 2), (depth - 3, 0)])
    return cuts


def _assert_equal_grads(m, a, b, what):
    for (n, _), u, v in zip(m.named_parameters(), a, b):
        assert bool(torch.isfinite(u).all()), (what, n)
        assert torch.equal(u, v), (what, n)


@pytest.mark.parametrize('depth,batch', [(3, 2), (3, 17), (2, 3)])
def test_uncut_backward_equals_the_backward_cut_into_ranges(depth, batch):
    """The uncut one-launch backward fuses the class-token block's A5 into block depth-2's launch and flushes block 0's qkv weight gradient
    behind the attention backward; cut into single blocks nothing is fused and every block flushes; cut as [(d-1, d-2), (d-3, 0)] the
    class-token launch is fused and the flush of block d-2 stands where a merged launch would carry it."""
    from rovit_hip import native
    m = _model(depth)
    torch.manual_seed(1)
    x = torch.randn(batch, 3, 224, 224, device='cuda')
    g_one, _ = _run(m, x, native.MLP_ONE_LAUNCH, None)
    assert max(float(g.abs().max()) for g in g_one) > 0
    for cut in _cuts(depth):
        g_cut, _ = _run(m, x, native.MLP_ONE_LAUNCH, cut)
        _assert_equal_grads(m, g_one, g_cut, cut)


def _assert_close_to_two_launch(m, g_one, g_two):
    """the existing bound of the one-launch / two-launch comparison (test_gpu_block_bwd): 3e-2 of the largest gradient, cosine > 0.9995"""
    f1, f0 = torch.cat([t.flatten() for t in g_one]), torch.cat([t.flatten() for t in g_two])
    top = float(f0.abs().max())
    cos = float(torch.nn.functional.cosine_similarity(f1, f0, dim=0))
    print('one-launch against two-launch: cosine', cos, 'max |g0|', top)
    for (n, _), a, b in zip(m.named_parameters(), g_one, g_two):
        d = float((a - b).abs().max())
        print('  %-40s max diff %.3e  (tensor max %.3e)' % (n, d, float(b.abs().max())))
        assert bool(torch.isfinite(a).all()), n
        assert d < 3e-2 * top, n
    assert cos > 0.9995


@pytest.mark.parametrize('depth', [1, 3])
def test_one_launch_against_two_launch(depth):
    """Depth 1: nothing is fused and the early flush belongs to the class-token block.  Depth 3: the fused class-token launch against the
    two-launch path, where it stays a launch of its own."""
    from rovit_hip import native
    m = _model(depth)
    torch.manual_seed(1)
    x = torch.randn(2, 3, 224, 224, device='cuda')
    g_one, _ = _run(m, x, native.MLP_ONE_LAUNCH, None)
    g_two, _ = _run(m, x, native.MLP_TWO_LAUNCH, None)
    _assert_close_to_two_launch(m, g_one, g_two)


def test_three_backwards_in_a_row_give_equal_bits():
    """The ordering of the moved hand-over: depth 3, batch 17, every parameter gradient of three runs."""
    from rovit_hip import native
    m = _model(3)
    torch.manual_seed(1)
    x = torch.randn(17, 3, 224, 224, device='cuda')
    runs = [_run(m, x, native.MLP_ONE_LAUNCH, None)[0] for _ in range(3)]
    _assert_equal_grads(m, runs[0], runs[1], 'run 2')
    _assert_equal_grads(m, runs[0], runs[2], 'run 3')


def test_image_gradient_with_parameter_gradients_cut_equals_uncut():
    from rovit_hip import native
    m = _model(3)
    torch.manual_seed(1)
    x = torch.randn(2, 3, 224, 224, device='cuda')
    g_one, dx_one = _run(m, x, native.MLP_ONE_LAUNCH, None, True)
    assert bool(torch.isfinite(dx_one).all()) and float(dx_one.abs().max()) > 0
    for cut in _cuts(3):
        g_cut, dx_cut = _run(m, x, native.MLP_ONE_LAUNCH, cut, True)
        _assert_equal_grads(m, g_one, g_cut, cut)
        assert torch.equal(dx_one, dx_cut), cut


class _Chain:
    """The training forward of a DeiTTiny(depth) on the one-launch path through the C entry points, and its dgrad chain alone
    (grads == NULL) over given block ranges."""

    def __init__(self, depth, batch):
        from rovit_hip import native
        self.native, self.depth, self.B = native, depth, batch
        self.m = _model(depth)
        self.eng = self.m.engine
        self.params = self.m.ordered_parameters()
        self.eng.prepare(self.params)
        self.pa = native.ptr_array(self.params)
        torch.manual_seed(1)
        self.x = torch.randn(batch, 3, 224, 224, device='cuda')
        self.seed = torch.randn(batch, 192, device='cuda')
        self.mlp = native.MLP_ONE_LAUNCH
        self.ws = self.eng.take_ws(batch, True, dev())

    def forward(self):
        n = self.native
        feats = torch.empty(self.B, 192, device=dev(), dtype=torch.float32)
        n.call('rovit_vit_forward', n.ptr(self.x), self.pa, n.ptr(self.eng.prep), n.ptr(self.ws), n.ptr(feats), self.B, self.depth, 1, self.mlp,
               n.stream_ptr())

    def dgrad(self, first, last, d_img=None):
        n = self.native
        n.call('rovit_vit_backward_input', n.ptr(self.x), n.ptr(self.seed), self.pa, n.ptr(self.eng.prep), n.ptr(self.ws), None, self.B,
               self.depth, first, last, self.mlp, n.stream_ptr(), n.ptr(d_img) if d_img is not None else None, 1, 1.0, 0)

    def field(self, field, block):
        off, nbytes = ctypes.c_size_t(), ctypes.c_size_t()
        self.native.call('rovit_vit_workspace_field', self.B, self.depth, field, block, ctypes.byref(off), ctypes.byref(nbytes))
        return self.ws.data_ptr() + off.value

    def close(self):
        torch.cuda.synchronize()
        self.eng.give_ws(self.B, True, self.ws)


def test_image_gradient_without_parameter_gradients_cut_equals_uncut():
    """grads == NULL: the dgrad chain alone, one stream; the class-token launch is fused all the same."""
    c = _Chain(3, 2)
    try:
        out = []
        for ranges in [[(2, 0)]] + _cuts(3):
            c.forward()
            d = torch.full((2, 3, 224, 224), float('nan'), device='cuda')
            for first, last in ranges:
                c.dgrad(first, last, d if last == 0 else None)
            torch.cuda.synchronize()
            out.append(d)
        assert bool(torch.isfinite(out[0]).all()) and float(out[0].abs().max()) > 0
        for d in out[1:]:
            assert torch.equal(out[0], d)
    finally:
        c.close()


def test_attention_relevance_equals_the_single_block_range_path():
    """rovit_vit_backward_relevance (grads == NULL, the whole depth, the class-token launch fused) against the same relevance steps issued
    behind single-block ranges of the dgrad chain, which run every launch unfused: equal bits."""
    from rovit_hip import taps
    c = _Chain(3, 2)
    n = c.native
    try:
        scratch = torch.empty(2 * 3 * 197, device='cuda')
        u1 = torch.full((2, 197), float('nan'), device='cuda')
        u2 = torch.full((2, 197), float('nan'), device='cuda')
        c.forward()
        n.call('rovit_vit_backward_relevance', n.ptr(c.seed), c.pa, n.ptr(c.eng.prep), n.ptr(c.ws), 2, 3, c.mlp, n.ptr(u1), n.ptr(scratch),
               n.stream_ptr())
        torch.cuda.synchronize()
        c.forward()
        for i in (2, 1, 0):
            c.dgrad(i, i)
            n.call('rovit_attention_relevance_step', c.field(taps.WS_QKV, i), c.field(taps.WS_LSE, i), c.field(taps.WS_DO, i), n.ptr(u2),
                   n.ptr(scratch), 2, int(i == 2), n.stream_ptr())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(u1).all()) and float(u1.abs().max()) > 0
        assert torch.equal(u1, u2)
    finally:
        c.close()
