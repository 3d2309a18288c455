"""GPU tests of every token row of every block of the backbone forwards, against fp64 runs of the oracle's blocks
(oracle/ref_cpu.py: vit_block_taps / vit_block_forward).

The other model-level tests see the backbone through its features: the final LayerNorm of the class-token row, which a wrong patch row
of a late block barely moves (and the last block does not consume at all).  Here:
  * bf16 training forward: every saved field of every block (include/rovit_hip.h: rovit_vit_workspace_field) against an fp64 run of the
    same block fed with the engine's own block input XHAT1_i / RSTD1_i (every later quantity is invariant to the row mean this drops),
    at tail tiles, the two half-batch chains, both MLP-half paths, and a peaked softmax.
  * fp32 forward (rovit_vit_forward_f32): X / QKV / ATTN_O / ACT after every depth, chained from the images, against one fp64 run; the
    bound calibrates itself on the fp32 CPU oracle's own distance to fp64 on the same rows.
  * the same for rows whose LayerNorm inputs are an offset plus a small signal (mean^2 / var from 0 to 1e4), on both sides of the
    fp32 forward's one-pass / two-pass switch.
  * each comparator rejects a copy of the engine's output with one element of one row changed.
Per row: max-abs error / max(max |reference row|, 1)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref_cpu  # noqa: E402  (checker only)

# bf16 fields against the teacher-forced fp64 block: per-row error / row scale, 1.5x the worst measured over BF16_CASES (DESIGN.md
# section 2; measured: xhat1 7.2e-3, rstd1 9.2e-4, qkv 5.4e-3, attn_o 1.0e-3 (4.8e-3 with the peaked softmax), xhat2 7.6e-3, rstd2 9.3e-4,
# act 8.8e-3, features 3.6e-3)
BF16_TOL = {'xhat1': 1.1e-2, 'rstd1': 1.4e-3, 'qkv': 8e-3, 'attn_o': 7.5e-3, 'xhat2': 1.15e-2, 'rstd2': 1.4e-3, 'act': 1.35e-2,
            'features': 5.5e-3}
# fp32 fields: the GPU's worst row error against fp64 may be F32_RATIO x the fp32 CPU oracle's on the same rows, plus F32_FLOOR
F32_RATIO, F32_FLOOR = 4.0, 1e-7
EPS = 1e-6
ROWS = 197


def dev():
    return torch.device('cuda:0')


def _vit_sd(depth, seed, peaked=False):
    """init_vit_state weights; peaked: qkv weights at std 0.15 and LayerNorm gamma = 1 + N(0, 0.3) -- a softmax far from uniform."""
    g = torch.Generator().manual_seed(seed)
    sd = ref_cpu.init_vit_state(depth, g)
    if peaked:
        for i in range(depth):
            b = f'blocks.{i}.'
            sd[b + 'attn.qkv.weight'] = torch.randn(576, 192, generator=g) * 0.15
            for n in ('norm1', 'norm2'):
                sd[b + n + '.weight'] = 1.0 + 0.3 * torch.randn(192, generator=g)
    return sd


def _images(B, seed):
    return torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(seed))


def _backbone(sd, depth):
    from models.backbone import DeiTTiny
    m = DeiTTiny(depth=depth)
    m.load_state_dict(sd, strict=True)
    return m.to(dev())


def _ln(t):
    """LayerNorm without its affine, and 1 / sqrt(var + eps) (biased variance)."""
    var = t.var(dim=-1, unbiased=False, keepdim=True)
    return (t - t.mean(-1, keepdim=True)) * (var + EPS).rsqrt(), (var + EPS).rsqrt().squeeze(-1)


def _row_err(got, ref):
    """Per row: max |got - ref| / max(max |ref row|, 1); got and ref hold the same rows (a trailing width may be absent: RSTD)."""
    r = ref.detach().double().cpu().reshape(ref.shape[0] if ref.dim() > 1 else ref.numel(), -1)
    g = got.detach().double().cpu().reshape(r.shape)
    return (g - r).abs().amax(1) / r.abs().amax(1).clamp_min(1.0)


def _bf16_worst(got, ref):
    """The bf16 comparator: the worst row (NaN if any row is not finite)."""
    e = _row_err(got, ref)
    return float('nan') if not torch.isfinite(e).all() else float(e.max())


# ---- bf16 training forward: every saved field of every block ----------------------------------------------------------------

def _bf16_fields(m, x, mlp_path):
    """Grad-mode forward; every field of every block through engine.last_ws (copied to the host, fp64)."""
    from rovit_hip import taps
    eng = m.engine
    eng.mlp_path = mlp_path
    feats = m(x.to(dev()))
    ws, B, path = eng.last_ws
    names = {'xhat1': taps.WS_XHAT1, 'rstd1': taps.WS_RSTD1, 'qkv': taps.WS_QKV, 'attn_o': taps.WS_ATTN_O, 'xhat2': taps.WS_XHAT2,
             'rstd2': taps.WS_RSTD2, 'act': taps.WS_ACT}
    out = [{n: taps.workspace_view(ws, B, eng.depth, f, i, path).double().cpu() for n, f in names.items()} for i in range(eng.depth)]
    feats = feats.detach().double().cpu()
    eng.mlp_path = None
    return out, feats


def _attention(qkv, B):
    """fp64 attention of qkv rows (B * 197, 576): the output before proj (B * 197, 192) and every softmax row's largest probability."""
    q, k, v = qkv.view(B, ROWS, 3, 3, 64).permute(2, 0, 3, 1, 4)
    a = torch.softmax((q * 0.125) @ k.transpose(-2, -1), dim=-1)
    return (a @ v).transpose(1, 2).reshape(B * ROWS, 192), a.amax(-1).flatten()


def _bf16_compare(fields, feats, x, sd, depth):
    """fp64 reference of every field of every block, each block fed with the engine's own block input XHAT1_i / RSTD1_i and each stage of it
    with the engine's own output of the stage before (so a field's error is its kernel's, not a peaked softmax's amplification of a bf16
    rounding upstream); the stream leaving the block (t_in + proj + fc2) is checked through XHAT1_{i+1} / RSTD1_{i+1}, and the last block's
    through the features.  Returns ({field: worst row error}, each field's first (got, ref) pair, every softmax row's largest probability)."""
    B = x.shape[0]
    sd64 = {k: v.double() for k, v in sd.items()}
    worst, pairs, pmax = {}, {}, []

    def cmp(name, got, ref, i):
        w, prev = _bf16_worst(got, ref), worst.get(name, 0.0)
        worst[name] = float('nan') if w != w or prev != prev else max(w, prev)
        pairs.setdefault(name, (got, ref))

    with torch.no_grad():
        xh, rs = _ln(ref_cpu.vit_embed(x.double(), sd64).reshape(-1, 192))        # block 0's input: the fp64 patch embedding
        cmp('xhat1', fields[0]['xhat1'], xh, 0)
        cmp('rstd1', fields[0]['rstd1'], rs, 0)
        for i in range(depth):
            f, p = fields[i], lambda n: sd64[f'blocks.{i}.{n}']                     # noqa: B023
            t_in = f['xhat1'] / f['rstd1']                                            # (M, 192); rstd1 is (M, 1)
            cmp('qkv', f['qkv'], F.linear(f['xhat1'] * p('norm1.weight') + p('norm1.bias'), p('attn.qkv.weight'), p('attn.qkv.bias')), i)
            o, pm = _attention(f['qkv'], B)
            pmax.append(pm)
            if i == depth - 1:                                                        # the last block: class-token rows only
                o, t_in = o.view(B, ROWS, 192)[:, 0], t_in.view(B, ROWS, 192)[:, 0]
            cmp('attn_o', f['attn_o'], o, i)
            xh2, rs2 = _ln(t_in + F.linear(f['attn_o'], p('attn.proj.weight'), p('attn.proj.bias')))
            cmp('xhat2', f['xhat2'], xh2, i)
            cmp('rstd2', f['rstd2'], rs2, i)
            cmp('act', f['act'], F.gelu(F.linear(f['xhat2'] * p('norm2.weight') + p('norm2.bias'), p('mlp.fc1.weight'), p('mlp.fc1.bias'))), i)
            t_out = xh2 / rs2.unsqueeze(-1) + F.linear(f['act'], p('mlp.fc2.weight'), p('mlp.fc2.bias'))   # (the row mean dropped again)
            if i < depth - 1:
                xh, rs = _ln(t_out)
                cmp('xhat1', fields[i + 1]['xhat1'], xh, i + 1)
                cmp('rstd1', fields[i + 1]['rstd1'], rs, i + 1)
            else:
                cmp('features', feats, F.layer_norm(t_out, (192,), sd64['norm.weight'], sd64['norm.bias'], EPS), i)
    return worst, pairs, torch.cat(pmax)


BF16_CASES = [  # depth, batch, mlp_path ('one' / 'two' / None = AUTO), peaked weights
    (12, 1, 'two', False), (12, 1, 'one', False), (12, 3, 'two', False), (12, 3, 'one', False),
    (12, 17, None, False),                                   # two half-batch chains (9 / 8 images)
    (4, 67, 'two', False), (4, 67, 'one', False),            # 13 199 rows: tail tiles in both chains
    (4, 172, None, False), (4, 173, None, False),            # 33 884 / 34 081 rows: the two sides of AUTO's one-launch switch
    (12, 3, None, True), (4, 17, None, True),
]


def _mlp(path):
    from rovit_hip import native
    return {None: None, 'one': native.MLP_ONE_LAUNCH, 'two': native.MLP_TWO_LAUNCH}[path]


@pytest.mark.parametrize('depth,B,path,peaked', BF16_CASES,
                         ids=[f'd{d}-b{b}-{p or "auto"}{"-peaked" if k else ""}' for d, b, p, k in BF16_CASES])
def test_bf16_training_forward_every_row_of_every_block(depth, B, path, peaked):
    sd = _vit_sd(depth, seed=100 + B + depth, peaked=peaked)
    x = _images(B, seed=B)
    m = _backbone(sd, depth)
    fields, feats = _bf16_fields(m, x, _mlp(path))
    worst, _, pmax = _bf16_compare(fields, feats, x, sd, depth)
    med = float(pmax.median())
    print(f'bf16 d{depth} b{B} {path or "auto"}{" peaked" if peaked else ""}: median softmax row max {med:.3f}; worst per field',
          {k: f'{v:.2e}' for k, v in worst.items()})
    if peaked:
        assert med >= 0.3, med
    assert set(worst) == set(BF16_TOL)
    for k, v in worst.items():
        assert v <= BF16_TOL[k], (k, v)


def test_bf16_comparator_rejects_one_bad_row():
    """Every field (block 0's; the features) with one element of one patch row moved by 5 % of that row's scale fails the comparator."""
    depth, B = 2, 3
    sd = _vit_sd(depth, seed=7)
    x = _images(B, seed=7)
    fields, feats = _bf16_fields(_backbone(sd, depth), x, None)
    worst, pairs, _ = _bf16_compare(fields, feats, x, sd, depth)
    assert all(v <= BF16_TOL[k] for k, v in worst.items()), worst
    assert set(pairs) == set(BF16_TOL)
    for name, (got, ref) in pairs.items():
        bad = got.clone().reshape(ref.shape[0] if ref.dim() > 1 else ref.numel(), -1)
        r = ROWS + 100 if bad.shape[0] > B else 1                               # a patch row of image 1 (features: image 1)
        scale = max(float(ref.reshape(bad.shape)[r].abs().max()), 1.0)
        bad[r, bad.shape[1] // 2] += 0.05 * scale
        assert _bf16_worst(got, ref) <= BF16_TOL[name], name
        assert _bf16_worst(bad, ref) > BF16_TOL[name], name


# ---- fp32 forward: chained, against fp64 --------------------------------------------------------------------------------------

F32_FIELDS = {'X': 't_out', 'QKV': 'qkv', 'ATTN_O': 'attn_o', 'ACT': 'act'}


class _F32:
    """rovit_vit_forward_f32 on one model and batch; after forward(depth) the workspace fields hold block depth-1."""

    def __init__(self, sd, depth, x):
        from rovit_hip import native
        m = _backbone(sd, depth)
        self.params = [p.detach().float().contiguous() for p in m.ordered_parameters()]
        self.x = x.float().contiguous().to(dev())
        self.B = x.shape[0]
        self.ws = torch.empty(native.load().rovit_vit_f32_workspace_bytes(self.B), dtype=torch.uint8, device=dev())
        self.feats = torch.empty(self.B, 192, device=dev())

    def forward(self, depth):
        from rovit_hip import taps
        from rovit_hip.native import call, ptr, ptr_array, stream_ptr
        call('rovit_vit_forward_f32', ptr(self.x), ptr_array(self.params), ptr(self.ws), ptr(self.feats), self.B, depth, stream_ptr())
        idx = {'X': taps.F32_WS_X, 'QKV': taps.F32_WS_QKV, 'ATTN_O': taps.F32_WS_ATTN_O, 'ACT': taps.F32_WS_ACT}
        return {n: taps.f32_workspace_view(self.ws, self.B, f).double().cpu() for n, f in idx.items()}


def _f32_verdict(got, cpu32, ref64):
    """The fp32 comparator: (the GPU's worst row error, its bound from the CPU oracle's worst on the same rows)."""
    e_gpu = _row_err(got, ref64)
    e_cpu = _row_err(cpu32, ref64)
    worst = float('nan') if not torch.isfinite(e_gpu).all() else float(e_gpu.max())
    return worst, F32_RATIO * float(e_cpu.max()) + F32_FLOOR


def _f32_taps(x, sd, depth):
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        t64, _ = ref_cpu.vit_block_taps(x.double(), sd64, eps=EPS, depth=depth)
        t32, _ = ref_cpu.vit_block_taps(x.float(), sd, eps=EPS, depth=depth)
    flat = lambda tp: {n: tp[k].reshape(-1, tp[k].shape[-1]) for n, k in F32_FIELDS.items()}  # noqa: E731
    return [flat(t) for t in t64], [flat(t) for t in t32]


def _f32_check_depths(sd, x, depths, label, groups=None):
    """Forward at each depth; every field against fp64, the bound calibrated separately on each group of token rows (groups: name ->
    row indices; None: all rows in one group).  Returns {field: worst GPU error / bound} over the depths and groups."""
    run = _F32(sd, max(depths), x)
    t64, t32 = _f32_taps(x, sd, max(depths))
    ratio, bad = {}, []
    for d in depths:
        got = run.forward(d)
        for n in F32_FIELDS:
            for gname, rows in (groups or {'': None}).items():
                g, c, r = got[n], t32[d - 1][n], t64[d - 1][n]
                if rows is not None:
                    g, c, r = g[rows], c[rows], r[rows]
                worst, bound = _f32_verdict(g, c, r)
                print(f'fp32 {label} depth {d} {n}{gname}: GPU {worst:.2e}, bound {bound:.2e} (CPU fp32 {(bound - F32_FLOOR) / F32_RATIO:.2e})')
                if not worst <= bound:
                    bad.append((d, n + gname, worst, bound))
                ratio[n] = max(ratio.get(n, 0.0), worst / bound)
    assert not bad, (label, bad)
    return ratio


@pytest.mark.parametrize('B', [1, 3, 7])
def test_fp32_forward_every_row_after_every_depth(B):
    """M = 197, 591 and 1379 rows (the last padded to 16 row tiles), one chain; depth 1..12 chained from the images."""
    sd = _vit_sd(12, seed=200 + B)
    ratio = _f32_check_depths(sd, _images(B, seed=50 + B), list(range(1, 13)), f'b{B}')
    print(f'fp32 b{B}: worst GPU error / bound per field', {k: f'{v:.2f}' for k, v in ratio.items()})


def test_fp32_forward_one_chain_and_two_chains_every_row():
    """Batches 191 (one chain), 192 (two chains of 96) and 193 (97 / 96) at depth 2."""
    sd = _vit_sd(2, seed=300)
    x = _images(193, seed=301)
    for B in (191, 192, 193):
        ratio = _f32_check_depths(sd, x[:B], [2], f'b{B}')
        print(f'fp32 b{B}: worst GPU error / bound per field', {k: f'{v:.2f}' for k, v in ratio.items()})


def test_fp32_forward_peaked_softmax_every_row():
    sd = _vit_sd(12, seed=400, peaked=True)
    x = _images(3, seed=401)
    t64, _ = _f32_taps(x, sd, 1)
    med = float(_attention(t64[0]['QKV'], 3)[1].median())
    assert med >= 0.3, med
    ratio = _f32_check_depths(sd, x, list(range(1, 13)), 'b3 peaked')
    print(f'fp32 b3 peaked (median softmax row max {med:.3f} in block 0): worst GPU error / bound per field',
          {k: f'{v:.2f}' for k, v in ratio.items()})


LN_RATIOS = (0.0, 1.0, 4.0, 16.0, 48.0, 63.0, 66.0, 100.0, 1e4)


def _offset_sd(B, seed):
    """pos_embed shifted by a per-token constant: block 0's norm1 rows sit at mean^2 / var ~ LN_RATIOS[token % 9]."""
    sd = _vit_sd(3, seed=seed)
    x = _images(B, seed=seed + 1)
    with torch.no_grad():
        t0 = ref_cpu.vit_embed(x.double(), {k: v.double() for k, v in sd.items()})
        mean, var = t0.mean(-1).mean(0), t0.var(-1, unbiased=False).mean(0)         # per token, over the images
        want = torch.tensor([LN_RATIOS[n % len(LN_RATIOS)] for n in range(ROWS)], dtype=torch.float64)
        shift = (want * var).sqrt() - mean
        sd['pos_embed'] = (sd['pos_embed'].double() + shift.view(1, ROWS, 1)).float()
        t0 = ref_cpu.vit_embed(x.double(), {k: v.double() for k, v in sd.items()})
        ratio = (t0.mean(-1) ** 2 / t0.var(-1, unbiased=False)).flatten()
    return sd, x, ratio


def test_fp32_layernorm_rows_on_both_sides_of_the_two_pass_switch():
    """The fp32 forward takes LayerNorm statistics from one-pass sums and recomputes a row in two passes when mean^2 is large against
    var (csrc/vit_f32.hip, F32Ln).  Rows from mean^2 / var = 0 to 1e4 (the residual stream keeps the offset through the later blocks'
    LayerNorms) must be as close to fp64 as the fp32 CPU oracle's, whichever side of the switch they fall on."""
    sd, x, ratio = _offset_sd(3, seed=500)
    below = int(((ratio >= 16) & (ratio < 64)).sum())
    above = int((ratio >= 64).sum())
    print(f'rows at mean^2 / var in [16, 64): {below}, >= 64: {above}')
    assert below >= 10 and above >= 10, (below, above)
    # each band of rows is held to the CPU oracle's error on that band (the rows at 1e4 carry the largest rounding of all, x - mean at
    # |x| ~ 55, and would otherwise set the bound for the rest)
    bands = {f' mean^2/var in [{lo:g}, {hi:g})': torch.nonzero((ratio >= lo) & (ratio < hi)).flatten()
             for lo, hi in ((0, 0.5), (0.5, 16), (16, 64), (64, 1000), (1000, float('inf')))}
    assert all(len(v) for v in bands.values())
    r = _f32_check_depths(sd, x, [1, 2, 3], 'offset rows', bands)
    print('fp32 offset rows: worst GPU error / bound per field', {k: f'{v:.2f}' for k, v in r.items()})


def test_fp32_comparator_rejects_one_bad_row():
    """Every field with one element of one patch row moved by 1e-4 of that row's scale fails the comparator."""
    sd = _vit_sd(2, seed=600)
    x = _images(3, seed=601)
    run = _F32(sd, 2, x)
    t64, t32 = _f32_taps(x, sd, 2)
    got = run.forward(2)
    for n in F32_FIELDS:
        worst, bound = _f32_verdict(got[n], t32[1][n], t64[1][n])
        assert worst <= bound, (n, worst, bound)
        bad = got[n].clone()
        r = ROWS + 100
        bad[r, bad.shape[1] // 2] += 1e-4 * max(float(t64[1][n][r].abs().max()), 1.0)
        worst, bound = _f32_verdict(bad, t32[1][n], t64[1][n])
        assert worst > bound, (n, worst, bound)
