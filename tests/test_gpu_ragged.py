"""GPU tests of the ragged-batch forward (rovit_attention_fwd_ragged, rovit_attention_cls_fwd_ragged, rovit_vit_forward_ragged, the
``ragged`` keyword): the attention kernels per sequence against rovit_attention_fwd / _cls_fwd at the sequence's own length, bit for
bit; the whole forward per sequence against rovit_vit_forward_tokens of that sequence alone, bit for bit, below and across the
two-stream threshold and under both MLP paths; against the fp64 forward of the kept tokens; independence of a sequence from its call;
clamped device offsets and indices; perturbation_curves and patch_shap with ragged=True.  Lengths: ragged_cases.L."""
import functools
import os

import numpy as np
import pytest
import torch

from ragged_cases import L_SHUFFLED, cycle_lengths, offsets_of

pytestmark = pytest.mark.gpu

from oracle import ref_cpu  # noqa: E402  (checker only)

FEAT_TOL, FEAT_RMS = 5e-2, 1.2e-2     # the engine's stated feature tolerance against fp64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TWO_LAUNCH, ONE_LAUNCH = 1, 2


def dev():
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _model(depth=2):
    """A RoViTKAN whose backbone holds the weights of tests/golden/vit_depth{depth}.npz (the fixture names the generator seed)."""
    from models.backbone import DeiTTiny
    from models.rovit_kan import RoViTKAN
    seed = int(np.load(os.path.join(GOLDEN, f'vit_depth{depth}.npz'))['seed'])
    sd = ref_cpu.init_rovit_state(depth=depth, seed=seed)      # its backbone: init_vit_state on the same generator, the fixture's weights
    m = RoViTKAN(pretrained=False)
    if depth != 12:
        m.backbone.model = DeiTTiny(depth=depth)
    m.load_state_dict(sd, strict=True)
    return m.to(dev()).eval(), sd


def _bb(m):
    from rovit_hip.input_grad import _Backbone
    return _Backbone(m, dev())


def _images(B, seed):
    return torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(seed))


def _tables(bb, imgs):
    t = torch.empty(imgs.shape[0], 197, 192, device=dev())
    bb.embed(imgs, t)
    return t


def _kept_rows(lengths, seed):
    """One src row set per sequence: the class token and length - 1 random patches in patch order (perturbation.source_rows)."""
    from rovit_hip.perturbation import source_rows
    g = torch.Generator().manual_seed(seed)
    return [source_rows((torch.randperm(196, generator=g) >= t - 1).view(1, 196), 'drop', t)[0] for t in lengths]


def _alone(bb, ti, img, src, mlp):
    """rovit_vit_forward_tokens of one sequence at its own length."""
    ws = bb.eng.take_ws(1, False, dev())
    f = bb.forward_tokens(ti, ti, 0, torch.tensor([img], dtype=torch.int32, device=dev()), src.view(1, -1).int().to(dev()), ws, mlp)
    bb.eng.give_ws(1, False, ws)
    return f[0]


def _ragged(bb, ti, seq_img, srcs, mlp, ws=None, off_dev=None):
    """rovit_vit_forward_ragged of the sequences packed in the order given."""
    from rovit_hip import ragged as rg
    off = offsets_of([len(s) for s in srcs])
    own = ws is None
    if own:
        ws = rg.take_ws(bb.eng, int(off[-1]), dev())
    f = bb.forward_ragged(ti, ti, 0, torch.as_tensor(seq_img, dtype=torch.int32).to(dev()), torch.cat(srcs).int().to(dev()),
                          torch.from_numpy(off).to(dev()) if off_dev is None else off_dev, off, ws, mlp)
    if own:
        bb.eng.give_ws(int(off[-1]), 'ragged', ws)
    return f


# ---- 1. the attention kernels alone ------------------------------------------------------------------------------------------------

def test_attention_kernels_equal_the_dense_kernels_per_sequence():
    from rovit_hip.native import call, ptr, stream_ptr
    H, pad = 3, 5
    off = offsets_of(L_SHUFFLED)
    n, total = len(L_SHUFFLED), int(off[-1])
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(total + pad, 3 * H * 64, generator=g).bfloat16().to(dev())
    x_rows = torch.randn(total, H * 64, generator=g).to(dev())
    off_d = torch.from_numpy(off).to(dev())
    out = torch.full((total + pad, H * 64), 7.0, dtype=torch.bfloat16, device=dev())
    lse = torch.full((H, total), -7.0, device=dev())
    call('rovit_attention_fwd_ragged', ptr(qkv), ptr(out), ptr(lse), ptr(off_d), off.ctypes.data, n, H, 64, 0.125, stream_ptr())
    out_c = torch.full((n + pad, H * 64), 7.0, dtype=torch.bfloat16, device=dev())
    lse_c = torch.full((H, total), -7.0, device=dev())
    x_cls = torch.full((n + pad, H * 64), 7.0, device=dev())
    call('rovit_attention_cls_fwd_ragged', ptr(qkv), ptr(out_c), ptr(lse_c), ptr(x_rows), ptr(x_cls), ptr(off_d), off.ctypes.data, n, H, 64,
         0.125, stream_ptr())
    for s, t in enumerate(L_SHUFFLED):
        r0 = int(off[s])
        one = qkv[r0:r0 + t].contiguous()
        o = torch.empty(t, H * 64, dtype=torch.bfloat16, device=dev())
        l2 = torch.empty(1, H, t, device=dev())
        call('rovit_attention_fwd', ptr(one), ptr(o), ptr(l2), 1, t, H, 64, 0.125, stream_ptr())
        assert torch.equal(out[r0:r0 + t], o), f'out of the sequence of {t} tokens'
        assert torch.equal(lse[:, r0:r0 + t], l2[0]), f'lse2 of the sequence of {t} tokens'
        oc = torch.zeros(t, H * 64, dtype=torch.bfloat16, device=dev())
        lc = torch.zeros(1, H, t, device=dev())
        call('rovit_attention_cls_fwd', ptr(one), ptr(oc), ptr(lc), 1, t, H, 64, 0.125, stream_ptr())
        assert torch.equal(out_c[s], oc[0]), f'class-token out of the sequence of {t} tokens'
        assert torch.equal(lse_c[:, r0], lc[0, :, 0]), f'class-token lse2 of the sequence of {t} tokens'
        assert bool((lse_c[:, r0 + 1:r0 + t] == -7.0).all())
    # nothing is written beyond the last offset / the last sequence
    assert bool((out[total:] == 7.0).all()) and bool((out_c[n:] == 7.0).all()) and bool((x_cls[n:] == 7.0).all())
    assert torch.equal(x_cls[:n], x_rows[torch.from_numpy(off[:-1]).long().to(dev())])
    # lse2 = NULL, x_rows = NULL (the inference path): the same out
    out2 = torch.full_like(out, 7.0)
    call('rovit_attention_fwd_ragged', ptr(qkv), ptr(out2), None, ptr(off_d), off.ctypes.data, n, H, 64, 0.125, stream_ptr())
    assert torch.equal(out2, out)
    out_c2 = torch.full_like(out_c, 7.0)
    call('rovit_attention_cls_fwd_ragged', ptr(qkv), ptr(out_c2), None, None, None, ptr(off_d), off.ctypes.data, n, H, 64, 0.125, stream_ptr())
    assert torch.equal(out_c2, out_c)


# ---- 2. the whole forward, bit for bit ---------------------------------------------------------------------------------------------

N_IMG = 3


@functools.lru_cache(maxsize=None)
def _cases(depth, n, mlp):
    """n sequences whose lengths cycle through the shuffled L, over three images, and every sequence's features from
    rovit_vit_forward_tokens alone at its own length: (bb, tables, seq_img, srcs, want).  Computed once per (depth, n, mlp)."""
    m, _ = _model(depth)
    bb = _bb(m)
    ti = _tables(bb, _images(N_IMG, 50 + depth).to(dev()))
    lengths = cycle_lengths(n)
    srcs = _kept_rows(lengths, 60 + depth)
    seq_img = [i % N_IMG for i in range(n)]
    want = torch.stack([_alone(bb, ti, seq_img[i], srcs[i], mlp) for i in range(n)])
    return bb, ti, seq_img, srcs, want


@pytest.mark.parametrize('mlp', [TWO_LAUNCH, ONE_LAUNCH])
@pytest.mark.parametrize('pick', ['one_token', 'full_length', 'L_below_two_streams', '37_across_two_streams'])
def test_forward_equals_forward_tokens_of_each_sequence_alone(pick, mlp):
    bb, ti, seq_img, srcs, want = _cases(2, 37, mlp)
    idx = {'one_token': [1], 'full_length': [2], 'L_below_two_streams': list(range(14)), '37_across_two_streams': list(range(37))}[pick]
    assert [len(srcs[i]) for i in idx] == {'one_token': [1], 'full_length': [197]}.get(pick, cycle_lengths(len(idx)))
    got = _ragged(bb, ti, [seq_img[i] for i in idx], [srcs[i] for i in idx], mlp)
    assert torch.equal(got, want[idx])


def test_forward_depth_12_sixteen_sequences():
    bb, ti, seq_img, srcs, want = _cases(12, 16, ONE_LAUNCH)
    assert torch.equal(_ragged(bb, ti, seq_img, srcs, ONE_LAUNCH), want)


# ---- 3. against the fp64 forward of the kept tokens --------------------------------------------------------------------------------

def test_forward_against_fp64_forward_of_the_kept_tokens():
    from test_gpu_perturbation import _vit64_kept          # the fp64 statement of the backbone on a subset of tokens
    m, sd = _model(2)
    sd64 = {k: v.double() for k, v in sd.items()}
    bb = _bb(m)
    x = _images(N_IMG, 70)
    srcs = _kept_rows(L_SHUFFLED, 71)
    seq_img = [i % N_IMG for i in range(len(srcs))]
    got = _ragged(bb, _tables(bb, x.to(dev())), seq_img, srcs, TWO_LAUNCH).cpu().double()
    want = torch.cat([_vit64_kept(x[i:i + 1].double(), sd64, s.view(1, -1).long()) for i, s in zip(seq_img, srcs)])
    err = (got - want).abs()
    rms = float(err.pow(2).mean().sqrt())
    print(f'ragged L against fp64: max-abs {float(err.max()):.2e} rms {rms:.2e}')
    assert float(err.max()) < FEAT_TOL and rms < FEAT_RMS


# ---- 4. independence and clamping --------------------------------------------------------------------------------------------------

def test_a_sequence_does_not_depend_on_its_call():
    from rovit_hip import ragged as rg
    bb, ti, seq_img, srcs, _ = _cases(2, 37, TWO_LAUNCH)
    a = 6                                                      # 49 tokens
    alone = _ragged(bb, ti, [seq_img[a]], [srcs[a]], TWO_LAUNCH)[0]
    others = [i for i in range(20) if i != a]
    first = _ragged(bb, ti, [seq_img[i] for i in [a] + others], [srcs[i] for i in [a] + others], TWO_LAUNCH)[0]
    last = _ragged(bb, ti, [seq_img[i] for i in others + [a]], [srcs[i] for i in others + [a]], TWO_LAUNCH)[-1]
    assert torch.equal(alone, first) and torch.equal(alone, last)
    # the same 37 sequences through ragged_layout at two max_rows: one call, and calls of at most 400 rows
    lengths = [len(s) for s in srcs]
    feats = []
    for max_rows in (197 * 256, 400):
        calls, perm = rg.ragged_layout(lengths, max_rows)
        assert (len(calls) == 1) == (max_rows > 400)
        f = torch.cat([_ragged(bb, ti, [seq_img[i] for i in seq], [srcs[i] for i in seq], TWO_LAUNCH) for seq, _ in calls])
        feats.append(f[torch.from_numpy(perm).to(dev())])
    assert torch.equal(feats[0], feats[1])
    assert torch.equal(feats[0][a], alone)


def test_device_offsets_that_disagree_stay_inside_the_buffers():
    """The kernels clamp what they read from the device copy of the offsets: with one length of 300 there (and every later offset
    shifted beyond the rows) the call computes on wrong rows, but finite values come out and nothing outside the workspace or the
    features is written (sentinel bytes around both)."""
    from rovit_hip.native import load
    bb, ti, seq_img, srcs, want = _cases(2, 37, TWO_LAUNCH)
    idx = list(range(14))
    lengths = [len(srcs[i]) for i in idx]
    off = offsets_of(lengths)
    bad = list(lengths)
    bad[3] = 300
    off_bad = torch.from_numpy(offsets_of(bad)).to(dev())
    need, pad = load().rovit_vit_ragged_workspace_bytes(int(off[-1]), 2), 4096
    big = torch.full((need + 2 * pad,), 0xA5, dtype=torch.uint8, device=dev())
    got = _ragged(bb, ti, [seq_img[i] for i in idx], [srcs[i] for i in idx], TWO_LAUNCH, ws=big[pad:pad + need], off_dev=off_bad)
    assert bool(torch.isfinite(got).all()) and tuple(got.shape) == (14, 192)
    assert bool((big[:pad] == 0xA5).all()) and bool((big[pad + need:] == 0xA5).all())
    assert torch.equal(got[:3], want[:3])                      # the sequences in front of the bad length are untouched by it
    # the same workspace with the true offsets: the true features
    good = _ragged(bb, ti, [seq_img[i] for i in idx], [srcs[i] for i in idx], TWO_LAUNCH, ws=big[pad:pad + need])
    assert torch.equal(good, want[idx])


def test_image_and_row_indices_are_clamped_into_the_tables():
    bb, ti, _, _, _ = _cases(2, 37, TWO_LAUNCH)
    bad = [torch.arange(197), torch.arange(33), torch.arange(2), torch.arange(16)]
    bad[0][5], bad[1][7], bad[2][1], bad[3][15] = 100000, -100000, -(2 ** 31), 2 ** 31 - 1
    good = [b.clone() for b in bad]
    good[0][5], good[1][7], good[2][1], good[3][15] = 196, -197, -197, 196
    got = _ragged(bb, ti, [-4, 1, 99, 2], bad, TWO_LAUNCH)
    want = _ragged(bb, ti, [0, 1, 2, 2], good, TWO_LAUNCH)
    assert torch.equal(got, want)


# ---- 5. user level -----------------------------------------------------------------------------------------------------------------

def test_perturbation_curves_ragged_equal_forward_tokens_per_sequence():
    """perturbation='drop', ragged=True, steps 7, batch 3: every value of the curves from rovit_vit_forward_tokens of that one sequence
    at the MLP path the ragged calls take (chunk 256 x 197 rows: one launch)."""
    from rovit_hip.input_grad import _head_outputs, _target_value
    from rovit_hip.perturbation import _ranks, patch_order, perturbed_mask, source_rows, step_counts
    m, _ = _model(2)
    bb = _bb(m)
    B, steps = 3, 7
    x = _images(B, 80).to(dev())
    sal = torch.randn(B, 14, 14, generator=torch.Generator().manual_seed(81))
    res = m.perturbation_curves(x, sal, target='mu', steps=steps, perturbation='drop', ragged=True)
    ti = _tables(bb, x)
    rank = _ranks(patch_order(sal))
    ks = step_counts(steps)
    for mode in ('deletion', 'insertion'):
        feats = []
        for b in range(B):
            for k in ks:
                pert = perturbed_mask(rank[b:b + 1], mode == 'deletion', k)
                tokens = 197 - int(pert.sum())
                feats.append(_alone(bb, ti, b, source_rows(pert, 'drop', tokens)[0], ONE_LAUNCH))
        want = _target_value('mu', _head_outputs(m, torch.stack(feats)), None).view(B, steps + 1)
        assert torch.equal(res[mode], want), mode
    again = m.perturbation_curves(x, sal, target='mu', steps=steps, perturbation='drop', ragged=True)
    assert all(torch.equal(res[k], again[k]) for k in res)
    # 'replace': every sequence has 197 tokens and the flag changes nothing
    rep = m.perturbation_curves(x, sal, target='mu', steps=steps, perturbation='replace', ragged=True)
    ref = m.perturbation_curves(x, sal, target='mu', steps=steps, perturbation='replace')
    assert all(torch.equal(rep[k], ref[k]) for k in rep)


def test_patch_shap_ragged_is_efficient_and_repeatable():
    """players=2 enumerates all 14 coalitions: the values sum to f(image) - f(nothing) within tests/test_gpu_shap.py's efficiency
    bound (the fp32 rounding of each player value plus the fp64 solve's 1e-12), are the same from run to run, and every coalition's
    value is rovit_vit_forward_tokens' of that sequence alone at the ragged calls' MLP path."""
    from rovit_hip.input_grad import _head_outputs
    from rovit_hip.perturbation import source_rows
    from rovit_hip.shap import player_map
    m, _ = _model(2)
    B = 2
    x = _images(B, 90).to(dev())
    res = m.patch_shap(x, players=2, num_samples=14, perturbation='drop', ragged=True, return_values=True)
    assert res['exact'] and res['num_samples'] == 14 and bool(res['ok'].all())
    pv = res['player_values'].double()
    gap = (res['value'].double() - res['base_value'].double() - pv.sum(1)).abs()
    tol = 2.0 ** -24 * pv.abs().sum(1) + 1e-12
    print('efficiency gap', gap.cpu().numpy(), 'tol', tol.cpu().numpy())
    assert bool((gap <= tol).all())
    again = m.patch_shap(x, players=2, num_samples=14, perturbation='drop', ragged=True, return_values=True)
    for k in ('shap', 'player_values', 'base_value', 'value', 'fit_rmse', 'ok', 'class_idx', 'values'):
        assert torch.equal(res[k], again[k]), k
    bb = _bb(m)
    ti = _tables(bb, x)
    pmap = torch.from_numpy(player_map(2, 'test')).to(dev()).long()
    absent = ~res['coalitions'][:, pmap]
    feats = [_alone(bb, ti, b, source_rows(absent[c:c + 1], 'drop', 197 - int(absent[c].sum()))[0], ONE_LAUNCH)
             for c in range(14) for b in range(B)]
    p = torch.softmax(_head_outputs(m, torch.stack(feats))[0], 1).view(14, B, -1)
    want = p.gather(2, res['class_idx'].view(1, B, 1).expand(14, B, 1)).squeeze(2)
    assert torch.equal(res['values'], want)
    from explainability import PatchSHAP
    got = PatchSHAP(m, device=dev()).explain_batch(x.cpu(), players=2, num_samples=14, ragged=True)
    assert torch.equal(got['player_values'], res['player_values'])
