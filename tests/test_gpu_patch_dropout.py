"""GPU tests of PatchDropout training (rovit_hip.patch_dropout; csrc/patch_dropout.hip, rovit_vit_forward_train_tokens and
rovit_vit_backward_tokens in csrc/vit.hip): the draw against its numpy statement, the scatter, bit-identity with the dense path at
k = 196, the forward on kept tokens against the inference token forward, the backward against an fp64 oracle with the dense path's own
error as the yardstick, exact zeros for dropped patches, and the module / Trainer semantics.

Backward bound (per parameter tensor, rel = ||g - g64|| / ||g64||): rel_T <= 2 * sqrt(197 / T) * rel_dense, rel_dense measured in the same
test on the same weights, images and w.  A gradient is a sum over rows of products with independent bf16 roundings, so its relative error
grows at most like 1 / sqrt(rows) when the signal is coherent and not at all when it is not; the factor 2 covers the seed.  Cases whose
bound is 0.5 or more would prove nothing; none has one (largest bound 0.15 at T = 2, largest rel_T / bound 0.47: DESIGN.md section 2).  With ROVIT_PATCH_DROPOUT_ERROR_OUT set to a file name every measured
pair is appended to it as one JSON line (profiles/patch_dropout_error.jsonl was written that way)."""
import copy
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref_cpu  # noqa: E402  (checker only)

TOKENS = 197
BATCHES = (1, 3, 17)          # 17: the two-stream split with an odd cut (9 + 8)


def dev():
    return torch.device('cuda:0')


def _paths():
    from rovit_hip import native
    return (native.MLP_TWO_LAUNCH, native.MLP_ONE_LAUNCH)


_SD = {}


def _sd(depth):
    if depth not in _SD:
        _SD[depth] = ref_cpu.init_vit_state(depth, torch.Generator().manual_seed(100 + depth))
    return _SD[depth]


def _vit(depth):
    from models.backbone import DeiTTiny
    m = DeiTTiny(depth=depth)
    m.load_state_dict(_sd(depth), strict=True)
    return m.to(dev()).train()


def _images(B):
    return torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B))


def _w(B):
    return torch.randn(B, 192, generator=torch.Generator().manual_seed(1000 + B))


def _keep(B, k):
    """Per-sample different subsets (for k < 196)."""
    from rovit_hip import patch_dropout as pd
    return pd.draw_reference(77, k, B, k)


def _grads_of(m, run):
    """Parameter gradients {name: fp32 cpu} of one forward + backward, written into a NaN-poisoned flat buffer."""
    params = m.ordered_parameters()
    for p in params:
        p.grad = None
    m.engine.ensure_grads(params)
    m.engine.grad_flat.fill_(float('nan'))
    feats = run()
    (feats * _w(feats.shape[0]).to(dev())).sum().backward()
    torch.cuda.synchronize()
    return feats.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


# ---- the draw and the scatter ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [1, 15, 98, 196])
def test_draw_equals_the_numpy_statement(k):
    from rovit_hip import native, patch_dropout as pd
    B, seed, step = 17, (5 << 32) + 123, (9 << 32) + 4          # both 64-bit words of the seed and of the step in use
    want = pd.draw_reference(seed, step, B, k)
    want_src, want_inv = pd.maps_reference(want)
    outs = []
    for _ in range(2):
        keep = torch.full((B, k), -12345, dtype=torch.int32, device=dev())
        src = torch.full((B, 1 + k), -12345, dtype=torch.int32, device=dev())
        inv = torch.full((B, TOKENS), -12345, dtype=torch.int32, device=dev())
        native.call('rovit_patch_dropout_draw', seed, step, native.ptr(keep), native.ptr(src), native.ptr(inv), B, k, native.stream_ptr())
        outs.append((keep.cpu().numpy(), src.cpu().numpy(), inv.cpu().numpy()))
    assert (outs[0][0] == want).all() and (outs[0][1] == want_src).all() and (outs[0][2] == want_inv).all()
    assert all((a == b).all() for a, b in zip(*outs))
    got = pd.draw(seed, step, B, k, dev())
    assert all((g.cpu().numpy() == o).all() for g, o in zip(got, outs[0]))
    for bad in (0, 197):
        with pytest.raises(native.RovitHipError):
            native.call('rovit_patch_dropout_draw', seed, step, native.ptr(keep), native.ptr(src), native.ptr(inv), B, bad, native.stream_ptr())


@pytest.mark.parametrize('B,k', [(1, 1), (3, 31), (17, 100), (2, 196)])
def test_scatter_writes_every_dense_row_once(B, k):
    from rovit_hip import native, patch_dropout as pd
    T = 1 + k
    keep = _keep(B, k) if k < 196 else np.tile(np.arange(196), (B, 1))
    src, inv = pd.maps_reference(keep)
    rows = torch.randn(B * T, 192, generator=torch.Generator().manual_seed(k)).to(torch.bfloat16).to(dev())
    dense = torch.full((B * TOKENS, 192), float('nan'), dtype=torch.bfloat16, device=dev())
    native.call('rovit_scatter_token_rows', native.ptr(rows), native.ptr(torch.from_numpy(inv).to(dev())), native.ptr(dense), B, T,
                native.stream_ptr())
    want = torch.zeros(B, TOKENS, 192, dtype=torch.bfloat16)
    r = rows.cpu().view(B, T, 192)
    for b in range(B):
        want[b, torch.from_numpy(src[b]).long()] = r[b]
    got = dense.cpu().view(B, TOKENS, 192)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))            # bits: copied rows, and +0.0 (not -0.0) where dropped
    # an index outside the short sequence is a dropped row, not a read outside `rows`
    bad = torch.from_numpy(inv).to(dev())
    bad[0, 5] = T
    bad[0, 6] = -9
    native.call('rovit_scatter_token_rows', native.ptr(rows), native.ptr(bad), native.ptr(dense), B, T, native.stream_ptr())
    assert float(dense.view(B, TOKENS, 192)[0, 5:7].abs().max()) == 0.0


# ---- k = 196: the token path, forced, is the dense path bit for bit ---------------------------------------------------------------------

def _identity_case(depth, B, mlp_path):
    from rovit_hip import patch_dropout as pd
    m = _vit(depth)
    m.engine.mlp_path = mlp_path
    x = _images(B).to(dev())
    f_dense, g_dense = _grads_of(m, lambda: m(x))
    f_tok, g_tok = _grads_of(m, lambda: pd.forward_kept(m, x, np.tile(np.arange(196), (B, 1))))
    assert torch.isfinite(f_dense).all() and torch.equal(f_dense, f_tok)
    for n in g_dense:
        assert torch.isfinite(g_dense[n]).all(), n
        assert torch.equal(g_dense[n], g_tok[n]), n


@pytest.mark.parametrize('B', BATCHES)
def test_identity_at_k196_depth2(B):
    for path in _paths():
        _identity_case(2, B, path)


def test_identity_at_k196_depth12():
    _identity_case(12, 3, None)


# ---- forward on kept tokens -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [1, 15, 16, 31, 32, 100])        # T = k + 1: the 16-key tile edges and the 32-key P.V block edges
def test_forward_equals_the_inference_token_forward_and_repeats(k):
    """The rule the existing tests hold between the dense training and inference forwards is bit-identity
    (test_gpu_model.py::test_inference_workspace_equals_training_forward_ragged_batches); the same here, against
    rovit_vit_forward_tokens of the same rows, and run to run."""
    from rovit_hip import native, patch_dropout as pd
    from rovit_hip.native import call, ptr, ptr_array, stream_ptr
    m = _vit(2)
    eng, params, T = m.engine, m.ordered_parameters(), 1 + k
    eng.prepare(params)
    lib = native.load()
    for B in BATCHES:
        x = _images(B).to(dev())
        src, inv = pd.maps_reference(_keep(B, k))
        src = torch.from_numpy(src).to(dev())
        seq = torch.arange(B, dtype=torch.int32, device=dev())
        parr = ptr_array(params)
        for path in _paths():
            feats = []
            for _ in range(2):
                ws = torch.empty(lib.rovit_vit_workspace_bytes(B, 2, 1), dtype=torch.uint8, device=dev())
                table = torch.full((B, TOKENS, 192), float('nan'), device=dev())
                f = torch.full((B, 192), float('nan'), device=dev())
                call('rovit_vit_forward_train_tokens', ptr(x), ptr(seq), ptr(src), T, parr, ptr(eng.prep), ptr(ws), ptr(table), ptr(f), B, 2,
                     path, 0, stream_ptr())
                feats.append(f)
            ws = torch.empty(lib.rovit_vit_workspace_bytes(B, 2, 0), dtype=torch.uint8, device=dev())
            table2 = torch.full((B, TOKENS, 192), float('nan'), device=dev())
            f_inf = torch.full((B, 192), float('nan'), device=dev())
            call('rovit_vit_embed', ptr(x), parr, ptr(eng.prep), ptr(table2), B, 2, stream_ptr())
            call('rovit_vit_forward_tokens', ptr(table2), ptr(table2), B, 0, ptr(seq), ptr(src), T, parr, ptr(eng.prep), ptr(ws), ptr(f_inf), B, 2,
                 path, stream_ptr())
            torch.cuda.synchronize()
            assert torch.isfinite(feats[0]).all(), (B, path)
            assert torch.equal(table, table2), (B, path)
            assert torch.equal(feats[0], feats[1]), (B, path)
            assert torch.equal(feats[0], f_inf), (B, path)
            # and through the Function: grad mode (training entry) and no_grad (embed + inference entry)
            eng.mlp_path = path
            keep = _keep(B, k)
            f_fn = pd.forward_kept(m, x, keep)
            with torch.no_grad():
                f_ng = pd.forward_kept(m, x, torch.from_numpy(keep).to(dev()))
            assert f_fn.requires_grad and not f_ng.requires_grad
            assert torch.equal(f_fn.detach(), feats[0]) and torch.equal(f_ng, feats[0]), (B, path)
            eng.mlp_path = None
    with pytest.raises(native.RovitHipError):
        call('rovit_vit_forward_train_tokens', ptr(x), ptr(seq), ptr(src), 1, parr, ptr(eng.prep), ptr(ws), ptr(table), ptr(f), B, 2, path, 0,
             stream_ptr())


# ---- backward against fp64 ------------------------------------------------------------------------------------------------------------

_ORACLE = {}


def _fp64_grads(depth, B, keep):
    """fp64 autograd: vit_embed -> gather -> vit_block_forward per block -> final norm; loss (features . w).sum().  keep None: all rows."""
    key = (depth, B, None if keep is None else keep.tobytes())
    if key in _ORACLE:
        return _ORACLE[key]
    sd = {n: v.double().requires_grad_() for n, v in _sd(depth).items()}
    t = ref_cpu.vit_embed(_images(B).double(), sd)
    if keep is not None:
        idx = torch.cat([torch.zeros(B, 1, dtype=torch.long), 1 + torch.from_numpy(keep).long()], dim=1)
        t = torch.gather(t, 1, idx[:, :, None].expand(-1, -1, 192))
    for i in range(depth):
        t = ref_cpu.vit_block_forward(t, sd, i)
    feats = F.layer_norm(t[:, 0], (192,), sd['norm.weight'], sd['norm.bias'], 1e-6)
    (feats * _w(B).double()).sum().backward()
    _ORACLE[key] = {n: v.grad.detach() for n, v in sd.items()}
    return _ORACLE[key]


def _rel(got, ref):
    return {n: float((got[n].double().cpu() - ref[n]).norm() / ref[n].norm()) for n in ref}


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('k', [1, 15, 16, 31, 32, 100])
def test_backward_against_fp64_with_the_dense_path_as_yardstick(k, B):
    from rovit_hip import patch_dropout as pd
    depth, T = 2, 1 + k
    keep = _keep(B, k)
    ref_t, ref_d = _fp64_grads(depth, B, keep), _fp64_grads(depth, B, None)
    m = _vit(depth)
    x = _images(B).to(dev())
    factor = 2.0 * math.sqrt(TOKENS / T)
    out = os.environ.get('ROVIT_PATCH_DROPOUT_ERROR_OUT')
    failures = []
    for path in _paths():
        m.engine.mlp_path = path
        _, g_d = _grads_of(m, lambda: m(x))
        _, g_t = _grads_of(m, lambda: pd.forward_kept(m, x, keep))
        rel_d, rel_t = _rel(g_d, ref_d), _rel(g_t, ref_t)
        for n in rel_t:
            bound = factor * rel_d[n]
            # (norm.bias at B = 1: the gradient is w itself, exact on both paths -- 0 <= 0 holds, and the ratio is recorded as 0)
            ratio = rel_t[n] / bound if bound > 0 else (0.0 if rel_t[n] == 0 else float('inf'))
            print(f'k={k} B={B} path={path} {n}: rel_T={rel_t[n]:.3e} rel_dense={rel_d[n]:.3e} bound={bound:.3e}')
            if out:
                with open(out, 'a') as fh:
                    fh.write(json.dumps({'k': k, 'tokens': T, 'batch': B, 'mlp_path': path, 'param': n, 'rel_tokens': rel_t[n],
                                         'rel_dense': rel_d[n], 'bound': bound, 'ratio': ratio}) + '\n')
            if not (math.isfinite(rel_t[n]) and rel_t[n] <= bound):
                failures.append((path, n, rel_t[n], rel_d[n], bound))
    assert not failures, failures


# ---- exact zeros ----------------------------------------------------------------------------------------------------------------------

def test_dropped_patches_get_exactly_zero_position_gradient():
    from rovit_hip import patch_dropout as pd
    B, k = 3, 31
    row = _keep(1, k)[0]
    keep = np.tile(row, (B, 1))                     # the same subset in every sample
    m = _vit(2)
    x = _images(B).to(dev())
    for path in _paths():
        m.engine.mlp_path = path
        _, g = _grads_of(m, lambda: pd.forward_kept(m, x, keep))
        gp = g['pos_embed'][0].cpu()
        kept = np.zeros(TOKENS, bool)
        kept[0] = True
        kept[1 + row] = True
        assert torch.isfinite(gp).all()
        assert float(gp[torch.from_numpy(~kept)].abs().max()) == 0.0
        assert bool((gp[torch.from_numpy(kept)].abs().amax(1) > 0).all())
        assert float(g['cls_token'].abs().max()) > 0 and float(g['patch_embed.proj.weight'].abs().max()) > 0


def test_token_forward_leaves_no_dense_workspace_for_the_tap_readers():
    """A pending dense training forward sets engine.last_ws; a token forward after it clears it, so rovit_hip.taps.norm1_output refuses
    instead of reading 197-token rows of a workspace that no longer belongs to the latest forward."""
    from rovit_hip import patch_dropout as pd, taps
    from rovit_hip.native import RovitHipError
    m = _vit(2)
    x = _images(3).to(dev())
    dense = m(x)                                     # grad-mode dense forward, backward pending
    assert m.engine.last_ws is not None and tuple(taps.norm1_output(m, 0).shape) == (3, TOKENS, 192)
    f = pd.forward_kept(m, x, _keep(3, 31))
    assert m.engine.last_ws is None
    with pytest.raises(RovitHipError, match='no training-mode forward is pending'):
        taps.norm1_output(m, 0)
    (dense.sum() + f.sum()).backward()               # both graphs still run their backward
    torch.cuda.synchronize()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())


# ---- module semantics, depth 12, B = 4 --------------------------------------------------------------------------------------------------

def _stage_for_epoch(epoch):
    return 4


def _one_step(model, x, y, **train_fields):
    from training import JointLoss, Trainer, build_optimizer, build_scheduler
    cfg = SimpleNamespace(
        train=SimpleNamespace(learning_rate=1e-3, weight_decay=1e-4, epochs=1, early_stop_patience=5, **train_fields),
        flags=SimpleNamespace(use_cutmix=False, use_mixup=False, cutmix_alpha=1.0, mixup_alpha=0.2, mixed_precision=True, gradient_clip=1.0,
                              freeze_backbone_epochs=0, curriculum=True),
        paths=SimpleNamespace(checkpoints_dir='.'), get_stage_for_epoch=_stage_for_epoch)
    opt = build_optimizer(model, cfg)
    t = Trainer(model, [(x, y, y.clone())], [], opt, build_scheduler(opt, cfg), JointLoss(), cfg, dev())
    torch.manual_seed(1234)                         # the heads' dropout masks
    metrics = t.train_epoch(1)
    torch.cuda.synchronize()
    return metrics


def test_module_semantics_and_trainer_step():
    from models.rovit_kan import RoViTKAN
    from rovit_hip import RovitHipError
    from rovit_hip.parallel import GradSync
    torch.manual_seed(0)
    base = RoViTKAN(pretrained=False)
    base.load_state_dict(ref_cpu.init_rovit_state(seed=3))
    x = torch.randn(4, 3, 224, 224, generator=torch.Generator().manual_seed(4)).to(dev())
    y = torch.tensor([0, 1, 2, 3], device=dev())

    # train() with keep = 0.5: a new subset per call, features (B, 192); eval(): the dense forward's bits
    m = copy.deepcopy(base).to(dev()).set_patch_dropout(0.5, seed=5)
    m.train()
    f1 = m.backbone(x)
    k1 = m.backbone.last_patch_keep.clone()
    f2 = m.backbone(x)
    k2 = m.backbone.last_patch_keep.clone()
    assert tuple(f1.shape) == tuple(f2.shape) == (4, 192) and torch.isfinite(f1).all() and torch.isfinite(f2).all()
    assert tuple(k1.shape) == (4, 98) and not torch.equal(k1, k2) and m.backbone.patch_dropout_step == 2
    assert not torch.equal(f1, f2)
    m.backbone.patch_dropout_step = 0               # the same seed and counter: the same subset, the same bits
    f1b = m.backbone(x)
    assert torch.equal(m.backbone.last_patch_keep, k1) and torch.equal(f1b, f1)
    plain = copy.deepcopy(base).to(dev()).eval()
    m.eval()
    with torch.no_grad():
        a, b = m(x), plain(x)
    assert torch.equal(a['features'], b['features']) and torch.equal(a['cls_logits'], b['cls_logits'])
    assert m.backbone.patch_dropout_step == 1       # eval() drew nothing

    # a frozen backbone: forward only, the heads still train
    m.train()
    m.freeze_backbone()
    out = m(x)
    out['cls_logits'].sum().backward()
    assert all(p.grad is None for p in m.backbone.parameters()) and m.classification_head.fc1.weight.grad is not None
    m.unfreeze_backbone()

    # the three refusals
    h = m.backbone.model.blocks[11].norm1.register_forward_hook(lambda *a: None)
    with pytest.raises(RovitHipError, match='hook'):
        m(x)
    h.remove()
    with pytest.raises(RovitHipError, match='images require grad'):
        m(x.clone().requires_grad_())
    dp = copy.deepcopy(base).to(dev()).set_patch_dropout(0.5)
    gs = GradSync(dp, buckets=2)                    # one process, no process group: inert, so wire what an active one installs
    assert not gs.active
    dp.train()
    assert tuple(dp.backbone(x).shape) == (4, 192)  # the inert wrapper is no reason to refuse
    eng = dp.backbone.model.engine
    eng.backward_ranges, eng.range_hook, eng.pre_backward_hook = gs.ranges, gs._on_range, gs._on_backbone_backward_start
    with pytest.raises(RovitHipError, match='data-parallel'):
        dp(x)

    # one Trainer.train_epoch step: keep = 1.0 is the dense step bit for bit
    never = copy.deepcopy(base)
    _one_step(never, x, y)
    one = copy.deepcopy(base)
    _one_step(one, x, y, patch_keep=1.0)
    for (n, p), (_, q) in zip(never.named_parameters(), one.named_parameters()):
        assert torch.equal(p, q), n
    # keep = 0.5: finite losses, changed parameters, and the same seed and counter reproduce the step bit for bit
    runs = []
    for _ in range(2):
        half = copy.deepcopy(base)
        metrics = _one_step(half, x, y, patch_keep=0.5, patch_seed=21)
        assert all(math.isfinite(v) for v in metrics.values()), metrics
        assert half.backbone.patch_dropout_step == 1 and tuple(half.backbone.last_patch_keep.shape) == (4, 98)
        runs.append(half)
    for (n, p), (_, q), (_, r) in zip(runs[0].named_parameters(), runs[1].named_parameters(), base.named_parameters()):
        assert torch.isfinite(p).all(), n
        assert torch.equal(p, q), n
        assert not torch.equal(p, r.to(p.device)), n
    assert not torch.equal(runs[0].backbone.last_patch_keep, k1)            # another seed, another subset
