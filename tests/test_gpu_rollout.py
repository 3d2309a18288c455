"""GPU tests of the attention rollout (csrc/rollout.hip, rovit_hip/rollout.py, explainability/attention_maps.py): the fused
rollout against a torch restatement of the reference's ViTAttentionRollout.generate (explainability/attention_maps.py:60-103)
applied to the same probabilities, against the fp32 oracle end to end, determinism, batch consistency and the drop-in class."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref_cpu  # noqa: E402  (checker only)

RAW_RTOL = 1e-5          # raw (B,14,14) rollout vs the restatement on the same probabilities (only summation order differs)
MAP_TOL = 1e-4           # (B,224,224) map, max-abs, same comparison
ORACLE_MAP_TOL = 1.5e-2  # map vs the fp32 oracle's probabilities, max-abs (DESIGN.md tolerance table: measured 5.05e-3)


def dev():
    return torch.device('cuda:0')


def restate(probs, head_fusion='mean'):
    """attention_maps.py:60-103 on a list of (B,3,197,197) probability tensors, for every image of the batch (the reference
    takes item 0): fuse the heads, + I, renormalise the rows, multiply in block order, row 0 without the class token.
    fp64, so the restatement's own rounding stays far below the tolerances.  Returns (raw (B,14,14), map (B,224,224))."""
    B, N = probs[0].shape[0], probs[0].shape[-1]
    eye = torch.eye(N, dtype=torch.float64, device=probs[0].device)
    roll = eye.expand(B, N, N)
    for a in probs:
        a = a.double()
        f = {'mean': lambda t: t.mean(1), 'max': lambda t: t.max(1)[0], 'min': lambda t: t.min(1)[0]}[head_fusion](a)
        f = f + eye
        f = f / f.sum(-1, keepdim=True)
        roll = roll @ f
    raw = roll[:, 0, 1:].reshape(B, 14, 14)
    m = F.interpolate(raw[:, None], size=(224, 224), mode='bilinear', align_corners=False)[:, 0]   # = cv2.resize INTER_LINEAR
    mn = m.flatten(1).min(1)[0][:, None, None]
    mx = m.flatten(1).max(1)[0][:, None, None]
    return raw, (m - mn) / (mx - mn + 1e-8)


def _vit(depth, seed):
    from models.backbone import DeiTTiny
    sd = ref_cpu.init_vit_state(depth, torch.Generator().manual_seed(seed))
    m = DeiTTiny(depth)
    m.load_state_dict(sd)
    return m.to(dev()).eval(), sd


def _full_model(seed):
    from models.rovit_kan import RoViTKAN
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(ref_cpu.init_rovit_state(seed=seed), strict=True)
    return m.to(dev()).eval()


@pytest.mark.parametrize('head_fusion', ['mean', 'max', 'min'])
@pytest.mark.parametrize('depth,B', [(3, 1), (3, 7), (3, 64), (12, 1), (12, 7), (12, 64)])
def test_rollout_matches_restatement_on_the_same_probabilities(head_fusion, depth, B):
    from rovit_hip import taps
    from rovit_hip.rollout import attention_rollout
    m, _ = _vit(depth, seed=100 + depth)
    x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B)).to(dev())
    raw = attention_rollout(m, x, head_fusion, upsample=False)
    amap = attention_rollout(m, x, head_fusion, upsample=True)
    assert raw.shape == (B, 14, 14) and amap.shape == (B, 224, 224)
    assert raw.dtype == torch.float32 and amap.dtype == torch.float32 and raw.is_cuda and amap.is_cuda
    ref_raw, ref_map = restate(taps.attention_probabilities(m, x), head_fusion)
    rel = float(((raw.double() - ref_raw).abs() / ref_raw.abs()).max())
    err = float((amap.double() - ref_map).abs().max())
    print(f'{head_fusion} depth={depth} B={B}: raw max rel {rel:.2e}, map max-abs {err:.2e}')
    assert rel < RAW_RTOL, rel
    assert err < MAP_TOL, err


def test_rollout_against_fp32_oracle_end_to_end():
    from rovit_hip.rollout import attention_rollout
    m, sd = _vit(12, seed=7)
    x = torch.randn(4, 3, 224, 224, generator=torch.Generator().manual_seed(4))
    probs = []
    with torch.no_grad():
        ref_cpu.vit_forward(x, sd, attn_probs=probs)
    ref_raw, ref_map = restate(probs)
    raw = attention_rollout(m, x.to(dev()), upsample=False).cpu()
    amap = attention_rollout(m, x.to(dev())).cpu()
    err = float((amap.double() - ref_map).abs().max())
    rel_raw = float(((raw.double() - ref_raw).abs() / ref_raw.abs()).max())
    corr = [float(np.corrcoef(amap[b].flatten().numpy(), ref_map[b].flatten().numpy())[0, 1]) for b in range(4)]
    print(f'vs fp32 oracle: map max-abs {err:.2e}, raw max rel {rel_raw:.2e}, pearson {min(corr):.6f}')
    assert err < ORACLE_MAP_TOL, err
    assert min(corr) > 0.999, corr
    assert torch.equal(raw.flatten(1).argmax(1), ref_raw.flatten(1).argmax(1))


def test_rollout_is_bit_identical_run_to_run():
    from rovit_hip.rollout import attention_rollout
    m, _ = _vit(12, seed=9)
    x = torch.randn(64, 3, 224, 224, generator=torch.Generator().manual_seed(9)).to(dev())
    for fusion in ('mean', 'max'):
        a = attention_rollout(m, x, fusion, upsample=False)
        b = attention_rollout(m, x, fusion, upsample=False)
        assert torch.equal(a, b), fusion
        assert bool(torch.isfinite(a).all())


def test_rollout_of_an_image_does_not_depend_on_its_batch():
    from rovit_hip.rollout import attention_rollout
    m, _ = _vit(12, seed=11)
    x = torch.randn(37, 3, 224, 224, generator=torch.Generator().manual_seed(37)).to(dev())
    raw = attention_rollout(m, x, upsample=False)
    amap = attention_rollout(m, x)
    for k in (0, 18, 36):
        r1 = attention_rollout(m, x[k:k + 1], upsample=False)[0]
        m1 = attention_rollout(m, x[k:k + 1])[0]
        assert float(((r1 - raw[k]).abs() / raw[k].abs()).max()) < RAW_RTOL, k
        assert float((m1 - amap[k]).abs().max()) < MAP_TOL, k


def test_model_methods_delegate():
    from rovit_hip.rollout import attention_rollout
    m = _full_model(seed=5)
    x = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(dev())
    a = m.attention_rollout(x, 'max')
    b = m.backbone.attention_rollout(x, 'max')
    c = attention_rollout(m.backbone.model, x, 'max')
    assert torch.equal(a, b) and torch.equal(b, c)
    assert m.attention_rollout(x, upsample=False).shape == (3, 14, 14)


def test_drop_in_class():
    from explainability.attention_maps import ViTAttentionRollout
    m = _full_model(seed=6)
    r = ViTAttentionRollout(m)
    assert r.discard_ratio == 0.9
    x = torch.randn(5, 3, 224, 224, generator=torch.Generator().manual_seed(6))
    one = r.generate(x)
    batch = r.generate_batch(x)
    assert isinstance(one, np.ndarray) and one.shape == (224, 224)
    assert batch.shape == (5, 224, 224) and batch.is_cuda
    assert np.array_equal(one, batch[0].cpu().numpy())
    assert np.array_equal(r.generate(x, head_fusion='bogus'), r.generate(x, head_fusion='mean'))
    assert not np.array_equal(r.generate(x, head_fusion='max'), one)
    assert 0.0 <= float(one.min()) and float(one.max()) <= 1.0
    with pytest.raises(NotImplementedError):
        r.visualize(x, np.zeros((224, 224, 3), np.uint8))
