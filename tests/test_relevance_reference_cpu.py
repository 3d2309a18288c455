"""CPU tests of the fp64 reference of gradient-weighted attention relevance (rovit_hip/relevance.py, Chefer, Gur & Wolf 2021): a
hand-computed two-block example, the forward-order matrix recursion against the backward-order vector recursion, and the reference on
the oracle ViT -- including the fact a backward-order implementation relies on: the last block's attention gradient lives on the class
token's row alone."""
import pytest
import torch

from oracle import ref_cpu  # (checker only)


def _vector_recursion(abar):
    """Row 0 of (I + A_L) ... (I + A_1) as u = e_0, u <- u + u A_l for l = L..1 (the order of a backward pass)."""
    B, N, _ = abar[0].shape
    u = torch.zeros(B, N, dtype=abar[0].dtype)
    u[:, 0] = 1
    for a in reversed(abar):
        u = u + (u.unsqueeze(1) @ a).squeeze(1)
    return u


def test_relevance_reference_hand_computed_two_blocks_three_tokens():
    """value = sum(C1 * P1) + sum(C2 * P2), so G_l = C_l; two heads, three tokens, one image.

    block 1: relu(C1 * P1) = [[1,1,0],[0,1,0],[0,0,1]] and [[0,1,0],[0,1,2],[1,0,0]] -> A1 = [[.5,1,0],[0,1,1],[.5,0,.5]]
    block 2: relu(C2 * P2) = [[1,0,1],[1,0,0],[0,1,0]] and [[0,1,1],[1,0,0],[0,0,0]] -> A2 = [[.5,.5,1],[1,0,0],[0,.5,0]]
    R1 = I + A1 = [[1.5,1,0],[0,2,1],[.5,0,1.5]];  row 0 of R2 = (I + A2)[0] R1 = 1.5 R1[0] + .5 R1[1] + R1[2] = [2.75, 2.5, 2]"""
    from rovit_hip.relevance import relevance_reference
    f64 = dict(dtype=torch.float64)
    P1 = torch.tensor([[[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.0, 0.0, 1.0]],
                       [[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5]]], **f64)[None].requires_grad_(True)
    C1 = torch.tensor([[[2.0, 4.0, -4.0], [0.0, 2.0, 0.0], [1.0, 1.0, 1.0]],
                       [[-2.0, 2.0, 3.0], [1.0, 2.0, 4.0], [2.0, 5.0, -2.0]]], **f64)[None]
    P2 = torch.tensor([[[0.25, 0.5, 0.25], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]],
                       [[0.0, 0.5, 0.5], [0.5, 0.5, 0.0], [0.0, 0.0, 1.0]]], **f64)[None].requires_grad_(True)
    C2 = torch.tensor([[[4.0, -2.0, 4.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]],
                       [[1.0, 2.0, 2.0], [2.0, -2.0, 0.0], [0.0, 0.0, -1.0]]], **f64)[None]
    value = (C1 * P1).sum((1, 2, 3)) + (C2 * P2).sum((1, 2, 3))
    got = relevance_reference([P1, P2], value)
    assert got.shape == (1, 3) and got.dtype == torch.float64
    assert torch.equal(got, torch.tensor([[2.75, 2.5, 2.0]], **f64))
    # the order of the blocks matters: swapped, row 0 of (I + A1)(I + A2) = 1.5 (I + A2)[0] + (I + A2)[1] = [3.25, 1.75, 1.5]
    value_swapped = (C2 * P2).sum((1, 2, 3)) + (C1 * P1).sum((1, 2, 3))
    assert torch.equal(relevance_reference([P2, P1], value_swapped), torch.tensor([[3.25, 1.75, 1.5]], **f64))


@pytest.mark.parametrize('B,N,L', [(1, 3, 1), (3, 17, 4), (2, 197, 12)])
def test_forward_matrix_recursion_equals_backward_vector_recursion(B, N, L):
    """relevance_reference's forward-order matrix recursion against the backward-order vector recursion the GPU path uses, on random
    fp64 A_l >= 0: value = sum(A_l * P_l) over one head with P_l = 1 gives G_l = A_l and relu(G_l * P_l) = A_l."""
    from rovit_hip.relevance import relevance_reference
    g = torch.Generator().manual_seed(100 * L + N)
    abar = [torch.rand(B, N, N, dtype=torch.float64, generator=g) * (2.0 / N) for _ in range(L)]
    probs = [torch.ones(B, 1, N, N, dtype=torch.float64, requires_grad=True) for _ in range(L)]
    value = sum((a[:, None] * p).sum((1, 2, 3)) for a, p in zip(abar, probs))
    assert torch.allclose(relevance_reference(probs, value), _vector_recursion(abar), rtol=1e-12, atol=0)


def test_relevance_reference_against_the_vector_recursion_on_random_probabilities():
    """value linear in the probabilities (G_l = C_l, of both signs): the reference equals the backward-order vector recursion on
    A_l = mean_h relu(C_l * P_l), image by image."""
    from rovit_hip.relevance import relevance_reference
    g = torch.Generator().manual_seed(7)
    B, H, N, L = 3, 3, 11, 5
    probs = [torch.softmax(torch.randn(B, H, N, N, dtype=torch.float64, generator=g), -1).requires_grad_(True) for _ in range(L)]
    coef = [torch.randn(B, H, N, N, dtype=torch.float64, generator=g) for _ in range(L)]
    value = sum((c * p).sum((1, 2, 3)) for c, p in zip(coef, probs))
    got = relevance_reference(probs, value)
    abar = [(c * p.detach()).clamp(min=0).mean(1) for c, p in zip(coef, probs)]
    assert torch.allclose(got, _vector_recursion(abar), rtol=1e-12, atol=0)
    # the graph is kept, so a second target shares the forward; relevance is not linear in the seed: 2y doubles every A_l, not R_L - I
    got2 = relevance_reference(probs, 2 * value)
    assert torch.allclose(got2, _vector_recursion([2 * a for a in abar]), rtol=1e-12, atol=0)
    assert not torch.allclose(got2 - got, got - torch.eye(N, dtype=torch.float64)[0], rtol=1e-3, atol=0)


def _oracle_relevance(x, sd64, cls):
    probs = []
    x = x.detach().requires_grad_(True)            # (the parameters are plain tensors: the images put the forward in a graph)
    feats = ref_cpu.vit_forward(x, sd64, prefix='backbone.model.', attn_probs=probs)
    logits = ref_cpu.heads_forward(feats, sd64, 4)['cls_logits']
    value = logits.gather(1, cls[:, None])[:, 0]
    return probs, value


def test_relevance_reference_on_the_oracle_vit():
    """Depth-2 oracle ViT in fp64, one class logit per image: the last block's gradient with respect to its probabilities is zero on
    every query row but the class token's (only token 0 leaves the last block), the reference equals the backward-order vector
    recursion on the autograd gradients, and an image's relevance does not depend on the other images of the batch."""
    from rovit_hip.relevance import relevance_reference
    sd = ref_cpu.init_rovit_state(depth=2, seed=3)
    sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
    x = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    cls = torch.tensor([1, 0, 3])
    probs, value = _oracle_relevance(x, sd64, cls)
    assert len(probs) == 2 and probs[0].shape == (3, 3, 197, 197)
    rel = relevance_reference(probs, value)
    assert rel.shape == (3, 197) and torch.isfinite(rel).all()
    grads = torch.autograd.grad(value.sum(), probs)
    assert torch.count_nonzero(grads[-1][:, :, 1:, :]) == 0 and torch.count_nonzero(grads[-1][:, :, 0, :]) > 0
    assert torch.count_nonzero(grads[0][:, :, 1:, :]) > 0
    want = _vector_recursion([(G * P.detach()).clamp(min=0).mean(1) for P, G in zip(probs, grads)])
    assert torch.allclose(rel, want, rtol=1e-12, atol=1e-15)
    # relevance rows: row 0 of (I + A_2)(I + A_1) with A >= 0, so every entry is >= the identity's
    assert bool((rel >= torch.eye(197, dtype=torch.float64)[0]).all()) and bool((rel[:, 1:] > 0).any())
    probs1, value1 = _oracle_relevance(x[1:2], sd64, cls[1:2])
    assert torch.allclose(relevance_reference(probs1, value1), rel[1:2], rtol=1e-10, atol=1e-14)
