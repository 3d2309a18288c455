"""fp64 restatement of the reference's joint loss and of its CutMix / MixUp mix, the batches and the tolerance check that the CPU and the
GPU tests of the training epoch share.  Nothing here goes through the code under test: the formulas are training/losses.py's, written with
``F.cross_entropy`` and ``F.binary_cross_entropy_with_logits`` in fp64."""
import torch
import torch.nn.functional as F

HEADS = ('cls_logits', 'ordinal_logits', 'mu', 'log_var', 'kan_severity')
LOSSES = ('cls_loss', 'ord_loss', 'unc_loss', 'kan_loss', 'total_loss')
WEIGHTS = (1.0, 0.5, 0.5, 2.0)          # lambda_ord, mu_unc, nu_kan, focal_gamma


def joint_loss_fp64(out, class_t, sev_t, stage, weights=WEIGHTS, alpha=None):
    """training/losses.py:15-38, 48-72, 80-101, 109-114, 139-181 in fp64: ``out`` holds fp64 tensors (requires_grad for gradients)."""
    lam_o, mu_w, nu_w, gamma = weights
    z = out['cls_logits']
    ce = F.cross_entropy(z, class_t, reduction='none')
    pt = torch.softmax(z, dim=1).gather(1, class_t.unsqueeze(1)).squeeze(1)
    focal = (1 - pt) ** gamma * ce
    if alpha is not None:
        focal = alpha.double()[class_t] * focal
    zero = torch.zeros((), dtype=torch.float64)
    l = {'cls_loss': focal.mean(), 'ord_loss': zero, 'unc_loss': zero, 'kan_loss': zero}
    total = l['cls_loss']
    y = sev_t.double().reshape(-1, 1)
    if stage >= 2:
        k = torch.arange(out['ordinal_logits'].shape[1]).reshape(1, -1)
        l['ord_loss'] = F.binary_cross_entropy_with_logits(out['ordinal_logits'], (y > k).double(), reduction='none').mean(dim=1).mean()
        total = total + lam_o * l['ord_loss']
    if stage >= 3:
        l['unc_loss'] = (0.5 * ((y - out['mu']) ** 2 * torch.exp(-out['log_var']) + out['log_var'])).mean()
        total = total + mu_w * l['unc_loss']
    if stage >= 4:
        l['kan_loss'] = ((out['kan_severity'] - y) ** 2).mean()
        total = total + nu_w * l['kan_loss']
    l['total_loss'] = total
    return l


def mixed_fp64(out, ta, tb, lam, sev_t, stage, weights=WEIGHTS, alpha=None):
    """trainer.py:104-111 in fp64 -> (five losses as floats, gradients of the total w.r.t. the five head outputs for an upstream of 1)."""
    o = {k: v.detach().double().requires_grad_(True) for k, v in out.items()}
    a = joint_loss_fp64(o, ta, sev_t, stage, weights, alpha)
    b = joint_loss_fp64(o, tb, sev_t, stage, weights, alpha)
    mix = {k: lam * a[k] + (1 - lam) * b[k] for k in a}
    mix['total_loss'].backward()
    return {k: float(v.detach()) for k, v in mix.items()}, {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in o.items()}


def make_batch(B, seed, device='cpu'):
    g = torch.Generator().manual_seed(seed)
    out = {'cls_logits': torch.randn(B, 4, generator=g) * 2, 'ordinal_logits': torch.randn(B, 3, generator=g) * 2,
           'mu': torch.randn(B, 1, generator=g) * 2, 'log_var': torch.randn(B, 1, generator=g) * 2,
           'kan_severity': 3 * torch.rand(B, 1, generator=g)}
    ta, tb = torch.randint(0, 4, (B,), generator=g), torch.randint(0, 4, (B,), generator=g)
    sev = torch.randint(0, 4, (B,), generator=g)
    alpha = 0.5 + torch.rand(4, generator=g)
    mv = lambda t: t.to(device)
    return {k: mv(v) for k, v in out.items()}, mv(ta), mv(tb), mv(sev), mv(alpha)


def check_against_fp64(got_losses, got_grads, ref_losses, ref_grads, upstream=1.0, tag=()):
    """The project's own tolerances (tests/test_gpu_loss.py): 1e-4 max(1, |v|) on losses, 1e-5 max(1, max |g|) on gradients.
    Returns the largest errors, in units of those bounds."""
    worst_l = worst_g = 0.0
    for k in LOSSES:
        err, bound = abs(float(got_losses[k]) - ref_losses[k]), 1e-4 * max(1.0, abs(ref_losses[k]))
        worst_l = max(worst_l, err / bound)
        assert err < bound, (tag, k, err)
    for k in HEADS:
        ref = upstream * ref_grads[k]
        got = torch.zeros_like(ref) if got_grads[k] is None else got_grads[k].detach().cpu().double()
        err, bound = float((got - ref).abs().max()), 1e-5 * max(1.0, float(ref.abs().max()))
        worst_g = max(worst_g, err / bound)
        assert err < bound, (tag, k, err)
    return worst_l, worst_g
