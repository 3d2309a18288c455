"""Joint multi-task loss that seeds the backward of the hot path.

Mirrors /root/reference/training/losses.py JointLoss (:117-181; FocalLoss :7-38, OrdinalBCELoss :41-72,
UncertaintyLoss :75-101, KANRegressionLoss :104-114): same constructor, same call signature, same returned dict.
On CUDA/HIP tensors the whole loss and its gradient are ONE HIP launch (rovit_joint_loss; backward = one scale by
the upstream gradient).  CPU tensors use the plain-tensor-op restatement below (same formulas; used by the CPU unit
tests of the host logic -- the head outputs of the HIP model are always device tensors).

``JointLoss.mixed`` is the CutMix / MixUp form of training/trainer.py:104-111, ``lam * L(labels_a) + (1 - lam) * L(labels_b)``, as ONE
launch (rovit_joint_loss_mixed: only the focal term depends on the class label, so the mix is a second label column of the same pass),
and it can leave the batch's losses and correct-prediction count in a ``rovit_hip.training.TrainRecord`` without a host read.
"""
from typing import Dict, Optional

import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import native
from .native import call, ptr, stream_ptr


def _scaled_grads(ctx, g_total, n_inputs):
    """The backward both loss Functions share: the kernel left d(total)/d(head output) in ctx.grads; chain them with the upstream gradient
    in one rovit_scale_buffers launch.  Returns the gradient tuple of ``n_inputs`` forward inputs (the five head outputs come first)."""
    if ctx.grads is None:
        raise native.RovitHipError('JointLoss: backward called twice on the same graph (the fused kernel scales its '
                                   'gradient buffers in place); call the loss again instead of retain_graph=True')
    if g_total is None:
        return (None,) * n_inputs
    grads, ctx.grads = ctx.grads, None
    live = [g for g in grads if g is not None]
    arr = (ctypes.c_void_p * len(live))(*[g.data_ptr() for g in live])
    cnt = (ctypes.c_int * len(live))(*[g.numel() for g in live])
    scale = g_total.detach().float().contiguous()
    call('rovit_scale_buffers', arr, cnt, len(live), ptr(scale), stream_ptr())
    return tuple(grads) + (None,) * (n_inputs - 5)


class JointLossFn(torch.autograd.Function):
    """inputs: cls, ord|None, mu|None, lv|None, kan|None, class_t, sev_t, alpha|None, (lambda, mu, nu, gamma)
    outputs: total (0-dim, differentiable), components (4,) detached [cls, ord, unc, kan]."""

    @staticmethod
    def forward(ctx, cls, ordl, mu, lv, kan, cls_t, sev_t, alpha, weights):
        f = lambda t: None if t is None else t.detach().float().contiguous()
        cls, ordl, mu, lv, kan = f(cls), f(ordl), f(mu), f(lv), f(kan)
        cls_t = cls_t.long().contiguous()
        # severity is used as float (reference losses.py:89-90,110-111): int64 labels are converted inside the kernel, anything else here
        sev_t = sev_t.detach().reshape(-1)
        sev_i64 = sev_t.dtype == torch.int64
        sev_t = (sev_t if sev_i64 else sev_t.float()).contiguous()
        alpha = f(alpha.to(cls.device)) if alpha is not None else None
        B, C = cls.shape
        out = torch.empty(5, device=cls.device, dtype=torch.float32)
        grads = [torch.empty_like(t) if t is not None else None for t in (cls, ordl, mu, lv, kan)]
        lam, muw, nu, gamma = weights
        call('rovit_joint_loss', ptr(cls), ptr(ordl), ptr(mu), ptr(lv), ptr(kan), ptr(cls_t), ptr(sev_t), int(sev_i64), ptr(alpha),
             ptr(grads[0]), ptr(grads[1]), ptr(grads[2]), ptr(grads[3]), ptr(grads[4]), ptr(out), B, C, lam, muw, nu, gamma,
             stream_ptr())
        ctx.grads = grads
        ctx.set_materialize_grads(False)      # no zeros(4) launch for the (non-differentiable) components' gradient
        comps = out[:4]
        ctx.mark_non_differentiable(comps)
        return out[4], comps

    @staticmethod
    def backward(ctx, g_total, _g_comps):
        return _scaled_grads(ctx, g_total, 9)


class JointLossMixedFn(torch.autograd.Function):
    """JointLossFn with a second label column and an epoch record: inputs cls, ord|None, mu|None, lv|None, kan|None, class_a,
    class_b|None, lam, sev_t, alpha|None, (lambda, mu, nu, gamma), record|None; same outputs.  ``class_b is None`` is bit-identical to
    JointLossFn.  The backward is the same single rovit_scale_buffers call."""

    @staticmethod
    def forward(ctx, cls, ordl, mu, lv, kan, cls_a, cls_b, lam, sev_t, alpha, weights, record):
        f = lambda t: None if t is None else t.detach().float().contiguous()
        cls, ordl, mu, lv, kan = f(cls), f(ordl), f(mu), f(lv), f(kan)
        dev = cls.device
        cls_a = cls_a.detach().reshape(-1).to(dev, non_blocking=True).long().contiguous()
        cls_b = None if cls_b is None else cls_b.detach().reshape(-1).to(dev, non_blocking=True).long().contiguous()
        sev_t = sev_t.detach().reshape(-1).to(dev, non_blocking=True)
        sev_i64 = sev_t.dtype == torch.int64
        sev_t = (sev_t if sev_i64 else sev_t.float()).contiguous()
        alpha = f(alpha.to(dev)) if alpha is not None else None
        B, C = cls.shape
        for name, t in (('labels_a', cls_a), ('labels_b', cls_b), ('severity_targets', sev_t)):
            if t is not None and t.numel() != B:
                raise native.RovitHipError(f'JointLoss.mixed: {name} has {t.numel()} values for a batch of {B}')
        out = torch.empty(5, device=dev, dtype=torch.float32)
        grads = [torch.empty_like(t) if t is not None else None for t in (cls, ordl, mu, lv, kan)]
        d = native.TrainLoss()
        d.batch, d.num_classes, d.severity_is_int64 = B, C, int(sev_i64)
        d.lam = float(lam)
        d.lambda_ord, d.mu_unc, d.nu_kan, d.focal_gamma = weights
        d.cls_logits, d.ordinal_logits, d.mu, d.log_var, d.kan_severity = ptr(cls), ptr(ordl), ptr(mu), ptr(lv), ptr(kan)
        d.class_targets_a, d.class_targets_b, d.severity_targets, d.focal_alpha = ptr(cls_a), ptr(cls_b), ptr(sev_t), ptr(alpha)
        d.d_cls, d.d_ord, d.d_mu, d.d_lv, d.d_kan = (ptr(g) for g in grads)
        d.losses_out = ptr(out)
        if record is not None:
            table, d.row, d.capacity = record._next_row(dev)
            d.table = ptr(table)
        call('rovit_joint_loss_mixed', ctypes.byref(d), stream_ptr())
        if record is not None:
            record._commit(B)
        ctx.grads = grads
        ctx.set_materialize_grads(False)
        comps = out[:4]
        ctx.mark_non_differentiable(comps)
        return out[4], comps

    @staticmethod
    def backward(ctx, g_total, _g_comps):
        return _scaled_grads(ctx, g_total, 12)


class JointLoss(nn.Module):
    def __init__(self, lambda_ord: float = 1.0, mu_unc: float = 0.5, nu_kan: float = 0.5, focal_gamma: float = 2.0,
                 focal_alpha: Optional[torch.Tensor] = None, num_classes: int = 4):
        super().__init__()
        self.lambda_ord, self.mu_unc, self.nu_kan = lambda_ord, mu_unc, nu_kan
        self.focal_gamma, self.num_classes = focal_gamma, num_classes
        self.focal_alpha = focal_alpha

    def forward(self, outputs: Dict[str, torch.Tensor], class_targets: torch.Tensor, severity_targets: torch.Tensor,
                stage: int = 4) -> Dict[str, torch.Tensor]:
        logits = outputs['cls_logits']
        ordl = outputs['ordinal_logits'] if stage >= 2 else None
        mu = outputs['mu'] if stage >= 3 else None
        lv = outputs['log_var'] if stage >= 3 else None
        if mu is None or lv is None:
            mu = lv = None
        kan = outputs['kan_severity'] if stage >= 4 else None
        if logits.is_cuda:
            total, comps = JointLossFn.apply(logits, ordl, mu, lv, kan, class_targets, severity_targets, self.focal_alpha,
                                             (self.lambda_ord, self.mu_unc, self.nu_kan, self.focal_gamma))
            return {'cls_loss': comps[0], 'ord_loss': comps[1], 'unc_loss': comps[2], 'kan_loss': comps[3], 'total_loss': total}
        return self._forward_tensor_ops(logits, ordl, mu, lv, kan, class_targets, severity_targets)

    def mixed(self, outputs: Dict[str, torch.Tensor], labels_a: torch.Tensor, labels_b: Optional[torch.Tensor], lam: float,
              severity_targets: torch.Tensor, stage: int = 4, record=None) -> Dict[str, torch.Tensor]:
        """``lam * self(outputs, labels_a, ...) + (1 - lam) * self(outputs, labels_b, ...)`` entry by entry (training/trainer.py:104-111),
        the same dict as ``forward``.  On device tensors it is one launch; ``labels_b=None`` or ``lam == 1.0`` is the unmixed loss (on
        the device: bit-identical to ``forward``).  ``record``: a ``rovit_hip.training.TrainRecord`` that receives this batch's five
        losses, the number of rows whose argmax equals ``labels_a``, the batch size and a non-finite flag -- on the device by the same
        launch, without a host read.

        One difference from the reference's arithmetic: at ``lam == 1.0`` exactly (CutMix draws it when its box is empty) ``labels_b``
        is not read at all, so an out-of-range label there does not turn the class loss into NaN, where the reference's
        ``0 * NaN`` would.  At every other ``lam``, 0 included, an out-of-range label in either column gives NaN."""
        lam = float(lam)
        if labels_b is None or lam == 1.0:
            labels_b, lam = None, 1.0
        elif not 0.0 <= lam <= 1.0:
            raise native.RovitHipError(f'JointLoss.mixed: lam must be in [0, 1], got {lam}')
        logits = outputs['cls_logits']
        ordl = outputs['ordinal_logits'] if stage >= 2 else None
        mu = outputs['mu'] if stage >= 3 else None
        lv = outputs['log_var'] if stage >= 3 else None
        if mu is None or lv is None:
            mu = lv = None
        kan = outputs['kan_severity'] if stage >= 4 else None
        if logits.is_cuda:
            total, comps = JointLossMixedFn.apply(logits, ordl, mu, lv, kan, labels_a, labels_b, lam, severity_targets, self.focal_alpha,
                                                  (self.lambda_ord, self.mu_unc, self.nu_kan, self.focal_gamma), record)
            return {'cls_loss': comps[0], 'ord_loss': comps[1], 'unc_loss': comps[2], 'kan_loss': comps[3], 'total_loss': total}
        losses = self._forward_tensor_ops(logits, ordl, mu, lv, kan, labels_a, severity_targets)
        if labels_b is not None:
            other = self._forward_tensor_ops(logits, ordl, mu, lv, kan, labels_b, severity_targets)
            losses = {k: lam * losses[k] + (1 - lam) * other[k] for k in losses}
        if record is not None:
            record.update(losses, logits, labels_a)
        return losses

    def _forward_tensor_ops(self, logits, ordl, mu, lv, kan, class_targets, severity_targets):
        logp = F.log_softmax(logits, dim=1)
        lp_t = logp.gather(1, class_targets.unsqueeze(1)).squeeze(1)
        focal = (1.0 - lp_t.exp()) ** self.focal_gamma * (-lp_t)
        if self.focal_alpha is not None:
            focal = self.focal_alpha.to(logits.device)[class_targets] * focal
        losses = {'cls_loss': focal.mean()}
        total = losses['cls_loss']
        zero = torch.zeros((), device=logits.device)
        sev = severity_targets.float().unsqueeze(1) if severity_targets.dim() == 1 else severity_targets.float()
        losses['ord_loss'] = losses['unc_loss'] = losses['kan_loss'] = zero
        if ordl is not None:
            thr = torch.arange(ordl.shape[1], device=ordl.device)
            bt = (sev.reshape(-1, 1) > thr).float()
            losses['ord_loss'] = F.binary_cross_entropy_with_logits(ordl, bt, reduction='none').mean(dim=1).mean()
            total = total + self.lambda_ord * losses['ord_loss']
        if mu is not None:
            losses['unc_loss'] = (0.5 * ((sev - mu) ** 2 * torch.exp(-lv) + lv)).mean()
            total = total + self.mu_unc * losses['unc_loss']
        if kan is not None:
            losses['kan_loss'] = F.mse_loss(kan, sev)
            total = total + self.nu_kan * losses['kan_loss']
        losses['total_loss'] = total
        return losses
