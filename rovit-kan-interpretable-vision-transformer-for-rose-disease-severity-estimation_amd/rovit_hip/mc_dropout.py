"""Monte-Carlo dropout over the heads on the GPU (csrc/mc_dropout.hip, rovit_head_mc_fwd): the model's own (epistemic) uncertainty
that the reference's users get by putting the heads' nn.Dropout(0.3) modules (models/heads.py:14,35,87) in training mode after
model.eval() -- the enable_dropout() interface of experiments/baselines.py:48-52 -- and running T forwards.  Here: ONE backbone forward
(DeiT-Tiny has no dropout, so its features are the same in every sample), ONE launch for all T samples of every head and their
per-image statistics, and -- at stage 4 -- the eval head phase for the deterministic kan_severity."""
import ctypes as C

import torch

from . import native
from .native import RovitHipError, call, ptr, stream_ptr

MAX_SAMPLES = 4096          # rovit_head_mc_fwd's limit


def _reserve(dev, batch: int, hid: int):
    """(seed, offset) from the device's default generator, reserving the counters like RoViTKAN._forward_head_phase does: two calls
    draw different masks and torch.manual_seed reproduces both."""
    gen = torch.cuda.default_generators[dev.index]
    n = batch * hid
    off = gen.get_offset()
    gen.set_offset(off + 4 * ((n + 3) // 4))
    return gen.initial_seed(), off


def mc_dropout_predict(model, x: torch.Tensor, num_samples: int = 30, seed=None, return_samples: bool = False, *, offset: int = 0):
    """MC-dropout predictions of a RoViTKAN for every image of the batch.

    ``num_samples`` T in 1..4096.  ``seed``: None -- the device generator's seed, with an offset reserved from it (so successive calls
    differ and torch.manual_seed reproduces them) -- or an int (with ``offset``, default 0): the same result whatever the generator's
    state.  Sample t draws the mask of unit k of image b from Philox4x32-10 with key seed and counter (b * hid + k, t, offset): sample 0
    is the mask a training forward draws with the same seed and offset.  The dropout probability is the heads' own Dropout p (every
    active head must have the same one); the Dropout modules' training flags do not matter here.

    Returns a dict keyed like predict() at the model's curriculum stage -- ``class`` (argmax of the mean probabilities), ``class_probs``
    (mean over the samples of the softmax), ``features``, and from stage 2 ``ordinal_probs`` / ``ordinal_severity``, from stage 3
    ``uncertainty_mu`` / ``uncertainty_std``, at stage 4 ``kan_severity`` (deterministic: KAN has no dropout) -- plus ``class_probs_std``,
    ``predictive_entropy`` H[mean p], ``expected_entropy`` E_t H[p_t], ``mutual_information`` (their difference, >= 0), from stage 2
    ``ordinal_severity_std``, from stage 3 ``epistemic_var`` (variance of mu), ``aleatoric_var`` (mean of exp(log_var)) and
    ``uncertainty_std`` = sqrt(aleatoric_var + epistemic_var).  Variances are over the samples, divided by T.  ``return_samples=True``
    adds ``samples``: {'cls_logits': (T,B,C), 'ordinal_logits': (T,B,C-1), 'mu': (T,B,1), 'log_var': (T,B,1)} of the active heads.

    Runs under no_grad, writes no ``.grad`` and leaves every module's training flag as it found it."""
    if isinstance(num_samples, bool) or not isinstance(num_samples, int) or not 1 <= num_samples <= MAX_SAMPLES:
        raise RovitHipError(f'mc_dropout_predict: num_samples must be an int in 1..{MAX_SAMPLES}, got {num_samples!r}')
    for name, v in (('seed', seed), ('offset', offset)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 64):
            raise RovitHipError(f'mc_dropout_predict: {name} must be None or an int in [0, 2**64), got {v!r}')
    if seed is None and offset:
        raise RovitHipError('mc_dropout_predict: an explicit offset needs an explicit seed')
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise RovitHipError(f'mc_dropout_predict: expects (B,3,H,W) images, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}')
    if not x.is_cuda:
        raise RovitHipError('mc_dropout_predict: the images must be on the GPU (there is no CPU fallback)')
    B = x.shape[0]
    if B < 1:
        raise RovitHipError('mc_dropout_predict: empty batch')
    c, o, u = model.classification_head, model.ordinal_head, model.uncertainty_head
    stage = model.curriculum_stage
    active = (c, o, u)[:3 if stage >= 3 else (2 if stage >= 2 else 1)]
    ps = {float(h.dropout.p) for h in active}
    if len(ps) != 1:
        raise RovitHipError(f'mc_dropout_predict: the active heads have different dropout probabilities {sorted(ps)} (one p per launch)')
    hid, C_ = c.fc1.out_features, c.fc2.out_features
    if not all(h.fc1.out_features == hid for h in active):
        raise RovitHipError('mc_dropout_predict: the heads have different hidden widths')
    T, dev = num_samples, x.device

    flags = [(m, m.training) for m in model.modules()]
    try:
        with torch.no_grad():
            features = model.backbone(x)
            feats = features.detach().float().contiguous()
            if seed is None:
                seed_v, off = _reserve(dev, B, hid)
            else:
                seed_v, off = seed, offset
            params = [t.detach().float().contiguous() for t in model._head_params()]
            f32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
            out = {'class_probs': f32(B, C_), 'class_probs_std': f32(B, C_), 'predictive_entropy': f32(B),
                   'expected_entropy': f32(B), 'mutual_information': f32(B)}
            if stage >= 2:
                out.update(ordinal_probs=f32(B, C_), ordinal_severity=f32(B, 1), ordinal_severity_std=f32(B, 1))
            if stage >= 3:
                out.update(uncertainty_mu=f32(B, 1), epistemic_var=f32(B, 1), aleatoric_var=f32(B, 1), uncertainty_std=f32(B, 1))
            samples = None
            if return_samples:
                samples = {'cls_logits': f32(T, B, C_)}
                if stage >= 2:
                    samples['ordinal_logits'] = f32(T, B, C_ - 1)
                if stage >= 3:
                    samples['mu'], samples['log_var'] = f32(T, B, 1), f32(T, B, 1)
            d = native.HeadMC()
            d.batch, d.embed, d.hid, d.num_classes, d.stage, d.num_samples = B, feats.shape[1], hid, C_, stage, T
            d.drop_p, d.seed, d.offset = ps.pop(), seed_v, off
            d.features = ptr(feats)
            for i, p_ in enumerate(params):
                d.head_params[i] = ptr(p_)
            g = out.get
            d.class_probs, d.class_probs_std = ptr(g('class_probs')), ptr(g('class_probs_std'))
            d.pred_entropy, d.exp_entropy, d.mutual_info = ptr(g('predictive_entropy')), ptr(g('expected_entropy')), ptr(g('mutual_information'))
            d.ord_probs, d.ord_severity, d.ord_severity_std = ptr(g('ordinal_probs')), ptr(g('ordinal_severity')), ptr(g('ordinal_severity_std'))
            d.unc_mu, d.epistemic_var = ptr(g('uncertainty_mu')), ptr(g('epistemic_var'))
            d.aleatoric_var, d.unc_std = ptr(g('aleatoric_var')), ptr(g('uncertainty_std'))
            if samples is not None:
                s = samples.get
                d.s_cls, d.s_ord, d.s_mu, d.s_lv = ptr(s('cls_logits')), ptr(s('ordinal_logits')), ptr(s('mu')), ptr(s('log_var'))
            call('rovit_head_mc_fwd', C.byref(d), stream_ptr())
            pred = {'class': torch.argmax(out['class_probs'], dim=1), **out, 'features': features}
            if stage >= 4:
                # the eval head phase predict() runs (or the per-module KAN where that cannot fuse): the same kan_severity bits
                model.eval()
                if model._head_phase_fusable(features):
                    pred['kan_severity'] = model._forward_head_phase(features, stage)['kan_severity']
                else:
                    pred['kan_severity'] = model.kan_module(features)
            if samples is not None:
                pred['samples'] = samples
            return pred
    finally:
        for m, f in flags:
            m.training = f
