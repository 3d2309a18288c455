"""Deletion and insertion curves of saliency maps (Petsiuk, Das & Saenko, "RISE", BMVC 2018; the positive / negative perturbation test
of Chefer, Gur & Wolf, CVPR 2021) for a RoViTKAN output, on the GPU.

A map ranks the 196 patches by the sum of its values over each patch.  Step s = 0..steps perturbs k_s = floor(196 s / steps) patches:
deletion the first k_s of the ranking, insertion all but the first k_s; the curve records the target after every step and its area
(trapezoid rule over k_s / 196) scores the map: low for deletion and high for insertion when the map is faithful.

The patch embedding is a 16x16 convolution with stride 16, so every token row of a patch-perturbed image is the clean image's row or the
baseline's.  Each image and its baseline are embedded once (rovit_vit_embed) and every perturbed sequence is gathered from those rows in
front of block 0 (rovit_vit_forward_tokens; csrc/perturb.hip): bit-identical to running the forward on the perturbed pixels, with no
pixel tensor per step.  ``perturbation='drop'`` removes the perturbed tokens from the sequence instead: no baseline square enters the
model and every kept token keeps its own position embedding."""
import numpy as np
import torch

from .input_grad import _Backbone, _check_args, _head_outputs, _target_value
from .native import MLP_AUTO, MLP_FUSED_MIN_ROWS, MLP_ONE_LAUNCH, MLP_TWO_LAUNCH, RovitHipError

NP = 196                     # patches of a 224x224 image in 16x16 patches (14 x 14, p = 14 row + column)
MODES = ('deletion', 'insertion')
PERTURBATIONS = ('replace', 'drop')
_SHAPES = ((14, 14), (196,), (224, 224), (3, 224, 224))


def step_counts(steps: int):
    """k_s = floor(196 s / steps), s = 0..steps: the patches step s perturbs."""
    return [NP * s // steps for s in range(steps + 1)]


def patch_scores(saliency: torch.Tensor) -> torch.Tensor:
    """(B,196) float64: the map summed over each patch's pixels and channels.  saliency: (B,14,14), (B,196), (B,224,224) or
    (B,3,224,224)."""
    s = saliency.detach().double()
    B = s.shape[0]
    if s.dim() == 4:
        s = s.sum(dim=1)
    if s.dim() == 3 and tuple(s.shape[1:]) == (224, 224):
        s = s.view(B, 14, 16, 14, 16).sum(dim=(2, 4))
    return s.reshape(B, NP)


def patch_order(saliency: torch.Tensor) -> torch.Tensor:
    """(B,196) int64: the patches by descending score; ties go to the lower patch index and NaN counts as -inf."""
    s = patch_scores(saliency)
    s = torch.where(torch.isnan(s), torch.full_like(s, float('-inf')), s)
    return torch.sort(-s, dim=1, stable=True).indices


def _ranks(order: torch.Tensor) -> torch.Tensor:
    """rank[b, p] = position of patch p in the order of image b."""
    r = torch.empty_like(order)
    r.scatter_(1, order, torch.arange(NP, device=order.device).expand_as(order))
    return r


def perturbed_mask(rank: torch.Tensor, deletion, k) -> torch.Tensor:
    """(n,196) bool: the patches perturbed at k, deletion (the first k of the ranking) or insertion (all but the first k).  rank: (n,196)
    from _ranks; deletion and k: bools / ints or (n,) tensors."""
    k = torch.as_tensor(k, device=rank.device).view(-1, 1)
    deletion = torch.as_tensor(deletion, device=rank.device).view(-1, 1)
    return torch.where(deletion, rank < k, rank >= k)


def source_rows(perturbed: torch.Tensor, perturbation: str, tokens: int = 197) -> torch.Tensor:
    """(n, tokens) int32: the src rows of rovit_vit_forward_tokens for perturbed masks (n,196).  'replace': row 0 the class token, row
    1 + p = 1 + p (the image's) or -2 - p (row 1 + p of the baseline's).  'drop': the class token and the kept patches in patch order;
    every mask must keep tokens - 1 patches."""
    n = perturbed.shape[0]
    p = torch.arange(NP, device=perturbed.device).expand(n, NP)
    cls = torch.zeros(n, 1, dtype=torch.long, device=perturbed.device)
    if perturbation == 'replace':
        return torch.cat([cls, torch.where(perturbed, -2 - p, 1 + p)], dim=1).int()
    keys = torch.where(perturbed, p + NP, p)
    return torch.cat([cls, 1 + torch.sort(keys, dim=1).values[:, :tokens - 1]], dim=1).int()


def trapezoid_auc(curve: torch.Tensor, fractions: torch.Tensor) -> torch.Tensor:
    """(B,) area under (B, steps+1) curves over the fractions k_s / 196, trapezoid rule."""
    return torch.trapezoid(curve, fractions, dim=1)


def _check(model, x, saliency, target, class_idx, modes, steps, perturbation, baseline, chunk, ragged=False):
    what = 'perturbation_curves'
    if not isinstance(ragged, bool):
        raise RovitHipError(f'{what}: ragged must be a bool, got {ragged!r}')
    if isinstance(steps, bool) or not isinstance(steps, int) or not 1 <= steps <= NP:
        raise RovitHipError(f'{what}: steps must be an int in [1, {NP}], got {steps!r}')
    ms = [modes] if isinstance(modes, str) else list(modes) if isinstance(modes, (list, tuple)) else None
    if not ms or not all(isinstance(m, str) and m in MODES for m in ms) or len(set(ms)) != len(ms):
        raise RovitHipError(f'{what}: modes must be a non-empty list / tuple out of {list(MODES)} without repeats, got {modes!r}')
    if perturbation not in PERTURBATIONS:
        raise RovitHipError(f'{what}: perturbation must be one of {list(PERTURBATIONS)}, got {perturbation!r}')
    if perturbation == 'drop' and baseline is not None:
        raise RovitHipError(f"{what}: perturbation='drop' removes patches from the sequence and takes no baseline")
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise RovitHipError(f'{what}: expects (B,3,224,224) images, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}')
    maps = saliency if isinstance(saliency, dict) else {None: saliency}
    if not maps or (isinstance(saliency, dict) and not all(isinstance(k, str) for k in maps)):
        raise RovitHipError(f'{what}: a dict of saliency maps must be non-empty with str keys')
    for name, s in maps.items():
        tag = f'saliency {name!r}' if name is not None else 'saliency'
        if not isinstance(s, torch.Tensor) or not s.dtype.is_floating_point:
            raise RovitHipError(f'{what}: {tag} must be a floating-point tensor, got '
                                f'{s.dtype if isinstance(s, torch.Tensor) else type(s).__name__}')
        if s.dim() < 2 or tuple(s.shape[1:]) not in _SHAPES:
            raise RovitHipError(f'{what}: {tag} must be (B,14,14), (B,196), (B,224,224) or (B,3,224,224), got {tuple(s.shape)}')
        if s.shape[0] != x.shape[0]:
            raise RovitHipError(f'{what}: {tag} holds {s.shape[0]} maps for {x.shape[0]} images')
    # the images, target, class_idx, baseline (broadcast to x, x's device), chunk and head shapes as input_gradients checks them
    targets = _check_args(model, x, target, class_idx, 1, baseline, chunk, what)
    return ms, maps, targets


def perturbation_curves(model, x: torch.Tensor, saliency, target='class', class_idx=None, modes=('deletion', 'insertion'),
                        steps: int = 28, perturbation: str = 'replace', baseline=None, chunk: int = 256, ragged: bool = False):
    """Deletion / insertion curves of saliency maps for one RoViTKAN output, every image of the batch.

    ``saliency``: (B,14,14), (B,196), (B,224,224) or (B,3,224,224); a patch's score is the sum of the map over its pixels and channels
    (pass ``g.abs()`` to rank by gradient magnitude); patches in descending score, ties to the lower index, NaN as -inf.  A dict of
    name -> map returns a dict of results from one call, sharing the image tables and the endpoints.
    ``target``: ``'class'`` -- the softmax probability of c_b (``class_idx``: an int or a (B,) integer tensor; None: each image's
    argmax at the unperturbed image) -- or ``'ordinal_severity'``, ``'mu'``, ``'log_var'``, ``'kan_severity'`` as input_gradients.
    ``steps`` (1..196): step s perturbs k_s = floor(196 s / steps) patches, s = 0..steps.
    ``perturbation='replace'``: a perturbed patch is ``baseline``'s (any tensor broadcastable to x; default zeros, the dataset's mean
    colour in the normalised input).  ``'drop'``: its token leaves the sequence (the class token stays, kept tokens in patch order).
    Returns ``{'fractions': (steps+1,), mode: (B, steps+1), mode + '_auc': (B,), 'class_idx': (B,) for 'class'}``, fp32 on x's device.

    The unperturbed and the fully perturbed sequence of each image are computed once for every map and mode, so all curves of an image
    start and end on identical values.  Sequences of equal length are packed into backbone calls of ``chunk``; the MLP path is the
    engine's override or is chosen from ``chunk`` x tokens, never from a call's size, so an image's values do not depend on the others.
    ``ragged=True`` with ``'drop'``: the sequences of ALL lengths are packed, longest first, into calls of ``chunk`` x 197 rows
    (rovit_hip.ragged, rovit_vit_forward_ragged) -- a handful of backbone calls instead of one and more per length; the MLP path is then
    the engine's override or chosen from ``chunk`` x 197 alone.  A short sequence may so take the other MLP path than with
    ``ragged=False`` (the two paths agree to bf16 rounding, not bit for bit), which is why the default stays False.  With
    ``'replace'`` every sequence has 197 tokens and the flag changes nothing.
    Eval semantics, as input_gradients: the bf16 engine whatever ``precision`` says, no dropout, no ``.grad`` written, flags untouched,
    workspaces from the engine's pool.  Every bad argument is refused (RovitHipError) before anything is launched."""
    from .functions import VitEngine
    ms, maps, targets = _check(model, x, saliency, target, class_idx, modes, steps, perturbation, baseline, chunk, ragged)
    dev = x.device
    B = x.shape[0]
    ks = step_counts(steps)
    names = list(maps)
    with torch.no_grad():
        x32 = x.detach().float().contiguous()
        ranks = torch.stack([_ranks(patch_order(maps[n].to(dev))) for n in names])          # (maps, B, 196)
        bb = _Backbone(model, dev)
        # the token tables: every image once, its baseline once (one row set when the baseline is one image)
        img_t = torch.empty(B, 197, 192, device=dev, dtype=torch.float32)
        for b0 in range(0, B, chunk):
            bb.embed(x32[b0:b0 + chunk], img_t[b0:b0 + chunk])
        base_shared = 0
        base_t = img_t                       # 'drop' reads no baseline row
        if perturbation == 'replace':
            xb = torch.zeros(1, 3, 224, 224, device=dev) if baseline is None else baseline.detach().float()
            base_shared = int(xb.dim() < 4 or xb.shape[0] == 1)
            xb = xb.expand(1 if base_shared else B, 3, 224, 224).contiguous()
            base_t = torch.empty(xb.shape[0], 197, 192, device=dev, dtype=torch.float32)
            for b0 in range(0, xb.shape[0], chunk):
                bb.embed(xb[b0:b0 + chunk], base_t[b0:b0 + chunk])
        # combos (map, deletion?, k): one sequence per image each; the endpoints first, shared by every map and mode
        combos = [(0, True, 0), (0, True, NP)]
        for m in range(len(names)):
            for mode in ms:
                combos += [(m, mode == 'deletion', ks[s]) for s in range(1, steps)]
        tokens_of = (lambda c: 197) if perturbation == 'replace' else (lambda c: 197 - c[2] if c[1] else 1 + c[2])
        groups = {}
        for ci, c in enumerate(combos):
            groups.setdefault(tokens_of(c), []).append(ci)
        override = bb.eng.mlp_path if bb.eng.mlp_path is not None else VitEngine.default_mlp_path
        C_ = model.classification_head.fc2.out_features
        raw = torch.empty(len(combos), B, C_ if target == 'class' else 1, device=dev, dtype=torch.float32)
        if ragged and perturbation == 'drop':
            from . import ragged as rg
            max_rows = chunk * 197
            mlp = override if override != MLP_AUTO else (MLP_ONE_LAUNCH if max_rows >= MLP_FUSED_MIN_ROWS else MLP_TWO_LAUNCH)
            lengths = np.repeat(np.array([tokens_of(c) for c in combos], dtype=np.int64), B)      # sequences combo-major, images inside
            calls, _ = rg.ragged_layout(lengths, max_rows)
            c_map = torch.tensor([c[0] for c in combos], device=dev)
            c_del = torch.tensor([c[1] for c in combos], device=dev)
            c_k = torch.tensor([c[2] for c in combos], device=dev)
            ws = rg.take_ws(bb.eng, max_rows, dev)
            for seq, off in calls:
                j = torch.from_numpy(seq).to(dev)
                ci, b = j // B, j % B
                pert = perturbed_mask(ranks[c_map[ci], b], c_del[ci], c_k[ci])
                full = source_rows(pert, 'drop', 197)                      # a sequence's rows are the first `length` of its 197
                off_d, seq_of_row, pos = rg.packed_rows(off, dev)
                feats = bb.forward_ragged(img_t, base_t, 0, b.int(), full[seq_of_row, pos].contiguous(), off_d, off, ws, mlp)
                outs = _head_outputs(model, feats)
                v = outs[0] if target == 'class' else _target_value(target, outs, None).unsqueeze(1)
                raw[ci, b] = v.float()
            bb.eng.give_ws(max_rows, 'ragged', ws)
        else:
            cap = min(chunk, max(len(g) for g in groups.values()) * B)
            ws = bb.eng.take_ws(cap, False, dev)
            for tokens, cis in groups.items():
                mlp = override if override != MLP_AUTO else (MLP_ONE_LAUNCH if chunk * tokens >= MLP_FUSED_MIN_ROWS else MLP_TWO_LAUNCH)
                c_map = torch.tensor([combos[c][0] for c in cis], device=dev)
                c_del = torch.tensor([combos[c][1] for c in cis], device=dev)
                c_k = torch.tensor([combos[c][2] for c in cis], device=dev)
                c_row = torch.tensor(cis, device=dev)
                total = len(cis) * B
                for j0 in range(0, total, chunk):
                    j = torch.arange(j0, min(total, j0 + chunk), device=dev)
                    ci, b = j // B, j % B                                  # sequences combo-major, images inside
                    pert = perturbed_mask(ranks[c_map[ci], b], c_del[ci], c_k[ci])
                    src = source_rows(pert, perturbation, tokens)
                    feats = bb.forward_tokens(img_t, base_t, base_shared, b.int(), src, ws, mlp)
                    outs = _head_outputs(model, feats)
                    v = outs[0] if target == 'class' else _target_value(target, outs, None).unsqueeze(1)
                    raw[c_row[ci], b] = v.float()
            bb.eng.give_ws(cap, False, ws)
        if target == 'class':
            cls = targets.long() if targets is not None else raw[0].argmax(dim=1)
            vals = torch.softmax(raw, dim=2).gather(2, cls.view(1, B, 1).expand(len(combos), B, 1)).squeeze(2)
        else:
            vals = raw.squeeze(2)
        fractions = torch.tensor([k / NP for k in ks], device=dev, dtype=torch.float32)
        results, ci = {}, 2
        for n in names:
            r = {'fractions': fractions}
            for mode in ms:
                inner = vals[ci:ci + steps - 1].t()
                ci += steps - 1
                clean, full = vals[0].unsqueeze(1), vals[1].unsqueeze(1)
                curve = torch.cat([clean, inner, full] if mode == 'deletion' else [full, inner, clean], dim=1).contiguous()
                r[mode] = curve
                r[mode + '_auc'] = trapezoid_auc(curve, fractions)
            if target == 'class':
                r['class_idx'] = cls
            results[n] = r
    return results if isinstance(saliency, dict) else results[None]


def perturbation_reference(f, x: torch.Tensor, saliency: torch.Tensor, mode: str, steps: int, baseline: torch.Tensor) -> torch.Tensor:
    """(B, steps+1) curve of one mode by the explicit pixel recipe of perturbation='replace': at every step the perturbed images are
    built -- each perturbed 16x16 patch, all three channels, taken from ``baseline`` (broadcast to x) -- and passed to ``f``:
    (N,3,224,224) -> (N,).  The ranking and k_s are those of perturbation_curves.  The oracle the tests run, in the pattern of
    input_grad.ig_reference."""
    B = x.shape[0]
    rank = _ranks(patch_order(saliency).to(x.device))
    xb = baseline.to(x.dtype).expand_as(x)
    out = []
    for k in step_counts(steps):
        m = perturbed_mask(rank, mode == 'deletion', k).view(B, 1, 14, 1, 14, 1).expand(B, 3, 14, 16, 14, 16).reshape(B, 3, 224, 224)
        out.append(f(torch.where(m, xb, x)))
    return torch.stack(out, dim=1)
