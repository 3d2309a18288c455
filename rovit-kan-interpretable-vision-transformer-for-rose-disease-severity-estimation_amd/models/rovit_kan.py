"""RoViT-KAN on the HIP path.  Mirrors /root/reference/models/rovit_kan.py (:9-181): constructor (config object or
scalars, plus the ``embed_dim=`` keyword the reference's own callers use: scripts/train.py:88-97,
evaluation/evaluator.py:233-242), curriculum-stage gate, 6-key output dict, predict/freeze/count helpers."""
from typing import Dict

import torch
import torch.nn as nn

from rovit_hip.functions import ACT_RELU, ACT_SIGMOID3, HeadPhaseFn, HeadsFn

from .backbone import DeiTTinyBackbone
from .heads import ClassificationHead, OrdinalHead, UncertaintyHead, dropout_active, dropout_mask
from .kan import KANSeverityModule


class RoViTKAN(nn.Module):
    def __init__(self, config_or_embed_dim=None, hidden_dim: int = 128, num_classes: int = 4, kan_layers: list = None,
                 kan_num_knots: int = 5, kan_degree: int = 3, dropout: float = 0.3, pretrained: bool = True,
                 embed_dim: int = None):
        super().__init__()
        if hasattr(config_or_embed_dim, 'model'):
            cfg = config_or_embed_dim
            embed_dim = cfg.model.embed_dim
            hidden_dim, num_classes = cfg.model.hidden_dim, cfg.data.num_classes
            kan_layers, kan_num_knots, kan_degree = cfg.model.kan_layers, cfg.model.kan_num_knots, cfg.model.kan_degree
            dropout, pretrained = cfg.model.dropout, cfg.model.pretrained
        elif config_or_embed_dim is not None:
            embed_dim = config_or_embed_dim
        self.backbone = DeiTTinyBackbone(pretrained=pretrained, freeze=False)
        if embed_dim is None:
            embed_dim = self.backbone.embed_dim
        if kan_layers is None:
            kan_layers = [embed_dim, 64, 16, 1]
        self.classification_head = ClassificationHead(embed_dim, hidden_dim, num_classes, dropout)
        self.ordinal_head = OrdinalHead(embed_dim, hidden_dim, num_classes, dropout)
        self.uncertainty_head = UncertaintyHead(embed_dim, hidden_dim, dropout)
        self.kan_module = KANSeverityModule(layers=kan_layers, num_knots=kan_num_knots, degree=kan_degree)
        self.kan_module.__dict__['_owner'] = self          # not a submodule link: a regrid clears this model's _head_grad_views through it
        self._curriculum_stage = 4

    @property
    def curriculum_stage(self) -> int:
        return self._curriculum_stage

    @curriculum_stage.setter
    def curriculum_stage(self, stage: int):
        assert 1 <= stage <= 4, "Stage must be between 1 and 4"
        self._curriculum_stage = stage

    def _head_params(self):
        c, o, u = self.classification_head, self.ordinal_head, self.uncertainty_head
        return [c.fc1.weight, c.fc1.bias, c.fc2.weight, c.fc2.bias, o.fc1.weight, o.fc1.bias, o.fc2.weight, o.fc2.bias,
                u.fc1.weight, u.fc1.bias, u.fc_mu.weight, u.fc_mu.bias, u.fc_logvar.weight, u.fc_logvar.bias]

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        stage = self._curriculum_stage
        if x.shape[0] == 0:
            return self._empty_outputs(x, stage)
        features = self.backbone(x)
        if self._head_phase_fusable(features):
            return self._forward_head_phase(features, stage)
        B, hid = features.shape[0], self.classification_head.fc1.out_features
        masks = None
        heads = ((self.classification_head, 1), (self.ordinal_head, 2), (self.uncertainty_head, 3))
        live = [stage >= need and dropout_active(h.dropout) for h, need in heads]      # each head's own Dropout flag
        if any(live):
            ps = {h.dropout.p for (h, _), a in zip(heads, live) if a}
            if len(ps) == 1:                      # one random draw for all active heads (3 launches instead of 9-12)
                keep = 1.0 - ps.pop()
                m = torch.empty(sum(live), B, hid, device=features.device).bernoulli_(keep).mul_(1.0 / keep)
                it = iter(m.unbind(0))
                masks = [next(it) if a else None for a in live]
            elif ps:
                masks = [dropout_mask(h.dropout, True, (B, hid), features.device) if a else None for (h, _), a in zip(heads, live)]
        cls_logits, ordinal_logits, mu, log_var = HeadsFn.apply(features, stage, masks, *self._head_params())
        return {
            'cls_logits': cls_logits,
            'features': features,
            'ordinal_logits': ordinal_logits if stage >= 2 else None,
            'mu': mu if stage >= 3 else None,
            'log_var': log_var if stage >= 3 else None,
            'kan_severity': self.kan_module(features) if stage >= 4 else None,
        }

    # ---- the head phase as one forward launch and a two-launch backward (csrc/head_phase.hip) ----------------------------
    head_phase_max_batch = 1024        # one workgroup per sample: beyond this the per-module kernels (sample tiles, matrix cores) win

    def _head_phase_fusable(self, features: torch.Tensor) -> bool:
        """Shapes the fused kernels cover, and nothing a caller could observe differently: a forward / backward hook on any
        head or KAN sub-module would not fire from inside the fused launch, so such a model takes the per-module path."""
        if not features.is_cuda or features.dim() != 2 or not (0 < features.shape[0] <= self.head_phase_max_batch):
            return False
        c, o, u, k = self.classification_head, self.ordinal_head, self.uncertainty_head, self.kan_module
        if not (type(c) is ClassificationHead and type(o) is OrdinalHead and type(u) is UncertaintyHead and type(k) is KANSeverityModule):
            return False
        E, hid, C = features.shape[1], c.fc1.out_features, c.fc2.out_features
        if not (c.fc1.in_features == o.fc1.in_features == u.fc1.in_features == E and o.fc1.out_features == hid == u.fc1.out_features):
            return False
        if not (E % 4 == 0 and E <= 768 and hid % 4 == 0 and hid <= 256 and 2 <= C <= 8 and o.fc2.out_features == C - 1):
            return False
        d = k.layers_dims
        if not (k.degree == 3 and 1 <= len(k.kan_layers) <= 4 and d[0] == E and all(1 <= w <= 64 for w in d[1:]) and
                all(8 <= l.knots.numel() <= 64 for l in k.kan_layers)):
            # (num_knots 5 / 6: dense basis rows; any other grid: one 16-byte load of the four live weights per (input, output) pair --
            # BASELINE configs[4], num_knots 32 at batch 512: 50 us forward against 54 for the three per-layer launches, backward 144 against 126)
            return False
        if len({self._drop_p(h) for h in (c, o, u)}) != 1:      # the kernel draws one p for every head, or none
            return False
        for top in (c, o, u, k):
            for m in top.modules():
                if m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, '_backward_pre_hooks', None):
                    return False
        return True

    @staticmethod
    def _drop_p(head) -> float:
        """The dropout probability a forward applies to this head's hidden layer: its Dropout's p if that module is in training
        mode, else 0."""
        return float(head.dropout.p) if dropout_active(head.dropout) else 0.0

    def _kan_params(self):
        out = []
        for l in self.kan_module.kan_layers:
            out += [l.spline_weights, l.linear.weight, l.linear.bias]
        return out

    def _forward_head_phase(self, features: torch.Tensor, stage: int) -> Dict[str, torch.Tensor]:
        k = self.kan_module
        nl = len(k.kan_layers)
        cfg = {'stage': stage, 'masks': None, 'drop_p': 0.0, 'seed': 0, 'offset': 0,
               'kan_dims': list(k.layers_dims) if stage >= 4 else [],
               'kan_knots': [l.knots for l in k.kan_layers] if stage >= 4 else [],
               'kan_acts': [ACT_SIGMOID3 if i == nl - 1 else ACT_RELU for i in range(nl)],
               'grad_views': getattr(self, '_head_grad_views', None)}
        p = self._drop_p(self.classification_head)          # every head's (_head_phase_fusable)
        if p > 0.0:
            # dropout drawn inside the kernel (Philox keyed by the device generator's seed, counter advanced like torch's own kernels do)
            gen = torch.cuda.default_generators[features.device.index]
            n = features.shape[0] * self.classification_head.fc1.out_features
            off = gen.get_offset()
            gen.set_offset(off + 4 * ((n + 3) // 4))
            cfg.update(drop_p=float(p), seed=gen.initial_seed(), offset=off)
        cls_logits, ordinal_logits, mu, log_var, kan = HeadPhaseFn.apply(features, cfg, *self._head_params(),
                                                                         *(self._kan_params() if stage >= 4 else []))
        return {
            'cls_logits': cls_logits,
            'features': features,
            'ordinal_logits': ordinal_logits if stage >= 2 else None,
            'mu': mu if stage >= 3 else None,
            'log_var': log_var if stage >= 3 else None,
            'kan_severity': kan if stage >= 4 else None,
        }

    def _empty_outputs(self, x: torch.Tensor, stage: int) -> Dict[str, torch.Tensor]:
        """An empty batch gives empty outputs of the right widths, as the reference's modules do (every op of
        rovit_kan.py:88-124 accepts a zero-length batch dimension); no kernel is launched."""
        from rovit_hip import native
        native.ptr(x)                             # same device / dtype rules as a real batch (CPU tensors raise)
        z = lambda w: torch.zeros(0, w, device=x.device, dtype=torch.float32)
        return {'cls_logits': z(self.classification_head.fc2.out_features), 'features': z(self.backbone.embed_dim),
                'ordinal_logits': z(self.ordinal_head.fc2.out_features) if stage >= 2 else None,
                'mu': z(1) if stage >= 3 else None, 'log_var': z(1) if stage >= 3 else None,
                'kan_severity': z(self.kan_module.layers_dims[-1]) if stage >= 4 else None}

    def predict(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        self.eval()
        with torch.no_grad():
            out = self.forward(x)
            probs = torch.softmax(out['cls_logits'], dim=1)
            pred = {'class': torch.argmax(probs, dim=1), 'class_probs': probs, 'features': out['features']}
            if out['ordinal_logits'] is not None:
                p = OrdinalHead.probabilities_from_logits(out['ordinal_logits'])
                levels = torch.arange(p.shape[1], dtype=torch.float32, device=p.device)
                pred['ordinal_probs'] = p
                pred['ordinal_severity'] = (p * levels).sum(dim=1, keepdim=True)
            if out['mu'] is not None:
                pred['uncertainty_mu'] = out['mu']
                pred['uncertainty_std'] = torch.exp(0.5 * out['log_var'])
            if out['kan_severity'] is not None:
                pred['kan_severity'] = out['kan_severity']
            return pred

    def predict_mc(self, x: torch.Tensor, num_samples: int = 30, seed=None, return_samples: bool = False, *,
                   offset: int = 0) -> Dict[str, torch.Tensor]:
        """Extension (not in the reference): Monte-Carlo dropout over the heads -- one backbone forward and one launch for every
        sample (rovit_hip.mc_dropout.mc_dropout_predict).  Unlike predict(), leaves every module's training flag as it found it.
        ``offset`` (with an explicit ``seed``) moves the Philox counter, so the batches of one pass draw different masks."""
        from rovit_hip import mc_dropout
        return mc_dropout.mc_dropout_predict(self, x, num_samples, seed, return_samples, offset=offset)

    def _head_dropouts(self):
        return (self.classification_head.dropout, self.ordinal_head.dropout, self.uncertainty_head.dropout)

    def enable_dropout(self):
        """The interface the reference's BaselineModel declares (experiments/baselines.py:48-52, empty there), for MC dropout: the
        three heads' Dropout modules to training mode (the only dropout with p > 0; the backbone's is 0), the rest as it is."""
        for d in self._head_dropouts():
            d.train()

    def disable_dropout(self):
        """BaselineModel.disable_dropout's slot (experiments/baselines.py:51-52): the heads' Dropout modules back to eval mode."""
        for d in self._head_dropouts():
            d.eval()

    def set_patch_dropout(self, keep: float = 1.0, seed: int = 0):
        """Extension (not in the reference): DeiTTinyBackbone.set_patch_dropout of the backbone (PatchDropout in train() mode)."""
        self.backbone.set_patch_dropout(keep, seed)
        return self

    def freeze_backbone(self):
        self.backbone.freeze()

    def unfreeze_backbone(self):
        self.backbone.unfreeze()

    def get_attention_maps(self, x: torch.Tensor):
        return self.backbone.get_attention_maps(x)

    def attention_rollout(self, x: torch.Tensor, head_fusion: str = 'mean', upsample: bool = True):
        """Extension (not in the reference): DeiTTinyBackbone.attention_rollout of the backbone."""
        return self.backbone.attention_rollout(x, head_fusion, upsample)

    def attention_head_stats(self, x_or_loader, per_token: bool = False, chunk: int = 256):
        """Extension (not in the reference): per-head attention statistics (rovit_hip.head_stats).  A (B,3,224,224) tensor gives the
        per-image dict of DeiTTinyBackbone.attention_head_stats; an iterable of (images, class_labels, severity_labels) batches gives
        their mean and variance over the data set, for all images and per class label (``per_token`` is refused there)."""
        from rovit_hip import head_stats
        return head_stats.model_head_stats(self, x_or_loader, per_token, chunk)

    def grad_cam_pp(self, x: torch.Tensor, class_idx=None, upsample: bool = True, return_taps: bool = False, target='class'):
        """Extension (not in the reference): Grad-CAM++ at blocks[-1].norm1 for every image of the batch on the GPU, of cls_logits or,
        with ``target=``, of ordinal_severity / mu / log_var / kan_severity, or of several of them from one forward
        (rovit_hip.gradcam.grad_cam_pp)."""
        from rovit_hip import gradcam
        return gradcam.grad_cam_pp(self, x, class_idx, upsample, return_taps, target)

    def input_gradients(self, x: torch.Tensor, target='class', class_idx=None, steps: int = 0, baseline=None, chunk: int = 256,
                        return_values: bool = False):
        """Extension (not in the reference): d target / d images of cls_logits, ordinal_severity, mu, log_var or kan_severity for every
        image of the batch on the GPU, or with ``steps >= 1`` their integrated gradients from ``baseline`` (rovit_hip.input_grad)."""
        from rovit_hip import input_grad
        return input_grad.input_gradients(self, x, target, class_idx, steps, baseline, chunk, return_values)

    def adversarial_examples(self, x: torch.Tensor, labels=None, **kw):
        """Extension (not in the reference): adversarial images of ``x`` inside an L-infinity or L2 ball by projected gradient ascent on
        the GPU, against the class (cross-entropy or margin) or a severity output (rovit_hip.attack.pgd_attack, whose keywords apply)."""
        from rovit_hip import attack
        return attack.pgd_attack(self, x, labels, **kw)

    def robustness_radius(self, x: torch.Tensor, labels, norm: str = 'linf', eps_max: float = 8 / 255, search_steps: int = 8, steps: int = 10,
                          **kw):
        """Extension (not in the reference): per image, the smallest radius at which the attack changes the class -- a bisection over
        eps for the whole batch at once; an upper bound on the true radius (rovit_hip.attack.robustness_radius)."""
        from rovit_hip import attack
        return attack.robustness_radius(self, x, labels, norm, eps_max, search_steps, steps, **kw)

    def attention_relevance(self, x: torch.Tensor, target='class', class_idx=None, upsample: bool = True, chunk: int = 256,
                            return_values: bool = False):
        """Extension (not in the reference): gradient-weighted attention relevance (Chefer, Gur & Wolf 2021) of cls_logits,
        ordinal_severity, mu, log_var or kan_severity for every image of the batch on the GPU, through every block
        (rovit_hip.relevance)."""
        from rovit_hip import relevance
        return relevance.attention_relevance(self, x, target, class_idx, upsample, chunk, return_values)

    def perturbation_curves(self, x: torch.Tensor, saliency, target='class', class_idx=None, modes=('deletion', 'insertion'),
                            steps: int = 28, perturbation: str = 'replace', baseline=None, chunk: int = 256, ragged: bool = False):
        """Extension (not in the reference): deletion / insertion curves and their areas (Petsiuk et al. 2018) of one or several
        saliency maps for cls_logits' probability, ordinal_severity, mu, log_var or kan_severity on the GPU, patches replaced by a
        baseline's or dropped from the sequence (rovit_hip.perturbation; ``ragged``: dropped sequences of all lengths share backbone calls)."""
        from rovit_hip import perturbation as pert
        return pert.perturbation_curves(self, x, saliency, target, class_idx, modes, steps, perturbation, baseline, chunk, ragged)

    def patch_shap(self, x: torch.Tensor, target='class', class_idx=None, num_samples: int = 2048, players=14, perturbation: str = 'drop',
                   baseline=None, seed: int = 0, chunk: int = 256, upsample: bool = True, return_values: bool = False,
                   ragged: bool = False):
        """Extension (not in the reference): KernelSHAP values of the patches, or of any grouping of them into players, for the
        probability of a class, ordinal_severity, mu, log_var or kan_severity on the GPU; absent players' patches are dropped from the
        sequence or replaced by a baseline's, and the values sum to f(image) - f(nothing) (rovit_hip.shap)."""
        from rovit_hip import shap
        return shap.patch_shap(self, x, target, class_idx, num_samples, players, perturbation, baseline, seed, chunk, upsample, return_values,
                               ragged)

    def kan_edge_stats(self, x_or_loader, chunk: int = 256):
        """Extension (not in the reference): per-edge activation statistics of the KAN head over images (a (B,3,224,224) tensor, or an
        iterable of batches whose first element is the images): magnitude, spline share, knot-span occupancy and dead-zone share
        of every edge on the GPU (rovit_hip.kan_stats)."""
        from rovit_hip import kan_stats
        return kan_stats.model_edge_stats(self, x_or_loader, chunk)

    def kan_regrid(self, x_or_loader, chunk: int = 256, **fit_kw):
        """Extension (not in the reference): KAN grid extension over images (a (B,3,224,224) tensor, or an iterable of batches whose first
        element is the images): every edge spline of the KAN head is refitted to a new uniform grid by least squares on this model's
        backbone features and installed (rovit_hip.kan_grid; ``num_knots``, ``knots``, ``span``, ``layout``, ``margin``, ``prior_weight``,
        ``layers`` as ``KANRegrid.fit``).  Returns the ``RegridResult``.  Build a new optimizer afterwards."""
        from rovit_hip import kan_grid
        return kan_grid.model_regrid(self, x_or_loader, chunk, **fit_kw)

    def kan_attribution(self, x_or_loader, chunk: int = 256):
        """Extension (not in the reference): ``kan_edge_stats`` plus pykan's attribution scores of every edge, node and backbone
        feature for the severity output: ``{'stats', 'edge_scores', 'node_scores', 'feature_scores'}``."""
        from rovit_hip import kan_stats
        stats = kan_stats.model_edge_stats(self, x_or_loader, chunk)
        return {'stats': stats, **kan_stats.kan_attribution(stats)}

    def fit_feature_density(self, x_or_loader, labels=None, shrinkage: float = 1e-3, chunk: int = 256):
        """Extension (not in the reference): a fitted ``rovit_hip.density.FeatureDensity`` of this model's backbone features over images
        (a (B,3,224,224) tensor with ``labels``, or an iterable of batches ``(images, class_labels, ...)``): class-conditional Gaussians
        with a tied, shrunk covariance, the moments on the GPU."""
        from rovit_hip import density
        return density.fit_model_density(self, x_or_loader, labels, shrinkage, chunk)

    def ood_scores(self, x: torch.Tensor, density) -> Dict[str, torch.Tensor]:
        """Extension (not in the reference): the forward plus ``density.score(features, cls_logits)``: Mahalanobis and relative
        Mahalanobis distance of every image's features from the fitted training features, with energy and 1 - max p beside them."""
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                out = self(x)
        finally:
            self.train(was_training)
        return density.score(out['features'], out['cls_logits'])

    def fit_laplace(self, x_or_loader, prior_precision='marglik', chunk: int = 256):
        """Extension (not in the reference): a fitted ``rovit_hip.laplace.HeadLaplace`` of this model's classification head and, from
        curriculum stage 3, of the Gaussian head's ``mu`` layer over images (a (B,3,224,224) tensor, or an iterable of batches whose first
        element is the images): last-layer Laplace approximation with the GGN Hessian, the weighted Grams on the GPU.  No labels."""
        from rovit_hip import laplace
        return laplace.fit_model_laplace(self, x_or_loader, prior_precision, chunk)

    def predict_laplace(self, x: torch.Tensor, laplace) -> Dict[str, torch.Tensor]:
        """Extension (not in the reference): the forward plus ``laplace.predict(features, cls_logits, mu, log_var)``: the closed-form
        logit covariance, probit-adjusted class probabilities and, from stage 3, the epistemic variance of ``mu`` and ``total_std``;
        ``class`` is the argmax of the adjusted probabilities."""
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                out = self(x)
        finally:
            self.train(was_training)
        pred = dict(laplace.predict(out['features'], out['cls_logits'], out.get('mu'), out.get('log_var')))
        pred['class'] = torch.argmax(pred['probs'], dim=1)
        return pred

    def fit_feature_index(self, x_or_loader, labels=None, severity=None, metric: str = 'cosine', chunk: int = 256):
        """Extension (not in the reference): a built ``rovit_hip.neighbors.FeatureIndex`` of this model's backbone features over images
        (a (B,3,224,224) tensor with optional ``labels`` and ``severity``, or an iterable of batches ``(images, class_labels,
        severity_labels, ...)``): the rows a nearest-neighbour search answers from."""
        from rovit_hip import neighbors
        return neighbors.fit_model_index(self, x_or_loader, labels, severity, metric, chunk)

    def feature_map(self, x_or_loader, chunk: int = 256, **tsne_kwargs) -> Dict:
        """Extension (not in the reference): the exact t-SNE map of this model's backbone features over images (a (B,3,224,224) tensor or
        an iterable of batches, gathered as ``fit_feature_index`` gathers them: eval mode, ``chunk`` images at a time, no ``.grad``
        written).  ``tsne_kwargs`` go to ``rovit_hip.embedding.TSNE``.  Returns ``map`` (n, 2), ``features`` (n, E) and
        ``kl_divergence`` (a 0-d device tensor: nothing is copied to the host)."""
        from rovit_hip import embedding, neighbors
        feats = neighbors.fit_model_index(self, x_or_loader, metric='l2', chunk=chunk).rows().clone()
        tsne = embedding.TSNE(**tsne_kwargs)
        return {'map': tsne.fit_transform(feats), 'features': feats, 'kl_divergence': tsne.kl_trace_[-1]}

    def cluster_features(self, x_or_loader, n_clusters: int, labels=None, chunk: int = 256, **kw) -> Dict:
        """Extension (not in the reference): k-means (k-means++ seeding) of this model's backbone features over images, gathered as
        ``fit_feature_index`` gathers them.  ``kw`` go to ``rovit_hip.clustering.KMeans``.  Returns the fitted object under ``kmeans``,
        ``features``, ``labels``, ``distances``, ``cluster_centers``, ``medoids``, ``counts``, ``silhouette``, and with class ``labels``
        the cluster-by-class ``score_card`` (purity, NMI, ARI: a label audit that needs no trained head)."""
        from rovit_hip import clustering
        return clustering.cluster_model_features(self, x_or_loader, n_clusters, labels, chunk, **kw)

    def nearest_examples(self, x: torch.Tensor, index, k: int = 5) -> Dict[str, torch.Tensor]:
        """Extension (not in the reference): explanation by example.  One forward, then ``index.search(features, k)``: the ``k`` nearest
        recorded rows of every image with their labels and severities, the neighbours' vote, and beside it the heads' own ``class``
        under ``head_class`` and, from curriculum stage 2, ``ordinal_severity`` under ``head_ordinal_severity``."""
        pred = self.predict(x)
        out = dict(index.search(pred['features'], k=k))
        out['head_class'] = pred['class']
        if 'ordinal_severity' in pred:
            out['head_ordinal_severity'] = pred['ordinal_severity']
        return out

    def fit_influence(self, train_loader, laplace=None, chunk: int = 256):
        """Extension (not in the reference): a ``rovit_hip.influence.HeadInfluence`` over an iterable of batches ``(images, class_labels,
        severity_labels, ...)``: the whitened last-layer gradients of every training row, embedded on the GPU in one pass.  Without a
        fitted ``laplace`` (a ``HeadLaplace``) the same pass fits one."""
        from rovit_hip import influence
        return influence.fit_model_influence(self, train_loader, laplace, chunk)

    def influential_examples(self, x: torch.Tensor, influence, k: int = 5, labels=None, relative: bool = True) -> Dict[str, torch.Tensor]:
        """Extension (not in the reference): explanation by training example.  One forward, then ``influence.search(features, cls_logits,
        labels, k=k, relative=relative)``: the ``k`` proponents and opponents of the loss of every image's label (without ``labels``: of
        the prediction made) with their scores, indices and labels, and beside them the head's own ``class`` under ``head_class``."""
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                fwd = self(x)
        finally:
            self.train(was_training)
        out = dict(influence.search(fwd['features'], fwd['cls_logits'], labels, k=k, relative=relative))
        out['head_class'] = torch.argmax(fwd['cls_logits'], dim=1)
        return out

    def count_parameters(self) -> Dict[str, int]:
        def n(m):
            return sum(p.numel() for p in m.parameters() if p.requires_grad)
        counts = {'backbone': n(self.backbone), 'classification_head': n(self.classification_head),
                  'ordinal_head': n(self.ordinal_head), 'uncertainty_head': n(self.uncertainty_head),
                  'kan_module': n(self.kan_module)}
        counts['total'] = sum(counts.values())
        return counts
