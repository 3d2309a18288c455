"""The reference's evaluation/evaluator.py (:16-110 Evaluator, :226-253 load_model_for_evaluation) on ``rovit_hip.evaluation``: one
launch per batch records the predictions on the device, one launch per epoch reduces them, one device-to-host copy brings the result
block back.  Same constructor, same returned dict, same printed table, same ``evaluation_results.txt``.  Figures are not drawn
(SURVEY.md section 2); ``evaluate(return_arrays=True)`` hands back the arrays the reference's plots are made from.  A last batch of one
sample works (the reference's ``squeeze()`` + ``np.concatenate`` raises there).  ``evaluate(bootstrap=R)`` adds percentile bootstrap
intervals (``EvalAccumulator.bootstrap``) to the dict, the table and the file; with the default 0 all three are what they were.
``evaluate(selective=True)`` adds the selective-prediction score card (``EvalAccumulator.selective``: AURC, E-AURC and the risk left at
80 % and 90 % coverage for every uncertainty score) in the same way.  ``fit_calibration(val_loader)`` fits a temperature and a sigma
scale on another split (``EvalAccumulator.calibrate``); ``evaluate(calibration=cal)`` reports NLL, ECE, Brier score, Gaussian NLL and
interval coverage of the test set before and after applying it, beside the raw model's headline metrics.
``fit_density(train_loader)`` fits the feature-space density of ``rovit_hip.density``; ``evaluate(density=fd)`` records each row's
Mahalanobis and relative Mahalanobis distance as extra columns (two more scores of the selective card), and ``evaluate_ood(ood_loader)``
scores the test set against an out-of-distribution loader: AUROC, AUPR and FPR at 95 % TPR of every uncertainty score.
``fit_conformal(val_loader)`` fits split-conformal thresholds on another split (``EvalAccumulator.conformal``);
``evaluate(conformal=cp)`` reports the coverage and size of the label sets and the coverage and width of the severity intervals on the
test set (``Conformal.evaluate``).
``fit_index(train_loader)`` records the training features in a ``rovit_hip.neighbors.FeatureIndex``; ``evaluate(index=fi, knn_k=10)``
records each row's distance to its k-th nearest training feature as the extra column ``knn_distance`` (one more score of the selective
card) and adds ``metrics['knn']``: how well the neighbour-weighted vote alone classifies and estimates severity, and how often it agrees
with the classification head; ``evaluate_ood(..., index=fi)`` adds the ``'knn'`` card.
``evaluate_corruptions(store_or_loader)`` is the corruption-robustness score card: the test images corrupted on the device from the uint8
store (``rovit_hip.corrupt``), one card per (corruption, severity) cell, the corruption errors and, against a baseline, CE and mCE.
``evaluate_adversarial(loader)`` is its worst-case counterpart: the test images attacked on the device inside a ball of each radius
(``rovit_hip.attack``), one card per radius with the robust accuracy, the flip rate and how far the severity outputs can be pushed.
``fit_laplace(train_loader)`` fits the last-layer Laplace approximation of the heads (``rovit_hip.laplace.HeadLaplace``);
``evaluate(laplace=la)`` records each row's mean logit variance and, from stage 3, the total standard deviation of ``mu`` as the extra
columns ``laplace_logit_var`` and ``laplace_mu_std`` (two more scores of the selective card) and adds ``metrics['laplace']``: the prior
precisions, and NLL, ECE, Brier score and accuracy before and after the probit adjustment; ``evaluate_ood(..., laplace=la)`` adds the
``'laplace'`` card.
``fit_influence(train_loader)`` embeds the training rows' whitened last-layer gradients (``rovit_hip.influence.HeadInfluence``);
``audit_labels(top)`` prints and saves the "Label audit" table: the training rows with the largest self-influence, the ones whose labels
deserve a second look.  Neither changes what ``evaluate`` returns, prints or saves."""
from pathlib import Path
from typing import Dict

import torch

from evaluation.metrics import count_params, fps
from rovit_hip.evaluation import EvalAccumulator, RovitHipError, class_table

RULE = '=' * 60


class Evaluator:

    def __init__(self, model, test_loader, config, device):
        self.model = model.to(device)
        self.test_loader = test_loader
        self.config = config
        self.device = torch.device(device)
        self.model.eval()
        self.accumulator = None
        self.calibration = None
        self.density = None
        self.conformal = None
        self.index = None
        self._knn_tally = None
        self.laplace = None
        self._laplace_acc = None
        self.influence = None

    MC_COLUMNS = ('predictive_entropy_mc', 'mutual_information', 'epistemic_var', 'uncertainty_std')

    DENSITY_COLUMNS = ('mahalanobis', 'relative_mahalanobis')
    KNN_COLUMN = 'knn_distance'
    LAPLACE_COLUMNS = ('laplace_logit_var', 'laplace_mu_std')
    OOD_LEVEL = 0.95

    def collect(self, selective: bool = False, mc_samples: int = 0, mc_seed: int = 0, record_mu: bool = False, density=None, index=None,
                knn_k: int = 10, laplace=None) -> EvalAccumulator:
        """The collection loop alone: one forward and one record launch per batch, nothing copied to the host.  ``selective`` (or
        ``record_mu``) also records the uncertainty head's ``mu`` as an extra column when the model returns one; ``mc_samples = T > 0``
        adds the MC-dropout columns of ``model.predict_mc(images, num_samples=T, seed=mc_seed, offset=batch index)``, a SECOND backbone
        pass per batch."""
        if mc_samples and not selective:
            raise RovitHipError('Evaluator: mc_samples records columns for the selective score card; pass selective=True with it')
        acc = self.accumulator = self._collect(self.test_loader, selective, mc_samples, mc_seed, record_mu, density, index, knn_k, laplace)
        return acc

    def fit_laplace(self, loader, prior_precision='marglik'):
        """Fit the last-layer Laplace approximation of the heads (``RoViTKAN.fit_laplace``) on another split, normally the training
        loader: one forward pass, the weighted Grams on the GPU, one device-to-host copy, the factorisation on the host.  No labels are
        read.  The ``HeadLaplace`` is returned and kept on ``self.laplace``; pass it to ``evaluate(laplace=...)`` or
        ``evaluate_ood(..., laplace=...)``."""
        self.laplace = self.model.fit_laplace(loader, prior_precision=prior_precision)
        return self.laplace

    def fit_influence(self, train_loader):
        """Embed the whitened last-layer gradients of the training rows (``RoViTKAN.fit_influence``): one forward pass that also fits the
        Laplace approximation unless ``fit_laplace`` has been called, one embed launch per head and batch.  The ``HeadInfluence`` is
        returned and kept on ``self.influence``; ``audit_labels`` reads it."""
        self.influence = self.model.fit_influence(train_loader, laplace=self.laplace)
        return self.influence

    def audit_labels(self, top: int = 50, results_dir=None) -> Dict:
        """The ``top`` training rows by self-influence (``HeadInfluence.label_audit``), the standard audit score for label noise: prints
        a "Label audit" table and saves ``label_audit.txt`` / ``label_audit.json`` to ``results_dir`` (default: the config's).  Returns
        ``{'counts', 'rows': [{'index', 'label', 'predicted', 'label_prob', 'self_influence'}, ...]}``."""
        import json
        if self.influence is None:
            raise RovitHipError('Evaluator.audit_labels: fit_influence(train_loader) first')
        audit = {k: v.cpu().tolist() for k, v in self.influence.label_audit(top).items()}
        names = list(self.config.data.class_names)
        name = lambda c: names[c] if 0 <= c < len(names) else str(c)
        rows = [{'index': i, 'label': y, 'predicted': p, 'label_prob': q, 'self_influence': s}
                for i, y, p, q, s in zip(audit['indices'], audit['labels'], audit['predicted'], audit['label_prob'], audit['scores']) if i >= 0]
        result = {'counts': self.influence.counts(), 'rows': rows}
        lines = [f"Label audit (top {len(rows)} of {result['counts']['n_valid']} valid training rows by self-influence):",
                 f"{'Index':>8}  {'Given label':<20}{'Predicted':<20}{'P(label)':>10}{'Self-influence':>16}", '-' * 76]
        lines += [f"{r['index']:>8}  {name(r['label']):<20}{name(r['predicted']):<20}{r['label_prob']:>10.4f}{r['self_influence']:>16.6g}" for r in rows]
        print('\n'.join(lines + ['']))
        if results_dir is None:
            results_dir = getattr(getattr(self.config, 'paths', None), 'results_dir', None)
        if results_dir is not None:
            results_dir = Path(results_dir)
            results_dir.mkdir(parents=True, exist_ok=True)
            (results_dir / 'label_audit.txt').write_text('\n'.join(lines) + '\n', encoding='utf-8')
            (results_dir / 'label_audit.json').write_text(json.dumps(result, indent=2) + '\n', encoding='utf-8')
        return result

    def fit_index(self, loader, metric: str = 'cosine'):
        """Record the backbone features of another split, normally the training loader, with their class labels and severities in a
        ``FeatureIndex`` (``RoViTKAN.fit_feature_index``): one backbone pass and one build launch, nothing copied to the host.  The index
        is returned and kept on ``self.index``; pass it to ``evaluate(index=...)`` or ``evaluate_ood(..., index=...)``."""
        self.index = self.model.fit_feature_index(loader, metric=metric)
        return self.index

    def fit_density(self, loader, shrinkage: float = 1e-3):
        """Fit the feature-space density (``RoViTKAN.fit_feature_density``) on another split, normally the training loader: one backbone
        pass, the moments on the GPU, one device-to-host copy.  The ``FeatureDensity`` is returned and kept on ``self.density``; pass it
        to ``evaluate(density=...)`` or ``evaluate_ood(..., density=...)``."""
        self.density = self.model.fit_feature_density(loader, shrinkage=shrinkage)
        return self.density

    def fit_calibration(self, loader):
        """Fit a post-hoc calibration on another split, normally the validation loader: the collection loop with ``mu`` recorded, then
        ONE ``EvalAccumulator.calibrate`` call (one device-to-host copy).  The ``Calibration`` is returned and kept on
        ``self.calibration``; pass it to ``evaluate(calibration=...)``."""
        self.calibration = self._collect(loader, False, 0, 0, True).calibrate()
        return self.calibration

    def fit_conformal(self, loader, **kw):
        """Fit split-conformal thresholds on another split, normally the validation loader: the collection loop with ``mu`` recorded,
        then ONE ``EvalAccumulator.conformal(**kw)`` call (one device-to-host copy).  The ``Conformal`` is returned and kept on
        ``self.conformal``; pass it to ``evaluate(conformal=...)``."""
        self.conformal = self._collect(loader, False, 0, 0, True).conformal(**kw)
        return self.conformal

    def _collect(self, loader, selective: bool, mc_samples: int, mc_seed: int, record_mu: bool, density=None, index=None,
                 knn_k: int = 10, laplace=None) -> EvalAccumulator:
        acc = EvalAccumulator(len(self.config.data.class_names))
        self._knn_tally = [] if index is not None else None
        self._laplace_acc = EvalAccumulator(len(self.config.data.class_names)) if laplace is not None else None
        self.model.eval()
        with torch.no_grad():
            for batch_index, (images, class_labels, severity_labels) in enumerate(loader):
                images = images.to(self.device)
                outputs = self.model(images)
                extra = {}
                if (selective or record_mu) and outputs.get('mu') is not None:
                    extra['mu'] = outputs['mu']
                if selective and mc_samples:
                    mc = self.model.predict_mc(images, num_samples=mc_samples, seed=mc_seed, offset=batch_index)
                    extra['predictive_entropy_mc'], extra['mutual_information'] = mc['predictive_entropy'], mc['mutual_information']
                    if 'epistemic_var' in mc:                 # from curriculum stage 3
                        extra['epistemic_var'], extra['uncertainty_std'] = mc['epistemic_var'], mc['uncertainty_std']
                if density is not None:
                    d = density.score(outputs['features'])
                    for k in self.DENSITY_COLUMNS:
                        extra[k] = d[k]
                if index is not None:
                    nn = index.search(outputs['features'], k=knn_k)
                    extra[self.KNN_COLUMN] = nn['kth_distance']
                    self._knn_tally.append(self._knn_row(nn, outputs, class_labels, severity_labels))
                if laplace is not None:
                    la = laplace.predict(outputs['features'], outputs['cls_logits'], outputs.get('mu'), outputs.get('log_var'))
                    extra[self.LAPLACE_COLUMNS[0]] = la['mean_logit_var']
                    if 'total_std' in la:                         # from curriculum stage 3
                        extra[self.LAPLACE_COLUMNS[1]] = la['total_std']
                    # the same rows with the probit-adjusted probabilities in place of the softmax: softmax(log p') = p'
                    adjusted = dict(outputs, cls_logits=torch.log(la['probs'].clamp_min(torch.finfo(torch.float32).tiny)))
                    self._laplace_acc.update(adjusted, class_labels, severity_labels)
                acc.update(outputs, class_labels, severity_labels, extra=extra or None)
        return acc

    @staticmethod
    def _knn_row(nn: Dict, outputs: Dict, class_labels, severity_labels) -> torch.Tensor:
        """One batch's tallies of the neighbour vote as a (4,) fp64 tensor on the features' device, over the rows that VOTED (a finite
        ``kth_distance``: at least one neighbour; a bad query row, or an index without a valid row, has none): such rows, those whose
        vote equals the label, the sum of |vote severity - label severity|, those whose vote equals the classification head's argmax.
        Nothing is copied to the host."""
        dev = nn['kth_distance'].device
        voted = torch.isfinite(nn['kth_distance'])
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        hit = agree = err = zero
        if 'class' in nn:
            vote = nn['class'].to(torch.int64)
            hit = (voted & (vote == class_labels.to(dev).reshape(-1).to(torch.int64))).sum().to(torch.float64)
            agree = (voted & (vote == outputs['cls_logits'].argmax(dim=1))).sum().to(torch.float64)
        if 'severity' in nn:
            diff = (nn['severity'].double() - severity_labels.to(dev).reshape(-1).double()).abs()
            err = torch.where(voted, diff, torch.zeros_like(diff)).sum()
        return torch.stack([voted.sum().to(torch.float64), hit, err, agree])

    def _knn_card(self, index, knn_k: int) -> Dict:
        """``metrics['knn']`` from the batches' tallies: one device-to-host copy of four numbers.  Every ratio is over the rows that
        voted (see ``_knn_row``); with none, the three figures are None."""
        rows, hit, err, agree = torch.stack(self._knn_tally).sum(dim=0).cpu().tolist()
        voted = bool(index.has_labels) and index.num_classes is not None and rows > 0
        return {'k': knn_k, 'accuracy': 100.0 * hit / rows if voted else None,
                'severity_mae': err / rows if index.has_severity and rows > 0 else None, 'agreement': agree / rows if voted else None}

    def evaluate(self, return_arrays: bool = False, bootstrap: int = 0, bootstrap_seed: int = 0, selective: bool = False,
                 mc_samples: int = 0, mc_seed: int = 0, calibration=None, density=None, conformal=None, index=None, knn_k: int = 10,
                 laplace=None):
        """``selective=True`` adds ``metrics['selective']`` (``EvalAccumulator.selective`` with 20 coverages: the built-in scores, and
        with ``mc_samples = T > 0`` the MC-dropout scores predictive_entropy_mc and mutual_information, from curriculum stage 3 also
        epistemic_var and uncertainty_std) and a "Selective prediction" section in the table and the file.  The MC columns cost a
        second backbone pass per batch, and they depend on the batch split (the dropout masks are drawn per batch position); the
        kernel's determinism holds for given columns.

        ``calibration`` (a ``Calibration``, normally ``fit_calibration(val_loader)``) adds ``metrics['calibration']``: ``temperature``,
        ``sigma_scale``, ``status`` and the dicts ``before`` / ``after`` with ``nll``, ``ece``, ``brier_score``, ``gaussian_nll``, ``coverage``
        and ``sigma_scale_refit`` of the test rows as recorded and after ``calibration.apply``; ``after`` comes from the applied
        accumulator's own ``compute()`` and ``calibrate()``.  The headline metrics stay those of the raw model.  With ``selective=True``
        the selective card of the applied accumulator is added under ``metrics['calibration']['selective']``.

        ``density`` (a fitted ``FeatureDensity``, normally ``fit_density(train_loader)``) records ``mahalanobis`` and
        ``relative_mahalanobis`` of every row as extra columns (one more launch per batch); with ``selective=True`` they are two more
        scores of the card: does distance from the training features know which rows the model gets wrong?

        ``conformal`` (a ``Conformal``, normally ``fit_conformal(val_loader)``) adds ``metrics['conformal']``, what
        ``Conformal.evaluate`` returns for the test rows (one more device-to-host copy), and a "Conformal prediction" section in the
        table and the file.

        ``index`` (a built ``FeatureIndex``, normally ``fit_index(train_loader)``) records ``knn_distance``, the distance of every row
        to its ``knn_k``-th nearest recorded feature, as an extra column (one more search per batch; with ``selective=True`` one more
        score of the card), and adds ``metrics['knn']`` = ``{'k', 'accuracy', 'severity_mae', 'agreement'}``: accuracy (per cent) and
        severity MAE of the neighbour-weighted vote alone, and the share of rows where the vote and the classification head agree, all
        three over the rows that have at least one neighbour; a "Nearest neighbours" section goes into the table and the file.

        ``laplace`` (a fitted ``HeadLaplace``, normally ``fit_laplace(train_loader)``) records ``laplace_logit_var``, the mean over the
        classes of every row's closed-form logit variance, and from stage 3 ``laplace_mu_std`` = sqrt(sigma^2 + the epistemic variance
        of mu) as extra columns (one launch per head and batch; with ``selective=True`` two more scores of the card), and adds
        ``metrics['laplace']`` = ``{'prior_precision', 'status', 'prior_precision_mu', 'status_mu', 'n', 'before', 'after'}``: ``before``
        and ``after`` hold ``nll``, ``ece``, ``brier_score`` and ``accuracy`` of the softmax and of the probit-adjusted probabilities; a
        "Laplace approximation" section goes into the table and the file."""
        print(f'\n{RULE}\nRunning Evaluation on Test Set\n{RULE}\n')
        names = list(self.config.data.class_names)
        acc = self.collect(selective, mc_samples, mc_seed, record_mu=calibration is not None or conformal is not None, density=density,
                           index=index, knn_k=knn_k, laplace=laplace)
        ci = acc.bootstrap(bootstrap, seed=bootstrap_seed) if bootstrap else None          # brings the point block along in its one copy
        m = acc.compute()                                   # the loop's one synchronisation
        metrics = {k: m[k] for k in ('accuracy', 'macro_f1', 'weighted_f1', 'mae', 'spearman_rho', 'spearman', 'brier_score', 'ece')}
        metrics['fps'] = fps(self.model, (1, 3, 224, 224), self.device, n=100)
        metrics['params'] = count_params(self.model)
        metrics['params_m'] = metrics['params'] / 1e6
        metrics['per_class'] = class_table(m['per_class'], names)
        if ci is not None:
            ci['per_class'] = class_table(ci['per_class'], names)
            metrics['confidence_intervals'] = ci
        if selective:
            have = acc._extra_names or ()
            scores = ['confidence', 'entropy'] + (['sigma'] if acc._has_uncertainty else []) + [c for c in self.MC_COLUMNS + self.DENSITY_COLUMNS + (self.KNN_COLUMN,) + self.LAPLACE_COLUMNS if c in have]
            risks = ['error', 'abs_err'] + (['mu_abs_err'] if 'mu' in have else [])
            metrics['selective'] = acc.selective(scores=scores, risks=risks)
        if calibration is not None:
            applied = calibration.apply(acc)
            metrics['calibration'] = {'temperature': calibration.temperature, 'sigma_scale': calibration.sigma_scale, 'status': calibration.status,
                                      'before': self._calibration_card(acc, m), 'after': self._calibration_card(applied, applied.compute())}
            if selective:
                metrics['calibration']['selective'] = applied.selective(scores=scores, risks=risks)
        if conformal is not None:
            metrics['conformal'] = conformal.evaluate(acc)
        if index is not None:
            metrics['knn'] = self._knn_card(index, knn_k)
        if laplace is not None:
            metrics['laplace'] = self._laplace_card(laplace, acc, m)
        self._print_results(metrics)
        self._save_results(metrics)
        return (metrics, acc.arrays()) if return_arrays else metrics

    def _laplace_card(self, laplace, acc: EvalAccumulator, m: Dict) -> Dict:
        """``metrics['laplace']``: the fit's prior precisions, and the record as it is beside the record with the probit-adjusted
        probabilities (``_collect`` filled it), each by its own ``compute()`` and a ``calibrate()`` whose NLL at T = 1 describes it."""
        side = lambda a, mm: {'nll': a.calibrate().diagnostics['nll'], 'ece': mm['ece'], 'brier_score': mm['brier_score'], 'accuracy': mm['accuracy']}
        return {'prior_precision': laplace.prior_precision, 'status': laplace.status, 'prior_precision_mu': laplace.prior_precision_mu,
                'status_mu': laplace.status_mu, 'n': laplace.n, 'before': side(acc, m), 'after': side(self._laplace_acc, self._laplace_acc.compute())}

    def _ood_columns(self, loader, density, index=None, knn_k: int = 10, laplace=None) -> Dict[str, torch.Tensor]:
        """The anomaly scores of every image of a loader as device columns: nothing is copied to the host."""
        cols: Dict[str, list] = {}
        self.model.eval()
        with torch.no_grad():
            for batch in loader:
                images = (batch[0] if isinstance(batch, (tuple, list)) else batch).to(self.device)
                out = self.model(images)
                logp = torch.log_softmax(out['cls_logits'].float(), dim=1)
                p = logp.exp()
                row = {'max_prob': 1.0 - p.max(dim=1).values, 'entropy': -(p * logp).sum(dim=1),
                       'energy': -torch.logsumexp(out['cls_logits'].float(), dim=1)}
                if out.get('log_var') is not None:
                    row['sigma'] = torch.exp(0.5 * out['log_var'].float()).reshape(-1)
                if density is not None:
                    d = density.score(out['features'])
                    row.update({k: d[k] for k in self.DENSITY_COLUMNS})
                if index is not None:
                    row['knn'] = index.search(out['features'], k=knn_k)['kth_distance']
                if laplace is not None:
                    row['laplace'] = laplace.predict(out['features'], out['cls_logits'])['mean_logit_var']
                for k, v in row.items():
                    cols.setdefault(k, []).append(v)
        return {k: torch.cat(v) for k, v in cols.items()}

    def evaluate_ood(self, ood_loader, density=None, index=None, knn_k: int = 10, laplace=None) -> Dict[str, Dict]:
        """Extension (not in the reference): how well each uncertainty score tells the test set (in-distribution) from ``ood_loader``
        (out-of-distribution; batches of images, or tuples whose first element is the images).  One ``rovit_hip.density.ood_metrics``
        card per score (AUROC, AUPR both ways, FPR at 95 % TPR; one device-to-host copy each): ``max_prob`` = 1 - max p, ``entropy``,
        ``energy`` = -logsumexp, ``sigma`` when the model returns log_var, and with a fitted ``density`` ``mahalanobis`` and
        ``relative_mahalanobis``, and with a built ``index`` (a ``FeatureIndex``) ``knn``, the distance to the ``knn_k``-th nearest
        recorded feature (Sun et al. 2022), and with a fitted ``laplace`` (a ``HeadLaplace``) ``laplace``, the mean closed-form logit
        variance.  Printed as a table; higher = more anomalous for every score."""
        from rovit_hip.density import ood_metrics
        inside, outside = (self._ood_columns(l, density, index, knn_k, laplace) for l in (self.test_loader, ood_loader))
        cards = {k: ood_metrics(inside[k], outside[k], tpr_levels=(self.OOD_LEVEL,)) for k in inside if k in outside}
        lines = ['', 'Out-of-distribution detection:', f"{'Score':<24}{'AUROC':>10}{'AUPR-out':>10}{'AUPR-in':>10}{'FPR@95%TPR':>12}", '-' * 66]
        for k, c in cards.items():
            lines.append(f"{k:<24}{c['auroc']:>10.4f}{c['aupr_out']:>10.4f}{c['aupr_in']:>10.4f}{c['fpr_at_tpr'][self.OOD_LEVEL]:>12.4f}")
        print('\n'.join(lines + ['']))
        return cards

    CORRUPTION_CARD = ('accuracy', 'macro_f1', 'mae', 'brier_score', 'ece')

    def _corruption_source(self, source):
        """(store, index list, batch size) of a ``DeviceImageStore`` or of a loader that carries one."""
        from rovit_hip.augment import DeviceImageStore
        source = self.test_loader if source is None else source
        if isinstance(source, DeviceImageStore):
            return source, list(range(len(source))), 64
        store, subset = getattr(source, 'store', None), getattr(source, 'dataset', None)
        if not isinstance(store, DeviceImageStore) or not hasattr(subset, 'indices'):
            raise RovitHipError('evaluate_corruptions needs the uint8 images on the device: pass a DeviceImageStore, or build the loaders '
                                'with create_dataloaders(..., device_cache=True)')
        return store, list(subset.indices), int(getattr(source, 'batch_size', 64))

    def _corruption_cell(self, store, order, batch_size: int, name: str, param: float, seed: int, clean_pred):
        """One cell: one pass into a fresh ``EvalAccumulator`` (nothing read back per batch), its ``compute()`` and ONE more
        device-to-host copy of three numbers: the predictions that differ from ``clean_pred``, the summed confidence and the summed
        sigma.  Returns the card and the predictions (on the device)."""
        acc = EvalAccumulator(len(self.config.data.class_names))
        self.model.eval()
        with torch.no_grad():
            for lo in range(0, order.numel(), batch_size):
                sel = order[lo:lo + batch_size]
                outputs = self.model(store.corrupt(sel, name, seed=seed, param=param))
                acc.update(outputs, store.labels.index_select(0, sel), store.severities.index_select(0, sel))
        m = acc.compute()
        if acc.device.type == 'cuda':
            rec = {k: acc._rec[k][:acc.n] for k in ('pred', 'probs', 'uncertainty')}
        else:
            rec = {k: torch.from_numpy(v) for k, v in acc._cpu_arrays().items() if k in ('pred', 'probs', 'uncertainty')}
        pred = rec['pred']
        flips = (pred != clean_pred).sum() if clean_pred is not None else torch.zeros((), dtype=torch.int64, device=pred.device)
        sigma = rec['uncertainty'].double().sum() if acc._has_uncertainty else torch.zeros((), dtype=torch.float64, device=pred.device)
        flips, conf, sigma = torch.stack([flips.double(), rec['probs'].max(dim=1).values.double().sum(), sigma]).cpu().tolist()
        card = {k: m[k] for k in self.CORRUPTION_CARD}
        card.update(n=m['n'], correct=m['correct'], mean_confidence=conf / m['n'], flip_rate=flips / m['n'])
        if acc._has_uncertainty:
            card['mean_sigma'] = sigma / m['n']
        return card, pred

    def evaluate_corruptions(self, source=None, corruptions=None, severities=(1, 2, 3, 4, 5), seed: int = 0, baseline=None, params=None):
        """Extension (not in the reference): the corruption-robustness score card of Hendrycks & Dietterich (ICLR 2019) with the
        corruptions of ``rovit_hip.corrupt`` -- one card per (corruption, severity) cell, each one pass over ``source`` with the images
        corrupted on the device from the uint8 store (one launch per batch, two for ``contrast``).

        ``source``: a ``DeviceImageStore`` or a loader that carries one (default ``self.test_loader``; a loader without a store raises:
        build it with ``create_dataloaders(..., device_cache=True)``).  ``corruptions``: names (default all eleven); ``severities``: a
        subset of 1..5; ``params``: ``{name: {severity: value}}`` replaces entries of the severity table.  Returned dict: ``'clean'``,
        the card of the uncorrupted pass (``brightness`` at c = 0, which is the plain normalisation, so that the clean and the corrupted
        passes share a code path and a resolution); ``'cells'[name][severity]`` with ``accuracy``, ``macro_f1`` (per cent), ``mae``,
        ``brier_score``, ``ece``, ``mean_confidence``, ``mean_sigma`` when the model returns ``log_var``, ``n``, ``correct`` and
        ``flip_rate``, the share of rows whose predicted class differs from the clean pass's (both passes visit the same rows in the
        same order); ``'error'[name]``, the mean error (100 - accuracy, per cent) over the severities; ``'mean_corruption_error'``, the
        mean of those; ``'relative_error'[name]``, the same after subtracting the clean error.  ``baseline``: another call's result for
        the same cells adds ``'ce'[name]`` = sum_s E_s / sum_s E_s^baseline (None where the baseline made no error) and their mean
        ``'mce'``: Hendrycks's normalised numbers with the user's own baseline in AlexNet's place.  The table is printed and saved as
        ``corruption_results.txt`` and ``.json`` in ``config.paths.results_dir``."""
        from rovit_hip.corrupt import CORRUPTIONS, _resolve
        store, indices, batch_size = self._corruption_source(source)
        names = list(CORRUPTIONS if corruptions is None else corruptions)
        severities = [int(s) for s in severities]
        if not names or not severities:
            raise RovitHipError('evaluate_corruptions: no corruption or no severity to evaluate')
        table = {name: {s: _resolve(name, s, (params or {}).get(name, {}).get(s)) for s in severities} for name in names}
        order = store.upload_indices(indices)
        clean, clean_pred = self._corruption_cell(store, order, batch_size, 'brightness', 0.0, seed, None)
        result = {'clean': clean, 'severities': severities, 'cells': {}, 'error': {}, 'relative_error': {}}
        clean_error = 100.0 - clean['accuracy']
        for name in names:
            result['cells'][name] = {s: self._corruption_cell(store, order, batch_size, name, table[name][s], seed, clean_pred)[0] for s in severities}
            errors = [100.0 - result['cells'][name][s]['accuracy'] for s in severities]
            result['error'][name] = sum(errors) / len(errors)
            result['relative_error'][name] = result['error'][name] - clean_error
        result['mean_corruption_error'] = sum(result['error'].values()) / len(names)
        if baseline is not None:
            result['ce'] = {}
            for name in names:
                mine = sum(100.0 - result['cells'][name][s]['accuracy'] for s in severities)
                theirs = sum(100.0 - baseline['cells'][name][s]['accuracy'] for s in severities)
                result['ce'][name] = mine / theirs if theirs > 0 else None
            known = [v for v in result['ce'].values() if v is not None]
            result['mce'] = sum(known) / len(known) if known else None
        lines = self._corruption_lines(result)
        print('\n'.join(lines))
        results_dir = getattr(getattr(self.config, 'paths', None), 'results_dir', None)
        if results_dir is not None:
            import json
            results_dir = Path(results_dir)
            results_dir.mkdir(parents=True, exist_ok=True)
            (results_dir / 'corruption_results.txt').write_text('\n'.join(lines) + '\n', encoding='utf-8')
            (results_dir / 'corruption_results.json').write_text(json.dumps(result, indent=1) + '\n', encoding='utf-8')
            print(f"Results saved to {results_dir / 'corruption_results.txt'}")
        return result

    @staticmethod
    def _corruption_lines(result: Dict):
        """Rows are corruptions, columns severities, entries accuracy (per cent), with the mean sigma under each when present."""
        sev = result['severities']
        has_sigma = 'mean_sigma' in result['clean']
        lines = ['', 'Corruption robustness (accuracy %' + (', mean sigma below' if has_sigma else '') + '):',
                 f"{'Corruption':<18}" + ''.join(f'{"s=" + str(s):>9}' for s in sev) + f"{'Error':>9}" + (f"{'CE':>8}" if 'ce' in result else ''),
                 '-' * (27 + 9 * len(sev) + (8 if 'ce' in result else 0))]
        for name, cells in result['cells'].items():
            ce = result.get('ce', {}).get(name)
            lines.append(f'{name:<18}' + ''.join(f"{cells[s]['accuracy']:>9.2f}" for s in sev) + f"{result['error'][name]:>9.2f}"
                         + ('' if 'ce' not in result else (f'{ce:>8.3f}' if ce is not None else f"{'n/a':>8}")))
            if has_sigma:
                lines.append(f"{'':<18}" + ''.join(f"{cells[s]['mean_sigma']:>9.4f}" for s in sev))
        clean = result['clean']
        lines += ['-' * (27 + 9 * len(sev) + (8 if 'ce' in result else 0)),
                  f"{'clean':<18}{clean['accuracy']:>9.2f}" + (f"   (mean sigma {clean['mean_sigma']:.4f})" if has_sigma else ''),
                  f"{'Mean corruption error:':<28}{result['mean_corruption_error']:.2f}%"]
        if result.get('mce') is not None:
            lines.append(f"{'mCE against the baseline:':<28}{result['mce']:.3f}")
        return lines + ['']

    def _adversarial_batches(self, source):
        """A function that yields (images, class_labels, severity_labels) on the device, in the same order at every call: a
        ``DeviceImageStore`` (or a loader that carries one) is read through its plain normalisation, any other loader is iterated."""
        from rovit_hip.augment import DeviceImageStore
        source = self.test_loader if source is None else source
        if source is None:
            raise RovitHipError('evaluate_adversarial needs images: pass a loader of (images, class_labels, severity_labels) batches or a '
                                'DeviceImageStore')
        if isinstance(source, DeviceImageStore) or isinstance(getattr(source, 'store', None), DeviceImageStore):
            store, indices, batch_size = self._corruption_source(source)
            order = store.upload_indices(indices)

            def batches():
                for lo in range(0, order.numel(), batch_size):
                    sel = order[lo:lo + batch_size]
                    yield store.corrupt(sel, 'brightness', param=0.0), store.labels.index_select(0, sel), store.severities.index_select(0, sel)
            return batches
        if not hasattr(source, '__iter__') or iter(source) is source:
            raise RovitHipError('evaluate_adversarial: the source is visited once per cell, so it must be a loader or a list of batches, '
                                'not an iterator')

        def batches():
            for images, class_labels, severity_labels in source:
                yield images.to(self.device), class_labels.to(self.device), severity_labels.to(self.device)
        return batches

    def _adversarial_cell(self, batches, eps, attack_kw: Dict, targets, clean_pred):
        """One cell: one pass into a fresh ``EvalAccumulator`` over the images attacked against their true labels (``eps=None``: the
        clean pass, no attack), its ``compute()`` and ONE more device-to-host copy: the flips against ``clean_pred``, the summed
        confidence and sigma, and per severity target the summed and the largest move of a ``direction=+1`` and a ``direction=-1``
        attack of the same budget.  Returns the card and the predictions (on the device)."""
        from rovit_hip.attack import pgd_attack
        acc = EvalAccumulator(len(self.config.data.class_names))
        self.model.eval()
        moves = {name: None for name in targets} if eps is not None else {}
        row = 0
        for images, class_labels, severity_labels in batches():
            n = images.shape[0]
            ids = torch.arange(row, row + n, device=images.device)          # the row in the data set: a start never depends on the split
            row += n
            if eps is not None:
                x_adv = pgd_attack(self.model, images, class_labels, eps=eps, ids=ids, check_labels=False, **attack_kw)
                for name in moves:
                    part = []
                    for direction in (1, -1):
                        kw = dict(attack_kw, objective=name, direction=direction)
                        _, info = pgd_attack(self.model, images, None, eps=eps, ids=ids, return_info=True, **kw)
                        move = (info['value'] - info['value_clean']).double()          # both carry the direction: a gain is positive
                        part += [move.sum(), move.max()]
                    part = torch.stack(part)
                    old = moves[name]
                    moves[name] = part if old is None else torch.stack([old[0] + part[0], torch.maximum(old[1], part[1]),
                                                                        old[2] + part[2], torch.maximum(old[3], part[3])])
            else:
                x_adv = images
            with torch.no_grad():
                acc.update(self.model(x_adv), class_labels, severity_labels)
        m = acc.compute()
        if acc.device.type == 'cuda':
            rec = {k: acc._rec[k][:acc.n] for k in ('pred', 'probs', 'uncertainty')}
        else:
            rec = {k: torch.from_numpy(v) for k, v in acc._cpu_arrays().items() if k in ('pred', 'probs', 'uncertainty')}
        pred = rec['pred']
        flips = (pred != clean_pred).sum() if clean_pred is not None else torch.zeros((), dtype=torch.int64, device=pred.device)
        sigma = rec['uncertainty'].double().sum() if acc._has_uncertainty else torch.zeros((), dtype=torch.float64, device=pred.device)
        head = torch.stack([flips.double(), rec['probs'].max(dim=1).values.double().sum(), sigma])
        numbers = torch.cat([head] + [moves[name].to(head.device) for name in moves]).cpu().tolist()          # the one copy
        flips, conf, sigma = numbers[:3]
        card = {k: m[k] for k in self.CORRUPTION_CARD}
        card.update(n=m['n'], correct=m['correct'], mean_confidence=conf / m['n'], flip_rate=flips / m['n'])
        if acc._has_uncertainty:
            card['mean_sigma'] = sigma / m['n']
        if eps is not None:
            card['severity'] = {}
            for i, name in enumerate(moves):
                up_sum, up_max, down_sum, down_max = numbers[3 + 4 * i:7 + 4 * i]
                card['severity'][name] = {'mean_up': up_sum / m['n'], 'max_up': up_max, 'mean_down': down_sum / m['n'], 'max_down': down_max}
        return card, pred

    def evaluate_adversarial(self, source=None, eps=(1 / 255, 2 / 255, 4 / 255, 8 / 255), norm: str = 'linf', steps: int = 10,
                             objective: str = 'ce', severity_targets=('ordinal_severity',), seed: int = 0):
        """Extension (not in the reference): the worst-case counterpart of ``evaluate_corruptions`` -- a clean card once, then one
        card per radius ``eps`` (pixel units, image in [0, 1]) over the images attacked against their TRUE labels with
        ``rovit_hip.attack.pgd_attack`` (``norm``, ``steps``, ``objective`` 'ce' or 'margin', a random start drawn from ``seed`` and the
        image's row in the data set).

        ``source``: a loader or a list of (images, class_labels, severity_labels) batches that yields the same rows in the same order
        at every visit (default ``self.test_loader``), or a ``DeviceImageStore``.  Returned dict: ``'clean'``; ``'eps'``; ``'cells'``,
        one card per radius in the order given, with ``accuracy`` (the robust accuracy), ``macro_f1``, ``mae``, ``brier_score``,
        ``ece``, ``mean_confidence``, ``mean_sigma`` when the model returns ``log_var``, ``n``, ``correct``, ``flip_rate`` (the share
        of predictions that differ from the clean pass's) and ``'severity'[name]`` for every name of ``severity_targets`` the model's
        curriculum stage has: ``mean_up`` / ``max_up``, how far a ``direction=+1`` attack of the same budget on that output raises it
        (mean and largest over the images), and ``mean_down`` / ``max_down`` for ``direction=-1`` (how far it is lowered, positive
        numbers).  Every number is what THIS attack finds: robust accuracy is an upper bound on the true one, the moves lower bounds.
        Each cell makes one device-to-host copy beyond the accumulator's own.  The table is printed and saved as
        ``adversarial_results.txt`` and ``.json`` in ``config.paths.results_dir``."""
        from rovit_hip.attack import CLASS_OBJECTIVES, PGD
        from rovit_hip.gradcam import TARGETS
        what = 'evaluate_adversarial'
        try:
            radii = [e for e in eps]
        except TypeError:
            raise RovitHipError(f'{what}: eps must be a sequence of radii, got {eps!r}') from None
        if not radii:
            raise RovitHipError(f'{what}: no radius to evaluate')
        try:
            for e in radii:
                PGD(norm, e, steps, None, True, 1, seed)
        except RovitHipError as err:
            raise RovitHipError(f'{what}: {err}') from None
        if any(isinstance(e, torch.Tensor) for e in radii):
            raise RovitHipError(f'{what}: every radius must be a number')
        if objective not in CLASS_OBJECTIVES:
            raise RovitHipError(f'{what}: objective must be one of {list(CLASS_OBJECTIVES)}, got {objective!r}')
        if isinstance(severity_targets, str) or not all(isinstance(n, str) and n in TARGETS and n != 'class' for n in severity_targets):
            raise RovitHipError(f"{what}: severity_targets must be names out of {[n for n in TARGETS if n != 'class']}, got {severity_targets!r}")
        batches = self._adversarial_batches(source)
        targets = [n for n in dict.fromkeys(severity_targets) if TARGETS[n][1] <= self.model.curriculum_stage]
        attack_kw = {'objective': objective, 'norm': norm, 'steps': steps, 'seed': seed}
        clean, clean_pred = self._adversarial_cell(batches, None, attack_kw, targets, None)
        result = {'clean': clean, 'norm': norm, 'steps': steps, 'objective': objective, 'eps': [float(e) for e in radii], 'cells': []}
        for e in radii:
            card, _ = self._adversarial_cell(batches, float(e), attack_kw, targets, clean_pred)
            result['cells'].append(dict(card, eps=float(e)))
        lines = self._adversarial_lines(result)
        print('\n'.join(lines))
        results_dir = getattr(getattr(self.config, 'paths', None), 'results_dir', None)
        if results_dir is not None:
            import json
            results_dir = Path(results_dir)
            results_dir.mkdir(parents=True, exist_ok=True)
            (results_dir / 'adversarial_results.txt').write_text('\n'.join(lines) + '\n', encoding='utf-8')
            (results_dir / 'adversarial_results.json').write_text(json.dumps(result, indent=1) + '\n', encoding='utf-8')
            print(f"Results saved to {results_dir / 'adversarial_results.txt'}")
        return result

    @staticmethod
    def _adversarial_lines(result: Dict):
        """Rows are radii; columns robust accuracy, flip rate, MAE, ECE, mean sigma and, per severity target, mean (largest) move up and down."""
        has_sigma = 'mean_sigma' in result['clean']
        names = list(result['cells'][0].get('severity', {})) if result['cells'] else []
        unit = '255 eps' if result['norm'] == 'linf' else 'eps'
        head = f"{unit:<10}{'Accuracy':>10}{'Flips %':>9}{'MAE':>9}{'ECE':>9}" + (f"{'Sigma':>9}" if has_sigma else '')
        head += ''.join(f"{n + ' up':>26}{n + ' down':>26}" for n in names)
        lines = ['', f"Adversarial robustness ({result['norm']}, {result['steps']} steps, {result['objective']}):", head, '-' * len(head)]

        def row(label, c):
            text = f"{label:<10}{c['accuracy']:>10.2f}{100.0 * c['flip_rate']:>9.2f}{c['mae']:>9.4f}{c['ece']:>9.4f}"
            text += f"{c['mean_sigma']:>9.4f}" if has_sigma else ''
            for n in names:
                s = c.get('severity', {}).get(n)
                text += ''.join(f"{f'{s[a]:.4f} ({s[b]:.4f})':>26}" for a, b in (('mean_up', 'max_up'), ('mean_down', 'max_down'))) if s else ''
            return text
        lines.append(row('clean', result['clean']))
        for c in result['cells']:
            lines.append(row(f"{c['eps'] * 255:g}" if result['norm'] == 'linf' else f"{c['eps']:g}", c))
        return lines + ['']

    @staticmethod
    def _summary(metrics: Dict, rho_label: str):
        rows = (('Accuracy:', f"{metrics['accuracy']:.2f}%"), ('Macro F1:', f"{metrics['macro_f1']:.2f}%"), ('MAE:', f"{metrics['mae']:.4f}"),
                (rho_label, f"{metrics['spearman_rho']:.4f}"), ('Brier Score:', f"{metrics['brier_score']:.4f}"),
                ('ECE:', f"{metrics['ece']:.4f}"), ('FPS:', f"{metrics['fps']:.1f}"), ('Parameters:', f"{metrics['params']:,}"))
        ci = metrics.get('confidence_intervals')
        if ci is None:
            return [f'{label:<16}{value}' for label, value in rows]
        # the bootstrap column: standard error and percentile interval, in the digits of the value beside it
        keys = ('accuracy', 'macro_f1', 'mae', 'spearman_rho', 'brier_score', 'ece', None, None)
        column = ['' if k is None else (f"± {ci[k]['se']:.2f} [{ci[k]['lo']:.2f}, {ci[k]['hi']:.2f}]" if k in ('accuracy', 'macro_f1') else
                                        f"± {ci[k]['se']:.4f} [{ci[k]['lo']:.4f}, {ci[k]['hi']:.4f}]") for k in keys]
        return [f'{label:<16}{value:<12}{extra}'.rstrip() for (label, value), extra in zip(rows, column)]

    @staticmethod
    def _calibration_card(acc: EvalAccumulator, m: Dict) -> Dict:
        """What calibration is judged by, of one accumulator: its own ``compute()`` (``m``) and a ``calibrate()`` on its rows, whose
        diagnostics at T = 1 and s = 1 describe the record as it is and whose refitted sigma scale says how far sigma is from calibrated."""
        fit = acc.calibrate()
        d = fit.diagnostics
        return {'nll': d['nll'], 'ece': m['ece'], 'brier_score': m['brier_score'], 'gaussian_nll': d['gaussian_nll'], 'coverage': d['coverage'],
                'levels': d['levels'], 'sigma_scale_refit': fit.sigma_scale}

    @staticmethod
    def _calibration_lines(metrics: Dict):
        """Before / after lines of NLL, ECE, Brier score, Gaussian NLL and the refitted sigma scale, then the interval coverage."""
        cal = metrics.get('calibration')
        if cal is None:
            return []
        num = lambda v, spec: format(v, spec) if v is not None else format('n/a', f'>{spec.split(".")[0].lstrip(">")}')
        scale = 'none' if cal['sigma_scale'] is None else f"{cal['sigma_scale']:.4f}"
        lines = [f"Calibration (temperature {cal['temperature']:.4f}, sigma scale {scale}, {cal['status']}):",
                 f"{'':<10}{'NLL':>10}{'ECE':>10}{'Brier':>10}{'Gauss. NLL':>12}{'s refit':>10}", '-' * 62]
        for side in ('before', 'after'):
            c = cal[side]
            lines.append(f"{side:<10}{c['nll']:>10.4f}{c['ece']:>10.4f}{c['brier_score']:>10.4f}{num(c['gaussian_nll'], '>12.4f')}"
                         f"{num(c['sigma_scale_refit'], '>10.4f')}")
        if cal['before']['coverage'] is not None:
            lines.append('Interval coverage (nominal / before / after):')
            for side, values in (('nominal', cal['before']['levels']), ('before', cal['before']['coverage']), ('after', cal['after']['coverage'])):
                lines.append(f'{side:<10}' + ''.join(f'{v:>7.3f}' for v in values))
        return lines + ['']

    @staticmethod
    def _conformal_lines(metrics: Dict):
        """One line per score and level: the target 1 - alpha, the observed coverage, and the mean set size with the share of
        singletons (class scores) or the mean interval width (severity scores)."""
        card = metrics.get('conformal')
        if card is None:
            return []
        lines = ['Conformal prediction:', f"{'Score':<16}{'Target':>8}{'Coverage':>10}{'Mean size':>11}{'Singletons':>12}{'Mean width':>12}", '-' * 69]
        for score, entry in card['scores'].items():
            for alpha, lv in entry['levels'].items():
                size = f"{lv['mean_set_size']:>11.3f}{lv['singleton_rate']:>12.3f}" if 'mean_set_size' in lv else f"{'':>23}"
                width = f"{lv['mean_width']:>12.4f}" if 'mean_width' in lv else ''
                lines.append(f"{score:<16}{1.0 - alpha:>8.3f}{lv['coverage']:>10.4f}{size}{width}".rstrip())
        return lines + ['']

    @staticmethod
    def _selective_lines(metrics: Dict):
        """One line per score and risk: AURC, E-AURC, normalized E-AURC and the risk left at 80 % and 90 % coverage (the curve points
        whose actual coverage k_p / n is the first at or above them)."""
        sel = metrics.get('selective')
        if sel is None:
            return []
        cov = sel['coverages']
        at = [min(int((cov < c - 1e-12).sum()), len(cov) - 1) for c in (0.8, 0.9)]
        lines = ['Selective prediction:', f"{'Score':<24}{'Risk':<12}{'AURC':>10}{'E-AURC':>10}{'Norm.':>8}{'Risk@80%':>10}{'Risk@90%':>10}", '-' * 84]
        for score, entry in sel['scores'].items():
            for risk in sel['risks']:
                e = entry[risk]
                lines.append(f"{score:<24}{risk:<12}{e['aurc']:>10.4f}{e['e_aurc']:>10.4f}{e['normalized']:>8.3f}"
                             f"{e['curve'][at[0]]:>10.4f}{e['curve'][at[1]]:>10.4f}")
        return lines + ['']

    @staticmethod
    def _knn_lines(metrics: Dict):
        """The neighbour vote beside the heads: its accuracy and severity MAE, and its agreement with the classification head."""
        card = metrics.get('knn')
        if card is None:
            return []
        num = lambda v, spec: 'n/a' if v is None else format(v, spec)
        return [f"Nearest neighbours (k = {card['k']}):", f"{'Vote accuracy:':<22}{num(card['accuracy'], '.2f')}%",
                f"{'Vote severity MAE:':<22}{num(card['severity_mae'], '.4f')}", f"{'Agreement with head:':<22}{num(card['agreement'], '.4f')}", '']

    @staticmethod
    def _laplace_lines(metrics: Dict):
        """The prior precisions with their status, then NLL, ECE, Brier score and accuracy before and after the probit adjustment."""
        card = metrics.get('laplace')
        if card is None:
            return []
        mu = '' if card['prior_precision_mu'] is None else f", mu head {card['prior_precision_mu']:.4g} ({card['status_mu']})"
        lines = [f"Laplace approximation (n = {card['n']}, prior precision {card['prior_precision']:.4g} ({card['status']}){mu}):",
                 f"{'':<10}{'NLL':>10}{'ECE':>10}{'Brier':>10}{'Accuracy':>10}", '-' * 50]
        for side in ('before', 'after'):
            c = card[side]
            lines.append(f"{side:<10}{c['nll']:>10.4f}{c['ece']:>10.4f}{c['brier_score']:>10.4f}{c['accuracy']:>9.2f}%")
        return lines + ['']

    def _print_results(self, metrics: Dict) -> None:
        print('\n'.join(['', RULE, 'Evaluation Results', RULE] + self._summary(metrics, 'Spearman rho:') + [RULE, '']))
        if 'selective' in metrics:
            print('\n'.join(self._selective_lines(metrics)))
        if 'calibration' in metrics:
            print('\n'.join(self._calibration_lines(metrics)))
        if 'conformal' in metrics:
            print('\n'.join(self._conformal_lines(metrics)))
        if 'knn' in metrics:
            print('\n'.join(self._knn_lines(metrics)))
        if 'laplace' in metrics:
            print('\n'.join(self._laplace_lines(metrics)))
        print('Per-Class Metrics:')
        print(f"{'Class':<20} {'Precision':<12} {'Recall':<12} {'F1-Score':<12} {'Support':<10}")
        print('-' * 70)
        for name, c in metrics['per_class'].items():
            print(f"{name:<20} {c['precision']:>10.2f}%  {c['recall']:>10.2f}%  {c['f1']:>10.2f}%  {c['support']:>8}")
        print()

    def _save_results(self, metrics: Dict) -> None:
        results_dir = getattr(getattr(self.config, 'paths', None), 'results_dir', None)
        if results_dir is None:
            return
        results_dir = Path(results_dir)
        results_dir.mkdir(parents=True, exist_ok=True)
        lines = ['RoViT-KAN Evaluation Results', RULE, ''] + self._summary(metrics, "Spearman's rho:") + ['', 'Per-Class Metrics:', '-' * 60]
        for name, c in metrics['per_class'].items():
            lines += [f'{name}:', f"  Precision: {c['precision']:.2f}%", f"  Recall:    {c['recall']:.2f}%", f"  F1-Score:  {c['f1']:.2f}%",
                      f"  Support:   {c['support']}", '']
        lines += self._selective_lines(metrics) + self._calibration_lines(metrics) + self._conformal_lines(metrics) + self._knn_lines(metrics) + self._laplace_lines(metrics)
        path = results_dir / 'evaluation_results.txt'
        path.write_text('\n'.join(lines) + '\n', encoding='utf-8')
        print(f'Results saved to {path}')


def load_model_for_evaluation(checkpoint_path: Path, config, device, use_ema=None):
    """``use_ema``: None loads the checkpoint's ``'ema_state_dict'`` (the averaged weights of an ``ema_decay`` run) when it has one and
    ``'model_state_dict'`` otherwise; True insists on the average (KeyError without one); False loads the raw weights."""
    from models.rovit_kan import RoViTKAN
    mc = config.model
    model = RoViTKAN(embed_dim=mc.embed_dim, hidden_dim=mc.hidden_dim, num_classes=config.data.num_classes, kan_layers=mc.kan_layers,
                     kan_num_knots=mc.kan_num_knots, kan_degree=mc.kan_degree, dropout=mc.dropout, pretrained=False)
    checkpoint = torch.load(checkpoint_path, map_location=device, weights_only=False)
    if use_ema and 'ema_state_dict' not in checkpoint:
        raise KeyError(f'{checkpoint_path} holds no ema_state_dict (use_ema=True)')
    averaged = use_ema is not False and 'ema_state_dict' in checkpoint
    state = checkpoint['ema_state_dict' if averaged else 'model_state_dict']
    model.kan_module.resize_grid_like(state, prefix='kan_module.')          # a checkpoint saved after a KAN grid extension
    model.load_state_dict(state)
    model.to(device)
    model.eval()
    print(f'Model loaded from {checkpoint_path}')
    print(f"Checkpoint epoch: {checkpoint['epoch']}")
    return model
