"""Paired comparison of two trained models on one test set: the significance column the reference's ablation summary lacks.

The reference's ``experiments/ablation.py`` (``get_component_importance``, the "delta Acc" column of its summary) subtracts point estimates of
two arms.  ``compare_models`` scores both models over the same loader into two ``EvalAccumulator``s and hands them to
``rovit_hip.evaluation.paired_bootstrap``: per metric a, b, b - a, the percentile interval of the difference over resamples that draw the
same rows for both models, the two-sided bootstrap p-value, and McNemar's exact test on the discordant predictions.  One device-to-host
copy for the whole comparison.  The loader must yield the same rows in the same order on both passes (a test loader does not shuffle);
differing class labels are refused."""
from typing import Dict

import torch

from rovit_hip.evaluation import EvalAccumulator, paired_bootstrap

RULE = '=' * 100
ROWS = (('Accuracy (%)', 'accuracy', 2), ('Macro F1 (%)', 'macro_f1', 2), ('Weighted F1 (%)', 'weighted_f1', 2), ('MAE', 'mae', 4),
        ('Spearman rho', 'spearman_rho', 4), ('Brier Score', 'brier_score', 4), ('ECE', 'ece', 4))


def _collect(model, loader, num_classes: int, device) -> EvalAccumulator:
    acc = EvalAccumulator(num_classes)
    model.to(device).eval()
    with torch.no_grad():
        for images, class_labels, severity_labels in loader:
            acc.update(model(images.to(device)), class_labels, severity_labels)
    return acc


def format_table(result: Dict, name_a: str = 'a', name_b: str = 'b') -> str:
    level = round(100 * result['confidence'])
    lines = [RULE, f"Paired comparison ({result['num_resamples']} resamples, seed {result['seed']}): {name_b} - {name_a}", RULE,
             f"{'Metric':<18}{name_a:>12}{name_b:>12}{'delta':>12}   {f'{level}% interval':<26}{'p':>8}", '-' * 100]
    for label, key, digits in ROWS:
        r = result[key]
        interval = f"[{r['lo']:+.{digits}f}, {r['hi']:+.{digits}f}]"
        lines.append(f"{label:<18}{r['a']:>12.{digits}f}{r['b']:>12.{digits}f}{r['diff']:>+12.{digits}f}   {interval:<26}{r['p_value']:>8.4f}")
    mc = result['mcnemar']
    lines += ['-' * 100, f"McNemar exact: {name_a} right / {name_b} wrong {mc['b01']}, {name_a} wrong / {name_b} right {mc['b10']}, "
                         f"p = {mc['p_value']:.4g}", RULE]
    return '\n'.join(lines)


def compare_models(model_a, model_b, test_loader, config, device, num_resamples: int = 1000, seed: int = 0, confidence: float = 0.95,
                   stratified: bool = False) -> Dict:
    """Score ``model_a`` and ``model_b`` over ``test_loader`` and print the paired table: metric, a, b, delta, interval, p, McNemar.
    Returns ``paired_bootstrap``'s dict."""
    device = torch.device(device)
    C = len(config.data.class_names)
    acc_a, acc_b = _collect(model_a, test_loader, C, device), _collect(model_b, test_loader, C, device)
    result = paired_bootstrap(acc_a, acc_b, num_resamples=num_resamples, seed=seed, confidence=confidence, stratified=stratified)
    print(format_table(result))
    return result
