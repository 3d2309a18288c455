"""Drop-in for the reference's explainability/kan_viz.py (KANVisualizer, :9-215).

The reference's four methods draw with matplotlib and seaborn, which this package does not depend on.  This class keeps their names (they
raise, naming the data method to call) and provides the arrays each of them plots -- plus what none of them shows: what the edges do on
data (``edge_attribution``: rovit_hip.kan_stats, csrc/kan_stats.hip)."""
import numpy as np
import torch

from rovit_hip import kan_stats

_PLOTS = 'KANVisualizer.{}: needs matplotlib and seaborn, which this package does not depend on (plots are out of scope); ' \
         'use {} and draw the arrays with your own plotting code'


class KANVisualizer:

    def __init__(self):
        pass

    # ---- the reference's plotting methods ----
    def plot_spline_activations(self, kan_module, save_path=None, num_samples=5):
        raise NotImplementedError(_PLOTS.format('plot_spline_activations', 'spline_activations()'))

    def plot_severity_trajectory(self, kan_module, features_batch, labels_batch, class_names, save_path=None):
        raise NotImplementedError(_PLOTS.format('plot_severity_trajectory', 'severity_trajectory()'))

    def plot_severity_distribution(self, predictions, labels, class_names, save_path=None):
        raise NotImplementedError(_PLOTS.format('plot_severity_distribution', 'the arrays you passed (it only groups predictions by label)'))

    def plot_spline_weights_heatmap(self, kan_module, save_path=None):
        raise NotImplementedError(_PLOTS.format('plot_spline_weights_heatmap', 'spline_weights_heatmap()'))

    # ---- the data behind them ----
    def spline_activations(self, kan_module, num_samples: int = 5, num_points: int = 100):
        """Per layer, the edges kan_viz.py:29-38 plots -- (i, i) for i < min(num_samples, in, out) -- as ``{'edges': [(i, j), ...],
        'x': (P,), 'y': (n_edges, P)}``, from one ``activation_curves`` call per layer."""
        out = []
        for layer in kan_module.kan_layers:
            k = min(num_samples, min(layer.in_features, layer.out_features))
            xs, ys = layer.activation_curves(num_points)
            out.append({'edges': [(i, i) for i in range(k)], 'x': xs, 'y': np.stack([ys[i, i] for i in range(k)]) if k else ys[:0, 0]})
        return out

    def severity_trajectory(self, kan_module, features, labels):
        """What kan_viz.py:61-92 scatters: the mean activation of every sample at every stage of the head, ``{'mean_activations': [(B,)
        per stage], 'labels': (B,)}``."""
        kan_module.eval()
        with torch.no_grad():
            acts = kan_module.get_activation_trajectory(features)
            means = torch.stack([a.mean(dim=1) for a in acts]).cpu().numpy()
        return {'mean_activations': [m for m in means], 'labels': torch.as_tensor(labels).cpu().numpy()}

    def spline_weights_heatmap(self, kan_module):
        """Per layer the (in, out) array kan_viz.py:191-197 draws: the spline weights averaged over the basis index."""
        return [w.mean(dim=2).cpu().numpy() for w in kan_module.get_spline_weights()]

    def edge_attribution(self, model_or_kan, features_or_loader, chunk: int = 256):
        """Per-edge statistics on data and pykan's attribution scores.  With a RoViTKAN: images or a loader (``model.kan_attribution``);
        with a KANSeverityModule: a (N, in) feature tensor or an iterable of them."""
        if hasattr(model_or_kan, 'kan_module'):
            return model_or_kan.kan_attribution(features_or_loader, chunk)
        acc = kan_stats.KANEdgeStats(model_or_kan)
        for f in ([features_or_loader] if isinstance(features_or_loader, torch.Tensor) else features_or_loader):
            acc.update(f[0] if isinstance(f, (tuple, list)) else f)
        stats = acc.compute()
        return {'stats': stats, **kan_stats.kan_attribution(stats)}
