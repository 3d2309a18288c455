"""bench.py --dump-outputs writes what the last timed step computed as float32 .npy files within 64 MB, sampling the
largest arrays at fixed positions; --steps below 1 is refused.  No GPU: dump_outputs is fed a CPU model and outputs."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _fake_step(rows):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Linear(16, 4))
    x = torch.randn(rows, 8)
    out = {'cls_logits': model(x), 'features': x * 2, 'mu': None}
    loss = out['cls_logits'].square().mean()
    loss.backward()
    return out, loss, model


def test_dump_writes_outputs_loss_params_and_grads_whole_when_small(tmp_path):
    out, loss, model = _fake_step(32)
    _bench().dump_outputs(str(tmp_path), out, loss, model)
    assert sorted(os.listdir(tmp_path)) == ['cls_logits.npy', 'features.npy', 'grads.npy', 'loss.npy', 'params.npy']
    d = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(a.dtype == np.float32 for a in d.values())
    np.testing.assert_array_equal(d['cls_logits'], out['cls_logits'].detach().numpy())
    np.testing.assert_array_equal(d['loss'], [float(loss)])
    params = list(model.parameters())
    np.testing.assert_array_equal(d['params'], torch.cat([p.detach().reshape(-1) for p in params]).numpy())
    np.testing.assert_array_equal(d['grads'], torch.cat([p.grad.reshape(-1) for p in params]).numpy())


def test_dump_stays_within_budget_with_a_fixed_sample(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 4096)
    out, loss, model = _fake_step(512)                    # features: 4096 floats, four times the budget alone
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), out, loss, model)
    total = sum(np.load(tmp_path / 'a' / f).size * 4 for f in os.listdir(tmp_path / 'a'))
    assert total <= 4096
    np.testing.assert_array_equal(np.load(tmp_path / 'a' / 'loss.npy'), [float(loss)])      # small arrays stay whole
    for f in os.listdir(tmp_path / 'a'):
        np.testing.assert_array_equal(np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f))
    feats = np.load(tmp_path / 'a' / 'features.npy')
    assert 0 < feats.size < out['features'].numel()
    assert np.isin(feats, out['features'].numpy().reshape(-1)).all()


def test_steps_below_one_is_refused():
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, BENCH, '--gpus', '1', '--steps', '0'], capture_output=True, text=True, env=env, timeout=180)
    assert r.returncode != 0 and '--steps must be >= 1' in r.stderr
