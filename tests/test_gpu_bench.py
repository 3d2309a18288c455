"""bench.py on the GPU: a plain run prints the headline line and nothing the headline figure does not need; --full adds the
roofline, fp32-mode and backbone-only sections after the timed steps (its CPU baseline, a minute of host time, is left out here)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
FULL_ONLY = ('roofline', 'roofline_attn', 'roofline_mlp', 'roofline_kan', 'roofline_patch', 'fp32_mode', 'backbone_only', 'cpu_baseline')


def _line(extra, timeout):
    env = {k: v for k, v in os.environ.items()
           if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT', 'ROVIT_FORCE_DIST')}
    r = subprocess.run([sys.executable, BENCH, '--gpus', '1', '--steps', '3', '--warmup', '2'] + extra,
                       capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_line_only():
    d = _line([], 300)
    assert d['metric'] == 'images/sec fwd+bwd, DeiT-Tiny+KAN 224^2, batch 256 per GPU'
    assert d['unit'] == 'images/sec' and d['higher_is_better'] is True and d['dtype'] == 'bf16'
    assert d['n_gpus'] == 1 and d['steps'] == 3 and d['warmup'] == 2
    assert d['value'] > 0 and d['ms_per_step'] > 0
    assert abs(d['value'] - 256 / (d['ms_per_step'] * 1e-3)) <= 1e-3 * d['value']
    assert d['final_loss'] == d['final_loss']
    assert not set(FULL_ONLY) & set(d)
    assert 'attention_half_us_per_block' not in d['config'] and 'allreduce' not in d['config']


def test_full_run_adds_the_kernel_sections():
    d = _line(['--full', '--no-cpu-baseline'], 600)
    assert d['unit'] == 'images/sec' and d['value'] > 0
    for k in FULL_ONLY[:-1]:
        assert k in d, k
    assert 'cpu_baseline' not in d
    assert d['roofline']['avg_us'] > 0 and d['fp32_mode']['ms_per_forward'] > 0 and d['backbone_only']['fwd_bwd_ms'] > 0
    assert 0 < d['config']['attention_half_frac_of_hbm_roofline']
