"""bench.py on one GPU: a plain run times the headline and prints its line, and nothing else runs; --full adds the legs
that take runs of their own (here on a reduced grid, with the CPU baseline and the per-configuration lines left out)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ('roofline_hbm', 'parity', 'sustained', 'unplanned', 'mask_sensitivity', 'contracted', 'configs', 'end_to_end',
        'cpu_baseline')


def _line(*extra):
    env = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT', 'XINV_FORCE_DEVICE', 'XINV_DIST_FORCE_INIT'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--ny', '360', '--nx', '720', '--steps', '2',
                          '--warmup', '1', '--sweeps', '40'] + list(extra),
                         capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_is_the_headline_alone():
    d = _line()
    assert d['value'] > 0 and d['ms_per_step'] > 0 and d['unit'] == 'point-sweeps/s'
    assert d['dtype'] == 'f64' and d['higher_is_better'] is True and d['steps'] == 2 and d['warmup'] == 1
    assert [k for k in LEGS if k in d] == []
    assert d['roofline']['parity_bitwise'] is None and d['roofline']['hbm_frac'] is None


def test_bench_full_runs_the_legs():
    d = _line('--full', '--no-cpu', '--no-configs')
    assert d['value'] > 0 and d['ms_per_step'] > 0
    assert d['parity']['bitwise'] and d['parity']['loop_equal'] and d['roofline']['parity_bitwise'] is True
    assert d['roofline_hbm']['parity_bitwise_10_sweeps'] and d['roofline']['hbm_frac'] > 0
    assert [k for k in LEGS if k in d] == ['roofline_hbm', 'parity']
