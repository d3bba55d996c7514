"""bench.py as the measurement contract uses it: a plain run prints the headline line only, `--steps` sets the timed steps,
and `--dump-outputs DIR` writes what the last timed step computed -- checked here against the C oracle on the same seeded set."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', *extra],
                       capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')][-1])


@pytest.mark.timeout(900)
def test_plain_run_is_the_headline_and_dumps_the_last_step(built, dev, tmp_path):
    from boxinstseg_amd import synthetic
    from tests.helpers import grad_report, oracle_path
    steps, warmup, n_sets = 7, 3, 4
    res = _bench('--steps', str(steps), '--warmup', str(warmup), '--sets', str(n_sets), '--dump-outputs', str(tmp_path))
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert key in res, key
    assert res['steps'] == steps and res['warmup'] == warmup and res['ms_per_step'] > 0 and res['value'] > 0
    assert abs(res['value'] - 2e3 / res['ms_per_step']) <= 1e-6 * res['value']       # 2 images per step
    for key in ('roofline', 'cpu_baseline', 'parity', 'extras', 'kernels'):             # what only --full measures
        assert key not in res, key
    assert sorted(os.listdir(tmp_path)) == ['grad_mask_logits.npy', 'loss_pairwise.npy', 'loss_prj.npy']
    d = synthetic.cfg2(seed=(warmup + steps - 1) % n_sets)                              # rank 0's set i has seed i
    ref = oracle_path(d, want_targets=False)
    lp, lw = float(np.load(tmp_path / 'loss_prj.npy')), float(np.load(tmp_path / 'loss_pairwise.npy'))
    assert abs(lp - ref['loss_prj']) <= 1e-4 * abs(ref['loss_prj'])
    assert abs(lw - ref['loss_pairwise']) <= 1e-4 * abs(ref['loss_pairwise'])
    grad = np.load(tmp_path / 'grad_mask_logits.npy')
    assert grad.dtype == np.float32 and grad.shape == d['mask_logits'].shape
    g_err, _ = grad_report(grad[:, 0], ref['grad'], d['mask_logits'][:, 0])
    assert g_err <= 1e-4, g_err
