"""A plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: the headline loop only (no roofline, CPU baseline, host-fed loop,
A/Bs or GP unit - those need --full), K timed steps in the record, and the last step's loss terms and weights in DIR as finite .npy arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_run_times_the_loop_only_and_dumps_its_outputs(tmp_path):
    e = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--dump-outputs', str(out)], env=e, capture_output=True, text=True, timeout=580)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec['steps'] == 3 and rec['warmup'] == 1 and rec['ms_per_step'] > 0 and rec['value'] > 0
    assert rec['unit'] == 'img/s' and rec['higher_is_better'] is True and rec['dtype'] == 'f32'
    assert rec['config']['loss_sane'] is True
    for k in ('roofline', 'cpu_baseline', 'gp_unit', 'host_feed', 'fp32_mfma_only', 'critic_step_ab', 'step'):
        assert rec[k] is None, k
    names = sorted(os.listdir(out))
    for n in ('critic_params.npy', 'generator_params.npy', 'd_cost.npy', 'g_cost.npy'):
        assert n in names, names
    total = 0
    for n in names:
        a = np.load(out / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        total += a.nbytes
    assert total <= 64 << 20
    assert float(np.load(out / 'd_cost.npy')) == pytest.approx(rec['config']['last_d_cost'], rel=1e-6)
