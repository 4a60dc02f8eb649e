"""`bench.py --dump-outputs DIR` (CPU): what the last timed iteration handed back - loss terms, trained weights - lands in DIR/<name>.npy as
float32 / float64, an array above the per-array cap as the same seeded sample on every run, the whole dump within its byte budget."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _trainer(n_d, n_g, seed=0):
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(d_opt=types.SimpleNamespace(theta=torch.randn(n_d, generator=g)),
                                 g_opt=types.SimpleNamespace(theta=torch.randn(n_g, generator=g)))


def test_dump_writes_losses_and_weights(tmp_path):
    tr = _trainer(1000, 300)
    d_out = {'cost': torch.tensor(1.25), 'gp': torch.tensor(0.5, dtype=torch.float64), 'acc_real': torch.tensor(3, dtype=torch.int32),
             'grads': {'w': torch.ones(3)}}
    bench.dump_outputs(str(tmp_path), d_out, {'cost': torch.tensor(-2.0)}, tr)
    names = sorted(os.listdir(tmp_path))
    assert names == ['critic_params.npy', 'd_acc_real.npy', 'd_cost.npy', 'd_gp.npy', 'g_cost.npy', 'generator_params.npy']
    for n in names:
        assert np.load(tmp_path / n).dtype in (np.float32, np.float64), n
    assert np.load(tmp_path / 'd_gp.npy').dtype == np.float64 and float(np.load(tmp_path / 'd_gp.npy')) == 0.5
    assert float(np.load(tmp_path / 'd_cost.npy')) == 1.25 and float(np.load(tmp_path / 'g_cost.npy')) == -2.0
    assert np.array_equal(np.load(tmp_path / 'critic_params.npy'), tr.d_opt.theta.numpy())
    assert np.array_equal(np.load(tmp_path / 'generator_params.npy'), tr.g_opt.theta.numpy())


def test_large_arrays_are_the_same_seeded_sample_every_run(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_MAX_ELEMENTS', 64)
    tr = _trainer(1000, 50)
    bench.dump_outputs(str(tmp_path / 'a'), {}, None, tr)
    bench.dump_outputs(str(tmp_path / 'b'), {}, None, tr)
    a = np.load(tmp_path / 'a' / 'critic_params.npy')
    assert a.shape == (64,) and np.array_equal(a, np.load(tmp_path / 'b' / 'critic_params.npy'))
    assert set(a.tolist()) <= set(tr.d_opt.theta.numpy().tolist())
    assert np.load(tmp_path / 'a' / 'generator_params.npy').shape == (50,)        # under the cap: written whole


def test_dump_refuses_to_exceed_its_byte_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 1000)
    import pytest
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path), {}, None, _trainer(1000, 10))
