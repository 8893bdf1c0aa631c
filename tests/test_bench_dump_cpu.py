"""CPU tests of bench.py's --dump-outputs helpers: the parameter sample is seeded and follows the parameters' logical order
whatever their memory layout, and what is written is float32 / float64 within the 64 MB budget."""
import importlib.util
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench_under_test', os.path.join(REPO, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_parameter_sample_is_seeded_and_follows_the_logical_order():
    B = _bench()
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.Linear(7, 4))
    m[0].weight.data = m[0].weight.data.to(memory_format=torch.channels_last)
    assert not m[0].weight.is_contiguous()
    flat = np.concatenate([p.detach().numpy().ravel(order='C') for p in m.parameters()])
    n = 1000
    s = B.param_sample(m, n)
    assert s.dtype == np.float32 and s.shape == (n,)
    np.testing.assert_array_equal(s, flat[np.sort(np.random.RandomState(0).randint(0, flat.size, size=n))])
    np.testing.assert_array_equal(s, B.param_sample(m, n))
    assert not np.array_equal(s, B.param_sample(m, n, seed=1))


def test_dump_outputs_writes_float32_or_float64_within_the_budget(tmp_path):
    B = _bench()
    out = str(tmp_path / 'dump')
    B.dump_outputs(out, {'loss': np.array([1.5], np.float32), 'sequences': np.arange(5).astype(np.float64),
                         'half': np.ones(3, np.float16), 'ids': np.arange(4)})
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert sorted(got) == ['half', 'ids', 'loss', 'sequences']
    assert got['sequences'].dtype == np.float64 and got['sequences'].tolist() == [0, 1, 2, 3, 4]
    assert all(got[k].dtype == np.float32 for k in ('loss', 'half', 'ids'))
    # the training dump: one loss value and the parameter sample, in float32
    assert 4 * (1 + B.DUMP_PARAM_SAMPLE) <= 64 * 2 ** 20
