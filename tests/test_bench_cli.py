"""bench.py's command line on a box without a GPU (`--stub-step`: the whole control flow on CPU tensors): a plain run times the
steps and nothing else, `--full` adds the side legs, `--dump-outputs` writes the last step's outputs reproducibly."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    out = subprocess.run([sys.executable, BENCH, '--gpus', '1', '--stub-step'] + list(argv), env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_line_and_reproducible_dump(tmp_path):
    """--steps sets the number of timed steps, the line carries the contract's keys, and two runs with the same arguments dump the same arrays"""
    recs = [_bench('--steps', '4', '--warmup', '1', '--dump-outputs', str(tmp_path / d)) for d in ('a', 'b')]
    rec = recs[0]
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert key in rec, key
    assert rec['steps'] == 4 and rec['warmup'] == 1 and rec['ms_per_step'] > 0
    # value = utterances of the 4 timed steps / their time
    assert abs(rec['value'] - rec['config']['global_batch'] * 1000.0 / rec['ms_per_step']) <= 1e-6 * rec['value']
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['loss.npy', 'wav_pred.npy'] and names == sorted(os.listdir(tmp_path / 'b'))
    for n in names:
        a, b = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert a.dtype == np.float32 and np.isfinite(a).all()
        assert np.array_equal(a, b), n
    assert np.load(tmp_path / 'a' / 'wav_pred.npy').shape == (rec['config']['batch_per_gpu'], 16, 9)


def test_dump_sample_is_bounded_and_fixed(tmp_path):
    """an output above the budget is written as the same seeded sample every time; a small one next to it stays whole"""
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    big = np.arange(20 * 1000 * 1000, dtype=np.float64).reshape(4, -1)       # 160 MB
    small = np.ones((3, 5), dtype=np.float32)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), {'big': big, 'small': small})
    a, b = np.load(tmp_path / 'a' / 'big.npy'), np.load(tmp_path / 'b' / 'big.npy')
    assert a.dtype == np.float64 and np.array_equal(a, b)
    assert a.ndim == 1 and 1000 * 1000 < a.size < big.size and (np.diff(a) > 0).all()      # distinct elements, in their order in the array
    assert np.array_equal(np.load(tmp_path / 'a' / 'small.npy'), small)
    total = sum(os.path.getsize(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a'))
    assert total <= 64 * 1000 * 1000
