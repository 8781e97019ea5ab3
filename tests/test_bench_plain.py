"""bench.py's plain run and its options: a plain run measures the headline figure alone (no CPU
baseline, no kernel timings, one window of exactly --steps steps), --full brings back the rest,
and --dump-outputs writes the engine's outputs of the last timed step as float32 .npy files that
repeat from run to run."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', *argv])
    return bench.parse()


def test_plain_run_measures_the_headline_alone(monkeypatch):
    a = _parse(monkeypatch, '--gpus', '1', '--steps', '7', '--warmup', '2')
    assert not a.full and a.no_cpu_baseline and a.no_kernel_timing
    assert a.min_seconds == 0 and a.steps == 7 and a.dump_outputs is None
    # an explicit window length is still honoured (A/B scripts)
    assert _parse(monkeypatch, '--min-seconds', '1').min_seconds == 1


def test_full_run_keeps_the_baseline_the_windows_and_the_kernel_table(monkeypatch):
    a = _parse(monkeypatch, '--full')
    assert a.full and not a.no_cpu_baseline and not a.no_kernel_timing and a.min_seconds == 2.0
    a = _parse(monkeypatch, '--full', '--no-cpu-baseline', '--no-kernel-timing', '--min-seconds', '0')
    assert a.no_cpu_baseline and a.no_kernel_timing and a.min_seconds == 0
    # the dumped step is step --steps of the run: one window, whatever else is measured
    assert _parse(monkeypatch, '--full', '--dump-outputs', 'd').min_seconds == 0


def _fake_engine(torch, overlap):
    def slot(k):
        g = torch.Generator().manual_seed(k)
        return dict(z=torch.rand(3, 4, 8, generator=g), actions=torch.randint(0, 6, (2, 4), dtype=torch.int32),
                    rewards=torch.rand(2, 4), terminals=torch.zeros(2, 4, dtype=torch.uint8),
                    returns=torch.rand(2, 4))
    slots = [slot(k) for k in range(2 if overlap else 1)]
    return types.SimpleNamespace(params=torch.arange(10, dtype=torch.float32), grads=torch.ones(10),
                                 loss=torch.zeros(4), overlap=overlap, slot=lambda k: slots[k]), slots


@pytest.mark.parametrize('overlap', [False, True])
def test_dump_outputs_writes_float32_arrays(tmp_path, overlap):
    torch = pytest.importorskip('torch')
    import bench
    eng, slots = _fake_engine(torch, overlap)
    bench.dump_outputs(eng, str(tmp_path / 'out'))
    names = sorted(os.listdir(tmp_path / 'out'))
    want = ['grads', 'loss', 'params'] + [f'slot{k}_{n}' for k in range(len(slots))
                                          for n in ('actions', 'returns', 'rewards', 'terminals', 'z')]
    assert names == sorted(w + '.npy' for w in want)
    for n in names:
        assert np.load(tmp_path / 'out' / n).dtype == np.float32
    assert np.array_equal(np.load(tmp_path / 'out' / 'params.npy'), np.arange(10, dtype=np.float32))
    k = len(slots) - 1
    assert np.array_equal(np.load(tmp_path / 'out' / f'slot{k}_z.npy'), slots[k]['z'].numpy())
    assert np.array_equal(np.load(tmp_path / 'out' / f'slot{k}_actions.npy'), slots[k]['actions'].numpy())


def test_dump_outputs_samples_what_is_over_the_bound(tmp_path, monkeypatch):
    torch = pytest.importorskip('torch')
    import bench
    eng, _ = _fake_engine(torch, False)
    monkeypatch.setattr(bench, 'DUMP_BYTES', 4 * 8 * 6)          # 8 arrays: 6 elements each
    for d in ('a', 'b'):
        bench.dump_outputs(eng, str(tmp_path / d))
    total = 0
    for n in os.listdir(tmp_path / 'a'):
        a, b = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert a.size <= 6 and np.array_equal(a, b)               # a fixed sample
        total += a.nbytes
    assert total <= 4 * 8 * 6
    p = np.load(tmp_path / 'a' / 'params.npy')
    assert p.size == 6 and np.all(np.diff(p) > 0)                 # elements of params, in order


def _bench(*argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--envs', '8', '--frames', '64',
                        *argv], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_bench_times_its_steps_and_repeats_its_outputs(tmp_path):
    """Two plain runs with the same arguments: one window of exactly --steps steps, no baseline or
    kernel table, and every dumped array after the last step is the same in both (same inputs, same
    seeds, and the engine sums in a fixed order: test_bench_shape_is_deterministic)."""
    lines = []
    for d in ('a', 'b'):
        lines.append(_bench('--steps', '3', '--warmup', '2', '--dump-outputs', str(tmp_path / d)))
    ln = lines[0]
    assert ln['steps'] == 3 and ln['warmup'] == 2 and ln['timing']['windows'] == 1
    assert ln['timing']['steps_per_window'] == 3
    assert ln['cpu_baseline'] is None and ln['roofline'] is None and ln['kernels'] == {}
    assert ln['unit'] == 'env-steps/s' and ln['higher_is_better'] is True and ln['dtype'] == 'fp32'
    assert ln['ms_per_step'] > 0
    assert ln['value'] == pytest.approx(8 * 5 / (ln['ms_per_step'] * 1e-3), rel=1e-3)
    assert ln['params_finite']
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == sorted(os.listdir(tmp_path / 'b')) and 'params.npy' in names and 'slot1_z.npy' in names
    size = 0
    for n in names:
        a, b = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all()
        size += a.nbytes
        assert np.array_equal(a, b), n
    assert size <= 64 << 20
    p = np.load(tmp_path / 'a' / 'params.npy')
    assert p.size > 600000 and np.abs(p).max() > 0


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_full_bench_brings_the_kernel_table_back():
    ln = _bench('--full', '--no-cpu-baseline', '--min-seconds', '0', '--steps', '3', '--warmup', '2')
    assert ln['roofline'] and ln['kernels'] and ln['cpu_baseline'] is None
    assert ln['roofline']['kernel'] in ln['kernels']
