"""bench.py --dump-outputs: a fixed particle sample by particle number (CPU, with a stand-in engine) and, on the GPU,
two runs with the same arguments leave the same outputs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_bench():
    spec = importlib.util.spec_from_file_location("fpx_bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class _FakeEngine:
    """download(first, count) as Engine.download returns it: float64 / int32 per particle, xmass1 as (nspec, n)."""

    def download(self, first, count):
        i = np.arange(first, first + count)
        return {"xtra1": i * 0.5, "itra1": (i % 7).astype(np.int32), "xmass1": np.stack([i * 1.0, i * 2.0])}


def _load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_sample_is_fixed_and_keyed_by_particle_number(tmp_path):
    bench = _load_bench()
    nper, base = 10**6, 500
    grids = {"gridunc": np.arange(6, dtype=np.float32).reshape(2, 3)}
    for d in ("a", "b"):
        bench.dump_outputs(_FakeEngine(), str(tmp_path / d), nper, base, grids)
    a, b = _load_dir(tmp_path / "a"), _load_dir(tmp_path / "b")
    assert sorted(a) == ["gridunc", "itra1", "particle_number", "xmass1", "xtra1"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    pn = a["particle_number"]
    n = bench.DUMP_BLOCKS * bench.DUMP_BLOCK
    assert pn.shape == (n,) and np.all(np.diff(pn) > 0) and pn[0] >= base and pn[-1] < base + nper
    assert np.array_equal(a["xtra1"], (pn - base) * 0.5) and np.array_equal(a["itra1"], (pn - base) % 7)
    assert a["xmass1"].shape == (2, n) and np.array_equal(a["xmass1"][1], (pn - base) * 2.0)
    assert np.array_equal(a["gridunc"], grids["gridunc"])
    # fewer particles than the sample: all of them
    bench.dump_outputs(_FakeEngine(), str(tmp_path / "small"), 1000, 0)
    assert np.array_equal(_load_dir(tmp_path / "small")["particle_number"], np.arange(1000))


def test_bench_rejects_zero_steps(monkeypatch):
    bench = _load_bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


@pytest.mark.gpu
def test_bench_dump_outputs_repeat(built, tmp_path):
    """Two plain runs with the same arguments (config 4: particles and the concentration grid; more particles than the
    sample) report the steps asked for and write the same outputs; a plain run has no CPU baseline and no counter pass."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    lines, dumps = [], []
    for k in range(2):
        d = tmp_path / f"out{k}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", "4", "--particles", "3e5", "--steps", "3", "--warmup", "1",
               "--dump-outputs", str(d)]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
        dumps.append(_load_dir(d))
    for line in lines:
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and "cpu_baseline" not in line and "valu" not in line["roofline"]
    a, b = dumps
    assert sorted(a) == sorted(b) and {"xtra1", "ytra1", "ztra1", "itra1", "particle_number", "gridunc", "drygridunc"} <= set(a)
    assert a["particle_number"].size == 32 * 8192
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert np.median(a["itra1"]) > 0          # the particles were stepped
    for k in a:
        if k in ("gridunc", "drygridunc"):       # sums of float atomics: the order may differ between runs
            np.testing.assert_allclose(a[k], b[k], rtol=1e-9, atol=0, err_msg=k)
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
