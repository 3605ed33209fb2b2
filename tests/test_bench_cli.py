"""
bench.py's command line: --dump-outputs writes what the last timed step computed (the arrays a caller of the timed path
receives), equal inputs from run to run; a plain run carries no --full sections.
"""
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_step_outputs_by_workload(bench, tmp_path):
    T, M = 3, 6
    rec = types.SimpleNamespace(fulldims=(2, 3), hyperparams={
        "lengthscale": [[1.0 + i, 2.0 + i] for i in range(2 * T)],      # two steps of T iterations each
        "variance": [float(i) for i in range(2 * T)], "noise": [0.1 * i for i in range(2 * T)], "inducing_points": []})
    res = torch.arange(2 * M, dtype=torch.float64).reshape(1, 2, M)
    out = bench.step_outputs("c2", res, 1, rec, T)
    assert sorted(out) == ["lengthscale", "mean", "noise", "sd", "variance"]
    assert out["mean"].shape == (2, 3) and out["sd"][0, 0] == M
    assert out["lengthscale"].shape == (T, 2) and out["variance"].tolist() == [3.0, 4.0, 5.0]
    res2 = torch.cat([res, res + 100]).reshape(2, 2, M)
    out2 = bench.step_outputs("c1", res2, 2, rec, T)
    assert out2["mean"].shape == (2, 2, 3) and out2["mean"][1, 0, 0] == 100
    cube = np.ones((4, 4, 2))
    assert sorted(bench.step_outputs("c3", (cube, cube), 1, None, T)) == ["mean", "sd"]
    assert bench.step_outputs("c2full", (cube.ravel(), cube.ravel(), 1.5), 1, None, 0)["nll"].tolist() == [1.5]
    hyp = {"variance": np.ones(T), "lengthscale": np.ones((T, 3)), "noise": np.ones(T), "loss": np.ones(T)}
    assert sorted(bench.step_outputs("c3cube", (cube.ravel(), cube.ravel(), hyp), 1, None, T)) == \
        ["lengthscale", "loss", "mean", "noise", "sd", "variance"]

    bench.dump_outputs(str(tmp_path / "d"), dict(out, single=np.ones(4, dtype=np.float32)))
    assert np.load(str(tmp_path / "d" / "mean.npy")).dtype == np.float64
    assert np.load(str(tmp_path / "d" / "single.npy")).dtype == np.float32
    assert_allclose(np.load(str(tmp_path / "d" / "lengthscale.npy")), out["lengthscale"], rtol=0)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1)})
    assert not os.path.exists(str(tmp_path / "big"))


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_dump_outputs_c1(ensure_built, tmp_path):
    """Config C1 at 3 Adam iterations: two plain runs dump the same posterior and hyper-parameter history."""
    args = ["--gpus", "1", "--workload", "c1", "--iterations", "3", "--steps", "2", "--warmup", "0", "--dump-outputs"]
    lines = [_bench(args + [str(tmp_path / name)]) for name in ("a", "b")]
    for line in lines:
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "grid-points/s"
        assert line["cpu_baseline"] is None and "extra" not in line and "stages" not in line["roofline"]
    for name, shape in (("mean", (128, 128)), ("sd", (128, 128)), ("lengthscale", (3, 2)), ("variance", (3,)),
                        ("noise", (3,))):
        a, b = np.load(str(tmp_path / "a" / (name + ".npy"))), np.load(str(tmp_path / "b" / (name + ".npy")))
        assert a.shape == shape and a.dtype == np.float64 and np.isfinite(a).all()
        assert_allclose(a, b, rtol=1e-12, atol=1e-14)
    assert (np.load(str(tmp_path / "a" / "sd.npy")) > 0).all()
