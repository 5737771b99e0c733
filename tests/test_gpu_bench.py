"""bench.py's plain line and --dump-outputs on the GPU: a plain run times exactly --steps steps and measures nothing beside them
(the CPU baseline, `warm_device`, the render leg and the developed plume need --full); the dumped fields are the ones the last timed
step left, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fluidx12_amd as fx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_line_is_lean_and_dumps_the_fields_of_the_last_timed_step(tmp_path):
    G, steps, warmup = 64, 6, 2
    lines = []
    for run in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--grid", str(G), "--steps", str(steps),
                              "--warmup", str(warmup), "--dump-outputs", str(tmp_path / run)],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        ls = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(ls) == 1, out.stdout
        lines.append(json.loads(ls[0]))
    d = lines[0]
    assert d["steps"] == steps and d["warmup"] == warmup and d["n_gpus"] == 1
    assert d["unit"] == "voxel-updates/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(G ** 3 / (d["ms_per_step"] * 1e-3))
    assert not any(k in d for k in ("cpu_baseline", "render", "developed_plume")) and d["warm_device"] is None
    # the same frames on a context of this process: 2 warm-up + 6 timed steps from the zero state
    f = fx.Fluid()
    assert f.Init(1920, 1080, (G, G, G))
    for k in range(warmup + steps):
        f.UpdateFrame(2.0 / G, k % 3)
        f.Simulate(k % 3)
    f.Synchronize()
    want = {"velocity": f.download(fx.FIELD_VELOCITY), "color": f.download(fx.FIELD_COLOR), "pressure": f.download(fx.FIELD_PRESSURE)}
    f.Release()
    assert sorted(os.listdir(tmp_path / "a")) == ["color.npy", "pressure.npy", "velocity.npy"]
    for name, w in want.items():
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == w.shape and w.any(), name
        assert np.array_equal(a, b) and np.array_equal(a, w), name
