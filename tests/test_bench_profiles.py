"""CPU tests of bench.py's handling of the committed counter summaries (profiles/*_pmc_traffic*.json, *_sq_counters*.json): a
summary counts only while its per-kernel source stamp equals the tree's (silently stale figures)."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_kernel_source_hash_names_every_profiled_kernel():
    from fluidx12_amd.build import kernel_source_hash
    for k in ("k_jacobi_strip4o", "k_jacobi_strip4x", "k_jacobi_strip4t", "k_jacobi_strip4q", "k_jacobi_strip3c", "k_jacobi_strip3h", "k_jacobi_block2", "k_jacobi_blockg", "k_advect_lds", "k_divergence_v4",
              "k_project_v4", "k_freeze_dense", "k_freeze_tiles", "k_jacobi_strip2u", "k_raymarch_light", "k_raymarch_view"):
        h = kernel_source_hash(k)
        assert h and len(h) == 16, k
    assert kernel_source_hash("k_no_such_kernel") is None
    # two kernels of one file share a stamp, kernels of different files do not
    assert kernel_source_hash("k_freeze_dense") == kernel_source_hash("k_freeze_tiles") != kernel_source_hash("k_jacobi_strip3c")


def test_stale_summary_is_flagged_and_not_used(tmp_path, monkeypatch):
    from fluidx12_amd.build import kernel_source_hash
    b = load_bench()
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(b, "ROOT", str(tmp_path))
    k = "k_jacobi_strip3c"
    fresh = {"grid": 256, "iters": 40, "storage": "fp32", "kernels": {k: {"traffic": 2.5e8, "dispatches": 60, "source_hash": kernel_source_hash(k)}}}
    (prof / "r09a_pmc_traffic.json").write_text(json.dumps(fresh))
    assert b.pmc_traffic(k, 256, 40, "fp32") == (2.5e8, "r09a_pmc_traffic.json", False)
    assert b.step_traffic(256, 40, "fp32")[2] == []
    stale = dict(fresh, kernels={k: dict(fresh["kernels"][k], source_hash="0" * 16)})
    (prof / "r09b_pmc_traffic.json").write_text(json.dumps(stale))            # newer file, taken on another version of the kernel
    assert b.pmc_traffic(k, 256, 40, "fp32") == (2.5e8, "r09b_pmc_traffic.json", True)
    assert b.step_traffic(256, 40, "fp32")[2] == [k]
    assert b.pmc_traffic(k, 256, 40, "fp32", "faithful") is None             # another workload: no summary at all
    sq = {"kernels": {k: {"limiter": "issuing", "source_hash": "0" * 16}}}
    (prof / "r09b_sq_counters.json").write_text(json.dumps(sq))
    assert b.limiter_note(k) is None
    sq["kernels"][k]["source_hash"] = kernel_source_hash(k)
    (prof / "r09c_sq_counters.json").write_text(json.dumps(sq))
    assert b.limiter_note(k) == "issuing (r09c_sq_counters.json)"


def test_bench_line_carries_both_truths_and_certifies_multi_rank_runs():
    """VERDICT round 5, items 4 and 7 (source-level: no GPU here; the GPU tests assert the values): the line has `value_cold` and
    `warm_device` beside `value`, the developed plume its own stage times, the default flags are SURVEY 8(d)'s 32 + 100, the device
    wake-up is opt-in, and every N > 1 line carries `multi_rank_parity` with a non-zero exit code on a mismatch"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    for key in ('"value_cold"', '"warm_device"', '"stage_ms_per_step"', '"multi_rank_parity"', '"rccl"'):
        assert key in src, key
    assert 'add_argument("--warmup", type=int, default=32)' in src and 'add_argument("--steps", type=int, default=100)' in src
    assert 'add_argument("--preheat", action="store_true"' in src and "args.preheat and not args.no_preheat" in src
    assert "raise SystemExit(parity_rc)" in src


def test_committed_summaries_of_the_headline_kernels_are_fresh():
    """the summaries bench.py's default line cites must have been taken on the committed kernels"""
    b = load_bench()
    for kernel, grid, iters, storage in (("k_jacobi_strip4o", 256, 40, "fp32"), ("k_jacobi_block2", 128, 40, "fp32"), ("k_jacobi_strip4x", 512, 80, "fp32"), ("k_jacobi_strip4t", 384, 40, "fp32")):
        t = b.pmc_traffic(kernel, grid, iters, storage)
        assert t is not None and t[2] is False, (kernel, t)


def test_dump_outputs_samples_large_fields_the_same_way_every_time(tmp_path):
    """--dump-outputs (bench.dump_outputs): fields over the 64 MB budget are written as one seeded sample of cells, the same cells of every
    field; small fields whole.  Here on host arrays standing in for a context's downloads."""
    import numpy as np
    from fluidx12_amd import capi
    b = load_bench()

    class FakeFluid:
        def __init__(self, shape):
            Z, Y, X = shape
            n = Z * Y * X
            c = np.arange(n, dtype=np.float32)
            self.fields = {capi.FIELD_VELOCITY: np.stack([c, c + 0.25, c + 0.5]).reshape(3, Z, Y, X),
                           capi.FIELD_COLOR: np.stack([c, c + 1, c + 2, c + 3], axis=-1).reshape(Z, Y, X, 4), capi.FIELD_PRESSURE: c.reshape(Z, Y, X)}

        def download(self, field):
            return self.fields[field].copy()

    small = FakeFluid((8, 16, 16))
    assert b.dump_outputs(small, str(tmp_path / "small")) == ["color", "pressure", "velocity"]
    for field, name in ((capi.FIELD_VELOCITY, "velocity"), (capi.FIELD_COLOR, "color"), (capi.FIELD_PRESSURE, "pressure")):
        assert np.array_equal(np.load(tmp_path / "small" / (name + ".npy")), small.fields[field])

    big = FakeFluid((128, 128, 128))                       # 8 floats per cell x 2 M cells = 67 MB: sampled
    for run in ("a", "b"):
        b.dump_outputs(big, str(tmp_path / run))
    total = 0
    for name in ("velocity", "color", "pressure"):
        x, y = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert x.dtype == np.float32 and len(x) == b.DUMP_SAMPLE_CELLS and np.array_equal(x, y)
        total += x.nbytes
    assert total <= b.DUMP_BUDGET_BYTES
    cells = np.load(tmp_path / "a" / "pressure.npy")         # the stand-in's pressure is the flat cell index
    assert (np.diff(cells) > 0).all() and cells[-1] < 128 ** 3
    assert np.array_equal(np.load(tmp_path / "a" / "velocity.npy"), np.stack([cells, cells + 0.25, cells + 0.5], axis=1))
    assert np.array_equal(np.load(tmp_path / "a" / "color.npy"), np.stack([cells, cells + 1, cells + 2, cells + 3], axis=1))
