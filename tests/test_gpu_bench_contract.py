"""bench.py's one JSON line: the driver's contract fields and `roofline` of a plain run (and what it writes with
--dump-outputs); with --full also `cpu_baseline` and under `also` the north_star's other shapes -- on reduced
sizes (headline launch, end-to-end files) so that the test takes a minute or two."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    return env


def _plain(dump_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--streams", "256", "--bits", "512",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(dump_dir)],
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_bench_line_and_its_outputs(gpu, tmp_path):
    """A plain run: the contract's fields, exactly --steps timed steps after --warmup, nothing of --full; and
    --dump-outputs writes the last timed step's probabilities, the same on a second run with the same arguments."""
    d = _plain(tmp_path / "a")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["unit"] == "bits/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["n_gpus"] == 1
    assert d["steps"] == 3 and d["warmup"] == 1 and d["config"]["streams_per_gpu"] == 256
    assert d["config"]["bits_per_step"] == 256 * 512 and d["config"]["total_bits"] == 3 * 256 * 512
    assert d["ms_per_step"] > 0 and abs(d["value"] - 256 * 512 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert d["roofline"]["kernel_ms_avg"] <= d["ms_per_step"] * 1.02
    assert "cpu_baseline" not in d and "also" not in d and "kernel_ms_min" not in d["roofline"]
    assert sorted(os.listdir(tmp_path / "a")) == ["p.npy"]
    p = np.load(tmp_path / "a" / "p.npy")
    assert p.dtype == np.float32 and p.shape == (256, 512)
    assert np.all(np.isfinite(p)) and np.all((p > 0) & (p < 1)) and len(np.unique(p)) > 1000
    _plain(tmp_path / "b")
    assert np.array_equal(np.load(tmp_path / "b" / "p.npy").view(np.uint32), p.view(np.uint32))


def test_bench_line_carries_the_contract(gpu):
    env = _env()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--streams", "1024", "--bits", "256", "--steps", "4",
                        "--cpu-sample-bits", "100000", "--e2e-bytes", "3000", "--e2e-many-bytes", "3000", "--decode-bytes", "300",
                        "--decode-streams", "8", "--also-streams-div", "4"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "fracs", "also", "tail_summary"):
        assert k in d, k
    assert d["unit"] == "bits/s" and d["n_gpus"] == 1 and d["steps"] == 4 and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert "configs[1]" in d["config"]["workload"] and "model" not in d["config"]
    kernels = {"synth3", "stock_held", "stock_real", "stock_fresh", "stock_S1", "single_S1", "indirect", "lstm"}
    whole = {"e2e_S1", "e2e_S1_mixers", "e2e_S64"}   # the run-ahead compressor on real files (scripts/bench_e2e.py)
    assert set(d["also"]) - {"e2e_decode"} == kernels | whole | {"real_trace"}
    assert list(d)[-1] == "tail_summary" and list(d).index("fracs") < list(d).index("also")
    assert set(d["fracs"]) >= kernels | {"single", "real_trace"} and d["tail_summary"]["fracs"] == d["fracs"]
    assert set(d["tail_summary"]["e2e"]) >= whole
    rt = d["also"]["real_trace"]   # the stock kernel on the reference's recorded mixer boundary
    assert "error" not in rt, rt
    assert rt["unit"] == "bits/s" and rt["value"] > 1e7 and rt["stream0_first_window_equals_reference"] is True
    assert rt["roofline"]["kernel"] == "gmx_stock_kernel" and 0 < rt["roofline"]["frac"] < 1
    for name in whole:
        e = d["also"][name]
        assert "error" not in e, (name, e)
        assert e["unit"] == "bits/s" and e["value"] > 1e4 and e["identical_to_stock"] is True
        assert e["config"]["streams"] == (64 if name == "e2e_S64" else 1) and e["cpu_baseline"]["value"] > 1e4
        # `value` is the whole process, exec to exit (like the reference CLI it is set against); the coding loops alone are faster
        assert e["value"] <= e["value_coding_loops"] and e["seconds"] >= e["in_process_seconds"] >= e["coding_loops_seconds"]
        assert abs(e["vs_cpu"] - e["value"] / e["cpu_baseline"]["value"]) < 1e-9
    assert d["also"]["e2e_S64"]["predictors_built_side_by_side"] is True
    for name, e in [("headline", d)] + [(k, d["also"][k]) for k in sorted(kernels)]:
        assert "error" not in e, (name, e)
        ro = e["roofline"]
        assert ro["bound"] == "hbm" and ro["peak"] == 8000.0 and ro["unit"] == "GB/s"
        assert abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-12 and 0 < ro["frac"] < 1
        if name not in ("indirect", "lstm"):  # (the producers' entries come from their own scripts: other units)
            assert ro["bytes_per_launch"] == ro["algorithmic_bytes_per_bit"] * e["config"]["streams_per_gpu"] * \
                e["config"]["bits_per_stream_per_step"]
        # the live HIP-event figure and the wall clock tell the same story
        assert ro["kernel_ms_avg"] <= e["ms_per_step"] * 1.02
        assert e["value"] > 0 and e["cpu_baseline"]["cores"] == 1 and e["cpu_baseline"]["kind"] in ("reference", "port")
        assert e["cpu_baseline"]["value"] > 1e4
    assert d["also"]["synth3"]["config"]["n_inputs"] == 256 and d["also"]["synth3"]["config"]["mixers"] == "24/8/1"
    assert d["also"]["stock_S1"]["config"]["streams_per_gpu"] == 1
    assert d["also"]["indirect"]["unit"] == "bits/s" and d["also"]["indirect"]["roofline"]["kernel"] == "gmx_indirect_kernel"
    assert d["also"]["lstm"]["unit"] == "bytes/s" and d["also"]["lstm"]["roofline"]["kernel"] == "gmx_lstm_kernel"
