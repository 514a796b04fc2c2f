"""bench.py's measurement helpers that need no GPU: the clock / power sampler degrades to `available: false` instead of
failing a run (no device, no librocm_smi64 device, no sysfs), percentiles, and the per-step grouping of launch samples
(a step of the wide fp16 paths is several launches of different sizes: they are summed step by step before the median)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402


def test_sampler_without_a_device_says_so():
    for bdf in (None, "", "0000:ff:1f.7"):
        with bench.ClockSampler(bdf) as c:
            pass
        s = c.summary()
        assert s["available"] is False and s["pci_bus_id"] == (bdf or None)


def test_percentiles():
    p = bench.pctl([1.0, 2.0, 3.0, 4.0, 100.0])
    assert p["latency_ms_p50"] == 3.0 and p["latency_samples"] == 5 and 4.0 < p["latency_ms_p95"] <= 100.0


def test_launch_samples_are_grouped_by_step():
    class Ctx:
        def prof_samples(self, kernel):
            assert kernel == "vec_scan_f16"
            return np.array([0.2, 1.0, 1.0, 0.2, 1.1, 1.1, 0.2], dtype=np.float32)  # 2 whole steps of 3 launches + a stray one

    per_step = bench.scan_step_samples(Ctx(), "vec_scan_f16", 3)
    assert np.allclose(per_step, [2.2, 2.4])
    assert bench.scan_step_samples(Ctx(), "vec_scan_f16", 8).size == 0


def _recorded_runs():
    import json
    root = Path(__file__).resolve().parent.parent / "profiles"
    return [json.loads(p.read_text()) for p in sorted(root.glob("r0[5-9]_bench_all_configs*.json"))]


def test_headline_line_fits(capfd, tmp_path):
    """Round 5's line grew to 24.9 KB and the driver's bounded tail of stdout no longer held a whole JSON object.  The LAST
    stdout line is now a compact object under HEADLINE_BUDGET; the full record goes to the details file and stderr."""
    import json
    runs = _recorded_runs()
    assert runs, "no recorded bench run under profiles/"
    for rec in runs:
        line = bench.headline_line(rec, "bench_details.json")
        text = json.dumps(line, separators=(",", ":"))
        assert len(text) < bench.HEADLINE_BUDGET == 4096
        for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                    "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
            assert key in line, key
        assert line["config"]["workload"] and "model" not in line["config"]
        for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
            assert key in line["roofline"], key
        assert abs(line["roofline"]["frac"] - rec["roofline"]["frac"]) < 1e-4
        assert abs(line["value"] - rec["value"]) / rec["value"] < 1e-5
        for key in ("value", "unit", "cores", "kind", "sample"):
            assert key in line["cpu_baseline"], key
        for leg in ("c2", "c3", "c4", "c5_shard"):
            assert set(line["configs"][leg]) == {"value", "ms_per_step", "latency_ms_p50", "roofline"}
    # what a driver that keeps the last 4 096 bytes of stdout would parse: emit() after 30 KB of other output
    rec = runs[-1]
    print("x" * 30000)
    bench.emit(rec, str(tmp_path / "d.json"))
    captured = capfd.readouterr()
    tail = captured.out[-4096:]
    parsed = json.loads(tail[tail.index("\n") + 1:] if "\n" in tail.rstrip("\n") else tail)
    assert parsed["roofline"]["frac"] and parsed["cpu_baseline"]["value"] and parsed["details"] == "d.json"
    assert json.loads((tmp_path / "d.json").read_text())["configs"]["c4"]["bm25_only"]["value"] == rec["configs"]["c4"]["bm25_only"]["value"]
    assert json.loads(captured.err.strip().splitlines()[-1]) == rec  # the long form went to stderr, whole


def test_headline_line_sheds_before_it_overflows():
    """A record with pathologically many legs still yields a line under the budget with the contract keys intact."""
    rec = _recorded_runs()[-1]
    rec = dict(rec, configs={f"leg{i}": rec["configs"]["c2"] for i in range(60)})
    line = bench.headline_line(rec)
    import json
    assert len(json.dumps(line, separators=(",", ":"))) < bench.HEADLINE_BUDGET and "roofline" in line and "cpu_baseline" in line


def test_plain_run_is_the_default(monkeypatch):
    """`bench.py --gpus 1 --steps N --warmup W` is the lean run: everything beyond the headline figure is `--full`'s."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse_args()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, "")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == "out"


def test_headline_line_of_a_plain_run():
    """A plain run measures no latency, checks nothing against the oracle and times no CPU baseline: its line carries the
    contract keys and leaves the absent parts out instead of reporting them as null."""
    import json
    rec = _recorded_runs()[-1]
    full_only = ("latency_ms_p50", "latency_ms_p95", "latency_samples", "latency_definition", "parity_check",
                 "latency_ms_p50_host_api", "latency_ms_p95_host_api", "cpu_baseline", "two_stage_exact", "configs")
    rec = {k: v for k, v in rec.items() if k not in full_only}
    line = bench.headline_line(rec)
    assert len(json.dumps(line, separators=(",", ":"))) < bench.HEADLINE_BUDGET
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "roofline"):
        assert key in line, key
    assert line["ms_per_step"] == round(rec["ms_per_step"], 4) and line["value"] == float(f"{rec['value']:.6g}")
    assert not set(full_only) & set(line)


def test_dumped_outputs_are_what_the_caller_received(tmp_path):
    """--dump-outputs: one .npy per array, float32 kept bit for bit, ids and counts as float64 (exact below 2**53)."""
    ids = np.array([[79_999_999, 0, 123_456_789]], dtype=np.uint64)
    dist = np.array([[0.25, np.float32(1) / 3, 1.5]], dtype=np.float32)
    cnt = np.array([3], dtype=np.uint32)
    bench.write_outputs(tmp_path / "out", ids=ids, distances=dist, counts=cnt)
    got = {p.stem: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert set(got) == {"ids", "distances", "counts"}
    assert got["ids"].dtype == np.float64 and got["ids"].astype(np.uint64).tolist() == ids.tolist()
    assert got["distances"].dtype == np.float32 and np.array_equal(got["distances"].view(np.uint32), dist.view(np.uint32))
    assert got["counts"].dtype == np.float64 and got["counts"].tolist() == [3.0]


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_answer(ctx, tmp_path):
    """A plain run times exactly --steps steps and writes the last one's answer: the direct search of the same seeded query
    over the same seeded rows returns the same ids and distance bits."""
    import json
    import subprocess

    import oramacore_amd as oa

    root = Path(__file__).resolve().parent.parent
    steps, warmup = 7, 2
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--workload", "c2", "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "out"), "--details-file", str(tmp_path / "d.json")],
                       capture_output=True, text=True, timeout=600, cwd=str(root))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["warmup"] == warmup and line["value"] > 0 and line["ms_per_step"] > 0
    assert "latency_ms_p50" not in line and "cpu_baseline" not in line and "configs" not in line
    # the HIP events of the timed region: the single-query fp32 scan is one launch per step, so exactly `steps` launches were
    # recorded there (not the warm-up, nothing behind it) and the roofline's median is over those steps
    rf = json.loads((tmp_path / "d.json").read_text())["roofline"]
    assert rf["launches"] == steps and rf["steps_in_median"] == steps and rf["of_which_behind_the_timed_region"] == 0, rf
    rows, dim, k, qb = bench.WORKLOADS["c2"][:4]
    q = np.random.default_rng(0xBEEF).standard_normal(((warmup + steps) * qb, dim)).astype(np.float32)[-qb:]
    st = oa.EmbeddingFieldStorage(ctx, dimensions=dim, reserve_rows=rows, dtype=oa.DTYPE_F32)
    st.fill_synthetic(rows, seed=0xC0FFEE, first_doc_id=0)
    ids, dist, cnt = st.storage_search(q, k)
    st.close()
    got = {p.stem: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert np.array_equal(got["ids"], ids.astype(np.float64))
    assert np.array_equal(got["distances"].view(np.uint32), dist.view(np.uint32))
    assert np.array_equal(got["counts"], cnt.astype(np.float64))
