"""bench.py's plain run, --full and --dump-outputs: the dumped arrays are what the timed query
returned (checked against a second engine on the same seeded stream), --steps sets the number
of timed steps, and only --full carries the measurements that take runs of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Stats:
    def stats(self):
        return np.array([3, 4], np.int64), np.array([1, 2], np.int64)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_samples_a_large_skyline_the_same_way_every_time(tmp_path, monkeypatch):
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 1000)
    g = 5000
    ids = torch.arange(g + 7, dtype=torch.int64) * 3 + 11       # rows past g are not output
    org = (torch.arange(g + 7, dtype=torch.int32) % 16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), _Stats(), g, ids, org, 0, 1)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == ["local_sizes", "skyline_ids", "skyline_origins", "skyline_sample_index", "skyline_size",
                         "survivors"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a[k], b[k])
    idx = a["skyline_sample_index"].astype(np.int64)
    assert 0 < len(idx) <= 1000 and idx.max() < g and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(a["skyline_ids"], idx * 3 + 11)
    np.testing.assert_array_equal(a["skyline_origins"], idx % 16)
    assert a["skyline_size"].tolist() == [g]
    assert a["local_sizes"].tolist() == [3, 4] and a["survivors"].tolist() == [1, 2]
    # a small skyline is written whole, without an index
    bench.dump_outputs(str(tmp_path / "c"), _Stats(), 5, ids, org, 0, 1)
    c = _load(str(tmp_path / "c"))
    assert "skyline_sample_index" not in c
    np.testing.assert_array_equal(c["skyline_ids"], ids[:5].numpy())


@pytest.mark.gpu
def test_plain_run_dumps_what_the_query_returns(tmp_path, gpu_engine_factory):
    import torch
    import bench
    n, steps = 300_001, 3
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "C3", "--tuples",
                        str(n), "--steps", str(steps), "--warmup", "1", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and len(line["step_ms"]) == steps
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(n / (line["ms_per_step"] / 1e3))
    assert line["higher_is_better"] is True and line["unit"] == "tuples/s" and line["dtype"] == "f64"
    assert line["metric"] == bench.METRIC
    # nothing that takes runs of its own in a plain line
    assert line["cpu_baseline"] is None
    for k in ("phases_ms_last_step", "counters_last_step", "configs", "end_to_end", "dominance_roofline",
              "csv_ingest", "sort_roofline", "operator_path"):
        assert k not in line
    # the same seeded stream through an engine of this process
    cfg = bench.CONFIGS["C3"]
    D, P = cfg["dims"], cfg["partitions"]
    eng = gpu_engine_factory(D, P, cfg["algo"])
    dev = torch.device("cuda", 0)
    vals, ids = bench.make_stream(eng, cfg["dist"], n, 1234 + D, 0, dev)
    oi = torch.empty(n, dtype=torch.int64, device=dev)
    oo = torch.empty(n, dtype=torch.int32, device=dev)
    g = eng.query_dev(ids, vals, oi, oo, n)
    eng.sync()
    ls, sv = eng.stats()
    got = _load(out)
    assert got["skyline_size"].tolist() == [g] and line["config"]["skyline_size"] == g
    assert 0 < g <= bench.DUMP_MAX_ROWS
    np.testing.assert_array_equal(got["skyline_ids"], oi[:g].cpu().numpy())
    np.testing.assert_array_equal(got["skyline_origins"], oo[:g].cpu().numpy())
    np.testing.assert_array_equal(got["local_sizes"], ls)
    np.testing.assert_array_equal(got["survivors"], sv)
    eng.close()
