"""bench.py's two modes: a plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line; `--full`
adds every secondary leg and in-run check after the same timed steps and writes the full record."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_bench_line import ROOT, _bench


def test_full_is_off_by_default(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--full"])
    assert bench.parse().full is True


def _line(out):
    rows = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert rows, out[-3000:]
    return json.loads(rows[-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_run_times_the_steps_only_and_full_adds_the_checks(tmp_path):
    small = ["--gpus", "1", "--frames", "12", "--width", "640", "--height", "480", "--kpts", "600", "--steps", "3", "--warmup", "1",
             "--full-line"]

    def run(flags, dump):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + small + flags + ["--dump-outputs", str(dump)],
                           cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return _line(r.stdout), r.stderr

    plain, err = run([], tmp_path / "plain")
    assert plain["full"] is False and plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["steps"] == 3
    assert plain["cpu_baseline"] is None and plain["parity_in_run"] is None and plain["full_record"] is None
    assert plain["roofline"]["kernel"].startswith("orb_") and "valu_issue" not in plain["roofline"]
    ex = plain["extra"]
    assert set(ex) == {"bf_match", "kernels", "roofline_pipeline", "valu_issue_probes_Ginst_per_s"}, sorted(ex)
    assert "all_pairs" not in ex["bf_match"] and not ex["valu_issue_probes_Ginst_per_s"]
    assert "] leg " not in err and "cpu baseline" not in err

    full, _ = run(["--full", "--no-ba", "--no-bow", "--no-c3", "--no-c5", "--no-host-fed", "--no-range"], tmp_path / "full")
    assert full["full"] is True and "errors" not in full["extra"], full["extra"].get("errors")
    par = full["parity_in_run"]
    assert par["frames"] == 12 and par["match_pairs"] == 11
    assert par["counts_equal"] and par["keypoints_equal"] and par["descriptors_equal"] and par["match_rows_equal"]
    assert full["cpu_baseline"]["value"] > 0 and full["full_record"]
    bf = full["extra"]["bf_match"]
    assert bf["valu_ceiling_Gpairs_per_s"] > 0 and bf["all_pairs"]["frame_pairs"] == 66
    assert bf["all_pairs_mfma"]["identical_to_popcount"]

    # the timed steps are the same in both modes: they leave the same outputs
    a, b = _load(tmp_path / "plain"), _load(tmp_path / "full")
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
