"""bench.py as every change is measured with it: a plain run prints the headline line alone, `--steps` sets the timed steps, and
`--dump-outputs` writes what the last timed step computed — checked here against the oracle's output for the same simulated families."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

FAMILIES = 20000


@pytest.mark.timeout(600)
def test_plain_run_dumps_the_oracle_output_of_its_last_step(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--families", str(FAMILIES),
           "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert not {"strong_scaling", "share_of_8", "end_to_end", "cpu_baseline"} & set(d), "a plain run measures the headline alone (--full for the rest)"

    f = {n[:-len(".npy")]: np.load(tmp_path / n) for n in os.listdir(tmp_path)}
    assert set(f) == {"counters", "record_windows", "window_offsets", "block_sums"}, "no deferred families: no deferred_groups.npy"
    assert all(a.dtype in (np.float32, np.float64) and a.size > 0 for a in f.values()) and sum(a.nbytes for a in f.values()) <= 64 << 20

    import bench
    import fgx_opts
    import orc
    from fgumi_amd import simulate_grouped_reads
    g = simulate_grouped_reads(FAMILIES, family_size=8, read_length=150)
    want = orc.process(fgx_opts.defaults(min_reads=1), g.blob, g.rec_off, g.rec_len, g.grp_first)
    data = np.frombuffer(want["data"], dtype=np.uint8)
    n = len(want["stats"])
    assert f["counters"][:3].tolist() == [want["count"], len(data), 0]
    assert np.array_equal(f["counters"][3:3 + n], want["stats"].astype(np.float64))
    off, w = bench.dump_window_offsets(len(data))
    assert np.array_equal(f["window_offsets"], off) and np.array_equal(f["record_windows"], data[off[:, None] + np.arange(w)])
    B = bench.DUMP_BLOCK_BYTES
    x = np.concatenate([data, np.zeros(-len(data) % B, dtype=np.uint8)]).astype(np.int64).reshape(-1, B)
    assert np.array_equal(f["block_sums"], np.stack([x.sum(1), (x * (np.arange(B) % 251 + 1)).sum(1)], 1))
