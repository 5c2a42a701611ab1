"""A plain `bench.py` run is the headline figure alone; --full adds the parity gate, the CPU baseline, the power leg and the secondary
workloads, and neither form changes what the timed steps compute."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "64"] + extra,
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_is_the_headline_alone_and_full_checks_the_same_outputs(tmp_path):
    # n = 8192, SEAL default primes: the headline configuration, whose --full run would time the secondary workloads too
    plain = _bench(["--dump-outputs", str(tmp_path / "plain")])
    assert plain["parity"].startswith("skipped") and plain["cpu_baseline"] is None
    assert "power" not in plain and "secondary" not in plain
    assert plain["summary"]["mulrelin_n8192"]["parity_ok"] is None and plain["value"] > 0
    full = _bench(["--full", "--no-secondary", "--no-power", "--cpu-sample", "64", "--dump-outputs", str(tmp_path / "full")])
    assert "bit-exact vs oracle on 64 items" in full["parity"] and "all 64 results decrypt" in full["parity"]
    assert full["cpu_baseline"]["value"] > 0 and full["summary"]["mulrelin_n8192"]["parity_ok"] is True
    assert plain["outputs_dumped"] == full["outputs_dumped"]
    for name in plain["outputs_dumped"]:
        assert np.array_equal(np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")), name
