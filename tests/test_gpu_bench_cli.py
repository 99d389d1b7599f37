"""GPU: bench.py's command line on the tiny configuration (the benchmark itself is what is under test).

A plain run times exactly --steps steps, prints one JSON line with the headline keys and none of the secondary
sections, and --dump-outputs writes the last timed step's codes and PCM; two runs with the same arguments write
identical files.  --full adds the secondary sections to the same line (sections switched off stay null).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from q3t_testutil import REPO

pytestmark = pytest.mark.gpu

NF = 8
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
SECONDARY = ("roofline", "cp_roofline", "vocoder_roofline", "batched", "serving", "cpu_baseline")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--cfg", "tiny", "--frames", str(NF),
                        *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_headline_only_and_dump_repeatable(tmp_path):
    res = []
    for name in ("a", "b"):
        res.append(_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / name)))
    r = res[0]
    for k in HEADLINE:
        assert k in r, k
    assert not any(k in r for k in SECONDARY), sorted(r)
    assert r["steps"] == 3 and r["warmup"] == 1 and r["unit"] == "frames/s" and r["higher_is_better"] is True
    # value is the timed steps' frames over their time: consistent with ms_per_step (both rounded to 2 decimals)
    assert r["value"] == pytest.approx(NF / (r["ms_per_step"] * 1e-3), rel=2e-2)
    assert r["breakdown_ms_per_step"]["frames_ms"] <= r["ms_per_step"]
    a = {n: np.load(str(tmp_path / "a" / f"{n}.npy")) for n in ("codes", "pcm")}
    b = {n: np.load(str(tmp_path / "b" / f"{n}.npy")) for n in ("codes", "pcm")}
    assert a["codes"].dtype == np.float32 and a["codes"].shape == (1, NF, 16)
    assert a["pcm"].dtype == np.float32 and a["pcm"].ndim == 2 and a["pcm"].shape[0] == 1 and a["pcm"].shape[1] > 0
    assert np.isfinite(a["pcm"]).all() and np.abs(a["pcm"]).max() > 0
    assert np.array_equal(a["codes"], a["codes"].round()) and a["codes"].min() >= 0
    assert np.array_equal(a["codes"], b["codes"]) and np.array_equal(a["pcm"], b["pcm"])


def test_full_run_adds_the_secondary_sections(tmp_path):
    r = _bench("--steps", "2", "--warmup", "1", "--full", "--batched", "4", "--serve", "0", "--cpu-baseline", "off",
               "--roofline-pos", "16", "--stage-iters", "2")
    for k in HEADLINE + SECONDARY:
        assert k in r, k
    assert r["steps"] == 2
    assert r["roofline"]["launch_ms"] > 0 and r["talker_step_ms"] > 0 and r["cp_frame_ms"] > 0
    assert r["batched"]["value"] > 0 and "4 concurrent utterances" in r["batched"]["config"]
    assert r["serving"] is None and r["cpu_baseline"] is None
