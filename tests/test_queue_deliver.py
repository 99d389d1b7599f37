"""The host bookkeeping of the queue's deliveries (qwen3-tts-jetson_amd/csrc/queue_deliver.h: queue_plan / queue_commit),
which Engine::QueueStreamer runs for every collected chunk: entries in utterance order, pieces without frames dropped,
nothing after a cancel or a final, and across a fallback re-run (a "fault" after every possible number of chunks, then
the whole queue again with the state kept) every frame handed out exactly once and a cancelled utterance cancelled
again where it stood.  CPU only: tests/cpp/test_queue_deliver.cpp built with g++ against the header."""
import os
import subprocess

from q3t_testutil import REPO


def test_queue_deliver_bookkeeping(tmp_path):
    exe = str(tmp_path / "test_queue_deliver")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(REPO, "qwen3-tts-jetson_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "test_queue_deliver.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
