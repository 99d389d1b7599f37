"""The queue's host scheduling (qwen3-tts-jetson_amd/csrc/queue_sched.h), which Engine::QueueLoop asks before every HIP
call of the continuous-batching loop: admission order and the busy-slot cap, the one-frame-late reap ("held is not
ended", the stop at max_len), the frame graph's slot count, a text round's blob int for int, the hold rule, the text log
and its replay after a fault, and every rejection's message.  CPU only: tests/cpp/test_queue_sched.cpp built with g++
against the header, which must compile without HIP."""
import os
import subprocess

from q3t_testutil import REPO


def test_queue_sched(tmp_path):
    exe = str(tmp_path / "test_queue_sched")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(REPO, "qwen3-tts-jetson_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "test_queue_sched.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
