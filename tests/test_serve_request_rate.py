"""The sample_rate key of a qwen3-tts-cli --serve request line (qwen3-tts-jetson_amd/cpp/serve_request.h): it parses
for every rate of the output stage, and a value out of range, malformed or given twice fails its request alone.
CPU only: tests/cpp/test_serve_request_rate.cpp built with g++ against the header."""
import os
import subprocess

from q3t_testutil import REPO


def test_serve_request_sample_rate_key(tmp_path):
    exe = str(tmp_path / "test_serve_request_rate")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "qwen3-tts-jetson_amd", "cpp"),
                    os.path.join(REPO, "tests", "cpp", "test_serve_request_rate.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
