"""The request-line parser of qwen3-tts-cli --serve (qwen3-tts-jetson_amd/cpp/serve_request.h): two-field lines as
before, the third TAB field's keys (language, temperature, top_k, repetition_penalty, max_tokens, speaker), an empty
third field, and the bad fields (unknown key, malformed number, ...) that fail their request alone.
CPU only: tests/cpp/test_serve_request.cpp built with g++ against the header."""
import os
import subprocess

from q3t_testutil import REPO


def test_serve_request_parser(tmp_path):
    exe = str(tmp_path / "test_serve_request")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "qwen3-tts-jetson_amd", "cpp"),
                    os.path.join(REPO, "tests", "cpp", "test_serve_request.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
