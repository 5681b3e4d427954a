"""host/job_queue.h (the queue under gz_encoder) as a stand-alone host program,
tests/native/job_queue_check.cc: plain, and under ThreadSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(name, extra):
    src = os.path.join(ROOT, "tests", "native", "job_queue_check.cc")
    hdr = os.path.join(ROOT, "guetzli-cuda-opencl_amd", "csrc", "host", "job_queue.h")
    out = os.path.join(ROOT, "tests", "_build", name)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        tmp = "%s.%d.tmp" % (out, os.getpid())
        subprocess.run(["g++", "-std=c++17", "-g", "-pthread", "-Wall", "-Werror"] + extra +
                       ["-I", os.path.join(ROOT, "guetzli-cuda-opencl_amd", "csrc"), src, "-o", tmp],
                       check=True)
        os.replace(tmp, out)
    return out


@pytest.mark.parametrize("name,flags", [("job_queue_check", ["-O2"]),
                                        ("job_queue_check_tsan", ["-O1", "-fsanitize=thread"])])
def test_job_queue_check(name, flags):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([build(name, flags)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "job_queue_check ok" in r.stdout
    assert "ThreadSanitizer" not in r.stderr
