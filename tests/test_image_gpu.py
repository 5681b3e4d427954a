"""The image entries (gz_process_image, gz_image_pack, gz_encoder_submit_image)
on the GPU, with torch tensors in HBM as the images: tests/image_gpu_child.py
holds the checks and says why they run in one process of their own, started
once here."""
import json
import subprocess
import sys

import pytest

import image_gpu_child as child

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def outcome():
    r = subprocess.run([sys.executable, child.__file__], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("name", list(child.CHECKS))
def test_image_gpu(outcome, name):
    assert outcome[name] == "ok", outcome[name]
