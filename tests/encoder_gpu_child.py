"""The checks of tests/test_encoder_gpu.py, run in a process of their own.

The frames are torch tensors in HBM, and torch's HIP runtime has to be the
first one initialised in a process (tests/test_strips.py,
test_rccl_collectives_beside_torch); a pytest process that ran other GPU
tests has initialised the library's already.  So test_encoder_gpu.py starts
this file once and asserts on the outcome of each check, printed as one JSON
line {check: "ok" | traceback}.

  gz_encoder and the frame entries on the GPU: the device import of pitched
  RGB / RGBA frames (k_import_rgb8) against numpy evaluating the definition
  of the packed image P, and encodes through gz_process_frame and the queue
  against the known answers of tests/golden/manifest.json.  Bit-exact
  throughout."""
import hashlib
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))
CASES = ["tex_64x48_q95", "tex_41x33_q95", "flat_48x40_q95", "tex_100x77_q95", "bees_88x64_q95"]
FORMS = ["rgb_device", "rgba_device", "rgba_host"]
SHAPES = [(32, 32), (41, 33), (65, 34), (100, 77)]

CHECKS = {}


def check(name):
    def reg(fn):
        CHECKS[name] = fn
        return fn
    return reg


def sha(b):
    return hashlib.sha256(b).hexdigest()


def blend(src):
    """P of an (h, w, 3|4) uint8 image, by the definition."""
    if src.shape[2] == 3:
        return np.ascontiguousarray(src)
    a = src[..., 3:4].astype(np.int64)
    return ((src[..., :3].astype(np.int64) * a + 128) // 255).astype(np.uint8)


def host_view(buf, h, w, c, stride, off):
    return np.lib.stride_tricks.as_strided(buf[off:], (h, w, c), (stride, c, 1))


def device_view(buf, h, w, c, stride, off):
    """The same view of a copy of `buf` in HBM."""
    import torch
    t = torch.empty(buf.size, dtype=torch.uint8, device="cuda")
    t.copy_(torch.from_numpy(buf))
    return t[off:].as_strided((h, w, c), (stride, c, 1))


_images = {}


def image(name):
    if name not in _images:
        e = MANIFEST["e2e"][name]
        a = np.fromfile(os.path.join(GOLDEN, e["input"]), np.uint8).reshape(e["h"], e["w"], 3)
        a.setflags(write=False)
        _images[name] = (e, a)
    return _images[name]


def form(name, kind, alpha=255):
    """The manifest image in one of the three input forms."""
    e, a = image(name)
    h, w = e["h"], e["w"]
    if kind == "rgb_device":
        import torch
        return torch.from_numpy(a.copy()).to("cuda")
    stride, off = 4 * w + 3, 1
    buf = np.random.default_rng(w).integers(0, 256, off + stride * h + 5, dtype=np.uint8)
    v = host_view(buf, h, w, 4, stride, off)
    v[..., :3] = a
    v[..., 3] = alpha
    return v if kind == "rgba_host" else device_view(buf, h, w, 4, stride, off)


def frame_pack_device(gz, shape, c):
    h, w = shape
    rng = np.random.default_rng(1000 * h + 10 * w + c)
    for pad in (0, 1, 3, 64):
        for off in (0, 1, 2, 3):
            stride = w * c + pad
            buf = rng.integers(0, 256, off + stride * h + 9, dtype=np.uint8)
            t = device_view(buf, h, w, c, stride, off)
            assert t.__cuda_array_interface__["data"][0] % 4 == off
            got = gz.frame_pack(t)
            assert np.array_equal(got, blend(host_view(buf, h, w, c, stride, off))), (pad, off)


for _shape in SHAPES:
    for _c in (3, 4):
        check("frame_pack_device-%dx%d-%d" % (_shape[0], _shape[1], _c))(
            lambda gz, s=_shape, c=_c: frame_pack_device(gz, s, c))


@check("frame_pack_device_all_blend_pairs")
def _(gz):
    v = np.zeros((256, 256, 4), np.uint8)
    v[..., 0] = np.arange(256)[None, :]           # R = x
    v[..., 1] = 255 - np.arange(256)[None, :]
    v[..., 2] = (np.arange(256)[None, :] * 7 + 3) % 256
    v[..., 3] = np.arange(256)[:, None]           # A = y
    want = blend(v)
    flat = v.reshape(-1)
    assert np.array_equal(gz.frame_pack(device_view(flat, 256, 256, 4, 1024, 0)), want)  # one load per pixel
    shifted = np.concatenate([np.zeros(1, np.uint8), flat])
    assert np.array_equal(gz.frame_pack(device_view(shifted, 256, 256, 4, 1024, 1)), want)  # byte loads


@check("frame_pack_device_small_and_layouts")
def _(gz):
    """Under 32 px a device frame is packed on the host after a pitched copy;
    a layout a frame cannot describe is refused, not copied; a tensor is
    checked against the device of the call."""
    rng = np.random.default_rng(3)
    for h, w, c, pad, off in ((24, 24, 4, 3, 1), (1, 1, 3, 0, 2), (31, 64, 4, 0, 0), (40, 20, 3, 5, 3)):
        stride = w * c + pad
        buf = rng.integers(0, 256, off + stride * h + 9, dtype=np.uint8)
        got = gz.frame_pack(device_view(buf, h, w, c, stride, off))
        assert np.array_equal(got, blend(host_view(buf, h, w, c, stride, off)))
    import torch
    t = torch.zeros((3, 40, 48), dtype=torch.uint8, device="cuda").permute(1, 2, 0)
    for call in (gz.frame_pack, gz.process_frame):
        try:
            call(t)
            raise AssertionError("a CHW layout was accepted")
        except gz.GuetzliError as err:
            assert err.status == 1 and ".contiguous()" in str(err)
    assert gz.frame_pack(t.contiguous()).shape == (40, 48, 3)
    try:
        gz.frame_pack(t.contiguous(), device=1)
        raise AssertionError("a tensor of device 0 was accepted for device 1")
    except gz.GuetzliError as err:
        assert err.status == 1 and "device" in str(err)


def process_frame_known_answer(gz, name, kind):
    e, _ = image(name)
    data, st = gz.process_frame(form(name, kind), gz.Params.for_quality(95), return_stats=True)
    assert (sha(data), st.iterations) == (e["sha256"], e["iters"])


for _name in CASES:
    for _kind in FORMS:
        check("process_frame_known_answers-%s-%s" % (_name, _kind))(
            lambda gz, n=_name, k=_kind: process_frame_known_answer(gz, n, k))


@check("process_frame_random_alpha")
def _(gz):
    alpha = np.random.default_rng(4).integers(0, 256, (48, 64), dtype=np.uint8)
    p = gz.Params.for_quality(95)
    host = form("tex_64x48_q95", "rgba_host", alpha)
    want = gz.process(blend(host), 64, 48, p)
    assert gz.process_frame(form("tex_64x48_q95", "rgba_device", alpha), p) == want
    assert gz.process_frame(host, p) == want


@check("queue_known_answers")
def _(gz):
    p = gz.Params.for_quality(95)
    work = [(n, k) for k in FORMS for n in CASES]
    png = open(os.path.join(GOLDEN, "png", "bees.png"), "rb").read()
    jpg = open(os.path.join(GOLDEN, "jpeg", "tiny_pil_q85_444.jpg"), "rb").read()
    with gz.Encoder(in_flight=4) as enc:
        jobs = [enc.submit(form(n, k), p, tag=i) for i, (n, k) in enumerate(work)]
        files = [enc.submit(png, p), enc.submit(jpg, p)]
        for i, ((n, k), job) in enumerate(zip(work, jobs)):
            data, st = job.result(return_stats=True)
            e = MANIFEST["e2e"][n]
            assert (sha(data), st.iterations, job.tag) == (e["sha256"], e["iters"], i), (n, k)
            assert "thread_cpu_s" in job.detail
        assert files[0].result() == gz.process_file(png, p)
        assert files[1].result() == gz.process_file(jpg, p)
        mixed = work[::2]
        out = list(enc.map((form(n, k) for n, k in mixed), p))
        assert [sha(b) for b in out] == [MANIFEST["e2e"][n]["sha256"] for n, _ in mixed]
        assert list(enc.results()) == []


@check("close_with_work_pending")
def _(gz):
    p = gz.Params.for_quality(95)
    e, _ = image("tex_64x48_q95")
    enc = gz.Encoder(in_flight=2)
    jobs = [enc.submit(form(CASES[i % 5], FORMS[i % 3]), p) for i in range(12)]
    enc.close()
    for j in jobs:  # nothing was collected before the close: every job says so
        try:
            j.result()
            raise AssertionError("a result outlived its encoder")
        except gz.GuetzliError as err:
            assert "closed" in str(err)
    with gz.Encoder(in_flight=2) as fresh:
        assert sha(fresh.submit(form("tex_64x48_q95", "rgba_device"), p).result()) == e["sha256"]


def main():
    import torch
    torch.ones(16, device="cuda").sum().item()  # torch's HIP runtime first
    sys.path.insert(0, os.path.join(ROOT, "guetzli-cuda-opencl_amd", "python"))
    import guetzli_amd as gz
    out = {}
    for name, fn in CHECKS.items():
        try:
            fn(gz)
            out[name] = "ok"
        except Exception:
            out[name] = traceback.format_exc()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
