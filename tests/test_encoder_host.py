"""gz_encoder and the frame entries on the paths that need no GPU: images
under 32 px (the no-search q=1 encode) and host packing.  Every expected
value is a known answer of tests/golden/manifest.json or numpy evaluating the
definition of the packed image P (include/guetzli_hip.h, gz_frame)."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))
SMALL = ["tex_1x1_q95", "tex_24x24_q95", "tex_20x300_q95", "tex_300x20_q95", "tex_31x64_q95"]


def sha(b):
    return hashlib.sha256(b).hexdigest()


def image(name, group="e2e_edge"):
    e = MANIFEST[group][name]
    a = np.fromfile(os.path.join(GOLDEN, e["input"]), np.uint8).reshape(e["h"], e["w"], 3)
    return e, a


def blend(src):
    """P of an (h, w, 3|4) uint8 image, by the definition."""
    if src.shape[2] == 3:
        return np.ascontiguousarray(src)
    a = src[..., 3:4].astype(np.int64)
    return ((src[..., :3].astype(np.int64) * a + 128) // 255).astype(np.uint8)


def strided(buf_rng, h, w, c, pad, off):
    """An (h, w, c) view with rows w*c + pad bytes apart, starting `off` bytes
    into its buffer, filled with random bytes."""
    stride = w * c + pad
    buf = buf_rng.integers(0, 256, off + stride * h + 7, dtype=np.uint8)
    v = np.lib.stride_tricks.as_strided(buf[off:], (h, w, c), (stride, c, 1))
    return v


def rgba_padded(rgb, alpha, pad=5, off=1):
    """rgb (h, w, 3) as a padded RGBA view with the given alpha plane."""
    h, w, _ = rgb.shape
    v = strided(np.random.default_rng(5), h, w, 4, pad, off)
    v[..., :3] = rgb
    v[..., 3] = alpha
    return v


def test_forty_jobs_known_answers(gz):
    p = gz.Params.for_quality(95)
    with gz.Encoder(in_flight=3, queue_capacity=2) as enc:
        jobs = []
        for i in range(40):
            e, a = image(SMALL[i % 5])
            jobs.append((e, enc.submit(a, p, tag=1000 + i)))
        for i, (e, job) in enumerate(jobs):
            data, st = job.result(return_stats=True)
            assert sha(data) == e["sha256"], (i, e["input"])
            assert st.iterations == e["iters"] == 0
            assert job.tag == 1000 + i
            assert job.seconds_queued >= 0.0 and isinstance(job.detail, dict)
        # a delivered id is gone
        r = gz._EncodeResult()
        assert gz.lib().gz_encoder_wait(enc._h, jobs[0][1].id, ctypes.byref(r)) == 1
        assert gz.lib().gz_encoder_wait(enc._h, 12345, ctypes.byref(r)) == 1
        assert list(enc.results()) == []


def test_single_worker_completes_in_submission_order(gz):
    p = gz.Params.for_quality(95)
    with gz.Encoder(in_flight=1) as enc:
        want = []
        for i in range(10):
            e, a = image(SMALL[(3 * i) % 5])
            want.append((enc.submit(a, p, tag=i).id, e["sha256"]))
        got = [(j.id, sha(j.result())) for j in enc.results()]
        assert got == want
        assert [w[0] for w in want] == list(range(1, 11))
        # nothing outstanding: a blocking next returns at once with job 0
        r = gz._EncodeResult()
        assert gz.lib().gz_encoder_next(enc._h, 1, ctypes.byref(r)) == 0 and r.job == 0
        assert gz.lib().gz_encoder_next(enc._h, 0, ctypes.byref(r)) == 0 and r.job == 0


def test_map_returns_submission_order(gz):
    p = gz.Params.for_quality(95)
    names = [SMALL[(7 * i) % 5] for i in range(23)]
    with gz.Encoder(in_flight=2, queue_capacity=1) as enc:
        out = list(enc.map((image(n)[1] for n in names), p))
    assert [sha(b) for b in out] == [MANIFEST["e2e_edge"][n]["sha256"] for n in names]


def test_failed_job_does_not_affect_neighbours(gz, gpu_available):
    p95, p83 = gz.Params.for_quality(95), gz.Params.for_quality(83)
    e, a = image("tex_24x24_q95")
    with gz.Encoder(in_flight=2) as enc:
        jobs = [enc.submit(a, p95), enc.submit(a, p83), enc.submit(a, p95)]
        big = None
        if not gpu_available:
            # needs a device: fails on its own
            big = enc.submit(np.zeros((48, 64, 3), np.uint8), p95)
            jobs.append(enc.submit(a, p95))
        with pytest.raises(gz.GuetzliError) as ei:
            jobs[1].result()
        assert ei.value.status == 1 and "quality below 84" in str(ei.value)
        if big is not None:
            with pytest.raises(gz.GuetzliError) as ei:
                big.result()
            assert ei.value.status == 2
        for j in jobs[:1] + jobs[2:]:
            assert sha(j.result()) == e["sha256"]


def test_create_needs_no_device_and_close_drops_pending(gz):
    p = gz.Params.for_quality(95)
    e, a = image("tex_20x300_q95")
    enc = gz.Encoder(device=0, in_flight=1, queue_capacity=8)
    jobs = [enc.submit(a, p) for _ in range(8)]
    enc.close()
    for j in jobs:  # delivered results are right; dropped jobs say so
        try:
            assert sha(j.result()) == e["sha256"]
        except gz.GuetzliError as err:
            assert "closed" in str(err)
    with pytest.raises(gz.GuetzliError):
        enc.submit(a, p)
    with gz.Encoder(in_flight=1) as enc2:
        assert sha(enc2.submit(a, p).result()) == e["sha256"]


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("shape", [(1, 1), (24, 24), (41, 33), (65, 34)])
def test_frame_pack_host(gz, shape, c):
    h, w = shape
    rng = np.random.default_rng(h * 131 + w + c)
    for pad in (0, 1, 3, 64):
        for off in (0, 1, 2, 3):
            v = strided(rng, h, w, c, pad, off)
            got = gz.frame_pack(v)
            assert got.shape == (h, w, 3)
            assert np.array_equal(got, blend(v)), (pad, off)


def test_frame_pack_host_all_blend_pairs(gz):
    v = np.zeros((256, 256, 4), np.uint8)
    v[..., 0] = np.arange(256)[None, :]           # R = x
    v[..., 1] = 255 - np.arange(256)[None, :]
    v[..., 2] = (np.arange(256)[None, :] * 7 + 3) % 256
    v[..., 3] = np.arange(256)[:, None]           # A = y
    got = gz.frame_pack(v)
    assert np.array_equal(got, blend(v))
    # alpha 255 is the identity, alpha 0 gives black
    assert np.array_equal(got[255], v[255, :, :3]) and not got[0].any()


def test_rgba_frames_encode_as_their_blend(gz):
    p = gz.Params.for_quality(95)
    e, a = image("tex_24x24_q95")
    opaque = rgba_padded(a, 255)
    assert opaque.strides[0] == 24 * 4 + 5
    data, st = gz.process_frame(opaque, p, return_stats=True)
    assert sha(data) == e["sha256"] and st.iterations == 0
    alpha = np.random.default_rng(9).integers(0, 256, (24, 24), dtype=np.uint8)
    v = rgba_padded(a, alpha, pad=3, off=3)
    assert gz.process_frame(v, p) == gz.process(blend(v), 24, 24, p)
    # a padded RGB view and a layout numpy has to copy (reversed rows)
    v3 = strided(np.random.default_rng(2), 24, 24, 3, 7, 2)
    v3[...] = a
    assert sha(gz.process_frame(v3, p)) == e["sha256"]
    assert sha(gz.process_frame(a[::-1][::-1], p)) == e["sha256"]
    assert gz.process_frame(a[::-1], p) == gz.process(np.ascontiguousarray(a[::-1]), 24, 24, p)


def test_invalid_frames(gz):
    L = gz.lib()
    p = gz.Params.for_quality(95)._c()
    buf = np.zeros(64 * 64 * 4, np.uint8)
    out, size = ctypes.c_void_p(), ctypes.c_size_t()
    rgb = np.zeros(3 * 64 * 64, np.uint8)

    def both(frame):
        st = L.gz_process_frame(0, ctypes.byref(p), frame and ctypes.byref(frame), ctypes.byref(out),
                                ctypes.byref(size), None)
        msg = L.gz_last_error().decode()
        st2 = L.gz_frame_pack(0, frame and ctypes.byref(frame), rgb.ctypes.data)
        assert st == st2 == 1, (st, st2, msg)
        assert msg.startswith("process_frame: ") and len(msg) > 20
        return msg

    ptr = buf.ctypes.data
    for ch in (0, 1, 2, 5, -3):
        assert "channels" in both(gz._Frame(ptr, 8, 8, ch, 0, 0))
    assert "row_stride" in both(gz._Frame(ptr, 8, 8, 3, 23, 0))
    assert "row_stride" in both(gz._Frame(ptr, 8, 8, 4, 24, 0))
    assert "null" in both(gz._Frame(None, 8, 8, 3, 0, 0))
    assert "null" in both(None)
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -5)):
        both(gz._Frame(ptr, w, h, 3, 0, 0))
    for w, h in ((65536, 8), (8, 65536), (1 << 20, 1 << 20)):
        both(gz._Frame(ptr, w, h, 3, 0, 0))
    fr = gz._Frame(ptr, 8, 8, 3, 0, 0)
    assert L.gz_process_frame(0, None, ctypes.byref(fr), ctypes.byref(out), ctypes.byref(size), None) == 1
    assert L.gz_process_frame(0, ctypes.byref(p), ctypes.byref(fr), None, ctypes.byref(size), None) == 1
    assert L.gz_frame_pack(0, ctypes.byref(fr), None) == 1
    # the same through the queue: the job fails, with the message
    with gz.Encoder(in_flight=1) as enc:
        with pytest.raises(gz.GuetzliError) as ei:
            enc.submit(np.zeros((8, 8, 2), np.uint8)).result()
        assert ei.value.status == 1 and "channels" in str(ei.value)
    with pytest.raises(gz.GuetzliError) as ei:
        gz.process_frame(np.zeros((8, 8), np.uint8))
    assert ei.value.status == 1


def test_small_png_file_job(gz):
    """A file job takes process_file's dispatch (under 32 px: no device)."""
    p = gz.Params.for_quality(95)
    small = [k for k, v in MANIFEST["png"].items() if not v.get("fail") and v["w"] < 32 and v["h"] < 32]
    assert small
    data = open(os.path.join(GOLDEN, MANIFEST["png"][small[0]]["file"]), "rb").read()
    with gz.Encoder(in_flight=1) as enc:
        good = enc.submit(data, p)
        bad = enc.submit(b"\x89PNG\r\n\x1a\n" + b"\0" * 40, p)
        assert good.result() == gz.process_file(data, p)
        with pytest.raises(gz.GuetzliError) as ei:
            bad.result()
        assert ei.value.status == 1
