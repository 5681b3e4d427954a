"""The image entries (gz_process_image, gz_image_pack, gz_encoder_submit_image)
on the paths that need no GPU: host packing of every layout, sample type and
value, the refusals, and encodes under 32 px.  Every expected value is numpy
evaluating the definition of the packed image P (tests/image_ref.py).  No
tolerance anywhere."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import image_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (7, 5), (33, 41)]
ORDERS = {1: ["L"], 2: ["LA", "AL"], 3: ["RGB", "BGR"], 4: ["RGBA", "BGRA", "ARGB", "ABGR"]}


def base_view(rng, kind, layout, h, w, c, pad, off):
    """A random (h, w) image in `layout`: rows padded by `pad` samples, `off`
    samples into its buffer."""
    row = w * (c if layout == "HWC" else 1) + pad
    plane = h * row + 5
    buf = ref.random_samples(rng, kind, ref.strided_need(layout, h, w, c, row, off, plane) + 2)
    return ref.strided(buf, layout, h, w, c, row, off, plane)


def hw_slice(view, layout, rows, cols):
    return view[:, rows, cols] if layout == "CHW" else view[rows, cols]


VIEWS = {
    "tight": lambda h, w: (h, w, 0, 0, slice(None), slice(None)),
    "padded": lambda h, w: (h, w, 3, 0, slice(None), slice(None)),
    "offset1": lambda h, w: (h, w, 1, 1, slice(None), slice(None)),
    "offset3": lambda h, w: (h, w, 0, 3, slice(None), slice(None)),
    "rows_reversed": lambda h, w: (h, w, 2, 2, slice(None, None, -1), slice(None)),
    "cols_reversed": lambda h, w: (h, w, 0, 1, slice(None), slice(None, None, -1)),
    "step_2_3": lambda h, w: (2 * h, 3 * w, 1, 0, slice(None, None, 2), slice(None, None, 3)),
}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("layout", ["HWC", "CHW", "HW"])
@pytest.mark.parametrize("kind", list(ref.DTYPES))
def test_image_pack_host(gz, kind, layout, shape):
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w + len(kind) + len(layout))
    for c in ([1] if layout == "HW" else [1, 2, 3, 4]):
        for name, make in VIEWS.items():
            bh, bw, pad, off, rows, cols = make(h, w)
            v = hw_slice(base_view(rng, kind, layout, bh, bw, c, pad, off), layout, rows, cols)
            for order in ORDERS[c]:
                got = gz.image_pack(v, layout=layout, order=order)
                assert got.shape == (h, w, 3) and got.dtype == np.uint8
                assert np.array_equal(got, ref.reference(v, layout, order)), (c, name, order)
            # the default order and the default layout
            assert np.array_equal(gz.image_pack(v, layout=layout), ref.reference(v, layout))
            if not (layout == "CHW" and w <= 4):
                assert np.array_equal(gz.image_pack(v), ref.reference(v, layout))


@pytest.mark.parametrize("kind", list(ref.DTYPES))
def test_image_pack_host_broadcast_channel(gz, kind):
    g = ref.random_samples(np.random.default_rng(3), kind, 33 * 41).reshape(33, 41)
    want = ref.reference(g, "HW")
    hwc = np.broadcast_to(g[..., None], (33, 41, 3))
    chw = np.broadcast_to(g, (3, 33, 41))
    assert hwc.strides[2] == 0 and chw.strides[0] == 0
    assert np.array_equal(gz.image_pack(hwc), want)
    assert np.array_equal(gz.image_pack(chw), want)
    assert np.array_equal(gz.image_pack(hwc, order="BGR"), want)
    row = np.broadcast_to(g[0], (33, 41))  # a row stride of 0
    assert np.array_equal(gz.image_pack(row), ref.reference(row, "HW"))


def test_all_u16_values(gz):
    a = ref.u16_value_image()
    got = gz.image_pack(a)
    assert np.array_equal(got, ref.reference(a, "HW"))
    assert np.array_equal(got[..., 0], np.repeat(np.arange(256, dtype=np.uint8), 256).reshape(256, 256))
    assert np.array_equal(gz.image_pack((np.arange(256, dtype=np.uint16) * 257).reshape(16, 16))[..., 0].ravel(),
                          np.arange(256))


def test_all_f16_bit_patterns(gz):
    a = ref.f16_value_image()
    assert np.array_equal(gz.image_pack(a), ref.reference(a, "HW"))
    exact = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float16).reshape(16, 16)
    assert np.array_equal(gz.image_pack(exact)[..., 1].ravel(), np.arange(256))


def test_all_la_pairs(gz):
    a = ref.la_pairs_image()
    got = gz.image_pack(a)
    assert np.array_equal(got, ref.reference(a, "HWC"))
    # alpha 255 is the identity, alpha 0 gives black
    assert np.array_equal(got[255, :, 0], np.arange(256)) and not got[0].any()
    assert np.array_equal(gz.image_pack(a[..., ::-1], order="AL"), got)


def test_f32_value_set(gz):
    a = ref.f32_value_image()
    assert np.array_equal(gz.image_pack(a), ref.reference(a, "HW"))
    # what the definition says about the values, stated directly
    one = lambda *v: gz.image_pack(np.array([v], np.float32))[0, :, 0].tolist()
    assert one(np.nan, -np.inf, -1.0, -0.0, 0.0, 1e-42) == [0] * 6
    assert one(1.0, 2.0, np.inf) == [255] * 3
    k = np.arange(255, dtype=np.float32)
    ties = ((k + np.float32(0.5)) / np.float32(255)).reshape(1, 255)
    assert np.array_equal(ties * np.float32(255), (k + np.float32(0.5)).reshape(1, 255))  # real ties
    assert np.array_equal(gz.image_pack(ties)[0, :, 0], k + (k.astype(np.int64) % 2))  # to even: 0.5 -> 0, 1.5 -> 2
    exact = (np.arange(256, dtype=np.float32) / np.float32(255)).reshape(16, 16)
    assert np.array_equal(gz.image_pack(exact)[..., 2].ravel(), np.arange(256))


def image_struct(gz, data, w=8, h=8, channels=3, sample=0, row=None, pixel=None, offsets=None):
    sb = (1, 2, 2, 4)[sample] if 0 <= sample <= 3 else 1
    row = w * channels * sb if row is None else row
    pixel = channels * sb if pixel is None else pixel
    offsets = [c * sb for c in range(4)] if offsets is None else offsets
    return gz._Image(data, w, h, channels, sample, row, pixel, (ctypes.c_ssize_t * 4)(*offsets), 0)


def test_invalid_images(gz):
    L = gz.lib()
    p = gz.Params.for_quality(95)._c()
    buf = np.zeros(64 * 64 * 16, np.uint8)
    ptr = buf.ctypes.data
    assert ptr % 4 == 0
    rgb = np.zeros(3 * 64 * 64, np.uint8)
    out, size = ctypes.c_void_p(), ctypes.c_size_t()

    def both(im):
        st = L.gz_process_image(0, ctypes.byref(p), im and ctypes.byref(im), ctypes.byref(out),
                                ctypes.byref(size), None)
        msg = L.gz_last_error().decode()
        st2 = L.gz_image_pack(0, im and ctypes.byref(im), rgb.ctypes.data)
        msg2 = L.gz_last_error().decode()
        assert st == st2 == 1, (st, st2, msg, msg2)
        assert msg.startswith("process_image: ") and msg2.startswith("image_pack: ")
        assert msg[len("process_image: "):] == msg2[len("image_pack: "):]
        return msg

    # every sample naturally aligned: data, both strides, each used offset
    for sample, sb in ((1, 2), (2, 2), (3, 4)):
        assert "data" in both(image_struct(gz, ptr + 1, sample=sample))
        assert "row_stride" in both(image_struct(gz, ptr, sample=sample, row=8 * 3 * sb + 1))
        assert "pixel_stride" in both(image_struct(gz, ptr, sample=sample, pixel=3 * sb + 1))
        for c in range(3):
            offs = [0, sb, 2 * sb, 1]  # (the unused fourth offset is ignored)
            ok = image_struct(gz, ptr, sample=sample, offsets=offs)
            assert L.gz_image_pack(0, ctypes.byref(ok), rgb.ctypes.data) == 0
            offs[c] += 1
            assert "channel_offset" in both(image_struct(gz, ptr, sample=sample, offsets=offs))
    assert "data" in both(image_struct(gz, ptr + 2, sample=3))
    for ch in (0, 5, -1):
        assert "channels" in both(image_struct(gz, ptr, channels=ch))
    for sample in (4, -1):
        assert "sample" in both(image_struct(gz, ptr, sample=sample))
    assert "null" in both(image_struct(gz, None))
    assert "null" in both(None)
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -1), (65536, 8), (8, 65536)):
        msg = both(image_struct(gz, ptr, w=w, h=h, row=0, pixel=0))
        assert "width" in msg and "height" in msg
    im = image_struct(gz, ptr)
    assert L.gz_process_image(0, None, ctypes.byref(im), ctypes.byref(out), ctypes.byref(size), None) == 1
    assert L.gz_process_image(0, ctypes.byref(p), ctypes.byref(im), None, ctypes.byref(size), None) == 1
    assert L.gz_image_pack(0, ctypes.byref(im), None) == 1
    # a quality the search does not support is refused before any device work
    p83 = gz.Params.for_quality(83)._c()
    big = image_struct(gz, ptr, w=64, h=64)
    assert L.gz_process_image(0, ctypes.byref(p83), ctypes.byref(big), ctypes.byref(out), ctypes.byref(size),
                              None) == 1
    assert "quality below 84" in L.gz_last_error().decode()


def test_invalid_python_images(gz):
    def refused(image, word, **kw):
        for call in (gz.image_pack, gz.process_image):
            with pytest.raises(gz.GuetzliError) as ei:
                call(image, **kw)
            assert ei.value.status == 1 and word in str(ei.value), str(ei.value)

    refused(np.zeros((8, 8, 3), np.float64), "float64")
    refused(np.zeros((8, 8, 3), np.int32), "int32")
    refused(np.zeros((8, 8, 3), np.dtype("V2")), "V2")  # what a bfloat16 tensor exports
    refused(np.zeros((8, 8, 3), np.dtype(">u2")), ">u2")
    refused(np.zeros((8, 8, 3), np.dtype(">f4")), ">f4")
    refused(np.zeros((8, 8, 3), np.uint8), "order", order="RGBA")
    refused(np.zeros((8, 8, 3), np.uint8), "order", order="RG")
    refused(np.zeros((8, 8, 3), np.uint8), "order", order="RGG")
    refused(np.zeros((8, 8), np.uint8), "order", order="RGB")
    refused(np.zeros((5, 6, 7), np.uint8), "layout")
    refused(np.zeros((5, 6, 7), np.uint8), "channels", layout="HWC")
    refused(np.zeros((8, 8, 3), np.uint8), "layout", layout="HW")
    refused(np.zeros((8, 8, 3), np.uint8), "layout", layout="NHWC")
    refused(np.zeros((0, 8, 3), np.uint8), "height")
    with gz.Encoder(in_flight=1) as enc:
        with pytest.raises(gz.GuetzliError) as ei:
            enc.submit_image(np.zeros((8, 8, 3), np.float64))
        assert ei.value.status == 1 and "float64" in str(ei.value)


def test_small_images_need_no_device(gz):
    """Under 32 px there is no search and no device work."""
    p = gz.Params.for_quality(95)
    g = ref.random_samples(np.random.default_rng(7), "u16", 24 * 24).reshape(24, 24)
    pack = gz.image_pack(g)
    assert np.array_equal(pack, ref.reference(g, "HW"))
    want = gz.process(pack, 24, 24, p)
    data, st = gz.process_image(g, p, return_stats=True)
    assert data == want and st.iterations == 0
    f = ref.random_samples(np.random.default_rng(8), "f32", 4 * 31 * 20).reshape(4, 31, 20)
    want_f = gz.process(ref.reference(f, "CHW", "ARGB"), 20, 31, p)
    with gz.Encoder(in_flight=1) as enc:
        jobs = [enc.submit_image(g, p, tag=7), enc.submit_image(f, p, order="ARGB"),
                enc.submit_image(np.zeros((8, 8, 3), np.uint8), gz.Params.for_quality(83)),
                enc.submit(pack, p), enc.submit_image(g[::-1, ::-1], p, tag="flipped")]
        assert jobs[0].result() == want and jobs[0].tag == 7
        assert jobs[1].result() == want_f
        with pytest.raises(gz.GuetzliError) as ei:
            jobs[2].result()
        assert ei.value.status == 1 and "process_image: " in str(ei.value)
        assert jobs[3].result() == want
        assert jobs[4].result() == gz.process(np.ascontiguousarray(pack[::-1, ::-1]), 24, 24, p)
        assert jobs[4].tag == "flipped"
        assert list(enc.results()) == []


def _links_with_sanitizers(tmp_path):
    src = tmp_path / "one.cc"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", str(src), "-o", str(tmp_path / "one")],
                       capture_output=True)
    return r.returncode == 0


def test_host_packer_reads_only_the_addressed_samples(tmp_path):
    """tests/native/image_pack_check.cc under AddressSanitizer and UBSan, as a
    program of its own."""
    if not _links_with_sanitizers(tmp_path):
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here")
    out = tmp_path / "image_pack_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "guetzli-cuda-opencl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "image_pack_check.cc"), "-o", str(out)], check=True)
    r = subprocess.run([str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.count(": ok") == 9, r.stdout
