"""The checks of tests/test_image_gpu.py, run in a process of their own.

The images are torch tensors in HBM, and torch's HIP runtime has to be the
first one initialised in a process (tests/encoder_gpu_child.py says why).  So
test_image_gpu.py starts this file once and asserts on the outcome of each
check, printed as one JSON line {check: "ok" | traceback}.

  The image entries on the GPU: the device import of images of any layout
  (k_import_image: its generic path, its four-pixels-per-lane path on both
  sides of each eligibility condition, row tails) against numpy evaluating the
  definition of the packed image P (tests/image_ref.py), and encodes through
  gz_process_image and the queue against the known answers of
  tests/golden/manifest.json.  Bit-exact throughout."""
import ctypes
import hashlib
import json
import os
import sys
import traceback

import numpy as np

import image_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))
CASES = ["tex_64x48_q95", "tex_41x33_q95", "bees_88x64_q95"]
FORMS = ["chw_u8", "hwc_bgr_u8", "chw_f32", "chw_f16", "hwc_u16", "hwc_rgba_f32"]
ORDERS = ["L", "LA", "RGB", "BGR", "RGBA", "BGRA", "ARGB"]
# (h, w): the smallest searched; odd both ways; w = 2 and 3 (mod 4); wider
# than a wave's 256 pixels of the wide path; wider than, and no multiple of,
# the 1024 pixels one workgroup covers there
SHAPES = [(32, 32), (41, 33), (65, 34), (32, 35), (40, 300), (33, 1031)]

CHECKS = {}


def check(name):
    def reg(fn):
        CHECKS[name] = fn
        return fn
    return reg


def sha(b):
    return hashlib.sha256(b).hexdigest()


def to_device(a):
    """A copy of the numpy array in HBM, with the same shape and dtype."""
    import torch
    return torch.from_numpy(np.array(a)).to("cuda")  # (a contiguous, writable copy first)


def device_strided(buf, layout, h, w, c, row, off, plane=0):
    """ref.strided of a copy of `buf` in HBM."""
    t = to_device(buf)
    if layout == "HW":
        return t.as_strided((h, w), (row, 1), off)
    if layout == "HWC":
        return t.as_strided((h, w, c), (row, c, 1), off)
    return t.as_strided((c, h, w), (plane, row, 1), off)


def pointer(t):
    return t.__cuda_array_interface__["data"][0]


def layout_matrix(gz, kind, layout):
    """Contiguous tensors of every channel count and order."""
    rng = np.random.default_rng(len(kind) * 7 + len(layout))
    for h, w in ((32, 32), (41, 33)):
        for order in (["L"] if layout == "HW" else ORDERS):
            c = len(order)
            shape = {"HW": (h, w), "HWC": (h, w, c), "CHW": (c, h, w)}[layout]
            a = ref.random_samples(rng, kind, int(np.prod(shape))).reshape(shape)
            got = gz.image_pack(to_device(a), layout=layout, order=order)
            assert np.array_equal(got, ref.reference(a, layout, order)), (h, w, order)


for _kind in ref.DTYPES:
    for _layout in ("HWC", "CHW", "HW"):
        check("image_pack_device-%s-%s" % (_kind, _layout))(
            lambda gz, k=_kind, l=_layout: layout_matrix(gz, k, l))


def wide_path_conditions(gz, kind):
    """Planar RGB and row-contiguous gray on both sides of each condition of
    the four-pixels-per-lane path: the first sample aligned to four samples or
    one sample off, the row stride a multiple of four samples or one more,
    w = 0, 1, 2, 3 (mod 4)."""
    rng = np.random.default_rng(len(kind))
    it = np.dtype(ref.DTYPES[kind]).itemsize
    for h, w in SHAPES:
        for layout, c in (("CHW", 3), ("HW", 1)):
            for off in (0, 1):
                for pad in (0, 1, 4):
                    row = (w + 3) // 4 * 4 + pad
                    plane = (h * row + 3) // 4 * 4
                    buf = ref.random_samples(rng, kind, ref.strided_need(layout, h, w, c, row, off, plane) + 3)
                    t = device_strided(buf, layout, h, w, c, row, off, plane)
                    assert pointer(t) % (4 * it) == off * it
                    got = gz.image_pack(t, layout=layout)
                    want = ref.reference(ref.strided(buf, layout, h, w, c, row, off, plane), layout)
                    assert np.array_equal(got, want), (h, w, layout, off, pad)


for _kind in ref.DTYPES:
    check("image_pack_device_wide_path-%s" % _kind)(lambda gz, k=_kind: wide_path_conditions(gz, k))


@check("image_pack_device_views")
def _(gz):
    rng = np.random.default_rng(11)
    a = ref.random_samples(rng, "f32", 3 * 80 * 128).reshape(3, 80, 128)
    t = to_device(a)
    assert np.array_equal(gz.image_pack(t[:, 8:72, 16:116]), ref.reference(a[:, 8:72, 16:116], "CHW"))
    b = ref.random_samples(rng, "u8", 90 * 70 * 4).reshape(90, 70, 4)
    assert np.array_equal(gz.image_pack(to_device(b)[::2, ::2], order="BGRA"),
                          ref.reference(b[::2, ::2], "HWC", "BGRA"))
    g = ref.random_samples(rng, "u16", 40 * 52).reshape(40, 52)
    want = ref.reference(g, "HW")
    assert np.array_equal(gz.image_pack(to_device(g).expand(3, 40, 52)), want)
    assert np.array_equal(gz.image_pack(to_device(g).unsqueeze(2).expand(40, 52, 3)), want)
    # negative strides (torch has none): bottom-up and mirrored rows of an HWC
    # and of a planar image, described by hand
    h, w = 37, 45
    for kind in ("u8", "f32"):
        it = np.dtype(ref.DTYPES[kind]).itemsize
        hwc = ref.random_samples(rng, kind, h * w * 3).reshape(h, w, 3)
        t = to_device(hwc)
        last = pointer(t) + ((h - 1) * w + (w - 1)) * 3 * it
        im = gz._Image(last, w, h, 3, {"u8": 0, "f32": 3}[kind], -w * 3 * it, -3 * it,
                       (ctypes.c_ssize_t * 4)(0, it, 2 * it, 0), 1)
        out = np.zeros((h, w, 3), np.uint8)
        assert gz.lib().gz_image_pack(0, ctypes.byref(im), out.ctypes.data) == 0
        assert np.array_equal(out, ref.reference(hwc[::-1, ::-1], "HWC"))
        chw = ref.random_samples(rng, kind, 3 * h * w).reshape(3, h, w)
        t = to_device(chw)
        im = gz._Image(pointer(t) + (h - 1) * w * it, w, h, 3, {"u8": 0, "f32": 3}[kind], -w * it, it,
                       (ctypes.c_ssize_t * 4)(0, h * w * it, 2 * h * w * it, 0), 1)
        assert gz.lib().gz_image_pack(0, ctypes.byref(im), out.ctypes.data) == 0
        assert np.array_equal(out, ref.reference(chw[:, ::-1], "CHW"))


@check("image_pack_device_all_u16_values")
def _(gz):
    a = ref.u16_value_image()
    assert np.array_equal(gz.image_pack(to_device(a)), ref.reference(a, "HW"))


@check("image_pack_device_all_f16_bit_patterns")
def _(gz):
    a = ref.f16_value_image()
    assert np.array_equal(gz.image_pack(to_device(a)), ref.reference(a, "HW"))


@check("image_pack_device_all_la_pairs")
def _(gz):
    a = ref.la_pairs_image()
    assert np.array_equal(gz.image_pack(to_device(a)), ref.reference(a, "HWC"))
    planar = np.ascontiguousarray(a.transpose(2, 0, 1))
    assert np.array_equal(gz.image_pack(to_device(planar)), ref.reference(a, "HWC"))


@check("image_pack_device_f32_value_set")
def _(gz):
    a = ref.f32_value_image()
    want = ref.reference(a, "HW")
    assert np.array_equal(gz.image_pack(to_device(a)), want)  # four pixels per lane
    shifted = np.concatenate([np.zeros(1, np.float32), a.reshape(-1)])
    t = to_device(shifted).as_strided((320, 320), (320, 1), 1)
    assert np.array_equal(gz.image_pack(t), want)  # one load per sample


@check("image_pack_device_matches_torch_rounding")
def _(gz):
    import torch
    t = torch.rand((3, 48, 80), dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    t = t * 1.5 - 0.25
    want = (t.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    assert np.array_equal(gz.image_pack(t), want)


@check("image_pack_device_small")
def _(gz):
    """Under 32 px there is no engine: the kernel packs into a scratch buffer."""
    rng = np.random.default_rng(13)
    a = ref.random_samples(rng, "f32", 3 * 24 * 24).reshape(3, 24, 24)
    assert np.array_equal(gz.image_pack(to_device(a)), ref.reference(a, "CHW"))
    b = ref.random_samples(rng, "u8", 1).reshape(1, 1)
    assert np.array_equal(gz.image_pack(to_device(b)), ref.reference(b, "HW"))
    c = ref.random_samples(rng, "u16", 31 * 64 * 2).reshape(31, 64, 2)
    assert np.array_equal(gz.image_pack(to_device(c)), ref.reference(c, "HWC"))
    crop = to_device(a)[:, 3:20, 5:9]  # planar, rows and planes far apart
    assert np.array_equal(gz.image_pack(crop, layout="CHW"), ref.reference(a[:, 3:20, 5:9], "CHW"))
    p = gz.Params.for_quality(95)
    assert gz.process_image(to_device(a), p) == gz.process(ref.reference(a, "CHW"), 24, 24, p)


_images = {}


def image(name):
    if name not in _images:
        e = MANIFEST["e2e"][name]
        a = np.fromfile(os.path.join(GOLDEN, e["input"]), np.uint8).reshape(e["h"], e["w"], 3)
        a.setflags(write=False)
        _images[name] = (e, a)
    return _images[name]


def form(name, kind):
    """(tensor, keyword arguments) of the manifest image in one input form."""
    _, a = image(name)
    chw = a.transpose(2, 0, 1)
    if kind == "chw_u8":
        return to_device(chw), {}
    if kind == "hwc_bgr_u8":
        return to_device(a[..., ::-1]), {"order": "BGR"}
    if kind == "chw_f32":
        return to_device(chw.astype(np.float32) / np.float32(255)), {}
    if kind == "chw_f16":
        return to_device((chw.astype(np.float32) / np.float32(255)).astype(np.float16)), {}
    if kind == "hwc_u16":
        return to_device(a.astype(np.uint16) * np.uint16(257)), {}
    rgba = np.ones(a.shape[:2] + (4,), np.float32)
    rgba[..., :3] = a.astype(np.float32) / np.float32(255)
    return to_device(rgba), {}


def known_answer(gz, name, kind):
    e, _ = image(name)
    t, kw = form(name, kind)
    data, st = gz.process_image(t, gz.Params.for_quality(95), return_stats=True, **kw)
    assert (sha(data), st.iterations) == (e["sha256"], e["iters"])


for _name in CASES:
    for _form in FORMS:
        check("process_image_known_answers-%s-%s" % (_name, _form))(
            lambda gz, n=_name, k=_form: known_answer(gz, n, k))


@check("process_image_gray")
def _(gz):
    g = ref.random_samples(np.random.default_rng(17), "u8", 48 * 64).reshape(48, 64)
    p = gz.Params.for_quality(95)
    t = to_device(g)
    pack = gz.image_pack(t)
    assert np.array_equal(pack, ref.reference(g, "HW"))
    assert gz.process_image(t, p) == gz.process(pack, 64, 48, p)


@check("queue_mixed_layouts")
def _(gz):
    p = gz.Params.for_quality(95)
    work = [(n, k) for k in ("chw_u8", "chw_f32", "hwc_bgr_u8", "hwc_u16") for n in CASES]
    with gz.Encoder(in_flight=4) as enc:
        jobs = []
        for i, (n, k) in enumerate(work):
            t, kw = form(n, k)
            jobs.append(enc.submit_image(t, p, tag=100 + i, **kw))
            jobs.append(enc.submit(to_device(image(n)[1]), p, tag=200 + i))
        for i, (n, k) in enumerate(work):
            t, kw = form(n, k)
            want = gz.process_image(t, p, **kw)
            assert sha(want) == MANIFEST["e2e"][n]["sha256"], (n, k)
            for job, tag in ((jobs[2 * i], 100 + i), (jobs[2 * i + 1], 200 + i)):
                assert job.result() == want and job.tag == tag, (n, k, tag)
        assert list(enc.results()) == []


@check("device_mismatch")
def _(gz):
    t = to_device(np.zeros((3, 40, 48), np.uint8))
    for call in (gz.image_pack, gz.process_image):
        try:
            call(t, device=1)
            raise AssertionError("a tensor of device 0 was accepted for device 1")
        except gz.GuetzliError as err:
            assert err.status == 1 and "device" in str(err)


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
