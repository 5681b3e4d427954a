"""The 8-bit image P that an encode of a gz_image starts from, stated in
numpy from its definition (include/guetzli_hip.h, gz_image), and the value
sets and views that tests/test_image_host.py and tests/image_gpu_child.py
share.  No tolerance anywhere: P is defined bit for bit.

  q(u8) = s        q(u16) = s >> 8
  q(f32) = 0 for NaN, else rint(min(max(s, 0), 1) * 255) -- one f32 product,
           round to nearest even
  q(f16) = q(f32) of the exactly widened value
  3 channels: (q R, q G, q B);  4: each blended on black with q A;
  1: R = G = B = q V;  2: R = G = B = blend(q V, q A)."""
import numpy as np

DTYPES = {"u8": np.uint8, "u16": np.uint16, "f16": np.float16, "f32": np.float32}
DEFAULT_ORDER = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}


def quant(a):
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a.copy()
    if a.dtype == np.uint16:
        return (a >> 8).astype(np.uint8)
    assert a.dtype in (np.float16, np.float32), a.dtype
    x = a.astype(np.float32)  # (exact for f16)
    with np.errstate(invalid="ignore"):
        t = np.minimum(np.maximum(x, np.float32(0)), np.float32(1))
    t = np.where(np.isnan(x), np.float32(0), t)
    prod = t * np.float32(255)
    assert prod.dtype == np.float32
    return np.rint(prod).astype(np.uint8)


def blend(v, a):
    return ((v.astype(np.int64) * a.astype(np.int64) + 128) // 255).astype(np.uint8)


def reference(view, layout, order=None):
    """P (h, w, 3) of `view` by plain indexing of the view itself."""
    view = np.asarray(view)
    if layout == "HW":
        planes = [view]
    elif layout == "HWC":
        planes = [view[:, :, i] for i in range(view.shape[2])]
    else:
        planes = [view[i] for i in range(view.shape[0])]
    order = order or DEFAULT_ORDER[len(planes)]
    q = {ch: quant(p) for ch, p in zip(order, planes)}
    if "L" in q:
        v = blend(q["L"], q["A"]) if "A" in q else q["L"]
        return np.stack([v, v, v], axis=-1)
    rgb = [q[ch] for ch in "RGB"]
    if "A" in q:
        rgb = [blend(p, q["A"]) for p in rgb]
    return np.stack(rgb, axis=-1)


def random_samples(rng, kind, n):
    """n samples that exercise q: every integer value range, floats on both
    sides of [0, 1]."""
    if kind == "u8":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "u16":
        return rng.integers(0, 65536, n, dtype=np.uint16)
    return rng.uniform(-0.25, 1.25, n).astype(DTYPES[kind])


def strided(buf, layout, h, w, c, row, off, plane=0):
    """A view of the 1-D sample buffer `buf` in `layout`, `off` samples in,
    rows `row` samples apart (CHW: planes `plane` samples apart)."""
    it = buf.itemsize
    b = buf[off:]
    if layout == "HW":
        return np.lib.stride_tricks.as_strided(b, (h, w), (row * it, it))
    if layout == "HWC":
        return np.lib.stride_tricks.as_strided(b, (h, w, c), (row * it, c * it, it))
    return np.lib.stride_tricks.as_strided(b, (c, h, w), (plane * it, row * it, it))


def strided_need(layout, h, w, c, row, off, plane=0):
    """Samples a buffer needs for strided(...)."""
    if layout == "CHW":
        return off + (c - 1) * plane + (h - 1) * row + w
    return off + (h - 1) * row + w * (c if layout == "HWC" else 1)


def f32_value_set():
    """Every tie (k + 0.5) / 255 with both f32 neighbours, every a / 255, the
    special values, and 10^5 random bit patterns (fixed seed)."""
    k = (np.arange(255, dtype=np.float32) + np.float32(0.5)) / np.float32(255)
    ties = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2))])
    exact = np.arange(256, dtype=np.float32) / np.float32(255)
    tiny = np.array([1, 2, 0x7fffff, 0x800001, 0x807fffff], np.uint32).view(np.float32)  # subnormals
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 2.0, 1.0, 0.5], np.float32)
    rnd = np.random.default_rng(20240607).integers(0, 1 << 32, 100000, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([ties, exact, tiny, special, rnd.view(np.float32)]).astype(np.float32)


def f32_value_image():
    """The f32 value set as a gray image (320 x 320, zero padded)."""
    v = f32_value_set()
    img = np.zeros(320 * 320, np.float32)
    assert v.size <= img.size
    img[:v.size] = v
    return img.reshape(320, 320)


def u16_value_image():
    return np.arange(65536, dtype=np.uint16).reshape(256, 256)


def f16_value_image():
    return np.arange(65536, dtype=np.uint16).view(np.float16).reshape(256, 256)


def la_pairs_image():
    """All 256 x 256 (v, a) pairs as an (h, w, 2) u8 image."""
    v = np.zeros((256, 256, 2), np.uint8)
    v[..., 0] = np.arange(256)[None, :]
    v[..., 1] = np.arange(256)[:, None]
    return v
