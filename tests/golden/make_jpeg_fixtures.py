#!/usr/bin/env python3
"""JPEG-input fixtures: input JPEG files and the reference's answers on them
(guetzli::Process(params, stats, jpeg, out), processor.cc:1029-1066, `--c`
mode, through oracle/_ref/guetzli_ref).  Build container only (needs PIL to
make the inputs and the reference build); writes tests/golden/jpeg/*.jpg and
tests/golden/manifest.json["jpeg"].

  python tests/golden/make_jpeg_fixtures.py            every input
  python tests/golden/make_jpeg_fixtures.py crafted    the crafted_* inputs only
                                                       (no PIL; the other entries stay)

Per input: sha256 of the reference decoder's RGB (DecodeJpegToRGB) and of its
quantized coefficients (ReadJpeg), and the encode's bytes sha256 + iteration
count at the given quality (or "reference_ok": false if the reference
rejects it).
"""
import hashlib
import io
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "guetzli-cuda-opencl_amd", "python"))
import guetzli_amd  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "guetzli_ref")
OUT_DIR = os.path.join(HERE, "jpeg")


def pil_jpeg(rgb, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", **kw)
    return buf.getvalue()


def inputs():
    from PIL import Image
    bees = np.fromfile(os.path.join(HERE, "bees.rgb"), np.uint8).reshape(258, 444, 3)
    synth = guetzli_amd.synthetic_frame(5, 160, 120)
    tiny = guetzli_amd.synthetic_frame(6, 40, 36)
    out = {
        # baseline 4:4:4, standard Huffman tables
        "bees_pil_q90_444": (pil_jpeg(bees, quality=90, subsampling=0), 95),
        # optimized Huffman tables, restart markers every 4 MCUs
        "synth_pil_q80_444_rst": (pil_jpeg(synth, quality=80, subsampling=0, optimize=True,
                                           restart_marker_blocks=4), 90),
        # above the 32-pixel Butteraugli minimum only just
        "tiny_pil_q85_444": (pil_jpeg(tiny, quality=85, subsampling=0), 95),
        # 4:2:0 and progressive: the reference handles them, this build does not
        "synth_pil_q85_420": (pil_jpeg(synth, quality=85, subsampling=2), 95),
        "synth_pil_q85_444_prog": (pil_jpeg(synth, quality=85, subsampling=0, progressive=True), 95),
        # APP1 (Exif) + COM segments, encoded with clear_metadata = false
        # (the input's APPn / COM are carried to the output)
        "synth_pil_q85_444_meta": (pil_jpeg(synth, quality=85, subsampling=0,
                                            exif=b"Exif\x00\x00MM\x00*\x00\x00\x00\x08\x00\x00",
                                            comment=b"guetzli-mi355x fixture"), 95),
    }
    # gray content in three components (R = G = B): a 4:4:4 YCbCr input the
    # reference encodes (its chroma planes carry only rounding noise); and a
    # one-component grayscale file, which the reference's ProcessJpegData
    # rejects (processor.cc:946-949: only 3-component YCbCr input)
    gray = np.repeat(bees[:120, :160, 1:2], 3, axis=2)
    out["graycontent_pil_q85_444"] = (pil_jpeg(np.ascontiguousarray(gray), quality=85,
                                               subsampling=0), 95)
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bees[:120, :160, 1])).save(buf, "JPEG", quality=85)
    out["gray1_pil_q85"] = (buf.getvalue(), 95)
    # 4:2:0 with all-zero chroma (YCbCr given directly: Cb = Cr = 128, no
    # colour conversion, so every chroma coefficient is 0): the reference
    # keeps one component and searches Y alone (processor.cc:990-1016)
    ycc = np.zeros((120, 160, 3), np.uint8)
    ycc[..., 0] = bees[:120, :160, 1]
    ycc[..., 1:] = 128
    buf = io.BytesIO()
    Image.fromarray(ycc, mode="YCbCr").save(buf, "JPEG", quality=85, subsampling=2)
    out["gray420_pil_q85"] = (buf.getvalue(), 95)
    # a guetzli output as input (SOF1, guetzli's own table layout)
    tmp = tempfile.mkdtemp()
    raw = os.path.join(tmp, "bees88.rgb")
    np.ascontiguousarray(bees[:64, :88]).tofile(raw)
    jp = os.path.join(tmp, "bees88.jpg")
    subprocess.run([REF, "encode", raw, "88", "64", "90", jp], check=True, capture_output=True)
    out["bees88_guetzli_q90"] = (open(jp, "rb").read(), 95)
    return out


# zigzag position -> natural (row-major) index of an 8x8 block (T.81 figure A.6)
NATURAL_ORDER = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def _segments(data):
    """(marker, offset of the marker's 0xff, segment length incl. the marker)
    of every segment up to and including the SOS header."""
    pos = 2
    while True:
        assert data[pos] == 0xFF, pos
        m = data[pos + 1]
        n = 2 + ((data[pos + 2] << 8) | data[pos + 3])
        yield m, pos, n
        if m == 0xDA:
            return
        pos += n


def _set_quant(data, q):
    """The file with every value of its 8-bit DQT tables replaced by q: the
    entropy-coded (in-file) values stay, what they stand for scales by q."""
    d = bytearray(data)
    for m, pos, n in _segments(data):
        if m == 0xDB:
            p = pos + 4
            while p < pos + n:
                assert d[p] >> 4 == 0, "8-bit tables"
                d[p + 1:p + 65] = bytes([q]) * 64
                p += 65
    return bytes(d)


def _repeat_mcus(data, mcus, width):
    """A file all of whose MCUs code to the same bits (written with two of
    them), re-cut to `mcus` MCUs in one row of `width` pixels."""
    segs = list(_segments(data))
    m, pos, n = segs[-1]
    scan = data[pos + n:-2].replace(b"\xff\x00", b"\xff")
    assert data[-2:] == b"\xff\xd9"
    bits = "".join("{:08b}".format(b) for b in scan)
    for pad in range(8):
        L = (len(bits) - pad) // 2
        if 2 * L + pad == len(bits) and bits[:L] == bits[L:2 * L] and set(bits[2 * L:]) <= {"1"}:
            break
    else:
        raise AssertionError("the two MCUs do not code alike")
    out = bits[:L] * mcus
    out += "1" * (-len(out) % 8)
    scan = bytes(int(out[i:i + 8], 2) for i in range(0, len(out), 8)).replace(b"\xff", b"\xff\x00")
    d = bytearray(data[:pos + n])
    for m, p, _ in segs:
        if m in (0xC0, 0xC1):
            d[p + 7:p + 9] = bytes([width >> 8, width & 255])
    return bytes(d) + scan + b"\xff\xd9"


def _set_scan_al(data, scan, al):
    """The file with the successive-approximation low bit (Al) of its
    scan-th SOS header set to `al`."""
    d = bytearray(data)
    pos, k = 2, 0
    while True:
        assert d[pos] == 0xFF and d[pos + 1] != 0xD9, "fewer scans than asked for"
        n = 2 + ((d[pos + 2] << 8) | d[pos + 3])
        if d[pos + 1] != 0xDA:
            pos += n
            continue
        if k == scan:
            d[pos + n - 1] = (d[pos + n - 1] & 0xF0) | al
            return bytes(d)
        k += 1
        pos += n  # then the entropy-coded bytes, up to the next marker
        while not (d[pos] == 0xFF and d[pos + 1] != 0 and not 0xD0 <= d[pos + 1] <= 0xD7):
            pos += 1


def crafted_inputs():
    """Inputs on the coefficient range CheckJpegSanity admits (|value x quant|
    <= 4096, four times what 8-bit pixels give) and just past the reader's
    and the sanity check's limits, written with the library's own host writer
    from stored (value x quant) coefficients.  64 x 48 unless noted."""
    w, h = 64, 48
    nb = (w // 8) * (h // 8)
    W = guetzli_amd.write_jpeg_host
    out = {}

    def walk(rng, lim, shape):
        # a random walk with steps <= 900, clipped to [-lim, lim]: in-file DC
        # differences stay within the reader's 11 bits
        dc = np.zeros(shape, np.int64)
        for c in range(shape[0]):
            v = 0
            for b in range(shape[1]):
                v = int(np.clip(v + rng.integers(-900, 901), -lim, lim))
                dc[c, b] = v
        return dc

    q4 = np.full((3, 64), 4, np.int32)
    rng = np.random.default_rng(4096)
    co = (rng.integers(0, 2, size=(3, nb, 64)) * 2 - 1) * 4096
    co[:, 0::2, 0] = 4096    # in-file 1024, -1023, 1024, ...: differences of +-2047,
    co[:, 1::2, 0] = -4092   # the largest a DC symbol of 11 bits carries
    out["crafted_pm4096_q4"] = (W(co.astype(np.int16), q4, w, h), 95)

    rng = np.random.default_rng(4097)
    co = rng.integers(-1024, 1025, size=(3, nb, 64))
    co[:, :, 0] = walk(rng, 1024, (3, nb))
    out["crafted_noise4096_q4"] = (W((4 * co).astype(np.int16), q4, w, h), 95)

    rng = np.random.default_rng(2047)
    co = rng.integers(-2047, 2048, size=(3, nb, 64))
    co[:, :, 0] = walk(rng, 2047, (3, nb))
    out["crafted_2047_q2"] = (W((2 * co).astype(np.int16), np.full((3, 64), 2, np.int32), w, h), 95)
    # the same values at quant 1: an all-ones input, which the search keeps
    # and codes as the original (size-11 symbols)
    ones = np.ones((3, 64), np.int32)
    out["crafted_2047_q1"] = (W(co.astype(np.int16), ones, w, h), 95)

    # a natural image quantized by a table of 2..24 (2 at the DC, 3..24 along
    # the zigzag), one AC coefficient per block and component replaced by
    # +-(4096 // q) * q: a search with outliers at the domain's edge
    bw, bh = 88, 64
    rgb = np.fromfile(os.path.join(HERE, "edge", "gray_bees_88x64.rgb"), np.uint8)
    raw = guetzli_amd.rgb_to_coeffs(rgb, bw, bh).reshape(3, -1, 64).astype(np.int64)
    q = np.zeros(64, np.int64)
    for z, n in enumerate(NATURAL_ORDER):
        q[n] = 2 if z == 0 else 3 + 21 * z // 63
    assert q.min() == 2 and q.max() == 24
    co = np.round(raw / q).astype(np.int64) * q
    rng = np.random.default_rng(88)
    for c in range(3):
        for b in range(co.shape[1]):
            k = int(rng.integers(1, 64))
            co[c, b, k] = int(rng.choice([-1, 1])) * (4096 // q[k]) * q[k]
    assert np.abs(co).max() <= 4096 and np.abs(co // q)[:, :, 1:].max() < 2048
    out["crafted_bees_outliers"] = (W(co.astype(np.int16), np.tile(q, (3, 1)).astype(np.int32), bw, bh), 95)

    # ---- refused by the reference
    co = np.zeros((3, nb, 64), np.int16)
    co[0, 5, 9] = 2048  # an AC symbol of size 12 (JPEG_NON_REPRESENTABLE_AC_COEFF)
    out["crafted_ac_size12"] = (W(co, ones, w, h), 95)
    co = np.zeros((3, nb, 64), np.int16)
    co[:, 0::2, 0] = 1024  # DC differences of +-2048: a DC symbol of 12 (JPEG_INVALID_SYMBOL)
    co[:, 1::2, 0] = -1024
    out["crafted_dc_size12"] = (W(co, ones, w, h), 95)
    # in-file 1025 at quant 4 = 4100: readable, refused by CheckJpegSanity.
    # Written at quant 1 (the writer takes no stored value past 4096), then
    # the tables set to 4.
    co = np.zeros((3, nb, 64), np.int16)
    co[1, 7, 1] = 1025
    co[:, :, 0] = 16
    out["crafted_sanity_4100"] = (_set_quant(W(co, ones, w, h), 4), 95)
    # 136 x 8: every DC difference 2047, so the 17th block's DC is 34799,
    # which coeff_t cannot hold (JPEG_NON_REPRESENTABLE_DC_COEFF).  No stored
    # coefficient says that, so the scan is the two-block file's MCU 17 times.
    co = np.zeros((3, 2, 64), np.int16)
    co[:, 0, 0], co[:, 1, 0] = 2047, 4094
    two = W(co, ones, 16, 8)
    ok16 = guetzli_amd.jpeg_decode(_repeat_mcus(two, 16, 128))[3].reshape(3, 16, 64)
    assert (ok16[:, :, 0] == 2047 * np.arange(1, 17)).all() and not ok16[:, :, 1:].any()
    out["crafted_dc_overflow"] = (_repeat_mcus(two, 17, 136), 95)
    # progressive scans, where the point transform counts: the committed
    # progressive input (scan 0: DC of all components, Al 1; scan 1: Y 1..5,
    # Al 2) with those Al set to 11 (the reference takes no Al above 10,
    # jpeg_data_reader.cc:811) and to 10 (s + Al >= 12 from s = 2 on)
    prog = open(os.path.join(OUT_DIR, "synth_pil_q85_444_prog.jpg"), "rb").read()
    out["crafted_prog_dc_al11"] = (_set_scan_al(prog, 0, 11), 95)
    out["crafted_prog_ac_al10"] = (_set_scan_al(prog, 1, 10), 95)
    return out


def main():
    os.makedirs(OUT_DIR, exist_ok=True)
    man_path = os.path.join(HERE, "manifest.json")
    man = json.load(open(man_path))
    crafted_only = sys.argv[1:] == ["crafted"]
    entries = {k: v for k, v in man.get("jpeg", {}).items() if crafted_only and not k.startswith("crafted_")}
    todo = dict(crafted_inputs())
    if not crafted_only:
        todo.update(inputs())
    tmp = tempfile.mkdtemp()
    for name, (data, quality) in sorted(todo.items()):
        path = os.path.join(OUT_DIR, name + ".jpg")
        open(path, "wb").write(data)
        e = {"input": "jpeg/%s.jpg" % name, "quality": quality,
             "input_sha256": hashlib.sha256(data).hexdigest()}
        rgb_p, co_p = os.path.join(tmp, "d.rgb"), os.path.join(tmp, "d.co")
        r = subprocess.run([REF, "decode", path, rgb_p, co_p], capture_output=True, text=True)
        if r.returncode == 0:
            info = json.loads(r.stdout)
            e.update(w=info["w"], h=info["h"], ncomp=info["ncomp"],
                     rgb_sha256=hashlib.sha256(open(rgb_p, "rb").read()).hexdigest(),
                     coeffs_sha256=hashlib.sha256(open(co_p, "rb").read()).hexdigest())
        out_p = os.path.join(tmp, "o.jpg")
        keep = name.endswith("_meta")
        if keep:
            e["clear_metadata"] = False
        r = subprocess.run([REF, "encode_jpeg", path, str(quality), out_p] + (["keep"] if keep else []),
                           capture_output=True, text=True)
        e["reference_ok"] = r.returncode == 0
        if r.returncode == 0:
            info = json.loads(r.stdout)
            e.update(sha256=hashlib.sha256(open(out_p, "rb").read()).hexdigest(),
                     bytes=info["bytes"], iters=info["iters"])
        entries[name] = e
        print(name, json.dumps(e))
    man["jpeg"] = entries
    json.dump(man, open(man_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
