"""JPEG input: guetzli::Process on a JPEG file (processor.cc:1029-1066).

The reader (ReadJpeg, jpeg_data_reader.cc) and the 4:4:4 decode
(DecodeJpegToRGB, jpeg_data_decoder.cc:45-55) are host code, checked on the
CPU against the reference's own answers on the committed inputs
(tests/golden/jpeg/, made by tests/golden/make_jpeg_fixtures.py: baseline,
optimized-Huffman with restart markers, progressive, 4:2:0, a guetzli
output): sha256 of the quantized coefficients and of the decoded RGB.  The
encode itself runs on the GPU and must reproduce the reference's bytes.

The crafted_* inputs carry coefficients no 8-bit image gives: dense values at
CheckJpegSanity's limit (|value x quant| <= 4096, four times the range of
pixel-derived coefficients), which the reference reads and encodes, and files
just past the reader's limits (an AC or DC symbol of 12 bits, a DC that
coeff_t cannot hold) or the sanity check's, which it refuses -- each at the
stage the manifest records (no rgb_sha256: the reference's decode failed).
"""
import hashlib
import json
import os

import numpy as np
import pytest

import guetzli_amd as gz

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = json.load(open(os.path.join(GOLDEN, "manifest.json")))["jpeg"]


def _data(name):
    return open(os.path.join(GOLDEN, CASES[name]["input"]), "rb").read()


def _sha(b):
    return hashlib.sha256(b).hexdigest()


CRAFTED_OK = ["crafted_2047_q1", "crafted_2047_q2", "crafted_bees_outliers", "crafted_noise4096_q4",
              "crafted_pm4096_q4"]
# name -> whether the reference's decode takes the file (its encode never does)
CRAFTED_REFUSED = {"crafted_ac_size12": False, "crafted_dc_size12": False, "crafted_dc_overflow": False,
                   "crafted_prog_ac_al10": False, "crafted_prog_dc_al11": False, "crafted_sanity_4100": True}


def test_crafted_known_answers_present():
    """The crafted inputs are in the manifest with the reference's verdicts:
    bytes and iteration count where it encodes, and for a refused file
    whether its decode still succeeded."""
    for name in CRAFTED_OK:
        e = CASES[name]
        assert e["reference_ok"] and e["iters"] >= 1 and e["bytes"] > 0 and len(e["sha256"]) == 64, name
        assert len(e["rgb_sha256"]) == 64 and len(e["coeffs_sha256"]) == 64, name
        assert os.path.exists(os.path.join(GOLDEN, e["input"])), name
    for name, decodes in CRAFTED_REFUSED.items():
        e = CASES[name]
        assert not e["reference_ok"] and "sha256" not in e, name
        assert ("rgb_sha256" in e) == decodes, name
        assert os.path.exists(os.path.join(GOLDEN, e["input"])), name
    assert sorted(n for n in CASES if n.startswith("crafted_")) == sorted(CRAFTED_OK + list(CRAFTED_REFUSED))


# (every input the reference's decode takes; the others: test_crafted_refused_*)
@pytest.mark.parametrize("name", sorted(n for n in CASES if "coeffs_sha256" in CASES[n]))
def test_read_and_decode_match_reference(name):
    e = CASES[name]
    data = _data(name)
    assert _sha(data) == e["input_sha256"]
    w, h, nc, coeffs, rgb = gz.jpeg_decode(data)
    assert (w, h, nc) == (e["w"], e["h"], e.get("ncomp", 3))
    assert _sha(coeffs.tobytes()) == e["coeffs_sha256"]
    # (4:2:0 via the fancy upsampler; a one-component file decodes to no RGB,
    # as DecodeJpegToRGB returns an empty vector)
    assert _sha(b"" if rgb is None else rgb.tobytes()) == e["rgb_sha256"]


def test_progressive_input_decodes_ac_coefficients():
    # the progressive file's AC bands come from first + refinement scans
    w, h, _, co, rgb = gz.jpeg_decode(_data("synth_pil_q85_444_prog"))
    assert rgb.shape == (h, w, 3)
    assert (co.reshape(3, -1, 64)[:, :, 1:] != 0).any()


@pytest.mark.parametrize("bad", [b"", b"\xff\xd8", b"not a jpeg at all",
                                 "truncated", "no_eoi_scan"])
def test_reader_rejects_invalid_input(bad):
    if bad == "truncated":
        bad = _data("bees_pil_q90_444")[:600]
    elif bad == "no_eoi_scan":
        d = _data("tiny_pil_q85_444")
        bad = d[:d.index(b"\xff\xda")]  # headers only
    with pytest.raises(gz.GuetzliError) as ei:
        gz.jpeg_decode(bad)
    assert ei.value.status == 1  # GZ_ERR_INVALID_ARG


@pytest.mark.parametrize("name", sorted(CRAFTED_REFUSED))
def test_crafted_refused_at_the_reference_stage(name):
    """A crafted file the reference refuses is refused here at the same
    stage: where its decode fails (ReadJpeg: an AC symbol of s + Al >= 12,
    jpeg_data_reader.cc:589, in a sequential and in a progressive first
    scan; a DC symbol of 12; a DC coeff_t cannot hold, :556; a scan with Al
    above 10, :811) jpeg_decode raises INVALID_ARG; where only the encode fails
    (CheckJpegSanity) jpeg_decode returns the reference's coefficients and
    pixels (test_read_and_decode_match_reference) and process_jpeg is refused
    (test_process_jpeg_crafted_refused, on the GPU)."""
    e = CASES[name]
    assert not e["reference_ok"]
    data = _data(name)
    assert _sha(data) == e["input_sha256"]
    if "rgb_sha256" in e:
        w, h, _, coeffs, rgb = gz.jpeg_decode(data)
        assert _sha(coeffs.tobytes()) == e["coeffs_sha256"] and _sha(rgb.tobytes()) == e["rgb_sha256"]
    else:
        with pytest.raises(gz.GuetzliError) as ei:
            gz.jpeg_decode(data)
        assert ei.value.status == gz.GZ_ERR_INVALID_ARG
        # (the reader's reason, not a later stage's)
        reason = {"crafted_ac_size12": "out of range AC coefficient", "crafted_dc_size12": "corrupt entropy-coded",
                  "crafted_dc_overflow": "DC coefficient not representable",
                  "crafted_prog_ac_al10": "out of range AC coefficient",
                  "crafted_prog_dc_al11": "Al > 10 is not supported"}[name]
        assert reason in str(ei.value), str(ei.value)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CRAFTED_REFUSED))
def test_process_jpeg_crafted_refused(name):
    """The encode of every refused crafted file fails with INVALID_ARG, as
    the reference's Process returns false -- the sanity-check case included,
    which reads and decodes."""
    with pytest.raises(gz.GuetzliError) as ei:
        gz.process_jpeg(_data(name), gz.Params.for_quality(CASES[name]["quality"]))
    assert ei.value.status == gz.GZ_ERR_INVALID_ARG


def test_write_jpeg_host_refuses_coefficients_outside_the_coder_domain():
    """gz_write_jpeg_host takes stored coefficients of |v| <= 4096 (the
    entropy coders' domain, sized for AC symbols of 13 bits and DC differences
    of 14): 4096 and -4096 at any position are written and read back, 4097 or
    -4097 anywhere -- DC, AC, last block of the last component -- is
    INVALID_ARG."""
    w, h = 24, 16
    q4 = np.full((3, 64), 4, np.int32)
    co = np.zeros((3, 6, 64), np.int16)
    co[0, 0, 0], co[1, 3, 17], co[2, 5, 63] = 4096, 4096, -4096
    # (at quant 4 the file holds +-1024: symbols of 11 bits, which the reader takes)
    back = gz.jpeg_decode(gz.write_jpeg_host(co, q4, w, h))[3]
    assert np.array_equal(back.reshape(3, 6, 64) * 4, co)
    # at quant 1 they are symbols of 13 bits: written all the same
    assert len(gz.write_jpeg_host(co, np.ones((3, 64), np.int32), w, h)) > 0
    for pos, v in [((0, 0, 0), 4097), ((0, 0, 0), -4097), ((1, 2, 5), 4100), ((2, 5, 63), -4097),
                   ((2, 5, 63), 32767), ((0, 4, 1), -32768)]:
        bad = co.copy()
        bad[pos] = v
        with pytest.raises(gz.GuetzliError) as ei:
            gz.write_jpeg_host(bad, q4, w, h)
        assert ei.value.status == gz.GZ_ERR_INVALID_ARG and "outside [-4096, 4096]" in str(ei.value), (pos, v)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n]["reference_ok"]))
def test_process_jpeg_matches_reference(name):
    e = CASES[name]
    assert e["reference_ok"]
    params = gz.Params.for_quality(e["quality"], clear_metadata=e.get("clear_metadata", True))
    out, st = gz.process_jpeg(_data(name), params, return_stats=True)
    assert st.iterations == e["iters"]
    assert len(out) == e["bytes"]
    assert _sha(out) == e["sha256"]


@pytest.mark.gpu
def test_process_jpeg_one_component_rejected_as_reference():
    """A one-component (grayscale) JPEG: the reference's Process returns
    false (ProcessJpegData accepts only 3-component YCbCr input), and so does
    this build -- with an error, not an encode."""
    assert not CASES["gray1_pil_q85"]["reference_ok"]
    with pytest.raises(gz.GuetzliError):
        gz.process_jpeg(_data("gray1_pil_q85"), gz.Params.for_quality(95))


@pytest.mark.gpu
def test_process_jpeg_rejects_garbage():
    with pytest.raises(gz.GuetzliError) as ei:
        gz.process_jpeg(b"\xff\xd8\xff\xe0garbage", gz.Params.for_quality(95))
    assert ei.value.status == 1


def test_oversized_sof_rejected_before_allocation():
    """A ~20-byte file whose SOF declares 65535 x 65535 (67 M blocks per
    component) is JPEG_IMAGE_TOO_LARGE in the reference (more than 2^21
    blocks, jpeg_data_reader.cc:151-158): refused with INVALID_ARG before
    any coefficient memory is allocated."""
    import resource
    sof = bytes([0xFF, 0xC0, 0x00, 0x11, 0x08, 0xFF, 0xFF, 0xFF, 0xFF, 0x03,
                 0x01, 0x11, 0x00, 0x02, 0x11, 0x00, 0x03, 0x11, 0x00])
    data = b"\xff\xd8" + sof + b"\xff\xd9"
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    with pytest.raises(gz.GuetzliError) as e:
        gz.jpeg_decode(data)
    assert e.value.status == gz.GZ_ERR_INVALID_ARG
    assert "too large" in str(e.value)
    # no multi-GB allocation happened on the way (max RSS grew < 64 MB)
    assert resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - rss0 < 64 * 1024
