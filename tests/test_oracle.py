"""The CPU oracle (oracle/gz_oracle.c) against the reference's own outputs.

Pins the restatement before anything is checked against it: every stage of
the `--c` Butteraugli pass, the reference-vs-reference activity mask, the
per-block greedy zeroing orders and the libstdc++ std::sort tie order are
compared bit-for-bit with fixtures generated from oracle/_ref (the reference
compiled from /root/reference) by tests/golden/make_fixtures.py.  The x_*
fixtures are extreme inputs (black, white, checkerboards, saturated
primaries, full-range noise, ramps into 0 and 255; *_coarse: candidates a 24
times coarser quantization away), which make the oracle the reference for
the device tests that go farther still.
"""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from oracle_lib import (COEFF_DTYPE, GOLDEN, ROOT, SQRT_DOMAIN, ZERO_VARIANTS, Fixture, Stages,
                        block_diff_sqrt_operand_bound, fixture_cases, idct_column_wrap_share, lib)

CASES = fixture_cases()


def bits_equal(a, b):
    a = np.asarray(a).ravel()
    b = np.asarray(b).ravel()
    assert a.shape == b.shape
    if a.dtype == np.float32:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


@pytest.mark.parametrize("case", CASES)
def test_oracle_compare_stages_bit_exact(case):
    L = lib()
    F = Fixture(case)
    w, h, n = F.w, F.h, F.w * F.h
    rgb = F.rgb()
    ref = np.zeros(3 * n, np.float32)
    L.gzo_srgb_to_linear_planes(w, h, rgb, ref)
    L.gzo_opsin_dynamics(w, h, ref)
    assert bits_equal(ref, F.f32("ref_xyb.f32"))
    coeffs = F.i16("cand_coeffs.i16")
    srgb = np.zeros(3 * n, np.uint8)
    L.gzo_coeffs_to_srgb(w, h, coeffs, srgb)
    assert bits_equal(srgb, np.fromfile(F.path("cand_srgb.u8"), np.uint8))
    cand = np.zeros(3 * n, np.float32)
    L.gzo_srgb_to_linear_planes(w, h, srgb, cand)
    assert bits_equal(cand, F.f32("cand_linear.f32"))
    L.gzo_opsin_dynamics(w, h, cand)
    assert bits_equal(cand, F.f32("cand_xyb.f32"))
    rn = F.rw * F.rh
    sizes = dict(mhic0=3 * n, mhic1=3 * n, edge=3 * rn, block_dc=3 * rn, block_ac=3 * rn,
                 block_ac_lf=3 * rn, mask=3 * n, mask_dc=3 * n, combined=rn)
    arrs = {k: np.zeros(v, np.float32) for k, v in sizes.items()}
    st = Stages(**{k: a.ctypes.data for k, a in arrs.items()})
    dm = np.zeros(n, np.float32)
    assert L.gzo_diffmap(w, h, ref.copy(), cand.copy(), dm, ctypes.addressof(st)) == 1
    for k in sizes:
        assert bits_equal(arrs[k], F.f32(k + ".f32")), k
    assert bits_equal(dm, F.f32("distmap.f32"))
    d = L.gzo_compare(w, h, rgb, coeffs, dm)
    assert np.float32(d) == np.float32(F.meta["distance"])


@pytest.mark.parametrize("variant", ZERO_VARIANTS)
@pytest.mark.parametrize("case", CASES)
def test_oracle_block_zeroing_bit_exact(case, variant):
    """Zeroing orders for every (lookahead, comp_mask, new_zeroing_model)
    variant the reference was run with (processor.cc:376-487)."""
    L = lib()
    F = Fixture(case)
    w, h, n = F.w, F.h, F.w * F.h
    rgb = F.rgb()
    ref = np.zeros(3 * n, np.float32)
    L.gzo_srgb_to_linear_planes(w, h, rgb, ref)
    L.gzo_opsin_dynamics(w, h, ref)
    m = np.zeros(3 * n, np.float32)
    mdc = np.zeros(3 * n, np.float32)
    L.gzo_mask(w, h, ref, ref, m, mdc)
    assert bits_equal(m, F.f32("ref_mask.f32"))
    out = np.zeros(F.nb * 192, COEFF_DTYPE)
    la, mask, new_model = variant
    L.gzo_block_zeroing_orders(w, h, rgb, m, F.i16("cand_coeffs.i16"), F.i16("orig_coeffs.i16"),
                               ctypes.c_float(F.target), la, mask, new_model, out.ctypes.data)
    z = F.zero_order(None if variant == (3, 7, 1) else variant).ravel()
    assert np.array_equal(out["idx"], z["idx"])
    assert bits_equal(out["block_err"], z["block_err"])


def test_fixture_mhic_planes_inside_sqrt_domain():
    """k_block_diff2 takes its Y square roots with sqrt_cr_big on operands
    scaled by 2^32, which is correctly rounded only below 2^96.  The bound of
    those operands in terms of the largest MHIC value (oracle_lib.
    block_diff_sqrt_operand_bound, derivation there) holds on the committed
    mhic0 / mhic1 planes of every stage fixture: a new fixture that leaves the
    proven range fails here, without a device."""
    for case in CASES:
        F = Fixture(case)
        m = max(np.abs(F.f32("mhic0.f32")).max(), np.abs(F.f32("mhic1.f32")).max())
        assert np.isfinite(m), case
        bound = block_diff_sqrt_operand_bound(m)
        assert bound < SQRT_DOMAIN, "%s: max |mhic| %g gives operands up to %g" % (case, m, bound)


JPEG_CASES = json.load(open(os.path.join(GOLDEN, "manifest.json")))["jpeg"]
CRAFTED_OK = sorted(n for n in JPEG_CASES if n.startswith("crafted_") and JPEG_CASES[n]["reference_ok"])


def _crafted_dequantized(name):
    """(w, h, [3][blocks][64] dequantized coefficients) of a crafted 4:4:4
    input: gz.jpeg_decode's quantized values times the file's (uniform or
    per-position) tables, which the generator's stored values were divided by."""
    import guetzli_amd as gz
    data = open(os.path.join(GOLDEN, JPEG_CASES[name]["input"]), "rb").read()
    w, h, nc, co, _ = gz.jpeg_decode(data)
    assert nc == 3
    # the file's tables, in order of appearance: 8-bit DQT segments, zigzag order
    tables, pos = [], 2
    while data[pos + 1] != 0xDA:
        n = 2 + ((data[pos + 2] << 8) | data[pos + 3])
        if data[pos + 1] == 0xDB:
            p = pos + 4
            while p < pos + n:
                assert data[p] >> 4 == 0
                tables.append(np.frombuffer(data[p + 1:p + 65], np.uint8).astype(np.int32))
                p += 65
        pos += n
    assert tables and all((t == tables[0]).all() for t in tables), "one table for all components"
    zz = np.zeros(64, np.int32)
    for z, nat in enumerate(_NATURAL_ORDER):
        zz[nat] = tables[0][z]
    return w, h, (co.reshape(3, -1, 64).astype(np.int32) * zz).astype(np.int16)


# zigzag position -> natural index (T.81 figure A.6)
_NATURAL_ORDER = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                  41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


@pytest.mark.parametrize("name", CRAFTED_OK)
def test_oracle_pixels_match_reference_on_jpeg_range(name):
    """gzo_coeffs_to_srgb on coefficients up to +-4096 at every position --
    where the IDCT's int16 column pass wraps on up to half its outputs --
    equals the reference decoder's RGB (DecodeJpegToRGB, the manifest's
    rgb_sha256) byte for byte.  This makes the oracle the reference of the
    device tests on that range (test_gpu.py, *_jpeg_range_*)."""
    w, h, deq = _crafted_dequantized(name)
    assert np.abs(deq.astype(np.int32)).max() <= 4096
    srgb = np.zeros(3 * w * h, np.uint8)
    lib().gzo_coeffs_to_srgb(w, h, np.ascontiguousarray(deq).ravel(), srgb)
    assert hashlib.sha256(srgb.tobytes()).hexdigest() == JPEG_CASES[name]["rgb_sha256"]


def test_idct_column_wrap_only_on_jpeg_range():
    """The gap the crafted inputs close, stated on the data: the column pass
    of the IDCT keeps its outputs in int16 (coeff_t colidcts, idct.cc:140-148),
    and no candidate of any stage fixture -- all of them quantized transforms
    of 8-bit pixels -- has a single output outside int16, so an IDCT that kept
    that pass in 32 bits would pass every stage test.  On the crafted inputs
    at least 40 % (random signs x 4096; measured 51 %) and 10 % (noise to
    +-4096; measured 23 %) of the outputs wrap."""
    # the helper on blocks worked by hand: a DC of 4096 gives 8192 * 4096 >> 11 =
    # 16384 at all 64 outputs; +4096 at every u of column x = 0 gives 2 * (the
    # matrix's row sums) = 122426, -33390, 26480, -9316, 14308, -1396, 8306,
    # 3654 there and 0 elsewhere: two outputs of 64 outside int16
    one = np.zeros((8, 8), np.int16)
    one[0, 0] = 4096
    assert idct_column_wrap_share(one) == 0.0
    one[:, 0] = 4096
    assert idct_column_wrap_share(one) == 2 / 64
    for case in CASES:
        assert idct_column_wrap_share(Fixture(case).i16("cand_coeffs.i16")) == 0.0, case
    shares = {n: idct_column_wrap_share(_crafted_dequantized(n)[2]) for n in CRAFTED_OK}
    print("column-pass wrap shares:", {k: round(v, 4) for k, v in shares.items()})
    assert shares["crafted_pm4096_q4"] >= 0.40
    assert shares["crafted_noise4096_q4"] >= 0.10


SORT_HARNESS = r"""
#include <algorithm>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>
extern "C" void gzo_sort_pairs(int* idx, float* key, int n);
int main() {
  std::mt19937 rng(12345);
  for (int t = 0; t < 4000; ++t) {
    int n = rng() % 200;
    int levels = 1 + rng() % (t % 3 == 0 ? 3 : 40);  // many ties in a third of the cases
    std::vector<std::pair<int, float>> v(n);
    std::vector<int> idx(n);
    std::vector<float> key(n);
    for (int i = 0; i < n; ++i) {
      v[i] = {i, static_cast<float>(rng() % levels) * 0.25f};
      idx[i] = v[i].first;
      key[i] = v[i].second;
    }
    if (t % 7 == 0) std::sort(v.begin(), v.end(), [](auto& a, auto& b) { return a.second > b.second; });
    for (int i = 0; i < n; ++i) { idx[i] = v[i].first; key[i] = v[i].second; }
    std::sort(v.begin(), v.end(), [](const std::pair<int, float>& a, const std::pair<int, float>& b) {
      return a.second < b.second; });
    gzo_sort_pairs(idx.data(), key.data(), n);
    for (int i = 0; i < n; ++i)
      if (idx[i] != v[i].first) { std::printf("MISMATCH t=%d n=%d i=%d\n", t, n, i); return 1; }
  }
  std::printf("OK\n");
  return 0;
}
"""


def test_oracle_sort_matches_libstdcxx(tmp_path):
    lib()  # builds the oracle
    src = tmp_path / "sort_check.cc"
    src.write_text(SORT_HARNESS)
    exe = tmp_path / "sort_check"
    odir = os.path.join(ROOT, "oracle", "_build")
    subprocess.run(["g++", "-O2", "-std=c++17", str(src), "-o", str(exe), "-L", odir, "-lgz_oracle",
                    "-Wl,-rpath," + odir], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "OK", res.stdout
