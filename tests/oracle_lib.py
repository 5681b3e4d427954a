"""ctypes binding of the CPU oracle (oracle/gz_oracle.c) and fixture readers.

Test infrastructure: only tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg import this module.
"""
import atexit
import ctypes
import hashlib
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ORACLE_SO = os.path.join(ROOT, "oracle", "_build", "libgz_oracle.so")
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "guetzli_ref")

_lib = None


class CoeffData(ctypes.Structure):
    _fields_ = [("idx", ctypes.c_int), ("block_err", ctypes.c_float)]


COEFF_DTYPE = np.dtype([("idx", "<i4"), ("block_err", "<f4")])


def build_oracle():
    if not os.path.exists(ORACLE_SO):
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "oracle"], check=True,
                       stdout=subprocess.DEVNULL)


def lib():
    global _lib
    if _lib is None:
        build_oracle()
        L = ctypes.CDLL(ORACLE_SO)
        P = np.ctypeslib.ndpointer
        f32 = P(np.float32, flags="C")
        f64 = P(np.float64, flags="C")
        u8 = P(np.uint8, flags="C")
        i16 = P(np.int16, flags="C")
        i32 = P(np.int32, flags="C")
        sz = ctypes.c_size_t
        L.gzo_init.restype = None
        L.gzo_block_idct.argtypes = [i16, u8]
        L.gzo_coeffs_to_srgb.argtypes = [ctypes.c_int, ctypes.c_int, i16, u8]
        L.gzo_srgb_to_linear_planes.argtypes = [ctypes.c_int, ctypes.c_int, u8, f32]
        L.gzo_blur.argtypes = [sz, sz, f32, ctypes.c_float, ctypes.c_float]
        L.gzo_opsin_dynamics.argtypes = [sz, sz, f32]
        L.gzo_mask_high_intensity_change.argtypes = [sz, sz, f32, f32, f32, f32]
        L.gzo_mask.argtypes = [sz, sz, f32, f32, f32, f32]
        L.gzo_diffmap.argtypes = [sz, sz, f32, f32, f32, ctypes.c_void_p]
        L.gzo_diffmap.restype = ctypes.c_int
        L.gzo_compare.argtypes = [ctypes.c_int, ctypes.c_int, u8, i16, f32]
        L.gzo_compare.restype = ctypes.c_float
        L.gzo_block_diff_double.argtypes = [f64, f64, f64, f64, f64]
        L.gzo_sort_pairs.argtypes = [i32, f32, ctypes.c_int]
        L.gzo_block_zeroing_orders.argtypes = [ctypes.c_int, ctypes.c_int, u8, f32, i16, i16,
                                               ctypes.c_float, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_void_p]
        L.gzo_compare_block.argtypes = [ctypes.c_int, ctypes.c_int, u8, f32, ctypes.c_int, i16]
        L.gzo_compare_block.restype = ctypes.c_double
        L.gzo_srgb8_to_linear.argtypes = [ctypes.c_int]
        L.gzo_srgb8_to_linear.restype = ctypes.c_double
        L.gzo_idct_matrix.argtypes = []
        L.gzo_idct_matrix.restype = ctypes.POINTER(ctypes.c_int)
        L.gzo_init()
        _lib = L
    return _lib


class Stages(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in
                ("mhic0", "mhic1", "edge", "block_dc", "block_ac", "block_ac_lf", "mask",
                 "mask_dc", "combined")]


def fixture_cases():
    return sorted(d[len("stages_"):] for d in os.listdir(GOLDEN) if d.startswith("stages_"))


_derived_dir = None  # this process's copies of the hashed fixtures' planes


def _derived_path(case, name):
    global _derived_dir
    if _derived_dir is None:
        _derived_dir = tempfile.mkdtemp(prefix="gz_fixture_")
        atexit.register(shutil.rmtree, _derived_dir, True)
    os.makedirs(os.path.join(_derived_dir, case), exist_ok=True)
    return os.path.join(_derived_dir, case, name)


class Fixture:
    """Reader for one tests/golden/stages_<case>/ directory.

    A directory with a sha256.txt is a hashed fixture: of the reference's
    dump it keeps the input, the coefficients, the block weights and meta.txt
    as files and every float plane and zeroing order only as the sha256 of the
    reference's bytes (they are 95 % of a dump's size).  path() of such a
    name forms the plane with the CPU oracle, fails unless its bytes hash to
    the reference's, and hands out a file with exactly those bytes -- so a
    reader sees the reference's dump, byte for byte, or an error."""

    def __init__(self, case):
        self.case = case
        self.dir = os.path.join(GOLDEN, "stages_" + case)
        self.hashes = {}
        if os.path.exists(os.path.join(self.dir, "sha256.txt")):
            self.hashes = dict(line.split() for line in open(os.path.join(self.dir, "sha256.txt")))
        meta = {}
        for line in open(os.path.join(self.dir, "meta.txt")):
            k, v = line.split()
            meta[k] = v
        self.meta = meta
        self.w, self.h = int(meta["w"]), int(meta["h"])
        self.target = float(meta["target"])
        self.bw, self.bh = (self.w + 7) // 8, (self.h + 7) // 8
        self.nb = self.bw * self.bh
        self.rw, self.rh = (self.w + 2) // 3, (self.h + 2) // 3

    def path(self, name):
        if name not in self.hashes:
            return os.path.join(self.dir, name)
        out = _derived_path(self.case, name)
        if not os.path.exists(out):
            self._derive(name)
        return out

    def _store(self, name, arr):
        data = np.ascontiguousarray(arr).tobytes()
        assert hashlib.sha256(data).hexdigest() == self.hashes[name], (
            "stages_%s/%s: the oracle's bytes differ from the reference's (sha256)" % (self.case, name))
        with open(_derived_path(self.case, name), "wb") as f:
            f.write(data)

    def _derive(self, name):
        L = lib()
        w, h, n = self.w, self.h, self.w * self.h
        rgb = self.rgb()
        zo = re.match(r"zero_order(?:_la(\d+)_m(\d+)_nm(\d+))?\.bin$", name)
        if zo:
            la, mask, new_model = [int(v) for v in zo.groups()] if zo.group(1) else (3, 7, 1)
            out = np.zeros(self.nb * 192, COEFF_DTYPE)
            L.gzo_block_zeroing_orders(w, h, rgb, self.f32("ref_mask.f32"), self.i16("cand_coeffs.i16"),
                                       self.i16("orig_coeffs.i16"), ctypes.c_float(self.target), la, mask,
                                       new_model, out.ctypes.data)
            self._store(name, out)
            return
        # every plane of one Compare, and the reference's mask against itself
        st = oracle_compare_planes(w, h, rgb, self.i16("cand_coeffs.i16"))
        assert np.float32(st.pop("distance")) == np.float32(self.meta["distance"]), self.case
        m = np.zeros(3 * n, np.float32)
        L.gzo_mask(w, h, st["ref_xyb"].copy(), st["ref_xyb"].copy(), m, np.zeros(3 * n, np.float32))
        st["ref_mask"] = m
        for k, arr in st.items():
            f = "cand_srgb.u8" if k == "cand_srgb" else k + ".f32"
            if f in self.hashes:
                self._store(f, arr)
        assert os.path.exists(_derived_path(self.case, name)), name

    def f32(self, name):
        return np.fromfile(self.path(name), dtype=np.float32)

    def planes(self, name):
        return self.f32(name).reshape(3, self.h, self.w)

    def i16(self, name):
        return np.fromfile(self.path(name), dtype=np.int16)

    def rgb(self):
        return np.fromfile(self.path("input.rgb"), dtype=np.uint8)

    def zero_order(self, variant=None):
        """zero_order.bin, or the (lookahead, comp_mask, new_model) variant
        zero_order_la<L>_m<M>_nm<N>.bin (make_fixtures.py zero-variants)."""
        name = "zero_order.bin" if variant is None else "zero_order_la%d_m%d_nm%d.bin" % variant
        return np.fromfile(self.path(name), dtype=COEFF_DTYPE).reshape(self.nb, 192)


def oracle_compare_planes(w, h, rgb, coeffs):
    """One Compare on the CPU oracle, stage by stage (the chain
    test_oracle_compare_stages_bit_exact pins against the reference):
    gzo_coeffs_to_srgb -> gzo_srgb_to_linear_planes -> gzo_opsin_dynamics ->
    gzo_diffmap with a Stages struct.  Returns every plane the device's
    compare_stages() returns, under the same names, the reference image's
    "ref_xyb", the candidate's "cand_srgb" bytes and "distance"."""
    L = lib()
    n = w * h
    rn = ((w + 2) // 3) * ((h + 2) // 3)
    rgb = np.ascontiguousarray(rgb, np.uint8).ravel()
    coeffs = np.ascontiguousarray(coeffs, np.int16).ravel()
    ref = np.zeros(3 * n, np.float32)
    L.gzo_srgb_to_linear_planes(w, h, rgb, ref)
    L.gzo_opsin_dynamics(w, h, ref)
    srgb = np.zeros(3 * n, np.uint8)
    L.gzo_coeffs_to_srgb(w, h, coeffs, srgb)
    cand = np.zeros(3 * n, np.float32)
    L.gzo_srgb_to_linear_planes(w, h, srgb, cand)
    out = {"ref_xyb": ref.copy(), "cand_srgb": srgb, "cand_linear": cand.copy()}
    L.gzo_opsin_dynamics(w, h, cand)
    out["cand_xyb"] = cand.copy()
    sizes = dict(mhic0=3 * n, mhic1=3 * n, edge=3 * rn, block_dc=3 * rn, block_ac=3 * rn,
                 block_ac_lf=3 * rn, mask=3 * n, mask_dc=3 * n, combined=rn)
    arrs = {k: np.zeros(v, np.float32) for k, v in sizes.items()}
    st = Stages(**{k: a.ctypes.data for k, a in arrs.items()})
    dm = np.zeros(n, np.float32)
    if L.gzo_diffmap(w, h, ref, cand, dm, ctypes.addressof(st)) != 1:
        raise RuntimeError("gzo_diffmap failed")
    out.update(arrs)
    out["distmap"] = dm
    out["distance"] = L.gzo_compare(w, h, rgb, coeffs, np.zeros(n, np.float32))
    return out


def idct_column_wrap_share(coeffs):
    """Share of the IDCT's column-pass outputs that leave int16, over the
    blocks of `coeffs` (dequantized, natural order, any shape of whole
    blocks).  ComputeBlockIDCT (idct.cc:139-149) stores (sum_u M[8 y + u] *
    block[8 u + x] + 1024) >> 11 in a coeff_t, which wraps outside [-32768,
    32767]; here the same sums in int64 with the oracle's copy of the matrix.
    (For |coefficient| <= 4096 a sum is at most 8 * 11363 * 4096 < 2^29, so
    the reference's 32-bit sum is this one.)"""
    m = np.ctypeslib.as_array(lib().gzo_idct_matrix(), (64,)).reshape(8, 8).astype(np.int64)
    b = np.asarray(coeffs).astype(np.int64).reshape(-1, 8, 8)  # [block][u][x]
    col = (np.einsum("yu,bux->byx", m, b) + 1024) >> 11
    return float(((col < -32768) | (col > 32767)).mean())


SQRT_DOMAIN = 2.0 ** 96  # sqrt_cr_big is correctly rounded on [0, 2^96) (tests/native/sqrt_check.hip)


def block_diff_sqrt_operand_bound(m):
    """Upper bound of every operand k_block_diff2 hands to sqrt_cr_big, given
    m >= |v| for every value v of the MHIC planes (mhic0, mhic1).

    The Y operands (butteraugli_kernels.inc, bd2_half / bd_columns_part):
      - fill() stages t = a + b or a - b of two MHIC values: |t| <= 2 m (2 m is
        a float when m is, so rounding cannot pass it);
      - the row and column 8-point FFTs (real_fft8, fft8_inplace) are
        unnormalised, run on the unhalved tile: each of re, im of a bin of the
        8x8 window is sum_{y,x} c t with |c| <= 1, so |re|, |im| <= 64 * 2 m =
        128 m in exact arithmetic.  Every intermediate is such a sum over a
        subset, so each of the fewer than 100 roundings on the way adds at
        most 2^-24 * 128 m: the computed values stay below 128 m (1 + 2^-17);
      - v = (re * re + im * im) * kBdVScaleY with kBdVScaleY = 0.000064f *
        0.25f * 2^32: v <= 2 (128 m)^2 * 0.000016 * 2^32 * (1 + 2^-16), the
        last factor covering the squares of the above and v's three roundings.
    So the operand is below 2^96 while m < 5.9e9; the planes hold a few
    hundred at most."""
    m = float(m)
    return 2.0 * (128.0 * m) ** 2 * (float(np.float32(0.000064)) * 0.25 * 2.0 ** 32) * (1.0 + 2.0 ** -16)


# (lookahead, comp_mask, new_zeroing_model) of the committed zeroing variants
ZERO_VARIANTS = [(3, 7, 1), (1, 7, 1), (2, 7, 1), (3, 1, 1), (3, 6, 1), (3, 7, 0), (2, 6, 0)]
