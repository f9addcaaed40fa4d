"""Decoding to a requested colour encoding (include/jxl_hip.h "output colour": JxlHipOutputColor, JxlHipBatchSetOutputColor, JxlHipPipelineSubmitColor,
JxlHipColorConversionMatrix, JxlHipDecoderSetOutputColorProfile — which has the argument list and the contract of libjxl's JxlDecoderSetOutputColorProfile; libjxl's
own two names stay error-returning stubs, whose list tests/test_abi_host.py pins).

Where the expected values come from.
 * The matrix: BT.2087's published BT.2020 -> BT.709 matrix, and a float64 numpy restatement with its own Bradford constants and D50 (nothing of the product imported).
 * XYB images: the twin — the same pixels encoded under a header that names the target at the source's intensity target.  The synthesiser's VarDCT payload does not
   depend on the header's colour encoding (asserted: common suffix), so the decode with a target must equal the plain decode of the twin bit for bit, and the twin's
   float32 decode is the oracle's to 1 ULP, as everywhere in the suite.
 * Images that are not XYB: textbook float64 transfer functions and matrices (those of test_oracle_goldens.py's colour-science pin, and their forward forms) applied to the
   product's own plain float32 decode.  The bounds per (source TF, target TF) pair are 4 x the deviation measured on the MI355X, rounded up to one digit (PARITY.md has both
   columns); none is above 1e-4, the loosest bound of that pin.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import synth_lib as S

W, H = 200, 136            # partial tiles, the fused kernel's packed stores
W2, H2 = 67, 41            # odd, below one tile

# name -> (keywords of synth_lib.set_color without the intensity target = the dict output_color= takes)
TARGETS = {
    "srgb": dict(white_point=1, primaries=1, tf=13),
    "linear_srgb": dict(white_point=1, primaries=1, tf=8),
    "p3_srgb_tf": dict(white_point=1, primaries=11, tf=13),
    "bt2100_pq": dict(white_point=1, primaries=9, tf=16),
    "bt2100_hlg": dict(white_point=1, primaries=9, tf=18),
    "dci_white_p3_gamma26": dict(white_point=11, primaries=11, tf=17),
    "bt2100_rec709_tf": dict(white_point=1, primaries=9, tf=1),
    "white_e_gamma22": dict(white_point=10, primaries=1, gamma=1 / 2.2),
}
# name -> (colour keywords, intensity target)
XYB_SOURCES = {
    "srgb": (TARGETS["srgb"], 255.0),
    "p3_srgb_tf": (TARGETS["p3_srgb_tf"], 255.0),
    "bt2100_pq_1000": (TARGETS["bt2100_pq"], 1000.0),
    "bt2100_hlg_1000": (TARGETS["bt2100_hlg"], 1000.0),
}
NON_XYB_SOURCES = dict(XYB_SOURCES, linear_srgb=(TARGETS["linear_srgb"], 255.0))
del NON_XYB_SOURCES["srgb"]
NON_XYB_SOURCES["srgb"] = (TARGETS["srgb"], 255.0)


@pytest.fixture(scope="module")
def jxh(built):
    import jpegxl_rs_amd as jx
    return jx


@pytest.fixture(scope="module")
def jx(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import jpegxl_rs_amd as jx
    return jx


def under(colour, intensity_target, make):
    """make() under image headers that name `colour` at `intensity_target`"""
    S.set_color(intensity_target=intensity_target, **colour)
    try:
        return make()
    finally:
        S.set_color()


# ---- float64 restatement: chromaticities -> matrices (own constants) ---------------------------------------------------------------------------------
SRGB_XY = (0.639998686, 0.330010138, 0.300003784, 0.600003357, 0.150002046, 0.059997204)      # the sRGB primaries as the codestream's enum defines them
BT709_XY = (0.64, 0.33, 0.30, 0.60, 0.15, 0.06)
P3_XY = (0.680, 0.320, 0.265, 0.690, 0.150, 0.060)
BT2100_XY = (0.708, 0.292, 0.170, 0.797, 0.131, 0.046)
D65, DCI, WHITE_E = (0.3127, 0.3290), (0.314, 0.351), (1 / 3, 1 / 3)
PRIMARIES = {1: SRGB_XY, 9: BT2100_XY, 11: P3_XY}
WHITES = {1: D65, 10: WHITE_E, 11: DCI}


def xy_of(colour):
    white = tuple(colour["white_xy"]) if "white_xy" in colour else WHITES[colour.get("white_point", 1)]
    prim = tuple(colour["red_xy"]) + tuple(colour["green_xy"]) + tuple(colour["blue_xy"]) if "red_xy" in colour else PRIMARIES[colour.get("primaries", 1)]
    return prim, white


def rgb_to_xyz(prim, white):
    P = np.array([[prim[0], prim[2], prim[4]], [prim[1], prim[3], prim[5]], [1 - prim[0] - prim[1], 1 - prim[2] - prim[3], 1 - prim[4] - prim[5]]], np.float64)
    Wv = np.array([white[0] / white[1], 1.0, (1 - white[0] - white[1]) / white[1]])
    return P * np.linalg.solve(P, Wv)


def bradford_to_d50(white):
    """linear Bradford adaptation of XYZ under `white` to D50 (Lindbloom's cone matrix; D50 = (0.96422, 1, 0.82521))"""
    M = np.array([[0.8951, 0.2664, -0.1614], [-0.7502, 1.7135, 0.0367], [0.0389, -0.0685, 1.0296]], np.float64)
    w = np.array([white[0] / white[1], 1.0, (1 - white[0] - white[1]) / white[1]])
    d50 = np.array([0.96422, 1.0, 0.82521])
    # the inverse cone matrix as the CMS code carries it (seven decimals), not numpy's inverse: that is the constant the 1e-12 agreement is about
    Minv = np.array([[0.9869929, -0.1470543, 0.1599627], [0.4323053, 0.5183603, 0.0492912], [-0.0085287, 0.0400428, 0.9684867]], np.float64)
    return Minv @ np.diag((M @ d50) / (M @ w)) @ M


def restated_matrix(a, b):
    (pa, wa), (pb, wb) = xy_of(a), xy_of(b)
    if (pa, wa) == (pb, wb):
        return np.eye(3)
    return np.linalg.inv(bradford_to_d50(wb) @ rgb_to_xyz(pb, wb)) @ bradford_to_d50(wa) @ rgb_to_xyz(pa, wa)


# ---- CPU: the matrix ------------------------------------------------------------------------------------------------------------------------------------
def test_matrix_against_bt2087(jxh):
    """BT.2087-0: linear BT.2020 -> BT.709 (both D65), published to four decimals.  The primaries are BT.709's published xy (0.64, 0.33 ...), given as custom
    chromaticities: the codestream's sRGB enum carries its own slightly different ones (0.639998686 ...), which move two entries by 3e-5."""
    published = np.array([[1.6605, -0.5876, -0.0728], [-0.1246, 1.1329, -0.0083], [-0.0182, -0.1006, 1.1187]])
    bt709 = dict(red_xy=BT709_XY[0:2], green_xy=BT709_XY[2:4], blue_xy=BT709_XY[4:6])
    m = jxh.color_conversion_matrix("rec2020_pq", bt709)
    print("BT.2087 deviation:", np.abs(m - published).max())
    assert np.abs(m - published).max() <= 5e-5
    assert np.abs(jxh.color_conversion_matrix("rec2020_hlg", "srgb") - published).max() <= 8e-5      # (the enum's own primaries: 3e-5 further off)


MATRIX_CASES = [
    ("display_p3", "srgb"), ("srgb", "display_p3"),
    (dict(white_point=11, primaries=11), dict(white_point=1, primaries=11)), (dict(white_point=1, primaries=1), dict(white_point=11, primaries=11)),
    (dict(white_point=10, primaries=1), "srgb"), ("rec2020_pq", dict(white_point=10, primaries=9)),
    (dict(white_xy=(0.3457, 0.3585), red_xy=(0.7347, 0.2653), green_xy=(0.1596, 0.8404), blue_xy=(0.0366, 0.0001)), "srgb"),
    ("display_p3", dict(white_xy=(0.32168, 0.33767), red_xy=(0.713, 0.293), green_xy=(0.165, 0.830), blue_xy=(0.128, 0.044))),
]


NAMED = {"srgb": dict(white_point=1, primaries=1, tf=13), "display_p3": dict(white_point=1, primaries=11, tf=13), "rec2020_pq": dict(white_point=1, primaries=9, tf=16)}


def as_dict(c):
    return NAMED[c] if isinstance(c, str) else c


@pytest.mark.parametrize("a,b", MATRIX_CASES)
def test_matrix_against_float64_restatement(jxh, a, b):
    m = jxh.color_conversion_matrix(a, b)
    want = restated_matrix(as_dict(a), as_dict(b))
    print("matrix deviation:", np.abs(m - want).max())
    assert np.abs(m - want).max() <= 1e-12
    back = jxh.color_conversion_matrix(b, a)
    assert np.abs(m @ back - np.eye(3)).max() <= 1e-12 and np.abs(back @ m - np.eye(3)).max() <= 1e-12
    for c in (a, b):
        assert np.array_equal(jxh.color_conversion_matrix(c, c), np.eye(3))      # exactly
    # the transfer function is not part of it
    assert np.array_equal(jxh.color_conversion_matrix(dict(as_dict(a), tf=8), dict(as_dict(b), gamma=0.5)), m)


def test_matrix_refusals(jxh):
    for bad, word in ((dict(color_space=2), "colour space"), (dict(color_space=3), "colour space"), (dict(tf=2), "transfer function"), (dict(white_xy=(0.3, 0.0)), "y <= 0"),
                      (dict(red_xy=(0.64, 0.33), green_xy=(0.3, -0.1), blue_xy=(0.15, 0.06)), "y <= 0"), (dict(gamma=1.5), "gamma")):
        with pytest.raises(jxh.GenericError, match="unsupported: output colour.*" + word):
            jxh.color_conversion_matrix(bad, "srgb")
    with pytest.raises(jxh.GenericError, match="grey"):
        jxh.color_conversion_matrix(dict(color_space=1), "srgb")
    with pytest.raises(ValueError):
        jxh.color_encoding("adobe_rgb")
    with pytest.raises(ValueError):
        jxh.color_encoding(dict(whitepoint=1))


# ---- CPU: JxlDecoder* through ctypes ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_streams():
    img = S.synthetic_image(31, W2, H2)
    pq = TARGETS["bt2100_pq"]
    xyb = under(pq, 1000.0, lambda: S.encode_vardct(img, seed=5, strategy_mix=2))
    import jpegxl_rs_amd as jx
    icc = jx.icc_profile_from_headers(under(TARGETS["p3_srgb_tf"], 255.0, lambda: S.encode_vardct(img, seed=5)))
    S.set_icc(icc)
    try:
        xyb_icc = S.encode_vardct(img, seed=5, strategy_mix=2)
        modular_icc = S.encode_modular(img.astype(np.int32), 8)
    finally:
        S.set_icc(b"")
    modular = under(pq, 1000.0, lambda: S.encode_modular(img.astype(np.int32), 8))
    grey = S.encode_modular(img[..., :1].astype(np.int32), 8)
    return dict(xyb=xyb, xyb_icc=xyb_icc, modular=modular, modular_icc=modular_icc, grey=grey, icc=icc)


def encoding(jx, colour):
    return jx.color_encoding(colour)


def open_decoder(jx, data, upto):
    """a decoder fed `data` and advanced until ProcessInput returns `upto` -> (handle, keepalive)"""
    L = jx.libjxl()
    raw = np.frombuffer(data, np.uint8)
    dec = L.JxlDecoderCreate(None)
    assert L.JxlDecoderSubscribeEvents(dec, jx.JXL_DEC_BASIC_INFO | jx.JXL_DEC_COLOR_ENCODING | jx.JXL_DEC_FRAME | jx.JXL_DEC_FULL_IMAGE) == 0
    assert L.JxlDecoderSetInput(dec, raw.ctypes.data, len(raw)) == 0
    L.JxlDecoderCloseInput(dec)
    while upto is not None:
        st = L.JxlDecoderProcessInput(dec)
        assert st in (jx.JXL_DEC_BASIC_INFO, jx.JXL_DEC_COLOR_ENCODING, jx.JXL_DEC_FRAME), (st, jx.last_error())
        if st == upto:
            break
    return dec, raw


def data_profile(jx, dec, target):
    L = jx.libjxl()
    e = jx.JxlColorEncoding()
    ok = L.JxlDecoderGetColorAsEncodedProfile(dec, target, C.byref(e)) == 0
    n = C.c_size_t()
    assert L.JxlDecoderGetICCProfileSize(dec, target, C.byref(n)) == 0
    icc = np.zeros(n.value, np.uint8)
    assert L.JxlDecoderGetColorAsICCProfile(dec, target, icc.ctypes.data, n.value) == 0
    return ((e.color_space, e.white_point, e.primaries, e.transfer_function, round(e.gamma * 1e7)) if ok else None), icc.tobytes()


ORIGINAL, DATA = 0, 1


def test_decoder_refusals_and_reported_profiles(jxh, monkeypatch):
    """Host only: the decoders are created under JXL_HIP_DEVICE=-1 (a host-only batch behind them: headers and settings work, a decode would not)"""
    jx, L, st = jxh, jxh.libjxl(), small_streams()
    monkeypatch.setenv("JXL_HIP_DEVICE", "-1")
    srgb = encoding(jx, "srgb")
    # before the headers
    dec, keep = open_decoder(jx, st["xyb"], None)
    assert L.JxlHipDecoderSetOutputColorProfile(dec, C.byref(srgb), None, 0) == 1 and "not known yet" in jx.last_error()
    L.JxlDecoderDestroy(dec)
    # an XYB stream: ICC data, an XYB / unknown target, an unknown transfer function, a grey target are refused and leave everything as it was; then success
    dec, keep = open_decoder(jx, st["xyb"], jx.JXL_DEC_COLOR_ENCODING)
    before = (data_profile(jx, dec, ORIGINAL), data_profile(jx, dec, DATA))
    assert before[0][0] == (0, 1, 9, 16, 0) and before[0] == before[1]
    icc = np.frombuffer(st["icc"], np.uint8)
    assert L.JxlHipDecoderSetOutputColorProfile(dec, None, icc.ctypes.data, len(icc)) == 1 and "needs a CMS" in jx.last_error()
    assert L.JxlHipDecoderSetOutputColorProfile(dec, C.byref(srgb), icc.ctypes.data, len(icc)) == 1 and "needs a CMS" in jx.last_error()
    for bad in (dict(color_space=2), dict(color_space=3), dict(tf=2), dict(color_space=1)):
        assert L.JxlHipDecoderSetOutputColorProfile(dec, C.byref(encoding(jx, bad)), None, 0) == 1 and "output colour" in jx.last_error()
    assert (data_profile(jx, dec, ORIGINAL), data_profile(jx, dec, DATA)) == before
    assert L.JxlHipDecoderSetOutputColorProfile(dec, C.byref(srgb), None, 0) == 0
    assert data_profile(jx, dec, ORIGINAL) == before[0]
    got = data_profile(jx, dec, DATA)
    assert got[0] == (0, 1, 1, 13, 0)
    assert got[1] == jx.icc_profile_from_headers(under(TARGETS["srgb"], 255.0, lambda: S.encode_vardct(S.synthetic_image(31, W2, H2), seed=5))) != before[1][1]
    # Rewind keeps the target, Reset clears it
    L.JxlDecoderRewind(dec)
    assert L.JxlDecoderSetInput(dec, keep.ctypes.data, len(keep)) == 0
    while L.JxlDecoderProcessInput(dec) != jx.JXL_DEC_COLOR_ENCODING:
        pass
    assert data_profile(jx, dec, DATA)[0] == (0, 1, 1, 13, 0)
    L.JxlDecoderReset(dec)
    assert L.JxlDecoderSubscribeEvents(dec, jx.JXL_DEC_COLOR_ENCODING) == 0 and L.JxlDecoderSetInput(dec, keep.ctypes.data, len(keep)) == 0
    while L.JxlDecoderProcessInput(dec) != jx.JXL_DEC_COLOR_ENCODING:
        pass
    assert data_profile(jx, dec, DATA) == before[1]
    # a gamma target; a call without an encoding is refused and leaves it
    assert L.JxlHipDecoderSetOutputColorProfile(dec, C.byref(encoding(jx, TARGETS["white_e_gamma22"])), None, 0) == 0
    assert data_profile(jx, dec, DATA)[0] == (0, 10, 1, 65535, 4545455)
    assert L.JxlHipDecoderSetOutputColorProfile(dec, None, None, 0) == 1 and "neither" in jx.last_error()
    assert data_profile(jx, dec, DATA)[0] == (0, 10, 1, 65535, 4545455)
    L.JxlDecoderDestroy(dec)
    # an XYB stream with an embedded ICC profile: ORIGINAL stays the profile, DATA becomes the target
    dec, keep = open_decoder(jx, st["xyb_icc"], jx.JXL_DEC_COLOR_ENCODING)
    orig = data_profile(jx, dec, ORIGINAL)
    assert orig == (None, st["icc"])
    assert L.JxlHipDecoderSetOutputColorProfile(dec, C.byref(encoding(jx, "display_p3")), None, 0) == 0
    assert data_profile(jx, dec, ORIGINAL) == orig
    assert data_profile(jx, dec, DATA)[0] == (0, 1, 11, 13, 0)
    L.JxlDecoderDestroy(dec)
    # a stream that is not XYB: success, and DATA stays what it was; a grey image refuses an RGB target and takes a grey one
    dec, keep = open_decoder(jx, st["modular"], jx.JXL_DEC_COLOR_ENCODING)
    before = (data_profile(jx, dec, ORIGINAL), data_profile(jx, dec, DATA))
    assert L.JxlHipDecoderSetOutputColorProfile(dec, C.byref(srgb), None, 0) == 0
    assert (data_profile(jx, dec, ORIGINAL), data_profile(jx, dec, DATA)) == before and before[1][0] == (0, 1, 9, 16, 0)
    # the host-only decoder these calls ran on refuses every entry that would decode, in one voice
    px = np.zeros(W2 * H2 * 3, np.uint8)
    fmt = jx.JxlPixelFormat(3, jx.JXL_TYPE_UINT8, jx.JXL_NATIVE_ENDIAN, 0)
    assert L.JxlDecoderProcessInput(dec) == jx.JXL_DEC_FRAME
    assert L.JxlDecoderSetImageOutBuffer(dec, C.byref(fmt), px.ctypes.data, px.size) == 0
    assert L.JxlDecoderFlushImage(dec) == 1 and "host-only decoder" in jx.last_error()
    assert L.JxlDecoderProcessInput(dec) == 1 and "host-only decoder" in jx.last_error()
    L.JxlDecoderDestroy(dec)
    dec, keep = open_decoder(jx, st["grey"], jx.JXL_DEC_COLOR_ENCODING)
    assert L.JxlHipDecoderSetOutputColorProfile(dec, C.byref(srgb), None, 0) == 1 and "grey image" in jx.last_error()
    assert L.JxlHipDecoderSetOutputColorProfile(dec, C.byref(encoding(jx, dict(color_space=1, tf=8))), None, 0) == 0
    L.JxlDecoderDestroy(dec)


# ---- CPU: JxlHipBatchSetOutputColor on a host-only batch ----------------------------------------------------------------------------------------------------
def test_batch_refusals_leave_the_output(jxh):
    jx, L, st = jxh, jxh.libjxl(), small_streams()
    b = jx.BatchDecoder(-1)
    for name in ("xyb", "modular", "modular_icc", "grey", "xyb_icc"):
        b.add(st[name], "uint16", 3)
    size = [b.out_size(i) for i in range(5)]

    def set_color(i, colour, non_xyb=0):
        c = jx.JxlHipOutputColor(jx.color_encoding(colour), non_xyb)
        return L.JxlHipBatchSetOutputColor(b._h, i, C.byref(c))
    for bad, word in ((dict(color_space=2), "colour space"), (dict(color_space=3), "colour space"), (dict(tf=2), "transfer function"), (dict(white_xy=(0.3, -1.0)), "y <= 0"),
                      (dict(color_space=1), "grey encoding for a colour image")):
        for i in (0, 1):
            assert set_color(i, bad) == 1 and "unsupported: output colour" in jx.last_error() and word in jx.last_error(), jx.last_error()
    assert set_color(3, "srgb") == 1 and "RGB encoding for a grey image" in jx.last_error()
    assert set_color(0, "srgb", 2) == 1 and "non_xyb" in jx.last_error()
    assert set_color(2, "srgb", 1) == 1 and jx.last_error().endswith("unsupported: output colour of an image whose colour is an ICC profile needs a CMS")
    assert [b.out_size(i) for i in range(5)] == size
    # accepted: every target on the XYB images (with or without a profile), on the others under either rule; NULL clears
    for name, colour in TARGETS.items():
        assert set_color(0, colour) == 0 and set_color(4, colour, 1) == 0 and set_color(1, colour, 0) == 0 and set_color(1, colour, 1) == 0, name
    assert set_color(2, "srgb", 0) == 0                       # (libjxl's rule: the samples stay, profile or not)
    assert set_color(3, dict(color_space=1, tf=8), 1) == 0
    assert L.JxlHipBatchSetOutputColor(b._h, 0, None) == 0
    assert [b.out_size(i) for i in range(5)] == size
    # an image whose own encoding cannot be taken to linear light is as unconvertible as an ICC-only one; under libjxl's rule it is left alone
    odd = under(dict(white_point=1, primaries=1, tf=2), 255.0, lambda: S.encode_modular(S.synthetic_image(31, W2, H2).astype(np.int32), 8))
    i = b.add(odd, "uint16", 3)
    assert set_color(i, "srgb", 0) == 0
    assert set_color(i, "srgb", 1) == 1 and "own encoding cannot be converted" in jx.last_error() and "unknown transfer function" in jx.last_error()
    # kept animation canvases (batch option "output_all_frames") refuse the conversion of an image that is not XYB, and take everything else
    ba = jx.BatchDecoder(-1)
    L.JxlHipBatchSetOption(ba._h, b"output_all_frames", 1)
    ba.add(st["modular"], "uint16", 3)
    ba.add(st["xyb"], "uint16", 3)
    c = jx.JxlHipOutputColor(jx.color_encoding("srgb"), 1)
    assert L.JxlHipBatchSetOutputColor(ba._h, 0, C.byref(c)) == 1 and "kept animation canvases" in jx.last_error()
    assert L.JxlHipBatchSetOutputColor(ba._h, 1, C.byref(c)) == 0
    c.non_xyb = 0
    assert L.JxlHipBatchSetOutputColor(ba._h, 0, C.byref(c)) == 0
    c = jx.JxlHipOutputColor(jx.color_encoding(TARGETS["bt2100_pq"]), 1)      # (its own encoding: nothing to convert)
    assert L.JxlHipBatchSetOutputColor(ba._h, 0, C.byref(c)) == 0
    # before any output is set; an image that is not there
    b2 = jx.BatchDecoder(-1)
    buf = np.frombuffer(st["xyb"], np.uint8)
    assert L.JxlHipBatchAddImage(b2._h, buf.ctypes.data, len(buf)) == 0
    c = jx.JxlHipOutputColor(jx.color_encoding("srgb"), 0)
    assert L.JxlHipBatchSetOutputColor(b2._h, 0, C.byref(c)) == 1 and "no output yet" in jx.last_error()
    assert L.JxlHipBatchSetOutputColor(b2._h, 3, C.byref(c)) == 1 and "no such image" in jx.last_error()


def transcode_444(w=40, h=24, seed=4):
    """a 4:4:4 JPEG transcode (YCbCr VarDCT, DCT8 only, RAW quantisation table): coefficients from the synthesiser, no JPEG file needed"""
    n = -(-w // 8) * -(-h // 8)
    rng = np.random.default_rng(seed)
    planes = [rng.integers(-3, 4, (n, 64)).astype(np.int16) for _ in range(3)]      # Cb, Y, Cr
    planes[1][:, 0] = rng.integers(-40, 40, n)
    return S.jpeg_transcode_codestream(w, h, [0, 0, 0], planes, np.full((3, 64), 16, np.int32))


def test_batch_refuses_libjpeg_exact_outputs_and_a_later_set_output_clears(jxh):
    jx, L = jxh, jxh.libjxl()
    data = transcode_444()
    b = jx.BatchDecoder(-1)
    fmt = jx.JxlPixelFormat(3, jx.JXL_TYPE_UINT8, jx.JXL_NATIVE_ENDIAN, 0)
    buf = np.frombuffer(data, np.uint8)
    assert L.JxlHipBatchAddImage(b._h, buf.ctypes.data, len(buf)) == 0
    assert L.JxlHipBatchSetOutput(b._h, 0, C.byref(fmt), None) == 0
    assert L.JxlHipBatchCanDecodeJpegPixels(b._h, 0) == 1, jx.last_error()
    c = jx.JxlHipOutputColor(jx.color_encoding("display_p3"), 1)
    assert L.JxlHipBatchSetOutputJpegScaled(b._h, 0, C.byref(fmt), None, 2, None, None) == 0
    assert L.JxlHipBatchSetOutputColor(b._h, 0, C.byref(c)) == 1 and "unsupported: output colour of a libjpeg-exact output" in jx.last_error()
    rs = jx.JxlHipOutputResample(24, 20, 0, 0, 0, 0, 0, 0)
    assert L.JxlHipBatchSetOutputJpegResampled(b._h, 0, C.byref(fmt), None, 1, None, C.byref(rs), jx.JXL_HIP_RESAMPLE_U8) == 0
    assert L.JxlHipBatchSetOutputColor(b._h, 0, C.byref(c)) == 1 and "libjpeg-exact" in jx.last_error()
    size = C.c_size_t()
    assert L.JxlHipBatchOutputPlanesLayout(b._h, 0, None, None, C.byref(size)) == 0 and size.value == 24 * 20 * 3      # (the refused call left the output that was set)
    # a target, then a later SetOutput...: the target is gone.  Were it still there, the libjpeg-exact output set next would be refused as above; and
    # JxlHipBatchSetOutputPlanes, which sets the image's present output again, goes through
    assert L.JxlHipBatchSetOutput(b._h, 0, C.byref(fmt), None) == 0
    assert L.JxlHipBatchSetOutputColor(b._h, 0, C.byref(c)) == 0
    assert L.JxlHipBatchSetOutputJpegScaled(b._h, 0, C.byref(fmt), None, 2, None, None) == 0
    assert L.JxlHipBatchSetOutputPlanes(b._h, 0, None) == 0
    # the bindings: no colour on jobs of libjpeg-exact pixels, convert_non_xyb needs a target
    with pytest.raises(jx.GenericError, match="output colour"):
        jx.Pipeline.submit(None, [data], jpeg_pixels=True, output_color="srgb")
    with pytest.raises(ValueError):
        jx.BatchDecoder(-1).add(data, convert_non_xyb=True)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------------
def run_batch(jx, items, dtype, nch=3, **common):
    """items: (stream, keywords of BatchDecoder.add) each -> (outputs as flat arrays, the batch): one prepare and one decode for all of them"""
    b = jx.BatchDecoder(0)
    for data, kw in items:
        b.add(data, dtype, nch, **dict(common, **kw))
    b.prepare(); b.decode(); b.finish()
    return [b.output(i) for i in range(len(items))], b


def ulp_diff(a, b):
    ai = a.view(np.int32).astype(np.int64); bi = b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7FFFFFFF), ai); bi = np.where(bi < 0, -(bi & 0x7FFFFFFF), bi)
    return np.abs(ai - bi).max() if a.size else 0


def xyb_stream(kind, w, h):
    """one XYB stream of `kind` under whatever header synth_lib.set_color has set"""
    img = S.synthetic_image(31, w, h)
    if kind == "gab_epf1":
        return S.encode_vardct(img, seed=5, strategy_mix=2)                                   # the fused kernel (sRGB / linear) or the unfused filters + OutputKernel
    if kind == "no_filters":
        return S.encode_vardct(img, seed=6, gab=0, epf_iters=0)
    if kind == "two_frames":                                                                   # the frame tail: ColorKernel
        tile = S.synthetic_image(9, w // 3, h // 3)
        return S.encode_vardct_frame(img, S.frame(is_last=0, save_as_reference=1), seed=3) + \
            S.encode_vardct_frame(tile, S.frame(emit=1, have_crop=1, crop_x0=w // 5, crop_y0=h // 4, canvas_w=w, canvas_h=h, blend_mode=1, blend_source=1), seed=4)
    if kind == "upsampled_2x":
        return S.encode_vardct(S.synthetic_image(31, (w + 1) // 2, (h + 1) // 2), seed=5, upsampling=2)
    if kind == "modular_xyb":
        return S.encode_modular_frame(img.astype(np.int32), S.frame(emit=0, xyb_image=1), bits=8)
    raise KeyError(kind)


def common_suffix(a, b):
    n = 0
    while n < min(len(a), len(b)) and a[-1 - n] == b[-1 - n]:
        n += 1
    return n


@functools.lru_cache(maxsize=None)
def xyb_family(kind, w, h):
    """-> (sources: name -> stream, twins: (target name, intensity target) -> stream); asserts that all of them carry one payload"""
    sources = {name: under(colour, it, lambda: xyb_stream(kind, w, h)) for name, (colour, it) in XYB_SOURCES.items()}
    twins = {(t, it): under(colour, it, lambda: xyb_stream(kind, w, h)) for t, colour in TARGETS.items() for it in (255.0, 1000.0)}
    every = list(sources.values()) + list(twins.values())
    shortest = min(len(s) for s in every)
    for s in every:
        # the headers differ by a few bytes (enums, a 24-bit gamma, the intensity target); everything behind them is the same bytes
        assert common_suffix(s, every[0]) >= shortest - 24, (kind, len(s), len(every[0]), common_suffix(s, every[0]))
    return sources, twins


XYB_KINDS = ["gab_epf1", "no_filters", "two_frames", "upsampled_2x", "modular_xyb"]


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(W, H), (W2, H2)], ids=["200x136", "67x41"])
@pytest.mark.parametrize("kind", XYB_KINDS)
def test_xyb_images_equal_their_twins(jx, kind, size):
    """Source headers {sRGB, P3, BT.2100 PQ 1000, BT.2100 HLG 1000} x the eight targets: the decode with a target is, bit for bit in u8, u16 and f32, the plain decode of
    the twin whose header names the target at the source's intensity target; the twin's f32 decode is the oracle's to 1 ULP.  One bit off means that the kernel choice
    or a parameter went by the header instead of the effective encoding."""
    sources, twins = xyb_family(kind, *size)
    pairs = [(a, t) for a in sources for t in TARGETS]
    for dtype in ("uint8", "uint16", "float32"):
        got, _ = run_batch(jx, [(sources[a], dict(output_color=TARGETS[t])) for a, t in pairs], dtype)
        keys = sorted(twins)
        want, _ = run_batch(jx, [(twins[k], {}) for k in keys], dtype)
        want = dict(zip(keys, want))
        for (a, t), g in zip(pairs, got):
            w = want[(t, XYB_SOURCES[a][1])]
            assert g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (kind, a, t, dtype, int((g != w).sum()))
        if dtype == "float32":
            for k in keys:
                ref = np.frombuffer(O.decode(twins[k]).pixels("f32", 3), np.float32)
                assert ulp_diff(want[k], ref) <= 1, (kind, k)
    # by name, and with convert_non_xyb (which only concerns images that are not XYB): the same bytes
    a = "bt2100_pq_1000"
    named, _ = run_batch(jx, [(sources[a], dict(output_color="srgb")), (sources[a], dict(output_color="display_p3", convert_non_xyb=True)), (sources[a], dict(output_color="linear_srgb"))], "uint16")
    want, _ = run_batch(jx, [(twins[(t, 1000.0)], {}) for t in ("srgb", "p3_srgb_tf", "linear_srgb")], "uint16")
    for g, w in zip(named, want):
        assert np.array_equal(g, w)


@pytest.mark.gpu
def test_xyb_grey_image(jx):
    """sample_grey.jxl: a real encoder's grey XYB image (40 x 50, D65, gamma 0.45455; the synthesiser writes no grey XYB stream, so there is no twin).  Its own encoding
    as the target gives the plain decode's bytes.  A grey linear target gives linear light L with plain = L^0.45455: the decoder's power function is libjxl's
    FastPowf (relative error 3e-5 by its own documentation; the plain decode is the oracle's bit for bit), so 1e-4 bounds |plain - L^g| for L in [0, 1].  RGB targets are refused."""
    from conftest import fixture_bytes
    data = fixture_bytes("sample_grey.jxl")
    own = dict(color_space=1, white_point=1, gamma=0.45455)
    (plain, same, linear, srgb), _ = run_batch(jx, [(data, {}), (data, dict(output_color=own)), (data, dict(output_color=dict(color_space=1, tf=8))),
                                                     (data, dict(output_color=dict(color_space=1, tf=13)))], "float32", 1)
    assert np.array_equal(plain.view(np.uint32), same.view(np.uint32))
    dev = np.abs(np.maximum(linear.astype(np.float64), 0) ** 0.45455 - plain).max()
    print("grey XYB: |plain - linear^g| max", dev)
    assert dev <= 1e-4 and np.abs(linear - plain).max() > 0.05
    lin = np.maximum(linear.astype(np.float64), 0)
    assert np.abs(np.where(lin <= 0.0031308, 12.92 * lin, 1.055 * lin ** (1 / 2.4) - 0.055) - srgb).max() <= 1e-5      # (LinearToSrgb's rational polynomial: 1e-6 by the oracle's pin)
    b = jx.BatchDecoder(0)
    with pytest.raises(jx.GenericError, match="RGB encoding for a grey image"):
        b.add(data, output_color="srgb")


@pytest.mark.gpu
def test_composition_with_the_other_output_options(jx):
    """One PQ-header stream with target sRGB through downscale 8, planar f16 with scale / bias, a cropped cubic resize and two extra planes: each is byte for byte the
    same options applied to the sRGB twin, and the planes are those of the decode without a target."""
    img, alpha = S.synthetic_image(31, W, H), S.synthetic_image(4, W, H)[..., 0]
    pq = under(TARGETS["bt2100_pq"], 1000.0, lambda: S.encode_vardct(img, seed=5, strategy_mix=2))
    twin = under(TARGETS["srgb"], 1000.0, lambda: S.encode_vardct(img, seed=5, strategy_mix=2))
    pq_a = under(TARGETS["bt2100_pq"], 1000.0, lambda: S.encode_vardct(img, seed=5, strategy_mix=2, alpha=alpha))
    twin_a = under(TARGETS["srgb"], 1000.0, lambda: S.encode_vardct(img, seed=5, strategy_mix=2, alpha=alpha))
    assert common_suffix(pq, twin) >= min(len(pq), len(twin)) - 24 and common_suffix(pq_a, twin_a) >= min(len(pq_a), len(twin_a)) - 24
    cases = [("uint8", dict(downscale=8)), ("float16", dict(planar=True, scale=(2.0, 0.5, 1.5), bias=(-0.5, 0.25, 0.0))),
             ("uint16", dict(resize=(48, 32), crop=(13, 7, 150, 101), filter="bicubic")), ("float32", dict(downscale=8, planar=True, resize=(9, 7)))]
    for dtype, kw in cases:
        (got, want, untouched), _ = run_batch(jx, [(pq, dict(kw, output_color="srgb")), (twin, kw), (pq, kw)], dtype)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), kw
        assert not np.array_equal(got.view(np.uint8), untouched.view(np.uint8)), kw
    kw = dict(planar=True, extra_planes=[0, 0], plane_scale=[1.0, -2.0], plane_bias=[0.0, 1.0])
    (got, want, untouched), b = run_batch(jx, [(pq_a, dict(kw, output_color="srgb")), (twin_a, kw), (pq_a, kw)], "float32")
    assert b.info_value("plane_outputs") == 6
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    n = 3 * W * H
    assert np.array_equal(got[n:], untouched[n:]) and not np.array_equal(got[:n], untouched[:n])
    assert np.array_equal(np.rint(got[n:n + W * H] * 255).astype(np.uint8), alpha.reshape(-1))


def decoder_frames(jx, data, w, h, target=None, dtype=np.uint16, flushes=None):
    """every JXL_DEC_FULL_IMAGE of `data` through the libjxl API, with an output colour set at JXL_DEC_COLOR_ENCODING; flushes: a list that takes what JxlDecoderFlushImage
    shows at every JXL_DEC_FRAME_PROGRESSION"""
    L = jx.libjxl()
    raw = np.frombuffer(data, np.uint8)
    dec = L.JxlDecoderCreate(None)
    try:
        assert L.JxlDecoderSubscribeEvents(dec, jx.JXL_DEC_COLOR_ENCODING | jx.JXL_DEC_FRAME | jx.JXL_DEC_FULL_IMAGE | (jx.JXL_DEC_FRAME_PROGRESSION if flushes is not None else 0)) == 0
        assert L.JxlDecoderSetInput(dec, raw.ctypes.data, len(raw)) == 0
        L.JxlDecoderCloseInput(dec)
        fmt = jx.JxlPixelFormat(3, {np.uint8: jx.JXL_TYPE_UINT8, np.uint16: jx.JXL_TYPE_UINT16, np.float32: jx.JXL_TYPE_FLOAT}[dtype], jx.JXL_NATIVE_ENDIAN, 0)
        frames, buf, decodes = [], None, 0
        while True:
            st = L.JxlDecoderProcessInput(dec)
            if st == jx.JXL_DEC_COLOR_ENCODING:
                if target is not None:
                    e = jx.color_encoding(target)
                    assert L.JxlHipDecoderSetOutputColorProfile(dec, C.byref(e), None, 0) == 0, jx.last_error()
            elif st == jx.JXL_DEC_FRAME:
                pass
            elif st == jx.JXL_DEC_FRAME_PROGRESSION:
                assert L.JxlDecoderFlushImage(dec) == 0, jx.last_error()
                flushes.append(buf.copy())
                if target is not None:                          # a flush has shown pixels in the target: too late for another one
                    assert L.JxlHipDecoderSetOutputColorProfile(dec, C.byref(jx.color_encoding("linear_srgb")), None, 0) == 1 and "has begun" in jx.last_error()
            elif st == 5:                                       # JXL_DEC_NEED_IMAGE_OUT_BUFFER
                buf = np.zeros(w * h * 3, dtype)
                assert L.JxlDecoderSetImageOutBuffer(dec, C.byref(fmt), buf.ctypes.data, buf.nbytes) == 0
            elif st == jx.JXL_DEC_FULL_IMAGE:
                frames.append(buf.copy())
                decodes += L.JxlHipDecoderInfo(dec, b"frame_decodes")
                if target is not None:                          # the frame decode has begun: too late for another target
                    assert L.JxlHipDecoderSetOutputColorProfile(dec, C.byref(jx.color_encoding("linear_srgb")), None, 0) == 1 and "has begun" in jx.last_error()
            elif st == 0:
                return frames, decodes
            else:
                raise AssertionError((st, jx.last_error()))
    finally:
        L.JxlDecoderDestroy(dec)


@pytest.mark.gpu
def test_decoder_api_converts_xyb_images(jx):
    img = S.synthetic_image(31, W, H)
    pq = under(TARGETS["bt2100_pq"], 1000.0, lambda: S.encode_vardct(img, seed=5, strategy_mix=2))
    twin = under(TARGETS["srgb"], 1000.0, lambda: S.encode_vardct(img, seed=5, strategy_mix=2))
    assert common_suffix(pq, twin) >= min(len(pq), len(twin)) - 24
    for dtype in (np.uint8, np.uint16, np.float32):
        (want,), _ = decoder_frames(jx, twin, W, H, dtype=dtype)
        (got,), _ = decoder_frames(jx, pq, W, H, "srgb", dtype=dtype)
        (plain,), _ = decoder_frames(jx, pq, W, H, dtype=dtype)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
        assert not np.array_equal(plain.view(np.uint8), want.view(np.uint8))
    # progressive flushes (the kDC step of a four-group frame) show the target's pixels too
    big = S.synthetic_image(21, 300, 280)
    pq4, twin4 = (under(TARGETS[t], 1000.0, lambda: S.encode_vardct(big, seed=21, strategy_mix=1)) for t in ("bt2100_pq", "srgb"))
    assert common_suffix(pq4, twin4) >= min(len(pq4), len(twin4)) - 24
    shown, shown_twin, shown_plain = [], [], []
    (got,), _ = decoder_frames(jx, pq4, 300, 280, "srgb", flushes=shown)
    (want,), _ = decoder_frames(jx, twin4, 300, 280, flushes=shown_twin)
    decoder_frames(jx, pq4, 300, 280, flushes=shown_plain)
    assert len(shown) == len(shown_twin) >= 1 and np.array_equal(got, want)
    for g, w_ in zip(shown, shown_twin):
        assert np.array_equal(g, w_)
    assert not np.array_equal(shown[0], shown_plain[0]) and not np.array_equal(shown[0], got)
    # a stream that is not XYB: success, pixels untouched
    lossless = under(TARGETS["bt2100_pq"], 1000.0, lambda: S.encode_modular(S.synthetic_image(31, W2, H2).astype(np.int32), 8))
    (a,), _ = decoder_frames(jx, lossless, W2, H2, "srgb")
    (b,), _ = decoder_frames(jx, lossless, W2, H2)
    assert np.array_equal(a, b) and np.array_equal(a.reshape(H2, W2, 3), S.synthetic_image(31, W2, H2).astype(np.uint16) * 257)
    # a three-frame animation decoded once with a target: every canvas is the twin's
    def animation():
        base = S.synthetic_image(3, W2, H2)
        S.set_animation(100, 1, 0)
        try:
            parts = [S.encode_vardct_frame(base, S.frame(is_last=0, save_as_reference=1, duration=2), seed=3)]
            for k in (1, 2):
                parts.append(S.encode_vardct_frame(S.synthetic_image(100 + k, 24, 16), S.frame(emit=1, is_last=1 if k == 2 else 0, have_crop=1, crop_x0=7 * k, crop_y0=5 * k, canvas_w=W2, canvas_h=H2,
                                                                                             blend_mode=k % 2, blend_source=1, save_as_reference=0 if k == 2 else 1, duration=1), seed=k))
            return b"".join(parts)
        finally:
            S.set_animation(0)
    anim, anim_twin = under(TARGETS["bt2100_hlg"], 1000.0, animation), under(TARGETS["p3_srgb_tf"], 1000.0, animation)
    got, decodes = decoder_frames(jx, anim, W2, H2, TARGETS["p3_srgb_tf"])
    want, _ = decoder_frames(jx, anim_twin, W2, H2)
    assert len(got) == 3 and decodes == 1                       # (decoded once: the canvases were kept)
    for g, w_ in zip(got, want):
        assert np.array_equal(g, w_)
    assert not np.array_equal(got[0], got[2])


# ---- images that are not XYB: textbook float64 ------------------------------------------------------------------------------------------------------------------
def tf_name(colour):
    if colour.get("gamma"):
        return "gamma"
    return {13: "srgb", 8: "linear", 1: "rec709", 16: "pq", 17: "gamma", 18: "hlg"}[colour.get("tf", 13)]


def gamma_of(colour):
    return colour["gamma"] if colour.get("gamma") else 1 / 2.6


M1, M2, C1, C2, C3 = 2610 / 16384, 2523 / 4096 * 128, 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
HLG_A = 0.17883277
HLG_B, HLG_C = 1 - 4 * HLG_A, 0.5599107295


def hlg_system_gamma(it):
    return 1.2 * 1.111 ** np.log2(it / 1000.0)


def luminances(colour, grey):
    return np.array([0.2126, 0.7152, 0.0722]) if grey else rgb_to_xyz(*xy_of(colour))[1]


def to_linear64(v, colour, it, grey):
    """encoded samples (..., 3) -> display light, 1.0 = the intensity target"""
    name, a = tf_name(colour), np.abs(v)
    if name == "srgb":
        return np.sign(v) * np.where(a <= 0.04045, a / 12.92, ((a + 0.055) / 1.055) ** 2.4)
    if name == "linear":
        return v
    if name == "rec709":
        return np.where(v < 0.081, v / 4.5, ((np.maximum(v, 0.081) + 0.099) / 1.099) ** (1 / 0.45))
    if name == "gamma":
        return np.where(v <= 1e-5, 0.0, np.maximum(v, 1e-5) ** (1 / gamma_of(colour)))
    if name == "pq":
        p = a ** (1 / M2)
        return np.sign(v) * (np.maximum(p - C1, 0) / (C2 - C3 * p)) ** (1 / M1) * (10000.0 / it)
    scene = np.sign(v) * np.where(a <= 0.5, a * a / 3, (np.exp((a - HLG_C) / HLG_A) + HLG_B) / 12)
    g = hlg_system_gamma(it)
    if abs(1 / g - 1) <= 0.01:
        return scene
    ys = np.maximum(scene @ luminances(colour, grey), 0.0)
    with np.errstate(divide="ignore"):
        return scene * np.minimum(ys ** (g - 1), 1e9)[..., None]


def from_linear64(l, colour, it, grey):
    """display light -> encoded samples; the second value masks the samples the definition covers (the HLG inverse OOTF raises the luminance to a power: only where it is positive)"""
    name, a, ok = tf_name(colour), np.abs(l), np.ones(l.shape[:-1], bool)
    if name == "srgb":
        return np.sign(l) * np.where(a <= 0.0031308, 12.92 * a, 1.055 * a ** (1 / 2.4) - 0.055), ok
    if name == "linear":
        return l, ok
    if name == "rec709":
        return np.where(l <= 0.018, 4.5 * l, 1.099 * np.maximum(l, 0.018) ** 0.45 - 0.099), ok
    if name == "gamma":
        return np.where(l <= 1e-5, 0.0, np.maximum(l, 1e-5) ** gamma_of(colour)), ok
    if name == "pq":
        y = (a * it / 10000.0) ** M1
        return np.sign(l) * ((C1 + C2 * y) / (1 + C3 * y)) ** M2, ok
    g = hlg_system_gamma(it)
    scene = l
    if abs(1 / g - 1) > 0.01:
        yd = l @ luminances(colour, grey)
        ok = yd > 0
        scene = l * np.minimum(np.where(ok, yd, 1.0) ** (1 / g - 1), 1e9)[..., None]
    s = np.abs(scene)
    return np.sign(scene) * np.where(s <= 1 / 12, np.sqrt(3 * s), HLG_A * np.log(np.maximum(12 * s - HLG_B, 1e-300)) + HLG_C), ok


def convert64(px, src, dst, it, grey):
    """-> (expected samples, mask of the pixels the bound is asserted on).  A linear target is held on every pixel: that is the whole of the new arithmetic (inverse transfer
    function, matrix).  Behind it sits TransferFromLinear, which the rule takes unchanged: libjxl's approximations, fitted to linear light in [0, 1] — the sRGB rational
    polynomial is within 5e-7 of IEC 61966-2-1 there, 1.2e-6 at 1.125, 4e-5 at 2 and 6e-3 at 10, where a PQ 1000-nit image's code 1.0 lands and every integer output
    clips anyway.  Under the other targets the bound is asserted where the target's linear light stays within [-0.125, 1.125], the float images' own range."""
    lin = to_linear64(px.astype(np.float64), src, it, grey)
    if not grey:
        lin = lin @ restated_matrix(src, dst).T
    want, ok = from_linear64(lin, dst, it, grey)
    if tf_name(dst) != "linear":
        ok = ok & np.all((lin >= -0.125) & (lin <= 1.125), axis=-1)
    return want, ok


# (source TF, target TF) -> bound on |product - float64|: 4 x the largest deviation measured on the MI355X over every image kind below, rounded up to one digit
# (PARITY.md "Output colour" has the measured column).  Pairs with the same function on both sides and the same primaries never convert; the others do.
# What the bounds cover (convert64 has the reasons): under a LINEAR target every pixel — the inverse transfer functions and the matrix, which is all the arithmetic this feature
# adds; under every other target only the pixels whose linear light in the target lies within [-0.125, 1.125], because TransferFromLinear behind it is libjxl's approximation
# fitted to [0, 1] and has to stay as it is.  For PQ 1000 -> SDR targets that is as little as 5 % of a full-range picture: the mask is NOT full coverage of those pairs.
CEILING = 1e-4            # the loosest bound of test_oracle_goldens.py's colour-science pin: no pair may need more
BOUNDS = {
    ("hlg", "gamma"): 7e-06,      # measured 1.63e-06
    ("hlg", "linear"): 5e-06,     # measured 1.12e-06
    ("hlg", "pq"): 2e-05,         # measured 3.73e-06
    ("hlg", "rec709"): 4e-06,     # measured 9.62e-07
    ("hlg", "srgb"): 5e-06,       # measured 1.08e-06
    ("linear", "gamma"): 4e-06,   # measured 9.47e-07
    ("linear", "hlg"): 2e-06,     # measured 4.07e-07
    ("linear", "pq"): 4e-06,      # measured 8.26e-07
    ("linear", "rec709"): 5e-06,  # measured 1.09e-06
    ("linear", "srgb"): 4e-06,    # measured 9.81e-07
    ("pq", "gamma"): 5e-06,       # measured 1.16e-06
    ("pq", "hlg"): 6e-07,         # measured 1.31e-07
    ("pq", "linear"): 3e-05,      # measured 7.34e-06 (on every pixel: linear light up to 10, and beyond it for the float image's codes above 1.0)
    ("pq", "rec709"): 5e-06,      # measured 1.10e-06
    ("pq", "srgb"): 5e-06,        # measured 1.09e-06
    ("srgb", "gamma"): 1e-05,     # measured 2.44e-06
    ("srgb", "hlg"): 3e-06,       # measured 6.85e-07
    ("srgb", "linear"): 2e-06,    # measured 3.75e-07
    ("srgb", "pq"): 7e-06,        # measured 1.61e-06
    ("srgb", "rec709"): 5e-06,    # measured 1.16e-06
    ("srgb", "srgb"): 5e-06,      # measured 1.07e-06 (P3 -> sRGB primaries under one transfer function)
}


def non_xyb_stream(kind):
    """-> (stream under the header synth_lib.set_color has set, w, h, channels)"""
    rng = np.random.default_rng(12)
    if kind == "rgb8":
        return S.encode_modular(S.synthetic_image(31, W, H).astype(np.int32), 8), W, H, 3
    if kind == "rgb16":
        return S.encode_modular(rng.integers(0, 65536, (H2, W2, 3)).astype(np.int32), 16), W2, H2, 3
    if kind == "float16":                                  # binary16 samples, uniform in [-0.125, 1.125]
        vals = rng.uniform(-0.125, 1.125, (H2, W2, 3)).astype(np.float16).view(np.uint16)
        S.set_float(5)
        try:
            return S.encode_modular(vals.astype(np.int32), 16), W2, H2, 3
        finally:
            S.set_float(0)
    if kind == "grey8":
        return S.encode_modular(S.synthetic_image(31, W2, H2)[..., :1].astype(np.int32), 8), W2, H2, 1
    if kind == "two_frames":
        a, b = S.synthetic_image(31, W2, H2).astype(np.int32) // 2, S.synthetic_image(9, 32, 20).astype(np.int32) // 2
        return S.encode_modular_frame(a, S.frame(is_last=0, save_as_reference=1), 8) + \
            S.encode_modular_frame(b, S.frame(emit=1, have_crop=1, crop_x0=10, crop_y0=12, canvas_w=W2, canvas_h=H2, blend_mode=1, blend_source=1), 8), W2, H2, 3
    if kind == "ycbcr444":
        return S.encode_ycbcr(S.synthetic_image(31, W, H), "444"), W, H, 3
    raise KeyError(kind)


NON_XYB_KINDS = ["rgb8", "rgb16", "float16", "grey8", "two_frames", "ycbcr444"]


def target_for(colour, grey):
    if not grey:
        return colour
    d = {k: v for k, v in colour.items() if k != "primaries"}
    return dict(d, color_space=1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", NON_XYB_KINDS)
def test_non_xyb_conversion_against_float64(jx, kind):
    """Source headers {P3 sRGB-TF, BT.2100 PQ 1000, BT.2100 HLG 1000, linear sRGB, sRGB} x the eight targets under convert_non_xyb=True: the f32 output against textbook
    float64 applied to the product's own plain f32 decode of the same stream; integer and half outputs are numpy applied to the converted f32 output, exactly.
    Measured on the MI355X (pytest -s prints every pair and kind): the worst pair is PQ -> linear at 7.3e-6, every other one below 4e-6; BOUNDS has the table.  (With the
    ST 2084 EOTF in float32 that pair stood at 5.6e-4 — on a linear light of 10 — which is why PqToLinear computes in double.)"""
    streams = {}
    for name, (colour, it) in NON_XYB_SOURCES.items():
        streams[name], w, h, nch = under(colour, it, lambda: non_xyb_stream(kind))
    grey = nch == 1
    names = list(streams)
    (*plain,), b = run_batch(jx, [(streams[a], {}) for a in names], "float32", nch)
    plain = dict(zip(names, plain))
    pairs = [(a, t) for a in names for t in TARGETS]
    got, b = run_batch(jx, [(streams[a], dict(output_color=target_for(TARGETS[t], grey), convert_non_xyb=True)) for a, t in pairs], "float32", nch)
    assert b.info_value("post_ops") > 0
    worst = {}
    for (a, t), g in zip(pairs, got):
        src, it = NON_XYB_SOURCES[a]
        dst = TARGETS[t]
        px = plain[a].reshape(h, w, nch)
        if tf_name(src) == tf_name(dst) and (grey or xy_of(src) == xy_of(dst)) and (tf_name(src) != "gamma" or gamma_of(src) == gamma_of(dst)):
            assert np.array_equal(g.view(np.uint32), plain[a].view(np.uint32)), (kind, a, t)           # the image's own encoding: the plain decode's bytes
            continue
        want, ok = convert64(np.repeat(px, 3, axis=2) if grey else px, src, dst, it, grey)
        want = want[..., :nch]
        assert ok.mean() > 0.05, (kind, a, t, ok.mean())          # (PQ 1000 -> SDR targets: most of a full-range picture is brighter than the target's white)
        dev = np.abs(g.reshape(h, w, nch).astype(np.float64) - want)[ok].max()
        key = (tf_name(src), tf_name(dst))
        worst[key] = max(worst.get(key, 0.0), float(dev))
    for key in sorted(worst):
        print("non-XYB %-10s %-7s -> %-7s max |product - float64| = %.3g (bound %.1g)" % (kind, key[0], key[1], worst[key], BOUNDS[key]))
    for key, dev in worst.items():
        assert dev <= BOUNDS[key] <= CEILING, (kind, key, dev)
    if kind in ("rgb8", "rgb16", "ycbcr444"):
        f32 = dict(zip(pairs, got))
        for dtype, conv in (("uint8", lambda v: np.rint(np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)),
                            ("uint16", lambda v: np.rint(np.clip(v, np.float32(0), np.float32(1)) * np.float32(65535)).astype(np.uint16)),
                            ("float16", lambda v: v.astype(np.float16))):
            outs, _ = run_batch(jx, [(streams[a], dict(output_color=TARGETS[t], convert_non_xyb=True)) for a, t in pairs], dtype, nch)
            for p, o in zip(pairs, outs):
                assert np.array_equal(o.view(np.uint8), conv(f32[p]).view(np.uint8)), (kind, p, dtype)


@pytest.mark.gpu
def test_identity_and_the_rule_for_images_that_are_not_xyb(jx):
    """A target equal to the image's own encoding, and any target under convert_non_xyb=False, give the plain decode's bytes and keep a simple Modular image off the frame
    tail ("post_ops" = 0: nothing was planned for it).  An image whose colour is only an ICC profile fails alone in a pipeline job."""
    import torch
    img = S.synthetic_image(31, W2, H2)
    p3, it = TARGETS["p3_srgb_tf"], 255.0
    data = under(p3, it, lambda: S.encode_modular(img.astype(np.int32), 8))
    ycc = under(p3, it, lambda: S.encode_ycbcr(S.synthetic_image(31, W, H), "444"))
    for dtype in ("uint8", "float32"):
        (plain, plain_y), b = run_batch(jx, [(data, {}), (ycc, {})], dtype)
        assert b.info_value("post_ops") == 0
        for kw in (dict(output_color=p3, convert_non_xyb=True), dict(output_color="display_p3", convert_non_xyb=True), dict(output_color="srgb"), dict(output_color="rec2020_pq", convert_non_xyb=False),
                   dict(output_color=dict(white_xy=D65, red_xy=P3_XY[0:2], green_xy=P3_XY[2:4], blue_xy=P3_XY[4:6], tf=13), convert_non_xyb=True)):
            (same, same_y), b = run_batch(jx, [(data, kw), (ycc, kw)], dtype)
            assert b.info_value("post_ops") == 0, kw
            assert np.array_equal(same.view(np.uint8), plain.view(np.uint8)) and np.array_equal(same_y.view(np.uint8), plain_y.view(np.uint8)), kw
        (other, _), b = run_batch(jx, [(data, dict(output_color="srgb", convert_non_xyb=True)), (ycc, {})], dtype)
        assert b.info_value("post_ops") > 0 and not np.array_equal(other.view(np.uint8), plain.view(np.uint8))
    assert np.array_equal(np.rint(plain.reshape(H2, W2, 3) * 255).astype(np.uint8), img)      # (float32, the last of the loop: the file's samples)
    st = small_streams()
    xyb = under(TARGETS["bt2100_pq"], 1000.0, lambda: S.encode_vardct(img, seed=5, strategy_mix=2))
    datas = [xyb, st["modular_icc"], data]
    (want_xyb, want_p3), _ = run_batch(jx, [(xyb, dict(output_color="srgb")), (data, dict(output_color="srgb", convert_non_xyb=True))], "uint16")
    p = jx.Pipeline(0, jobs_in_flight=2, lf_streams=2, prepare_threads=1, parse_threads=2)
    try:
        n = W2 * H2 * 3 * 2
        outs = [torch.zeros(n, dtype=torch.uint8, device="cuda:0") for _ in datas]
        status, _ = p.wait(p.submit(datas, "uint16", 3, device_ptrs=[o.data_ptr() for o in outs], capacities=[n] * 3, output_color="srgb", convert_non_xyb=True), check=False)
        torch.cuda.synchronize()
        assert status == [0, 1, 0] and jx.last_error().endswith("unsupported: output colour of an image whose colour is an ICC profile needs a CMS")
        assert np.array_equal(outs[0].cpu().numpy().view(np.uint16), want_xyb) and np.array_equal(outs[2].cpu().numpy().view(np.uint16), want_p3)
        # libjxl's rule: the same job with convert_non_xyb=False decodes all three, the two that are not XYB untouched
        status, _ = p.wait(p.submit(datas, "uint16", 3, device_ptrs=[o.data_ptr() for o in outs], capacities=[n] * 3, output_color="srgb"))
        torch.cuda.synchronize()
        assert status == [0, 0, 0]
        assert np.array_equal(outs[0].cpu().numpy().view(np.uint16), want_xyb) and np.array_equal(outs[2].cpu().numpy().view(np.uint16).reshape(H2, W2, 3), img.astype(np.uint16) * 257)
    finally:
        p.close()


@pytest.mark.gpu
def test_pipeline_jobs_and_reused_batches(jx):
    """One job of sRGB, P3, PQ 1000 and HLG 1000 XYB streams of different sizes with target sRGB, as planar f16 into the slices of one [4, 3, 32, 48] tensor and to pinned
    host memory: the batch results.  A job with a target, a plain job and a job with a target again through one pipeline; a decode without a target after one with it
    from the same reset BatchDecoder equals a fresh decode."""
    import torch
    sizes = [(W, H), (W2, H2), (96, 64), (130, 90)]
    datas = [under(colour, it, lambda: S.encode_vardct(S.synthetic_image(20 + k, *sizes[k]), seed=5 + k, strategy_mix=2)) for k, (colour, it) in enumerate(XYB_SOURCES.values())]
    kw = dict(planar=True, resize=(48, 32))
    want, _ = run_batch(jx, [(d, dict(kw, output_color="srgb")) for d in datas], "float16")
    plain, _ = run_batch(jx, [(d, kw) for d in datas], "float16")
    assert all(w.size == 3 * 32 * 48 for w in want) and not np.array_equal(want[2], plain[2]) and np.array_equal(want[0], plain[0])
    slice_bytes = 3 * 32 * 48 * 2
    p = jx.Pipeline(0, jobs_in_flight=3, lf_streams=2, prepare_threads=2, parse_threads=2)
    try:
        t = torch.zeros((4, 3, 32, 48), dtype=torch.float16, device="cuda:0")
        ptrs = [t.data_ptr() + k * slice_bytes for k in range(4)]
        t2 = torch.zeros((4, 3, 32, 48), dtype=torch.float16, device="cuda:0")
        ptrs2 = [t2.data_ptr() + k * slice_bytes for k in range(4)]
        t3 = torch.zeros((4, 3, 32, 48), dtype=torch.float16, device="cuda:0")
        ptrs3 = [t3.data_ptr() + k * slice_bytes for k in range(4)]
        tickets = [p.submit(datas, "float16", 3, device_ptrs=ptrs, capacities=[slice_bytes] * 4, output_color="srgb", **kw),
                   p.submit(datas, "float16", 3, device_ptrs=ptrs2, capacities=[slice_bytes] * 4, **kw),
                   p.submit(datas, "float16", 3, device_ptrs=ptrs3, capacities=[slice_bytes] * 4, output_color=TARGETS["srgb"], convert_non_xyb=True, **kw)]
        for tk in tickets:
            assert p.wait(tk)[0] == [0, 0, 0, 0]
        torch.cuda.synchronize()
        for k in range(4):
            assert np.array_equal(t[k].cpu().numpy().reshape(-1), want[k]) and np.array_equal(t3[k].cpu().numpy().reshape(-1), want[k])
            assert np.array_equal(t2[k].cpu().numpy().reshape(-1), plain[k])
        pinned = [jx.PinnedBuffer(slice_bytes) for _ in datas]
        assert p.wait(p.submit(datas, "float16", 3, host_ptrs=[o.ptr for o in pinned], capacities=[slice_bytes] * 4, output_color="srgb", **kw))[0] == [0, 0, 0, 0]
        for k in range(4):
            assert np.array_equal(pinned[k].array.view(np.float16), want[k])
    finally:
        p.close()
    b = jx.BatchDecoder(0)
    for d in datas:
        b.add(d, "float16", 3, output_color="srgb", **kw)
    b.prepare(); b.decode(); b.finish()
    assert all(np.array_equal(b.output(k), want[k]) for k in range(4))
    b.reset()
    for d in datas:
        b.add(d, "float16", 3, **kw)
    b.prepare(); b.decode(); b.finish()
    assert all(np.array_equal(b.output(k), plain[k]) for k in range(4))
