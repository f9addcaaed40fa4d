"""The lossless batch encoder (include/jxl_hip.h JxlHipEncoder*, csrc/encode_lossless.cc + encode_lossless.hip; jpegxl_rs_amd.encode_lossless / LosslessEncoder /
encoder_builder): prefix-coded Modular codestreams whose tokens, bit counts and bits are computed on the GPU.

Host side (no GPU): the size bound against its documented formula, every refusal with its message, the Python mirror's refusals.
GPU side: every stream is decoded by the CPU oracle and by this library's own decoder, and the expected value is always the SOURCE array — for a depth that does not
fill its container (1, 10, 12 bits) the decoder's full-range samples are mapped back to the depth first, which is exact (the scaling is injective and the steps are
at least 16 apart).  Geometry cases are the smallest shapes that reach each branch of the group / edge / TOC logic; all of them go through ONE encode call and ONE
product decode (module fixtures), so a case costs one oracle decode of a small image."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import synth_lib as S

GD = 256


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


# ---- host side ---------------------------------------------------------------------------------------------------------------------------------
def documented_bound(w, h, c, bits):
    """include/jxl_hip.h JxlHipEncodeLosslessBound, restated"""
    groups = -(-w // GD) * -(-h // GD)
    toc = 1 if groups == 1 else 2 + -(-w // 2048) * -(-h // 2048) + groups
    n = bits + (1 if c >= 3 else 0)
    extra = n - 2 if n >= 4 else 0
    return 48 + 8192 + 2 + 6 * toc + -(-(w * h * c * (15 + extra)) // 8)


@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_bound_is_its_documented_formula(jxh, dtype, c):
    for bits in (1, 8, 10, 16):
        for (w, h) in ((1, 1), (256, 256), (257, 255), (2049, 3)):
            if dtype == "uint8" and bits > 8:
                with pytest.raises(jxh.EncodeError, match="does not fit the depth"):
                    jxh.encode_lossless_bound(w, h, c, bits, dtype)
                continue
            assert jxh.encode_lossless_bound(w, h, c, bits, dtype) == documented_bound(w, h, c, bits), (w, h, c, bits)


def test_bound_is_monotone_in_every_argument(jxh):
    base = dict(width=300, height=280, num_channels=2, bits=9, dtype="uint16")
    b0 = jxh.encode_lossless_bound(**base)
    for key, values in (("width", (301, 512, 513, 2049)), ("height", (281, 512, 513, 2049)), ("num_channels", (3, 4)), ("bits", (10, 12, 16))):
        last = b0
        for v in values:
            b = jxh.encode_lossless_bound(**dict(base, **{key: v}))
            assert b >= last and b > b0, (key, v)
            last = b
    assert jxh.encode_lossless_bound(8192, 8192, 4, 16, "uint16") > 8192 * 8192 * 8      # the largest side that must work


def _image(jxh, a, **over):
    f = dict(pixels=a.ctypes.data, on_device=0, xsize=a.shape[1], ysize=a.shape[0], num_channels=a.shape[2], bits_per_sample=8 * a.itemsize,
             data_type=jxh.JXL_TYPE_UINT8 if a.itemsize == 1 else jxh.JXL_TYPE_UINT16, row_pitch=0, alpha_premultiplied=0)
    f.update(over)
    return jxh.JxlHipEncodeImage(*[f[n] for n, _ in jxh.JxlHipEncodeImage._fields_])


REFUSALS = [
    (dict(xsize=0), "xsize and ysize must be 1..16384"), (dict(ysize=0), "xsize and ysize must be 1..16384"),
    (dict(xsize=16385), "xsize and ysize must be 1..16384"), (dict(ysize=1 << 20), "xsize and ysize must be 1..16384"),
    (dict(num_channels=0), "num_channels must be 1..4"), (dict(num_channels=5), "num_channels must be 1..4"),
    (dict(bits_per_sample=0), "bits_per_sample must be 1..16"), (dict(bits_per_sample=17), "bits_per_sample must be 1..16"),
    (dict(bits_per_sample=9), "does not fit the depth"), (dict(data_type=0), "data_type must be JXL_TYPE_UINT8 or JXL_TYPE_UINT16"),
    (dict(data_type=5), "data_type must be JXL_TYPE_UINT8 or JXL_TYPE_UINT16"),
    (dict(row_pitch=23), "row_pitch is below one row (24 bytes)"), (dict(pixels=None), "pixels is NULL"),
    (dict(on_device=1), "a device pointer on a host-only encoder"),
]


def test_refusals_of_a_host_only_encoder(jxh):
    L = jxh.libjxl()
    enc = L.JxlHipEncoderCreate(-1)
    assert enc
    try:
        a = np.zeros((5, 8, 3), np.uint8)
        good = _image(jxh, a)
        for over, message in REFUSALS:
            arr = (jxh.JxlHipEncodeImage * 2)(good, _image(jxh, a, **over))
            assert L.JxlHipEncoderEncodeLossless(enc, arr, 2, None) == 1
            assert L.JxlHipEncoderStatus(enc, 1) == 1 and message in jxh.last_error() and "image 1" in jxh.last_error(), (over, jxh.last_error())
            assert L.JxlHipEncoderSize(enc, 1) == 0 and L.JxlHipEncoderCopy(enc, 1, None, 0) == 1
            # the valid neighbour is not refused for its arguments: a host-only encoder just cannot encode it
            assert L.JxlHipEncoderStatus(enc, 0) == 1 and "host-only encoder cannot encode" in jxh.last_error()
        assert L.JxlHipEncoderStatus(enc, 2) == 1 and "no such image" in jxh.last_error()
        assert L.JxlHipEncoderEncodeLossless(enc, None, 0, None) == 0                 # an empty call is fine
        n = C.c_size_t()
        assert L.JxlHipEncodeLosslessBound(None, C.byref(n)) == 1 and L.JxlHipEncodeLosslessBound(C.byref(good), None) == 1
        assert L.JxlHipEncodeLosslessBound(C.byref(_image(jxh, a, pixels=None)), C.byref(n)) == 0 and n.value == documented_bound(8, 5, 3, 8)     # (the bound ignores `pixels`)
    finally:
        L.JxlHipEncoderDestroy(enc)
    assert not L.JxlHipEncoderCreate(1 << 20) and "no such HIP device" in jxh.last_error()


def test_python_mirror_refusals(jxh):
    with pytest.raises(jxh.EncodeError, match="unsupported: lossy"):
        jxh.encoder_builder()
    with pytest.raises(jxh.EncodeError, match="unsupported: lossy"):
        jxh.encoder_builder(lossless=False)
    for opt, v in (("quality", 2.0), ("speed", 3), ("jpeg_quality", 90.0), ("use_container", True), ("uses_original_profile", True), ("decoding_speed", 1),
                   ("color_encoding", "srgb"), ("target_intensity", 255.0), ("use_box", True), ("init_buffer_size", 64)):
        with pytest.raises(jxh.EncodeError, match="unsupported: encoder option " + opt):
            jxh.encoder_builder(lossless=True, **{opt: v})
    with pytest.raises(TypeError):
        jxh.encoder_builder(lossless=True, no_such_option=1)
    e = jxh.encoder_builder(lossless=True, has_alpha=False, device=-1)
    for call in (lambda: e.encode_jpeg(b"\xff\xd8"), lambda: e.add_metadata(None), lambda: e.multiple(4, 4), lambda: e.encode_frame(None, 4, 4), lambda: e.set_frame_option(0, 1)):
        with pytest.raises(jxh.EncodeError, match="unsupported: "):
            call()
    with pytest.raises(jxh.EncodeError, match="does not hold width x height"):
        e.encode(np.zeros(50, np.uint8), 4, 4)
    with pytest.raises(jxh.EncodeError, match="4 channels need has_alpha"):
        e.encode(np.zeros(64, np.uint8), 4, 4)
    with pytest.raises(jxh.EncodeError, match="3 channels contradict has_alpha"):
        jxh.encoder_builder(lossless=True, has_alpha=True, device=-1).encode(np.zeros(48, np.uint8), 4, 4)
    with pytest.raises(jxh.EncodeError, match="unsupported: samples of type float32"):
        e.encode(np.zeros(48, np.float32), 4, 4)
    with pytest.raises(jxh.EncodeError, match="host-only encoder cannot encode"):
        e.encode(np.zeros(48, np.uint8), 4, 4)
    enc = jxh.LosslessEncoder(-1)
    with pytest.raises(jxh.EncodeError, match="unsupported: samples of type"):
        enc.encode([np.zeros((4, 4), np.int16)])
    with pytest.raises(jxh.EncodeError, match="unsupported: an image of 4 dimensions"):
        enc.encode([np.zeros((1, 4, 4, 3), np.uint8)])
    got = enc.encode([np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 5), np.uint8)], raise_on_error=False)
    assert [type(g) for g in got] == [jxh.EncodeError] * 2 and "num_channels must be 1..4" in str(got[1])


# ---- GPU side ------------------------------------------------------------------------------------------------------------------------------------
def picture(w, h, c=3, dtype=np.uint8, seed=7):
    """the synthesiser's picture in the asked shape: 1 channel = its green; 2 = its red as grey and its green as alpha; 4 = RGB with its red, mirrored, as alpha;
    16 bits = this test's own widening of the 8-bit picture (x 257, the two low bits toggled by the column), not an input the synthesiser itself makes"""
    img = S.synthetic_image(seed, w, h)
    if dtype == np.uint16:
        img = (img.astype(np.uint16) * 257) ^ (np.arange(w, dtype=np.uint16)[None, :, None] & 3)
    if c == 1:
        return np.ascontiguousarray(img[..., 1:2])
    if c == 2:
        return np.ascontiguousarray(img[..., :2])
    if c == 4:
        return np.concatenate([img, img[:, ::-1, :1]], axis=2)
    return img


def back_to_depth(got, bits):
    """full-range samples of the decoder -> the `bits`-deep integers they stand for"""
    full = 8 * got.itemsize
    if bits == full:
        return got
    return np.rint(got.astype(np.float64) * ((1 << bits) - 1) / ((1 << full) - 1)).astype(got.dtype)


def oracle_image(data, src, bits):
    d = O.decode(data)
    i = d.info
    c = src.shape[2]
    assert (i.xsize, i.ysize, i.bits_per_sample, i.num_color_channels, i.num_extra_channels, i.alpha_bits) == (src.shape[1], src.shape[0], bits, 1 if c <= 2 else 3, 1 - c % 2, bits * (1 - c % 2))
    return back_to_depth(d.image("u8" if src.dtype == np.uint8 else "u16"), bits)


def product_decode(jx, datas, srcs, bitss, premultiplied=0):
    """one BatchDecoder for all: -> the decoded arrays, mapped back to their depth; checks the basic info on the way"""
    b = jx.BatchDecoder()
    for data, src in zip(datas, srcs):
        b.add(data, dtype="uint8" if src.dtype == np.uint8 else "uint16", num_channels=src.shape[2])
    b.prepare(); b.decode()
    out = []
    for k, (src, bits) in enumerate(zip(srcs, bitss)):
        i, c = b.info(k), src.shape[2]
        assert (i.xsize, i.ysize, i.bits_per_sample, i.num_color_channels, i.num_extra_channels, i.alpha_bits, i.alpha_premultiplied, i.orientation) == \
            (src.shape[1], src.shape[0], bits, 1 if c <= 2 else 3, 1 - c % 2, bits * (1 - c % 2), premultiplied * (1 - c % 2), 1), k
        out.append(back_to_depth(b.output(k).reshape(src.shape), bits))
    return out


SHAPES = [(1, 1), (1, 9), (9, 1), (64, 1), (65, 3), (256, 256), (257, 255), (255, 257), (300, 280), (2049, 3), (3, 2049)]      # (width, height)
VARIANTS = [(1, np.uint8), (2, np.uint8), (3, np.uint8), (4, np.uint8), (3, np.uint16)]


@pytest.fixture(scope="module")
def geometry(jx):
    """every shape x variant through one encode call and one product decode -> {(shape, variant): (source, bytes, product's decode)}"""
    keys = [(s, v) for s in SHAPES for v in range(len(VARIANTS))]
    srcs = [picture(s[0], s[1], *VARIANTS[v]) for s, v in keys]
    datas = jx.LosslessEncoder().encode(srcs)
    bitss = [8 * a.itemsize for a in srcs]
    dec = product_decode(jx, datas, srcs, bitss)
    return {k: (a, d, p) for k, a, d, p in zip(keys, srcs, datas, dec)}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_geometry_round_trips(jx, geometry, shape):
    """1x1 smallest; 1x9 / 9x1 every edge rule of W / N / NW; 64x1, 65x3 a wavefront boundary; 256x256 exactly one group (single-section TOC); 257x255 / 255x257 groups
    one sample wide / tall; 300x280 four ragged groups; 2049x3 / 3x2049 two LF groups and nine groups in a row (the empty LfGroup slots of the TOC)."""
    import libjxl_probe as P
    found = P.probe()
    for v, (c, dtype) in enumerate(VARIANTS):
        src, data, prod = geometry[(shape, v)]
        assert data[:2] == b"\xff\x0a"
        assert np.array_equal(oracle_image(data, src, 8 * src.itemsize), src), (shape, c, dtype)
        assert np.array_equal(prod, src), (shape, c, dtype)
        assert len(data) <= documented_bound(shape[0], shape[1], c, 8 * src.itemsize)
        if found["available"]:
            ref = P.decode(found, data, "u8" if dtype == np.uint8 else "u16", c)
            assert ref is not None and np.array_equal(ref.reshape(src.shape), src), (shape, c, dtype)


def toc_allowance(w, h):
    groups = -(-w // GD) * -(-h // GD)
    return 2 + 4 * (1 if groups == 1 else 2 + -(-w // 2048) * -(-h // 2048) + groups)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(65, 41), (300, 280)], ids=["65x41", "300x280"])
def test_content_classes(jx, shape):
    w, h = shape
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.zeros((h, w, 3), np.uint16)
    checker[..., 0] = np.where((xx + yy) & 1, 65535, 0)            # R and B alternate between 0 and the maximum in opposite phase: Co swings over its whole range
    checker[..., 2] = 65535 - checker[..., 0]
    cases = {
        "picture": (picture(w, h), 8), "picture_rgba16": (picture(w, h, 4, np.uint16), 16),
        "constant": (np.full((h, w, 3), 77, np.uint8), 8), "constant_grey16": (np.full((h, w, 1), 40000, np.uint16), 16),
        "noise": (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), 8), "noise_rgba16": (rng.integers(0, 65536, (h, w, 4), dtype=np.uint16), 16),
        "checker": (checker, 16),
        "ramp": (np.stack([(xx * 255 // max(1, w - 1)), (yy * 255 // max(1, h - 1)), ((xx + yy) & 255)], axis=2).astype(np.uint8), 8),
        "ramp16": (((xx * 211 + yy * 97) & 65535).astype(np.uint16)[..., None], 16),
        "depth1": (rng.integers(0, 2, (h, w, 1), dtype=np.uint8), 1), "depth1_u16": (rng.integers(0, 2, (h, w, 3), dtype=np.uint16), 1),
        "depth10": (rng.integers(0, 1024, (h, w, 3), dtype=np.uint16), 10), "depth12": (rng.integers(0, 4096, (h, w, 2), dtype=np.uint16), 12),
        "depth5_u8": ((picture(w, h, 4) >> 3), 5),
    }
    names = list(cases)
    srcs, bitss = [cases[n][0] for n in names], [cases[n][1] for n in names]
    enc = jx.LosslessEncoder()
    datas = enc.encode(srcs, bits=bitss)
    prod = product_decode(jx, datas, srcs, bitss)
    size, top = {}, {}
    for k, n in enumerate(names):
        assert np.array_equal(oracle_image(datas[k], srcs[k], bitss[k]), srcs[k]), n
        assert np.array_equal(prod[k], srcs[k]), n
        assert len(datas[k]) <= documented_bound(w, h, srcs[k].shape[2], bitss[k]), n
        size[n], top[n] = len(datas[k]), enc.max_token(k)
        print("%s %dx%d: %d bytes, %.3f of raw, top token %d" % (n, w, h, size[n], size[n] / srcs[k].nbytes, top[n]))
    # each case, the class it is there for
    assert size["constant"] < 200 + toc_allowance(w, h) and size["constant_grey16"] < 200 + toc_allowance(w, h)       # single-symbol histograms, zero-bit codes
    assert size["noise"] > srcs[names.index("noise")].nbytes and size["noise_rgba16"] > srcs[names.index("noise_rgba16")].nbytes      # incompressible (and within the bound, above)
    assert top["checker"] == 71                                                                                      # the largest residuals: the top token
    assert top["noise_rgba16"] >= 68 and top["depth1"] <= 2 and top["constant"] < 32
    assert size["picture"] < 0.7 * srcs[0].nbytes and size["ramp"] < 0.5 * srcs[names.index("ramp")].nbytes


@pytest.mark.gpu
def test_layout_and_determinism(jx):
    import torch
    L = jx.libjxl()
    rng = np.random.default_rng(9)
    enc = jx.LosslessEncoder()
    # a row pitch above tight: a view into a wider array, 8 and 16 bits; the pad holds values that would fail the range check of a 10-bit image
    wide8 = rng.integers(0, 256, (37, 90, 3), dtype=np.uint8)
    wide16 = rng.integers(0, 1024, (280, 310, 3), dtype=np.uint16)
    wide16[:, 300:] = 65535
    v8, v16 = wide8[:, :70], wide16[:, :300]
    assert v8.strides[0] > 70 * 3 and v16.strides[0] > 300 * 6
    pitched = enc.encode([v8, v16], bits=[8, 10])
    tight = enc.encode([np.ascontiguousarray(v8), np.ascontiguousarray(v16)], bits=[8, 10])
    assert pitched == tight
    assert np.array_equal(oracle_image(pitched[0], v8, 8), v8) and np.array_equal(oracle_image(pitched[1], v16, 10), v16)
    # host against device input (contiguous and pitched device tensors): the same bytes
    dev8, dev16 = torch.from_numpy(wide8).cuda(), torch.from_numpy(wide16).cuda()
    assert enc.encode([dev8[:, :70], dev16[:, :300]], bits=[8, 10]) == tight
    assert enc.encode([dev8[:, :70].contiguous()], bits=8) == tight[:1]
    # six images of mixed sizes, channel counts and depths; number 3 carries a sample above its depth
    bad = rng.integers(0, 1024, (41, 65, 3), dtype=np.uint16)
    bad[40, 64, 2] = 1024
    six = [picture(300, 280), picture(65, 41, 1), picture(257, 255, 4, np.uint16), bad, rng.integers(0, 4096, (3, 2049, 2), dtype=np.uint16), picture(9, 1, 2)]
    bits = [8, 8, 16, 10, 12, 8]
    got = enc.encode(six, bits=bits, raise_on_error=False)
    assert isinstance(got[3], jx.EncodeError) and "image 3: a sample is above 2^bits_per_sample - 1" in str(got[3])
    assert L.JxlHipEncoderStatus(enc._h, 3) == 1 and L.JxlHipEncoderSize(enc._h, 3) == 0 and all(L.JxlHipEncoderStatus(enc._h, k) == 0 for k in (0, 1, 2, 4, 5))
    with pytest.raises(jx.EncodeError, match="image 3: a sample is above"):
        enc.encode(six, bits=bits)
    for k in (0, 1, 2, 4, 5):
        assert got[k] == jx.LosslessEncoder().encode([six[k]], bits=bits[k])[0], k          # alone or in a batch: the same bytes
        assert np.array_equal(oracle_image(got[k], six[k], bits[k]), six[k]), k
    # two identical calls
    again = enc.encode(six, bits=bits, raise_on_error=False)
    assert [a if isinstance(a, bytes) else None for a in again] == [g if isinstance(g, bytes) else None for g in got]
    # Copy writes exactly Size bytes and refuses a buffer one byte short
    n = L.JxlHipEncoderSize(enc._h, 0)
    assert n == len(got[0])
    guard = np.full(n + 64, 0xA5, np.uint8)
    assert L.JxlHipEncoderCopy(enc._h, 0, guard.ctypes.data + 32, n) == 0
    assert bytes(guard[32:32 + n]) == got[0] and (guard[:32] == 0xA5).all() and (guard[32 + n:] == 0xA5).all()
    guard[:] = 0xA5
    assert L.JxlHipEncoderCopy(enc._h, 0, guard.ctypes.data + 32, n - 1) == 1 and "too small" in jx.last_error() and (guard == 0xA5).all()
    # the Python mirror of encode.rs on the same image
    r = jx.encoder_builder(lossless=True, has_alpha=True).encode(six[2].reshape(-1), 257, 255)
    assert isinstance(r, jx.EncoderResult) and r.data == got[2]
    assert jx.encode_lossless([six[1]])[0] == got[1]


@pytest.mark.gpu
def test_premultiplied_flag_is_written_as_given(jx):
    """alpha_premultiplied = 1 takes the header's explicit ExtraChannelInfo (at 8 bits the default alpha channel cannot say it); the samples are stored as they are."""
    srcs = [picture(65, 41, 4), picture(65, 41, 2), picture(300, 280, 4, np.uint16), picture(9, 1, 2, np.uint16)]
    bitss = [8, 8, 16, 16]
    enc = jx.LosslessEncoder()
    plain, premul = enc.encode(srcs), enc.encode(srcs, alpha_premultiplied=True)
    for flag, datas in ((0, plain), (1, premul)):
        dec = product_decode(jx, datas, srcs, bitss, premultiplied=flag)          # (asserts BatchDecoder.info(k).alpha_premultiplied == flag)
        for a, d, p, bits in zip(srcs, datas, dec, bitss):
            assert np.array_equal(oracle_image(d, a, bits), a) and np.array_equal(p, a)          # neither decoder unpremultiplies unless asked to
    assert all(a != b for a, b in zip(plain, premul))                             # the flag is in the stream ...
    assert all(abs(len(a) - len(b)) <= 4 for a, b in zip(plain, premul))          # ... and only in its header
    # an image without alpha has nowhere to put it: the same bytes
    rgb = picture(65, 41)
    assert enc.encode([rgb], alpha_premultiplied=True) == enc.encode([rgb])


@pytest.mark.gpu
def test_compression_against_the_synthesiser(jx):
    """A broken histogram or a fixed code would still round-trip; it would not compress.  The synthesiser's prefix-coded Modular stream of the same image (same model
    class: fixed gradient tree, RCT 6, clustered histograms) is the yardstick; this encoder's stream may be at most 10 % larger (a margin chosen, not derived: another
    tree or clustering costs a few per cent, a wrong code tens)."""
    srcs = [picture(200, 136, 3, seed=11), picture(520, 300, 4, seed=11), picture(257, 255, 3, np.uint16, seed=11)]
    datas = jx.encode_lossless(srcs)
    S.set_prefix(True)
    try:
        refs = [S.encode_modular(a, bits=8 * a.itemsize, rct=True) for a in srcs]
    finally:
        S.set_prefix(False)
    for a, d, r in zip(srcs, datas, refs):
        assert np.array_equal(O.decode(r).image("u8" if a.itemsize == 1 else "u16"), a)                # (the yardstick itself is a valid stream of this image)
        print("%dx%dx%d %s: %d bytes = %.3f of raw; synthesiser %d = %.3f of raw; ratio %.4f" % (a.shape[1], a.shape[0], a.shape[2], a.dtype, len(d), len(d) / a.nbytes, len(r), len(r) / a.nbytes, len(d) / len(r)))
        assert len(d) <= 1.10 * len(r)
        assert np.array_equal(oracle_image(d, a, 8 * a.itemsize), a)
