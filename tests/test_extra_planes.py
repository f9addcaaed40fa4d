"""Extra-channel planes beside the colour output, all from one decode (include/jxl_hip.h JxlHipOutputPlanes; OutputSpec::planes, EcPlanesOutKernel).

Where the expected values come from.  A lossless plane is pinned against the plane handed to the synthesiser (tests/synth_extra.py), which shares nothing with the
decoder; a blended or patched plane against the oracle's decode of the stream's twin whose only alpha-typed channel is that one (test_many_extra_channels.py has the
scheme and the streams: `oracle_plane`).  Nothing is compared with the product's own alpha_from_extra decode.  Formats, orientations and layouts follow from a plain
float32 plane by numpy (the scheme of test_write_stage.py); a resized plane is held against the float64 restatement of the filter over the plain float32 plane with the
derived bound of test_resample_jobs.py.

The float32 fused multiply-add of the scale / bias test is restated exactly: the product of two float32 values is exact in float64; TwoSum gives the error of the
float64 sum, and where there is one the sum is moved to the neighbouring ODD float64 on the error's side (round to odd), which a 53-bit format may do for a 24-bit
target (53 >= 2 x 24 + 2) without changing the float32 the exact value rounds to.
"""
import ctypes as C
import functools
import numpy as np
import pytest
import oracle_lib as O
import synth_lib as S
import synth_extra as X
import test_many_extra_channels as M
from test_write_stage import convert_samples, padded_stride
from test_resample_jobs import restate

FILL, FRONT, EXTRA = 0xA5, 128, 320
BPS = {"uint8": 1, "uint16": 2, "float16": 2, "float32": 4}
SIZES = [(1, 1), (63, 5), (64, 1), (65, 41), (300, 280)]      # the last: four groups with a ragged corner


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


# ---- streams -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def simple(kind, n, w, h, orientation=1, seed=0):
    """a single-frame image without features, n lossless extra channels (8 and 16 bits from n = 4 on) -> (stream, source planes, extras)"""
    ex, a = M._extras(n, blend=False)
    pl = M._planes(n, w, h, 40 + seed, ex)
    S.set_orientation(orientation)
    try:
        if kind == "vardct":
            data = X.encode_vardct_ec(S.synthetic_image(7 + seed, max(w, 8), max(h, 8))[:h, :w], pl, ex, S.frame(), color_alpha=a, seed=5 + seed)
        else:
            data = X.encode_modular_ec(S.synthetic_image(7 + seed, max(w, 8), max(h, 8))[:h, :w].astype(np.int32), pl, ex, S.frame(), color_alpha=a)
    finally:
        S.set_orientation(1)
    return data, pl, ex


def orient(a, o):
    """(h, w) array as orientation o (EXIF numbering) shows it"""
    return [a, a[:, ::-1], a[::-1, ::-1], a[::-1], a.T, a[::-1].T, a[::-1, ::-1].T, a[:, ::-1].T][o - 1]


def fmaf32(v, s, b):
    """float32 fmaf(v, s, b), exact (module docstring)"""
    p = np.asarray(v, np.float32).astype(np.float64) * np.float64(np.float32(s))
    bb = np.float64(np.float32(b))
    t = p + bb
    bv = t - p
    e = (p - (t - bv)) + (bb - bv)
    even = (t.view(np.int64) & 1) == 0
    moved = np.where(e > 0, np.nextafter(t, np.inf), np.where(e < 0, np.nextafter(t, -np.inf), t))
    return np.where(even & (e != 0), moved, t).astype(np.float32)


def test_fmaf32_restatement():
    from fractions import Fraction
    rng = np.random.RandomState(3)
    v = np.concatenate([rng.uniform(-2, 2, 4000), [0.0, 1.0, 1 / 3, 0.1]]).astype(np.float32)
    for s, b in ((1 / 0.229, -0.485 / 0.229), (3.7, 0.125), (-0.5, 1.0), (1.0000001, -1.0)):
        got = fmaf32(v, s, b)
        for x, g in zip(v[:600], got[:600]):
            exact = Fraction(float(x)) * Fraction(float(np.float32(s))) + Fraction(float(np.float32(b)))
            lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
            assert abs(Fraction(float(g)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))


# ---- one batch, many outputs ---------------------------------------------------------------------------------------------------------------------
def decode_items(jx, items, keep_orientation=False):
    """items: (data, BatchDecoder.add keywords).  Every item is one image of ONE batch, decoded into a device buffer of out_size + EXTRA bytes filled with FILL, the
    destination FRONT bytes into it.  -> (list of dicts: dest (whole buffer, uint8), size, layout (offset, pitch, total), dims of the stored image), the batch)"""
    import torch
    b = jx.BatchDecoder(0)
    b.set_option("keep_orientation", 1 if keep_orientation else 0)
    bufs, res = [], []
    for data, sp in items:
        size = jx.image_out_size(data, **{k: v for k, v in sp.items() if k not in ("filter", "mirror")})[1]
        t = torch.full((size + EXTRA,), FILL, dtype=torch.uint8, device="cuda:0")
        i = b.add(data, device_ptr=t.data_ptr() + FRONT, **sp)
        assert b.out_size(i) == size and b.planes_layout(i)[2] == size, (sp, b.out_size(i), size)
        bufs.append(t)
        res.append(dict(size=size, layout=b.planes_layout(i), dims=(b.info(i).xsize, b.info(i).ysize)))
    b.prepare(); b.decode(); b.finish()
    torch.cuda.synchronize()
    for r, t in zip(res, bufs):
        r["dest"] = t.cpu().numpy()
        assert (r["dest"][:FRONT] == FILL).all() and (r["dest"][FRONT + r["size"]:] == FILL).all(), "written outside the destination"
    return res, b


def plane_rows(r, k, w, h, dtype, align=0):
    """plane k of result r as an (h, w) array of `dtype`'s native-endian integer view (u8, u16, the bits of f16 as u16, of f32 as u32); the row padding is checked to hold FILL"""
    off, pitch, _ = r["layout"]
    stride = padded_stride(w * BPS[dtype], align)
    raw = r["dest"][FRONT + off + k * pitch:FRONT + off + k * pitch + h * stride].reshape(h, stride)
    assert (raw[:, w * BPS[dtype]:] == FILL).all()
    tail = r["dest"][FRONT + off + k * pitch + h * stride:FRONT + off + (k + 1) * pitch]
    assert (tail == FILL).all()
    view = {"uint8": np.uint8, "uint16": np.uint16, "float16": np.uint16, "float32": np.uint32}[dtype]
    return np.ascontiguousarray(raw[:, :w * BPS[dtype]]).view(view)


def f32_planes(r, m, w, h):
    return [plane_rows(r, k, w, h, "float32").view(np.float32) for k in range(m)]


def colour_of(r, w, h, nch, dtype):
    """the interleaved colour output of result r as a flat array of the sample type"""
    n = w * h * nch * BPS[dtype]
    return r["dest"][FRONT:FRONT + n].copy()


FORMATS = [("uint8", "LE"), ("uint16", "LE"), ("uint16", "BE"), ("float16", "LE"), ("float32", "LE")]


def want_samples(f32, dtype, order):
    q = convert_samples(f32, dtype)
    return q.byteswap() if order == "BE" else q


def endian(jx, order):
    return jx.JXL_BIG_ENDIAN if order == "BE" else jx.JXL_LITTLE_ENDIAN


# ---- CPU: sizes, layout, refusals ------------------------------------------------------------------------------------------------------------------
def test_size_and_layout_arithmetic(jxh):
    """every sample type x colour channels 1 - 4 x align {0, 64} x {interleaved, tight planar, padded plane_stride} x m in {1, 3, 9} x explicit offset, on a transposed
    image (orientation 6: the oriented picture is 41 x 65 for a stored 65 x 41)"""
    jx = jxh
    data, _, _ = simple("modular", 9, 65, 41, orientation=6)
    ow, oh = 41, 65
    b = jx.BatchDecoder(-1)
    for dtype, bps in BPS.items():
        for nch in (1, 2, 3, 4):
            for align in (0, 64):
                for mode in ("interleaved", "planar", "padded"):
                    for m in (1, 3, 9):
                        for explicit in (0, 1):
                            crow = padded_stride(ow * bps * (nch if mode == "interleaved" else 1), align)
                            prow = padded_stride(ow * bps, align)
                            kw = dict(dtype=dtype, num_channels=nch, align=align, extra_planes=list(range(m)))
                            if mode == "interleaved":
                                colour = crow * (oh - 1) + ow * nch * bps
                                offset, pitch = (colour + 15) // 16 * 16, prow * oh
                            else:
                                cplane = crow * oh + (52 * bps if mode == "padded" else 0)
                                kw.update(planar=True, plane_stride=cplane if mode == "padded" else 0)
                                offset, pitch = nch * cplane, cplane
                            if explicit:
                                offset += 48 * bps
                                pitch += 20 * bps
                                kw.update(planes_offset=offset, planes_stride=pitch)
                            total = offset + m * pitch
                            assert jx.image_out_size(data, **kw)[1] == total, kw
                            b.reset()
                            i = b.add(data, **kw)
                            assert b.planes_layout(i) == (offset, pitch, total) and b.out_size(i) == total, kw
    # an offset / pitch below the default, or no multiple of the sample size
    for kw, text in ((dict(planes_offset=16), "offset 16 is below the default"), (dict(planes_stride=2 * 41), "plane_stride 82 is below the default"),
                     (dict(planes_offset=3 * 41 * 65 * 2 + 33), "offset must be a multiple of the sample size"), (dict(planes_stride=41 * 65 * 2 + 1), "plane_stride must be a multiple")):
        with pytest.raises(jx.DecodeError, match=text):
            jx.image_out_size(data, dtype="uint16", num_channels=3, planar=True, extra_planes=[0], **kw)
    with pytest.raises(ValueError, match="need extra_planes"):
        jx.image_out_size(data, planes_offset=64)


def test_refusals(jxh):
    """Every refusal with its message: "unsupported: extra planes ..." (host-only batch, the stand-alone size query, a pipeline submission's arguments).  Previews and
    the C calls of libjpeg-exact jobs have no argument that carries plane requests, so there is nothing to refuse (JxlDecoderSetPreviewOutBuffer takes a pixel format alone)."""
    jx = jxh
    data, _, _ = simple("modular", 2, 65, 41)
    b = jx.BatchDecoder(-1)
    with pytest.raises(jx.DecodeError, match="unsupported: extra planes of extra channel 2: the image has 2 extra channels"):
        b.add(data, extra_planes=[0, 2])
    with pytest.raises(jx.DecodeError, match="unsupported: extra planes of extra channel 2"):
        jx.image_out_size(data, extra_planes=[2])
    for dtype in ("uint8", "uint16"):
        with pytest.raises(jx.DecodeError, match="unsupported: extra planes with scale / bias need a float sample type"):
            b.reset(); b.add(data, dtype=dtype, extra_planes=[0], plane_scale=[2.0])
        with pytest.raises(jx.DecodeError, match="unsupported: extra planes with scale / bias need a float sample type"):
            jx.image_out_size(data, dtype=dtype, extra_planes=[1], plane_bias=[0.5])
    plain = S.encode_vardct(S.synthetic_image(3, 64, 48), seed=2)
    with pytest.raises(jx.DecodeError, match="unsupported: extra planes of the 1:8 decode"):
        jx.image_out_size(plain, downscale=8, extra_planes=[0])
    # (the batch path: the 1:8 colour output of a plain VarDCT image is taken, the planes behind it are refused in their own words)
    with pytest.raises(jx.DecodeError, match="unsupported: extra planes of the 1:8 decode"):
        b.reset(); b.add(plain, downscale=8, extra_planes=[0])
    # libjpeg-exact outputs: jpeg_scale, the integer resample, jobs of libjpeg-exact pixels
    with pytest.raises(jx.DecodeError, match="unsupported: extra planes beside a libjpeg-exact output"):
        jx.image_out_size(data, jpeg_scale=2, extra_planes=[0])
    L = jx.libjxl()
    import jpeg_cases as JC
    import jpeg_tools as J
    from test_jpeg_exact_pixels import make_jpeg
    ycc = J.transcode(make_jpeg(JC.photo(64, 48, seed=1), 0, 85))
    b.reset()
    i = b.add(ycc, dtype="uint8", num_channels=3, jpeg_scale=2)
    idx = (C.c_uint32 * 1)(0)
    req = jx.JxlHipOutputPlanes(1, C.cast(idx, C.POINTER(C.c_uint32)), 0, 0, None, None)
    assert L.JxlHipBatchSetOutputPlanes(b._h, i, C.byref(req)) != 0 and "unsupported: extra planes beside a libjpeg-exact output" in jx.last_error()
    b.reset()
    i = b.add(ycc, dtype="uint8", num_channels=3, resize=(32, 24), resize_u8=True)
    assert L.JxlHipBatchSetOutputPlanes(b._h, i, C.byref(req)) != 0 and "unsupported: extra planes beside a libjpeg-exact output" in jx.last_error()
    # kept animation canvases
    b.reset()
    b.set_option("output_all_frames", 1)
    i = b.add(data, dtype="uint8", num_channels=3)
    b.set_option("output_all_frames", 0)
    assert L.JxlHipBatchSetOutputPlanes(b._h, i, C.byref(req)) != 0 and "unsupported: extra planes of kept animation canvases" in jx.last_error()
    # a request without indices, too many requests
    none = jx.JxlHipOutputPlanes(1, None, 0, 0, None, None)
    b.reset()
    i = b.add(data)
    assert L.JxlHipBatchSetOutputPlanes(b._h, i, C.byref(none)) != 0 and "no list of extra-channel indices" in jx.last_error()
    with pytest.raises(jx.DecodeError, match="unsupported: extra planes beyond 4096 requests"):
        jx.image_out_size(data, extra_planes=[0] * 4097)
    assert jx.image_out_size(data, dtype="uint8", num_channels=3, extra_planes=[1] * 4096)[1] == (65 * 41 * 3 + 15) // 16 * 16 + 4096 * 65 * 41


def test_refusals_of_pipeline_arguments(jxh):
    """what the Python layer and the C call refuse before a pipeline exists: planes in a libjpeg-exact job"""
    jx = jxh
    with pytest.raises(jx.DecodeError, match="unsupported: extra planes beside a libjpeg-exact output"):
        jx.Pipeline.submit(None, [b""], jpeg_pixels=True, extra_planes=[0])


def test_a_refused_request_leaves_the_output_that_was_set(jxh):
    """A JxlHipBatchSetOutputPlanes call that fails — an offset or pitch below its default or no multiple of the sample size, a channel the image does not have — leaves
    layout and size of the image as they were: over a colour-only output (also through add(), which has set the colour output when the planes are refused) and over an
    output that had planes."""
    jx = jxh
    data, _, _ = simple("modular", 2, 65, 41)
    L = jx.libjxl()
    colour = 65 * 41 * 3 * 2
    fmt = dict(dtype="uint16", num_channels=3, planar=True)
    bad = [(dict(planes_offset=16), "offset 16 is below the default"), (dict(planes_stride=2 * 41), "plane_stride 82 is below the default"),
           (dict(planes_offset=colour + 33), "offset must be a multiple of the sample size"), (dict(planes_stride=65 * 41 * 2 + 1), "plane_stride must be a multiple"),
           (dict(extra=[0, 2]), "unsupported: extra planes of extra channel 2")]
    b = jx.BatchDecoder(-1)
    for kw, text in bad:
        kw = dict(kw)
        idx = kw.pop("extra", [1, 0])
        # over a colour-only output, through add(): the image is in the batch with its colour output
        b.reset()
        with pytest.raises(jx.DecodeError, match=text):
            b.add(data, extra_planes=idx, **fmt, **kw)
        off, pitch, total = C.c_size_t(), C.c_size_t(), C.c_size_t()
        assert L.JxlHipBatchOutputPlanesLayout(b._h, 0, C.byref(off), C.byref(pitch), C.byref(total)) == 0
        assert (off.value, pitch.value, total.value) == (colour, 0, colour), (kw, off.value, pitch.value, total.value)
        # over an output with planes
        b.reset()
        i = b.add(data, extra_planes=[1, 0, 1], **fmt)
        before = b.planes_layout(i)
        assert before == (colour, colour // 3, colour + 3 * (colour // 3)) and b.out_size(i) == before[2]
        req = jx._planes(idx, None, None, kw.get("planes_offset", 0), kw.get("planes_stride", 0))
        assert L.JxlHipBatchSetOutputPlanes(b._h, i, C.byref(req)) != 0 and text in jx.last_error(), kw
        assert b.planes_layout(i) == before and b.out_size(i) == before[2], kw
    # ... and the same for a colour output that is refused: a plane_stride the image does not fit, over an output with planes
    b.reset()
    i = b.add(data, extra_planes=[0], **fmt)
    before = b.planes_layout(i)
    lay = jx._layout(True, 64, None, None)
    f = jx.JxlPixelFormat(3, jx._PIXEL_TYPES["uint16"][0], jx.JXL_NATIVE_ENDIAN, 0)
    assert L.JxlHipBatchSetOutputLayout(b._h, i, C.byref(f), None, 1, C.byref(lay)) != 0 and "plane_stride 64 is below" in jx.last_error()
    assert b.planes_layout(i) == before


def test_a_later_set_output_clears_the_planes(jxh):
    jx = jxh
    data, _, _ = simple("modular", 2, 65, 41)
    L = jx.libjxl()
    b = jx.BatchDecoder(-1)
    i = b.add(data, dtype="uint8", num_channels=3, extra_planes=[1, 0])
    colour = 65 * 41 * 3
    assert b.planes_layout(i) == ((colour + 15) // 16 * 16, 65 * 41, (colour + 15) // 16 * 16 + 2 * 65 * 41)
    fmt = jx.JxlPixelFormat(3, jx._PIXEL_TYPES["uint8"][0], jx.JXL_LITTLE_ENDIAN, 0)
    assert L.JxlHipBatchSetOutput(b._h, i, C.byref(fmt), None) == 0
    assert b.planes_layout(i) == (colour, 0, colour)
    # ... and so does an empty request
    assert L.JxlHipBatchSetOutputPlanes(b._h, i, C.byref(b._planes[i])) == 0 and b.planes_layout(i)[2] > colour
    assert L.JxlHipBatchSetOutputPlanes(b._h, i, None) == 0 and b.planes_layout(i) == (colour, 0, colour)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------------
def check_colour(jx, r, stream, w, h, dtype, order):
    if dtype == "float16":
        return
    ctype = {"uint8": "u8", "uint16": "u16", "float32": "f32"}[dtype]
    got = colour_of(r, w, h, 3, dtype).view({"uint8": np.uint8, "uint16": np.uint16, "float32": np.float32}[dtype])
    if order == "BE":
        got = got.byteswap()
    M.assert_colour(got, stream, ctype)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["modular", "vardct"])
@pytest.mark.parametrize("n", [1, 2, 5, 9])
def test_lossless_planes_of_simple_images(jx, kind, n):
    """Planes of single-frame images without features = the planes handed to the synthesiser, in every sample type; a permuted list with repeats; the colour output of
    these images — which take the frame tail because of the planes — against the oracle."""
    perm = list(reversed(range(n))) + [0, n - 1, 0]
    items, meta = [], []
    for w, h in SIZES:
        data, pl, ex = simple(kind, n, w, h)
        for dtype, order in FORMATS:
            idx = perm if dtype == "float32" else list(range(n))
            items.append((data, dict(dtype=dtype, num_channels=3, endianness=endian(jx, order), extra_planes=idx)))
            meta.append((data, pl, ex, w, h, dtype, order, idx))
    res, b = decode_items(jx, items)
    assert b.info_value("plane_outputs") == sum(len(m[7]) for m in meta)
    for r, (data, pl, ex, w, h, dtype, order, idx) in zip(res, meta):
        for k, e in enumerate(idx):
            want = want_samples(M._as_float(pl[e], ex[e]), dtype, order)
            got = plane_rows(r, k, w, h, dtype)
            assert np.array_equal(got, want), (kind, n, (w, h), dtype, order, k, e, int((got != want).sum()))
        check_colour(jx, r, data, w, h, dtype, order)


@pytest.mark.gpu
def test_float16_channel(jx):
    data, pl, ex = M.float_stream(None, 5)
    assert ex[2].exp_bits == 5
    items = [(data, dict(dtype=d, num_channels=3, endianness=endian(jx, o), extra_planes=[2, 0, 4])) for d, o in FORMATS]
    res, _ = decode_items(jx, items)
    for r, (dtype, order) in zip(res, FORMATS):
        for k, e in enumerate([2, 0, 4]):
            assert np.array_equal(plane_rows(r, k, M.W, M.H, dtype), want_samples(M._as_float(pl[e], ex[e]), dtype, order)), (dtype, order, e)
        check_colour(jx, r, data, M.W, M.H, dtype, order)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["layered-modular", "layered-vardct", "patched"])
def test_layered_and_patched_images(jx, what):
    """Two frames, the second cropped, six channels under the five blend modes / a patched frame: every plane = the oracle twin's alpha, f32 bit for bit; the colour bytes
    = the decode of the same image without planes, byte for byte (these images took the frame tail already)."""
    if what == "patched":
        data, make = M.patched(None, False, 6), (lambda e: M.patched(e, False, 6))
    else:
        kind = what.split("-")[1]
        data, make = M.layered(kind, 6)[0], (lambda e: M.layered(kind, 6, relabel=e)[0])
    f = dict(dtype="float32", num_channels=3, endianness=jx.JXL_LITTLE_ENDIAN)
    u = dict(dtype="uint8", num_channels=4)
    res, b = decode_items(jx, [(data, dict(f, extra_planes=list(range(6)))), (data, f), (data, dict(u, extra_planes=[5, 0])), (data, u)])
    assert b.info_value("plane_outputs") == 8
    for e, got in enumerate(f32_planes(res[0], 6, M.W, M.H)):
        want = M.oracle_plane(make, e)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, e, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    assert np.array_equal(colour_of(res[0], M.W, M.H, 3, "float32"), colour_of(res[1], M.W, M.H, 3, "float32"))
    assert np.array_equal(colour_of(res[2], M.W, M.H, 4, "uint8"), colour_of(res[3], M.W, M.H, 4, "uint8"))
    for k, e in enumerate([5, 0]):
        assert np.array_equal(plane_rows(res[2], k, M.W, M.H, "uint8"), convert_samples(M.oracle_plane(make, e), "uint8")), e


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["modular", "vardct"])
def test_orientations(jx, kind):
    """Orientations 1 - 8 and keep_orientation: each f32 plane = numpy's re-orientation of the orientation-1 f32 plane; every integer / f16 / big-endian plane = numpy
    applied to that f32 plane."""
    w, h, n = 65, 41, 2
    f = dict(dtype="float32", num_channels=3, endianness=jx.JXL_LITTLE_ENDIAN, extra_planes=[1, 0])
    (r1,), _ = decode_items(jx, [(simple(kind, n, w, h)[0], f)])
    base = f32_planes(r1, 2, w, h)
    src, ex = simple(kind, n, w, h)[1:]
    assert all(np.array_equal(base[k], M._as_float(src[e], ex[e])) for k, e in enumerate([1, 0]))
    items = []
    for o in range(1, 9):
        data = simple(kind, n, w, h, orientation=o)[0]
        items += [(data, dict(dtype=d, num_channels=3, endianness=endian(jx, od), align=64 if d == "uint16" else 0, extra_planes=[1, 0])) for d, od in FORMATS]
    res, _ = decode_items(jx, items)
    for o in range(1, 9):
        ow, oh = (h, w) if o > 4 else (w, h)
        for (dtype, order), r in zip(FORMATS, res[(o - 1) * 5:o * 5]):
            for k in range(2):
                want = want_samples(np.ascontiguousarray(orient(base[k], o)), dtype, order)
                assert np.array_equal(plane_rows(r, k, ow, oh, dtype, 64 if dtype == "uint16" else 0), want), (kind, o, dtype, order, k)
    kept, _ = decode_items(jx, [(simple(kind, n, w, h, orientation=o)[0], f) for o in (3, 6, 8)], keep_orientation=True)
    for r in kept:
        for k in range(2):
            assert np.array_equal(f32_planes(r, 2, w, h)[k], base[k])


@pytest.mark.gpu
def test_one_tensor(jx):
    """Planar f16, 3 colour + 4 extra planes, scale / bias on colour and planes, an align that pads, plane_stride + 52 samples, into a guarded destination: everything
    outside the samples keeps the fill value; each f16 sample = numpy's float16 of the float32 fmaf applied to the plain f32 sample."""
    w, h, n = 65, 41, 5
    data, _, _ = simple("vardct", n, w, h)
    idx = [4, 0, 3, 3]
    scale, bias = [1 / 0.229, 1.0, 3.7], [-0.485 / 0.229, 0.0, 0.125]
    pscale, pbias = [2.0, -0.5, 1 / 3, 1.0], [0.25, 1.0, -0.1, 0.0]
    row = padded_stride(w * 2, 64)
    assert row > w * 2
    stride = row * h + 52 * 2
    plain = dict(dtype="float32", num_channels=3, endianness=jx.JXL_LITTLE_ENDIAN, planar=True, extra_planes=idx)
    tensor = dict(dtype="float16", num_channels=3, endianness=jx.JXL_LITTLE_ENDIAN, planar=True, plane_stride=stride, align=64, scale=scale, bias=bias, extra_planes=idx,
                  plane_scale=pscale, plane_bias=pbias)
    (rp, rt), _ = decode_items(jx, [(data, plain), (data, tensor)])
    assert rp["layout"] == (3 * w * h * 4, w * h * 4, 7 * w * h * 4) and rt["layout"] == (3 * stride, stride, 7 * stride)
    v = rp["dest"][FRONT:FRONT + 7 * w * h * 4].view(np.float32).reshape(7, h, w)
    got = rt["dest"][FRONT:FRONT + 7 * stride].reshape(7, stride)
    for c in range(7):
        s, bs = (scale[c], bias[c]) if c < 3 else (pscale[c - 3], pbias[c - 3])
        want = fmaf32(v[c], s, bs).astype(np.float16).view(np.uint16)
        rows = got[c, :row * h].reshape(h, row)
        assert np.array_equal(np.ascontiguousarray(rows[:, :w * 2]).view(np.uint16), want), c
        assert (rows[:, w * 2:] == FILL).all() and (got[c, row * h:] == FILL).all(), c


@pytest.mark.gpu
def test_resized_planes(jx):
    """203 x 139 -> 48 x 32 triangle and -> 224 x 224 cubic, a crop touching an edge, mirror, target width 1: each f32 plane within the derived bound of
    test_resample_jobs.py of the float64 restatement over the plain f32 plane; a target of the source's size is the plain plane, exactly; the planes of all images are
    resampled by the one-slot groups beside the colour groups."""
    w, h, n = 203, 139, 2
    data, pl, ex = simple("modular", n, w, h, seed=1)
    f = dict(dtype="float32", num_channels=3, endianness=jx.JXL_LITTLE_ENDIAN, extra_planes=[1, 0])
    cases = [dict(resize=(48, 32), filter="bilinear"), dict(resize=(224, 224), filter="bicubic"), dict(resize=(48, 32), crop=(103, 0, 100, 90), filter="bicubic"),
             dict(resize=(48, 32), filter="bilinear", mirror=True), dict(resize=(1, 32), filter="bicubic"), dict(resize=(w, h), filter="bicubic")]
    res, b = decode_items(jx, [(data, f)] + [(data, dict(f, **c)) for c in cases])
    # two groups of the resample table: the colour entries (three slots) and the plane entries (one slot), a launch pair each
    assert b.info_value("resize_launches") == 4 and b.info_value("plane_outputs") == 2 * (1 + len(cases))
    plain = f32_planes(res[0], 2, w, h)
    assert all(np.array_equal(plain[k], M._as_float(pl[e], ex[e])) for k, e in enumerate([1, 0]))
    for c, r in zip(cases, res[1:]):
        tw, th = c["resize"]
        got = f32_planes(r, 2, tw, th)
        for k in range(2):
            src = plain[k]
            if "crop" in c:
                x0, y0, cw, ch = c["crop"]
                src = src[y0:y0 + ch, x0:x0 + cw]
            g = got[k][:, ::-1] if c.get("mirror") else got[k]
            if (tw, th) == (w, h):
                assert np.array_equal(g, src), k
                continue
            want, (tx, ty), (lx, ly) = restate(src[..., None], (tw, th), c["filter"])
            bound = (tx + ty + 8) * 2.0 ** -24 * lx * ly * float(np.abs(src).max())
            err = float(np.abs(g.astype(np.float64) - want[..., 0]).max())
            print(c, "plane", k, "max error", err, "bound", bound)
            assert np.isfinite(g).all() and err <= bound, (c, k, err, bound)
    # every format of a resized plane follows from its f32 plane
    spec = dict(resize=(48, 32), filter="bicubic", mirror=True, num_channels=3, extra_planes=[1, 0])
    res, _ = decode_items(jx, [(data, dict(spec, dtype=d, endianness=endian(jx, o))) for d, o in FORMATS])
    ref = f32_planes(res[4], 2, 48, 32)
    for (dtype, order), r in zip(FORMATS, res):
        for k in range(2):
            assert np.array_equal(plane_rows(r, k, 48, 32, dtype), want_samples(ref[k], dtype, order)), (dtype, order, k)


@pytest.mark.gpu
def test_pipeline_job(jx):
    """A job of three differently sized images, each with two extra planes, into slices of one [3, 5, 32, 48] device tensor and into pinned host memory = the batch
    results.  An image whose channel list names a channel it does not have, and a capacity one byte short, fail alone.  Planes, plain and planes jobs run through one
    pipeline."""
    import torch
    datas = [simple("modular", 2, 65, 41)[0], simple("vardct", 2, 300, 280)[0], simple("modular", 5, 203, 139, seed=1)[0]]
    n = 3
    lay = dict(dtype="float32", num_channels=3, endianness=jx.JXL_LITTLE_ENDIAN, planar=True, resize=(48, 32), filter="bicubic", extra_planes=[1, 0])
    one = 5 * 32 * 48 * 4
    res, _ = decode_items(jx, [(d, lay) for d in datas])
    refs = [r["dest"][FRONT:FRONT + one].copy() for r in res]
    assert all(r["size"] == one for r in res) and len({x.tobytes() for x in refs}) == 3
    p = jx.Pipeline(0, jobs_in_flight=2, lf_streams=2, prepare_threads=1, parse_threads=2, reserve_frames=3, reserve_width=320, reserve_height=320)
    try:
        out = torch.full((n, 5, 32, 48), 7.0, dtype=torch.float32, device="cuda:0")
        st, _ = p.wait(p.submit(datas, device_ptrs=[out[k].data_ptr() for k in range(n)], capacities=[one] * n, **lay))
        torch.cuda.synchronize()
        assert st == [0] * n
        got = out.cpu().numpy()
        for k in range(n):
            assert np.array_equal(got[k].view(np.uint8).reshape(-1), refs[k]), k
        pinned = jx.PinnedBuffer(n * one)
        st, _ = p.wait(p.submit(datas, host_ptrs=[pinned.ptr + k * one for k in range(n)], capacities=[one] * n, **lay))
        assert st == [0] * n and np.array_equal(pinned.array, np.concatenate(refs))
        # channel 4: only image 2 has it
        lay4 = dict(lay, extra_planes=[4, 0])
        (r4,), _ = decode_items(jx, [(datas[2], lay4)])
        pinned = [jx.PinnedBuffer(one) for _ in datas]
        st, _ = p.wait(p.submit(datas, host_ptrs=[o.ptr for o in pinned], capacities=[one] * n, **lay4), check=False)
        assert st == [1, 1, 0] and "unsupported: extra planes of extra channel 4" in jx.last_error()
        assert np.array_equal(pinned[2].array, r4["dest"][FRONT:FRONT + one])
        # one byte short: that image alone
        pinned = [jx.PinnedBuffer(one) for _ in datas]
        st, _ = p.wait(p.submit(datas, host_ptrs=[o.ptr for o in pinned], capacities=[one, one - 1, one], **lay), check=False)
        assert st == [0, 1, 0] and "too small" in jx.last_error()
        for k in (0, 2):
            assert np.array_equal(pinned[k].array, refs[k]), k
        # a 1:8 job with planes is refused as a whole
        with pytest.raises(jx.DecodeError, match="unsupported: extra planes of the 1:8 decode"):
            p.submit(datas, host_ptrs=[o.ptr for o in pinned], downscale=8, extra_planes=[0])
        # planes, plain, planes
        plain_refs = [O.decode(d).pixels("u8", 3) for d in datas]
        a, c = [jx.PinnedBuffer(one) for _ in datas], [jx.PinnedBuffer(one) for _ in datas]
        bb = [jx.PinnedBuffer(r.size) for r in plain_refs]
        t1 = p.submit(datas, host_ptrs=[o.ptr for o in a], capacities=[one] * n, **lay)
        t2 = p.submit(datas, "uint8", 3, host_ptrs=[o.ptr for o in bb], capacities=[r.size for r in plain_refs])
        t3 = p.submit(datas, host_ptrs=[o.ptr for o in c], capacities=[one] * n, **lay)
        assert p.wait(t1)[0] == [0] * n and p.wait(t2)[0] == [0] * n and p.wait(t3)[0] == [0] * n
        for o, r in zip(a + c, refs + refs):
            assert np.array_equal(o.array, r)
        for o, r in zip(bb, plain_refs):
            assert np.array_equal(np.array(o.array), r.reshape(-1).view(np.uint8))
    finally:
        p.close()


@pytest.mark.gpu
def test_planes_do_not_outlive_their_output(jx):
    """a decode without planes after one with planes, from the same reset BatchDecoder = a fresh decode; plane_outputs is m, then 0"""
    data, _, _ = simple("vardct", 5, 300, 280)
    b = jx.BatchDecoder(0)
    b.add(data, dtype="uint8", num_channels=4, extra_planes=[0, 1, 2])
    b.prepare(); b.decode(); b.finish()
    assert b.info_value("plane_outputs") == 3
    b.reset()
    i = b.add(data, dtype="uint8", num_channels=4)
    b.prepare(); b.decode(); b.finish()
    assert b.info_value("plane_outputs") == 0 and b.planes_layout(i) == (300 * 280 * 4, 0, 300 * 280 * 4)
    again = b.output(i)
    fresh = jx.BatchDecoder(0)
    j = fresh.add(data, dtype="uint8", num_channels=4)
    fresh.prepare(); fresh.decode(); fresh.finish()
    assert np.array_equal(again, fresh.output(j))
    assert np.array_equal(again, O.decode(data).pixels("u8", 4).reshape(again.shape))


@pytest.mark.gpu
def test_a_refused_request_is_not_decoded(jx):
    """add() with an offset below the default raises after the colour output has been set; the batch decodes all the same: no plane is written, nothing outside the colour
    output of the guarded destination is touched, the colour is the oracle's."""
    import torch
    data, _, _ = simple("modular", 2, 65, 41)
    size = 65 * 41 * 3
    t = torch.full((size + EXTRA,), FILL, dtype=torch.uint8, device="cuda:0")
    b = jx.BatchDecoder(0)
    with pytest.raises(jx.DecodeError, match="offset 8 is below the default"):
        b.add(data, dtype="uint8", num_channels=3, device_ptr=t.data_ptr() + FRONT, extra_planes=[1, 0], planes_offset=8)
    b.prepare(); b.decode(); b.finish()
    torch.cuda.synchronize()
    assert b.info_value("plane_outputs") == 0
    d = t.cpu().numpy()
    assert (d[:FRONT] == FILL).all() and (d[FRONT + size:] == FILL).all()
    assert np.array_equal(d[FRONT:FRONT + size], O.decode(data).pixels("u8", 3).reshape(-1))


def abi_frame_decodes(jx, stream, formats):
    """JxlDecoder* as a caller drives it, one extra-channel buffer per entry of `formats` (JxlDataType, endianness, numpy dtype) -> (planes, frame_decodes)"""
    L = jx.libjxl()
    fmt = jx.JxlPixelFormat(3, jx.JXL_TYPE_UINT8, jx.JXL_NATIVE_ENDIAN, 0)
    data = np.frombuffer(stream, np.uint8)
    dec = L.JxlDecoderCreate(None)
    try:
        assert L.JxlDecoderSubscribeEvents(dec, jx.JXL_DEC_BASIC_INFO | jx.JXL_DEC_FULL_IMAGE) == 0
        assert L.JxlDecoderSetInput(dec, data.ctypes.data, len(data)) == 0
        L.JxlDecoderCloseInput(dec)
        planes, px = [], None
        while True:
            st = L.JxlDecoderProcessInput(dec)
            if st == jx.JXL_DEC_NEED_IMAGE_OUT_BUFFER:
                size = C.c_size_t()
                assert L.JxlDecoderImageOutBufferSize(dec, C.byref(fmt), C.byref(size)) == 0
                px = np.zeros(size.value, np.uint8)
                assert L.JxlDecoderSetImageOutBuffer(dec, C.byref(fmt), px.ctypes.data, size.value) == 0
                for k, (jt, en, dt) in enumerate(formats):
                    ef = jx.JxlPixelFormat(1, jt, en, 0)
                    assert L.JxlDecoderExtraChannelBufferSize(dec, C.byref(ef), C.byref(size), k) == 0, jx.last_error()
                    planes.append(np.zeros(size.value // np.dtype(dt).itemsize, dt))
                    assert L.JxlDecoderSetExtraChannelBuffer(dec, C.byref(ef), planes[k].ctypes.data, size.value, k) == 0
            elif st == jx.JXL_DEC_FULL_IMAGE:
                return px, planes, int(L.JxlHipDecoderInfo(dec, b"frame_decodes"))
            elif st not in (jx.JXL_DEC_BASIC_INFO,):
                raise jx.DecodeError(jx.last_error())
    finally:
        L.JxlDecoderDestroy(dec)


@pytest.mark.gpu
def test_libjxl_api_serves_the_buffers_from_the_main_decode(jx):
    """The layered six-channel stream with all six buffers set, in differing sample types: one decode, every plane = numpy applied to the oracle twin's f32 alpha, the
    colour against the oracle.  A simple RGBA Modular image with its buffer set: two decodes, as before."""
    stream = M.layered("modular", 6)[0]
    fm = [(jx.JXL_TYPE_FLOAT, jx.JXL_LITTLE_ENDIAN, np.float32), (jx.JXL_TYPE_UINT8, jx.JXL_NATIVE_ENDIAN, np.uint8), (jx.JXL_TYPE_UINT16, jx.JXL_BIG_ENDIAN, np.uint16),
          (jx.JXL_TYPE_FLOAT16, jx.JXL_LITTLE_ENDIAN, np.uint16), (jx.JXL_TYPE_UINT16, jx.JXL_LITTLE_ENDIAN, np.uint16), (jx.JXL_TYPE_FLOAT, jx.JXL_LITTLE_ENDIAN, np.float32)]
    names = [("float32", "LE"), ("uint8", "LE"), ("uint16", "BE"), ("float16", "LE"), ("uint16", "LE"), ("float32", "LE")]
    px, planes, decodes = abi_frame_decodes(jx, stream, fm)
    assert decodes == 1
    M.assert_colour(px, stream, "u8")
    for e, (dtype, order) in enumerate(names):
        want = want_samples(M.oracle_plane(lambda k: M.layered("modular", 6, relabel=k)[0], e), dtype, order).reshape(-1)
        got = planes[e].view(want.dtype)
        assert np.array_equal(got, want), (e, dtype, order, int((got != want).sum()))
    rgba = S.encode_modular(np.dstack([S.synthetic_image(4, 64, 48), (np.arange(64 * 48) % 256).astype(np.uint8).reshape(48, 64)]).astype(np.int32))
    px, planes, decodes = abi_frame_decodes(jx, rgba, [(jx.JXL_TYPE_UINT8, jx.JXL_NATIVE_ENDIAN, np.uint8)])
    assert decodes == 2
    assert np.array_equal(planes[0], (np.arange(64 * 48) % 256).astype(np.uint8))
