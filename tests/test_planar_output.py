"""Planar (CHW) and affine output straight from the write stage (include/jxl_hip.h JxlHipOutputLayout; pixel_ops.h StorePixel / OutPixelPtr; the packed planar
stores of kernels.hip FusedGabEpf1OutKernel).

The interleaved output of every format is pinned against numpy by test_write_stage.py.  A planar output holds the same samples somewhere else, so its reference
here is the product's own interleaved decode of the same format, rearranged by numpy — exact, byte for byte, with every byte of the destination that is not a
sample (row padding, the gap between planes, guard regions in front of and behind the output) still holding the fill value.  An affine output is
fmaf(v, scale, bias) of the plain f32 sample v: within one float32 ULP of the float64 product-and-sum (twice-rounded against once-rounded), exact where the
arithmetic is (scale 1 / bias 0, power-of-two scales), and every other format of it derived exactly from the f32 affine decode.

Streams, shapes and the numpy write stage are test_write_stage.py's (200x136, 203x139, 67x41, 77x61, 520x72 = three groups).  One BatchDecoder holds the same
stream many times, once per format, so a whole format matrix costs one decode launch sequence."""
import numpy as np
import pytest

from conftest import fixture_bytes
import synth_lib as S
from test_write_stage import DTYPES, ORIENT, STREAMS, build_stream, convert_samples, padded_stride, padding_align
from test_downscaled_decode import plain_stream

FILL = 0xA5
FRONT, EXTRA = 256, 4096             # the output starts FRONT bytes into a destination that is EXTRA bytes larger than the output
BPS = {"uint8": 1, "uint16": 2, "float16": 2, "float32": 4}


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


_stream_cache = {}


def stream(name, orientation=1):
    key = (name, orientation)
    if key not in _stream_cache:
        _stream_cache[key] = build_stream(name, orientation)
    return _stream_cache[key]


# ---- one batch, many outputs --------------------------------------------------------------------------------------------------------------
def decode_specs(jx, data, specs, keep_orientation=False):
    """specs: dicts of BatchDecoder.add keywords (dtype, num_channels, endianness, align, downscale, planar, plane_stride, scale, bias) plus `shift` (extra bytes in
    front of the output, default 0).  Every spec is one more copy of `data` in ONE batch, decoded into a destination of its own: a device buffer of
    out_size + EXTRA bytes filled with FILL, the output FRONT + shift bytes into it.  -> list of (whole destination as uint8 array, out_size, (output width, height))"""
    import torch
    b = jx.BatchDecoder(0)
    b.set_option("keep_orientation", 1 if keep_orientation else 0)
    bufs, sizes = [], []
    for sp in specs:
        kw = {k: v for k, v in sp.items() if k != "shift"}
        assert not keep_orientation or not kw.get("align")                      # (image_out_size applies the orientation; without row padding the size is the same)
        size = jx.image_out_size(data, **kw)[1]
        t = torch.full((size + EXTRA,), FILL, dtype=torch.uint8, device="cuda:0")
        i = b.add(data, device_ptr=t.data_ptr() + FRONT + sp.get("shift", 0), **kw)
        assert b.out_size(i) == size, (sp, b.out_size(i), size)
        bufs.append(t); sizes.append(size)
    b.prepare(); b.decode(); b.finish()
    torch.cuda.synchronize()
    dims = []
    for i, sp in enumerate(specs):
        w, h = b.info(i).xsize, b.info(i).ysize
        dims.append(((w + 7) // 8, (h + 7) // 8) if sp.get("downscale", 1) == 8 else (w, h))
    return [(t.cpu().numpy(), n, d) for t, n, d in zip(bufs, sizes, dims)]


def samples_of_interleaved(dest, size, dims, sp):
    """(oh, ow, nch, bps) uint8: the sample bytes of an interleaved output; asserts the size formula and that nothing outside the output was written"""
    ow, oh = dims
    nch, bps, shift = sp["num_channels"], BPS[sp["dtype"]], sp.get("shift", 0)
    row = ow * nch * bps
    stride = padded_stride(row, sp.get("align", 0))
    assert size == stride * (oh - 1) + row, (sp, size)
    assert (dest[:FRONT + shift] == FILL).all() and (dest[FRONT + shift + size:] == FILL).all(), sp
    rows = np.full(stride * oh, FILL, np.uint8)
    rows[:size] = dest[FRONT + shift:FRONT + shift + size]
    rows = rows.reshape(oh, stride)
    assert (rows[:, row:] == FILL).all(), (sp, "row padding written")
    return rows[:, :row].reshape(oh, ow, nch, bps)


def expected_planar_dest(samples, sp, size):
    """The whole destination a planar decode must leave: samples (oh, ow, nch, bps) put plane by plane, FILL everywhere else"""
    oh, ow, nch, bps = samples.shape
    rs = padded_stride(ow * bps, sp.get("align", 0))
    ps = sp.get("plane_stride", 0) or rs * oh
    assert size == nch * ps, (sp, size, nch, ps)
    want = np.full(size + EXTRA, FILL, np.uint8)
    start = FRONT + sp.get("shift", 0)
    for c in range(nch):
        plane = np.full((oh, rs), FILL, np.uint8)
        plane[:, :ow * bps] = samples[:, :, c, :].reshape(oh, ow * bps)
        want[start + c * ps:start + c * ps + oh * rs] = plane.reshape(-1)
    return want


def assert_dest(got, want, tag):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError((tag, "%d differing bytes, first at byte %d of the destination: got %d want %d" % (len(bad), bad[0], got[bad[0]], want[bad[0]])))


def check_planar_against_interleaved(jx, data, formats, keep_orientation=False, what=""):
    """formats: dicts (dtype, num_channels, endianness, align[, downscale, scale, bias]) + optional planar-only keys (plane_stride, shift).  One batch decodes every
    format planar and — once per distinct format — interleaved; each planar destination must be its interleaved twin's samples plane by plane and FILL elsewhere."""
    inter, specs = {}, []
    for f in formats:
        key = repr(sorted((k, v) for k, v in f.items() if k not in ("plane_stride", "shift")))
        if key not in inter:
            inter[key] = len(specs)
            specs.append({k: v for k, v in f.items() if k not in ("plane_stride", "shift")})
    first_planar = len(specs)
    specs += [dict(f, planar=True) for f in formats]
    res = decode_specs(jx, data, specs, keep_orientation)
    for k, f in enumerate(formats):
        key = repr(sorted((k2, v) for k2, v in f.items() if k2 not in ("plane_stride", "shift")))
        di, ni, dims = res[inter[key]]
        dp, size_p, dims_p = res[first_planar + k]
        assert dims == dims_p
        samples = samples_of_interleaved(di, ni, dims, specs[inter[key]])
        assert_dest(dp, expected_planar_dest(samples, specs[first_planar + k], size_p), (what, f))


# ---- 1. sizes and refusals (no GPU) -----------------------------------------------------------------------------------------------------------
def test_sizes_and_refusals(jxh):
    """image_out_size(planar=True) = nch x oh x round_up(ow x bps, align) for every type, 1-4 channels, align 0 / 64, on a transposed image; a larger plane_stride gives
    nch x plane_stride; a plane_stride below the tight value or not a multiple of the sample size, and scale / bias with an integer type, are refused with a message;
    without a layout the sizes are the interleaved ones."""
    S.set_orientation(6)
    try:
        data = S.encode_vardct(S.synthetic_image(1, 203, 139), seed=4, strategy_mix=1, epf_iters=1, gab=1)
    finally:
        S.set_orientation()
    ow, oh = 139, 203
    for dtype in DTYPES:
        bps = BPS[dtype]
        for nch in (1, 2, 3, 4):
            for align in (0, 64):
                info, size = jxh.image_out_size(data, dtype, nch, align=align, planar=True)
                assert (info.xsize, info.ysize) == (ow, oh)
                rs = padded_stride(ow * bps, align)
                assert size == nch * oh * rs, (dtype, nch, align, size)
                assert jxh.image_out_size(data, dtype, nch, align=align, planar=True, plane_stride=oh * rs)[1] == size
                assert jxh.image_out_size(data, dtype, nch, align=align, planar=True, plane_stride=oh * rs + 52)[1] == nch * (oh * rs + 52)
                with pytest.raises(jxh.DecodeError, match="plane_stride"):
                    jxh.image_out_size(data, dtype, nch, align=align, planar=True, plane_stride=oh * rs - bps)
                if bps > 1:
                    with pytest.raises(jxh.DecodeError, match="multiple of the sample size"):
                        jxh.image_out_size(data, dtype, nch, align=align, planar=True, plane_stride=oh * rs + bps + 1)
                # no layout: today's size, through the old call and through the new one with a NULL layout
                row = ow * nch * bps
                want = padded_stride(row, align) * (oh - 1) + row
                assert jxh.image_out_size(data, dtype, nch, align=align)[1] == want
                import ctypes as C
                fmt = jxh.JxlPixelFormat(nch, jxh._PIXEL_TYPES[dtype][0], jxh.JXL_LITTLE_ENDIAN, align)
                n = C.c_size_t()
                buf = np.frombuffer(data, np.uint8)
                assert jxh.libjxl().JxlHipImageOutSizeLayout(buf.ctypes.data, len(data), C.byref(fmt), 1, None, None, C.byref(n)) == 0 and n.value == want
                # affine alone does not change the size
                if dtype in ("float16", "float32"):
                    assert jxh.image_out_size(data, dtype, nch, align=align, scale=[2, 3, 4, 5], bias=[1])[1] == want
    for dtype in ("uint8", "uint16"):
        for planar in (False, True):
            with pytest.raises(jxh.DecodeError, match="affine output needs a float sample type"):
                jxh.image_out_size(data, dtype, 3, planar=planar, scale=[0.5, 0.5, 0.5])
    with pytest.raises(ValueError):
        jxh.image_out_size(data, "uint8", 3, plane_stride=1 << 20)               # (a plane stride without planes)
    # 1:8: the small picture's planes
    assert jxh.image_out_size(data, "float16", 3, planar=True, downscale=8)[1] == 3 * 26 * 18 * 2


# ---- 2. planar == de-interleaved, through every write path ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STREAMS))
def test_planar_is_the_interleaved_output_rearranged(jx, name):
    """{u8, u16, f16, f32} x channel counts x both byte orders x {align 0, one that pads} x {tight planes, tight + 52 bytes}: the planar decode is the interleaved decode of
    the same format plane by plane, and no byte of the destination outside the samples is touched."""
    data, grey, unpremul = stream(name)
    w, h = jx.image_out_size(data)[0].xsize, jx.image_out_size(data)[0].ysize
    formats = []
    for dtype in DTYPES:
        for nch in (1, 2, 3, 4):
            for align in (0, padding_align(w * BPS[dtype])):
                assert padded_stride(w * BPS[dtype], align) > w * BPS[dtype] or align == 0
                for big in (False, True):
                    base = dict(dtype=dtype, num_channels=nch, endianness=jx.JXL_BIG_ENDIAN if big else jx.JXL_LITTLE_ENDIAN, align=align)
                    tight = h * padded_stride(w * BPS[dtype], align)
                    formats.append(base)
                    formats.append(dict(base, plane_stride=tight + 52))
    check_planar_against_interleaved(jx, data, formats, what=name)


# ---- 3. the packed planar stores of the fused kernel and their fall-backs --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fused_rgb_w4", "fused_rgba_w4", "fused_rgb_three_groups", "fused_rgb_odd", "fused_rgba_odd"])
def test_packed_planar_stores_and_their_fallbacks(jx, name):
    """u8, 3 and 4 channels of the fused streams: under the conditions of the dword form (width % 4 == 0, destination, rows and planes 4-byte aligned, stored orientation)
    and under each single condition that rules it out — destination shifted by one byte, rows = 2 mod 4 apart, planes = 2 mod 4 apart, orientation 2, odd width —
    the same bytes, and the guard bytes intact."""
    data, _, _ = stream(name)
    info = jx.image_out_size(data)[0]
    w, h = info.xsize, info.ysize
    up4 = lambda n: (n + 3) // 4 * 4
    # align = 2 leaves these widths' rows where they are; a row pitch = 2 mod 4 of a width that is a multiple of 4 takes an align that is itself = 2 mod 4
    a2 = next(a for a in (202, 206, 522, 526, 70, 74) if a > w and a % 4 == 2)
    assert padded_stride(w, a2) % 4 == 2
    formats = []
    for nch in (3, 4):
        base = dict(dtype="uint8", num_channels=nch, endianness=jx.JXL_LITTLE_ENDIAN, align=0)
        formats += [base, dict(base, align=64), dict(base, plane_stride=up4(w * h) + 52),        # the dword form (where the width allows it)
                    dict(base, shift=1), dict(base, shift=2), dict(base, shift=3),                 # destination not 4-byte aligned
                    dict(base, align=2), dict(base, align=a2),                                     # rows = 2 mod 4 apart
                    dict(base, plane_stride=up4(w * h) + 2),                                       # planes = 2 mod 4 apart
                    dict(base, plane_stride=up4(w * h) + 1), dict(base, plane_stride=up4(w * h) + 3)]
    check_planar_against_interleaved(jx, data, formats, what=name)
    if name in ("fused_rgb_w4", "fused_rgba_w4"):
        data2, _, _ = stream(name, 2)
        check_planar_against_interleaved(jx, data2, [dict(dtype="uint8", num_channels=n, endianness=jx.JXL_LITTLE_ENDIAN, align=0) for n in (3, 4)], what=name + " orientation 2")
        # (and that this is the mirrored picture, not the stored one)
        (d1, n1, dims), = decode_specs(jx, data, [dict(dtype="uint8", num_channels=3, planar=True)])
        (d2, n2, _), = decode_specs(jx, data2, [dict(dtype="uint8", num_channels=3, planar=True)])
        p1 = d1[FRONT:FRONT + n1].reshape(3, h, w); p2 = d2[FRONT:FRONT + n2].reshape(3, h, w)
        assert np.array_equal(p2, p1[:, :, ::-1]) and not np.array_equal(p2, p1)


# ---- 4. orientation -------------------------------------------------------------------------------------------------------------------------
def stored_f32(jx, data):
    (d, n, (w, h)), = decode_specs(jx, data, [dict(dtype="float32", num_channels=4, endianness=jx.JXL_LITTLE_ENDIAN)], keep_orientation=True)
    assert n == w * h * 16
    return d[FRONT:FRONT + n].view("<f4").reshape(h, w, 4).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(n for n in STREAMS if n != "sample_grey"))
def test_orientation_per_plane(jx, name):
    """Orientations 6 and 7 (all of 2..8 on fused_rgb_w4 and modular_layers): planar u16 big endian and f16 at 3 and 4 channels; every plane is the numpy re-orientation
    (ORIENT of test_write_stage.py) of that channel of the stored-orientation f32 decode, converted by numpy."""
    every = name in ("fused_rgb_w4", "modular_layers")
    for o in (range(2, 9) if every else (6, 7)):
        data, grey, _ = stream(name, o)
        base = stored_f32(jx, data)
        assert base.shape[0] != base.shape[1]
        specs = [dict(dtype=dt, num_channels=nch, endianness=jx.JXL_BIG_ENDIAN if big else jx.JXL_LITTLE_ENDIAN, planar=True) for dt, big in (("uint16", True), ("float16", False)) for nch in (3, 4)]
        for sp, (d, n, (ow, oh)) in zip(specs, decode_specs(jx, data, specs)):
            nch = sp["num_channels"]
            assert (oh, ow) == ORIENT[o](base[..., 0]).shape and n == nch * ow * oh * 2
            got = d[FRONT:FRONT + n].view(">u2" if sp["endianness"] == jx.JXL_BIG_ENDIAN else "<u2").reshape(nch, oh, ow)
            for c in range(nch):
                want = convert_samples(np.ascontiguousarray(ORIENT[o](base[..., c])), sp["dtype"])
                assert np.array_equal(got[c], want), (name, o, sp, c, int((got[c] != want).sum()))
            assert (d[:FRONT] == FILL).all() and (d[FRONT + n:] == FILL).all()


# ---- 5. affine ----------------------------------------------------------------------------------------------------------------------------
SCALE = [1.0 / 0.229, 1.0, 3.7, -0.5]
BIAS = [-0.485 / 0.229, 0.0, 0.125, 1.0]          # slot 1 is left at (1, 0)
AFFINE_STREAMS = ("fused_rgba_w4", "modular_rgba8", "vardct_layers")


def ulp_distance(a, b):
    ai = a.view(np.int32).astype(np.int64); bi = b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7FFFFFFF), ai); bi = np.where(bi < 0, -(bi & 0x7FFFFFFF), bi)
    return np.abs(ai - bi)


def f32_of(res, nch):
    d, n, (w, h) = res
    assert n == w * h * nch * 4
    return d[FRONT:FRONT + n].view("<f4").reshape(h, w, nch).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", AFFINE_STREAMS)
def test_affine_f32_is_one_fused_multiply_add(jx, name):
    """(a) f32 interleaved with scale / bias: within 1 ULP of float32(float64(v) x scale + bias), v the plain f32 decode — the most a product-then-sum rounded twice
    (the float64 expression: the product of a float32 and a float32 is exact there, the sum rounds once, the cast once more) can differ from one fused rounding; the
    (1, 0) slot is exact; power-of-two scales without bias are exact."""
    data, _, _ = stream(name)
    f = dict(dtype="float32", num_channels=4, endianness=jx.JXL_LITTLE_ENDIAN)
    pow2 = [2.0, 0.25, -8.0, 1.0]
    res = decode_specs(jx, data, [f, dict(f, scale=SCALE, bias=BIAS), dict(f, scale=pow2), dict(f, scale=SCALE[:3], bias=BIAS[:3], num_channels=3)])
    v, aff, p2, aff3 = f32_of(res[0], 4), f32_of(res[1], 4), f32_of(res[2], 4), f32_of(res[3], 3)
    assert np.isfinite(v).all() and v[..., :3].std() > 0.01
    for c in range(4):
        want = (v[..., c].astype(np.float64) * np.float64(np.float32(SCALE[c])) + np.float64(np.float32(BIAS[c]))).astype(np.float32)
        d = ulp_distance(aff[..., c], want)
        print(name, "slot", c, "max ULP distance", int(d.max()), "samples off by one", int((d == 1).sum()))
        assert d.max() <= 1, (name, c, int(d.max()))
        assert np.array_equal(p2[..., c], v[..., c] * np.float32(pow2[c])), (name, c)         # (values: x * s + 0 turns a -0 product into +0)
    assert np.array_equal(aff[..., 1], v[..., 1])
    assert not np.array_equal(aff[..., 0], v[..., 0]) and not np.array_equal(aff[..., 3], v[..., 3])
    assert np.array_equal(aff3.view(np.uint32), aff[..., :3].view(np.uint32))        # (the slots are the output's, whatever the channel count)


@pytest.mark.gpu
@pytest.mark.parametrize("name", AFFINE_STREAMS)
def test_affine_formats_follow_from_the_f32_affine_decode(jx, name):
    """(b) f16, both byte orders, planar, padded and oriented affine outputs = numpy applied to the product's own f32 affine decode with the same parameters, exact
    (NaN-free streams)."""
    for o in (1, 6):
        data, _, _ = stream(name, o)
        f = dict(dtype="float32", num_channels=4, endianness=jx.JXL_LITTLE_ENDIAN, scale=SCALE, bias=BIAS)
        (r,) = decode_specs(jx, data, [f])
        base = f32_of(r, 4)                                                        # oriented, affine
        oh, ow = base.shape[:2]
        specs = []
        for dtype in ("float16", "float32"):
            for big in (False, True):
                for nch in (3, 4):
                    for planar in (False, True):
                        for align in (0, padding_align(ow * BPS[dtype] * (1 if planar else nch))):
                            specs.append(dict(dtype=dtype, num_channels=nch, endianness=jx.JXL_BIG_ENDIAN if big else jx.JXL_LITTLE_ENDIAN, align=align, planar=planar,
                                              scale=SCALE[:nch], bias=BIAS[:nch]))
        for sp, (d, n, dims) in zip(specs, decode_specs(jx, data, specs)):
            assert dims == (ow, oh)
            nch, bps = sp["num_channels"], BPS[sp["dtype"]]
            q = convert_samples(base[..., :nch], sp["dtype"])
            if sp["endianness"] == jx.JXL_BIG_ENDIAN:
                q = q.byteswap()
            samples = np.ascontiguousarray(q).view(np.uint8).reshape(oh, ow, nch, bps)
            if sp["planar"]:
                want = expected_planar_dest(samples, sp, n)
            else:
                row = ow * nch * bps
                stride = padded_stride(row, sp["align"])
                assert n == stride * (oh - 1) + row
                rows = np.full((oh, stride), FILL, np.uint8)
                rows[:, :row] = samples.reshape(oh, row)
                want = np.full(n + EXTRA, FILL, np.uint8)
                want[FRONT:FRONT + n] = rows.reshape(-1)[:n]
            assert_dest(d, want, (name, o, sp))


@pytest.mark.gpu
def test_affine_does_not_outlive_its_output(jx):
    """(c) the same BatchDecoder, reset, decodes without scale / bias what a fresh one decodes."""
    data, _, _ = stream("fused_rgba_w4")
    b = jx.BatchDecoder(0)
    outs = []
    for kw in (dict(scale=SCALE, bias=BIAS, planar=True), dict()):
        b.reset()
        b.add(data, "float32", 4, **kw)
        b.prepare(); b.decode(); b.finish()
        outs.append(b.output(0).copy())
    fresh = jx.BatchDecoder(0)
    fresh.add(data, "float32", 4)
    fresh.prepare(); fresh.decode(); fresh.finish()
    assert np.array_equal(outs[1].view(np.uint32), fresh.output(0).view(np.uint32))
    assert not np.array_equal(outs[0], outs[1])


# ---- 6. 1:8 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_downscaled_planar(jx):
    """planar f16 with scale / bias and planar u8 of the 1030x520 plain stream at 1:8 = the interleaved 1:8 decode of the same format, plane by plane."""
    data = plain_stream(1030, 520)
    f16 = dict(dtype="float16", num_channels=3, endianness=jx.JXL_LITTLE_ENDIAN, align=0, downscale=8, scale=SCALE[:3], bias=BIAS[:3])
    u8 = dict(dtype="uint8", num_channels=3, endianness=jx.JXL_LITTLE_ENDIAN, align=0, downscale=8)
    check_planar_against_interleaved(jx, data, [f16, u8, dict(u8, num_channels=4, align=64, plane_stride=65 * 192 + 52)], what="1:8")
    (d, n, dims), = decode_specs(jx, data, [dict(u8, planar=True)])
    assert dims == (129, 65) and n == 3 * 129 * 65 and d[FRONT:FRONT + n].std() > 1


# ---- 7. pipeline ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pipeline_planar_affine_jobs(jx):
    """A job of a fused VarDCT frame, a Modular RGBA image and sample.jxl as planar f16 with scale / bias, to device and to pinned host destinations of exactly the
    required capacity: each result is the BatchDecoder's for the same image and layout.  A capacity one byte short fails that image alone; an interleaved job behind a
    planar one through the same pipeline is the batch's interleaved result."""
    import torch
    datas = [stream("fused_rgb_w4")[0], stream("modular_rgba8")[0], fixture_bytes("sample.jxl")]
    lay = dict(planar=True, scale=SCALE, bias=BIAS)

    def batch(data, **kw):
        (d, n, _), = decode_specs(jx, data, [dict(dtype=kw.pop("dtype"), num_channels=4, endianness=jx.JXL_LITTLE_ENDIAN, **kw)])
        return d[FRONT:FRONT + n].copy()
    refs = [batch(d, dtype="float16", **lay) for d in datas]
    refs_u8 = [batch(d, dtype="uint8") for d in datas]
    sizes = [jx.image_out_size(d, "float16", 4, **lay)[1] for d in datas]
    assert sizes == [r.size for r in refs]
    p = jx.Pipeline(0, jobs_in_flight=2, lf_streams=2, prepare_threads=1, parse_threads=2, reserve_frames=4, reserve_width=1024, reserve_height=640)
    try:
        outs = [torch.full((s,), FILL, dtype=torch.uint8, device="cuda:0") for s in sizes]
        st, _ = p.wait(p.submit(datas, "float16", 4, device_ptrs=[o.data_ptr() for o in outs], capacities=sizes, **lay))
        torch.cuda.synchronize()
        assert st == [0, 0, 0]
        for o, r in zip(outs, refs):
            assert np.array_equal(o.cpu().numpy(), r)
        pinned = [jx.PinnedBuffer(s) for s in sizes]
        st, _ = p.wait(p.submit(datas, "float16", 4, host_ptrs=[o.ptr for o in pinned], capacities=sizes, **lay))
        assert st == [0, 0, 0]
        for o, r in zip(pinned, refs):
            assert np.array_equal(o.array, r)
        # one byte short: that image alone
        pinned = [jx.PinnedBuffer(s) for s in sizes]
        caps = [sizes[0], sizes[1] - 1, sizes[2]]
        st, _ = p.wait(p.submit(datas, "float16", 4, host_ptrs=[o.ptr for o in pinned], capacities=caps, **lay), check=False)
        assert st == [0, 1, 0] and "too small" in jx.last_error()
        assert np.array_equal(pinned[0].array, refs[0]) and np.array_equal(pinned[2].array, refs[2])
        # a plane stride the second image does not fit: that image alone
        ps = sizes[0] // 4
        assert sizes[1] > sizes[0]
        big = [jx.PinnedBuffer(4 * max(sizes)) for _ in datas]
        st, _ = p.wait(p.submit(datas, "float16", 4, host_ptrs=[o.ptr for o in big], plane_stride=ps, **lay), check=False)
        assert st[0] == 0 and st[1] == 1 and "plane_stride" in jx.last_error()
        assert np.array_equal(big[0].array[:sizes[0]], refs[0])
        # planar job, then interleaved job: nothing of the layout stays behind in the slots or the shared planes
        pl = [jx.PinnedBuffer(s) for s in sizes]
        il = [jx.PinnedBuffer(r.size) for r in refs_u8]
        t1 = p.submit(datas, "float16", 4, host_ptrs=[o.ptr for o in pl], capacities=sizes, **lay)
        t2 = p.submit(datas, "uint8", 4, host_ptrs=[o.ptr for o in il], capacities=[r.size for r in refs_u8])
        t3 = p.submit(datas, "float16", 4, host_ptrs=[o.ptr for o in pinned], capacities=sizes, **lay)
        assert p.wait(t1)[0] == [0, 0, 0] and p.wait(t2)[0] == [0, 0, 0] and p.wait(t3)[0] == [0, 0, 0]
        for o, r in zip(pl + il + pinned, refs + refs_u8 + refs):
            assert np.array_equal(o.array, r)
        # integer samples with scale / bias: the submission is refused
        with pytest.raises(jx.DecodeError, match="affine output needs a float sample type"):
            p.submit(datas, "uint8", 4, host_ptrs=[o.ptr for o in il], scale=[2.0])
    finally:
        p.close()
