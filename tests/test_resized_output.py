"""Output of a requested size: antialiased resize, and crop, at the write stage (include/jxl_hip.h JxlHipOutputResize; decoder.cc ResizeAxis;
kernels_features.hip ResizeKernel).

The filter is defined by a formula (jxl_hip.h): separable, per channel slot, the triangle filter with half-pixel centres widened by the ratio where it shrinks,
the tap range cut at the edges and renormalised.  `restate` below is that formula in float64 numpy; test_restatement_equals_torch_float64 pins it against torch's
float64 interpolate(mode="bilinear", antialias=True) without a device.  Every GPU comparison then has the product's own plain f32 decode as its input: the resized
f32 output against restate() of it within a bound derived from the number of roundings, every other format and layout byte for byte against numpy applied to the
f32 resized decode of the same parameters — with every byte of the destination that is no sample still holding the fill value.

The bound.  The host builds each normalised weight in double and rounds it to f32 once (relative error 2^-24); the kernel accumulates w0 x v0, then one fmaf per
further tap, in f32: per axis one rounding per tap plus the one on the weight, which stays inside the `taps + 4` the bound allows per axis:
(taps_x + taps_y + 8) x 2^-24 x max|v|, taps the longest tap range hi - lo of the axis (normalised non-negative weights: no partial sum exceeds max|v|).

Streams, shapes and the numpy write stage are test_write_stage.py's, the destinations with guard bytes test_planar_output.py's.  One BatchDecoder holds the same
stream many times, once per output, so each test is one launch sequence."""
import ctypes as C

import numpy as np
import pytest

from conftest import fixture_bytes
import synth_lib as S
from test_write_stage import DTYPES, ORIENT, convert_samples, padded_stride, padding_align
from test_downscaled_decode import plain_stream
from test_planar_output import BIAS, BPS, EXTRA, FILL, FRONT, SCALE, assert_dest, expected_planar_dest, stream

PAIRS = [((203, 139), (48, 32)), ((203, 131), (224, 224)), ((1030, 520), (224, 224)), ((520, 72), (300, 7)), ((67, 41), (67, 41)), ((2056, 24), (9, 5)), ((9, 9), (1, 1))]


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


# ---- the defining formula ------------------------------------------------------------------------------------------------------------------
def axis_taps(n_in, n_out):
    """per output index: (lo, hi, normalised float64 weights of the samples lo .. hi - 1)"""
    scale = n_in / n_out
    support = max(scale, 1.0)
    taps = []
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo = max(0, int(c - support + 0.5))
        hi = min(n_in, int(c + support + 0.5))
        w = np.maximum(0.0, 1.0 - np.abs((np.arange(lo, hi) - c + 0.5) / support))
        taps.append((lo, hi, w / w.sum()))
    return taps


def restate(x, ow, oh):
    """(h, w, c) array -> ((oh, ow, c) float64, longest tap range across, longest down): horizontal pass, then vertical"""
    x = np.asarray(x, np.float64)
    tx, ty = axis_taps(x.shape[1], ow), axis_taps(x.shape[0], oh)
    tmp = np.stack([np.tensordot(w, x[:, lo:hi], axes=(0, 1)) for lo, hi, w in tx], axis=1)
    out = np.stack([np.tensordot(w, tmp[lo:hi], axes=(0, 0)) for lo, hi, w in ty], axis=0)
    return out, max(hi - lo for lo, hi, _ in tx), max(hi - lo for lo, hi, _ in ty)


def test_restatement_equals_torch_float64(jxh):
    """restate() = torch.nn.functional.interpolate(x.double(), size, mode="bilinear", antialias=True) on the CPU to 1e-12, on random arrays of seven source / target
    pairs (shrinking, enlarging, both at once, the same size, a 457-tap axis, everything into one pixel) — the filter include/jxl_hip.h promises for JxlHipOutputResize."""
    import torch
    assert [n for n, _ in jxh.JxlHipOutputResize._fields_] == ["xsize", "ysize", "crop_x0", "crop_y0", "crop_xsize", "crop_ysize"] and C.sizeof(jxh.JxlHipOutputResize) == 24
    rng = np.random.default_rng(7)
    assert max(hi - lo for lo, hi, _ in axis_taps(2056, 9)) == 457
    assert all(hi - lo == 2 and w[0] == 1.0 and w[1] == 0.0 for lo, hi, w in axis_taps(67, 67)[:-1])        # (the same size: weights exactly (1, 0))
    for (w, h), (ow, oh) in PAIRS:
        x = rng.standard_normal((h, w, 3))
        want = torch.nn.functional.interpolate(torch.from_numpy(x).permute(2, 0, 1)[None].double(), size=(oh, ow), mode="bilinear", antialias=True, align_corners=False)
        got = restate(x, ow, oh)[0]
        err = np.abs(got - want[0].permute(1, 2, 0).numpy()).max()
        print((w, h), "->", (ow, oh), "max difference", err)
        assert err <= 1e-12, ((w, h), (ow, oh), err)


# ---- sizes and refusals (no GPU) -------------------------------------------------------------------------------------------------------------
def test_sizes_and_refusals(jxh):
    """image_out_size(resize=(ow, oh)) is the size formula of an ow x oh picture for every type, 1-4 channels, align 0 / 64, interleaved, tight planes and a padded
    plane stride — whatever the size of the source (two sizes, one of them transposed by its orientation); a target side of 0 or above 65535, an empty crop, a crop
    that leaves the picture and a crop without a target are refused with a message; a NULL resize is the ...Layout call."""
    S.set_orientation(6)
    try:
        turned = S.encode_vardct(S.synthetic_image(1, 203, 139), seed=4, strategy_mix=1, epf_iters=1, gab=1)
    finally:
        S.set_orientation()
    small = stream("fused_rgba_odd")[0]                       # 67 x 41
    ow, oh = 48, 33
    for data in (turned, small):
        for dtype in DTYPES:
            bps = BPS[dtype]
            for nch in (1, 2, 3, 4):
                for align in (0, 64):
                    row = ow * nch * bps
                    info, size = jxh.image_out_size(data, dtype, nch, align=align, resize=(ow, oh))
                    assert size == padded_stride(row, align) * (oh - 1) + row, (dtype, nch, align, size)
                    assert (info.xsize, info.ysize) in ((139, 203), (67, 41))               # (the info stays the image's)
                    rs = padded_stride(ow * bps, align)
                    assert jxh.image_out_size(data, dtype, nch, align=align, planar=True, resize=(ow, oh))[1] == nch * oh * rs
                    assert jxh.image_out_size(data, dtype, nch, align=align, planar=True, plane_stride=oh * rs + 52 * bps, resize=(ow, oh))[1] == nch * (oh * rs + 52 * bps)
                    with pytest.raises(jxh.DecodeError, match="plane_stride"):              # (the plane of the TARGET must fit, not the source's)
                        jxh.image_out_size(data, dtype, nch, align=align, planar=True, plane_stride=oh * rs - bps, resize=(ow, oh))
                    # a crop and a downscale change nothing about the size
                    assert jxh.image_out_size(data, dtype, nch, align=align, resize=(ow, oh), crop=(3, 2, 20, 30))[1] == size
                    # NULL resize: the ...Layout size of the image itself
                    fmt = jxh.JxlPixelFormat(nch, jxh._PIXEL_TYPES[dtype][0], jxh.JXL_LITTLE_ENDIAN, align)
                    n, m = C.c_size_t(), C.c_size_t()
                    buf = np.frombuffer(data, np.uint8)
                    L = jxh.libjxl()
                    assert L.JxlHipImageOutSizeResized(buf.ctypes.data, len(data), C.byref(fmt), 1, None, None, None, C.byref(n)) == 0
                    assert L.JxlHipImageOutSizeLayout(buf.ctypes.data, len(data), C.byref(fmt), 1, None, None, C.byref(m)) == 0 and n.value == m.value
                    assert n.value == jxh.image_out_size(data, dtype, nch, align=align)[1] != size
    assert jxh.image_out_size(turned, "float16", 3, planar=True, downscale=8, resize=(ow, oh))[1] == 3 * ow * oh * 2
    for bad in ((0, 5), (5, 0), (0, 0)):
        with pytest.raises(jxh.DecodeError, match="a target side of 0"):
            jxh.image_out_size(turned, "uint8", 3, resize=bad)
    for bad in ((65536, 5), (5, 70000)):
        with pytest.raises(jxh.DecodeError, match="a target side above 65535"):
            jxh.image_out_size(turned, "uint8", 3, resize=bad)
    assert jxh.image_out_size(turned, "uint8", 1, resize=(65535, 1))[1] == 65535
    # the picture is 139 x 203 (orientation 6); at 1:8 it is 18 x 26
    for crop in ((0, 0, 140, 10), (139, 0, 1, 1), (0, 203, 1, 1), (130, 0, 10, 10), (0, 200, 5, 4), (0, 0, 203, 139), (2 ** 32 - 1, 0, 2, 2)):
        with pytest.raises(jxh.DecodeError, match="leaves the 139 x 203 picture"):
            jxh.image_out_size(turned, "uint8", 3, resize=(5, 5), crop=crop)
    with pytest.raises(jxh.DecodeError, match="leaves the 18 x 26 picture"):
        jxh.image_out_size(turned, "uint8", 3, resize=(5, 5), crop=(0, 0, 19, 26), downscale=8)
    for crop in ((3, 3, 0, 0), (0, 0, 5, 0), (0, 0, 0, 5)):
        with pytest.raises(jxh.DecodeError, match="the crop is empty"):
            jxh.image_out_size(turned, "uint8", 3, resize=(5, 5), crop=crop)
    for crop in ((0, 0, 139, 203), (138, 202, 1, 1), (0, 0, 0, 0)):                           # (all zero: the whole picture)
        assert jxh.image_out_size(turned, "uint8", 3, resize=(5, 5), crop=crop)[1] == 75
    with pytest.raises(ValueError):
        jxh.image_out_size(turned, "uint8", 3, crop=(0, 0, 5, 5))                           # (a crop without a target)
    # ... and through the C call itself
    st = C.c_size_t()
    rs = jxh.JxlHipOutputResize(0, 4, 0, 0, 0, 0)
    fmt = jxh.JxlPixelFormat(3, jxh._PIXEL_TYPES["uint8"][0], jxh.JXL_LITTLE_ENDIAN, 0)
    buf = np.frombuffer(turned, np.uint8)
    assert jxh.libjxl().JxlHipImageOutSizeResized(buf.ctypes.data, len(turned), C.byref(fmt), 1, None, C.byref(rs), None, C.byref(st)) != 0
    assert "a target side of 0" in jxh.last_error()


# ---- one batch, many outputs -----------------------------------------------------------------------------------------------------------------
def decode_specs(jx, data, specs, keep_orientation=False):
    """specs: dicts of BatchDecoder.add keywords (dtype, num_channels, endianness, align, downscale, planar, plane_stride, scale, bias, resize, crop).  Every spec is one
    more copy of `data` in ONE batch, decoded into a device buffer of out_size + EXTRA bytes filled with FILL, the output FRONT bytes into it.
    -> list of (whole destination as uint8 array, out_size, (output width, height))"""
    import torch
    b = jx.BatchDecoder(0)
    b.set_option("keep_orientation", 1 if keep_orientation else 0)
    bufs, sizes = [], []
    for sp in specs:
        assert not keep_orientation or not sp.get("align") or sp.get("resize")              # (image_out_size applies the orientation; a target size does not depend on it)
        size = jx.image_out_size(data, **sp)[1]
        t = torch.full((size + EXTRA,), FILL, dtype=torch.uint8, device="cuda:0")
        i = b.add(data, device_ptr=t.data_ptr() + FRONT, **sp)
        assert b.out_size(i) == size, (sp, b.out_size(i), size)
        bufs.append(t); sizes.append(size)
    b.prepare(); b.decode(); b.finish()
    torch.cuda.synchronize()
    dims = []
    for i, sp in enumerate(specs):
        w, h = b.info(i).xsize, b.info(i).ysize
        dims.append(tuple(sp["resize"]) if sp.get("resize") else ((w + 7) // 8, (h + 7) // 8) if sp.get("downscale", 1) == 8 else (w, h))
    return [(t.cpu().numpy(), n, d) for t, n, d in zip(bufs, sizes, dims)]


def f32_of(res, nch):
    d, n, (w, h) = res
    assert n == w * h * nch * 4, (n, w, h, nch)
    assert (d[:FRONT] == FILL).all() and (d[FRONT + n:] == FILL).all()
    return d[FRONT:FRONT + n].view("<f4").reshape(h, w, nch).copy()


def F32(jx, nch, **kw):
    return dict(dtype="float32", num_channels=nch, endianness=jx.JXL_LITTLE_ENDIAN, **kw)


def assert_within_bound(got, plain, ow, oh, tag):
    want, tx, ty = restate(plain, ow, oh)
    bound = (tx + ty + 8) * 2.0 ** -24 * float(np.abs(plain).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(tag, "taps", (tx, ty), "max error", err, "bound", bound)
    assert got.shape == want.shape and np.isfinite(got).all()
    assert err <= bound, (tag, err, bound)
    return tx, ty


# ---- 1. the f32 output against the formula -------------------------------------------------------------------------------------------------
def _stream_of(name):
    if name == "plain_2056x24":
        return plain_stream(2056, 24), False
    data, grey, _ = stream(name)
    return data, grey


F32_CASES = {
    "fused_rgb_odd": [(3, (48, 32)), (3, (224, 224)), (4, (48, 32))],                  # 203 x 139: odd sides, 9 taps; enlarging, 2 taps, the edges renormalised
    "modular_rgba8": [(4, (48, 32)), (4, (224, 224)), (3, (48, 32))],                  # 203 x 139 with a real alpha channel, through ModularOutputKernel
    "fused_rgb_three_groups": [(3, (300, 7)), (4, (300, 7))],                           # 520 x 72
    "plain_2056x24": [(3, (9, 5)), (4, (9, 5))],                                        # 457 taps across
    "fused_rgba_odd": [(4, (1, 1)), (3, (1, 1))],                                       # 67 x 41 into one pixel
    "fused_rgb_w4": [(3, (33, 17)), (4, (33, 17))],                                     # 200 x 136: the last block of threads is partly outside, both ways
    "modular_grey8": [(1, (33, 17)), (2, (48, 32)), (1, (100, 150))],                   # 77 x 139, grey
    "vardct_layers": [(4, (48, 32))],                                                   # the frame tail's WriteKernel
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(F32_CASES))
def test_f32_against_the_defining_formula(jx, name):
    """The f32 resized output of a stream against restate() of the product's own plain f32 decode of the same stream and channel count, within
    (taps_x + taps_y + 8) x 2^-24 x max|v| (module docstring)."""
    data, _ = _stream_of(name)
    cases = F32_CASES[name]
    chans = sorted({nch for nch, _ in cases})
    specs = [F32(jx, nch) for nch in chans] + [F32(jx, nch, resize=size) for nch, size in cases]
    res = decode_specs(jx, data, specs)
    plain = {nch: f32_of(res[k], nch) for k, nch in enumerate(chans)}
    taps = set()
    for (nch, (ow, oh)), r in zip(cases, res[len(chans):]):
        assert plain[nch][..., 0].std() > 0.01
        taps.add(assert_within_bound(f32_of(r, nch), plain[nch], ow, oh, (name, nch, (ow, oh))))
    if name == "plain_2056x24":
        assert {tx for tx, _ in taps} == {457}
    if name == "fused_rgb_odd":
        assert (9, 9) in taps and (2, 2) in taps


# ---- 2. the same size ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fused_rgb_odd", "modular_rgba8", "fused_rgba_odd"])
def test_same_size_is_the_plain_decode(jx, name):
    """target = the picture's own size: one tap of weight 1 per axis, the output is the decode without a resize byte for byte — u8 and f32, interleaved and planar,
    and under orientation 6."""
    for o in (1, 6):
        data = stream(name, o)[0]
        info = jx.image_out_size(data)[0]
        size = (info.xsize, info.ysize)
        base = [dict(dtype="uint8", num_channels=4, align=64), F32(jx, 4), F32(jx, 3, planar=True), dict(dtype="uint8", num_channels=3)]
        res = decode_specs(jx, data, base + [dict(sp, resize=size) for sp in base])
        for k, sp in enumerate(base):
            assert res[k][1] == res[len(base) + k][1]
            assert_dest(res[len(base) + k][0], res[k][0], (name, o, sp))
        assert res[0][0][FRONT:FRONT + res[0][1]].std() > 1


# ---- 3. crop --------------------------------------------------------------------------------------------------------------------------------------
CROPS = [((0, 0, 100, 50), (48, 32)), ((103, 89, 100, 50), (48, 32)), ((0, 40, 203, 30), (48, 32)), ((50, 0, 20, 139), (48, 32)), ((77, 33, 1, 1), (3, 2)),
         ((10, 20, 31, 17), (64, 40)), ((0, 0, 203, 139), (48, 32))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,nch", [("fused_rgb_odd", 3), ("modular_rgba8", 4)])
def test_crop_is_crop_then_resize(jx, name, nch):
    """Crops of the 203 x 139 picture that touch each edge, a one-pixel crop, an enlarged crop and the whole picture: the output is restate() of the cropped plain f32
    decode, same bound; the whole-picture crop and no crop give the same bytes.  Under orientation 6 the rectangle is one of the oriented picture."""
    data = stream(name)[0]
    specs = [F32(jx, nch)] + [F32(jx, nch, resize=size, crop=crop) for crop, size in CROPS] + [F32(jx, nch, resize=(48, 32))]
    res = decode_specs(jx, data, specs)
    plain = f32_of(res[0], nch)
    assert plain.shape == (139, 203, nch)
    for ((x0, y0, w, h), (ow, oh)), r in zip(CROPS, res[1:]):
        assert_within_bound(f32_of(r, nch), plain[y0:y0 + h, x0:x0 + w], ow, oh, (name, (x0, y0, w, h)))
    assert_dest(res[len(CROPS)][0], res[len(CROPS) + 1][0], (name, "whole-picture crop"))
    one = f32_of(res[5], nch)
    assert np.array_equal(one, np.broadcast_to(plain[33, 77], one.shape))                    # (one source pixel: every weight is 1)
    data6 = stream(name, 6)[0]
    crop = (9, 100, 120, 90)
    res = decode_specs(jx, data6, [F32(jx, nch), F32(jx, nch, resize=(40, 30), crop=crop)])
    plain = f32_of(res[0], nch)
    assert plain.shape == (203, 139, nch)
    assert_within_bound(f32_of(res[1], nch), plain[100:190, 9:129], 40, 30, (name, "orientation 6", crop))


# ---- 4. every format and layout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,size", [("modular_rgba8", (48, 32)), ("fused_rgb_odd", (211, 7)), ("modular_greya8", (33, 17))])
def test_formats_follow_from_the_f32_resized_output(jx, name, size):
    """{u8, u16 both byte orders, f16, f32} x 1-4 channels x {align 0, one that pads} x {interleaved, tight planes, plane_stride + 52 samples} and, for the float types,
    the same with scale / bias: each destination is numpy (convert_samples, planes as in test_planar_output.py) applied to the f32 resized decode of the same channel
    count, target and scale / bias — byte for byte, guard bytes, row padding and plane gaps still FILL."""
    data = stream(name)[0]
    ow, oh = size
    crop = (5, 3, 120, 70) if name == "modular_rgba8" else None
    common = dict(resize=size) if crop is None else dict(resize=size, crop=crop)
    aff = lambda nch: dict(scale=SCALE[:nch], bias=BIAS[:nch])
    bases = [(nch, affine) for nch in (1, 2, 3, 4) for affine in (False, True)]
    specs = [F32(jx, nch, **common, **(aff(nch) if affine else {})) for nch, affine in bases]
    formats = []
    for dtype, big in (("uint8", False), ("uint16", False), ("uint16", True), ("float16", False), ("float32", True)):
        for nch in (1, 2, 3, 4):
            for planar, gap in ((False, 0), (True, 0), (True, 52)):
                for align in (0, padding_align(ow * BPS[dtype] * (1 if planar else nch))):
                    for affine in ((False, True) if dtype in ("float16", "float32") else (False,)):
                        sp = dict(dtype=dtype, num_channels=nch, endianness=jx.JXL_BIG_ENDIAN if big else jx.JXL_LITTLE_ENDIAN, align=align, **common)
                        if planar:
                            sp.update(planar=True, plane_stride=(oh * padded_stride(ow * BPS[dtype], align) + 52 * BPS[dtype]) if gap else 0)
                        if affine:
                            sp.update(aff(nch))
                        formats.append((sp, nch, affine))
    res = decode_specs(jx, data, specs + [sp for sp, _, _ in formats])
    base = {key: f32_of(res[k], key[0]) for k, key in enumerate(bases)}
    assert base[(4, False)][..., 0].std() > 0.01 and not np.array_equal(base[(4, True)], base[(4, False)])
    for (sp, nch, affine), (d, n, dims) in zip(formats, res[len(specs):]):
        assert dims == size
        bps = BPS[sp["dtype"]]
        q = convert_samples(base[(nch, affine)], sp["dtype"])
        if sp["endianness"] == jx.JXL_BIG_ENDIAN:
            q = q.byteswap()
        samples = np.ascontiguousarray(q).view(np.uint8).reshape(oh, ow, nch, bps)
        if sp.get("planar"):
            want = expected_planar_dest(samples, sp, n)
        else:
            row = ow * nch * bps
            stride = padded_stride(row, sp["align"])
            assert n == stride * (oh - 1) + row
            rows = np.full((oh, stride), FILL, np.uint8)
            rows[:, :row] = samples.reshape(oh, row)
            want = np.full(n + EXTRA, FILL, np.uint8)
            want[FRONT:FRONT + n] = rows.reshape(-1)[:n]
        assert_dest(d, want, (name, sp))


# ---- 5. orientation, 1:8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_orientation_and_downscale(jx):
    """Orientations 2, 6 and 7, and keep_orientation on a stream of orientation 6: the resized output against restate() of the plain f32 decode with the same options
    (the source of the resize is the oriented picture, or the stored one).  downscale = 8 with a target: 1030 x 520 -> 129 x 65 -> 64 x 32, against restate() of the 1:8
    f32 decode."""
    for o, keep in ((2, False), (6, False), (7, False), (6, True)):
        data = stream("fused_rgb_odd", o)[0]
        res = decode_specs(jx, data, [F32(jx, 3), F32(jx, 3, resize=(48, 32)), F32(jx, 3, resize=(32, 48), crop=(7, 11, 100, 120))], keep_orientation=keep)
        plain = f32_of(res[0], 3)
        assert plain.shape[:2] == ((203, 139) if o > 4 and not keep else (139, 203))
        assert_within_bound(f32_of(res[1], 3), plain, 48, 32, ("orientation", o, keep))
        assert_within_bound(f32_of(res[2], 3), plain[11:131, 7:107], 32, 48, ("orientation", o, keep, "crop"))
        if o == 6 and not keep:
            stored = f32_of(decode_specs(jx, stream("fused_rgb_odd")[0], [F32(jx, 3)])[0], 3)
            assert np.array_equal(plain, ORIENT[6](stored))
    data = plain_stream(1030, 520)
    res = decode_specs(jx, data, [F32(jx, 3, downscale=8), F32(jx, 3, downscale=8, resize=(64, 32)), F32(jx, 4, downscale=8, resize=(20, 30), crop=(100, 5, 29, 60))])
    small = f32_of(res[0], 3)
    assert small.shape == (65, 129, 3)
    assert_within_bound(f32_of(res[1], 3), small, 64, 32, "1:8")
    assert_within_bound(f32_of(res[2], 4)[..., :3], small[5:65, 100:129], 20, 30, "1:8 crop")


# ---- 6. pipeline --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pipeline_job_into_one_tensor(jx):
    """A job of four differently sized streams (a fused VarDCT frame, a Modular RGBA image, sample.jxl, the 2056 x 24 frame) as planar f16 with scale / bias into
    consecutive slices of one [4, 3, 32, 48] device tensor, and to pinned host memory: the batch's results for the same parameters.  A crop that leaves some of the
    images, and a capacity one byte short, fail those images alone; resized, plain, resized jobs go through one pipeline."""
    import torch
    datas = [stream("fused_rgb_w4")[0], stream("modular_rgba8")[0], fixture_bytes("sample.jxl"), plain_stream(2056, 24)]
    sizes_px = [(i.xsize, i.ysize) for i in (jx.image_out_size(d)[0] for d in datas)]
    assert len(set(sizes_px)) == 4
    lay = dict(planar=True, scale=SCALE[:3], bias=BIAS[:3], resize=(48, 32))

    def batch(data, dtype, **kw):
        (d, n, _), = decode_specs(jx, data, [dict(dtype=dtype, num_channels=3, endianness=jx.JXL_LITTLE_ENDIAN, **kw)])
        return d[FRONT:FRONT + n].copy()
    refs = [batch(d, "float16", **lay) for d in datas]
    one = 3 * 32 * 48 * 2
    assert [r.size for r in refs] == [one] * 4 and [jx.image_out_size(d, "float16", 3, **lay)[1] for d in datas] == [one] * 4
    p = jx.Pipeline(0, jobs_in_flight=2, lf_streams=2, prepare_threads=1, parse_threads=2, reserve_frames=4, reserve_width=2112, reserve_height=640)
    try:
        out = torch.full((4, 3, 32, 48), 7.0, dtype=torch.float16, device="cuda:0")
        st, _ = p.wait(p.submit(datas, "float16", 3, device_ptrs=[out[k].data_ptr() for k in range(4)], capacities=[one] * 4, **lay))
        torch.cuda.synchronize()
        assert st == [0, 0, 0, 0]
        got = out.cpu().numpy()
        for k in range(4):
            assert np.array_equal(got[k].view(np.uint8).reshape(-1), refs[k]), k
        # (and it is the normalised picture: slot 1 has scale 1 / bias 0, within half precision of the formula applied to the plain decode)
        plain = batch(datas[0], "float32").view("<f4").reshape(136, 200, 3)
        assert np.abs(got[0, 1].astype(np.float64) - restate(plain, 48, 32)[0][..., 1]).max() <= 2.0 ** -10 * max(1.0, float(np.abs(plain).max()))
        pinned = jx.PinnedBuffer(4 * one)
        st, _ = p.wait(p.submit(datas, "float16", 3, host_ptrs=[pinned.ptr + k * one for k in range(4)], capacities=[one] * 4, **lay))
        assert st == [0, 0, 0, 0] and np.array_equal(pinned.array, np.concatenate(refs))
        # a crop some of the images do not hold: those fail alone, the others are the batch's result for that crop
        crop = (150, 4, 60, 20)
        fits = [x >= 210 and y >= 24 for x, y in sizes_px]
        assert fits[3] and not fits[0] and not fits[1]
        pinned = [jx.PinnedBuffer(one) for _ in datas]
        st, _ = p.wait(p.submit(datas, "float16", 3, host_ptrs=[o.ptr for o in pinned], capacities=[one] * 4, crop=crop, **lay), check=False)
        assert st == [0 if f else 1 for f in fits] and "leaves the 200 x 136 picture" in jx.last_error()
        for k in range(4):
            if fits[k]:
                assert np.array_equal(pinned[k].array, batch(datas[k], "float16", crop=crop, **lay)), k
        # one byte short: that image alone
        pinned = [jx.PinnedBuffer(one) for _ in datas]
        st, _ = p.wait(p.submit(datas, "float16", 3, host_ptrs=[o.ptr for o in pinned], capacities=[one, one - 1, one, one], **lay), check=False)
        assert st == [0, 1, 0, 0] and "too small" in jx.last_error()
        for k in (0, 2, 3):
            assert np.array_equal(pinned[k].array, refs[k]), k
        # resized, plain, resized: nothing of the resize stays behind in the slots
        refs_u8 = [batch(d, "uint8") for d in datas]
        a = [jx.PinnedBuffer(one) for _ in datas]
        b = [jx.PinnedBuffer(r.size) for r in refs_u8]
        c = [jx.PinnedBuffer(one) for _ in datas]
        t1 = p.submit(datas, "float16", 3, host_ptrs=[o.ptr for o in a], capacities=[one] * 4, **lay)
        t2 = p.submit(datas, "uint8", 3, host_ptrs=[o.ptr for o in b], capacities=[r.size for r in refs_u8])
        t3 = p.submit(datas, "float16", 3, host_ptrs=[o.ptr for o in c], capacities=[one] * 4, **lay)
        assert p.wait(t1)[0] == [0] * 4 and p.wait(t2)[0] == [0] * 4 and p.wait(t3)[0] == [0] * 4
        for o, r in zip(a + b + c, refs + refs_u8 + refs):
            assert np.array_equal(o.array, r)
        # a target side of 0: the submission is refused
        with pytest.raises(jx.DecodeError, match="a target side of 0"):
            p.submit(datas, "uint8", 3, host_ptrs=[o.ptr for o in b], resize=(0, 4))
    finally:
        p.close()


# ---- 7. nothing stays behind --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_resize_does_not_outlive_its_output(jx):
    """The same BatchDecoder, reset, decodes without a resize what a fresh one decodes.  device_bytes of a batch with a resized output exceeds that of the same batch
    without it by at least the two intermediates (the 200 x 136 x 4 f32 picture and the 136 rows of 48 filtered pixels; both destinations are the caller's)."""
    import torch
    data = stream("fused_rgba_w4")[0]
    dst = torch.zeros(200 * 136 * 16, dtype=torch.uint8, device="cuda:0")
    b = jx.BatchDecoder(0)
    outs, dev = [], []
    for kw in (dict(resize=(48, 32), crop=None), dict()):
        b.reset()
        b.add(data, "float32", 4, device_ptr=dst.data_ptr(), **kw)
        b.prepare(); b.decode(); b.finish()
        outs.append(b.output(0).copy())
        dev.append(b.device_bytes)
    fresh = jx.BatchDecoder(0)
    fresh.add(data, "float32", 4, device_ptr=dst.data_ptr())
    fresh.prepare(); fresh.decode(); fresh.finish()
    assert np.array_equal(outs[1].view(np.uint32), fresh.output(0).view(np.uint32))
    assert outs[0].size == 48 * 32 * 4 and outs[1].size == 200 * 136 * 4
    print("device_bytes resized", dev[0], "plain", dev[1], "fresh plain", fresh.device_bytes)
    assert dev[0] - fresh.device_bytes >= 200 * 136 * 16 + 136 * 48 * 16
