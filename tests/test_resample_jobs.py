"""Per-image crop, mirror and bicubic filter of resized outputs, and the table-driven resize launch (include/jxl_hip.h JxlHipOutputResample; decoder.cc ResizeAxis;
kernels_features.hip ResizeKernel; pipeline.cc).

Both filters are one rule per axis with a kernel k of radius r (jxl_hip.h): n_in -> n_out, scale = n_in / n_out, s = max(scale, 1), target sample i centred at
c = scale x (i + 0.5) takes the samples j of [max(0, int(c - r s + 0.5)), min(n_in, int(c + r s + 0.5))) with weights k((j - c + 0.5) / s) over their sum.  `restate`
below is that rule in float64 numpy, importing nothing from the product; test_restatement_equals_torch_float64 pins it against torch's float64
interpolate(mode="bilinear" / "bicubic", antialias=True) without a device.  Every GPU comparison then has the product's own plain f32 decode as its input.

The bound of the f32 comparison is derived, not measured: (taps_x + taps_y + 8) x 2^-24 x L_x x L_y x max|v|.  `taps` is the longest tap range of the axis; L is the
largest sum of |w| of any output sample of the axis, computed here from restate's weights (1 for the triangle filter, whose weights are non-negative: the bound of
test_resized_output.py).  The host rounds each normalised weight to f32 once and the kernel accumulates w0 x v0, then one fmaf per further tap: every rounding is
relative 2^-24 on a partial sum of at most L x max|v|, and the vertical pass sees inputs of up to L_x x max|v|.

A mirrored output is the output without mirror with its columns reversed, exactly: the tests flip the sample bytes of the whole destination, guard bytes included.

Streams, the numpy write stage and the destinations with guard bytes are those of test_write_stage.py, test_planar_output.py and test_resized_output.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import fixture_bytes
from test_write_stage import convert_samples, padded_stride, padding_align
from test_downscaled_decode import plain_stream
from test_planar_output import BIAS, BPS, EXTRA, FILL, FRONT, SCALE, assert_dest, expected_planar_dest, stream
from test_resized_output import CROPS, PAIRS

FILTERS = {"bilinear": 0, "bicubic": 1}


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
def kernel(filter, x):
    x = np.abs(np.asarray(x, np.float64))
    if filter == "bilinear":
        return np.maximum(0.0, 1.0 - x)
    assert filter == "bicubic"
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, a * (((x - 5.0) * x + 8.0) * x - 4.0), 0.0))


def axis_taps(n_in, n_out, filter):
    """per output index: (lo, hi, normalised float64 weights of the samples lo .. hi - 1)"""
    scale = n_in / n_out
    s = max(scale, 1.0)
    r = {"bilinear": 1.0, "bicubic": 2.0}[filter]
    taps = []
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo = max(0, int(c - r * s + 0.5))
        hi = min(n_in, int(c + r * s + 0.5))
        w = kernel(filter, (np.arange(lo, hi) - c + 0.5) / s)
        taps.append((lo, hi, w / w.sum()))
    return taps


def restate(x, size, filter):
    """(h, w, c) array, (ow, oh) -> ((oh, ow, c) float64, (longest tap range across, down), (largest sum of |w| across, down)): horizontal pass, then vertical"""
    x = np.asarray(x, np.float64)
    ow, oh = size
    tx, ty = axis_taps(x.shape[1], ow, filter), axis_taps(x.shape[0], oh, filter)
    tmp = np.stack([np.tensordot(w, x[:, lo:hi], axes=(0, 1)) for lo, hi, w in tx], axis=1)
    out = np.stack([np.tensordot(w, tmp[lo:hi], axes=(0, 0)) for lo, hi, w in ty], axis=0)
    return out, tuple(max(hi - lo for lo, hi, _ in t) for t in (tx, ty)), tuple(max(float(np.abs(w).sum()) for _, _, w in t) for t in (tx, ty))


def test_restatement_equals_torch_float64(jxh):
    """restate() = torch.nn.functional.interpolate(x.double(), size, mode, antialias=True, align_corners=False) on the CPU to 1e-12 for mode "bilinear" and "bicubic", on
    random arrays of the seven source / target pairs of test_resized_output.py plus 5 x 3 -> 11 x 7 (an enlargement whose every tap range is cut by an edge)."""
    import torch
    rng = np.random.default_rng(11)
    assert max(hi - lo for lo, hi, _ in axis_taps(2056, 9, "bicubic")) == 914
    for lo, hi, w in axis_taps(67, 67, "bicubic"):                      # (the same size: the weights are exactly 0, 1, 0, 0 — what is left after the trim is a copy)
        assert sorted(w.tolist())[-1] == 1.0 and np.count_nonzero(w) == 1
    assert len(PAIRS) == 7
    for (w, h), (ow, oh) in PAIRS + [((5, 3), (11, 7))]:
        x = rng.standard_normal((h, w, 3))
        for filter in ("bilinear", "bicubic"):
            want = torch.nn.functional.interpolate(torch.from_numpy(x).permute(2, 0, 1)[None].double(), size=(oh, ow), mode=filter, antialias=True, align_corners=False)
            got, taps, lsum = restate(x, (ow, oh), filter)
            err = np.abs(got - want[0].permute(1, 2, 0).numpy()).max()
            print(filter, (w, h), "->", (ow, oh), "taps", taps, "sum |w|", lsum, "max difference", err)
            assert err <= 1e-12, (filter, (w, h), (ow, oh), err)
            assert filter == "bicubic" or max(lsum) <= 1.0 + 1e-15                 # (non-negative weights: L = 1, the triangle filter's bound)


# ---- refusals (no GPU) ------------------------------------------------------------------------------------------------------------------------
def test_refusals(jxh):
    """The layout of JxlHipOutputResample; filter = 2, a NULL resample, an empty crop, a target side of 0 and above 65535 are refused by message through
    JxlHipBatchOutBufferSizeResampled, which checks its arguments before it looks at the batch (a NULL batch here: no device is needed, and valid arguments then end in
    "no such image"); the Python keywords refuse a filter or a mirror without a target and an unknown filter name.  Two entries with different targets are a matter of
    the submission: test_pipeline_job_with_a_resample_per_image."""
    R = jxh.JxlHipOutputResample
    assert [n for n, _ in R._fields_] == ["xsize", "ysize", "crop_x0", "crop_y0", "crop_xsize", "crop_ysize", "filter", "mirror"] and C.sizeof(R) == 32
    assert C.sizeof(jxh.JxlHipOutputResize) == 24                       # (read by callers through a fixed layout: unchanged)
    L = jxh.libjxl()
    fmt = jxh.JxlPixelFormat(3, jxh._PIXEL_TYPES["uint8"][0], jxh.JXL_LITTLE_ENDIAN, 0)
    size = C.c_size_t()

    def refused(rs, downscale=1):
        assert L.JxlHipBatchOutBufferSizeResampled(None, 0, C.byref(fmt), downscale, None, None if rs is None else C.byref(rs), C.byref(size)) != 0
        return jxh.last_error()
    assert "filter 2 is not known" in refused(R(48, 32, 0, 0, 0, 0, 2, 0))
    assert "filter 4294967295 is not known" in refused(R(48, 32, 0, 0, 0, 0, 2 ** 32 - 1, 1))
    assert "no JxlHipOutputResample given" in refused(None)
    for crop in ((3, 3, 0, 0), (0, 0, 5, 0), (0, 0, 0, 5)):
        assert "the crop is empty" in refused(R(48, 32, *crop, 1, 1))
    assert "a target side of 0" in refused(R(0, 32, 0, 0, 0, 0, 1, 0))
    assert "a target side above 65535" in refused(R(48, 65536, 0, 0, 0, 0, 0, 1))
    assert "downscale must be 1 or 8" in refused(R(48, 32, 0, 0, 0, 0, 1, 0), downscale=4)
    for ok in (R(48, 32, 0, 0, 0, 0, 0, 0), R(48, 32, 1, 2, 3, 4, 1, 1)):
        assert "no such image" in refused(ok)
    assert L.JxlHipBatchSetOutputResampled(None, 0, C.byref(fmt), None, 1, None, C.byref(R(48, 32, 0, 0, 0, 0, 2, 0))) != 0 and "filter 2 is not known" in jxh.last_error()
    with pytest.raises(ValueError, match="need resize"):
        jxh._resample(None, None, "bicubic", False)
    with pytest.raises(ValueError, match="filter must be one of"):
        jxh._resample((4, 4), None, "lanczos", False)
    # one value for the job or per-image values: four plain integers are one crop, any other iterable — a generator included — is a sequence of n entries
    one_crop = lambda v: len(v) == 4 and all(isinstance(x, int) for x in v)
    assert jxh._per_image((1, 2, 3, 4), 4, one_crop) == ([(1, 2, 3, 4)] * 4, False)
    assert jxh._per_image((c for c in [(1, 2, 3, 4), None]), 2, one_crop) == ([(1, 2, 3, 4), None], True)
    assert jxh._per_image(iter([1, 2, 3, 4]), 3, one_crop) == ([(1, 2, 3, 4)] * 3, False)
    assert jxh._per_image("bicubic", 2, lambda v: False) == (["bicubic"] * 2, False) and jxh._per_image(None, 2, one_crop) == ([None] * 2, False)
    assert jxh._per_image((m for m in (True, False, True)), 3, lambda v: False) == ([True, False, True], True)
    with pytest.raises(ValueError, match="needs 3 entries"):
        jxh._per_image([True, False], 3, lambda v: False)
    rs = jxh._resample((48, 32), (1, 2, 3, 4), "bicubic", True)
    assert [getattr(rs, n) for n, _ in R._fields_] == [48, 32, 1, 2, 3, 4, 1, 1]


# ---- one batch, many outputs -----------------------------------------------------------------------------------------------------------------
def decode_items(jx, items, keep_orientation=False, options=()):
    """items: (data, dict of BatchDecoder.add keywords) pairs.  Every item is one image of ONE batch, decoded into a device buffer of out_size + EXTRA bytes filled with
    FILL, the output FRONT bytes into it.  -> (list of (whole destination as uint8 array, out_size, (output width, height)), resize launches of the decode)"""
    import torch
    b = jx.BatchDecoder(0)
    b.set_option("keep_orientation", 1 if keep_orientation else 0)
    for name, value in options:
        b.set_option(name, value)
    bufs, sizes = [], []
    for data, sp in items:
        size = jx.image_out_size(data, **{k: v for k, v in sp.items() if k not in ("filter", "mirror")})[1]      # (neither changes a size)
        t = torch.full((size + EXTRA,), FILL, dtype=torch.uint8, device="cuda:0")
        i = b.add(data, device_ptr=t.data_ptr() + FRONT, **sp)
        assert b.out_size(i) == size, (sp, b.out_size(i), size)
        bufs.append(t); sizes.append(size)
    b.prepare(); b.decode(); b.finish()
    torch.cuda.synchronize()
    launches = b.info_value("resize_launches")
    dims = []
    for i, (_, sp) in enumerate(items):
        w, h = b.info(i).xsize, b.info(i).ysize
        dims.append(tuple(sp["resize"]) if sp.get("resize") else ((w + 7) // 8, (h + 7) // 8) if sp.get("downscale", 1) == 8 else (w, h))
    return [(t.cpu().numpy(), n, d) for t, n, d in zip(bufs, sizes, dims)], launches


def decode_specs(jx, data, specs, keep_orientation=False):
    return decode_items(jx, [(data, sp) for sp in specs], keep_orientation)[0]


def f32_of(res, nch):
    d, n, (w, h) = res
    assert n == w * h * nch * 4, (n, w, h, nch)
    assert (d[:FRONT] == FILL).all() and (d[FRONT + n:] == FILL).all()
    return d[FRONT:FRONT + n].view("<f4").reshape(h, w, nch).copy()


def F32(jx, nch, **kw):
    return dict(dtype="float32", num_channels=nch, endianness=jx.JXL_LITTLE_ENDIAN, **kw)


def assert_within_bound(got, plain, size, filter, tag):
    want, (tx, ty), (lx, ly) = restate(plain, size, filter)
    bound = (tx + ty + 8) * 2.0 ** -24 * lx * ly * float(np.abs(plain).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(tag, filter, "taps", (tx, ty), "sum |w|", (round(lx, 4), round(ly, 4)), "max error", err, "bound", bound)
    assert got.shape == want.shape and np.isfinite(got).all()
    assert err <= bound, (tag, err, bound)
    return tx, ty


def _stream_of(name):
    return plain_stream(2056, 24) if name == "plain_2056x24" else stream(name)[0]


# ---- 1. the cubic f32 output against the formula ---------------------------------------------------------------------------------------------
CUBIC_CASES = {
    "fused_rgb_odd": [(3, (48, 32)), (3, (224, 224)), (4, (48, 32))],                  # 203 x 139: odd sides; an enlargement
    "modular_rgba8": [(4, (48, 32)), (4, (224, 224)), (3, (224, 224))],                # 203 x 139 with a real alpha channel and samples of exactly 0 and 1 next to each other
    "fused_rgb_three_groups": [(3, (300, 7)), (4, (300, 7))],                           # 520 x 72
    "plain_2056x24": [(3, (9, 5)), (4, (9, 5))],                                        # 914 taps across
    "fused_rgba_odd": [(4, (67, 41)), (3, (67, 41)), (4, (1, 1)), (3, (1, 1))],         # 67 x 41: the same size, and everything into one pixel
    "fused_rgb_w4": [(3, (33, 17)), (4, (33, 17))],                                     # 200 x 136: the last block of threads is partly outside, both ways
    "modular_grey8": [(1, (33, 17)), (2, (48, 32)), (1, (100, 150))],                   # 77 x 139, grey: one and two slots
    "vardct_layers": [(4, (48, 32))],                                                   # the frame tail's WriteKernel
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CUBIC_CASES))
def test_cubic_f32_against_the_defining_formula(jx, name):
    """The f32 output resampled with filter="bicubic" against restate(..., "bicubic") of the product's own plain f32 decode of the same stream and channel count, within
    (taps_x + taps_y + 8) x 2^-24 x L_x x L_y x max|v| (module docstring).  The enlargement of the 203 x 139 Modular picture leaves [0, 1] on both sides (the negative lobes);
    a target of the source's size is the plain decode bit for bit; crops that touch each edge are the formula applied to the cropped decode."""
    data = _stream_of(name)
    cases = CUBIC_CASES[name]
    chans = sorted({nch for nch, _ in cases})
    crops = CROPS if name == "fused_rgb_odd" else []
    specs = [F32(jx, nch) for nch in chans] + [F32(jx, nch, resize=size, filter="bicubic") for nch, size in cases] + \
            [F32(jx, 3, resize=size, crop=crop, filter="bicubic") for crop, size in crops]
    res = decode_specs(jx, data, specs)
    plain = {nch: f32_of(res[k], nch) for k, nch in enumerate(chans)}
    taps = set()
    for (nch, size), r in zip(cases, res[len(chans):]):
        got = f32_of(r, nch)
        assert plain[nch][..., 0].std() > 0.01
        taps.add(assert_within_bound(got, plain[nch], size, "bicubic", (name, nch, size)))
        if size == (224, 224):
            print(name, nch, "range of the enlarged picture", float(got.min()), float(got.max()), "of the plain decode", float(plain[nch].min()), float(plain[nch].max()))
            if name == "modular_rgba8":       # (its samples of exactly 0 and 1 lie next to each other; the VarDCT picture spans 0.045 .. 0.999 and its enlargement stays inside)
                assert got.min() < 0.0 and got.max() > 1.0, (name, nch, float(got.min()), float(got.max()))
        if size == plain[nch].shape[1::-1]:
            assert np.array_equal(got.view(np.uint32), plain[nch].view(np.uint32)), (name, nch, "the same size is not a copy")
    for (crop, size), r in zip(crops, res[len(chans) + len(cases):]):
        x0, y0, w, h = crop
        assert_within_bound(f32_of(r, 3), plain[3][y0:y0 + h, x0:x0 + w], size, "bicubic", (name, crop))
    if name == "plain_2056x24":
        assert {tx for tx, _ in taps} == {914}
    if name == "fused_rgba_odd":
        assert taps == {(4, 4), (67, 41)}             # (the formula's own ranges: four samples at the same size, of which the host keeps the one of weight 1; the whole picture)


# ---- 2. every format and layout of the enlargement ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cubic_formats_follow_from_f32(jx):
    """The 203 x 139 RGBA picture enlarged to 224 x 224 with the cubic filter: {u8, u16, f16, f32} x 3 / 4 channels x {interleaved, tight planes, plane_stride + 52 samples}
    x {align 0, one that pads} and, for the float types, the same with scale / bias.  Each destination is numpy (convert_samples: clip, then round half to even) applied to
    the f32 cubic output of the same channel count and scale / bias — byte for byte, guard bytes, row padding and plane gaps still FILL.  The f32 picture leaves [0, 1] on
    both sides; the integer types hold 0 and their maximum exactly there."""
    data = stream("modular_rgba8")[0]
    size = ow, oh = (224, 224)
    common = dict(resize=size, filter="bicubic")
    aff = lambda nch: dict(scale=SCALE[:nch], bias=BIAS[:nch])
    bases = [(nch, affine) for nch in (3, 4) for affine in (False, True)]
    specs = [F32(jx, nch, **common, **(aff(nch) if affine else {})) for nch, affine in bases]
    formats = []
    for dtype in ("uint8", "uint16", "float16", "float32"):
        for nch in (3, 4):
            for planar, gap in ((False, 0), (True, 0), (True, 52)):
                for align in (0, padding_align(ow * BPS[dtype] * (1 if planar else nch))):
                    for affine in ((False, True) if dtype in ("float16", "float32") else (False,)):
                        sp = dict(dtype=dtype, num_channels=nch, endianness=jx.JXL_LITTLE_ENDIAN, align=align, **common)
                        if planar:
                            sp.update(planar=True, plane_stride=(oh * padded_stride(ow * BPS[dtype], align) + 52 * BPS[dtype]) if gap else 0)
                        if affine:
                            sp.update(aff(nch))
                        formats.append((sp, nch, affine))
    res = decode_specs(jx, data, specs + [sp for sp, _, _ in formats])
    base = {key: f32_of(res[k], key[0]) for k, key in enumerate(bases)}
    below, above = base[(4, False)] < 0.0, base[(4, False)] > 1.0
    print("samples below 0:", int(below.sum()), "above 1:", int(above.sum()), "range", float(base[(4, False)].min()), float(base[(4, False)].max()))
    assert below.any() and above.any()
    for (sp, nch, affine), (d, n, dims) in zip(formats, res[len(specs):]):
        assert dims == size
        bps = BPS[sp["dtype"]]
        q = convert_samples(base[(nch, affine)], sp["dtype"])
        if sp["dtype"] in ("uint8", "uint16") and nch == 4:
            full = 255 if sp["dtype"] == "uint8" else 65535
            assert (q[below] == 0).all() and (q[above] == full).all()                     # (the overshoot is clamped, not wrapped)
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
        assert_dest(d, want, ("modular_rgba8", sp))


# ---- 3. mirror ---------------------------------------------------------------------------------------------------------------------------------
def flipped_dest(dest, n, sp, dims):
    """The destination `dest` (of a decode without mirror) with the sample bytes of every row reversed pixel by pixel; every other byte as it is"""
    ow, oh = dims
    nch, bps, align = sp["num_channels"], BPS[sp["dtype"]], sp.get("align", 0)
    want = dest.copy()
    if sp.get("planar"):
        rs = padded_stride(ow * bps, align)
        ps = sp.get("plane_stride", 0) or rs * oh
        assert n == nch * ps
        for c in range(nch):
            for y in range(oh):
                o = FRONT + c * ps + y * rs
                want[o:o + ow * bps] = dest[o:o + ow * bps].reshape(ow, bps)[::-1].reshape(-1)
    else:
        row = ow * nch * bps
        stride = padded_stride(row, align)
        assert n == stride * (oh - 1) + row
        for y in range(oh):
            o = FRONT + y * stride
            want[o:o + row] = dest[o:o + row].reshape(ow, nch * bps)[::-1].reshape(-1)
    return want


def check_mirror(jx, data, specs, tag, keep_orientation=False):
    """every spec decoded without and with mirror in one batch: the mirrored destination is the flipped plain one, byte for byte over the whole destination"""
    res = decode_specs(jx, data, specs + [dict(sp, mirror=True) for sp in specs], keep_orientation)
    for k, sp in enumerate(specs):
        (d0, n0, dims0), (d1, n1, dims1) = res[k], res[len(specs) + k]
        assert n0 == n1 and dims0 == dims1 == tuple(sp["resize"])
        assert (d0[:FRONT] == FILL).all() and (d0[FRONT + n0:] == FILL).all() and d0[FRONT:FRONT + n0].std() > 0
        assert_dest(d1, flipped_dest(d0, n0, sp, dims0), (tag, sp))
        if dims0[0] > 1:
            assert not np.array_equal(d0, d1), (tag, sp, "the mirror changed nothing")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fused_rgb_odd", "modular_rgba8"])
def test_mirror_is_the_flipped_output(jx, name):
    """mirror=True stores target column ox at column width - 1 - ox: the destination of the same decode without mirror with its columns reversed — both filters, u8 / f16 /
    f32, 3 and 4 channels, interleaved and planar with padded rows and a plane gap, target widths 1, 7, 64 and 65 (one block of threads, one more), a crop, scale / bias;
    under orientation 6, with keep_orientation, and at downscale = 8."""
    data = stream(name)[0]
    specs = []
    for filter in ("bilinear", "bicubic"):
        for dtype in ("uint8", "float16", "float32"):
            for nch in (3, 4):
                for ow, oh in ((1, 3), (7, 5), (64, 9), (65, 33)):
                    bps = BPS[dtype]
                    base = dict(dtype=dtype, num_channels=nch, endianness=jx.JXL_LITTLE_ENDIAN, resize=(ow, oh), filter=filter)
                    specs.append(dict(base, align=padding_align(ow * nch * bps)))
                    al = padding_align(ow * bps)
                    specs.append(dict(base, align=al, planar=True, plane_stride=oh * padded_stride(ow * bps, al) + 52 * bps))
        specs.append(F32(jx, 4, resize=(65, 33), crop=(103, 89, 100, 50), filter=filter))
        specs.append(dict(dtype="float16", num_channels=3, endianness=jx.JXL_LITTLE_ENDIAN, resize=(7, 5), crop=(0, 40, 203, 30), filter=filter, planar=True,
                          scale=SCALE[:3], bias=BIAS[:3]))
    check_mirror(jx, data, specs, name)
    few = [dict(dtype=dtype, num_channels=nch, endianness=jx.JXL_LITTLE_ENDIAN, resize=(65, 33), filter=filter, align=0, **lay)
           for filter in ("bilinear", "bicubic") for dtype, nch, lay in (("uint8", 3, {}), ("float32", 4, dict(planar=True)), ("float16", 3, dict(crop=(9, 100, 120, 90))))]
    data6 = stream(name, 6)[0]
    check_mirror(jx, data6, few, (name, "orientation 6"))                                     # (the picture is 139 x 203: the crop is one of the oriented picture)
    check_mirror(jx, data6, few[:2] + few[3:5], (name, "keep_orientation"), keep_orientation=True)
    if name == "fused_rgb_odd":
        small = [dict(sp, downscale=8, resize=(7, 5)) for sp in few if "crop" not in sp] + [F32(jx, 3, downscale=8, resize=(64, 9), crop=(3, 2, 20, 15), filter="bicubic")]
        check_mirror(jx, data, small, (name, "downscale 8"))                                  # (203 x 139 at 1:8 is 26 x 18)


# ---- 4. pipeline: a resample per image -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pipeline_job_with_a_resample_per_image(jx):
    """One job of five differently sized streams, each with a crop (one None), a filter and a mirror of its own, as planar f16 with scale / bias into consecutive slices
    of one [5, 3, 32, 48] device tensor, and to pinned host memory: each slice is the BatchDecoder's result for that image with the same parameters, exactly.  An image
    whose crop leaves it, and a capacity one byte short, fail alone and the others stay exact; resampled, plain, resampled jobs go through one pipeline; differing targets
    and filter = 2 refuse the submission."""
    import torch
    datas = [stream("fused_rgb_w4")[0], stream("modular_rgba8")[0], fixture_bytes("sample.jxl"), plain_stream(2056, 24), stream("fused_rgb_three_groups")[0]]
    sizes_px = [(i.xsize, i.ysize) for i in (jx.image_out_size(d)[0] for d in datas)]
    assert len(set(sizes_px)) == 5
    n = len(datas)
    sw, sh = sizes_px[2]
    crops = [(100, 4, 100, 132), None, (sw // 4, sh // 5, sw // 2, sh // 2), (1000, 2, 600, 20), (0, 0, 520, 72)]
    filters = ["bicubic", "bilinear", "bicubic", "bicubic", "bilinear"]
    mirrors = [True, True, False, True, True]
    lay = dict(planar=True, scale=SCALE[:3], bias=BIAS[:3], resize=(48, 32))

    def batch(data, dtype, **kw):
        (d, m, _), = decode_specs(jx, data, [dict(dtype=dtype, num_channels=3, endianness=jx.JXL_LITTLE_ENDIAN, **kw)])
        return d[FRONT:FRONT + m].copy()

    def own(k, crop):
        return dict({} if crop is None else dict(crop=crop), filter=filters[k], mirror=mirrors[k])
    refs = [batch(datas[k], "float16", **own(k, crops[k]), **lay) for k in range(n)]
    one = 3 * 32 * 48 * 2
    assert [r.size for r in refs] == [one] * n
    # (the five parameter sets really differ: no slice is the job-wide triangle resize of its image)
    assert all(not np.array_equal(refs[k], batch(datas[k], "float16", **lay)) for k in range(n))
    p = jx.Pipeline(0, jobs_in_flight=2, lf_streams=2, prepare_threads=1, parse_threads=2, reserve_frames=5, reserve_width=2112, reserve_height=640)
    try:
        out = torch.full((n, 3, 32, 48), 7.0, dtype=torch.float16, device="cuda:0")
        st, _ = p.wait(p.submit(datas, "float16", 3, device_ptrs=[out[k].data_ptr() for k in range(n)], capacities=[one] * n, crop=crops, filter=filters, mirror=mirrors, **lay))
        torch.cuda.synchronize()
        assert st == [0] * n
        got = out.cpu().numpy()
        for k in range(n):
            assert np.array_equal(got[k].view(np.uint8).reshape(-1), refs[k]), k
        pinned = jx.PinnedBuffer(n * one)
        st, _ = p.wait(p.submit(datas, "float16", 3, host_ptrs=[pinned.ptr + k * one for k in range(n)], capacities=[one] * n, crop=crops, filter=filters, mirror=mirrors, **lay))
        assert st == [0] * n and np.array_equal(pinned.array, np.concatenate(refs))
        # one value for the job and a sequence mix: the same filter for all, per-image mirrors
        cub = [batch(datas[k], "float16", filter="bicubic", mirror=mirrors[k], **lay) for k in range(n)]
        pinned = jx.PinnedBuffer(n * one)
        st, _ = p.wait(p.submit(datas, "float16", 3, host_ptrs=[pinned.ptr + k * one for k in range(n)], capacities=[one] * n, filter="bicubic", mirror=mirrors, **lay))
        assert st == [0] * n and np.array_equal(pinned.array, np.concatenate(cub))
        # the crop of image 1 leaves its 203 x 139 picture: that image alone, the others stay exact
        bad = list(crops); bad[1] = (150, 4, 60, 20)
        pinned = [jx.PinnedBuffer(one) for _ in datas]
        st, _ = p.wait(p.submit(datas, "float16", 3, host_ptrs=[o.ptr for o in pinned], capacities=[one] * n, crop=bad, filter=filters, mirror=mirrors, **lay), check=False)
        assert st == [0, 1, 0, 0, 0] and "leaves the 203 x 139 picture" in jx.last_error()
        for k in (0, 2, 3, 4):
            assert np.array_equal(pinned[k].array, refs[k]), k
        # one byte short: that image alone
        pinned = [jx.PinnedBuffer(one) for _ in datas]
        st, _ = p.wait(p.submit(datas, "float16", 3, host_ptrs=[o.ptr for o in pinned], capacities=[one, one, one, one - 1, one], crop=crops, filter=filters, mirror=mirrors, **lay),
                       check=False)
        assert st == [0, 0, 0, 1, 0] and "too small" in jx.last_error()
        for k in (0, 1, 2, 4):
            assert np.array_equal(pinned[k].array, refs[k]), k
        # resampled, plain, resampled: nothing of the resample stays behind in the slots
        refs_u8 = [batch(d, "uint8") for d in datas]
        a = [jx.PinnedBuffer(one) for _ in datas]
        b = [jx.PinnedBuffer(r.size) for r in refs_u8]
        c = [jx.PinnedBuffer(one) for _ in datas]
        t1 = p.submit(datas, "float16", 3, host_ptrs=[o.ptr for o in a], capacities=[one] * n, crop=crops, filter=filters, mirror=mirrors, **lay)
        t2 = p.submit(datas, "uint8", 3, host_ptrs=[o.ptr for o in b], capacities=[r.size for r in refs_u8])
        t3 = p.submit(datas, "float16", 3, host_ptrs=[o.ptr for o in c], capacities=[one] * n, crop=crops, filter=filters, mirror=mirrors, **lay)
        assert p.wait(t1)[0] == [0] * n and p.wait(t2)[0] == [0] * n and p.wait(t3)[0] == [0] * n
        for o, r in zip(a + b + c, refs + refs_u8 + refs):
            assert np.array_equal(o.array, r)
        # refused submissions: a filter above 1, a sequence of the wrong length, differing targets and a NULL table through the C call
        with pytest.raises(jx.DecodeError, match="filter 2 is not known"):
            p.submit(datas, "uint8", 3, host_ptrs=[o.ptr for o in b], resize=(48, 32), filter=2)
        with pytest.raises(jx.DecodeError, match="image 3: .*filter 2 is not known"):
            p.submit(datas, "uint8", 3, host_ptrs=[o.ptr for o in b], resize=(48, 32), filter=[0, 1, 0, 2, 1])
        with pytest.raises(ValueError, match="needs 5 entries"):
            p.submit(datas, "uint8", 3, host_ptrs=[o.ptr for o in b], resize=(48, 32), mirror=[True, False])
        L = jx.libjxl()
        ptrs = (C.c_char_p * n)(*datas)
        lens = (C.c_size_t * n)(*[len(d) for d in datas])
        host = (C.c_void_p * n)(*[o.ptr for o in a])
        fmt = jx.JxlPixelFormat(3, jx._PIXEL_TYPES["uint8"][0], jx.JXL_LITTLE_ENDIAN, 0)
        each = (jx.JxlHipOutputResample * n)(*[jx.JxlHipOutputResample(48, 32 if k != 2 else 33, 0, 0, 0, 0, 1, 0) for k in range(n)])
        assert L.JxlHipPipelineSubmitResampled(p._h, ptrs, lens, n, C.byref(fmt), None, host, None, 1, None, each) == -1
        assert "image 2 asks for 48 x 33, image 0 for 48 x 32: one target size per job" in jx.last_error()
        assert L.JxlHipPipelineSubmitResampled(p._h, ptrs, lens, n, C.byref(fmt), None, host, None, 1, None, None) == -1
        assert "no JxlHipOutputResample given" in jx.last_error()
        # ... and the pipeline still works
        pinned = jx.PinnedBuffer(n * one)
        st, _ = p.wait(p.submit(datas, "float16", 3, host_ptrs=[pinned.ptr + k * one for k in range(n)], capacities=[one] * n, crop=crops, filter=filters, mirror=mirrors, **lay))
        assert st == [0] * n and np.array_equal(pinned.array, np.concatenate(refs))
    finally:
        p.close()


# ---- 5. one launch pair per group ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_launch_pair_per_group(jx):
    """A batch of 18 three-channel images of mixed source and target sizes — the 2056 x 24 frame and the 67 x 41 one in one group, so that blocks of the grid lie beyond
    an image's extents both ways —, two RGBA images and one image without a resize: every output is that image decoded alone, byte for byte over the whole destination,
    and the decode took 4 resize launches (a pair for the three-slot group, a pair for the four-slot one).  With resize_group_max = 3, seven three-channel images take
    6 launches (groups of 3, 3 and 1) and give the same bytes."""
    names = ["plain_2056x24", "fused_rgba_odd", "fused_rgb_odd", "fused_rgb_three_groups", "fused_rgb_w4", "modular_rgba8"]
    targets = [dict(resize=(9, 5), filter="bicubic"), dict(resize=(130, 70)), dict(resize=(48, 32), mirror=True), dict(resize=(300, 7), filter="bicubic", mirror=True),
               dict(resize=(1, 1)), dict(resize=(33, 97), crop=(3, 2, 60, 20), filter="bicubic")]
    three = [(names[k % 6], dict(dtype=("uint8", "float32", "float16")[k % 3], num_channels=3, endianness=jx.JXL_LITTLE_ENDIAN, **targets[(k + k // 6) % 6])) for k in range(18)]
    assert {(nm, sp["resize"]) for nm, sp in three} >= {("plain_2056x24", (9, 5)), ("fused_rgba_odd", (130, 70)), ("fused_rgba_odd", (48, 32)), ("plain_2056x24", (130, 70))}
    four = [("modular_rgba8", F32(jx, 4, resize=(65, 33), filter="bicubic", mirror=True)), ("fused_rgba_odd", dict(dtype="uint8", num_channels=4, resize=(7, 50), planar=True))]
    plain = [("fused_rgb_odd", dict(dtype="uint8", num_channels=3))]
    alone = {}

    def decoded_alone(nm, sp):
        key = (nm, repr(sorted(sp.items())))
        if key not in alone:
            res, launches = decode_items(jx, [(_stream_of(nm), sp)])
            assert launches == (2 if sp.get("resize") else 0)
            alone[key] = res[0]
        return alone[key]

    def check(items, want_launches, options=()):
        res, launches = decode_items(jx, [(_stream_of(nm), sp) for nm, sp in items], options=options)
        for (nm, sp), (d, m, dims) in zip(items, res):
            d0, m0, dims0 = decoded_alone(nm, sp)
            assert m == m0 and dims == dims0
            assert_dest(d, d0, (nm, sp))
            assert d[FRONT:FRONT + m].std() > 0 or dims == (1, 1)
        assert launches == want_launches, (launches, want_launches)
    # (interleaved with each other: the table is sorted by slot count, whatever the order of the images)
    check(three[:5] + four[:1] + three[5:11] + plain + three[11:] + four[1:], 4)
    check(three[:7], 6, options=(("resize_group_max", 3),))
    check(three[:7], 2)
    check(plain, 0)


# ---- 6. nothing stays behind --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_resample_does_not_outlive_its_output(jx):
    """The same BatchDecoder, reset after a mirrored cubic decode, decodes without a resize, and with the ...Resized call, what fresh decoders decode."""
    import torch
    data = stream("fused_rgba_w4")[0]
    dst = torch.zeros(200 * 136 * 16, dtype=torch.uint8, device="cuda:0")
    runs = (dict(resize=(48, 32), crop=(10, 20, 150, 100), filter="bicubic", mirror=True), dict(), dict(resize=(48, 32), crop=(10, 20, 150, 100)))
    b = jx.BatchDecoder(0)
    outs, fresh = [], []
    for kw in runs:
        b.reset()
        b.add(data, "float32", 4, device_ptr=dst.data_ptr(), **kw)
        b.prepare(); b.decode(); b.finish()
        outs.append(b.output(0).copy())
    for kw in runs:
        f = jx.BatchDecoder(0)
        f.add(data, "float32", 4, device_ptr=dst.data_ptr(), **kw)
        f.prepare(); f.decode(); f.finish()
        fresh.append(f.output(0).copy())
    assert [o.size for o in outs] == [48 * 32 * 4, 200 * 136 * 4, 48 * 32 * 4]
    for o, f in zip(outs, fresh):
        assert np.array_equal(o.view(np.uint32), f.view(np.uint32))
    assert not np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))
    tri = outs[2].reshape(32, 48, 4)
    assert not np.array_equal(outs[0].reshape(32, 48, 4)[:, ::-1], tri)              # (cubic, not the triangle filter flipped)
