"""libjpeg-exact pixels of JPEG transcodes (include/jxl_hip.h JxlHipBatchDecodeJpegPixels; BatchDecoder.decode_jpeg_pixels; csrc/jpeg_pixels.hip): the samples libjpeg gives for
the original file, from the coefficients the entropy stages leave on the device.  The yardstick is a decoder this repository has no part in: Pillow's libjpeg-turbo, which
also wrote the files.  Every comparison with it is np.array_equal on u8.

`restate` is the definition in numpy int64, from the coefficients and tables tests/jpeg_tools.parse_jpeg reads out of the file; it imports nothing from oracle/ or the product:
  1. d[v][u] = coef[v * 8 + u] x q[v * 8 + u]
  2. jpeg_idct_islow (jidctint.c, CONST_BITS 13, PASS1_BITS 2): the 1-D transform over the 8 columns with DESCALE(., 11), then over the 8 rows of that with DESCALE(., 18);
     + 128, clamp to [0, 255]
  3. "fancy" chroma upsampling (jdsample.c) over the component's real extent cw x ch: h2v1 (3 s[x] + s[x -+ 1] + 1 / 2) >> 2 with out[0] = s[0], out[last] = s[cw - 1];
     h2v2 with c[x] = 3 s[y][x] + s[y -+ 1][x] (rows clamped), (3 c[x] + c[x -+ 1] + 8 / 7) >> 4, first column (4 c[0] + 8) >> 4, last (4 c[cw - 1] + 7) >> 4; cw <= 2: plain
     replication in both modes
  4. jdcolor.c: r = y + ((91881 cr + 32768) >> 16), g = y + ((-22554 cb - 46802 cr + 32768) >> 16), b = y + ((116130 cb + 32768) >> 16), cb and cr less 128, clamped
test_restatement_equals_pillow pins it (and with it the rules as written in include/jxl_hip.h) against Pillow without a device; the resized-output test uses it for its
f32 source picture.  Integer sample k enters the write stage as float32(k) x float32(1 / 255): u8 gives k, u16 257 k, the float types that product, the rest follows from
the layout — expected_dest below builds the whole destination, guard bytes included.

The bound of the resized outputs is the derived one of test_resample_jobs.py: (taps_x + taps_y + 8) x 2^-24 x L_x x L_y x max|v| (every rounding of the two passes is
relative 2^-24 on a partial sum of at most L x max|v|); the filter is restated here."""
import functools
import io
import os
import struct

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_tools as J
import synth_lib as S
from conftest import FIXTURES, ROOT, fixture_bytes

FILL, FRONT, EXTRA = 0xA5, 64, 192
REFUSAL = "unsupported: libjpeg-exact decode of "


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


def pillow(jpeg):
    """(h, w, 3) u8, or (h, w) for a grey file (mode L)"""
    from PIL import Image
    im = Image.open(io.BytesIO(jpeg))
    assert im.mode in ("RGB", "L"), im.mode
    return np.asarray(im)


# ---- the definition --------------------------------------------------------------------------------------------------------------------------
def _idct_1d(i, shift):
    i0, i1, i2, i3, i4, i5, i6, i7 = i
    z1 = (i2 + i6) * 4433
    t2 = z1 - i6 * 15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) * 8192
    t1 = (i0 - i4) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    outs = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return [(o + (1 << (shift - 1))) >> shift for o in outs]


def _component_plane(coef, q, stats):
    """(grid rows, grid columns, 64) int16 coefficients, natural order -> u8 samples of the whole padded grid, as int64"""
    gh, gw = coef.shape[:2]
    d = coef.astype(np.int64).reshape(gh, gw, 8, 8) * np.asarray(q, np.int64).reshape(8, 8)
    cols = np.stack(_idct_1d([d[:, :, r, :] for r in range(8)], 11), axis=2)
    rows = np.stack(_idct_1d([cols[:, :, :, u] for u in range(8)], 18), axis=3) + 128
    stats["idct_min"] = min(stats.get("idct_min", 1 << 40), int(rows.min()))
    stats["idct_max"] = max(stats.get("idct_max", -(1 << 40)), int(rows.max()))
    return np.clip(rows, 0, 255).transpose(0, 2, 1, 3).reshape(gh * 8, gw * 8)


def _columns(c, r_even, r_odd, shift, edge):
    """one row filter of rule 3 over c (rows x cw, cw > 2): -> rows x 2 cw"""
    left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    even = (3 * c + left + r_even) >> shift
    odd = (3 * c + right + r_odd) >> shift
    even[:, 0], odd[:, -1] = edge(c[:, 0], r_even), edge(c[:, -1], r_odd)
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
    out[:, 0::2], out[:, 1::2] = even, odd
    return out


def _upsample(s, cw, ch, hx, vx):
    s = s[:ch, :cw]
    if hx == 1 and vx == 1:
        return s
    assert hx == 2 and vx in (1, 2), (hx, vx)
    if cw <= 2:
        return np.repeat(np.repeat(s, 2, axis=1), vx, axis=0)
    if vx == 1:
        return _columns(s, 1, 2, 2, lambda v, r: v)
    out = np.empty((2 * ch, 2 * cw), np.int64)
    for phase, step in ((0, -1), (1, 1)):
        nb = s[np.clip(np.arange(ch) + step, 0, ch - 1)]
        out[phase::2] = _columns(3 * s + nb, 8, 7, 4, lambda v, r: (4 * v + r) >> 4)
    return out


def restate(jpeg, stats=None):
    stats = {} if stats is None else stats
    j = J.parse_jpeg(jpeg)
    W, H = j.width, j.height
    hmax, vmax = max(c["h"] for c in j.components), max(c["v"] for c in j.components)
    full = []
    for c, comp in enumerate(j.components):
        plane = _component_plane(j.coef[c], j.qt[comp["tq"]], stats)
        cw, ch = -(-W * comp["h"] // hmax), -(-H * comp["v"] // vmax)
        full.append(_upsample(plane, cw, ch, hmax // comp["h"], vmax // comp["v"])[:H, :W])
    if len(full) == 1:
        return full[0].astype(np.uint8)
    y, cb, cr = full[0], full[1] - 128, full[2] - 128
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], axis=-1)
    stats["rgb_min"], stats["rgb_max"] = int(rgb.min()), int(rgb.max())
    return np.clip(rgb, 0, 255).astype(np.uint8)


# ---- files -----------------------------------------------------------------------------------------------------------------------------------
SAMPLINGS = (0, 1, 2, "grey")
SHAPES = [(1, 1), (8, 8), (16, 16), (17, 9), (5, 5), (6, 3), (3, 5), (4, 17), (2, 17), (1, 5), (67, 41), (21, 13), (300, 280), (520, 264)]


def make_jpeg(img, ss, quality, **kw):
    from PIL import Image
    buf = io.BytesIO()
    if ss == "grey":
        Image.fromarray(np.ascontiguousarray(img[:, :, 0])).save(buf, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=ss, **kw)
    return buf.getvalue()


def saturated(w=48, h=40):
    """flat black and white patches, the six saturated colours and a black / white checkerboard over a photo: samples at both ends of both clamps"""
    img = JC.photo(w, h, seed=5)
    img[:16, :16], img[:16, 16:32] = 0, 255
    for k, colour in enumerate([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]):
        img[16:28, 8 * k:8 * k + 8] = colour
    yy, xx = np.mgrid[0:12, 0:w]
    img[28:40] = (((xx // 3 + yy // 3) & 1) * 255)[:, :, None]
    return img


@functools.lru_cache(maxsize=None)
def shape_files(ss):
    """(name, file) per shape of the issue's list, at sampling ss"""
    out = [("%dx%d" % (w, h), make_jpeg(JC.photo(w, h, seed=w + h), ss, 85)) for w, h in SHAPES]
    out += [("saturated q5", make_jpeg(saturated(), ss, 5)), ("saturated q100", make_jpeg(saturated(), ss, 100))]
    out += [("progressive", make_jpeg(JC.photo(40, 24, seed=9), ss, 85, progressive=True)), ("restart", make_jpeg(JC.photo(40, 24, seed=9), ss, 85, restart_marker_blocks=2))]
    return out


def check_shape_properties(ss):
    """what the issue's list says about each shape, asserted on the files themselves"""
    files = dict(shape_files(ss))
    hx, vx = {0: (1, 1), 1: (2, 1), 2: (2, 2), "grey": (1, 1)}[ss]
    for name, d in files.items():
        j = J.parse_jpeg(d)
        assert len(j.components) == (1 if ss == "grey" else 3)
        assert (j.components[0]["h"], j.components[0]["v"]) == ((1, 1) if ss == "grey" else (hx, vx)) and all((c["h"], c["v"]) == (1, 1) for c in j.components[1:])
    grid = lambda name: J.parse_jpeg(files[name]).coef[0].shape[:2]
    cw = lambda w: -(-w // hx)
    assert grid("8x8") == (vx, hx) and grid("1x1") == (vx, hx)                      # one block (one MCU)
    assert grid("16x16") == (2, 2)                                                  # one MCU of 4:2:0, four blocks otherwise
    assert 17 % (8 * hx) and 9 % (8 * vx)                                           # partial MCUs both ways
    if hx == 2:
        assert cw(5) == 3 and cw(6) == 3                                            # the narrowest interpolated plane
        assert cw(3) == 2 and cw(4) == 2 and cw(2) == 1 and cw(1) == 1              # replication
        assert (cw(67), -(-41 // vx)) == (34, 21 if vx == 2 else 41) and grid("67x41")[1] * 8 // hx > 34      # padded chroma columns behind the real extent
        assert cw(300) > 128 and cw(520) > 256                                      # chroma taps across the 256-pixel group border(s)
    assert J.parse_jpeg(files["progressive"]).sof == 0xC2 and J.parse_jpeg(files["restart"]).restart_interval == 2
    for name, q in (("saturated q5", 5), ("saturated q100", 100)):
        st = {}
        out = restate(files[name], st)
        print(ss, name, st, "output range", int(out.min()), int(out.max()))
        assert out.min() == 0 and out.max() == 255                                  # both ends of the output range are reached ...
        assert st["idct_min"] < 0 and st["idct_max"] > 255                          # ... and both clamps cut at both ends: by hundreds of levels at quality 5, by one or two at 100
        assert ss == "grey" or (st["rgb_min"] < 0 and st["rgb_max"] > 255)
        assert q == 100 or (st["idct_min"] < -100 and st["idct_max"] > 355)


def strip_boxes(data, drop=(b"jbrd",)):
    """container without the boxes of `drop`; -> (container, bare codestream)"""
    assert data[4:8] == b"JXL "
    pos, kept, cs = 0, b"", b""
    while pos < len(data):
        size, typ = struct.unpack(">I4s", data[pos:pos + 8])
        head = 8
        if size == 1:
            size, head = struct.unpack(">Q", data[pos + 8:pos + 16])[0], 16
        end = len(data) if size == 0 else pos + size
        if typ == b"jxlc":
            cs += data[pos + head:end]
        if typ == b"jxlp":
            cs += data[pos + head + 4:end]
        if typ not in drop:
            kept += data[pos:end]
        pos = end
    assert cs[:2] == b"\xff\x0a"
    return kept, cs


def transcode_440(w=16, h=16):
    """a 4:4:0 transcode (luma 1 x 2, chroma 1 x 1): Pillow writes no such file, the synthesiser takes any sampling"""
    mx, my = -(-w // 8), -(-h // 16)
    rng = np.random.default_rng(4)
    planes = [rng.integers(-3, 4, (n, 64)).astype(np.int16) for n in (mx * my, mx * my * 2, mx * my)]      # Cb, Y, Cr
    return S.jpeg_transcode_codestream(w, h, [0, 3, 0], planes, np.full((3, 64), 16, np.int32))


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_pillow():
    with open(os.path.join(FIXTURES, "sample.jpg"), "rb") as f:
        files = [("sample.jpg", f.read())]
    files += [(str(c), JC.jpeg_bytes(c)) for c in JC.CASES + JC.PROGRESSIVE]
    files += [("grey 75x52", JC.grey_jpeg_bytes(75, 52, 85)), ("grey 41x30", JC.grey_jpeg_bytes(41, 30, 70, optimize=True))]
    for ss in SAMPLINGS:
        files += [("%s %s" % (ss, name), d) for name, d in shape_files(ss)]
    for name, d in files:
        want, got = pillow(d), restate(d)
        assert got.shape == want.shape, name
        assert np.array_equal(got, want), (name, int((got != want).sum()))
    for ss in SAMPLINGS:
        check_shape_properties(ss)


def test_symbols_and_refusals(jxh):
    L = jxh.libjxl()
    with open(os.path.join(ROOT, "include", "jxl_hip.h")) as f:
        header = f.read()
    for name in ("JxlHipBatchCanDecodeJpegPixels", "JxlHipBatchDecodeJpegPixels", "JxlHipBatchJpegPixelsStatus"):
        assert hasattr(L, name) and name + "(" in header
    jpeg = make_jpeg(JC.photo(40, 24, seed=9), 2, 85)
    jxl = J.transcode(jpeg)
    sample = fixture_bytes("sample_jpg.jxl")
    no_jbrd, bare = strip_boxes(sample)
    assert b"jbrd" in sample and b"jbrd" not in no_jbrd
    xyb = S.encode_vardct(S.synthetic_image(3, 40, 24), seed=2, strategy_mix=0, epf_iters=0, gab=0)
    b = jxh.BatchDecoder(-1)             # (a host-only batch: nothing here needs a device)
    refused = [b.add(fixture_bytes("sample.jxl")), b.add(xyb), b.add(jxl, downscale=8), b.add(transcode_440())]
    taken = [b.add(sample), b.add(no_jbrd), b.add(bare), b.add(jxl), b.add(strip_boxes(jxl)[1])]
    assert not b.info(refused[1]).uses_original_profile                         # (the synthesiser's VarDCT frame is XYB)
    for i in refused:
        assert not b.can_decode_jpeg_pixels(i)
        assert jxh.last_error().startswith(REFUSAL), jxh.last_error()
    assert not b.can_decode_jpeg_pixels(refused[2]) and "downscale 8" in jxh.last_error()
    assert not b.can_decode_jpeg_pixels(refused[3]) and "chroma sampling" in jxh.last_error()
    for i in taken:
        assert b.can_decode_jpeg_pixels(i), jxh.last_error()
    assert b.can_reconstruct_jpeg(taken[0]) and not b.can_reconstruct_jpeg(taken[1]) and not b.can_reconstruct_jpeg(taken[2])      # (the reconstruction's own conditions stay)
    assert L.JxlHipBatchCanDecodeJpegPixels(b._h, 99) == 0 and "no such image" in jxh.last_error()
    assert L.JxlHipBatchJpegPixelsStatus(b._h, 0) != 0 and "has not run" in jxh.last_error()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def exact_batch(jx, jxls, channels):
    """decode_jpeg_pixels of one batch, u8 -> (batch, per-image errors, per-image (h, w, c) or (h, w) arrays)"""
    b = jx.BatchDecoder()
    for d, nc in zip(jxls, channels):
        b.add(d, num_channels=nc)
    errs = b.decode_jpeg_pixels()
    outs = []
    for i, nc in enumerate(channels):
        w, h = b.info(i).xsize, b.info(i).ysize
        outs.append(None if errs[i] else b.output(i).reshape((h, w) if nc == 1 else (h, w, nc)))
    return b, errs, outs


def assert_exact(jx, files):
    want = [pillow(d) for d in files]
    channels = [1 if w.ndim == 2 else 3 for w in want]
    b, errs, outs = exact_batch(jx, [J.transcode(d) for d in files], channels)
    assert errs == [None] * len(files), errs
    for i, (got, w) in enumerate(zip(outs, want)):
        assert got.shape == w.shape and np.array_equal(got, w), (i, w.shape, int((got != w).sum()))
    assert b.info_value("jpeg_pixel_images") == len(files)
    return b


@pytest.mark.gpu
def test_every_real_file_equals_pillow(jx):
    files = [JC.jpeg_bytes(c) for c in JC.CASES + JC.PROGRESSIVE] + [JC.grey_jpeg_bytes(75, 52, 85), JC.grey_jpeg_bytes(41, 30, 70, optimize=True)]
    b = assert_exact(jx, files)
    with open(os.path.join(FIXTURES, "sample.jpg"), "rb") as f:
        sample = pillow(f.read())
    one, errs, outs = exact_batch(jx, [fixture_bytes("sample_jpg.jxl")], [1 if sample.ndim == 2 else 3])
    assert errs == [None] and np.array_equal(outs[0], sample)
    assert one.info_value("jpeg_pixel_images") == 1
    # one launch of each kernel per group of the image table, whatever the group holds: the 16 files of two channel counts take no more than one file of each would
    assert 0 < b.info_value("jpeg_pixel_launches") <= 2 * one.info_value("jpeg_pixel_launches")


@pytest.mark.gpu
@pytest.mark.parametrize("ss", SAMPLINGS)
def test_shapes(jx, ss):
    check_shape_properties(ss)
    assert_exact(jx, [d for _, d in shape_files(ss)])


def decode_items(jx, items):
    """items: (data, BatchDecoder.add keywords).  Every item is one image of ONE batch, written into a device buffer of out_size + EXTRA bytes filled with FILL, FRONT bytes
    into it -> (batch, per-image errors, per-image (whole destination as u8 array, out_size))"""
    import torch
    b = jx.BatchDecoder(0)
    bufs = []
    for data, kw in items:
        size = jx.image_out_size(data, **{k: v for k, v in kw.items() if k not in ("filter", "mirror")})[1]
        t = torch.full((size + EXTRA,), FILL, dtype=torch.uint8, device="cuda:0")
        i = b.add(data, device_ptr=t.data_ptr() + FRONT, **kw)
        assert b.out_size(i) == size
        bufs.append((t, size))
    errs = b.decode_jpeg_pixels()
    torch.cuda.synchronize()
    return b, errs, [(t.cpu().numpy(), n) for t, n in bufs]


BPS = {"uint8": 1, "uint16": 2, "float16": 2, "float32": 4}


def expected_dest(jx, k, size, dtype="uint8", num_channels=3, endianness=None, align=0, planar=False, plane_stride=0, scale=None, bias=None):
    """The whole destination (FRONT guard bytes, `size` bytes of output, the rest of EXTRA) for the oriented picture k — (h, w) grey or (h, w, 3) u8 — in that format."""
    grey = k.ndim == 2
    h, w = k.shape[:2]
    k3 = np.stack([k] * 3, -1) if grey else k
    v = k3.astype(np.float32) * np.float32(1.0 / 255)
    alpha_k, alpha_v = np.full((h, w, 1), 255, np.uint8), np.ones((h, w, 1), np.float32)
    pick = {1: [0 if grey else 1], 2: [0 if grey else 1, 3], 3: [0, 1, 2], 4: [0, 1, 2, 3]}[num_channels]
    kk, vv = np.concatenate([k3, alpha_k], -1)[:, :, pick], np.concatenate([v, alpha_v], -1)[:, :, pick]
    if scale is not None:
        # (powers of two and small dyadic offsets: the product is exact, the sum rounds once — what fmaf gives)
        vv = (vv.astype(np.float64) * np.asarray(scale, np.float64)[:num_channels] + np.asarray(bias, np.float64)[:num_channels]).astype(np.float32)
    if dtype == "uint8":
        samples = kk.astype(np.uint8)
    elif dtype == "uint16":
        samples = kk.astype(np.uint16) * np.uint16(257)
    elif dtype == "float32":
        samples = vv
    else:
        samples = vv.astype(np.float16)
    big = endianness == jx.JXL_BIG_ENDIAN
    raw = np.ascontiguousarray(samples.astype(samples.dtype.newbyteorder(">" if big else "<"))).view(np.uint8).reshape(h, w, num_channels, BPS[dtype])
    dest = np.full(FRONT + size + (EXTRA - FRONT), FILL, np.uint8)
    out = dest[FRONT:FRONT + size]
    bps = BPS[dtype]
    row = w * bps * (1 if planar else num_channels)
    stride = -(-row // align) * align if align > 1 else row
    if planar:
        ps = plane_stride or stride * h
        assert size == num_channels * ps
        for c in range(num_channels):
            for y in range(h):
                out[c * ps + y * stride:c * ps + y * stride + row] = raw[y, :, c].reshape(-1)
    else:
        assert size == stride * (h - 1) + row
        for y in range(h):
            out[y * stride:y * stride + row] = raw[y].reshape(-1)
    return dest


@pytest.mark.gpu
def test_formats_follow_from_the_integers(jx):
    colour, grey = make_jpeg(JC.photo(21, 13, seed=34), 2, 85), make_jpeg(JC.photo(21, 13, seed=34), "grey", 85)
    LE, BE = jx.JXL_LITTLE_ENDIAN, jx.JXL_BIG_ENDIAN
    SC, BI = [2.0, 0.5, 4.0, 1.0], [-1.0, 0.25, -0.5, 0.0]
    specs = [dict(dtype="uint16", num_channels=3, endianness=LE), dict(dtype="uint16", num_channels=3, endianness=BE),
             dict(dtype="float32", num_channels=3, endianness=LE), dict(dtype="float32", num_channels=3, endianness=BE),
             dict(dtype="float16", num_channels=3, endianness=LE), dict(dtype="float16", num_channels=4, endianness=BE)]
    specs += [dict(dtype="uint8", num_channels=nc) for nc in (1, 2, 3, 4)]
    specs += [dict(dtype="uint8", num_channels=3, align=32), dict(dtype="uint16", num_channels=2, endianness=LE, align=64)]                     # padded rows
    specs += [dict(dtype="uint8", num_channels=3, planar=True), dict(dtype="float32", num_channels=4, endianness=LE, planar=True, align=16, plane_stride=-64)]   # (-64: tight + 64, below)
    specs += [dict(dtype="float32", num_channels=3, endianness=LE, scale=SC, bias=BI), dict(dtype="float16", num_channels=4, endianness=LE, planar=True, scale=SC, bias=BI)]
    S.set_orientation(6)
    try:
        turned = [J.transcode(colour), J.transcode(grey)]
    finally:
        S.set_orientation(1)
    streams = [(J.transcode(colour), pillow(colour)), (J.transcode(grey), pillow(grey)),
               (turned[0], np.rot90(pillow(colour), -1)), (turned[1], np.rot90(pillow(grey), -1))]       # (orientation 6: the picture turned 90 degrees clockwise)
    items, want = [], []
    for si, (data, k) in enumerate(streams):
        for sp in (specs if si < 2 else specs[:1] + specs[6:8] + specs[12:13]):
            sp = dict(sp)
            if sp.get("plane_stride") == -64:
                row = k.shape[1] * BPS[sp["dtype"]]
                sp["plane_stride"] = -(-row // sp["align"]) * sp["align"] * k.shape[0] + 64        # a gap of 64 bytes between the planes
            items.append((data, sp)); want.append((k, sp))
    b, errs, dests = decode_items(jx, items)
    assert errs == [None] * len(items), errs
    first_turned = b.info(len(specs) * 2)            # (the header's orientation 6 is applied by the write stage: the batch reports the oriented size)
    assert (b.info(0).xsize, b.info(0).ysize) == (21, 13) and (first_turned.xsize, first_turned.ysize) == (13, 21)
    for n, ((got, size), (k, sp)) in enumerate(zip(dests, want)):
        exp = expected_dest(jx, np.ascontiguousarray(k), size, **sp)
        assert np.array_equal(got, exp), (n, sp, int((got != exp).sum()))
    # u16 is 257 k and f32 is float32(k) x float32(1 / 255), said once more without the helper
    k = pillow(colour)
    assert np.array_equal(dests[0][0][FRONT:FRONT + dests[0][1]].view("<u2").reshape(k.shape), k.astype(np.uint16) * 257)
    assert np.array_equal(dests[2][0][FRONT:FRONT + dests[2][1]].view("<f4").reshape(k.shape), k.astype(np.float32) * np.float32(1 / 255))


# ---- resized outputs: the filter of include/jxl_hip.h, restated ---------------------------------------------------------------------------------
def filter_kernel(name, x):
    x = np.abs(np.asarray(x, np.float64))
    if name == "bilinear":
        return np.maximum(0.0, 1.0 - x)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, a * (((x - 5.0) * x + 8.0) * x - 4.0), 0.0))


def axis_taps(n_in, n_out, name):
    scale = n_in / n_out
    s, r = max(scale, 1.0), {"bilinear": 1.0, "bicubic": 2.0}[name]
    taps = []
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo, hi = max(0, int(c - r * s + 0.5)), min(n_in, int(c + r * s + 0.5))
        w = filter_kernel(name, (np.arange(lo, hi) - c + 0.5) / s)
        taps.append((lo, hi, w / w.sum()))
    return taps


def resample(x, size, name):
    """(h, w, c), (ow, oh) -> ((oh, ow, c) float64, longest tap ranges, largest sums of |w|): horizontal pass, then vertical"""
    x = np.asarray(x, np.float64)
    tx, ty = axis_taps(x.shape[1], size[0], name), axis_taps(x.shape[0], size[1], name)
    tmp = np.stack([np.tensordot(w, x[:, lo:hi], axes=(0, 1)) for lo, hi, w in tx], axis=1)
    out = np.stack([np.tensordot(w, tmp[lo:hi], axes=(0, 0)) for lo, hi, w in ty], axis=0)
    return out, [max(hi - lo for lo, hi, _ in t) for t in (tx, ty)], [max(float(np.abs(w).sum()) for _, _, w in t) for t in (tx, ty)]


@pytest.mark.gpu
def test_resized_output(jx):
    jpeg = make_jpeg(JC.photo(130, 77, seed=207), 2, 95)
    data = J.transcode(jpeg)
    plain = restate(jpeg).astype(np.float32) * np.float32(1.0 / 255)             # the f32 picture the write stage leaves for the resize
    x0, y0, cw, ch = 10, 6, 100, 60
    f32 = dict(dtype="float32", num_channels=3, endianness=jx.JXL_LITTLE_ENDIAN)
    items = [(data, dict(f32, resize=(48, 32))), (data, dict(f32, resize=(48, 32), crop=(x0, y0, cw, ch), filter="bicubic", mirror=True))]
    b, errs, dests = decode_items(jx, items)
    assert errs == [None, None], errs
    for (got, size), src, name, mirror in ((dests[0], plain, "bilinear", False), (dests[1], plain[y0:y0 + ch, x0:x0 + cw], "bicubic", True)):
        assert size == 48 * 32 * 3 * 4 and (got[:FRONT] == FILL).all() and (got[FRONT + size:] == FILL).all()
        out = got[FRONT:FRONT + size].view("<f4").reshape(32, 48, 3)
        want, (tx, ty), (lx, ly) = resample(src, (48, 32), name)
        if mirror:
            want = want[:, ::-1]
        bound = (tx + ty + 8) * 2.0 ** -24 * lx * ly * float(np.abs(src).max())
        err = float(np.abs(out.astype(np.float64) - want).max())
        print(name, "taps", (tx, ty), "sum |w|", (lx, ly), "max error", err, "bound", bound)
        assert np.isfinite(out).all() and err <= bound, (name, err, bound)


@pytest.mark.gpu
def test_without_jbrd_and_bare_codestream(jx):
    jpeg = make_jpeg(JC.photo(67, 41, seed=108), 2, 85)
    full = J.transcode(jpeg)
    no_jbrd, bare = strip_boxes(full)
    assert b"jbrd" in full and b"jbrd" not in no_jbrd and bare[:2] == b"\xff\x0a"
    b, errs, outs = exact_batch(jx, [full, no_jbrd, bare], [3, 3, 3])
    assert errs == [None] * 3, errs
    assert b.can_reconstruct_jpeg(0) and not b.can_reconstruct_jpeg(1) and not b.can_reconstruct_jpeg(2)
    for got in outs:
        assert np.array_equal(got, pillow(jpeg))


def float_decode(b, datas):
    for d in datas:
        b.add(d, num_channels=3)
    b.prepare(); b.decode(); b.finish()
    return [b.output(i) for i in range(len(datas))]


@pytest.mark.gpu
def test_differs_from_the_float_path_and_leaves_it_alone(jx):
    jpeg = make_jpeg(JC.photo(203, 139, seed=342), 2, 75)
    data, want = J.transcode(jpeg), pillow(jpeg)
    fresh = float_decode(jx.BatchDecoder(), [data])[0]
    assert (fresh.reshape(want.shape) != want).any()                  # the reason the feature exists: libjxl's rendering of the transcode is not libjpeg's decode
    b = jx.BatchDecoder()
    b.add(data, num_channels=3)
    assert b.decode_jpeg_pixels() == [None]
    assert np.array_equal(b.output(0).reshape(want.shape), want)
    b.decode(); b.finish()
    assert np.array_equal(b.output(0), fresh)                         # the float path of the same batch object afterwards ...
    b.reconstruct_jpegs()
    assert b.jpeg(0) == jpeg                                          # ... the file's bytes ...
    assert b.decode_jpeg_pixels() == [None] and np.array_equal(b.output(0).reshape(want.shape), want)
    b.reset()
    assert np.array_equal(float_decode(b, [data])[0], fresh)          # ... and after reset()
    b.reset()
    b.add(data)
    b.reconstruct_jpegs()
    assert b.jpeg(0) == jpeg


@pytest.mark.gpu
def test_failures_stay_with_their_image(jx):
    good = make_jpeg(JC.photo(100, 60, seed=160), 2, 80, restart_marker_blocks=3)
    jxl = J.transcode(good)
    _, cs = strip_boxes(jxl)
    jbrd = J.build_jbrd(J.parse_jpeg(good))
    assert jxl == J.container(jbrd, cs)
    rng = np.random.default_rng(11)
    mutated = []
    for k in range(5):
        bad = bytearray(cs)
        for pos in rng.integers(len(cs) * 6 // 10, len(cs), 1 + k % 3):                      # the AC sections fill the back of the codestream
            bad[pos] ^= 1 << int(rng.integers(0, 8))
        mutated.append(J.container(jbrd, bytes(bad)))
    mutated.append(J.container(jbrd, cs[:-40]))
    xyb = S.encode_vardct(S.synthetic_image(3, 40, 24), seed=2, strategy_mix=0, epf_iters=0, gab=0)
    b = jx.BatchDecoder()
    index = []
    for d in [jxl, fixture_bytes("sample.jxl"), xyb] + mutated:
        try:
            index.append(b.add(d, num_channels=3))
        except jx.DecodeError as e:                                                         # (a stream the host parser refuses never enters the batch)
            assert str(e)
            index.append(None)
    assert index[:3] == [0, 1, 2]
    errs = b.decode_jpeg_pixels()
    want = pillow(good)
    assert errs[0] is None and np.array_equal(b.output(0).reshape(want.shape), want)
    for i in (1, 2):
        assert errs[i].startswith(REFUSAL) and not b.can_decode_jpeg_pixels(i)
    for i in index[3:]:
        if i is None:
            continue
        assert errs[i] is None or errs[i]
        assert b.output(i).size == want.size                                                # an error, or an output of the right size
    assert b.info_value("jpeg_pixel_images") == sum(1 for e in errs if e is None)
    again, errs2, outs = exact_batch(jx, [jxl], [3])
    assert errs2 == [None] and np.array_equal(outs[0], want)
