"""The integer resample of libjpeg-exact outputs (include/jxl_hip.h JxlHipBatchSetOutputJpegResampled; BatchDecoder.add(..., resize_u8=True), Pipeline.submit(...,
jpeg_pixels=True, resize_u8=True); csrc/kernels_features.hip ResizeU8Kernel): Pillow's 8-bit resize over the u8 picture libjpeg gives.  The yardstick is Pillow itself,
im.crop(box).resize(size, BILINEAR | BICUBIC) on the original JPEG file; every comparison is np.array_equal.

`restate_u8` is the rule in numpy int64 / Python float (IEEE double), importing nothing from the product or oracle/.  Per axis, n_in -> n_out, kernel k of radius r
(triangle: k(x) = max(0, 1 - |x|), r = 1; cubic, a = -0.5: ((a + 2)|x| - (a + 3))|x|^2 + 1 below 1, a(((|x| - 5)|x| + 8)|x| - 4) below 2, r = 2):
  scale = n_in / n_out, s = max(scale, 1); target i is centred at c = scale x (i + 0.5) and takes the source samples j of
  [max(0, int(c - r s + 0.5)), min(n_in, int(c + r s + 0.5))) with w_j = k((j - c + 0.5) / s) over their sum;
  kk_j = int(w_j x 2^22 + 0.5) for w_j >= 0, int(w_j x 2^22 - 0.5) below (int truncates towards zero), not renormalised;
  sample = clamp((2^21 + sum_j p_j x kk_j) >> 22, 0, 255), the shift arithmetic.
The horizontal pass runs first and gives u8, the vertical pass runs over that: cubic overshoot is cut twice.  test_restatement_equals_pillow pins it against Pillow without
a device.  A finished value k is stored as the libjpeg-exact decode stores a sample (test_jpeg_exact_pixels.expected_dest: u8 k, u16 257 k, floats float32(k) x
float32(1 / 255) through scale / bias)."""
import functools
import inspect
import io
import os

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_tools as J
import synth_lib as S
from conftest import ROOT
from test_jpeg_exact_pixels import EXTRA, FILL, FRONT, REFUSAL, expected_dest, float_decode, make_jpeg

FILTERS = ("bilinear", "bicubic")
U8_REFUSAL = "unsupported: integer resample"


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


def cdiv(a, b):
    return -(-a // b)


# ---- the definition --------------------------------------------------------------------------------------------------------------------------
def _kernel(name, x):
    x = abs(x)
    if name == "bilinear":
        return max(0.0, 1.0 - x)
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return a * (((x - 5.0) * x + 8.0) * x - 4.0)
    return 0.0


@functools.lru_cache(maxsize=None)
def axis_u8(n_in, n_out, name):
    """-> per target sample (first source sample, int64 weights kk)"""
    r = 1.0 if name == "bilinear" else 2.0
    scale = n_in / n_out
    s = max(scale, 1.0)
    out = []
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo, hi = max(0, int(c - r * s + 0.5)), min(n_in, int(c + r * s + 0.5))
        w = [_kernel(name, (j - c + 0.5) / s) for j in range(lo, hi)]
        total = 0.0
        for v in w:
            total += v
        kk = []
        for v in w:
            v = v / total
            kk.append(int(v * 4194304.0 + 0.5) if v >= 0 else int(v * 4194304.0 - 0.5))
        out.append((lo, np.asarray(kk, np.int64)))
    return out


def _pass_u8(img, n_out, name, stats, key):
    """resamples axis 1 of the (rows, n_in, channels) u8 array"""
    taps = axis_u8(img.shape[1], n_out, name)
    src = img.astype(np.int64)
    out = np.empty((img.shape[0], n_out, img.shape[2]), np.int64)
    for i, (lo, kk) in enumerate(taps):
        acc = (src[:, lo:lo + len(kk), :] * kk[None, :, None]).sum(axis=1)
        assert int(np.abs(src[:, lo:lo + len(kk), :] * kk[None, :, None]).sum(axis=1).max(initial=0)) < 2 ** 31 - 2 ** 21     # (the sum fits int32 whatever its order)
        out[:, i, :] = (acc + (1 << 21)) >> 22
    if stats is not None:
        stats[key] = stats.get(key, 0) + int(((out < 0) | (out > 255)).sum())
        stats["max_taps"] = max(stats.get("max_taps", 0), max(len(kk) for _, kk in taps))
    return np.clip(out, 0, 255).astype(np.uint8)


def restate_u8(img, size, name, crop=None, stats=None):
    """(h, w) or (h, w, c) u8, target (width, height), crop (x0, y0, w, h) -> the resampled u8 picture"""
    grey = img.ndim == 2
    a = img[:, :, None] if grey else img
    if crop is not None:
        x0, y0, cw, ch = crop
        a = a[y0:y0 + ch, x0:x0 + cw]
    h = _pass_u8(a, size[0], name, stats, "clamped_h")
    v = _pass_u8(np.ascontiguousarray(h.transpose(1, 0, 2)), size[1], name, stats, "clamped_v").transpose(1, 0, 2)
    return np.ascontiguousarray(v[:, :, 0] if grey else v)


def pil_filter(name):
    from PIL import Image
    return {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[name]


def pillow_resize(im, size, name, crop=None):
    """im: a PIL image (or an array) -> np.asarray(im.crop(box).resize(size, filter))"""
    from PIL import Image
    if isinstance(im, np.ndarray):
        im = Image.fromarray(im)
    if crop is not None:
        x0, y0, cw, ch = crop
        im = im.crop((x0, y0, x0 + cw, y0 + ch))
    return np.asarray(im.resize(tuple(size), pil_filter(name)))


def noisy(w, h, channels, seed):
    """random picture whose first min(h, 20) rows are pure 0 / 255 noise: cubic overshoot leaves [0, 255] in both passes"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    n = min(h, 20)
    img[:n] = rng.integers(0, 2, (n, w, channels), dtype=np.uint8) * 255
    return img if channels == 3 else img[:, :, 0]


GEOMETRIES = [((203, 139), (48, 32)), ((203, 139), (224, 224)), ((203, 139), (203, 50)), ((520, 72), (300, 7)), ((2056, 24), (9, 5)), ((67, 41), (67, 41)), ((67, 41), (1, 1)),
              ((5, 3), (11, 7)), ((1, 1), (1, 1))]
# crops of the 203 x 139 picture: touching the left / top, the right, the bottom edge, all of them (the whole picture), and one pixel
CROPS_203 = [(0, 0, 90, 70), (150, 20, 53, 60), (30, 100, 120, 39), (0, 0, 203, 139), (117, 64, 1, 1)]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FILTERS)
def test_restatement_equals_pillow(name):
    for channels in (3, 1):
        for k, ((w, h), size) in enumerate(GEOMETRIES):
            img = noisy(w, h, channels, seed=100 + k)
            st = {}
            got, want = restate_u8(img, size, name, stats=st), pillow_resize(img, size, name)
            assert got.shape == want.shape and got.dtype == np.uint8
            assert np.array_equal(got, want), (name, channels, (w, h), size, int((got != want).sum()))
            print(name, channels, (w, h), "->", size, st)
            if (w, h) == size:
                assert np.array_equal(got, img)                                              # the single weight is 2^22: a copy
            if name == "bicubic" and (w, h) == (203, 139) and size == (224, 224):
                assert st["clamped_h"] > 0 and st["clamped_v"] > 0, st                       # the clamp is exercised in both passes: cubic overshoot is cut twice
            if (w, h) == (2056, 24) and name == "bicubic":
                assert st["max_taps"] >= 914, st
        img = noisy(203, 139, channels, seed=7)
        for crop in CROPS_203:
            for size in ((48, 32), (64, 64)):
                got, want = restate_u8(img, size, name, crop=crop), pillow_resize(img, size, name, crop=crop)
                assert np.array_equal(got, want), (name, channels, crop, size, int((got != want).sum()))
    # crop().resize() is not resize(box=): the latter reads taps outside the box
    from PIL import Image
    img = noisy(203, 139, 3, seed=7)
    x0, y0, cw, ch = CROPS_203[1]
    boxed = np.asarray(Image.fromarray(img).resize((48, 32), pil_filter(name), box=(x0, y0, x0 + cw, y0 + ch)))
    assert not np.array_equal(boxed, pillow_resize(img, (48, 32), name, crop=CROPS_203[1]))


def test_symbols_sizes_and_refusals(jxh):
    L = jxh.libjxl()
    with open(os.path.join(ROOT, "include", "jxl_hip.h")) as f:
        header = f.read()
    for name in ("JxlHipBatchSetOutputJpegResampled", "JxlHipPipelineSubmitJpegPixelsResampled"):
        assert hasattr(L, name) and name + "(" in header, name
    assert "JXL_HIP_RESAMPLE_U8 1u" in header and jxh.JXL_HIP_RESAMPLE_U8 == 1
    for fn in (jxh.BatchDecoder.add, jxh.BatchDecoder.add_many, jxh.Pipeline.submit):
        assert inspect.signature(fn).parameters["resize_u8"].default is False
    jxl = J.transcode(make_jpeg(JC.photo(67, 41, seed=108), 2, 85))
    # sizes are those of the calls without the flag
    b = jxh.BatchDecoder(-1)                  # (a host-only batch: nothing here needs a device)
    for s in (1, 2, 8):
        for kw in (dict(dtype="uint8", num_channels=3), dict(dtype="uint16", num_channels=4, align=64), dict(dtype="float32", num_channels=3, planar=True, align=16),
                   dict(dtype="float16", num_channels=1)):
            rs = dict(resize=(21, 13), crop=(1, 2, 5, 3), filter="bicubic", mirror=True)
            i, k = b.add(jxl, jpeg_scale=s, resize_u8=True, **kw, **rs), b.add(jxl, jpeg_scale=s, **kw, **rs)
            assert b.out_size(i) == b.out_size(k) == jxh.image_out_size(jxl, jpeg_scale=s, resize=(21, 13), crop=(1, 2, 5, 3), **kw)[1]
            assert b.can_decode_jpeg_pixels(i), jxh.last_error()
    i = b.add(jxl, num_channels=3, resize=(8, 8), resize_u8=True)      # (no filter, no mirror: the triangle filter)
    assert b.out_size(i) == 8 * 8 * 3
    # flags = 0 is the ...JpegScaled call; unknown bits are refused; the flag needs a resample
    import ctypes as C
    fmt = jxh.JxlPixelFormat(3, jxh._PIXEL_TYPES["uint8"][0], jxh.Endianness.Native, 0)
    rs = jxh.JxlHipOutputResample(8, 8, 0, 0, 0, 0, 1, 0)
    h = b._h
    assert L.JxlHipBatchSetOutputJpegResampled(h, 0, C.byref(fmt), None, 1, None, C.byref(rs), 0) == 0
    assert L.JxlHipBatchSetOutputJpegResampled(h, 0, C.byref(fmt), None, 1, None, None, 0) == 0
    for flags in (2, 3, 0x80000000):
        assert L.JxlHipBatchSetOutputJpegResampled(h, 0, C.byref(fmt), None, 1, None, C.byref(rs), flags) != 0
        assert "unknown flag bits" in jxh.last_error()
    assert L.JxlHipBatchSetOutputJpegResampled(h, 0, C.byref(fmt), None, 1, None, None, 1) != 0
    assert U8_REFUSAL in jxh.last_error() and "target size" in jxh.last_error()
    assert L.JxlHipBatchSetOutputJpegResampled(h, 0, C.byref(fmt), None, 3, None, C.byref(rs), 1) != 0 and "jpeg_scale must be" in jxh.last_error()
    # the refusals of the bindings (a batch of its own each: a refused add leaves its image behind)
    with pytest.raises(jxh.DecodeError, match=U8_REFUSAL + " without a target size"):
        jxh.BatchDecoder(-1).add(jxl, num_channels=3, resize_u8=True)
    with pytest.raises(jxh.DecodeError, match=U8_REFUSAL + " together with downscale 8"):
        jxh.BatchDecoder(-1).add(jxl, num_channels=3, resize=(8, 8), downscale=8, resize_u8=True)
    xyb = S.encode_vardct(S.synthetic_image(3, 40, 24), seed=2, strategy_mix=0, epf_iters=0, gab=0)
    with pytest.raises(jxh.DecodeError) as e:
        jxh.BatchDecoder(-1).add(xyb, num_channels=3, resize=(8, 8), resize_u8=True)
    assert str(e.value).startswith(U8_REFUSAL) and REFUSAL in str(e.value), str(e.value)
    with pytest.raises(jxh.DecodeError, match="leaves the 67 x 41 picture"):
        jxh.BatchDecoder(-1).add(jxl, num_channels=3, resize=(8, 8), crop=(60, 0, 8, 8), resize_u8=True)
    # a pipeline job that is not a libjpeg-exact one: refused before the pipeline is touched, so an object without one will do where there is no device
    p = jxh.Pipeline.__new__(jxh.Pipeline)
    p._h, p._keep = None, {}
    with pytest.raises(jxh.DecodeError, match=U8_REFUSAL + " in a job that is not a libjpeg-exact one"):
        p.submit([jxl], "uint8", 3, host_ptrs=[0], resize=(8, 8), resize_u8=True)
    with pytest.raises(jxh.DecodeError, match=U8_REFUSAL + " without a target size"):
        p.submit([jxl], "uint8", 3, host_ptrs=[0], jpeg_pixels=True, resize_u8=True)
    with pytest.raises(jxh.DecodeError, match=U8_REFUSAL + " together with downscale 8"):
        p.submit([jxl], "uint8", 3, host_ptrs=[0], jpeg_pixels=True, resize=(8, 8), downscale=8, resize_u8=True)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
SAMPLINGS = (0, 1, 2, "grey")
SIZES = ((203, 139), (67, 41))


@functools.lru_cache(maxsize=None)
def files(ss):
    """(JPEG file, its transcode) per size of SIZES"""
    out = []
    for w, h in SIZES:
        d = make_jpeg(JC.photo(w, h, seed=w + h + 1), ss, 90)
        out.append((d, J.transcode(d)))
    return out


def pil_open(jpeg, scale=1, turn=None):
    """the file as a loader opens it: draft() for libjpeg's scale (asserted to be reached), the orientation as a transpose"""
    from PIL import Image
    im = Image.open(io.BytesIO(jpeg))
    W, H = im.size
    if scale != 1:
        assert W >= scale and H >= scale
        im.draft(im.mode, (max(1, W // scale), max(1, H // scale)))
        assert im.decoderconfig[0] == scale and im.size == (cdiv(W, scale), cdiv(H, scale)), (im.size, im.decoderconfig)
    assert im.mode in ("RGB", "L")
    im.load()
    return im if turn is None else im.transpose(turn)


def decode_items(jx, items, keep_orientation=False):
    """test_jpeg_exact_pixels.decode_items for items with resize_u8 (image_out_size has no such keyword: the size is the one without it)"""
    import torch
    b = jx.BatchDecoder(0)
    b.set_option("keep_orientation", 1 if keep_orientation else 0)
    bufs = []
    for data, kw in items:
        # (image_out_size applies the orientation, also to the picture it checks a crop against; the target's size does not depend on the crop)
        size = jx.image_out_size(data, **{k: v for k, v in kw.items() if k not in ("filter", "mirror", "resize_u8") + (("crop",) if keep_orientation else ())})[1]
        t = torch.full((size + EXTRA,), FILL, dtype=torch.uint8, device="cuda:0")
        i = b.add(data, device_ptr=t.data_ptr() + FRONT, **kw)
        assert b.out_size(i) == size
        bufs.append((t, size))
    errs = b.decode_jpeg_pixels()
    torch.cuda.synchronize()
    return b, errs, [(t.cpu().numpy(), n) for t, n in bufs]


def check_u8(jx, items, want, nc):
    """items decoded in ONE batch as u8 of nc channels with resize_u8; want: the pictures they must equal, guard bytes included"""
    b, errs, dests = decode_items(jx, [(d, dict(kw, dtype="uint8", num_channels=nc, resize_u8=True)) for d, kw in items])
    assert errs == [None] * len(items), errs
    for n, ((got, size), w) in enumerate(zip(dests, want)):
        assert size == w.size, (n, size, w.shape)
        assert (got[:FRONT] == FILL).all() and (got[FRONT + size:] == FILL).all(), n
        out = got[FRONT:FRONT + size].reshape(w.shape)
        assert np.array_equal(out, w), (n, items[n][1], int((out != w).sum()), int(np.abs(out.astype(int) - w).max()))
    assert b.info_value("resize_u8_images") == len(items)
    return b


def targets(w, h):
    """the issue's targets for a w x h source: widths 1 / 7 / 64 / 65 are a partial wave, a whole one and one lane more"""
    return [(48, 32), (224, 224), (1, 1), (w, h), (w, 50), (1, 9), (7, 9), (64, 9), (65, 9)]


def edge_crops(w, h):
    return [(0, 3, w // 2, h - 5), (w - 31, 2, 31, 20), (5, 0, 40, 17), (9, h - 23, w - 20, 23), (w // 2, h // 2, 1, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("ss", SAMPLINGS)
def test_equals_pillow(jx, ss):
    """the yardstick: crop().resize() of the file as Pillow's libjpeg opens it, both filters, whole and partial waves, crops at every edge, draft() scales"""
    nc = 1 if ss == "grey" else 3
    items, want = [], []
    for (w, h), (jpeg, data) in zip(SIZES, files(ss)):
        im = pil_open(jpeg)
        assert im.size == (w, h)
        for name in FILTERS:
            for size in targets(w, h):
                items.append((data, dict(resize=size, filter=name))); want.append(pillow_resize(im, size, name))
            for crop in edge_crops(w, h):
                items.append((data, dict(resize=(48, 32), crop=crop, filter=name))); want.append(pillow_resize(im, (48, 32), name, crop=crop))
            for s in (2, 8):
                ims = pil_open(jpeg, s)
                sw, sh = ims.size
                crop = (sw - sw // 2, 0, sw // 2, sh - 1)
                items.append((data, dict(resize=(48, 32), filter=name, jpeg_scale=s))); want.append(pillow_resize(ims, (48, 32), name))
                items.append((data, dict(resize=(7, 9), crop=crop, filter=name, jpeg_scale=s))); want.append(pillow_resize(ims, (7, 9), name, crop=crop))
    check_u8(jx, items, want, nc)
    if ss != 2:
        return
    # what the f32 resample of the same job gives is close to these bytes, not equal to them: this test fails without the integer pass
    jpeg, data = files(ss)[0]
    _, errs, dests = decode_items(jx, [(data, dict(dtype="uint8", num_channels=3, resize=(48, 32), filter="bicubic"))])
    f32 = dests[0][0][FRONT:FRONT + 48 * 32 * 3].reshape(32, 48, 3)
    w = pillow_resize(pil_open(jpeg), (48, 32), "bicubic")
    diff = np.abs(f32.astype(int) - w)
    print("f32 resample vs Pillow: differing bytes", int((diff != 0).sum()), "largest", int(diff.max()))
    assert errs == [None] and (diff != 0).any()


@pytest.mark.gpu
def test_long_filters_once_each(jx):
    """520 x 72 -> 300 x 7 and a 2056 x 24 file -> 9 x 5 (914 cubic taps per target sample)"""
    a, c = make_jpeg(noisy(520, 72, 3, seed=3), 2, 95), make_jpeg(noisy(2056, 24, 3, seed=4), 0, 95)
    items = [(J.transcode(a), dict(resize=(300, 7), filter="bicubic")), (J.transcode(a), dict(resize=(300, 7), filter="bilinear")),
             (J.transcode(c), dict(resize=(9, 5), filter="bicubic")), (J.transcode(c), dict(resize=(9, 5), filter="bilinear"))]
    want = [pillow_resize(pil_open(a), (300, 7), "bicubic"), pillow_resize(pil_open(a), (300, 7), "bilinear"),
            pillow_resize(pil_open(c), (9, 5), "bicubic"), pillow_resize(pil_open(c), (9, 5), "bilinear")]
    assert max(len(kk) for _, kk in axis_u8(2056, 9, "bicubic")) >= 914
    check_u8(jx, items, want, 3)


@pytest.mark.gpu
def test_formats_follow_from_the_u8_result(jx):
    jpeg, data = files(1)[1]                                                               # 67 x 41, 4:2:2
    LE, BE = jx.JXL_LITTLE_ENDIAN, jx.JXL_BIG_ENDIAN
    rs = dict(resize=(21, 13), crop=(3, 2, 60, 37), filter="bicubic")
    pic = pillow_resize(pil_open(jpeg), (21, 13), "bicubic", crop=rs["crop"])
    pic.setflags(write=False)
    SC, BI = [2.0, 0.5, 4.0, 1.0], [-1.0, 0.25, -0.5, 0.0]
    specs = []
    for dtype, end in (("uint8", LE), ("uint16", LE), ("uint16", BE), ("float16", LE), ("float32", LE), ("float32", BE)):
        for nc in (3, 4):
            for align in (0, 64):                                                          # (21 pixels: every row of every type is padded at 64)
                bps = {"uint8": 1, "uint16": 2, "float16": 2, "float32": 4}[dtype]
                row = 21 * bps
                tight = (cdiv(row, align) * align if align else row) * 13
                for lay in (dict(), dict(planar=True), dict(planar=True, plane_stride=tight + 52 * bps)):
                    sp = dict(dtype=dtype, num_channels=nc, endianness=end, align=align, **lay)
                    specs.append(sp)
                    if dtype.startswith("float"):
                        specs.append(dict(sp, scale=SC, bias=BI))
    b, errs, dests = decode_items(jx, [(data, dict(sp, resize_u8=True, **rs)) for sp in specs])
    assert errs == [None] * len(specs), errs
    for n, ((got, size), sp) in enumerate(zip(dests, specs)):
        exp = expected_dest(jx, pic, size, **sp)                                           # guard bytes, row padding and plane gaps hold the fill value
        assert np.array_equal(got, exp), (n, sp, int((got != exp).sum()))
    assert b.info_value("resize_u8_images") == len(specs)
    # one and two channels of a colour file (G; G and alpha), and of a grey one
    gj, gd = files("grey")[1]
    gpic = pillow_resize(pil_open(gj), (21, 13), "bicubic", crop=rs["crop"])
    few = [(data, pic, dict(dtype="uint8", num_channels=1)), (data, pic, dict(dtype="uint16", num_channels=2, endianness=LE)),
           (gd, gpic, dict(dtype="uint8", num_channels=3)), (gd, gpic, dict(dtype="float32", num_channels=2, endianness=LE, planar=True)), (gd, gpic, dict(dtype="uint8", num_channels=4))]
    _, errs, dests = decode_items(jx, [(d, dict(sp, resize_u8=True, **rs)) for d, _, sp in few])
    assert errs == [None] * len(few), errs
    for (got, size), (_, k, sp) in zip(dests, few):
        assert np.array_equal(got, expected_dest(jx, k, size, **sp)), sp


@pytest.mark.gpu
def test_mirror_and_orientation(jx):
    from PIL import Image
    jpeg, data = files(2)[0]                                                               # 203 x 139
    S.set_orientation(6)
    try:
        turned = J.transcode(jpeg)
    finally:
        S.set_orientation(1)
    upright, rotated = pil_open(jpeg), pil_open(jpeg, turn=Image.ROTATE_270)               # orientation 6: the stored picture turned 90 degrees clockwise
    assert rotated.size == (139, 203)
    crop = (100, 9, 39, 150)
    for name in FILTERS:
        plain = pillow_resize(upright, (48, 32), name, crop=(20, 10, 150, 100))
        items = [(data, dict(resize=(48, 32), crop=(20, 10, 150, 100), filter=name)), (data, dict(resize=(48, 32), crop=(20, 10, 150, 100), filter=name, mirror=True)),
                 (turned, dict(resize=(48, 32), filter=name)), (turned, dict(resize=(32, 48), crop=crop, filter=name, mirror=True)),
                 (turned, dict(resize=(48, 32), filter=name, jpeg_scale=2))]
        want = [plain, np.ascontiguousarray(plain[:, ::-1]), pillow_resize(rotated, (48, 32), name),
                np.ascontiguousarray(pillow_resize(rotated, (32, 48), name, crop=crop)[:, ::-1]),
                pillow_resize(pil_open(jpeg, 2, turn=Image.ROTATE_270), (48, 32), name)]
        check_u8(jx, items, want, 3)
        # keep_orientation: the picture as stored
        b, errs, dests = decode_items(jx, [(turned, dict(dtype="uint8", num_channels=3, resize=(48, 32), crop=(20, 10, 150, 100), filter=name, resize_u8=True))], keep_orientation=True)
        assert errs == [None] and np.array_equal(dests[0][0][FRONT:FRONT + plain.size].reshape(plain.shape), plain)


def small_pipeline(jx, **kw):
    opts = dict(jobs_in_flight=3, lf_streams=2, hf_streams=1, prepare_threads=1, parse_threads=2)
    opts.update(kw)
    return jx.Pipeline(0, **opts)


def xyb_stream(w=40, h=24, seed=3):
    return S.encode_vardct(S.synthetic_image(seed, w, h), seed=2, strategy_mix=0, epf_iters=0, gab=0)


@pytest.mark.gpu
def test_jobs_of_a_pipeline(jx):
    import torch
    jpegs = [make_jpeg(JC.photo(90, 70, seed=1), "grey", 85), make_jpeg(JC.photo(130, 77, seed=2), 0, 90), make_jpeg(JC.photo(101, 64, seed=3), 1, 80),
             make_jpeg(JC.photo(203, 139, seed=4), 2, 75), make_jpeg(JC.photo(67, 41, seed=5), 2, 95)]
    datas = [J.transcode(d) for d in jpegs]
    n = len(datas)
    crops = [(0, 0, 60, 50), None, (50, 10, 51, 54), (3, 100, 200, 39), (66, 40, 1, 1)]
    filters = ["bicubic", "bilinear", "bicubic", "bilinear", "bicubic"]
    mirrors = [False, True, True, False, True]
    lay = dict(planar=True, resize=(48, 32))
    b, errs, dests = decode_items(jx, [(d, dict(dtype="uint8", num_channels=3, crop=crops[k], filter=filters[k], mirror=mirrors[k], resize_u8=True, **lay)) for k, d in enumerate(datas)])
    assert errs == [None] * n, errs
    one = 3 * 32 * 48
    refs = [d[FRONT:FRONT + m].copy() for d, m in dests]
    assert [r.size for r in refs] == [one] * n
    for k in range(n):                                                                     # (the batch result is Pillow's: planes of the flipped crop().resize())
        w = pillow_resize(pil_open(jpegs[k]), (48, 32), filters[k], crop=crops[k])
        w = np.stack([w] * 3, -1) if w.ndim == 2 else w
        w = w[:, ::-1] if mirrors[k] else w
        assert np.array_equal(refs[k].reshape(3, 32, 48), w.transpose(2, 0, 1)), k
    kw = dict(jpeg_pixels=True, resize_u8=True, crop=crops, filter=filters, mirror=mirrors, **lay)
    f32_refs = [d[FRONT:FRONT + m].copy() for d, m in
                decode_items(jx, [(d, dict(dtype="uint8", num_channels=3, crop=crops[k], filter=filters[k], mirror=mirrors[k], **lay)) for k, d in enumerate(datas)])[2]]
    assert any((a != c).any() for a, c in zip(refs, f32_refs))
    fresh = float_decode(jx.BatchDecoder(), datas)
    p = small_pipeline(jx)
    try:
        out = torch.full((n, 3, 32, 48), 7, dtype=torch.uint8, device="cuda:0")
        st, _ = p.wait(p.submit(datas, "uint8", 3, device_ptrs=[out[k].data_ptr() for k in range(n)], capacities=[one] * n, **kw))
        torch.cuda.synchronize()
        assert st == [0] * n
        assert np.array_equal(out.cpu().numpy().reshape(-1), np.concatenate(refs))
        assert p.info("jpeg_pixel_images") == n and p.info("resize_u8_images") == n
        pinned = jx.PinnedBuffer(n * one)
        st, _ = p.wait(p.submit(datas, "uint8", 3, host_ptrs=[pinned.ptr + k * one for k in range(n)], capacities=[one] * n, **kw))
        assert st == [0] * n and np.array_equal(pinned.array, np.concatenate(refs))
        # an ineligible image and a capacity one byte short fail alone
        mixed, caps = [datas[3], xyb_stream(), datas[4], datas[1]], [one, one, one - 1, one]
        bufs = [jx.PinnedBuffer(one) for _ in mixed]
        for x in bufs:
            x.array[:] = FILL
        st, _ = p.wait(p.submit(mixed, "uint8", 3, host_ptrs=[x.ptr for x in bufs], capacities=caps, jpeg_pixels=True, resize_u8=True, filter="bilinear", **lay), check=False)
        assert st == [0, 1, 1, 0] and jx.last_error().startswith("image 1: " + U8_REFUSAL) and REFUSAL in jx.last_error(), (st, jx.last_error())
        for k, src in ((0, 3), (3, 1)):
            w = pillow_resize(pil_open(jpegs[src]), (48, 32), "bilinear")
            assert np.array_equal(np.array(bufs[k].array).reshape(3, 32, 48), w.transpose(2, 0, 1)), k
        assert (np.array(bufs[1].array) == FILL).all() and (np.array(bufs[2].array) == FILL).all()
        # resize_u8, f32-resampled and plain jobs alternate through one pipeline, submitted before any of them is collected
        sizes = [jx.image_out_size(d, "uint8", 3)[1] for d in datas]
        kinds = ["u8", "f32", "plain", "u8", "plain", "f32", "u8"]
        tickets = []
        for kind in kinds:
            m = sizes if kind == "plain" else [one] * n
            bufs = [jx.PinnedBuffer(x) for x in m]
            args = dict(kw) if kind == "u8" else dict(kw, resize_u8=False) if kind == "f32" else {}
            tickets.append((p.submit(datas, "uint8", 3, host_ptrs=[x.ptr for x in bufs], capacities=m, **args), bufs))
        for kind, (t, bufs) in zip(kinds, tickets):
            st, _ = p.wait(t)
            assert st == [0] * n
            for k in range(n):
                ref = refs[k] if kind == "u8" else f32_refs[k] if kind == "f32" else fresh[k].reshape(-1)
                assert np.array_equal(np.array(bufs[k].array), ref), (kind, k)
    finally:
        p.close()
    # a plain decode after a resize_u8 one from the same reset BatchDecoder is a fresh decode
    b.reset()
    for got, w in zip(float_decode(b, datas), fresh):
        assert np.array_equal(got, w)


@pytest.mark.gpu
def test_decode_fails_an_integer_resample_alone(jx):
    """decode() writes the other images; finish() names the image whose output only the libjpeg-exact decode writes"""
    jpeg, data = files(2)[1]
    b = jx.BatchDecoder()
    b.add(data, num_channels=3)
    b.add(data, num_channels=3, resize=(21, 13), resize_u8=True)
    b.prepare(); b.decode()
    with pytest.raises(jx.DecodeError, match=U8_REFUSAL + " of image 1"):
        b.finish()
    assert np.array_equal(b.output(0), float_decode(jx.BatchDecoder(), [data])[0])
    assert b.decode_jpeg_pixels() == [None, None]
    assert np.array_equal(b.output(1).reshape(13, 21, 3), pillow_resize(pil_open(jpeg), (21, 13), "bilinear"))


@pytest.mark.gpu
def test_u8_intermediates_take_a_quarter(jx):
    """520 x 264 RGB -> 64 x 64: the f32 batch holds the source picture (520 x 264 x 3 samples) and the horizontally filtered rows (264 x 64 x 3) at four bytes a sample,
    the integer one at one byte: 3 x source + 3 x tmp less, up to the arenas' 256-byte granularity (Batch::Prepare's take_big) — far below the one source size of slack"""
    jpeg = make_jpeg(JC.photo(520, 264, seed=12), 2, 85)
    data = J.transcode(jpeg)
    src, tmp = 520 * 264 * 3, 264 * 64 * 3
    stats = []
    for u8 in (False, True):
        b = jx.BatchDecoder()
        b.add(data, num_channels=3, resize=(64, 64), filter="bicubic", resize_u8=u8)
        assert b.decode_jpeg_pixels() == [None]
        stats.append((b.device_bytes, b.info_value("resize_u8_images"), b.info_value("resize_launches")))
        if u8:
            assert np.array_equal(b.output(0).reshape(64, 64, 3), pillow_resize(pil_open(jpeg), (64, 64), "bicubic"))
    (f32_bytes, f32_images, f32_launches), (u8_bytes, u8_images, u8_launches) = stats
    print("device_bytes f32", f32_bytes, "u8", u8_bytes, "difference", f32_bytes - u8_bytes, "3 x (source + tmp)", 3 * (src + tmp))
    assert f32_bytes - u8_bytes >= 2 * src
    assert abs((f32_bytes - u8_bytes) - 3 * (src + tmp)) <= 4 * 256
    assert (f32_images, u8_images) == (0, 1) and f32_launches == u8_launches == 2


@pytest.mark.gpu
def test_one_launch_pair_per_slot_count(jx):
    """18 RGB images of mixed sizes and two 4-channel outputs in one batch: each is what it is alone, and the batch takes one launch pair per slot count"""
    shapes = [(40 + 13 * k, 24 + 7 * (k % 5)) for k in range(18)]
    jpegs = [make_jpeg(JC.photo(w, h, seed=300 + k), (0, 1, 2)[k % 3], 85) for k, (w, h) in enumerate(shapes)]
    datas = [J.transcode(d) for d in jpegs]
    items = [(d, dict(dtype="uint8", num_channels=3, resize=(48, 32), filter=FILTERS[k % 2], mirror=bool(k % 3 == 0), resize_u8=True)) for k, d in enumerate(datas)]
    items.insert(5, (datas[2], dict(dtype="uint8", num_channels=4, resize=(33, 20), filter="bicubic", resize_u8=True)))
    items.append((datas[7], dict(dtype="uint16", num_channels=4, resize=(48, 32), crop=(1, 1, 30, 20), filter="bilinear", resize_u8=True)))
    b, errs, dests = decode_items(jx, items)
    assert errs == [None] * len(items), errs
    assert b.info_value("resize_launches") == 4 and b.info_value("resize_u8_images") == len(items)
    for n, (item, (got, size)) in enumerate(zip(items, dests)):
        alone, errs, one = decode_items(jx, [item])
        assert errs == [None] and alone.info_value("resize_launches") == 2
        assert np.array_equal(got, one[0][0]), n
    # integer and f32 resamples of one batch never share a group
    mixed = [items[0], (datas[1], dict(dtype="uint8", num_channels=3, resize=(48, 32), filter="bicubic")), items[1], items[5]]
    b, errs, dests = decode_items(jx, mixed)
    assert errs == [None] * 4 and b.info_value("resize_launches") == 6 and b.info_value("resize_u8_images") == 3
    for k, src in ((0, 0), (2, 1), (3, 5)):
        assert np.array_equal(dests[k][0], decode_items(jx, [items[src]])[2][0][0])
