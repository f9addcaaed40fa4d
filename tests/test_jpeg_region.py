"""Crops of libjpeg-exact outputs decoded by region (include/jxl_hip.h JxlHipBatchJpegRegion; BatchDecoder.set_option("jpeg_region", 1), Pipeline.set_option): with the
option on, an output written by decode_jpeg_pixels() (or a libjpeg-exact pipeline job) that carries a crop decodes only the 256x256 groups the crop needs — HF entropy
stage, integer IDCT, colour stage — and delivers the bytes of the decode without the option.  The yardstick is Pillow on the original JPEG file,
np.asarray(Image.open(f).crop(box)) or .crop(box).resize(size, filter), after draft() for jpeg_scale and after ImageOps.exif_transpose for the orientation; every
comparison is np.array_equal over the whole destination, guard bytes included.

`region` is the rule restated in Python integers, importing nothing from the product.  For a W x H file of sampling ss at jpeg_scale s and orientation o, crop
(x0, y0, w, h) of the oriented scaled picture:
  1. the crop is mapped back through the orientation to a rectangle of the stored picture at scale s, which is ceil(W / s) x ceil(H / s);
  2. a luma block covers n x n of its pixels, n = 8 / s: luma blocks floor(first / n) .. floor(last / n) per axis;
  3. widened outwards to whole MCUs of mx x my luma blocks (4:2:2: 2 x 1, 4:2:0: 2 x 2, 4:4:4 and grey: 1 x 1);
  4. one MCU more on every side, clamped to the frame's block grid (ceil(W / 8 mx) mx by ceil(H / 8 my) my blocks);
  5. every group (32 x 32 blocks) that rectangle touches: gx0 <= gx < gx1, gy0 <= gy < gy1."""
import functools
import io

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_tools as J
import synth_lib as S
from test_jpeg_exact_pixels import EXTRA, FILL, FRONT, float_decode, make_jpeg

MCU = {0: (1, 1), 1: (2, 1), 2: (2, 2), "grey": (1, 1)}
# (width, height, sampling): 3 x 3 groups with a centre group; 2 x 2 groups, odd sizes, partial MCUs; 9 x 2 groups and two LF groups
PICTURES = {"600x520": (600, 520, 2), "301x279_422": (301, 279, 1), "301x279_444": (301, 279, 0), "301x279_grey": (301, 279, "grey"), "2100x300": (2100, 300, 2)}
CROPS = {
    "600x520": [(272, 272, 200, 200), (256, 256, 100, 100), (255, 0, 2, 520), (0, 200, 40, 90), (300, 0, 90, 30), (570, 100, 30, 200), (100, 490, 300, 30), (599, 519, 1, 1),
                (0, 0, 600, 520)],
    "2100x300": [(2000, 100, 100, 100), (2060, 0, 40, 300)],
    "301x279_422": [(200, 200, 100, 70), (296, 272, 5, 7)],
    "301x279_444": [(200, 200, 100, 70), (296, 272, 5, 7)],
    "301x279_grey": [(200, 200, 100, 70), (296, 272, 5, 7)],
}


def cdiv(a, b):
    return -(-a // b)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------------
def stored_rect(w, h, o, crop):
    """crop (x0, y0, cw, ch) of the picture oriented by o -> inclusive (x0, x1, y0, y1) of the stored w x h picture"""
    X0, Y0, X1, Y1 = crop[0], crop[1], crop[0] + crop[2] - 1, crop[1] + crop[3] - 1
    # stored (x, y) lands at oriented (X, Y): 1 (x, y); 2 (w-1-x, y); 3 (w-1-x, h-1-y); 4 (x, h-1-y); 5 (y, x); 6 (h-1-y, x); 7 (h-1-y, w-1-x); 8 (y, w-1-x)
    return {1: (X0, X1, Y0, Y1), 2: (w - 1 - X1, w - 1 - X0, Y0, Y1), 3: (w - 1 - X1, w - 1 - X0, h - 1 - Y1, h - 1 - Y0), 4: (X0, X1, h - 1 - Y1, h - 1 - Y0),
            5: (Y0, Y1, X0, X1), 6: (Y0, Y1, h - 1 - X1, h - 1 - X0), 7: (w - 1 - Y1, w - 1 - Y0, h - 1 - X1, h - 1 - X0), 8: (w - 1 - Y1, w - 1 - Y0, X0, X1)}[o]


def region(W, H, ss, s, o, crop):
    """-> (gx0, gy0, gx1, gy1)"""
    x0, x1, y0, y1 = stored_rect(cdiv(W, s), cdiv(H, s), o, crop)
    n = 8 // s
    out = []
    for first, last, mcu, size in ((x0, x1, MCU[ss][0], W), (y0, y1, MCU[ss][1], H)):
        blocks = cdiv(size, 8 * mcu) * mcu
        b0, b1 = first // n, last // n
        b0, b1 = b0 // mcu * mcu, b1 // mcu * mcu + mcu - 1
        b0, b1 = max(b0 - mcu, 0), min(b1 + mcu, blocks - 1)
        out.append((b0 // 32, b1 // 32 + 1))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def groups_of(W, H, ss):
    return cdiv(cdiv(W, 8 * MCU[ss][0]) * MCU[ss][0], 32) * cdiv(cdiv(H, 8 * MCU[ss][1]) * MCU[ss][1], 32)


def count(r):
    return (r[2] - r[0]) * (r[3] - r[1])


# ---- files -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def jpeg_of(pic):
    w, h, ss = PICTURES[pic]
    return make_jpeg(JC.photo(w, h, seed=w + h + 3), ss, 85)


@functools.lru_cache(maxsize=None)
def transcode(pic, o=1):
    S.set_orientation(o)
    try:
        return J.transcode(jpeg_of(pic))
    finally:
        S.set_orientation(1)


def pil_open(pic, scale=1, o=1):
    """the file as a loader opens it: draft() for libjpeg's scale, the orientation through ImageOps.exif_transpose"""
    from PIL import Image, ImageOps
    im = Image.open(io.BytesIO(jpeg_of(pic)))
    W, H = im.size
    if scale != 1:
        im.draft(im.mode, (max(1, W // scale), max(1, H // scale)))
        assert im.decoderconfig[0] == scale and im.size == (cdiv(W, scale), cdiv(H, scale)), (im.size, im.decoderconfig)
    im.load()
    if o != 1:
        im.getexif()[0x0112] = o
        im = ImageOps.exif_transpose(im)
    return im


def pil_crop(im, crop, size=None, name=None, mirror=False):
    from PIL import Image
    x0, y0, cw, ch = crop
    im = im.crop((x0, y0, x0 + cw, y0 + ch))
    if size is not None:
        im = im.resize(tuple(size), {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[name])
    a = np.asarray(im)
    a = np.stack([a] * 3, -1) if a.ndim == 2 else a          # (three channels of a grey file: the sample three times)
    return np.ascontiguousarray(a[:, ::-1] if mirror else a)


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


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------
def rule_crops(ow, oh):
    """crops of an ow x oh picture: the middle, one across 256 where the picture has it, the four edges, the far corner's pixel, the whole picture"""
    out = [(ow // 3, oh // 3, max(1, ow // 3), max(1, oh // 3)), (0, oh // 2, max(1, ow // 8), max(1, oh // 4)), (ow // 2, 0, max(1, ow // 4), max(1, oh // 8)),
           (ow - max(1, ow // 9), oh // 4, max(1, ow // 9), max(1, oh // 3)), (ow // 4, oh - max(1, oh // 9), max(1, ow // 2), max(1, oh // 9)), (ow - 1, oh - 1, 1, 1), (0, 0, ow, oh)]
    if ow > 260 and oh > 260:
        out += [(250, 250, 10, 10), (256, 256, 4, 4), (255, 0, 2, oh)]
    return out


def test_region_equals_the_rule(jxh):
    checked = partial = 0
    for pic, (W, H, ss) in PICTURES.items():
        for o, keep in ((1, False), (2, False), (6, False), (7, False), (6, True)):
            data = transcode(pic, o)
            b = jxh.BatchDecoder(-1)                                                          # (host only)
            b.set_option("jpeg_region", 1)
            b.set_option("keep_orientation", 1 if keep else 0)
            eff = 1 if keep else o
            for s in (1, 2, 4, 8):
                w, h = cdiv(W, s), cdiv(H, s)
                ow, oh = (h, w) if eff > 4 else (w, h)
                for crop in rule_crops(ow, oh):
                    i = b.add(data, num_channels=3, resize=(8, 8), crop=crop, jpeg_scale=s, resize_u8=True)
                    if s == 8 and ss != 2:
                        assert b.jpeg_dc_only(i) and b.jpeg_region(i) is None, (pic, o, crop)      # DC-only: no region
                        continue
                    want = region(W, H, ss, s, eff, crop)
                    assert b.jpeg_region(i) == want, (pic, o, keep, s, crop, b.jpeg_region(i), want)
                    checked += 1
                    partial += count(want) < groups_of(W, H, ss)
                    if crop == (0, 0, ow, oh):
                        assert count(want) == groups_of(W, H, ss)                             # the whole picture: every group
    assert checked > 600 and partial > 250, (checked, partial)
    # no region: without a crop, for an image that decode does not take; with jpeg_dc_only off a 4:4:4 image at scale 8 has one
    b = jxh.BatchDecoder(-1)
    b.set_option("jpeg_region", 1)
    data = transcode("301x279_444")
    assert b.jpeg_region(b.add(data, num_channels=3, resize=(8, 8), resize_u8=True)) is None
    assert b.jpeg_region(b.add(data, num_channels=3)) is None
    assert b.jpeg_region(b.add(data, num_channels=3, resize=(8, 8), crop=(3, 3, 9, 9), jpeg_scale=8)) is None
    xyb = S.encode_vardct(S.synthetic_image(3, 300, 280), seed=2, strategy_mix=0, epf_iters=0, gab=0)
    assert b.jpeg_region(b.add(xyb, num_channels=3, resize=(8, 8), crop=(3, 3, 9, 9))) is None
    assert jxh.libjxl().JxlHipBatchJpegRegion(b._h, 99, None) == 0 and "no such image" in jxh.last_error()
    b.set_option("jpeg_dc_only", 0)
    assert b.jpeg_region(2) == region(301, 279, 0, 8, 1, (3, 3, 9, 9)) == (0, 0, 1, 1)
    # the query answers for the option on whether or not it is set
    off = jxh.BatchDecoder(-1)
    assert off.jpeg_region(off.add(transcode("600x520"), num_channels=3, resize=(8, 8), crop=(272, 272, 200, 200), resize_u8=True)) == (1, 1, 2, 2)
    # the centre group alone, and the seam crop that needs the groups before it
    assert region(600, 520, 2, 1, 1, (272, 272, 200, 200)) == (1, 1, 2, 2) and region(600, 520, 2, 1, 1, (256, 256, 100, 100)) == (0, 0, 2, 2)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def decode_items(jx, items, on, keep_orientation=False, setup=None):
    """items: (data, BatchDecoder.add keywords), one batch, each into a device buffer of out_size + EXTRA bytes filled with FILL, FRONT bytes into it
    -> (batch, whole destinations as u8 arrays, out sizes)"""
    import torch
    sizes = jx.BatchDecoder(-1)                                                               # (host only: the sizes of the destinations)
    sizes.set_option("keep_orientation", 1 if keep_orientation else 0)
    b = jx.BatchDecoder(0)
    b.set_option("jpeg_region", 1 if on else 0)
    b.set_option("keep_orientation", 1 if keep_orientation else 0)
    if setup is not None:
        setup(b)
    bufs = []
    for data, kw in items:
        size = sizes.out_size(sizes.add(data, **kw))
        t = torch.full((size + EXTRA,), FILL, dtype=torch.uint8, device="cuda:0")
        assert b.out_size(b.add(data, device_ptr=t.data_ptr() + FRONT, **kw)) == size
        bufs.append((t, size))
    errs = b.decode_jpeg_pixels()
    torch.cuda.synchronize()
    assert errs == [None] * len(items), errs
    return b, [t.cpu().numpy() for t, _ in bufs], [n for _, n in bufs]


def dest_of(pic_u8):
    want = np.full(pic_u8.size + EXTRA, FILL, np.uint8)
    want[FRONT:FRONT + pic_u8.size] = pic_u8.reshape(-1)
    return want


def counters(b):
    return {k: b.info_value(k) for k in ("hf_groups_total", "hf_groups_decoded", "hf_nonzeros")}


def copy_kw(crop, **kw):
    return dict(dtype="uint8", num_channels=3, resize=(crop[2], crop[3]), crop=crop, resize_u8=True, **kw)


@functools.lru_cache(maxsize=None)
def scale1(pic, on):
    """every crop of CROPS[pic] as an image of one batch, u8 x 3, target = the crop's size -> (destinations, counters)"""
    import jpegxl_rs_amd as jx
    b, dests, _ = decode_items(jx, [(transcode(pic), copy_kw(c)) for c in CROPS[pic]], on)
    for d in dests:
        d.setflags(write=False)
    return dests, counters(b)


@pytest.mark.gpu
@pytest.mark.parametrize("pic", sorted(PICTURES))
def test_crops_equal_pillow(jx, pic):
    """1. exactness against Pillow at scale 1, the option on"""
    dests, _ = scale1(pic, True)
    im = pil_open(pic)
    for crop, got in zip(CROPS[pic], dests):
        want = dest_of(pil_crop(im, crop))
        assert np.array_equal(got, want), (pic, crop, int((got != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("pic", sorted(PICTURES))
def test_same_bytes_as_without_the_option_and_fewer_groups(jx, pic):
    """2. the bytes of the option off; hf_groups_decoded is the rule's count, hf_groups_total the frames' groups, fewer non-zeros decoded whenever a group is skipped"""
    W, H, ss = PICTURES[pic]
    (on, con), (off, coff) = scale1(pic, True), scale1(pic, False)
    for crop, a, c in zip(CROPS[pic], on, off):
        assert np.array_equal(a, c), (pic, crop)
    want = sum(count(region(W, H, ss, 1, 1, c)) for c in CROPS[pic])
    total = len(CROPS[pic]) * groups_of(W, H, ss)
    print(pic, "on", con, "off", coff, "rule", want, "of", total)
    assert con["hf_groups_total"] == total and con["hf_groups_decoded"] == want and want < total
    assert 0 < con["hf_nonzeros"] < coff["hf_nonzeros"]
    if pic != "600x520":
        return
    # the centre group alone: 1 of 9; the whole picture: all 9 and every non-zero
    data = transcode(pic)
    b, dests, _ = decode_items(jx, [(data, copy_kw((272, 272, 200, 200)))], True)
    assert (b.info_value("hf_groups_decoded"), b.info_value("hf_groups_total")) == (1, 9) and np.array_equal(dests[0], on[0])
    whole = [(data, copy_kw((0, 0, 600, 520)))]
    (b1, d1, _), (b0, d0, _) = decode_items(jx, whole, True), decode_items(jx, whole, False)
    assert counters(b1) == counters(b0) and b1.info_value("hf_groups_decoded") == 9 and b1.info_value("hf_nonzeros") > 0
    assert np.array_equal(d1[0], d0[0]) and np.array_equal(d1[0], on[-1])
    # the stage bytes go by the region: the HF, IDCT and output stages of the centre crop are below those of the option off
    sb_on, sb_off = b.stage_bytes, decode_items(jx, [(data, copy_kw((272, 272, 200, 200)))], False)[0].stage_bytes
    print("stage bytes on", sb_on, "off", sb_off)
    assert all(sb_on[k] < sb_off[k] for k in ("hf", "idct", "out")) and sb_on["lf"] == sb_off["lf"]


@pytest.mark.gpu
@pytest.mark.parametrize("pic", sorted(PICTURES))
def test_option_off(jx, pic):
    """7. the default: every group is decoded, and the bytes are Pillow's"""
    dests, c = scale1(pic, False)
    W, H, ss = PICTURES[pic]
    assert c["hf_groups_decoded"] == c["hf_groups_total"] == len(CROPS[pic]) * groups_of(W, H, ss)
    im = pil_open(pic)
    for crop, got in zip(CROPS[pic], dests):
        assert np.array_equal(got, dest_of(pil_crop(im, crop))), (pic, crop)


# kernels.h kHfVar*: HfDecodeWaveKernel, HfDecodeSimtKernel<true, false, false> / <true, true, true> / <false, true, true>, HfDecodeKernel (lane stride)
HF_KERNELS = {
    "wave": (1, ("301x279_444", "301x279_grey"), lambda b: (b.set_lane_stride(8, 1), b.set_option("hf_lanes_per_wave", 1))),
    "simt_plain": (2, ("301x279_444", "301x279_grey"), lambda b: b.set_lane_stride(8, 1)),
    "simt_all_lds": (4, ("600x520", "301x279_422"), lambda b: b.set_lane_stride(8, 1)),
    "simt_global": (8, ("600x520", "301x279_422"), lambda b: (b.set_lane_stride(8, 1), b.set_option("lds_code_budget", 0))),
    "lane_stride": (16, ("301x279_444", "301x279_grey"), lambda b: b.set_lane_stride(8, 64)),      # (chroma-subsampled frames always take the SIMT kernel)
}


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", sorted(HF_KERNELS))
def test_every_hf_kernel_takes_the_list(jx, kernel):
    """the three HF kernels and every instantiation of the SIMT one, asserted to be the one that ran: the bytes are Pillow's and the groups decoded are the rule's"""
    variant, pics, setup = HF_KERNELS[kernel]
    items, want, rule, total = [], [], 0, 0
    for pic in pics:
        W, H, ss = PICTURES[pic]
        for crop in CROPS[pic][:3]:
            items.append((transcode(pic), copy_kw(crop))); want.append(dest_of(pil_crop(pil_open(pic), crop)))
            rule += count(region(W, H, ss, 1, 1, crop)); total += groups_of(W, H, ss)
    b, dests, _ = decode_items(jx, items, True, setup=setup)
    assert b.info_value("hf_variant") == variant, (kernel, b.info_value("hf_variant"))
    for (d, kw), got, w in zip(items, dests, want):
        assert np.array_equal(got, w), (kernel, kw["crop"], int((got != w).sum()))
    assert (b.info_value("hf_groups_decoded"), b.info_value("hf_groups_total")) == (rule, total) and rule < total


def scaled_crops(w, h):
    """crops of the w x h scaled picture: the middle, the far corner, the left edge, the whole picture"""
    return [(w // 3, h // 3, max(1, w // 3), max(1, h // 4)), (w - max(1, w // 7), h - max(1, h // 6), max(1, w // 7), max(1, h // 6)), (0, h // 2, max(1, w // 5), max(1, h // 3)),
            (0, 0, w, h)]


@pytest.mark.gpu
def test_scales(jx):
    """3. jpeg_scale 2, 4, 8 (4:2:0) and 2, 4 (4:2:2, grey), crops given in the scaled picture, against draft() + crop()"""
    for pic, scales in (("600x520", (2, 4, 8)), ("2100x300", (2, 4, 8)), ("301x279_422", (2, 4)), ("301x279_grey", (2, 4))):
        W, H, ss = PICTURES[pic]
        items, want, rule = [], [], 0
        for s in scales:
            im = pil_open(pic, s)
            for crop in scaled_crops(*im.size):
                items.append((transcode(pic), copy_kw(crop, jpeg_scale=s))); want.append(dest_of(pil_crop(im, crop)))
                rule += count(region(W, H, ss, s, 1, crop))
        b, dests, _ = decode_items(jx, items, True)
        for (d, kw), got, w in zip(items, dests, want):
            assert np.array_equal(got, w), (pic, kw["jpeg_scale"], kw["crop"], int((got != w).sum()))
        assert b.info_value("hf_groups_decoded") == rule < b.info_value("hf_groups_total") == len(items) * groups_of(W, H, ss)


@pytest.mark.gpu
def test_resampled_and_float_outputs(jx):
    """3. resize_u8 with bilinear and bicubic targets and a mirror against crop().resize(); one planar float16 output with scale / bias against the option-off bytes"""
    pic = "600x520"
    data, im = transcode(pic), pil_open(pic)
    items, want = [], []
    for name in ("bilinear", "bicubic"):
        for crop, size, mirror in (((280, 250, 300, 260), (224, 224), False), ((10, 400, 100, 100), (64, 48), True), ((256, 256, 100, 100), (64, 48), True)):
            items.append((data, dict(dtype="uint8", num_channels=3, resize=size, crop=crop, filter=name, mirror=mirror, resize_u8=True)))
            want.append(dest_of(pil_crop(im, crop, size, name, mirror)))
    ims = pil_open(pic, 2)
    items.append((data, dict(dtype="uint8", num_channels=3, resize=(64, 48), crop=(150, 130, 140, 120), filter="bicubic", jpeg_scale=2, resize_u8=True)))
    want.append(dest_of(pil_crop(ims, (150, 130, 140, 120), (64, 48), "bicubic")))
    b, dests, _ = decode_items(jx, items, True)
    for (d, kw), got, w in zip(items, dests, want):
        assert np.array_equal(got, w), (kw, int((got != w).sum()))
    assert b.info_value("hf_groups_decoded") < b.info_value("hf_groups_total")
    f16 = [(transcode(p), dict(dtype="float16", num_channels=3, planar=True, align=64, scale=[2.0, 0.5, 4.0, 1.0], bias=[-1.0, 0.25, -0.5, 0.0], resize=(31, 17), crop=c, filter="bicubic",
                               resize_u8=u8)) for p, c, u8 in (("600x520", (300, 300, 200, 120), True), ("301x279_422", (250, 3, 40, 200), False), ("301x279_444", (0, 250, 301, 29), True))]
    (b1, d1, _), (b0, d0, _) = decode_items(jx, f16, True), decode_items(jx, f16, False)
    for a, c in zip(d1, d0):
        assert np.array_equal(a, c) and (a[:FRONT] == FILL).all() and (a[FRONT:] != FILL).any()
    assert b1.info_value("hf_groups_decoded") < b0.info_value("hf_groups_decoded") == b0.info_value("hf_groups_total")


def corner_crops(ow, oh):
    return [(0, 0, 40, 30), (ow - 37, 0, 37, 45), (0, oh - 33, 50, 33), (ow - 41, oh - 29, 41, 29)]


@pytest.mark.gpu
def test_orientation(jx):
    """4. orientations 6 and 2 and keep_orientation, crops near each corner of the oriented picture, against Pillow after exif_transpose"""
    for pic in ("600x520", "301x279_422"):
        W, H, ss = PICTURES[pic]
        for o, keep in ((6, False), (2, False), (6, True)):
            eff = 1 if keep else o
            for s in (1, 2):
                im = pil_open(pic, s, eff)
                ow, oh = im.size
                assert (ow, oh) == ((cdiv(H, s), cdiv(W, s)) if eff > 4 else (cdiv(W, s), cdiv(H, s)))
                crops = corner_crops(ow, oh)
                b, dests, _ = decode_items(jx, [(transcode(pic, o), copy_kw(c, jpeg_scale=s)) for c in crops], True, keep_orientation=keep)
                for crop, got in zip(crops, dests):
                    want = dest_of(pil_crop(im, crop))
                    assert np.array_equal(got, want), (pic, o, keep, s, crop, int((got != want).sum()))
                assert b.info_value("hf_groups_decoded") == sum(count(region(W, H, ss, s, eff, c)) for c in crops) < b.info_value("hf_groups_total")


@pytest.mark.gpu
def test_one_prepared_batch_several_regions(jx):
    """5. one resident BatchDecoder: crop A, then crop B after another SetOutput, then no crop — each what a fresh batch gives; after reset() a float decode() of the
    same streams is a fresh one: Run ignores the lists, and the coefficient planes were left clean"""
    import ctypes as C
    pic = "600x520"
    datas = [transcode(pic), transcode("2100x300")]
    L = jx.libjxl()
    fmt = jx.JxlPixelFormat(3, jx._PIXEL_TYPES["uint8"][0], jx.Endianness.Native, 0)
    b = jx.BatchDecoder(0)
    b.set_option("jpeg_region", 1)
    for d in datas:
        b.add(d, dtype="uint8", num_channels=3, resize=(64, 48), crop=(10, 10, 100, 90), filter="bicubic", resize_u8=True)
    ims = [pil_open(pic), pil_open("2100x300")]
    for crop in ((10, 10, 100, 90), (400, 300, 150, 200), None):
        groups = 27 if crop is None else count(region(600, 520, 2, 1, 1, crop)) + count(region(2100, 300, 2, 1, 1, (crop[0] + 1500, 5, crop[2], 250)))
        assert groups in (1 + 4, 4 + 4, 27)
        for i in range(2):
            c = crop if i == 0 or crop is None else (crop[0] + 1500, 5, crop[2], 250)
            rs = jx.JxlHipOutputResample(64, 48, *(c or (0, 0, 0, 0)), 1, 0)
            assert L.JxlHipBatchSetOutputJpegResampled(b._h, i, C.byref(fmt), None, 1, None, C.byref(rs), jx.JXL_HIP_RESAMPLE_U8) == 0, jx.last_error()
        assert b.decode_jpeg_pixels() == [None, None]
        for i in range(2):
            c = crop if i == 0 or crop is None else (crop[0] + 1500, 5, crop[2], 250)
            want = pil_crop(ims[i], c or (0, 0) + ims[i].size, (64, 48), "bicubic")
            assert np.array_equal(b.output(i).reshape(48, 64, 3), want), (crop, i)
        assert b.info_value("hf_groups_decoded") == groups and b.info_value("hf_groups_total") == 27, (crop, b.info_value("hf_groups_decoded"))
    # a float decode() of the same prepared batch: every group, whatever the option says — what a fresh batch without the option decodes
    for i in range(2):
        rs = jx.JxlHipOutputResample(64, 48, 300, 100, 200, 150, 1, 0)
        assert L.JxlHipBatchSetOutputResampled(b._h, i, C.byref(fmt), None, 1, None, C.byref(rs)) == 0, jx.last_error()
    assert b.jpeg_region(0) is not None
    b.prepare(); b.decode(); b.finish()
    plain = jx.BatchDecoder(0)
    for d in datas:
        plain.add(d, dtype="uint8", num_channels=3, resize=(64, 48), crop=(300, 100, 200, 150), filter="bicubic")
    plain.prepare(); plain.decode(); plain.finish()
    for i in range(2):
        assert np.array_equal(b.output(i), plain.output(i)), i
    assert b.stage_bytes == plain.stage_bytes                                                  # (the stage bytes go by the region for the libjpeg-exact decode alone)
    fresh = float_decode(jx.BatchDecoder(0), datas)
    b.reset()
    for got, w in zip(float_decode(b, datas), fresh):
        assert np.array_equal(got, w)


def small_pipeline(jx, **kw):
    opts = dict(jobs_in_flight=3, lf_streams=2, hf_streams=2, prepare_threads=1, parse_threads=2)
    opts.update(kw)
    return jx.Pipeline(0, **opts)


@pytest.mark.gpu
def test_pipeline_jobs(jx):
    """6. jobs of a pipeline with set_option("jpeg_region", 1): the bytes of a pipeline without it; region, float, reconstruction and region jobs through one pipeline
    with shared coefficient sets; a crop that leaves its image fails alone"""
    import torch
    pics = ["600x520", "301x279_422", "2100x300", "301x279_grey", "301x279_444"]
    datas = [transcode(p) for p in pics]
    n = len(datas)
    crops = [(272, 272, 200, 200), (200, 200, 100, 70), None, (0, 0, 60, 50), (296, 272, 5, 7)]
    filters = ["bicubic", "bilinear", "bicubic", "bilinear", "bicubic"]
    mirrors = [False, True, True, False, True]
    kw = dict(jpeg_pixels=True, resize_u8=True, crop=crops, filter=filters, mirror=mirrors, planar=True, resize=(48, 32))
    one = 3 * 32 * 48
    want = np.stack([pil_crop(pil_open(p), c or (0, 0) + PICTURES[p][:2], (48, 32), f, m).transpose(2, 0, 1) for p, c, f, m in zip(pics, crops, filters, mirrors)])

    def job(p, **more):
        out = torch.full((n, 3, 32, 48), 7, dtype=torch.uint8, device="cuda:0")
        st, _ = p.wait(p.submit(datas, "uint8", 3, device_ptrs=[out[k].data_ptr() for k in range(n)], capacities=[one] * n, **dict(kw, **more)))
        torch.cuda.synchronize()
        assert st == [0] * n
        return out.cpu().numpy()

    off = small_pipeline(jx)
    try:
        ref = job(off)
        assert off.info("hf_groups_decoded") == off.info("hf_groups_total") == 9 + 4 + 18 + 4 + 4
        sizes = [jx.image_out_size(d, "uint8", 3)[1] for d in datas]
        bufs = [jx.PinnedBuffer(x) for x in sizes]
        off.wait(off.submit(datas, "uint8", 3, host_ptrs=[x.ptr for x in bufs], capacities=sizes))
        plain_ref = [np.array(x.array) for x in bufs]
        files_ref = off.wait_jpegs(off.submit_jpegs(datas))[0]
    finally:
        off.close()
    assert np.array_equal(ref, want)
    assert files_ref == [jpeg_of(p) for p in pics]
    p = small_pipeline(jx)
    try:
        p.set_option("jpeg_region", 1)
        got = job(p)
        assert np.array_equal(got, ref)
        rule = 1 + 4 + 18 + 1 + 1
        assert (p.info("hf_groups_decoded"), p.info("hf_groups_total")) == (rule, 39)
        assert [count(region(*PICTURES[q], 1, 1, c)) if c else groups_of(*PICTURES[q]) for q, c in zip(pics, crops)] == [1, 4, 18, 1, 1]
        # region, plain float, reconstruction and region jobs again, all submitted before any is collected
        kinds = ["region", "plain", "files", "region", "plain", "files", "region"]
        tickets = []
        for kind in kinds:
            if kind == "files":
                tickets.append((p.submit_jpegs(datas), None))
            elif kind == "plain":
                bufs = [jx.PinnedBuffer(x) for x in sizes]
                tickets.append((p.submit(datas, "uint8", 3, host_ptrs=[x.ptr for x in bufs], capacities=sizes), bufs))
            else:
                bufs = [jx.PinnedBuffer(one) for _ in range(n)]
                tickets.append((p.submit(datas, "uint8", 3, host_ptrs=[x.ptr for x in bufs], capacities=[one] * n, **kw), bufs))
        for kind, (t, bufs) in zip(kinds, tickets):
            if kind == "files":
                files, errors, _ = p.wait_jpegs(t)
                assert errors == [None] * n and files == files_ref
                continue
            st, _ = p.wait(t)
            assert st == [0] * n
            for k in range(n):
                w = ref[k].reshape(-1) if kind == "region" else plain_ref[k]
                assert np.array_equal(np.array(bufs[k].array), w), (kind, k)
        # a crop that leaves its image fails alone
        bad = [(272, 272, 200, 200), (250, 200, 100, 70), None, (0, 0, 60, 50), (296, 272, 5, 7)]
        bufs = [jx.PinnedBuffer(one) for _ in range(n)]
        for x in bufs:
            x.array[:] = FILL
        st, _ = p.wait(p.submit(datas, "uint8", 3, host_ptrs=[x.ptr for x in bufs], capacities=[one] * n, **dict(kw, crop=bad)), check=False)
        assert st == [0, 1, 0, 0, 0] and "leaves the 301 x 279 picture" in jx.last_error(), (st, jx.last_error())
        assert (np.array(bufs[1].array) == FILL).all()
        for k in (0, 2, 3, 4):
            assert np.array_equal(np.array(bufs[k].array), ref[k].reshape(-1)), k
        assert p.info("hf_groups_decoded") < p.info("hf_groups_total")
        # the option is read at the submit: off again, every group
        p.set_option("jpeg_region", 0)
        assert np.array_equal(job(p), ref) and p.info("hf_groups_decoded") == p.info("hf_groups_total") == 39
    finally:
        p.close()
