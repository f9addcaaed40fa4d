"""libjpeg's scaled decodes of JPEG transcodes, exact (include/jxl_hip.h JxlHipBatchSetOutputJpegScaled; BatchDecoder.add(..., jpeg_scale=); csrc/jpeg_pixels.hip
JpegIdctScaledKernel / JpegColorOutScaledKernel): the samples libjpeg gives for the original file at scale 1/2, 1/4, 1/8.  The yardstick is again a decoder this repository
has no part in: Pillow's libjpeg-turbo through Image.draft.  Every comparison with it is np.array_equal on u8.

draft(mode, (max(1, W // s), max(1, H // s))) reaches scale s exactly when both sides are >= s (asserted on im.decoderconfig and the size); only below that a case falls
back to `restate_scaled`, the rules in numpy int64 from the coefficients and tables tests/jpeg_tools.parse_jpeg reads out of the file (nothing from oracle/ or the product),
with m = 8 / s, DESCALE(x, n) = (x + 2^(n-1)) >> n:
  1. IDCT size per component: n = m; while n < 8 and (hmax m) % (h_c n 2) == 0 and (vmax m) % (v_c n 2) == 0: n = 2 n.  A block gives n x n samples, the component's real
     extent is ceil(W h_c n / (hmax 8)) x ceil(H v_c n / (vmax 8)); the picture is ceil(W / s) x ceil(H / s).
  2. d[v][u] = coef x q for every n.
  3. n = 8: jpeg_idct_islow (test_jpeg_exact_pixels._idct_1d).
  4. n = 4 (jidctred.c jpeg_idct_4x4): t0 = i0 << 14, t2 = 15137 i2 - 6270 i6, a0 = -1730 i7 + 11893 i5 - 17799 i3 + 8697 i1, a2 = -4176 i7 - 4926 i5 + 7373 i3 + 20995 i1;
     out0 = D(t0 + t2 + a2), out1 = D(t0 - t2 + a0), out2 = D(t0 - t2 - a0), out3 = D(t0 + t2 - a2); columns 0, 1, 2, 3, 5, 6, 7 with D = DESCALE(., 12), then the four
     workspace rows over the same entries with DESCALE(., 19).
  5. n = 2 (jpeg_idct_2x2): t10 = i0 << 15, t0 = -5906 i7 + 6967 i5 - 10426 i3 + 29692 i1, outputs DESCALE(t10 +- t0, 13) over columns 0, 1, 3, 5, 7, then the two rows over
     the same entries with DESCALE(., 20).
  6. n = 1: DESCALE(d[0][0], 3).
  7. + 128, clamp to [0, 255].
  8. A component of half the picture's width (4:2:2 chroma only): the h2v1 "fancy" rule if m > 1 and its width > 2, else replication.
  9. jdcolor.c as at full size.
test_restatement_equals_pillow pins the restatement against Pillow without a device.  The bound of the resampled outputs is the derived one of test_resample_jobs.py, through
test_jpeg_exact_pixels.resample: (taps_x + taps_y + 8) x 2^-24 x L_x x L_y x max|v|; no new number."""
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
from test_jpeg_exact_pixels import (BPS, EXTRA, FILL, FRONT, REFUSAL, _columns, _idct_1d, decode_items, expected_dest, float_decode, make_jpeg, pillow, resample, saturated,
                                    strip_boxes)

SAMPLINGS = (0, 1, 2, "grey")
SCALES = (2, 4, 8)
SHAPES = [(1, 1), (2, 2), (4, 4), (8, 8), (9, 9), (16, 16), (17, 9), (12, 10), (20, 33), (67, 41), (300, 280), (520, 264)]


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


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------------
def pillow_scaled(jpeg, s):
    """Pillow's decode at scale 1 / s, or None where draft cannot reach that scale (a side shorter than s)"""
    from PIL import Image
    im = Image.open(io.BytesIO(jpeg))
    W, H = im.size
    im.draft(im.mode, (max(1, W // s), max(1, H // s)))
    if W < s or H < s:
        return None
    assert im.decoderconfig[0] == s, (W, H, s, im.decoderconfig)
    assert im.size == (cdiv(W, s), cdiv(H, s)), (im.size, W, H, s)
    assert im.mode in ("RGB", "L")
    return np.asarray(im)


# ---- the definition --------------------------------------------------------------------------------------------------------------------------
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct4_1d(i, shift):
    i0, i1, i2, i3, _, i5, i6, i7 = i
    t0 = i0 << 14
    t2 = 15137 * i2 - 6270 * i6
    a0 = -1730 * i7 + 11893 * i5 - 17799 * i3 + 8697 * i1
    a2 = -4176 * i7 - 4926 * i5 + 7373 * i3 + 20995 * i1
    return [_descale(t0 + t2 + a2, shift), _descale(t0 - t2 + a0, shift), _descale(t0 - t2 - a0, shift), _descale(t0 + t2 - a2, shift)]


def _idct2_1d(i, shift):
    i0, i1, _, i3, _, i5, _, i7 = i
    t10 = i0 << 15
    t0 = -5906 * i7 + 6967 * i5 - 10426 * i3 + 29692 * i1
    return [_descale(t10 + t0, shift), _descale(t10 - t0, shift)]


def component_plane(coef, q, n, stats):
    """(grid rows, grid columns, 64) coefficients, natural order -> the n x n samples of every block of the padded grid, int64"""
    gh, gw = coef.shape[:2]
    d = coef.astype(np.int64).reshape(gh, gw, 8, 8) * np.asarray(q, np.int64).reshape(8, 8)
    if n == 1:
        out = _descale(d[:, :, :1, :1], 3)
    else:
        one_d, s1, s2 = {8: (_idct_1d, 11, 18), 4: (_idct4_1d, 12, 19), 2: (_idct2_1d, 13, 20)}[n]
        # pass 1 over the columns: ws[r][u] for r < n, all eight u (the entries of the columns a form never transforms are computed and never read); pass 2 over its rows
        ws = np.stack(one_d([d[:, :, r, :] for r in range(8)], s1), axis=2)
        out = np.stack(one_d([ws[:, :, :, u] for u in range(8)], s2), axis=3)
    out = out + 128
    stats["idct_min"] = min(stats.get("idct_min", 1 << 40), int(out.min()))
    stats["idct_max"] = max(stats.get("idct_max", -(1 << 40)), int(out.max()))
    return np.clip(out, 0, 255).transpose(0, 2, 1, 3).reshape(gh * n, gw * n)


def idct_sizes(components, s):
    """rule 1 -> n per component"""
    m = 8 // s
    hmax, vmax = max(c["h"] for c in components), max(c["v"] for c in components)
    out = []
    for c in components:
        n = m
        while n < 8 and (hmax * m) % (c["h"] * n * 2) == 0 and (vmax * m) % (c["v"] * n * 2) == 0:
            n *= 2
        out.append(n)
    return out


def restate_scaled(jpeg, s, stats=None):
    stats = {} if stats is None else stats
    j = J.parse_jpeg(jpeg)
    W, H, m = j.width, j.height, 8 // s
    ow, oh = cdiv(W, s), cdiv(H, s)
    hmax, vmax = max(c["h"] for c in j.components), max(c["v"] for c in j.components)
    full = []
    for c, (comp, n) in enumerate(zip(j.components, idct_sizes(j.components, s))):
        plane = component_plane(j.coef[c], j.qt[comp["tq"]], n, stats)
        cw, ch = cdiv(W * comp["h"] * n, hmax * 8), cdiv(H * comp["v"] * n, vmax * 8)
        p = plane[:ch, :cw]
        if (cw, ch) != (ow, oh):
            assert ch == oh and cw == cdiv(ow, 2), (cw, ch, ow, oh)                  # half the picture's width, all of its height: 4:2:2 chroma
            stats.setdefault("chroma_widths", set()).add((m, cw))
            p = _columns(p, 1, 2, 2, lambda v, r: v) if m > 1 and cw > 2 else np.repeat(p, 2, axis=1)
        full.append(p[:oh, :ow])
    if len(full) == 1:
        return full[0].astype(np.uint8)
    y, cb, cr = full[0], full[1] - 128, full[2] - 128
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], axis=-1)
    stats["rgb_min"] = min(stats.get("rgb_min", 1 << 40), int(rgb.min()))
    stats["rgb_max"] = max(stats.get("rgb_max", -(1 << 40)), int(rgb.max()))
    return np.clip(rgb, 0, 255).astype(np.uint8)


# ---- files -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_files(ss):
    out = [("%dx%d" % (w, h), make_jpeg(JC.photo(w, h, seed=w + h), ss, 85)) for w, h in SHAPES]
    out += [("saturated q5", make_jpeg(saturated(), ss, 5)), ("saturated q100", make_jpeg(saturated(), ss, 100))]
    out += [("progressive", make_jpeg(JC.photo(40, 24, seed=9), ss, 85, progressive=True)), ("restart", make_jpeg(JC.photo(40, 24, seed=9), ss, 85, restart_marker_blocks=2))]
    out += [("coarse dc", coarse_dc(ss))]
    return out


def coarse_dc(ss):
    """Flat black and flat white 16 x 16 patches under a quantiser of 225 for every coefficient (quality 50 leaves a given table as it is): the DC term of a white
    block, (255 - 128) x 8 = 1016, is coded as 5 and comes back as 1125, that of a black one, -1024, as -1125 — DESCALE(+-1125, 3) + 128 is 269 and -13, so the IDCT
    clamp cuts at both ends at every scale, the 1 x 1 form included, where no ringing could pass the range"""
    img = np.zeros((32, 32, 3), np.uint8)
    img[:16, 16:], img[16:, :16] = 255, 255
    return make_jpeg(img, ss, 50, qtables=[[225] * 64, [225] * 64])


@functools.lru_cache(maxsize=None)
def transcodes(ss):
    return [J.transcode(d) for _, d in shape_files(ss)]


@functools.lru_cache(maxsize=None)
def wanted(ss, s):
    """per file of shape_files(ss): Pillow's picture at scale 1 / s where draft reaches it, else the restatement (a side shorter than s); computed once, never changed"""
    out = []
    for _, d in shape_files(ss):
        k = pillow(d) if s == 1 else pillow_scaled(d, s)
        if k is None:
            j = J.parse_jpeg(d)
            assert j.width < s or j.height < s
            k = restate_scaled(d, s)
        k.setflags(write=False)
        out.append(k)
    return out


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_pillow():
    for ss in SAMPLINGS:
        hx, vx = {0: (1, 1), 1: (2, 1), 2: (2, 2), "grey": (1, 1)}[ss]
        files = dict(shape_files(ss))
        assert J.parse_jpeg(files["progressive"]).sof == 0xC2 and J.parse_jpeg(files["restart"]).restart_interval == 2
        for s in SCALES:
            m = 8 // s
            compared, st_all = 0, {}
            for name, d in files.items():
                j = J.parse_jpeg(d)
                # rule 1 on the file itself: luma, grey, 4:4:4 and 4:2:2 chroma take m, 4:2:0 chroma twice that
                assert idct_sizes(j.components, s) == ([m] if ss == "grey" else [m, 2 * m, 2 * m] if ss == 2 else [m, m, m]), (ss, s, name)
                st = {}
                got, want = restate_scaled(d, s, st), pillow_scaled(d, s)
                assert got.shape[:2] == (cdiv(j.height, s), cdiv(j.width, s))
                for key, v in st.items():
                    st_all.setdefault(name, {})[key] = v
                if want is None:
                    assert j.width < s or j.height < s, (name, s)                 # the only cases left out
                    continue
                compared += 1
                assert got.shape == want.shape, (ss, s, name)
                assert np.array_equal(got, want), (ss, s, name, int((got != want).sum()))
            assert compared >= 9 + 4, (ss, s, compared)
            if ss == 1:
                widths = set().union(*[v.get("chroma_widths", set()) for v in st_all.values()])
                if m > 1:
                    assert (m, 2) in widths and (m, 3) in widths, (s, widths)   # replication of a two-sample plane beside the narrowest interpolated one
                if s == 2:
                    assert st_all["12x10"]["chroma_widths"] == {(4, 3)}
                if s == 4:
                    assert st_all["12x10"]["chroma_widths"] == {(2, 2)} and st_all["17x9"]["chroma_widths"] == {(2, 3)}
            for name in ("saturated q5", "saturated q100"):
                st = st_all[name]
                print(ss, s, name, st)
                # the colour clamp cuts at both ends at every scale; the IDCT's does at quality 5 for n = 4 and n = 2 (a 1 x 1 "transform" is the block's mean: it
                # cannot overshoot the way ringing does — there, and at quality 100, the samples reach both ends of the range without passing them)
                assert ss == "grey" or (st["rgb_min"] < 0 and st["rgb_max"] > 255)
                if name == "saturated q5" and s < 8:
                    assert st["idct_min"] < 0 and st["idct_max"] > 255
                if name == "saturated q100":
                    assert st["idct_min"] == 0 and st["idct_max"] >= 255
            st = st_all["coarse dc"]
            print(ss, s, "coarse dc", st)
            assert st["idct_min"] < 0 and st["idct_max"] > 255, (ss, s, st)     # the IDCT clamp cuts at both ends at every n, 1 x 1 included (coarse_dc)
            if s == 8:
                assert (st["idct_min"], st["idct_max"]) == (-13, 269), st


def size_formula(w, h, dtype, nc, align, planar):
    bps = BPS[dtype]
    row = w * bps * (1 if planar else nc)
    stride = cdiv(row, align) * align if align > 1 else row
    return nc * stride * h if planar else stride * (h - 1) + row


def test_symbols_sizes_and_refusals(jxh):
    L = jxh.libjxl()
    with open(os.path.join(ROOT, "include", "jxl_hip.h")) as f:
        header = f.read()
    for name in ("JxlHipBatchOutBufferSizeJpegScaled", "JxlHipBatchSetOutputJpegScaled", "JxlHipImageOutSizeJpegScaled", "JxlHipPipelineSubmitJpegPixelsScaled"):
        assert hasattr(L, name) and name + "(" in header, name
    for fn in (jxh.BatchDecoder.add, jxh.BatchDecoder.add_many, jxh.image_out_size, jxh.Pipeline.submit):
        assert "jpeg_scale" in inspect.signature(fn).parameters
    W, H = 67, 41
    jpeg = make_jpeg(JC.photo(W, H, seed=108), 2, 85)
    jxl = J.transcode(jpeg)
    b = jxh.BatchDecoder(-1)                 # (a host-only batch: nothing here needs a device)
    for s in (1, 2, 4, 8):
        w, h = cdiv(W, s), cdiv(H, s)
        for dtype in ("uint8", "uint16", "float16", "float32"):
            for nc in (1, 2, 3, 4):
                for align in (0, 64):
                    for planar in (False, True):
                        kw = dict(dtype=dtype, num_channels=nc, align=align, planar=planar)
                        size = jxh.image_out_size(jxl, jpeg_scale=s, **kw)[1]
                        assert size == size_formula(w, h, dtype, nc, align, planar), (s, kw)
                        if s == 1:
                            assert size == jxh.image_out_size(jxl, **kw)[1]
        i = b.add(jxl, dtype="uint16", num_channels=3, align=64, jpeg_scale=s)
        assert b.out_size(i) == size_formula(w, h, "uint16", 3, 64, False)
        assert b.can_decode_jpeg_pixels(i), jxh.last_error()
        i = b.add(jxl, dtype="float32", num_channels=3, resize=(48, 32), crop=(w - 5, h - 3, 5, 3), filter="bicubic", mirror=True, jpeg_scale=s)
        assert b.out_size(i) == 48 * 32 * 3 * 4 and b.can_decode_jpeg_pixels(i), jxh.last_error()
    plain = jxh.BatchDecoder(-1)
    i1, i2 = plain.add(jxl, num_channels=3), b.add(jxl, num_channels=3, jpeg_scale=1)
    assert plain.out_size(i1) == b.out_size(i2) == W * H * 3
    assert jxh.image_out_size(jxl, resize=(20, 10), crop=(1, 2, 30, 30), jpeg_scale=1)[1] == jxh.image_out_size(jxl, resize=(20, 10), crop=(1, 2, 30, 30))[1]
    # the refusals (a batch of its own each: a refused add leaves its image behind)
    with pytest.raises(jxh.DecodeError, match="jpeg_scale must be 1, 2, 4 or 8"):
        jxh.BatchDecoder(-1).add(jxl, jpeg_scale=3)
    with pytest.raises(jxh.DecodeError, match="jpeg_scale must be 1, 2, 4 or 8"):
        jxh.image_out_size(jxl, jpeg_scale=16)
    with pytest.raises(jxh.DecodeError, match="jpeg_scale 2 together with downscale 8"):
        jxh.BatchDecoder(-1).add(jxl, jpeg_scale=2, downscale=8)
    with pytest.raises(jxh.DecodeError, match="jpeg_scale 4 together with downscale 8"):
        jxh.image_out_size(jxl, jpeg_scale=4, downscale=8)
    # a crop that lies inside the full picture and leaves the scaled one (17 x 11 at s = 4)
    assert jxh.image_out_size(jxl, resize=(8, 8), crop=(10, 0, 8, 8))[1] == 8 * 8 * 3
    assert jxh.image_out_size(jxl, resize=(8, 8), crop=(9, 3, 8, 8), jpeg_scale=4)[1] == 8 * 8 * 3
    with pytest.raises(jxh.DecodeError, match="leaves the 17 x 11 picture"):
        jxh.image_out_size(jxl, resize=(8, 8), crop=(10, 0, 8, 8), jpeg_scale=4)
    with pytest.raises(jxh.DecodeError, match="leaves the 17 x 11 picture"):
        jxh.BatchDecoder(-1).add(jxl, resize=(8, 8), crop=(10, 0, 8, 8), jpeg_scale=4)
    # an image the libjpeg-exact decode does not take has no scaled picture
    xyb = S.encode_vardct(S.synthetic_image(3, 40, 24), seed=2, strategy_mix=0, epf_iters=0, gab=0)
    with pytest.raises(jxh.DecodeError) as e:
        jxh.BatchDecoder(-1).add(xyb, jpeg_scale=2)
    assert str(e.value).startswith(REFUSAL) or REFUSAL in str(e.value)
    # jpeg_scale on a pipeline job that is not a libjpeg-exact one: refused before the pipeline is touched, so an object without one will do where there is no device
    p = jxh.Pipeline.__new__(jxh.Pipeline)
    p._h, p._keep = None, {}
    with pytest.raises(jxh.DecodeError, match="not a libjpeg-exact"):
        p.submit([jxl], "uint8", 3, host_ptrs=[0], jpeg_scale=2)
    with pytest.raises(jxh.DecodeError, match="downscale 8"):
        p.submit([jxl], "uint8", 3, host_ptrs=[0], jpeg_pixels=True, jpeg_scale=2, downscale=8)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def small_pipeline(jx, **kw):
    opts = dict(jobs_in_flight=3, lf_streams=2, hf_streams=1, prepare_threads=1, parse_threads=2)
    opts.update(kw)
    return jx.Pipeline(0, **opts)


def scaled_batch(jx, entries, nc):
    """entries: (transcode, scale) -> (batch, errors, u8 pictures) of ONE decode_jpeg_pixels"""
    b = jx.BatchDecoder()
    for d, s in entries:
        b.add(d, num_channels=nc, jpeg_scale=s)
    errs = b.decode_jpeg_pixels()
    outs = []
    for i, (d, s) in enumerate(entries):
        w, h = cdiv(b.info(i).xsize, s), cdiv(b.info(i).ysize, s)
        outs.append(None if errs[i] else b.output(i).reshape((h, w) if nc == 1 else (h, w, nc)))
    return b, errs, outs


@pytest.mark.gpu
@pytest.mark.parametrize("ss", SAMPLINGS)
def test_every_shape_at_every_scale_in_one_batch(jx, ss):
    datas = transcodes(ss)
    entries, want = [], []
    for k, d in enumerate(datas):
        for s in (1, 2, 4, 8):
            entries.append((d, s)); want.append(wanted(ss, s)[k])
    b, errs, outs = scaled_batch(jx, entries, 1 if ss == "grey" else 3)
    assert errs == [None] * len(entries), errs
    for i, (got, w) in enumerate(zip(outs, want)):
        assert got.shape == w.shape and np.array_equal(got, w), (shape_files(ss)[i // 4][0], entries[i][1], w.shape, int((got != w).sum()))
    assert b.info_value("jpeg_pixel_images") == len(entries)


@pytest.mark.gpu
def test_launches_do_not_depend_on_the_number_of_images(jx):
    datas = transcodes(2)
    few = [(datas[5], s) for s in (1, 2, 4, 8)]
    many = [(datas[k % len(datas)], (1, 2, 4, 8)[k % 4]) for k in range(40)]
    counts = []
    for entries in (few, many):
        b, errs, _ = scaled_batch(jx, entries, 3)
        assert errs == [None] * len(entries) and b.info_value("jpeg_pixel_images") == len(entries)
        counts.append(b.info_value("jpeg_pixel_launches"))
    assert counts[0] == counts[1] == 4, counts          # two kernels x (the group of scale 1, the group of the scaled entries)
    only_scaled, errs, _ = scaled_batch(jx, [(datas[5], 2), (datas[6], 8)], 3)
    assert errs == [None, None] and only_scaled.info_value("jpeg_pixel_launches") == 2


@functools.lru_cache(maxsize=None)
def fresh_float(ss):
    import jpegxl_rs_amd as jx
    outs = float_decode(jx.BatchDecoder(), transcodes(ss))
    for o in outs:
        o.setflags(write=False)
    return outs


# ---- the zeroing -------------------------------------------------------------------------------------------------------------------------------
# A decode that leaves dwords behind shows only if the NEXT user of the planes has other content at the same offsets: the HF stage writes its non-zero coefficients over
# whatever is there, so the same file again hides every leftover.  Hence the twins: for every file a flat picture of the same size and sampling — the same frame layout,
# so the refilled batch keeps its planes without a dense clear, and no AC coefficient at all, so every dword a scaled decode left behind is a wrong pixel in the twin.
W2, H2 = 300, 280


@functools.lru_cache(maxsize=None)
def dense_and_twins(ss):
    """(files, their flat twins): the shape files and a quality-100 300x280 picture (dense coefficient planes), then flat pictures of the same sizes, in the same order"""
    files = [d for _, d in shape_files(ss)] + [make_jpeg(JC.photo(W2, H2, seed=77), ss, 100)]
    j = J.parse_jpeg(files[-1])
    for c in range(len(j.components)):
        ac = np.asarray(j.coef[c]).reshape(-1, 64)[:, 1:]
        assert (ac != 0).mean() > 0.5, (c, float((ac != 0).mean()))                         # most dwords of its planes are written, in every row and column of a block
    twins = []
    for d in files:
        j = J.parse_jpeg(d)
        t = make_jpeg(np.full((j.height, j.width, 3), 120, np.uint8), ss, 85)
        assert all(not np.asarray(c).reshape(-1, 64)[:, 1:].any() for c in J.parse_jpeg(t).coef)
        twins.append(t)
    return files, twins


@functools.lru_cache(maxsize=None)
def twin_references(ss):
    """(transcodes of the files, transcodes of the twins, the twins' float decode on a fresh batch, Pillow's pictures of the twins)"""
    import jpegxl_rs_amd as jx
    files, twins = dense_and_twins(ss)
    tf, tt = [J.transcode(d) for d in files], [J.transcode(d) for d in twins]
    fresh = float_decode(jx.BatchDecoder(), tt)
    for o in fresh:
        o.setflags(write=False)
    return tf, tt, fresh, [pillow(d) for d in twins]


@pytest.mark.gpu
@pytest.mark.parametrize("ss", (2, 0))
@pytest.mark.parametrize("s", SCALES)
def test_scaled_decode_leaves_clean_planes(jx, ss, s):
    """what catches dwords left unzeroed — the columns and rows a reduced transform ignores, all of a block's AC at n = 1: the batch is refilled with the flat twins"""
    files, _ = dense_and_twins(ss)
    tf, tt, fresh, twin_px = twin_references(ss)
    b = jx.BatchDecoder()

    def scaled_decode():
        for d in tf:
            b.add(d, num_channels=3, jpeg_scale=s)
        assert b.decode_jpeg_pixels() == [None] * len(tf)

    scaled_decode()
    for i, d in enumerate(files):
        w = pillow_scaled(d, s)
        w = restate_scaled(d, s) if w is None else w
        assert np.array_equal(b.output(i).reshape(w.shape), w), i
    b.reset()
    for i, (got, w) in enumerate(zip(float_decode(b, tt), fresh)):                           # decode(): the float path over the same planes
        assert np.array_equal(got, w), (i, int((got != w).sum()))
    b.reset()
    scaled_decode()
    b.reset()
    for d in tt:
        b.add(d, num_channels=3)
    assert b.decode_jpeg_pixels() == [None] * len(tt)                                       # decode_jpeg_pixels() at scale 1
    for i, w in enumerate(twin_px):
        assert np.array_equal(b.output(i).reshape(w.shape), w), i
    assert (twin_px[-1] == twin_px[-1][0, 0]).all()                                         # (the twins are flat: any leftover coefficient is a visible pixel)


@pytest.mark.gpu
@pytest.mark.parametrize("s", SCALES)
def test_scaled_jobs_leave_clean_coefficient_sets(jx, s):
    """test_jpeg_pixel_jobs.test_coefficient_sets_stay_clean with scaled jobs: dense 4:4:4 and 4:2:0 transcodes at scale s alternate with a flat and a textured XYB stream of
    the same size over the three shared coefficient sets of one pipeline, no wait in between; every plain result is the BatchDecoder's, the flat one stays one colour"""
    img = JC.photo(W2, H2, seed=77)
    q444, q420 = make_jpeg(img, 0, 100), make_jpeg(img, 2, 100)
    t444, t420 = J.transcode(q444), J.transcode(q420)
    flat = S.encode_vardct(np.full((H2, W2, 3), 120, np.uint8), seed=2, strategy_mix=0, epf_iters=0, gab=0)
    textured = S.encode_vardct(S.synthetic_image(8, W2, H2), seed=2, strategy_mix=0, epf_iters=0, gab=0)
    ref_flat, ref_tex = float_decode(jx.BatchDecoder(), [flat])[0], float_decode(jx.BatchDecoder(), [textured])[0]
    px = ref_flat.reshape(H2, W2, 3)
    assert (px == px[0, 0]).all()
    p = jx.Pipeline(0, jobs_in_flight=4, lf_streams=2, hf_streams=2, prepare_threads=2, parse_threads=2, reserve_frames=2, reserve_width=512, reserve_height=512)
    try:
        sets = p.info("coefficient_sets")
        assert sets == 3
        cycle = [(t444, pillow_scaled(q444, s), True), (flat, ref_flat, False), (t420, pillow_scaled(q420, s), True), (textured, ref_tex, False)]
        plan = [cycle[k % 4] for k in range(3 * sets + 1 + 2)]                              # (every set sees scaled -> plain and plain -> scaled)
        jobs = []
        for data, want, exact in plan:                                                      # no wait in between
            buf = jx.PinnedBuffer(want.size)
            kw = dict(jpeg_pixels=True, jpeg_scale=s) if exact else {}
            jobs.append((p.submit([data], "uint8", 3, host_ptrs=[buf.ptr], capacities=[want.size], **kw), buf, want, exact))
        for n, (t, buf, want, exact) in enumerate(jobs):
            st, _ = p.wait(t, check=False)
            assert st == [0], (n, jx.last_error())
            got = np.array(buf.array)
            assert np.array_equal(got, want.reshape(-1)), (n, "scaled" if exact else "plain", int((got != want.reshape(-1)).sum()))
            if want is ref_flat:
                assert (got.reshape(H2, W2, 3) == px[0, 0]).all(), n
        assert p.info("private_plane_jobs") == 0                                            # every job ran on the shared sets
    finally:
        p.close()


@pytest.mark.gpu
def test_decode_fails_a_scaled_output_alone(jx):
    """decode() writes the other images; finish() names the image whose output only the libjpeg-exact decode writes, and nothing is written outside its destination"""
    import torch
    datas = transcodes(2)
    d = datas[9]                                         # 67x41
    fresh = fresh_float(2)[9]
    b = jx.BatchDecoder()
    size = jx.image_out_size(d, num_channels=3, jpeg_scale=2)[1]
    t = torch.full((size + EXTRA,), FILL, dtype=torch.uint8, device="cuda:0")
    b.add(d, num_channels=3)
    b.add(d, num_channels=3, device_ptr=t.data_ptr() + FRONT, jpeg_scale=2)
    b.prepare(); b.decode()
    with pytest.raises(jx.DecodeError, match="image 1 has an output with jpeg_scale 2"):
        b.finish()
    torch.cuda.synchronize()
    whole = t.cpu().numpy()
    assert (whole[:FRONT] == FILL).all() and (whole[FRONT + size:] == FILL).all()
    assert np.array_equal(b.output(0), fresh)
    assert b.decode_jpeg_pixels() == [None, None]
    assert np.array_equal(t.cpu().numpy()[FRONT:FRONT + size].reshape(wanted(2, 2)[9].shape), wanted(2, 2)[9])
    assert np.array_equal(b.output(0).reshape(wanted(2, 1)[9].shape), wanted(2, 1)[9])


@pytest.mark.gpu
def test_formats_follow_from_the_integers(jx):
    ss, k = 1, [n for n, _ in shape_files(1)].index("67x41")
    data = transcodes(ss)[k]
    LE = jx.JXL_LITTLE_ENDIAN
    SC, BI = [2.0, 0.5, 4.0, 1.0], [-1.0, 0.25, -0.5, 0.0]
    specs = [dict(dtype="uint16", num_channels=3, endianness=LE), dict(dtype="float32", num_channels=3, endianness=LE),
             dict(dtype="float16", num_channels=3, endianness=LE, planar=True, scale=SC, bias=BI), dict(dtype="uint8", num_channels=4, align=64),
             dict(dtype="float32", num_channels=4, endianness=LE, planar=True, align=16, scale=SC, bias=BI)]
    items, want = [], []
    for s in (2, 8):
        for sp in specs:
            items.append((data, dict(sp, jpeg_scale=s))); want.append((wanted(ss, s)[k], sp))
    b, errs, dests = decode_items(jx, items)
    assert errs == [None] * len(items), errs
    for n, ((got, size), (pic, sp)) in enumerate(zip(dests, want)):
        exp = expected_dest(jx, np.ascontiguousarray(pic), size, **sp)
        assert np.array_equal(got, exp), (n, sp, int((got != exp).sum()))
    pic = wanted(ss, 2)[k]
    assert pic.shape == (21, 34, 3)
    assert np.array_equal(dests[0][0][FRONT:FRONT + dests[0][1]].view("<u2").reshape(pic.shape), pic.astype(np.uint16) * 257)
    # orientation 6 applies to the scaled picture
    S.set_orientation(6)
    try:
        turned = J.transcode(shape_files(ss)[k][1])
    finally:
        S.set_orientation(1)
    _, errs, dests = decode_items(jx, [(turned, dict(dtype="uint8", num_channels=3, jpeg_scale=4))])
    pic = np.ascontiguousarray(np.rot90(wanted(ss, 4)[k], -1))
    assert errs == [None] and np.array_equal(dests[0][0], expected_dest(jx, pic, dests[0][1], dtype="uint8", num_channels=3))


@pytest.mark.gpu
def test_resampled_output_of_a_scaled_source(jx):
    k = [n for n, _ in shape_files(2)].index("300x280")
    jpeg, data = shape_files(2)[k][1], transcodes(2)[k]
    f32 = dict(dtype="float32", num_channels=3, endianness=jx.JXL_LITTLE_ENDIAN)
    crops = {2: (50, 40, 100, 100), 4: (0, 10, 60, 60)}       # 150 x 140: touches the right and the bottom edge; 75 x 70: the left and the bottom edge
    items, meta = [], []
    for s in (2, 4):
        src = restate_scaled(jpeg, s)
        assert np.array_equal(src, wanted(2, s)[k]) and src.shape == (cdiv(280, s), cdiv(300, s), 3)
        x0, y0, cw, ch = crops[s]
        assert x0 + cw == src.shape[1] or x0 == 0
        assert y0 + ch == src.shape[0]
        rect = (src.astype(np.float32) * np.float32(1.0 / 255))[y0:y0 + ch, x0:x0 + cw]
        for name, mirror in (("bilinear", False), ("bicubic", True)):
            items.append((data, dict(f32, resize=(48, 32), crop=crops[s], filter=name, mirror=mirror, jpeg_scale=s))); meta.append((rect, name, mirror, s))
    b, errs, dests = decode_items(jx, items)
    assert errs == [None] * len(items), errs
    for (got, size), (rect, name, mirror, s) in zip(dests, meta):
        assert size == 48 * 32 * 3 * 4 and (got[:FRONT] == FILL).all() and (got[FRONT + size:] == FILL).all()
        out = got[FRONT:FRONT + size].view("<f4").reshape(32, 48, 3)
        want, (tx, ty), (lx, ly) = resample(rect, (48, 32), name)
        if mirror:
            want = want[:, ::-1]
        bound = (tx + ty + 8) * 2.0 ** -24 * lx * ly * float(np.abs(rect).max())
        err = float(np.abs(out.astype(np.float64) - want).max())
        print("scale", s, name, "taps", (tx, ty), "sum |w|", (lx, ly), "max error", err, "bound", bound)
        assert np.isfinite(out).all() and err <= bound, (s, name, err, bound)


def xyb_stream(w=40, h=24, seed=3):
    return S.encode_vardct(S.synthetic_image(seed, w, h), seed=2, strategy_mix=0, epf_iters=0, gab=0)


@pytest.mark.gpu
def test_scaled_jobs_of_a_pipeline(jx):
    import torch
    jpegs = [make_jpeg(JC.photo(90, 70, seed=1), "grey", 85), make_jpeg(JC.photo(130, 77, seed=2), 0, 90), make_jpeg(JC.photo(101, 64, seed=3), 1, 80),
             make_jpeg(JC.photo(203, 139, seed=4), 2, 75), make_jpeg(JC.photo(67, 41, seed=5), 2, 95)]
    datas = [J.transcode(d) for d in jpegs]
    n = len(datas)
    LE = jx.JXL_LITTLE_ENDIAN
    lay = dict(planar=True, resize=(48, 32))
    b, errs, dests = decode_items(jx, [(d, dict(dtype="float32", num_channels=3, endianness=LE, jpeg_scale=2, **lay)) for d in datas])
    assert errs == [None] * n, errs
    one = 3 * 32 * 48 * 4
    refs = [d[FRONT:FRONT + m].copy() for d, m in dests]
    assert [r.size for r in refs] == [one] * n
    full_refs = [d[FRONT:FRONT + m].copy() for d, m in decode_items(jx, [(d, dict(dtype="float32", num_channels=3, endianness=LE, **lay)) for d in datas])[2]]
    assert any((a != c).any() for a, c in zip(refs, full_refs))                      # (scaling inside the IDCT gives other samples than resizing the full decode)
    fresh = float_decode(jx.BatchDecoder(), datas)
    p = small_pipeline(jx)
    try:
        out = torch.full((n, 3, 32, 48), 7.0, dtype=torch.float32, device="cuda:0")
        st, _ = p.wait(p.submit(datas, "float32", 3, device_ptrs=[out[k].data_ptr() for k in range(n)], capacities=[one] * n, endianness=LE, jpeg_pixels=True, jpeg_scale=2, **lay))
        torch.cuda.synchronize()
        assert st == [0] * n
        assert np.array_equal(out.cpu().numpy().view(np.uint8).reshape(-1), np.concatenate(refs))
        assert p.info("jpeg_pixel_images") == n and p.info("jpeg_pixel_launches") == 2
        pinned = jx.PinnedBuffer(n * one)
        st, _ = p.wait(p.submit(datas, "float32", 3, host_ptrs=[pinned.ptr + k * one for k in range(n)], capacities=[one] * n, endianness=LE, jpeg_pixels=True, jpeg_scale=2, **lay))
        assert st == [0] * n and np.array_equal(pinned.array, np.concatenate(refs))
        # scaled, plain and scale-1 libjpeg-exact jobs through one pipeline, submitted before any of them is collected
        want = {s: [pillow(d) if s == 1 else pillow_scaled(d, s) for d in jpegs] for s in (1, 4, 8)}
        kinds = [("scaled", 4), ("plain", 1), ("exact", 1), ("scaled", 8), ("plain", 1), ("scaled", 4)]
        tickets = []
        for kind, s in kinds:
            if kind == "plain":
                sizes = [jx.image_out_size(d, "uint8", 3)[1] for d in datas]
            else:
                sizes = [jx.image_out_size(d, "uint8", 3, jpeg_scale=s)[1] for d in datas]
            bufs = [jx.PinnedBuffer(m) for m in sizes]
            kw = dict(jpeg_pixels=True, jpeg_scale=s) if kind == "scaled" else dict(jpeg_pixels=True) if kind == "exact" else {}
            tickets.append((p.submit(datas, "uint8", 3, host_ptrs=[x.ptr for x in bufs], capacities=sizes, **kw), bufs))
        for (kind, s), (t, bufs) in zip(kinds, tickets):
            st, _ = p.wait(t)
            assert st == [0] * n
            for k in range(n):
                got = np.array(bufs[k].array)
                if kind == "plain":
                    assert np.array_equal(got, fresh[k].reshape(-1)), (kind, k)
                else:
                    w = want[s][k]
                    w = np.stack([w] * 3, -1) if w.ndim == 2 else w
                    assert np.array_equal(got.reshape(w.shape), w), (kind, s, k)
        # an XYB image in a scaled job fails alone, with the reason of can_decode_jpeg_pixels
        mixed = [datas[3], xyb_stream(), datas[4]]
        sizes = [jx.image_out_size(mixed[0], "uint8", 3, jpeg_scale=4)[1], 40 * 24 * 3, jx.image_out_size(mixed[2], "uint8", 3, jpeg_scale=4)[1]]
        bufs = [jx.PinnedBuffer(m) for m in sizes]
        st, _ = p.wait(p.submit(mixed, "uint8", 3, host_ptrs=[x.ptr for x in bufs], capacities=sizes, jpeg_pixels=True, jpeg_scale=4), check=False)
        assert st == [0, 1, 0] and jx.last_error().startswith("image 1: " + REFUSAL), (st, jx.last_error())
        for k in (0, 2):
            w = want[4][3 + k // 2]
            assert np.array_equal(np.array(bufs[k].array).reshape(w.shape), w)
        # refused submissions
        with pytest.raises(jx.DecodeError, match="jpeg_scale must be 1, 2, 4 or 8"):
            p.submit(datas, "uint8", 3, host_ptrs=[x.ptr for x in bufs[:1]] * n, jpeg_pixels=True, jpeg_scale=3)
        with pytest.raises(jx.DecodeError, match="not a libjpeg-exact"):
            p.submit(datas, "uint8", 3, host_ptrs=[x.ptr for x in bufs[:1]] * n, jpeg_scale=2)
        with pytest.raises(jx.DecodeError, match="downscale 8"):
            p.submit(datas, "uint8", 3, host_ptrs=[x.ptr for x in bufs[:1]] * n, jpeg_pixels=True, jpeg_scale=2, downscale=8)
    finally:
        p.close()


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
    # (a stream the host parser refuses never enters a batch; the mutations sit behind the headers, so what parses is as eligible as the good file)
    keep = [jxl]
    for d in mutated:
        try:
            jx.BatchDecoder(-1).add(d, num_channels=3, jpeg_scale=4)
            keep.append(d)
        except jx.DecodeError as e:
            assert str(e)
    b = jx.BatchDecoder()
    index = [b.add(d, num_channels=3, jpeg_scale=4) for d in keep]
    assert index[0] == 0 and len(keep) > 1
    errs = b.decode_jpeg_pixels()
    want = pillow_scaled(good, 4)
    assert want.shape == (15, 25, 3)
    assert errs[0] is None and np.array_equal(b.output(0).reshape(want.shape), want)
    for i in index[1:]:
        assert errs[i] is None or errs[i]
        assert b.output(i).size == want.size                                                # an error, or an output of the right size
    assert b.info_value("jpeg_pixel_images") == sum(1 for e in errs if e is None)
    again, errs2, outs = scaled_batch(jx, [(jxl, 4), (jxl, 1)], 3)
    assert errs2 == [None, None] and np.array_equal(outs[0], want) and np.array_equal(outs[1], pillow(good))
