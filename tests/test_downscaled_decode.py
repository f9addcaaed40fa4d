"""The 1:8 decode (include/jxl_hip.h JxlHipBatchSetOutputScaled / JxlHipPipelineSubmitScaled / JxlHipImageOutSizeScaled; kernels.hip LfOutputKernel): a VarDCT
frame's LF image — one sample per 8x8 block, after dequantisation and adaptive smoothing — through the colour transform and the write stage of the full decode, with no
AC coefficient decoded and no IDCT or filter run.

What pins it:
  * against the oracle (tests 2, 3, 5): for frames of 8x8 DCTs only without gaborish and EPF, the oracle's render at the kDC progression step (`dc_only`: every AC
    coefficient zero) is constant over every 8x8 block — asserted on the oracle alone first —, so its samples at [::8, ::8] are the 1:8 picture;
  * without the oracle (tests 4, 5): float64 restatements of inverse opsin + sRGB (the formulas of test_stage_formulas.py) and of the (1/4, 3/4) chroma taps + the
    YCbCr matrix, applied to the LF planes read off the device after a FULL decode of the same stream;
  * the write stage at the small geometry (test 6) by numpy from the f32 keep-orientation 1:8 decode, the scheme of test_write_stage.py;
  * the prefix property, the skipped work, mixed batches / pipelines, refusals and robustness (tests 7 - 10)."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import fixture_bytes
import oracle_lib as O
import synth_lib as S


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


def ulp_diff(a, b):
    ai = a.view(np.int32).astype(np.int64); bi = b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7FFFFFFF), ai); bi = np.where(bi < 0, -(bi & 0x7FFFFFFF), bi)
    return np.abs(ai - bi).max() if a.size else 0


def cdiv(a, b):
    return -(-a // b)


# ---- streams (synthesised once per process) ------------------------------------------------------------------------------------------------
PLAIN_SIZES = [(203, 131), (1030, 520), (2056, 24)]      # one group with ragged sides; several groups; two LF groups (a seam under the smoothing) in the smallest frame that has one


@functools.lru_cache(maxsize=None)
def plain_stream(w, h, orientation=1, num_passes=1):
    """8x8 DCT only, gaborish off, EPF 0, XYB, 4:4:4 (adaptive LF smoothing on)"""
    return S.encode_vardct(S.synthetic_image(100 + w, w, h), seed=w, strategy_mix=0, epf_iters=0, gab=0, orientation=orientation, num_passes=num_passes)


def oracle_stream(w, h):
    """The stream of test 3 for a size.  A frame of one group and one pass is a single section, and the oracle has no kDC step for those (it decodes the section to its
    end): the one-group size is pinned against the oracle with two passes — the TOC then lists the LF part on its own — and, as a one-section frame, through the
    float64 restatement (test_one_section_frame_against_the_defining_formulas) and the write-stage test."""
    return plain_stream(w, h, 1, 2 if (w, h) == (203, 131) else 1)


@functools.lru_cache(maxsize=None)
def general_stream():
    return S.encode_vardct(S.synthetic_image(61, 1030, 520), seed=61, strategy_mix=1, epf_iters=2, gab=1)


@functools.lru_cache(maxsize=None)
def progressive_stream():
    """the 1030x520 three-pass stream of test_progressive.py::test_pass_steps_of_a_progressive_frame"""
    return S.encode_vardct(S.synthetic_image(31, 1030, 520), seed=31, strategy_mix=2, epf_iters=1, gab=1, num_passes=3, pass_ds=1)


@functools.lru_cache(maxsize=None)
def ycbcr_stream(sub):
    return S.encode_ycbcr(S.synthetic_image(71, 291, 227), subsampling=sub, seed=7)


@functools.lru_cache(maxsize=None)
def oracle_dc(data, kind, nch=3):
    """the oracle's kDC render of `data`, (h, w, nch)"""
    return O.decode(data, dc_only=True).image(kind, nch)


def lf_part_end(jxm, data):
    """byte offset behind the LF part (LfGlobal, LfGroups, HfGlobal) of the first frame, from its TOC (JxlHipDebugDescribe)"""
    L = jxm.libjxl()
    L.JxlHipDebugDescribe.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 16)
    assert L.JxlHipDebugDescribe(data, len(data), buf, len(buf)) == 0, jxm.last_error()
    line = [l for l in buf.value.decode().split("\n") if l.startswith("  quantizer")][0]
    return int(dict(t.split("=") for t in line.split() if "=" in t)["lf_part_end"])


def decode8(jxm, data, dtype="uint8", nch=3, **kw):
    """1:8 decode of one image through a BatchDecoder -> (bh, bw, nch) array"""
    b = jxm.BatchDecoder(0)
    b.add(data, dtype, nch, downscale=8, **kw)
    b.prepare(); b.decode(); b.finish()
    info = b.info(0)
    return b.output(0).reshape(cdiv(info.ysize, 8), cdiv(info.xsize, 8), nch)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------------
def test_scaled_output_sizes(jxh):
    """1. image_out_size(downscale=8) = ceil(w / 8) x ceil(h / 8) x channels x sample size with row alignment, the transposing orientations swap the sides;
    other factors are refused; 1 is the call without the keyword."""
    cases = [(plain_stream(203, 131), 203, 131), (plain_stream(1030, 520), 1030, 520), (ycbcr_stream("420"), 291, 227)]
    for data, w, h in cases:
        bw, bh = cdiv(w, 8), cdiv(h, 8)
        for dtype, bps in (("uint8", 1), ("uint16", 2), ("float16", 2), ("float32", 4)):
            for nch in (1, 2, 3, 4):
                for align in (0, 64):
                    info, size = jxh.image_out_size(data, dtype, nch, align=align, downscale=8)
                    assert (info.xsize, info.ysize) == (w, h)                                 # the info stays the full-size image's
                    row = bw * nch * bps
                    stride = row if align <= 1 else cdiv(row, align) * align
                    assert size == stride * (bh - 1) + row, (w, h, dtype, nch, align)
        assert jxh.image_out_size(data, "uint8", 3, downscale=1)[1] == jxh.image_out_size(data, "uint8", 3)[1] == (w * 3) * h
        assert jxh.image_out_size(data, "uint16", 4, align=32, downscale=1)[1] == jxh.image_out_size(data, "uint16", 4, align=32)[1]
        for bad in (3, 0, 2, 16, -8):
            with pytest.raises(jxh.DecodeError):
                jxh.image_out_size(data, "uint8", 3, downscale=bad)
            assert "downscale must be 1 or 8" in jxh.last_error()
    for o in range(1, 9):
        data = plain_stream(203, 131, o)
        info, size = jxh.image_out_size(data, "uint8", 3, align=16, downscale=8)
        ow, oh = (cdiv(131, 8), cdiv(203, 8)) if o > 4 else (cdiv(203, 8), cdiv(131, 8))
        assert size == cdiv(ow * 3, 16) * 16 * (oh - 1) + ow * 3, o
    # a prefix that holds the headers is enough
    assert jxh.image_out_size(plain_stream(1030, 520)[:200], "uint8", 3, downscale=8)[1] == 129 * 3 * 65


def block_spread(img):
    h, w, _ = img.shape
    pad = np.pad(img, ((0, -h % 8), (0, -w % 8), (0, 0)), mode="edge").reshape(cdiv(h, 8), 8, cdiv(w, 8), 8, 3)
    return float((pad.max(axis=(1, 3)) - pad.min(axis=(1, 3))).max())


@pytest.mark.parametrize("which", ["203x131", "1030x520", "2056x24", "ycbcr444"])
def test_oracle_dc_render_is_constant_per_block(which):
    """2. the oracle's kDC render of the streams of tests 3 and 5 is constant over every 8x8 block (max - min == 0 in f32): its [::8, ::8] samples are the 1:8 picture"""
    data = ycbcr_stream("444") if which == "ycbcr444" else oracle_stream(*[int(v) for v in which.split("x")])
    assert block_spread(oracle_dc(data, "f32")) == 0.0


def test_oracle_has_no_dc_render_of_a_one_section_frame():
    """2. ... which does not hold for a frame of one group and one pass: the oracle's `dc_only` leaves such a frame as it is (the whole section is decoded), so that
    stream is pinned through the restatement of test 4 instead (PARITY.md)"""
    data = plain_stream(203, 131)
    dc = oracle_dc(data, "f32")
    assert block_spread(dc) > 0 and np.array_equal(dc, O.decode(data).image("f32", 3))


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", PLAIN_SIZES)
def test_exact_against_the_oracle(jx, w, h):
    """3. u8 / u16 equal, f32 <= 1 ULP against the oracle's kDC render sampled at [::8, ::8]"""
    data = oracle_stream(w, h)
    for dtype, kind in (("uint8", "u8"), ("uint16", "u16"), ("float32", "f32")):
        got = decode8(jx, data, dtype)
        want = np.ascontiguousarray(oracle_dc(data, kind)[::8, ::8])
        assert got.shape == want.shape == (cdiv(h, 8), cdiv(w, 8), 3)
        if dtype == "float32":
            assert ulp_diff(np.ascontiguousarray(got), want) <= 1
        else:
            assert np.array_equal(got, want), f"{dtype}: {int((got != want).sum())} of {got.size} samples differ"


def srgb_oetf(v):
    a = np.abs(v)
    return np.sign(v) * np.where(a <= 0.0031308, a * 12.92, 1.055 * np.power(a, 1 / 2.4) - 0.055)


def xyb_to_linear(X, Y, B):
    """stage_xyb.cc / opsin_params.h in float64, as tests/test_stage_formulas.py::test_inverse_opsin_and_transfer_function states it"""
    bias = -0.0037930732552754493
    cb = np.cbrt(bias)
    mixed = [np.power(Y + X - cb, 3) + bias, np.power(Y - X - cb, 3) + bias, np.power(B - cb, 3) + bias]
    inv = np.array([[11.031566901960783, -9.866943921568629, -0.16462299647058826],
                    [-3.254147380392157, 4.418770392156863, -0.16462299647058826],
                    [-3.6588512862745097, 2.7129230470588235, 1.9459282392156863]])
    return np.stack([sum(inv[r, k] * mixed[k] for k in range(3)) for r in range(3)], axis=-1)


@pytest.mark.gpu
@pytest.mark.parametrize("tf", ["srgb", "linear"])
def test_general_frame_against_the_defining_formulas(jx, tf):
    """4. mixed transforms, gaborish, EPF 2: the 1:8 picture is inverse opsin + transfer function of the smoothed LF planes ("lf_smooth", read off the device after a
    FULL decode of the same stream), within the tolerance PARITY.md gives for that stage (1.5e-5 sRGB, 4e-6 linear) — and it is not the full decode subsampled, because
    gaborish and EPF are not applied."""
    if tf == "linear":
        S.set_color(1, 1, 8)
    try:
        data = S.encode_vardct(S.synthetic_image(61, 1030, 520), seed=61, strategy_mix=1, epf_iters=2, gab=1) if tf == "linear" else general_stream()
    finally:
        S.set_color()
    full = jx.BatchDecoder(0)
    full.add(data, "float32", 3)
    full.prepare(); full.decode(); full.finish()
    bw, bh = full.info_value("frame0_bw"), full.info_value("frame0_bh")
    assert (bw, bh) == (129, 65)
    X, Y, B = [full.debug_read(0, "lf_smooth", c).reshape(bh, bw).astype(np.float64) for c in range(3)]
    lin = xyb_to_linear(X, Y, B)
    want = lin if tf == "linear" else srgb_oetf(lin)
    got = decode8(jx, data, "float32").astype(np.float64)
    dev = float(np.abs(got - want).max())
    print(f"\n[1:8 general frame, {tf}] max |kernel - float64 restatement| = {dev:.3e}")
    assert dev <= (4e-6 if tf == "linear" else 1.5e-5), dev
    sub = full.output(0).reshape(520, 1030, 3)[::8, ::8].astype(np.float64)
    assert np.abs(sub - got).max() > 1e-3                           # the filters are not applied: the test looks at the LF path


@pytest.mark.gpu
def test_one_section_frame_against_the_defining_formulas(jx):
    """3 / 4. the 203 x 131 frame of one group and one pass (a single section: HfGlobal is found behind the LF stage's pre-run) has no kDC render in the oracle; its f32
    1:8 picture is pinned through the float64 restatement at that stage's tolerance, every other format follows exactly from the f32 one (write-stage test)"""
    data = plain_stream(203, 131)
    full = jx.BatchDecoder(0)
    full.add(data, "float32", 3)
    full.prepare(); full.decode(); full.finish()
    X, Y, B = [full.debug_read(0, "lf_smooth", c).reshape(17, 26).astype(np.float64) for c in range(3)]
    got = decode8(jx, data, "float32").astype(np.float64)
    dev = float(np.abs(got - srgb_oetf(xyb_to_linear(X, Y, B))).max())
    print(f"\n[1:8 one-section frame] max |kernel - float64 restatement| = {dev:.3e}")
    assert dev <= 1.5e-5, dev


def upsample_taps(p, hs, vs, w, h):
    """float64 restatement of the (1/4, 3/4) chroma upsampling (stage_chroma_upsampling.cc), horizontal then vertical, neighbours clamped at the channel's own
    edges: p = the channel (ceil(h / 2^vs), ceil(w / 2^hs)) -> (h, w)"""
    p = p.astype(np.float64)
    if hs:
        x = np.arange(w); sx = x >> 1
        nb = np.where(x & 1, np.minimum(sx + 1, p.shape[1] - 1), np.maximum(sx - 1, 0))
        p = 0.75 * p[:, sx] + 0.25 * p[:, nb]
    if vs:
        y = np.arange(h); sy = y >> 1
        nb = np.where(y & 1, np.minimum(sy + 1, p.shape[0] - 1), np.maximum(sy - 1, 0))
        p = 0.75 * p[sy] + 0.25 * p[nb]
    return p


def ycbcr_to_rgb(cb, y, cr):
    yb = y + 128.0 / 255
    return np.stack([yb + 1.402 * cr, yb - (0.114 * 1.772 / 0.587) * cb - (0.299 * 1.402 / 0.587) * cr, yb + 1.772 * cb], axis=-1)


SHIFTS = {"420": ((1, 1), (0, 0), (1, 1)), "422": ((1, 0), (0, 0), (1, 0))}      # (hs, vs) of the channels Cb, Y, Cr


@pytest.mark.gpu
@pytest.mark.parametrize("sub", ["420", "422"])
def test_subsampled_ycbcr_against_the_defining_formulas(jx, sub):
    """5. chroma-subsampled frames of odd size (291 x 227: 37 x 29 blocks): f32 against the float64 taps + YCbCr matrix on the LF planes.  The bound is twice the largest
    deviation of the FULL-RESOLUTION subsampled path (OutputKernel's branch) from the same restatement on the same stream — the same arithmetic on another grid —,
    measured here and recorded in PARITY.md."""
    data = ycbcr_stream(sub)
    w, h = 291, 227
    lw, lh = cdiv(w, 8), cdiv(h, 8)
    full = jx.BatchDecoder(0)
    full.add(data, "float32", 3)
    full.prepare(); full.decode(); full.finish()
    bw, bh = full.info_value("frame0_bw"), full.info_value("frame0_bh")
    lf, px = [], []
    for c, (hs, vs) in enumerate(SHIFTS[sub]):
        plane = full.debug_read(0, "lf", c).reshape(bh, bw)
        lf.append(upsample_taps(plane[:cdiv(lh, 1 << vs), :cdiv(lw, 1 << hs)], hs, vs, lw, lh))
        plane = full.debug_read(0, "plane_a", c).reshape(bh * 8, bw * 8)
        px.append(upsample_taps(plane[:cdiv(h, 1 << vs), :cdiv(w, 1 << hs)], hs, vs, w, h))
    full_dev = float(np.abs(full.output(0).reshape(h, w, 3).astype(np.float64) - ycbcr_to_rgb(*px)).max())
    got = decode8(jx, data, "float32")
    assert got.shape == (lh, lw, 3)
    dev = float(np.abs(got.astype(np.float64) - ycbcr_to_rgb(*lf)).max())
    print(f"\n[1:8 YCbCr {sub}] full-resolution path vs float64: {full_dev:.3e}; 1:8 path vs float64: {dev:.3e} (bound {2 * full_dev:.3e})")
    assert full_dev > 0 and dev <= 2 * full_dev, (dev, full_dev)


@pytest.mark.gpu
def test_ycbcr_444_equals_the_oracle(jx):
    """5. a 4:4:4 YCbCr frame (8x8 DCT, no filters): byte-equal to the oracle's kDC render at [::8, ::8]"""
    data = ycbcr_stream("444")
    got = decode8(jx, data, "uint8")
    want = oracle_dc(data, "u8")[::8, ::8]
    assert got.shape == want.shape == (29, 37, 3) and np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("orientation", range(1, 9))
def test_write_stage_at_the_small_geometry(jx, orientation):
    """6. every output type x byte order x channel count x row alignment {0, 64} of one 203 x 131 stream with the given orientation, all in one batch, each equal to
    numpy applied to the f32 keep-orientation 4-channel 1:8 decode of the same stream (tests/test_write_stage.py expected_output); the alpha slot is full scale."""
    from test_write_stage import DTYPES, expected_output
    data = plain_stream(203, 131, orientation)
    bw, bh = 26, 17
    b = jx.BatchDecoder(0)
    b.set_option("keep_orientation", 1)
    b.add(data, "float32", 4, downscale=8)
    b.set_option("keep_orientation", 0)
    combos = [(d, e, n, a) for d in DTYPES for e in (jx.Endianness.Little, jx.Endianness.Big) for n in (1, 2, 3, 4) for a in (0, 64)]
    for d, e, n, a in combos:
        b.add(data, d, n, endianness=e, align=a, downscale=8)
    b.prepare(); b.decode(); b.finish()
    L = jx.libjxl()

    def raw(i):
        out = np.zeros(b.out_size(i), np.uint8)
        assert L.JxlHipBatchCopyOutput(b._h, i, out.ctypes.data, out.size, None) == 0
        return out

    ref = raw(0).view(np.float32).reshape(bh, bw, 4)
    assert np.all(ref[..., 3] == 1.0)
    for i, (d, e, n, a) in enumerate(combos, start=1):
        want = expected_output(ref, dtype=d, nch=n, big_endian=e == jx.Endianness.Big, align=a, orientation=orientation)
        got = raw(i)
        row = want.shape[1] if a <= 1 else (bh if orientation > 4 else bw) * n * np.dtype(d).itemsize
        assert got.size == want.shape[1] * (want.shape[0] - 1) + row, (d, e, n, a)
        got = np.concatenate([got, np.zeros(want.size - got.size, np.uint8)]).reshape(want.shape)
        assert np.array_equal(got[:, :row], want[:, :row]), (d, e, n, a)


@pytest.mark.gpu
def test_a_prefix_decodes_to_the_same_thumbnail(jx):
    """7. the three-pass stream cut at 45 % and 95 % of its bytes — both behind the LF part, by the TOC — decodes at 1:8 to the bytes of the whole file; a cut inside the
    LF part fails with "truncated"; a prefix that is not decoded at 1:8 fails, too"""
    data = progressive_stream()
    end = lf_part_end(jx, data)
    whole = decode8(jx, data, "uint8")
    assert whole.shape == (65, 129, 3)
    for frac in (0.45, 0.95):
        cut = int(len(data) * frac)
        assert end < cut < len(data)
        assert np.array_equal(decode8(jx, data[:cut], "uint8"), whole), frac
    assert np.array_equal(decode8(jx, data[:end], "uint8"), whole)                  # exactly the LF part
    for cut in (end - 1, end // 2):
        with pytest.raises(jx.DecodeError):
            decode8(jx, data[:cut], "uint8")
        assert "truncated" in jx.last_error()
    # through a pipeline, into host memory
    size = jx.image_out_size(data[:200], "uint8", 3, downscale=8)[1]
    bufs = [jx.PinnedBuffer(size) for _ in range(3)]
    p = jx.Pipeline(0, jobs_in_flight=2)
    try:
        t = p.submit([data[: int(len(data) * 0.45)], data[: end // 2], data], "uint8", 3, host_ptrs=[x.ptr for x in bufs], downscale=8)
        st, _ = p.wait(t, check=False)
        assert st == [0, 1, 0] and "truncated" in jx.last_error()
        assert np.array_equal(bufs[0].array.reshape(whole.shape), whole) and np.array_equal(bufs[2].array.reshape(whole.shape), whole)
    finally:
        p.close()
    b = jx.BatchDecoder(0)
    b.set_option("allow_partial", 1)
    b.add(data[: int(len(data) * 0.45)], "uint8", 3)                                # let in, but not decoded at 1:8
    with pytest.raises(jx.DecodeError):
        b.prepare()
    assert "truncated" in jx.last_error()


@pytest.mark.gpu
def test_skipped_work(jx):
    """8. a batch of scaled frames only: no algorithmic bytes for the HF stage, the IDCT and the filters, less device memory than the same images unscaled, no AC
    coefficient decoded"""
    streams = [general_stream(), plain_stream(1030, 520), progressive_stream()]
    scaled, plain = jx.BatchDecoder(0), jx.BatchDecoder(0)
    scaled.add_many(streams, "uint8", 3, downscale=8)
    plain.add_many(streams, "uint8", 3)
    scaled.prepare(); plain.prepare()
    sb, pb = scaled.stage_bytes, plain.stage_bytes
    assert sb["hf"] == 0 and sb["idct"] == 0 and sb["filter"] == 0 and sb["lf"] == pb["lf"] and sb["lfpost"] == pb["lfpost"]
    assert sb["out"] == 3 * 129 * 65 * (12 + 3)
    assert pb["idct"] > 0 and pb["hf"] > 0
    assert scaled.device_bytes < plain.device_bytes
    # (the planes of three 1030 x 520 frames alone: 12 B/px of pixel planes and 12 B/px of coefficient planes)
    assert plain.device_bytes - scaled.device_bytes >= 3 * 1030 * 520 * 24
    scaled.decode(); scaled.finish()
    plain.decode(); plain.finish()
    assert scaled.info_value("hf_nonzeros") == 0 and plain.info_value("hf_nonzeros") > 0
    assert scaled.stage_bytes["hf"] == 0
    for i in range(3):
        assert scaled.output(i).size == 129 * 65 * 3


@pytest.mark.gpu
def test_mixed_batch_and_pipeline(jx):
    """9. scaled and unscaled images side by side in a batch; scaled, unscaled and scaled jobs through one pipeline (shared planes, coefficient-set rotation); what the
    1:8 decode does not take fails alone"""
    data = plain_stream(1030, 520)
    sample = fixture_bytes("sample.jxl")
    small = np.ascontiguousarray(oracle_dc(data, "u8")[::8, ::8])
    alone = jx.BatchDecoder(0)
    alone.add(data, "uint8", 3); alone.add(sample, "uint8", 4)
    alone.prepare(); alone.decode(); alone.finish()
    want_full, want_sample = alone.output(0), alone.output(1)
    assert np.array_equal(want_full, O.decode(data).pixels("u8", 3))
    b = jx.BatchDecoder(0)
    b.add(data, "uint8", 3, downscale=8); b.add(data, "uint8", 3); b.add(sample, "uint8", 4)
    b.prepare(); b.decode(); b.finish()
    assert np.array_equal(b.output(0).reshape(small.shape), small)
    assert np.array_equal(b.output(1), want_full) and np.array_equal(b.output(2), want_sample)
    with pytest.raises(jx.DecodeError):
        b.add(data, "uint8", 3, downscale=4)
    assert "downscale must be 1 or 8" in jx.last_error()

    gen = general_stream()
    gen_small = decode8(jx, gen, "uint8")
    gen_full = O.decode(gen).pixels("u8", 3)
    s_small, s_full = small.size, want_full.size
    p = jx.Pipeline(0, jobs_in_flight=3)
    try:
        outs = [[jx.PinnedBuffer(n), jx.PinnedBuffer(n)] for n in (s_small, s_full, s_small)]
        tickets = [p.submit([data, gen], "uint8", 3, host_ptrs=[x.ptr for x in outs[k]], capacities=[x.nbytes for x in outs[k]], downscale=(8, 1, 8)[k]) for k in range(3)]
        for t in tickets:
            assert p.wait(t)[0] == [0, 0]
        for k in (0, 2):
            assert np.array_equal(outs[k][0].array.reshape(small.shape), small) and np.array_equal(outs[k][1].array.reshape(gen_small.shape), gen_small)
        assert np.array_equal(outs[1][0].array, want_full) and np.array_equal(outs[1][1].array, gen_full)
        # refusals: a Modular image, an RGBA image (VarDCT with alpha) and a two-frame image fail alone, the VarDCT image beside them decodes
        img = S.synthetic_image(5, 200, 136)
        rgba = S.encode_vardct(img, seed=5, alpha=np.full((136, 200), 200, np.uint8))
        two = S.encode_vardct_frame(img, S.frame(is_last=0, save_as_reference=1), seed=6) + S.encode_vardct_frame(img, S.frame(emit=1, blend_mode=2, blend_source=1), seed=7)
        big = [jx.PinnedBuffer(1 << 20) for _ in range(4)]
        t = p.submit([sample, rgba, data, two], "uint8", 0, host_ptrs=[x.ptr for x in big], downscale=8)
        st, _ = p.wait(t, check=False)
        assert st == [1, 1, 0, 1], st
        assert jx.last_error().startswith("image 0: unsupported: downscaled decode of")
        assert np.array_equal(big[2].array[:small.size].reshape(small.shape), small)
    finally:
        p.close()
    for bad in (sample, rgba, two):
        with pytest.raises(jx.DecodeError):
            jx.BatchDecoder(0).add(bad, "uint8", 0, downscale=8)
        assert jx.last_error().startswith("unsupported: downscaled decode of"), jx.last_error()
    L = jx.libjxl()
    fmt = jx.JxlPixelFormat(3, jx.JXL_TYPE_UINT8, jx.JXL_NATIVE_ENDIAN, 0)
    ptrs = (C.c_char_p * 1)(data); sizes = (C.c_size_t * 1)(len(data)); host = (C.c_void_p * 1)(big[0].ptr)
    p2 = jx.Pipeline(0, jobs_in_flight=2)
    try:
        assert L.JxlHipPipelineSubmitScaled(p2._h, ptrs, sizes, 1, C.byref(fmt), None, host, None, 3) == -1 and "downscale must be 1 or 8" in jx.last_error()
    finally:
        p2.close()


@pytest.mark.gpu
def test_damaged_lf_parts_fail_cleanly_or_decode(jx):
    """10. bit flips and truncations over the LF part of one stream (fixed seed, the mutations of test_round6_wave.py's loop): an error or an output of the right size;
    the decoder then decodes the clean stream correctly"""
    data = plain_stream(1030, 520)
    end = lf_part_end(jx, data)
    rng = np.random.default_rng(808)
    outcomes = {"error": 0, "decoded": 0}
    trials = 36
    for trial in range(trials):
        bad = bytearray(data)
        for pos in rng.integers(end // 8, end, 1 + trial % 4):                   # (past the headers: the decode reaches the GPU)
            bad[pos] ^= 1 << int(rng.integers(0, 8))
        if trial % 6 == 5:
            bad = bad[: int(rng.integers(end // 2, len(bad)))]
        try:
            px = decode8(jx, bytes(bad), "uint8")
            assert px.shape == (65, 129, 3)
            outcomes["decoded"] += 1
        except jx.DecodeError:
            outcomes["error"] += 1
    assert outcomes["error"] > 0 and outcomes["error"] + outcomes["decoded"] == trials
    assert np.array_equal(decode8(jx, data, "uint8"), oracle_dc(data, "u8")[::8, ::8])
