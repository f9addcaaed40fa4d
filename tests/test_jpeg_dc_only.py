"""libjpeg's 1/8 decode from the DC terms alone (include/jxl_hip.h JxlHipBatchJpegDcOnly, JxlHipLfPartSize; csrc/jpeg_pixels.hip JpegDcOutKernel): at jpeg_scale = 8 grey,
4:4:4 and 4:2:2 transcodes take the 1 x 1 IDCT for every component, so the picture is a function of the DC terms the LF stage writes — the HF stage, the IDCT and the
planes are left out for such an image, and a prefix of the file that holds the LF part of its frame is enough.  The yardstick is that of test_jpeg_scaled_pixels.py:
Pillow's draft() picture (`restate_scaled` where a side is shorter than 8), np.array_equal throughout; formats, layouts and resamples are pinned against the same call
on the general path (set_option("jpeg_dc_only", 0)), guard bytes included."""
import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_tools as J
import synth_lib as S
from test_downscaled_decode import lf_part_end
from test_jpeg_exact_pixels import EXTRA, FILL, FRONT, float_decode, make_jpeg, strip_boxes
from test_jpeg_scaled_pixels import (dense_and_twins, pillow_scaled, restate_scaled, scaled_batch, shape_files, small_pipeline, transcodes, twin_references, wanted)

DC_SAMPLINGS = (0, 1, "grey")
BIG = ("300x280", "520x264")


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


def named(ss, name):
    """(transcode in its container, the bare codestream, Pillow's picture at scale 8) of one of shape_files(ss)"""
    k = [n for n, _ in shape_files(ss)].index(name)
    data = transcodes(ss)[k]
    return data, strip_boxes(data)[1], wanted(ss, 8)[k]


def payload_offset(data, bare):
    """where the codestream starts in the container (one jxlc box behind the jbrd box)"""
    at = data.find(bare[:32])
    assert at > 0 and data[at:] == bare
    return at


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------
def test_lf_part_size(jxh):
    for ss in (0, 1, 2, "grey"):
        for name in BIG:
            data, bare, _ = named(ss, name)
            off = payload_offset(data, bare)
            assert off == (300 if ss == "grey" else 520), (ss, off)
            for d, base in ((data, off), (bare, 0)):
                n = jxh.lf_part_size(d)
                assert n == base + lf_part_end(jxh, d) and 0 < n < len(d), (ss, name, base, n)
                print(ss, name, "container" if base else "bare", "LF part", n, "of", len(d), "bytes: %.1f %%" % (100.0 * n / len(d)))
                assert n < 0.3 * len(d)
                b = jxh.BatchDecoder(-1)
                b.set_option("allow_partial", 1)
                assert b.add(d[:n]) == 0
                with pytest.raises(jxh.DecodeError, match="truncated"):
                    b.add(d[:n - 1])
                assert jxh.lf_part_size(d[:n]) == n                           # the same from any prefix that holds the headers and the TOC
            with pytest.raises(jxh.DecodeError, match="truncated"):           # 64 bytes of the container end inside its jbrd box: no codestream byte yet
                jxh.lf_part_size(data[:64])
            assert jxh.lf_part_size(bare[:64]) == jxh.lf_part_size(bare)      # (64 bytes of the bare codestream hold its headers and the TOC of seven sections)
            with pytest.raises(jxh.DecodeError, match="truncated"):
                jxh.lf_part_size(bare[:16])
        data, bare, _ = named(ss, "progressive")                              # 40 x 24: one group, one section
        assert jxh.lf_part_size(data) == 0 and jxh.lf_part_size(bare) == 0


def test_which_images_are_dc_only(jxh):
    L = jxh.libjxl()
    for ss in (0, 1, 2, "grey"):
        data = named(ss, "300x280")[0]
        on, off = jxh.BatchDecoder(-1), jxh.BatchDecoder(-1)
        off.set_option("jpeg_dc_only", 0)
        for s in (1, 2, 4, 8):
            i, k = on.add(data, jpeg_scale=s), off.add(data, jpeg_scale=s)
            assert on.jpeg_dc_only(i) is (s == 8 and ss != 2), (ss, s)
            assert off.jpeg_dc_only(k) is False
        assert L.JxlHipBatchJpegDcOnly(on._h, 99) == 0 and "no such image" in jxh.last_error()
    one = jxh.BatchDecoder(-1)                                                # a one-section frame is DC-only, too (from the whole file)
    assert one.jpeg_dc_only(one.add(named(1, "progressive")[0], jpeg_scale=8))
    plain = jxh.BatchDecoder(-1)
    assert not plain.jpeg_dc_only(plain.add(named(0, "300x280")[0], downscale=8))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def eighth(jx, datas, nc, dc_only=True):
    """the images at jpeg_scale 8 in ONE batch -> (batch, errors, flat outputs)"""
    b = jx.BatchDecoder()
    b.set_option("jpeg_dc_only", 1 if dc_only else 0)
    for d in datas:
        b.add(d, num_channels=nc, jpeg_scale=8)
    errs = b.decode_jpeg_pixels()
    return b, errs, [None if e else b.output(i) for i, e in enumerate(errs)]


@pytest.mark.gpu
@pytest.mark.parametrize("ss", DC_SAMPLINGS)
def test_exact_and_really_skipped(jx, ss):
    datas, want = transcodes(ss), wanted(ss, 8)
    n = len(datas)
    b, errs, outs = eighth(jx, datas, 1 if ss == "grey" else 3)
    assert errs == [None] * n, errs
    for i, (got, w) in enumerate(zip(outs, want)):
        assert got.size == w.size and np.array_equal(got.reshape(w.shape), w), (shape_files(ss)[i][0], w.shape, int((got.reshape(w.shape) != w).sum()))
    assert all(b.jpeg_dc_only(i) for i in range(n))
    assert b.info_value("jpeg_pixel_images") == n and b.info_value("jpeg_dc_only_images") == n
    assert b.info_value("jpeg_pixel_launches") == 1
    assert b.info_value("hf_nonzeros") == 0
    sb = b.stage_bytes
    assert sb["hf"] == 0 and sb["idct"] == 0 and sb["filter"] == 0, sb
    nc = 1 if ss == "grey" else 3
    assert sb["out"] == sum(w.shape[0] * w.shape[1] * (4 * nc + nc) for w in want), sb      # 4 bytes per component read, one u8 per channel written
    old, errs0, outs0 = eighth(jx, datas, nc, dc_only=False)
    assert errs0 == [None] * n
    for i in range(n):
        assert np.array_equal(outs0[i], outs[i]), i
    assert old.info_value("jpeg_dc_only_images") == 0 and old.info_value("jpeg_pixel_launches") == 2
    assert old.info_value("hf_nonzeros") > 0 and old.stage_bytes["hf"] > 0 and old.stage_bytes["idct"] > 0
    pixels = sum(J.parse_jpeg(d).width * J.parse_jpeg(d).height for _, d in shape_files(ss))
    print(ss, "device bytes", b.device_bytes, "general path", old.device_bytes, "full-size pixels", pixels)
    assert old.device_bytes - b.device_bytes >= 24 * pixels                   # 12 B/px of coefficient planes and 12 B/px of pixel planes


@pytest.mark.gpu
def test_mixed_batch(jx):
    entries, want, eligible = [], [], 0
    for ss in (0, 1, "grey", 2):
        names = [n for n, _ in shape_files(ss)]
        for name in ("67x41", "300x280"):
            k = names.index(name)
            for s in (1, 2, 4, 8):
                w = wanted(ss, s)[k]
                entries.append((transcodes(ss)[k], s)); want.append(np.stack([w] * 3, -1) if w.ndim == 2 else w)
                eligible += s == 8 and ss != 2
    assert eligible == 6
    b, errs, outs = scaled_batch(jx, entries, 3)
    assert errs == [None] * len(entries), errs
    for i, (got, w) in enumerate(zip(outs, want)):
        assert got.shape == w.shape and np.array_equal(got, w), (i, entries[i][1], int((got != w).sum()))
    assert [b.jpeg_dc_only(i) for i in range(len(entries))] == [s == 8 and i // 8 != 3 for i, (_, s) in enumerate(entries)]
    assert b.info_value("jpeg_pixel_images") == len(entries) and b.info_value("jpeg_dc_only_images") == eligible
    assert b.info_value("hf_nonzeros") > 0
    # two kernels x (the group of scale 1, the group of the scaled entries) as before, and one launch for the DC-only group
    assert b.info_value("jpeg_pixel_launches") == 4 + 1
    old = jx.BatchDecoder()
    old.set_option("jpeg_dc_only", 0)
    for d, s in entries:
        old.add(d, num_channels=3, jpeg_scale=s)
    assert old.decode_jpeg_pixels() == [None] * len(entries)
    assert old.info_value("jpeg_pixel_launches") == 4 and old.info_value("jpeg_dc_only_images") == 0
    for i, w in enumerate(want):
        assert np.array_equal(old.output(i).reshape(w.shape), w), i


def dests(jx, items, dc_only):
    """test_jpeg_exact_pixels.decode_items with the option, and for items with resize_u8 (image_out_size has no such keyword: the size is the one without it)"""
    import torch
    b = jx.BatchDecoder(0)
    b.set_option("jpeg_dc_only", 1 if dc_only else 0)
    bufs = []
    for data, kw in items:
        size = jx.image_out_size(data, **{k: v for k, v in kw.items() if k not in ("filter", "mirror", "resize_u8")})[1]
        t = torch.full((size + EXTRA,), FILL, dtype=torch.uint8, device="cuda:0")
        i = b.add(data, device_ptr=t.data_ptr() + FRONT, **kw)
        assert b.out_size(i) == size
        bufs.append((t, size))
    errs = b.decode_jpeg_pixels()
    torch.cuda.synchronize()
    return b, errs, [(t.cpu().numpy(), n) for t, n in bufs]


@pytest.mark.gpu
def test_formats_layouts_and_resamples_follow(jx):
    jpegs = [make_jpeg(JC.photo(203, 139, seed=4), 0, 75), make_jpeg(JC.photo(101, 64, seed=3), 1, 80)]      # 26 x 18 and 13 x 8 at scale 8
    S.set_orientation(6)
    try:
        turned = [J.transcode(d) for d in jpegs]
    finally:
        S.set_orientation(1)
    LE, BE = jx.JXL_LITTLE_ENDIAN, jx.JXL_BIG_ENDIAN
    SC, BI = [2.0, 0.5, 4.0, 1.0], [-1.0, 0.25, -0.5, 0.0]
    items = []
    for jpeg, rot, crop in zip(jpegs, turned, ((3, 2, 20, 14), (2, 1, 10, 6))):
        data = J.transcode(jpeg)
        items += [(data, dict(dtype="uint8", num_channels=3, align=64, jpeg_scale=8)),
                  (data, dict(dtype="uint16", num_channels=4, endianness=BE, align=64, jpeg_scale=8)),
                  (data, dict(dtype="float16", num_channels=3, endianness=LE, planar=True, scale=SC, bias=BI, jpeg_scale=8)),
                  (data, dict(dtype="float32", num_channels=3, endianness=LE, resize=(48, 32), crop=crop, filter="bicubic", mirror=True, jpeg_scale=8)),
                  (data, dict(dtype="uint8", num_channels=3, resize=(16, 12), resize_u8=True, jpeg_scale=8)),
                  (rot, dict(dtype="uint8", num_channels=3, jpeg_scale=8))]
    new, errs, got = dests(jx, items, True)
    old, errs0, ref = dests(jx, items, False)
    assert errs == [None] * len(items) and errs0 == [None] * len(items), (errs, errs0)
    assert new.info_value("jpeg_dc_only_images") == len(items) and old.info_value("jpeg_dc_only_images") == 0
    assert new.info_value("hf_nonzeros") == 0 and old.info_value("hf_nonzeros") > 0
    assert new.info_value("resize_u8_images") == 2
    for n, ((g, size), (r, size0)) in enumerate(zip(got, ref)):
        assert size == size0 and np.array_equal(g, r), (n, items[n][1], int((g != r).sum()))
        assert (g[:FRONT] == FILL).all() and (g[FRONT + size:] == FILL).all() and (g[FRONT:FRONT + size] != FILL).any()
    # the plain u8 case against Pillow itself, and the turned one against its rotation
    for k, jpeg in enumerate(jpegs):
        w = pillow_scaled(jpeg, 8)
        g, size = got[6 * k]
        stride = -(-w.shape[1] * 3 // 64) * 64
        rows = np.stack([g[FRONT + y * stride:FRONT + y * stride + w.shape[1] * 3] for y in range(w.shape[0])])
        assert np.array_equal(rows.reshape(w.shape), w)
        g, size = got[6 * k + 5]
        assert np.array_equal(g[FRONT:FRONT + size].reshape(w.shape[1], w.shape[0], 3), np.rot90(w, -1))


@pytest.mark.gpu
def test_prefixes(jx):
    def one(data, nc, s=8):
        b = jx.BatchDecoder()
        b.add(data, num_channels=nc, jpeg_scale=s)
        assert b.decode_jpeg_pixels() == [None]
        assert b.info_value("jpeg_dc_only_images") == 1 and b.info_value("hf_nonzeros") == 0
        return b.output(0)

    def refused(data, nc, s=8):
        with pytest.raises(jx.DecodeError):
            b = jx.BatchDecoder()
            b.add(data, num_channels=nc, jpeg_scale=s)
            b.decode_jpeg_pixels()
        assert "truncated" in jx.last_error(), jx.last_error()

    for ss in DC_SAMPLINGS:
        nc = 1 if ss == "grey" else 3
        for name in BIG:
            data, bare, w = named(ss, name)
            for d in (data, bare):
                n = jx.lf_part_size(d)
                assert np.array_equal(one(d, nc).reshape(w.shape), w)
                assert np.array_equal(one(d[:n], nc).reshape(w.shape), w), (ss, name, n)
                assert n < len(d) // 2                                                       # the cut at 50 % lies behind the LF part
                assert np.array_equal(one(d[:len(d) // 2], nc).reshape(w.shape), w), (ss, name)
                refused(d[:n - 1], nc)
                refused(d[:n // 2], nc)
    d420 = named(2, "300x280")[0]
    refused(d420[:jx.lf_part_size(d420)], 3)                                                 # 4:2:0 needs AC terms: let in, not DC-only
    d444, _, w444 = named(0, "300x280")
    refused(d444[:jx.lf_part_size(d444)], 3, s=4)
    d422, _, w422 = named(1, "520x264")
    # through a pipeline, into pinned memory
    jobs = [d444[:jx.lf_part_size(d444)], d420[:jx.lf_part_size(d420)], d444[:jx.lf_part_size(d444) // 2], d422]
    sizes = [jx.image_out_size(d, "uint8", 3, jpeg_scale=8)[1] for d in (d444, d420, d444, d422)]
    bufs = [jx.PinnedBuffer(m) for m in sizes]
    p = small_pipeline(jx)
    try:
        st, _ = p.wait(p.submit(jobs, "uint8", 3, host_ptrs=[x.ptr for x in bufs], capacities=sizes, jpeg_pixels=True, jpeg_scale=8), check=False)
        assert st == [0, 1, 1, 0] and "truncated" in jx.last_error(), (st, jx.last_error())
        assert np.array_equal(np.array(bufs[0].array).reshape(w444.shape), w444) and np.array_equal(np.array(bufs[3].array).reshape(w422.shape), w422)
        assert p.info("jpeg_pixel_images") == 2 and p.info("jpeg_dc_only_images") == 2 and p.info("jpeg_pixel_launches") == 1 and p.info("hf_nonzeros") == 0
        # the 4:2:0 prefix alone in a job: nothing of it can be decoded
        st, _ = p.wait(p.submit(jobs[1:2], "uint8", 3, host_ptrs=[bufs[1].ptr], capacities=sizes[1:2], jpeg_pixels=True, jpeg_scale=8), check=False)
        assert st == [1] and "truncated" in jx.last_error(), (st, jx.last_error())
        # ... and the whole 4:2:0 file at scale 8 keeps the general path
        st, _ = p.wait(p.submit([d420], "uint8", 3, host_ptrs=[bufs[1].ptr], capacities=sizes[1:2], jpeg_pixels=True, jpeg_scale=8))
        w420 = named(2, "300x280")[2]
        assert st == [0] and np.array_equal(np.array(bufs[1].array).reshape(w420.shape), w420)
        assert p.info("jpeg_dc_only_images") == 0 and p.info("jpeg_pixel_launches") == 2 and p.info("hf_nonzeros") > 0
    finally:
        p.close()


@pytest.mark.gpu
def test_dc_only_jobs_in_the_rotation_of_coefficient_sets(jx):
    """test_jpeg_scaled_pixels.test_scaled_jobs_leave_clean_coefficient_sets with a DC-only job in the cycle: it takes nothing of its coefficient set and must still
    leave the set's events in order for the job that uses it next"""
    W2, H2 = 300, 280
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
        cycle = [(t444, pillow_scaled(q444, 8), True), (flat, ref_flat, False), (t420, pillow_scaled(q420, 8), True), (textured, ref_tex, False)]
        plan = [cycle[k % 4] for k in range(3 * sets + 3)]
        jobs = []
        for data, want, exact in plan:                                                      # no wait in between
            buf = jx.PinnedBuffer(want.size)
            kw = dict(jpeg_pixels=True, jpeg_scale=8) if exact else {}
            jobs.append((p.submit([data], "uint8", 3, host_ptrs=[buf.ptr], capacities=[want.size], **kw), buf, want, exact))
        for n, (t, buf, want, exact) in enumerate(jobs):
            st, _ = p.wait(t, check=False)
            assert st == [0], (n, jx.last_error())
            got = np.array(buf.array)
            assert np.array_equal(got, want.reshape(-1)), (n, "scale 8" if exact else "plain", int((got != want.reshape(-1)).sum()))
            if want is ref_flat:
                assert (got.reshape(H2, W2, 3) == px[0, 0]).all(), n
        assert p.info("private_plane_jobs") == 0                                            # every job ran on the shared sets
    finally:
        p.close()


@pytest.mark.gpu
def test_leaves_nothing_behind(jx):
    """test_jpeg_scaled_pixels.test_scaled_decode_leaves_clean_planes for ss = 0 at s = 8, on the DC-only path: one reused BatchDecoder"""
    files, _ = dense_and_twins(0)
    tf, tt, fresh, twin_px = twin_references(0)
    b = jx.BatchDecoder()

    def dc_decode():
        for d in tf:
            b.add(d, num_channels=3, jpeg_scale=8)
        assert b.decode_jpeg_pixels() == [None] * len(tf)
        assert b.info_value("jpeg_dc_only_images") == len(tf) and b.info_value("hf_nonzeros") == 0

    dc_decode()
    for i, d in enumerate(files):
        w = pillow_scaled(d, 8)
        w = restate_scaled(d, 8) if w is None else w
        assert np.array_equal(b.output(i).reshape(w.shape), w), i
    b.reset()
    for i, (got, w) in enumerate(zip(float_decode(b, tt), fresh)):                           # the float path of the flat twins over the same object
        assert np.array_equal(got, w), (i, int((got != w).sum()))
    b.reset()
    dc_decode()
    b.reset()
    for d in tt:
        b.add(d, num_channels=3)
    assert b.decode_jpeg_pixels() == [None] * len(tt)                                       # scale 1 of the twins
    for i, w in enumerate(twin_px):
        assert np.array_equal(b.output(i).reshape(w.shape), w), i
    assert b.info_value("jpeg_dc_only_images") == 0


@pytest.mark.gpu
def test_damaged_lf_parts(jx):
    """24 seeded bit flips and truncations inside the LF part of one 4:2:2 transcode, with the intact file in one batch: an error or an output of the right size"""
    data, bare, want = named(1, "300x280")
    off, n = payload_offset(data, bare), jx.lf_part_size(data)
    rng = np.random.default_rng(2468)
    keep, refused = [data], 0
    for k in range(24):
        if k % 4 == 3:
            bad = data[:int(rng.integers(off + 80, n))]                                     # a cut inside the LF part
        else:
            raw = bytearray(data)
            for pos in rng.integers(off + 80, n, 1 + k % 3):                                # behind the headers and the TOC, inside the LF part
                raw[pos] ^= 1 << int(rng.integers(0, 8))
            bad = bytes(raw)
        try:
            jx.BatchDecoder(-1).add(bad, num_channels=3, jpeg_scale=8)                      # (a stream the host parser refuses never enters a batch)
            keep.append(bad)
        except jx.DecodeError as e:
            assert str(e)
            refused += 1
            if k % 4 == 3:
                assert "truncated" in str(e)
    assert refused >= 6 and len(keep) > 1, (refused, len(keep))
    b, errs, outs = eighth(jx, keep, 3)
    assert errs[0] is None and np.array_equal(outs[0].reshape(want.shape), want)
    for i in range(1, len(keep)):
        assert errs[i] or b.output(i).size == want.size, i
    print("damaged LF parts: refused by the host", refused, "failed on the device", sum(1 for e in errs if e), "decoded", sum(1 for e in errs if e is None) - 1)
    assert b.info_value("jpeg_pixel_images") == sum(1 for e in errs if e is None)
    _, errs2, outs2 = eighth(jx, [data, named(0, "520x264")[0]], 3)                         # the decoder works afterwards
    assert errs2 == [None, None] and np.array_equal(outs2[0].reshape(want.shape), want)
    assert np.array_equal(outs2[1].reshape(named(0, "520x264")[2].shape), named(0, "520x264")[2])
