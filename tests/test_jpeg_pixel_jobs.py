"""libjpeg-exact pixels of JPEG transcodes as jobs of a pipeline (include/jxl_hip.h JxlHipPipelineSubmitJpegPixels; Pipeline.submit(jpeg_pixels=True); csrc/pipeline.cc), and
the kernel behind them and behind BatchDecoder.decode_jpeg_pixels(): csrc/jpeg_pixels.hip JpegIdctPlanesKernel, the integer IDCT that reads the HF stage's coefficient planes
in place and zeroes what it read.

The yardstick is the one of test_jpeg_exact_pixels.py, whose files, cases and helpers are imported, not copied: Pillow's libjpeg-turbo, np.array_equal on u8.  A job is
compared with the batch call byte for byte over the whole destination; the resized f32 output with the filter restated over restate() / 255 under the derived bound of
test_resample_jobs.py, (taps_x + taps_y + 8) x 2^-24 x L_x x L_y x max|v|.

The zeroing is tested by what the NEXT user of a coefficient set decodes: exact and plain float jobs alternate over the pipeline's shared sets with no host wait in between;
every plain result is the BatchDecoder's bit for bit, and a flat picture — whose own stream carries no AC coefficient at all — stays constant: a coefficient the integer IDCT
left behind would show in it as texture.  (With the kernel's two zeroing stores removed, test_coefficient_sets_stay_clean fails at the first plain job behind an exact one;
test_batch_call_leaves_clean_planes alone could not tell: an HF stage that writes the same stream over its own left-overs writes the same values.)"""
import inspect
import os

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_tools as J
import synth_lib as S
from conftest import FIXTURES, ROOT, fixture_bytes
from test_jpeg_exact_pixels import (EXTRA, FILL, FRONT, REFUSAL, SAMPLINGS, check_shape_properties, decode_items, float_decode, make_jpeg, pillow, resample, restate, shape_files,
                                    strip_boxes, transcode_440)


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


def small_pipeline(jx, **kw):
    opts = dict(jobs_in_flight=3, lf_streams=2, hf_streams=1, prepare_threads=1, parse_threads=2)
    opts.update(kw)
    return jx.Pipeline(0, **opts)


def xyb_stream(w=40, h=24, seed=3):
    return S.encode_vardct(S.synthetic_image(seed, w, h), seed=2, strategy_mix=0, epf_iters=0, gab=0)


# ---- 1. CPU ------------------------------------------------------------------------------------------------------------------------------------
def test_symbol_and_refusals(jxh):
    L = jxh.libjxl()
    with open(os.path.join(ROOT, "include", "jxl_hip.h")) as f:
        header = f.read()
    assert hasattr(L, "JxlHipPipelineSubmitJpegPixels") and "JxlHipPipelineSubmitJpegPixels(" in header
    assert "jpeg_pixels" in inspect.signature(jxh.Pipeline.submit).parameters
    try:
        p = jxh.Pipeline(0, jobs_in_flight=1, lf_streams=1, hf_streams=1, prepare_threads=1, parse_threads=1)
    except jxh.CannotCreateDecoder:
        return                                                    # (no device here: the symbol check stands alone)
    try:
        data = J.transcode(make_jpeg(JC.photo(16, 16, seed=2), 2, 85))
        out = jxh.PinnedBuffer(16 * 16 * 3)
        with pytest.raises(jxh.DecodeError, match="downscale 8"):
            p.submit([data], "uint8", 3, host_ptrs=[out.ptr], downscale=8, jpeg_pixels=True)
    finally:
        p.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def run_job(jx, p, datas, want, channels, host=False, check=True):
    """One exact u8 job of `datas` (want[i]: Pillow's picture, or None for an image expected to fail) -> per-image status.  Device destinations sit FRONT bytes into a
    buffer filled with FILL whose other bytes must come back untouched; host destinations are pinned buffers."""
    import torch
    sizes = [jx.image_out_size(d, "uint8", channels)[1] for d in datas]
    if host:
        bufs = [jx.PinnedBuffer(s) for s in sizes]
        t = p.submit(datas, "uint8", channels, host_ptrs=[b.ptr for b in bufs], capacities=sizes, jpeg_pixels=True)
    else:
        bufs = [torch.full((s + EXTRA,), FILL, dtype=torch.uint8, device="cuda:0") for s in sizes]
        t = p.submit(datas, "uint8", channels, device_ptrs=[b.data_ptr() + FRONT for b in bufs], capacities=sizes, jpeg_pixels=True)
    status, _ = p.wait(t, check=check)
    torch.cuda.synchronize()
    for i, (b, s, w) in enumerate(zip(bufs, sizes, want)):
        whole = np.array(b.array) if host else b.cpu().numpy()
        if not host:
            assert (whole[:FRONT] == FILL).all() and (whole[FRONT + s:] == FILL).all(), ("guard bytes", i)
        if w is None or status[i] != 0:
            continue
        got = whole[:s] if host else whole[FRONT:FRONT + s]
        exp = w if channels == 1 or w.ndim == 3 else np.stack([w] * 3, -1)           # (a grey image in a 3-channel job: L in all three)
        assert got.size == exp.size and np.array_equal(got.reshape(exp.shape), exp), (i, exp.shape, int((got.reshape(exp.shape) != exp).sum()))
    return status


@pytest.mark.gpu
def test_every_real_file_as_jobs(jx):
    colour = [JC.jpeg_bytes(c) for c in JC.CASES + JC.PROGRESSIVE]
    grey = [JC.grey_jpeg_bytes(75, 52, 85), JC.grey_jpeg_bytes(41, 30, 70, optimize=True)]
    with open(os.path.join(FIXTURES, "sample.jpg"), "rb") as f:
        sample = f.read()
    p = small_pipeline(jx)
    try:
        jobs = [([J.transcode(d) for d in colour] + [fixture_bytes("sample_jpg.jxl")], [pillow(d) for d in colour + [sample]], 3, False),
                ([J.transcode(d) for d in grey], [pillow(d) for d in grey], 1, True),
                ([J.transcode(d) for d in colour + grey] + [fixture_bytes("sample_jpg.jxl")], [pillow(d) for d in colour + grey + [sample]], 3, False)]
        for datas, want, nc, host in jobs:
            assert run_job(jx, p, datas, want, nc, host=host) == [0] * len(datas)
            assert p.info("jpeg_pixel_images") == len(datas)
            assert p.info("jpeg_pixel_launches") == 2 * -(-len(datas) // 32768) == 2
    finally:
        p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ss", SAMPLINGS)
def test_shapes_as_jobs(jx, ss):
    check_shape_properties(ss)
    files = [d for _, d in shape_files(ss)]
    p = small_pipeline(jx)
    try:
        assert run_job(jx, p, [J.transcode(d) for d in files], [pillow(d) for d in files], 1 if ss == "grey" else 3) == [0] * len(files)
    finally:
        p.close()


@pytest.mark.gpu
def test_job_equals_the_batch_call(jx):
    import torch
    jpegs = [make_jpeg(JC.photo(90, 70, seed=1), "grey", 85), make_jpeg(JC.photo(130, 77, seed=2), 0, 90), make_jpeg(JC.photo(101, 64, seed=3), 1, 80),
             make_jpeg(JC.photo(203, 139, seed=4), 2, 75), make_jpeg(JC.photo(67, 41, seed=5), 2, 95)]
    datas = [J.transcode(d) for d in jpegs]
    n = len(datas)
    crops = [(10, 6, 60, 50), None, (1, 2, 99, 60), (100, 30, 100, 100), (0, 0, 64, 40)]
    filters = ["bicubic", "bilinear", "bicubic", "bilinear", "bicubic"]
    mirrors = [True, False, True, True, False]
    SC, BI = [2.0, 0.5, 4.0], [-1.0, 0.25, -0.5]
    LE, BE = jx.JXL_LITTLE_ENDIAN, jx.JXL_BIG_ENDIAN
    lay = dict(planar=True, scale=SC, bias=BI, resize=(48, 32))

    def own(k):
        return dict({} if crops[k] is None else dict(crop=crops[k]), filter=filters[k], mirror=mirrors[k])
    b, errs, dests = decode_items(jx, [(datas[k], dict(dtype="float16", num_channels=3, endianness=LE, **own(k), **lay)) for k in range(n)])
    assert errs == [None] * n, errs
    one = 3 * 32 * 48 * 2
    refs = [d[FRONT:FRONT + m].copy() for d, m in dests]
    assert [r.size for r in refs] == [one] * n
    p = small_pipeline(jx)
    try:
        out = torch.full((n, 3, 32, 48), 7.0, dtype=torch.float16, device="cuda:0")
        st, _ = p.wait(p.submit(datas, "float16", 3, device_ptrs=[out[k].data_ptr() for k in range(n)], capacities=[one] * n, endianness=LE, crop=crops, filter=filters,
                                mirror=mirrors, jpeg_pixels=True, **lay))
        torch.cuda.synchronize()
        assert st == [0] * n
        assert np.array_equal(out.cpu().numpy().view(np.uint8).reshape(-1), np.concatenate(refs))
        pinned = jx.PinnedBuffer(n * one)
        st, _ = p.wait(p.submit(datas, "float16", 3, host_ptrs=[pinned.ptr + k * one for k in range(n)], capacities=[one] * n, endianness=LE, crop=crops, filter=filters,
                                mirror=mirrors, jpeg_pixels=True, **lay))
        assert st == [0] * n and np.array_equal(pinned.array, np.concatenate(refs))
        # a plain interleaved job: u16 big endian, rows padded to 32 bytes
        u16 = dict(dtype="uint16", num_channels=3, endianness=BE, align=32)
        _, errs, dests = decode_items(jx, [(d, u16) for d in datas])
        assert errs == [None] * n, errs
        sizes = [m for _, m in dests]
        bufs = [torch.full((m + EXTRA,), FILL, dtype=torch.uint8, device="cuda:0") for m in sizes]
        st, _ = p.wait(p.submit(datas, "uint16", 3, device_ptrs=[t.data_ptr() + FRONT for t in bufs], capacities=sizes, endianness=BE, align=32, jpeg_pixels=True))
        torch.cuda.synchronize()
        assert st == [0] * n
        for k in range(n):
            assert np.array_equal(bufs[k].cpu().numpy(), dests[k][0]), k             # (the whole destination: guard bytes and row padding included)
        # one image, f32, against the restated filter over the integer picture
        k = 3
        x0, y0, cw, ch = crops[k]
        src = (restate(jpegs[k]).astype(np.float32) * np.float32(1.0 / 255))[y0:y0 + ch, x0:x0 + cw]
        f32 = torch.full((32, 48, 3), 9.0, dtype=torch.float32, device="cuda:0")
        st, _ = p.wait(p.submit([datas[k]], "float32", 3, device_ptrs=[f32.data_ptr()], capacities=[48 * 32 * 3 * 4], endianness=LE, resize=(48, 32), crop=crops[k], filter=filters[k],
                                mirror=mirrors[k], jpeg_pixels=True))
        torch.cuda.synchronize()
        assert st == [0]
        want, (tx, ty), (lx, ly) = resample(src, (48, 32), filters[k])
        want = want[:, ::-1] if mirrors[k] else want
        got = f32.cpu().numpy()
        bound = (tx + ty + 8) * 2.0 ** -24 * lx * ly * float(np.abs(src).max())
        err = float(np.abs(got.astype(np.float64) - want).max())
        print("taps", (tx, ty), "sum |w|", (lx, ly), "max error", err, "bound", bound)
        assert np.isfinite(got).all() and err <= bound, (err, bound)
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
    want = pillow(good)
    datas = [jxl, fixture_bytes("sample.jxl"), xyb_stream(), transcode_440()] + mutated
    p = small_pipeline(jx)
    try:
        status = run_job(jx, p, datas, [want, None, None, None] + [None] * len(mutated), 3, check=False)       # (run_job compares image 0 and checks every guard byte)
        assert status[:4] == [0, 1, 1, 1], status
        assert jx.last_error().startswith("image 1: " + REFUSAL), jx.last_error()
        assert all(s in (0, 1) for s in status[4:])                                         # an error, or an output of the right size (the guard bytes around it are intact)
        assert p.info("jpeg_pixel_images") == sum(1 for s in status if s == 0)
        assert run_job(jx, p, [jxl, jxl], [want, want], 3) == [0, 0]                          # a clean job afterwards
        # a capacity one byte short fails that image alone
        size = want.size
        bufs = [jx.PinnedBuffer(size) for _ in range(2)]
        st, _ = p.wait(p.submit([jxl, jxl], "uint8", 3, host_ptrs=[b.ptr for b in bufs], capacities=[size, size - 1], jpeg_pixels=True), check=False)
        assert st == [0, 1] and "too small" in jx.last_error()
        assert np.array_equal(np.array(bufs[0].array).reshape(want.shape), want)
        with pytest.raises(jx.DecodeError, match="downscale 8"):
            p.submit([jxl], "uint8", 3, host_ptrs=[bufs[0].ptr], downscale=8, jpeg_pixels=True)
        assert run_job(jx, p, [jxl], [want], 3, host=True) == [0]
    finally:
        p.close()


# ---- the zeroing -------------------------------------------------------------------------------------------------------------------------------
W, H = 300, 280


def clean_set_inputs():
    img = JC.photo(W, H, seed=77)
    q444, q420 = make_jpeg(img, 0, 100), make_jpeg(img, 2, 100)
    j = J.parse_jpeg(q444)
    for c in range(3):
        ac = np.asarray(j.coef[c]).reshape(-1, 64)[:, 1:]
        assert (ac != 0).mean() > 0.5, (c, float((ac != 0).mean()))                         # dense coefficient planes: most dwords of the set are written
    flat = S.encode_vardct(np.full((H, W, 3), 120, np.uint8), seed=2, strategy_mix=0, epf_iters=0, gab=0)
    textured = S.encode_vardct(S.synthetic_image(8, W, H), seed=2, strategy_mix=0, epf_iters=0, gab=0)
    return q444, q420, flat, textured


@pytest.mark.gpu
def test_coefficient_sets_stay_clean(jx):
    q444, q420, flat, textured = clean_set_inputs()
    t444, t420 = J.transcode(q444), J.transcode(q420)
    ref_flat, ref_tex = float_decode(jx.BatchDecoder(), [flat])[0], float_decode(jx.BatchDecoder(), [textured])[0]
    px = ref_flat.reshape(H, W, 3)
    assert (px == px[0, 0]).all()                                                           # the flat stream decodes to one colour
    assert not (ref_tex.reshape(H, W, 3) == ref_tex.reshape(H, W, 3)[0, 0]).all()
    _, cs = strip_boxes(t444)
    bad = bytearray(cs)
    bad[len(cs) * 3 // 4] ^= 0x5A; bad[len(cs) * 3 // 4 + 7] ^= 0xFF                          # (the AC sections fill the back of the codestream)
    bad = J.container(J.build_jbrd(J.parse_jpeg(q444)), bytes(bad))
    p = jx.Pipeline(0, jobs_in_flight=4, lf_streams=2, hf_streams=2, prepare_threads=2, parse_threads=2, reserve_frames=2, reserve_width=512, reserve_height=512)
    try:
        sets = p.info("coefficient_sets")
        assert sets == 3
        cycle = [(t444, pillow(q444), True), (flat, ref_flat, False), (t420, pillow(q420), True), (textured, ref_tex, False)]
        plan = [(bad, None, True)] + [cycle[k % 4] for k in range(3 * sets + 1 + 2)]        # (3 sets + 1 and two more: every set sees exact -> plain and plain -> exact)
        size = W * H * 3
        jobs = []
        for data, want, exact in plan:                                                      # no wait in between
            buf = jx.PinnedBuffer(size)
            jobs.append((p.submit([data], "uint8", 3, host_ptrs=[buf.ptr], capacities=[size], jpeg_pixels=exact), buf, want, exact))
        for n, (t, buf, want, exact) in enumerate(jobs):
            st, _ = p.wait(t, check=False)
            if want is None:
                assert st[0] in (0, 1)
                continue
            assert st == [0], (n, jx.last_error())
            got = np.array(buf.array)
            assert np.array_equal(got, want.reshape(-1)), (n, "exact" if exact else "plain", int((got != want.reshape(-1)).sum()))
            if want is ref_flat:
                assert (got.reshape(H, W, 3) == px[0, 0]).all(), n
        assert p.info("private_plane_jobs") == 0                                            # every job ran on the shared sets
    finally:
        p.close()


@pytest.mark.gpu
def test_batch_call_leaves_clean_planes(jx):
    q444, _, flat, _ = clean_set_inputs()
    t444 = J.transcode(q444)
    fresh = float_decode(jx.BatchDecoder(), [t444, flat])
    b = jx.BatchDecoder()
    b.add(t444, num_channels=3)
    b.add(flat, num_channels=3)
    errs = b.decode_jpeg_pixels()
    assert errs[0] is None and errs[1].startswith(REFUSAL), errs
    want = pillow(q444)
    assert np.array_equal(b.output(0).reshape(want.shape), want)
    b.decode(); b.finish()                                                                  # no reset in between
    for i in range(2):
        assert np.array_equal(b.output(i), fresh[i]), i
    b.reconstruct_jpegs()
    assert b.jpeg(0) == q444
    # ... and with nothing but eligible images, where the call itself says that the planes are clean
    c = jx.BatchDecoder()
    c.add(t444, num_channels=3)
    assert c.decode_jpeg_pixels() == [None] and c.decode_jpeg_pixels() == [None]
    assert np.array_equal(c.output(0).reshape(want.shape), want)
    c.decode(); c.finish()
    assert np.array_equal(c.output(0), fresh[0])
    c.reconstruct_jpegs()
    assert c.jpeg(0) == q444
