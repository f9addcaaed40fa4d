"""JPEG reconstruction as jobs of a pipeline (include/jxl_hip.h JxlHipPipelineSubmitJpegs / ...WaitJpegs / ...JpegStatus / ...CopyJpeg / ...ReleaseJpegs;
Pipeline.submit_jpegs / wait_jpegs; csrc/pipeline.cc), and the kernel behind them and behind BatchDecoder.reconstruct_jpegs(): csrc/jpeg_pixels.hip JpegGatherKernel,
which moves the quantised coefficients of a whole job from the HF stage's planes into the JPEG writer's arena in one launch and zeroes what it read.

The yardstick is the one of test_jpeg_batch.py, whose files, cases and helpers are imported, not copied: the file Pillow's libjpeg wrote, compared byte for byte — every
coefficient of every block decides bytes of the file.  A job is compared with the batch call over files AND error texts.

The zeroing is tested as in test_jpeg_pixel_jobs.py, by what the NEXT user of a coefficient set decodes: reconstruction, plain float and libjpeg-exact jobs alternate over
the pipeline's shared sets with no host wait in between; every plain result is the BatchDecoder's bit for bit and a flat picture — whose own stream carries no AC coefficient
at all — stays constant: a coefficient the gather left behind would show in it as texture."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_tools as J
import test_jpeg_batch as B
import test_jpeg_progressive as P
from conftest import ROOT, fixture_bytes
from test_jpeg_exact_pixels import float_decode, pillow, strip_boxes
from test_jpeg_pixel_jobs import H, W, clean_set_inputs, small_pipeline

SYMBOLS = ("JxlHipPipelineSubmitJpegs", "JxlHipPipelineWaitJpegs", "JxlHipPipelineJpegStatus", "JxlHipPipelineCopyJpeg", "JxlHipPipelineReleaseJpegs")
COUNTS = ("jpeg_device_images", "jpeg_host_images", "jpeg_device_progressive_images", "jpeg_gather_launches")


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


# ---- 1. CPU ------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_methods(jxh):
    L = jxh.libjxl()
    with open(os.path.join(ROOT, "include", "jxl_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name + "(" in header, name
    assert "#define JXL_HIP_JPEG_DEVICE_PROGRESSIVE 1u" in header and "#define JXL_HIP_JPEG_HOST_WRITER" in header
    assert (jxh.JXL_HIP_JPEG_DEVICE_PROGRESSIVE, jxh.JXL_HIP_JPEG_HOST_WRITER) == (1, 2)
    assert list(inspect.signature(jxh.Pipeline.submit_jpegs).parameters) == ["self", "datas", "progressive_on_device", "host_writer"]
    assert list(inspect.signature(jxh.Pipeline.wait_jpegs).parameters) == ["self", "ticket"]
    assert C.sizeof(jxh.JxlHipPipelineOptions) == 56                  # the two switches are flags of the submission, not options of the pipeline


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def sof_counts(files):
    sofs = [J.parse_jpeg(d).sof for d in files]
    assert all(s in (0xC0, 0xC1, 0xC2) for s in sofs), sofs
    return sum(1 for s in sofs if s != 0xC2), sum(1 for s in sofs if s == 0xC2)


def counts(p):
    return tuple(p.info(k) for k in COUNTS)


def collect(p, ticket, files, what):
    """wait_jpegs(ticket): every image has its file, and it is `files[i]` byte for byte"""
    got, errors, end_ms = p.wait_jpegs(ticket)
    assert errors == [None] * len(files), (what, errors)
    for i, (g, w) in enumerate(zip(got, files)):
        assert g == w, "%s: image %d differs" % (what, i)
    assert end_ms > 0
    return got


@pytest.mark.gpu
def test_every_real_file_as_jobs(jx):
    base = [JC.jpeg_bytes(c) for c in JC.CASES]
    grey = [JC.grey_jpeg_bytes(75, 52, 85), JC.grey_jpeg_bytes(41, 30, 70, optimize=True)]
    prog = [JC.jpeg_bytes(c) for c in JC.PROGRESSIVE]
    sample = fixture_bytes("sample.jpg")                               # the one real libjxl transcode: 4:4:4 with chroma from luma
    jobs = [base, prog + grey, base + prog + grey + [sample]]
    jxls = [[J.transcode(d) for d in base], [J.transcode(d) for d in prog + grey], [J.transcode(d) for d in base + prog + grey] + [fixture_bytes("sample_jpg.jxl")]]
    p = small_pipeline(jx)
    try:
        tickets = [p.submit_jpegs(x) for x in jxls]                    # none waited for before all are submitted
        for k, (t, files) in enumerate(zip(tickets, jobs)):
            collect(p, t, files, "job %d" % k)
            n_base, n_prog = sof_counts(files)
            assert counts(p) == (n_base, n_prog, 0, 1), (k, counts(p))
        files = jobs[2]
        collect(p, p.submit_jpegs(jxls[2], progressive_on_device=True), files, "progressive on the device")
        assert counts(p) == (len(files), 0, sof_counts(files)[1], 1)
        assert sof_counts(files)[1] >= len(JC.PROGRESSIVE)
    finally:
        p.close()


@pytest.mark.gpu
def test_shapes_as_jobs(jx):
    """The smallest inputs at which the gather can go wrong, as one baseline job and one progressive job.  The cases assert their own properties (test_jpeg_batch.SHAPES,
    test_jpeg_progressive.SHAPES): one block; 17 x 23 / 9 x 9 / odd MCU counts at 4:2:0 and 4:2:2 — component grids smaller than the frame's, chroma positions
    (sx << hs, sy << vs) —; 520 x 264 and 300 x 280: several 256 x 256 groups (g x 65536 + coef_off); quality 100: most AC dwords non-zero, every zeroing branch taken;
    quality 5: almost none."""
    baseline = [B.SHAPES[name](jx) for name in B.SHAPES]
    progressive = []
    for name in P.SHAPES:
        data, j = P.SHAPES[name]()
        assert j.sof == 0xC2
        progressive.append(data)
    # 4:4:4 over several 256 x 256 groups: more than one chroma-from-luma tile (a tile is 8 x 8 blocks) in both directions
    cfl = B.colour_jpeg(300, 280, 0, 90)
    j = J.parse_jpeg(cfl)
    assert [(c["h"], c["v"]) for c in j.components] == [(1, 1)] * 3 and j.width > 256 and j.height > 256
    baseline.append(cfl)
    p = small_pipeline(jx)
    try:
        tb = p.submit_jpegs([J.transcode(d) for d in baseline])
        tp = p.submit_jpegs([J.transcode(d) for d in progressive], progressive_on_device=True)
        collect(p, tb, baseline, "baseline shapes")
        assert counts(p) == (len(baseline), 0, 0, 1)
        collect(p, tp, progressive, "progressive shapes")
        assert counts(p) == (len(progressive), 0, len(progressive), 1)
    finally:
        p.close()


def batch_call(jx, jxls, progressive_on_device, host_writer):
    b = jx.BatchDecoder()
    if host_writer:
        b.set_option("jpeg_host_writer", 1)
    for d in jxls:
        b.add(d)
    b.reconstruct_jpegs(progressive_on_device=progressive_on_device)
    files, errors = [], []
    for i in range(len(jxls)):
        try:
            files.append(b.jpeg(i)); errors.append(None)
        except jx.DecodeError as e:
            files.append(None); errors.append(str(e))
    return b, files, errors


@pytest.mark.gpu
def test_job_equals_the_batch_call(jx):
    jpegs = [JC.grey_jpeg_bytes(90, 70, 85), B.colour_jpeg(130, 77, 0, 90), B.colour_jpeg(101, 64, 1, 80), B.colour_jpeg(203, 139, 2, 75),
             P.prog_colour(67, 41, 2, 95), P.prog_colour(120, 90, 0, 85), P.save_jpeg(JC.photo(75, 52, seed=3)[:, :, 0], quality=80)]
    assert sof_counts(jpegs) == (4, 3)
    jxls = [J.transcode(d) for d in jpegs] + [fixture_bytes("sample.jxl")]              # ... and one image that fails alone, with the batch call's text
    p = small_pipeline(jx)
    try:
        for prog, host in ((False, False), (True, False), (False, True)):
            b, files, errors = batch_call(jx, jxls, prog, host)
            assert files[:len(jpegs)] == jpegs and errors[-1].startswith("JPEG reconstruction: ")
            got, errs, _ = p.wait_jpegs(p.submit_jpegs(jxls, progressive_on_device=prog, host_writer=host))
            assert got == files and errs == errors, (prog, host, errs, errors)
            assert counts(p)[:3] == tuple(b.info_value(k) for k in COUNTS[:3]), (prog, host)
            assert counts(p)[3] == b.info_value("jpeg_gather_launches") == 1
            if host:
                assert p.info("jpeg_device_images") == 0 and p.info("jpeg_host_images") == len(jpegs)
    finally:
        p.close()


# ---- the zeroing -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_coefficient_sets_stay_clean(jx):
    q444, q420, flat, textured = clean_set_inputs()                                       # (asserts > 50 % non-zero AC in every component of the 4:4:4 file)
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
        R444, R420 = ("files", t444, q444), ("files", t420, q420)
        FLAT, TEX, X420 = ("plain", flat, ref_flat), ("plain", textured, ref_tex), ("exact", t420, pillow(q420))
        # job n meets set n % 3: with the damaged job at 0 every set sees reconstruction -> plain, and set 0 reconstruction -> exact
        cycle = [R444, FLAT, R420, TEX, R444, X420, R420, TEX]
        plan = [("files", bad, None)] + [cycle[k % 8] for k in range(3 * sets + 3)]
        size = W * H * 3
        jobs = []
        for kind, data, want in plan:                                                       # no wait in between
            if kind == "files":
                jobs.append((p.submit_jpegs([data]), None, want, kind))
            else:
                buf = jx.PinnedBuffer(size)
                jobs.append((p.submit([data], "uint8", 3, host_ptrs=[buf.ptr], capacities=[size], jpeg_pixels=kind == "exact"), buf, want, kind))
        for n, (t, buf, want, kind) in enumerate(jobs):
            if kind == "files":
                files, errors, _ = p.wait_jpegs(t)
                if want is None:
                    assert (files[0] is None) != (errors[0] is None)                        # the damaged job: a file or a reason
                    continue
                assert errors == [None] and files[0] == want, (n, errors)
                continue
            st, _ = p.wait(t, check=False)
            assert st == [0], (n, jx.last_error())
            got = np.array(buf.array)
            assert np.array_equal(got, want.reshape(-1)), (n, kind, int((got != want.reshape(-1)).sum()))
            if want is ref_flat:
                assert (got.reshape(H, W, 3) == px[0, 0]).all(), n
        assert p.info("private_plane_jobs") == 0                                            # every job ran on the shared sets
    finally:
        p.close()


# ---- failures ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_failures_stay_with_their_image(jx):
    good = B.colour_jpeg(100, 60, 2, 80, restart_marker_blocks=3)
    good_prog = P.prog_colour(90, 70, 2, 85)
    jxl = J.transcode(good)
    no_jbrd, cs = strip_boxes(jxl)
    jbrd = J.build_jbrd(J.parse_jpeg(good))
    assert jxl == J.container(jbrd, cs)
    rng = np.random.default_rng(11)
    mutated = []
    for k in range(5):                                                                      # the mutations of test_jpeg_batch.py
        bad = bytearray(cs)
        for pos in rng.integers(len(cs) * 6 // 10, len(cs), 1 + k % 3):                      # the AC sections fill the back of the codestream
            bad[pos] ^= 1 << int(rng.integers(0, 8))
        mutated.append(J.container(jbrd, bytes(bad)))
    mutated.append(J.container(jbrd, cs[:-40]))
    ineligible = [fixture_bytes("sample.jxl"), no_jbrd, J.container(jbrd[:len(jbrd) // 2], cs)]
    datas = [jxl, J.transcode(good_prog)] + ineligible + mutated
    _, _, batch_errors = batch_call(jx, [jxl] + ineligible, False, False)
    p = small_pipeline(jx)
    try:
        files, errors, _ = p.wait_jpegs(p.submit_jpegs(datas))
        assert files[0] == good and files[1] == good_prog and errors[:2] == [None, None]      # whatever the others do
        for k in range(3):
            assert files[2 + k] is None and errors[2 + k] == batch_errors[1 + k], (k, errors[2 + k], batch_errors[1 + k])
        assert "no jbrd box" in errors[2] and "no jbrd box" in errors[3] and "jbrd" in errors[4]
        from PIL import Image
        import io
        for k in range(5, len(datas)):
            if files[k] is None:
                assert errors[k]
                continue
            assert errors[k] is None
            Image.open(io.BytesIO(files[k])).load()                                         # a file Pillow opens
        collect(p, p.submit_jpegs([jxl, jxl]), [good, good], "a clean job afterwards")
        # a job in which no image can be reconstructed fails as a whole, with a message, and leaves the pipeline usable
        files, errors, _ = p.wait_jpegs(p.submit_jpegs([fixture_bytes("sample.jxl")]))
        assert files == [None] and errors[0] and "JPEG reconstruction" in errors[0]
        # unknown flag bits refuse the submission
        assert jx.libjxl().JxlHipPipelineSubmitJpegs(p._h, (C.c_char_p * 1)(jxl), (C.c_size_t * 1)(len(jxl)), 1, 4) == -1 and "unknown flag bits" in jx.last_error()
        collect(p, p.submit_jpegs([jxl]), [good], "after the refusals")
    finally:
        p.close()


# ---- collection --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_collection(jx):
    L = jx.libjxl()
    files = [B.colour_jpeg(67, 45, 2, 85), B.colour_jpeg(64, 48, 0, 80, restart_marker_blocks=2), JC.grey_jpeg_bytes(41, 30, 70)]
    jxls = [J.transcode(d) for d in files]
    p = jx.Pipeline(0, jobs_in_flight=1, lf_streams=1, hf_streams=1, prepare_threads=1, parse_threads=2)
    try:
        # out of order
        ta, tb, tc = p.submit_jpegs(jxls[:2]), p.submit_jpegs(jxls[2:]), p.submit_jpegs(jxls)
        collect(p, tc, files, "third first")
        collect(p, ta, files[:2], "first second")
        collect(p, tb, files[2:], "second last")
        # JxlHipPipelineWait on a reconstruction ticket: the statuses, and the files are gone
        t = p.submit_jpegs(jxls)
        st, _ = p.wait(t)
        assert st == [0, 0, 0]
        assert L.JxlHipPipelineJpegStatus(p._h, t, 0) == jx.JXL_DEC_ERROR and "unknown ticket" in jx.last_error()
        # JxlHipPipelineWaitJpegs on a plain ticket is refused, and the ticket stays waitable
        size = jx.image_out_size(jxls[0], "uint8", 3)[1]
        buf = jx.PinnedBuffer(size)
        t = p.submit([jxls[0]], "uint8", 3, host_ptrs=[buf.ptr], capacities=[size])
        st, sizes = (C.c_int * 1)(), (C.c_size_t * 1)()
        assert L.JxlHipPipelineWaitJpegs(p._h, t, st, sizes, 1, None) == jx.JXL_DEC_ERROR and "not a reconstruction job" in jx.last_error()
        assert p.wait(t)[0] == [0]
        # the C calls one by one: sizes, a capacity one byte short, the right one, release
        t = p.submit_jpegs(jxls)
        n = len(jxls)
        st, sizes, end = (C.c_int * n)(), (C.c_size_t * n)(), C.c_float()
        assert L.JxlHipPipelineWaitJpegs(p._h, t, st, sizes, n, C.byref(end)) == jx.JXL_DEC_SUCCESS
        assert list(st) == [0] * n and list(sizes) == [len(d) for d in files]
        for i, want in enumerate(files):
            assert L.JxlHipPipelineJpegStatus(p._h, t, i) == jx.JXL_DEC_SUCCESS
            out = np.full(len(want) + 8, 0xA5, np.uint8)
            assert L.JxlHipPipelineCopyJpeg(p._h, t, i, out.ctypes.data, len(want) - 1) == jx.JXL_DEC_ERROR and "smaller" in jx.last_error()
            assert (out == 0xA5).all()
            assert L.JxlHipPipelineCopyJpeg(p._h, t, i, out.ctypes.data, len(want)) == jx.JXL_DEC_SUCCESS
            assert out[:len(want)].tobytes() == want and (out[len(want):] == 0xA5).all()
        assert L.JxlHipPipelineJpegStatus(p._h, t, n) == jx.JXL_DEC_ERROR and "no such image" in jx.last_error()
        L.JxlHipPipelineReleaseJpegs(p._h, t)
        assert L.JxlHipPipelineJpegStatus(p._h, t, 0) == jx.JXL_DEC_ERROR and "unknown ticket" in jx.last_error()
        assert L.JxlHipPipelineWaitJpegs(p._h, t, st, sizes, n, None) == jx.JXL_DEC_ERROR and "unknown ticket" in jx.last_error()
        p._keep.pop(t, None)
        # more jobs than slots, nobody waiting until the end: the prepare thread's harvest gives the same bytes
        slots = p.info("slots")
        tickets = [p.submit_jpegs(jxls if k % 2 else jxls[::-1]) for k in range(2 * slots + 1)]
        for k, t in enumerate(tickets):
            collect(p, t, files if k % 2 else files[::-1], "job %d of %d" % (k, len(tickets)))
    finally:
        p.close()
