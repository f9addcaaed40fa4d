"""Batch JPEG reconstruction (include/jxl_hip.h JxlHipBatchReconstructJpegs; BatchDecoder.reconstruct_jpegs): one entropy run for all images, the
entropy-coded segments of sequential Huffman scans written by the device (csrc/jpeg_write.hip), markers and splicing on the host (csrc/jpeg_recon.cc
WriteJpegMarkers / SpliceJpegScan), progressive files through the host writer.  The yardstick is exact everywhere: the bytes of the JPEG file that Pillow's
libjpeg wrote and tests/jpeg_tools.py transcoded.  The last test needs no GPU: the marker / splice half under ASan + UBSan in a stand-alone program."""
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_tools as J
from conftest import FIXTURES, ROOT, fixture_bytes

STUFF_CHUNK = 1024      # bytes of the unstuffed segment buffer per workgroup of the stuffing kernels (jpeg_write.hip kStuffChunk)
BLOCKS_PER_WORKGROUP = 4


@pytest.fixture(scope="module")
def jx(built):
    import jpegxl_rs_amd as jx
    return jx


def colour_jpeg(w, h, ss, q, seed=None, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(JC.photo(w, h, seed=w + h if seed is None else seed)).save(buf, "JPEG", quality=q, subsampling=ss, **kw)
    return buf.getvalue()


def reconstruct_batch(jx, jxls, host_writer=False):
    b = jx.BatchDecoder()
    if host_writer:
        b.set_option("jpeg_host_writer", 1)
    for d in jxls:
        b.add(d)
    b.reconstruct_jpegs()
    return b, [b.jpeg(i) for i in range(len(jxls))]


def entropy_segments(data):
    """(first byte, last byte + 1) of every entropy-coded segment of a JPEG file, restart segments separately."""
    out, pos = [], 2
    while data[pos + 1] != 0xD9:
        m, ln = data[pos + 1], struct.unpack(">H", data[pos + 2:pos + 4])[0]
        pos += 2 + ln
        if m != 0xDA:
            continue
        start = pos
        while True:
            if data[pos] == 0xFF and data[pos + 1] != 0:
                out.append((start, pos))
                if 0xD0 <= data[pos + 1] <= 0xD7:
                    pos += 2
                    start = pos
                    continue
                break
            pos += 1
    return out


def code_stats(j):
    """Over the blocks of a parsed baseline file: the longest zero run in front of a coefficient, the longest Huffman code + magnitude bits of one coefficient,
    the shortest block in bits."""
    depth = {}
    for h in j.huff:
        d, k = {}, 0
        for ln in range(1, 17):
            for _ in range(h["counts"][ln - 1]):
                d[h["values"][k]] = ln
                k += 1
        depth[(h["is_ac"], h["id"])] = d
    max_run, max_piece, min_block = 0, 0, 1 << 30
    for ci, dct, act in j.scans[0]["comps"]:
        zz = j.coef[ci].reshape(-1, 64)[:, J.ZIGZAG].astype(int)
        for blk in zz:
            bits, run = 2, 0
            for k in range(1, 64):
                if blk[k] == 0:
                    run += 1
                    continue
                nb = int(abs(blk[k])).bit_length()
                piece = depth[(1, act)][((run & 15) << 4) | nb] + nb
                max_run, max_piece = max(max_run, run), max(max_piece, piece)
                bits += piece + (run >> 4) * depth[(1, act)][0xF0]
                run = 0
            if run:
                bits += depth[(1, act)][0]
            min_block = min(min_block, bits)
    return max_run, max_piece, min_block


# ---- 1, 2: every real file in one batch, device writer == host writer ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_files():
    base = [JC.jpeg_bytes(c) for c in JC.CASES] + [JC.grey_jpeg_bytes(75, 52, 85), JC.grey_jpeg_bytes(41, 30, 70, optimize=True)]
    prog = [JC.jpeg_bytes(c) for c in JC.PROGRESSIVE]
    with open(os.path.join(FIXTURES, "sample.jpg"), "rb") as f:
        sample = f.read()
    files = base + prog + [sample]
    jxls = [J.transcode(d) for d in base + prog] + [fixture_bytes("sample_jpg.jxl")]
    sample_baseline = J.parse_jpeg(sample).sof != 0xC2
    return files, jxls, len(base) + (1 if sample_baseline else 0), len(prog) + (0 if sample_baseline else 1)


@pytest.mark.gpu
def test_every_real_file_in_one_batch(jx, real_files):
    files, jxls, n_base, n_prog = real_files
    b, out = reconstruct_batch(jx, jxls)
    for i, (got, want) in enumerate(zip(out, files)):
        assert b.can_reconstruct_jpeg(i)
        assert got == want, "image %d differs" % i
    assert b.info_value("jpeg_device_images") == n_base
    assert b.info_value("jpeg_host_images") == n_prog


@pytest.mark.gpu
def test_device_writer_equals_host_writer(jx, real_files):
    files, jxls, _, _ = real_files
    b, out = reconstruct_batch(jx, jxls, host_writer=True)
    assert out == files
    assert b.info_value("jpeg_device_images") == 0 and b.info_value("jpeg_host_images") == len(files)


# ---- 3: the smallest shapes at which the device writer can go wrong ---------------------------------------------------------------------------
def _mcus(j):
    mh, mv = max(c["h"] for c in j.components), max(c["v"] for c in j.components)
    return -(-j.width // (8 * mh)), -(-j.height // (8 * mv))


def case_grey_one_block():
    d = JC.grey_jpeg_bytes(8, 8, 85)
    j = J.parse_jpeg(d)
    assert len(j.components) == 1 and j.coef[0].shape[:2] == (1, 1) and len(entropy_segments(d)) == 1
    return d


def case_420(w, h, odd):
    d = colour_jpeg(w, h, 2, 85)
    j = J.parse_jpeg(d)
    assert [(c["h"], c["v"]) for c in j.components] == [(2, 2), (1, 1), (1, 1)] and w % 16 and h % 16      # MCU padding in both directions
    mx, my = _mcus(j)
    assert (mx * my) % 2 == (1 if odd else 0) and (odd or (mx > 1 and my > 1))
    return d


def case_422():
    d = colour_jpeg(50, 37, 1, 80)
    j = J.parse_jpeg(d)
    assert [(c["h"], c["v"]) for c in j.components] == [(2, 1), (1, 1), (1, 1)] and 50 % 16 and 37 % 8
    return d


def case_restart_every_mcu():
    d = colour_jpeg(64, 48, 2, 80, restart_marker_blocks=1)
    j = J.parse_jpeg(d)
    mx, my = _mcus(j)
    assert j.restart_interval == 1 and len(entropy_segments(d)) == mx * my == 12
    assert d.count(b"\xff\xd7") >= 1 and d.count(b"\xff\xd0") >= 2                         # the counter wrapped past D7
    return d


def case_restart_short_last_segment():
    d = colour_jpeg(64, 48, 2, 80, restart_marker_blocks=5)
    j = J.parse_jpeg(d)
    mx, my = _mcus(j)
    assert j.restart_interval == 5 and (mx * my) % 5 != 0 and len(entropy_segments(d)) == -(-(mx * my) // 5)
    return d


def case_restart_rows():
    d = colour_jpeg(70, 50, 2, 80, restart_marker_rows=1)
    j = J.parse_jpeg(d)
    mx, my = _mcus(j)
    assert j.restart_interval == mx and len(entropy_segments(d)) == my > 1
    return d


def _check_q100(d):
    j = J.parse_jpeg(d)
    assert any(b"\xff\x00" in d[a:e] for a, e in entropy_segments(d))                      # stuffed bytes inside the entropy-coded data
    max_run, max_piece, _ = code_stats(j)
    assert max_run > 15 and max_piece > 24                                                 # ZRL symbols; symbol + magnitude beyond 24 bits
    return j


def q100_jpeg(w, h):
    """photo() noise at quality 100 (every quantiser 1: long codes, 0xFF bytes); in the left quarter flat blocks that carry one strong coefficient at the highest
    frequency, i.e. behind a run of 62 zeros: three ZRL symbols and a symbol whose code and magnitude bits exceed 24 bits."""
    from PIL import Image
    img = JC.photo(w, h, seed=w + h).astype(float)
    y, x = np.mgrid[0:h, 0:w // 4]
    img[:, :w // 4] = (128 + 104 * np.cos((2 * x + 1) * 7 * np.pi / 16) * np.cos((2 * y + 1) * 7 * np.pi / 16))[:, :, None]
    buf = io.BytesIO()
    Image.fromarray(np.clip(np.rint(img), 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=100, subsampling=2)
    return buf.getvalue()


def case_q100_small():
    d = q100_jpeg(64, 64)
    _check_q100(d)
    return d


def case_q100_large():
    d = q100_jpeg(520, 264)
    j = _check_q100(d)
    blocks = sum(c.shape[0] * c.shape[1] for c in j.coef)
    a, e = entropy_segments(d)[0]
    assert blocks > 64 * BLOCKS_PER_WORKGROUP and e - a > 8 * STUFF_CHUNK                   # many workgroups of both passes, several stuffing chunks
    return d


def case_q5():
    from PIL import Image
    buf = io.BytesIO()
    flat = np.kron(JC.photo(6, 4, seed=9), np.ones((16, 16, 1), np.uint8))                  # one colour per MCU: nothing but DC differences
    flat[40:48, 8:24] = JC.photo(16, 8, seed=2)                                             # ... and two blocks that are not
    Image.fromarray(flat).save(buf, "JPEG", quality=5, subsampling=2)
    d = buf.getvalue()
    j = J.parse_jpeg(d)
    zz = np.concatenate([c.reshape(-1, 64) for c in j.coef])
    assert 0.9 < (np.count_nonzero(zz[:, 1:], axis=1) == 0).mean() < 1                        # most blocks are DC + EOB
    assert code_stats(j)[2] < 8                                                             # blocks shorter than a byte: neighbours share words
    return d


def case_three_scans(jx):
    """A baseline 4:2:0 file re-serialised by the host writer with one scan per component (as tests/test_jpeg_transcode.py does)."""
    import test_jpeg_transcode as T
    data = colour_jpeg(67, 39, 2, 85)
    j = J.parse_jpeg(data)
    first = j.marker_order.index(0xDA)
    j.marker_order[first:first + 1] = [0xDA] * 3
    j.scans = [dict(comps=[c]) for c in j.scans[0]["comps"]]
    j.padding_bits = []
    split = T._write(jx, j, J.build_jbrd(j))
    k = J.parse_jpeg(split)
    assert len(k.scans) == 3 and all(len(s["comps"]) == 1 for s in k.scans) and k.components[0]["h"] == 2
    mx, my = _mcus(k)
    assert -(-k.width // 8) < 2 * mx and -(-k.height // 8) < 2 * my                          # the luma scan's own grid is smaller than the MCU-padded plane it indexes
    assert np.array_equal(JC.pil_pixels(split), JC.pil_pixels(data))                        # (the padding blocks no scan codes any more do not show)
    return split


def case_optimize():
    d = colour_jpeg(90, 70, 2, 85, optimize=True)
    j = J.parse_jpeg(d)
    assert all(len(h["values"]) < (100 if h["is_ac"] else 12) for h in j.huff)               # tables that lack most of the 162 / 12 symbols
    return d


SHAPES = {
    "grey_8x8": lambda jx: case_grey_one_block(),
    "420_9x9": lambda jx: case_420(9, 9, True),
    "420_17x23": lambda jx: case_420(17, 23, False),
    "420_33x40_odd_mcus": lambda jx: case_420(33, 40, True),
    "422_50x37": lambda jx: case_422(),
    "restart_every_mcu": lambda jx: case_restart_every_mcu(),
    "restart_short_last": lambda jx: case_restart_short_last_segment(),
    "restart_rows": lambda jx: case_restart_rows(),
    "q100_small": lambda jx: case_q100_small(),
    "q100_520x264": lambda jx: case_q100_large(),
    "q5": lambda jx: case_q5(),
    "three_scans": case_three_scans,
    "optimize": lambda jx: case_optimize(),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_take_the_device_path(jx, name):
    data = SHAPES[name](jx)
    b, out = reconstruct_batch(jx, [J.transcode(data)])
    assert out[0] == data
    assert b.info_value("jpeg_device_images") == 1 and b.info_value("jpeg_host_images") == 0


# ---- 4: recorded padding bits -------------------------------------------------------------------------------------------------------------
def zero_padded_file():
    """A baseline file with restart markers whose padding in front of one RSTn and in front of EOI has its last bit cleared (a 0 among the padding bits, which jbrd then
    records); the variant is kept only if the cleared bits were padding — the coefficients are unchanged and libjpeg decodes the file."""
    data = colour_jpeg(64, 48, 2, 80, restart_marker_blocks=2)
    ref = J.parse_jpeg(data)
    assert all(b == 1 for b in ref.padding_bits)
    segs = entropy_segments(data)
    for k in range(len(segs) - 1):
        mod = bytearray(data)
        ends = (segs[k][1], segs[-1][1])
        if any(mod[e - 1] == 0 and mod[e - 2] == 0xFF for e in ends) or not all(mod[e - 1] & 1 for e in ends):
            continue
        for e in ends:
            mod[e - 1] &= 0xFE
        mod = bytes(mod)
        try:
            j = J.parse_jpeg(mod)
        except (AssertionError, IndexError, KeyError):
            continue
        if j.padding_bits.count(0) == 2 and all(np.array_equal(a, b) for a, b in zip(j.coef, ref.coef)):
            JC.pil_pixels(mod)
            return mod, j
    raise AssertionError("no variant with zero padding bits found")


def test_zero_padded_case_holds():
    mod, j = zero_padded_file()
    assert 0 in j.padding_bits and mod[-2:] == b"\xff\xd9"


@pytest.mark.gpu
def test_recorded_padding_bits(jx):
    """The device writes the segments, the host pads their last bytes from jbrd's recorded bits (cursor running across the restart segments): device path."""
    mod, j = zero_padded_file()
    assert 0 in j.padding_bits
    b, out = reconstruct_batch(jx, [J.transcode(mod)])
    assert out[0] == mod
    assert b.info_value("jpeg_device_images") == 1


# ---- 5: failures stay with their image ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_failures_stay_with_their_image(jx):
    good = colour_jpeg(100, 60, 2, 80, restart_marker_blocks=3)
    jxl = J.transcode(good)
    j = J.parse_jpeg(good)
    jbrd = J.build_jbrd(j)
    at = jxl.rindex(b"jxlc")
    cs = jxl[at + 4:]
    assert jxl == J.container(jbrd, cs)
    rng = np.random.default_rng(11)
    mutated = []
    for k in range(5):
        bad = bytearray(cs)
        for pos in rng.integers(len(cs) * 6 // 10, len(cs), 1 + k % 3):                      # the AC sections fill the back of the codestream
            bad[pos] ^= 1 << int(rng.integers(0, 8))
        mutated.append(J.container(jbrd, bytes(bad)))
    mutated.append(J.container(jbrd, cs[:-40]))
    batch = [jxl, fixture_bytes("sample.jxl"), J.container(jbrd[:len(jbrd) // 2], cs)] + mutated
    b = jx.BatchDecoder()
    index = []
    for d in batch:
        try:
            index.append(b.add(d))
        except jx.DecodeError as e:                                                         # (a stream the host parser refuses never enters the batch)
            assert str(e)
            index.append(None)
    assert index[0] == 0 and index[1] is not None and index[2] is not None
    b.reconstruct_jpegs()
    assert b.jpeg(index[0]) == good
    for i, why in ((index[1], "no jbrd box"), (index[2], "jbrd")):
        assert not b.can_reconstruct_jpeg(i)
        with pytest.raises(jx.DecodeError, match=why):
            b.jpeg(i)
    for i in index[3:]:
        if i is None:
            continue
        try:
            got = b.jpeg(i)
        except jx.DecodeError as e:
            assert str(e)
            continue
        assert len(got) > 4 and got[:2] == b"\xff\xd8" and got[-2:] == b"\xff\xd9"
    _, again = reconstruct_batch(jx, [jxl])
    assert again[0] == good


# ---- 6: the pixel path is untouched ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pixel_decode_after_reconstruction(jx):
    datas = [J.transcode(colour_jpeg(67, 45, 2, 85)), J.transcode(colour_jpeg(64, 48, 0, 80, restart_marker_blocks=2))]
    b = jx.BatchDecoder()
    for d in datas:
        b.add(d)
    b.reconstruct_jpegs()
    b.reset()

    def pixels(dec):
        for d in datas:
            dec.add(d, num_channels=3)
        dec.prepare(); dec.decode(); dec.finish()
        return [dec.output(i) for i in range(len(datas))]
    again, fresh = pixels(b), pixels(jx.BatchDecoder())
    assert all(np.array_equal(a, f) for a, f in zip(again, fresh))


# ---- 7: the marker / splice half on the CPU, under ASan + UBSan ------------------------------------------------------------------------------
def test_splice_of_segment_records_host_only(tmp_path):
    """tests/jpeg_splice_check.cc: sample.jpg assembled from the jbrd box of sample_jpg.jxl and the segment bytes cut out of the file itself; synthetic
    records for padding with ones / recorded bits, a padded 0xFF, the RSTn counter past D7, exhausted padding bits."""
    exe = str(tmp_path / "jpeg_splice_check")
    csrc = os.path.join(ROOT, "jpegxl-rs_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "jpeg_splice_check.cc"), os.path.join(csrc, "jpeg_recon.cc"), "-ldl"])
    out = subprocess.run([exe, os.path.join(FIXTURES, "sample_jpg.jxl"), os.path.join(FIXTURES, "sample.jpg")], capture_output=True, text=True)
    sys.stdout.write(out.stdout + out.stderr)
    assert out.returncode == 0 and "0 failures" in out.stdout
