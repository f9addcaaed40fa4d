"""Progressive scans of the batch JPEG reconstruction written by the device (BatchDecoder.reconstruct_jpegs(progressive_on_device=True), batch option
"jpeg_device_progressive"; csrc/jpeg_write.hip).  The yardstick is the JPEG file that Pillow's libjpeg wrote, byte for byte.

The device does not walk a scan block after block the way the canonical writer does (csrc/jpeg_recon.cc EobState): every block gets a `head` (the bits it emits itself),
a `tail` (the correction bits it buffers) and, where it starts an end-of-band run, the EOBn symbol between the two; the stream is the concatenation in block order.
`model_segments` below restates that form in Python with the Huffman tables of the file's own DHT markers; the CPU test holds it against the files, the second CPU test
holds the lane arithmetic of the refinement kernel (masks, popcounts, prefix sums) against the serial walk."""
import io
import struct

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_tools as J
import test_jpeg_batch as B
from conftest import fixture_bytes

EOB_RUN_MAX = 0x7FFF
TAIL_LIMIT = (1 << 16) - 64 + 1      # 65473: the canonical writer flushes once more correction bits than this wait for their run


@pytest.fixture(scope="module")
def jx(built):
    import jpegxl_rs_amd as jx
    return jx


# ---- the file's own tables and segments ---------------------------------------------------------------------------------------------------------
def _codes(counts, vals):
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            out[vals[k]] = format(code, "0%db" % ln)
            code += 1; k += 1
        code <<= 1
    return out


def scan_tables(data):
    """Per SOS marker of the file: the Huffman tables in force (symbol -> code as a bit string) and the restart interval."""
    out, pos, dc, ac, restart = [], 2, {}, {}, 0
    while data[pos + 1] != 0xD9:
        m, ln = data[pos + 1], struct.unpack(">H", data[pos + 2:pos + 4])[0]
        seg = data[pos + 4:pos + 2 + ln]
        pos += 2 + ln
        if m == 0xC4:
            p = 0
            while p < len(seg):
                counts = list(seg[p + 1:p + 17]); n = sum(counts)
                (ac if seg[p] >> 4 else dc)[seg[p] & 15] = _codes(counts, list(seg[p + 17:p + 17 + n]))
                p += 17 + n
        elif m == 0xDD:
            restart = struct.unpack(">H", seg[:2])[0]
        elif m == 0xDA:
            out.append(dict(dc=dict(dc), ac=dict(ac), restart=restart))
            while not (data[pos] == 0xFF and data[pos + 1] != 0 and not 0xD0 <= data[pos + 1] <= 0xD7):
                pos += 1
    return out


def scan_blocks(j, scan):
    """The blocks of a scan in scan order: (MCU index, component, zigzag coefficients, dc table, ac table)."""
    comps = scan["comps"]
    maxh = max(c["h"] for c in j.components); maxv = max(c["v"] for c in j.components)
    inter = len(comps) > 1
    if inter:
        cols, rows = -(-j.width // (8 * maxh)), -(-j.height // (8 * maxv))
    else:
        c = j.components[comps[0][0]]
        cols = -(-(j.width * c["h"]) // (8 * maxh)); rows = -(-(j.height * c["v"]) // (8 * maxv))
    zz = {ci: j.coef[ci][:, :, J.ZIGZAG].astype(np.int32) for ci, _, _ in comps}
    out = []
    if not inter:
        ci, dct, act = comps[0]
        flat = zz[ci][:rows, :cols].reshape(-1, 64)
        return [(k, ci, flat[k], dct, act) for k in range(rows * cols)], cols * rows
    for my in range(rows):
        for mx in range(cols):
            for ci, dct, act in comps:
                c = j.components[ci]
                for iy in range(c["v"]):
                    for ix in range(c["h"]):
                        out.append((my * cols + mx, ci, zz[ci][my * c["v"] + iy, mx * c["h"] + ix], dct, act))
    return out, cols * rows


# ---- what one block contributes (T.81 G.1.2; csrc/jpeg_recon.cc EncodeBlockProgressive / EncodeBlockRefinement) ---------------------------------
def _magnitude(v, negative, nbits):
    return format((~v if negative else v) & ((1 << nbits) - 1), "0%db" % nbits) if nbits else ""


def ac_first_block(blk, ss, se, al, act, stats):
    """head, tail, joins of a block of a first AC scan: ZRLs, symbols and magnitude bits of |c| >> Al; trailing zeros join the end-of-band run."""
    out, r = [], 0
    for k in range(ss, se + 1):
        c = int(blk[k]); v = abs(c) >> al
        if v == 0:
            r += 1
            continue
        while r > 15:
            out.append(act[0xF0]); r -= 16
        nb = v.bit_length()
        out.append(act[(r << 4) + nb] + _magnitude(v, c < 0, nb))
        r = 0
    return "".join(out), "", r > 0


def ac_refine_block(blk, ss, se, al, act, stats):
    """head, tail, joins of a block of an AC refinement scan, as EncodeBlockRefinement emits: correction bits ride behind the next symbol."""
    a = [abs(int(blk[k])) >> al for k in range(64)]
    eob = max([k for k in range(ss, se + 1) if a[k] == 1], default=0)
    out, gathered, r = [], [], 0
    for k in range(ss, se + 1):
        if a[k] == 0:
            r += 1
            continue
        here = 0
        while r > 15 and k <= eob:
            out.append(act[0xF0]); r -= 16; here += 1
            out.extend(gathered); gathered = []
        if here:
            stats["refine_zrl"] += here
            stats["refine_zrl_repeated"] += here > 1
        if a[k] > 1:
            gathered.append(str(a[k] & 1))
            continue
        out.append(act[(r << 4) + 1] + ("0" if blk[k] < 0 else "1"))
        out.extend(gathered); gathered = []
        r = 0
    return "".join(out), "".join(gathered), r > 0 or bool(gathered)


def eob_symbol(n, act):
    nbits = n.bit_length() - 1
    return act[nbits << 4] + (format(n & ((1 << nbits) - 1), "0%db" % nbits) if nbits else "")


def stuff(raw: bytes) -> bytes:
    return raw.replace(b"\xff", b"\xff\x00")


_MODELS = {}


def model_segments(data, j=None, use_reset_points=True):
    """model_segments_uncached, once per file (the cases assert on the facts, the CPU test compares the segments)."""
    key = (data, use_reset_points)
    if key not in _MODELS:
        _MODELS[key] = model_segments_uncached(data, j, use_reset_points)
    return _MODELS[key]


def model_segments_uncached(data, j=None, use_reset_points=True):
    """The entropy-coded segments of a progressive file from its coefficients, in the block-ordered form: per block head | EOBn if it is a run head | tail.  Returns
    the segments (padded with ones, stuffed) and per-scan facts the cases assert.  Without the reset points the runs are not the file's any more and its tables need
    not have their EOBn symbols: the facts only, no segments."""
    j = j or J.parse_jpeg(data)
    assert j.sof == 0xC2
    segments, facts = [], []
    for scan, tabs in zip(j.scans, scan_tables(data)):
        ss, se, ah, al = scan["ss"], scan["se"], scan["ah"], scan["al"]
        blocks, mcus = scan_blocks(j, scan)
        per_mcu = len(blocks) // mcus
        per_seg = tabs["restart"] * per_mcu if tabs["restart"] else len(blocks)
        st = dict(ss=ss, se=se, ah=ah, al=al, blocks=len(blocks), refine_zrl=0, refine_zrl_repeated=0, max_run=0, max_span_tail=0, tail_only_span=0, zero_bit_blocks=0,
                  reset_points=len(scan["reset_points"]), first_segment=len(segments))
        n = len(blocks)
        head, tail, joins = [""] * n, [""] * n, [False] * n
        if ss == 0:
            assert se == 0
            last = {}
            for b, (mcu, ci, blk, dct, act) in enumerate(blocks):
                if ah:
                    head[b] = str((int(blk[0]) >> al) & 1)
                    continue
                if b % per_seg == 0:
                    last = {}
                v = int(blk[0]) >> al
                d = v - last.get(ci, 0); last[ci] = v
                nb = abs(d).bit_length()
                assert nb < 13
                head[b] = tabs["dc"][dct][nb] + _magnitude(abs(d), d < 0, nb)
        else:
            assert len(scan["comps"]) == 1
            act = tabs["ac"][scan["comps"][0][2]]
            band = np.stack([blk[ss:se + 1] for _, _, blk, _, _ in blocks])
            active = ((np.abs(band) >> al) != 0).any(axis=1)
            one = ac_refine_block if ah else ac_first_block
            for b in range(n):
                if active[b]:
                    head[b], tail[b], joins[b] = one(blocks[b][2], ss, se, al, act, st)
                else:
                    joins[b] = True
        eob = [0] * n
        resets = set(scan["reset_points"]) if use_reset_points else set()
        for lo in range(0, n, per_seg):
            hi = min(lo + per_seg, n)
            if ss > 0:
                flush = [b for b in range(lo, hi) if b == lo or head[b] or b in resets]          # a block that breaks, a reset point, the segment's first block
                for f, e in zip(flush, flush[1:] + [hi]):
                    first = f if joins[f] else f + 1                                                # the span's joining blocks: first .. e - 1
                    for at in range(first, e, EOB_RUN_MAX):
                        eob[at] = min(EOB_RUN_MAX, e - at)                                          # run heads
                    span_tail = sum(len(tail[b]) for b in range(first, e))
                    st["max_span_tail"] = max(st["max_span_tail"], span_tail)
                    st["max_run"] = max(st["max_run"], e - first)
                    if not head[f] and span_tail > 0:
                        st["tail_only_span"] = max(st["tail_only_span"], e - f)
            if not use_reset_points:
                continue
            bits = "".join(head[b] + (eob_symbol(eob[b], act) if eob[b] else "") + tail[b] for b in range(lo, hi))
            st["zero_bit_blocks"] += sum(1 for b in range(lo, hi) if not head[b] and not eob[b] and not tail[b])
            bits += "1" * (-len(bits) % 8)
            segments.append(stuff(int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""))
        st["segments"] = len(segments) - st["first_segment"]
        facts.append(st)
    return segments, facts


def file_segments(data):
    return [data[a:e] for a, e in B.entropy_segments(data)]


# ---- the lane form of the refinement kind (jpeg_write.hip RefineLane): every lane places its own pieces ------------------------------------------
def _below(k):
    return (1 << k) - 1


def _between(lo, hi):
    """bits lo + 1 .. hi - 1"""
    return _below(hi) & ~_below(lo + 1) if hi > lo + 1 else 0


def _popc(x):
    return bin(x).count("1")


def refine_lanes(blk, ss, se, al, act):
    """head and tail of a refinement block assembled from per-lane pieces at per-lane offsets, with the masks and counts the kernel uses."""
    a = [(abs(int(blk[k])) >> al) if ss <= k <= se else 0 for k in range(64)]
    newm = sum(1 << k for k in range(64) if a[k] == 1)
    oldm = sum(1 << k for k in range(64) if a[k] > 1)
    nzm = newm | oldm
    zerom = (_below(se + 1) & ~_below(ss)) & ~nzm
    eob = newm.bit_length() - 1 if newm else 0
    zl = len(act.get(0xF0, ""))
    A, Bn, pieceA, pieceB, event = [0] * 64, [0] * 64, [""] * 64, [""] * 64, 0
    for k in range(64):
        if not (nzm >> k) & 1 or k > eob:
            continue
        lastnew = newm & _below(k)
        ln = lastnew.bit_length() - 1 if lastnew else ss - 1
        z = _popc(zerom & _between(ln, k))
        pn = nzm & _between(ln, k)
        zprev = _popc(zerom & _between(ln, pn.bit_length() - 1)) if pn else 0
        nz = (z >> 4) - (zprev >> 4)
        sym = (act[((z & 15) << 4) + 1] + ("0" if blk[k] < 0 else "1")) if (newm >> k) & 1 else ""
        if nz:
            pieceA[k], pieceB[k] = act[0xF0], act[0xF0] * (nz - 1) + sym
        else:
            pieceA[k] = sym
        A[k], Bn[k] = len(pieceA[k]), len(pieceB[k])
        if nz or sym:
            event |= 1 << k
        assert not nz or A[k] == zl
    exE = [sum(A[q] + Bn[q] for q in range(k)) for k in range(64)]
    head_len = sum(A) + sum(Bn) + (_popc(oldm & _below(eob)) if newm else 0)
    tail_len = _popc(oldm & ~_below(eob + 1))
    head, tail = [None] * head_len, [None] * tail_len

    def put(buf, at, s):
        for i, ch in enumerate(s):
            assert buf[at + i] is None
            buf[at + i] = ch
    for k in range(64):
        if (event >> k) & 1:
            pem = event & _below(k)
            olds_before = _popc(oldm & _below(pem.bit_length() - 1)) if pem else 0
            put(head, exE[k] + olds_before, pieceA[k])
            put(head, exE[k] + A[k] + _popc(oldm & _below(k)), pieceB[k])
        if (oldm >> k) & 1:
            if newm and k < eob:
                later = event & ~_below(k + 1)
                ne = (later & -later).bit_length() - 1
                put(head, exE[ne] + A[ne] + _popc(oldm & _below(k)), str(a[k] & 1))
            else:
                put(tail, _popc(oldm & ~_below(eob + 1) & _below(k)), str(a[k] & 1))
    assert None not in head and None not in tail
    return "".join(head), "".join(tail)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------
def save_jpeg(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", progressive=True, **kw)
    return buf.getvalue()


def prog_colour(w, h, ss, q, **kw):
    return save_jpeg(JC.photo(w, h, seed=w + h), quality=q, subsampling=ss, **kw)


def _sampling(j):
    return [(c["h"], c["v"]) for c in j.components]


def case_grey_one_block():
    d = save_jpeg(JC.photo(8, 8, seed=16)[:, :, 0], quality=85)
    j = J.parse_jpeg(d)
    assert len(j.components) == 1 and j.coef[0].shape[:2] == (1, 1) and len(j.scans) == 6            # one block, six scans
    return d, j


def case_padded(w, h, ss, sampling, smaller_grid):
    d = prog_colour(w, h, ss, 85)
    j = J.parse_jpeg(d)
    mx, my = B._mcus(j)
    assert _sampling(j) == sampling and (w % (8 * sampling[0][0]) or h % (8 * sampling[0][1]))       # MCU padding
    # the luma scans walk a grid of their own, smaller than the MCU-padded plane wherever the size allows it (9 x 9 fills its one MCU)
    assert any(len(s["comps"]) == 1 and s["comps"][0][0] == 0 for s in j.scans)
    assert (-(-w // 8) < mx * sampling[0][0] or -(-h // 8) < my * sampling[0][1]) == smaller_grid
    return d, j


def case_restart(every):
    d = prog_colour(64, 48, 2, 80, restart_marker_blocks=every)
    j = J.parse_jpeg(d)
    mx, my = B._mcus(j)
    assert j.restart_interval == every and _sampling(j)[0] == (2, 2)
    mcus = [scan_blocks(j, s)[1] for s in j.scans]
    assert len(B.entropy_segments(d)) == sum(-(-n // every) for n in mcus)                           # every == 1: a flush and a byte boundary per MCU
    assert every == 1 or all(n % every for n in mcus)                                                # a short last segment in every scan
    return d, j


def case_gratings():
    d = JC.jpeg_bytes(JC.PROGRESSIVE[5])
    j = J.parse_jpeg(d)
    assert sum(1 for s in j.scans if s["reset_points"]) >= 2                                         # >= 1 reset point in two scans
    _, facts = model_segments(d, j)
    assert max(f["tail_only_span"] for f in facts) >= j.width // 8                                           # spans of whole block rows carrying only tails
    return d, j


def flat_1480():
    img = np.full((1480, 1480, 3), 97, np.uint8)
    img[:8, :8] = JC.photo(8, 8, seed=5)
    return save_jpeg(img, quality=85, subsampling=0)


def case_flat_1480():
    d = flat_1480()
    j = J.parse_jpeg(d)
    assert _sampling(j) == [(1, 1)] * 3 and len(d) < 40000
    _, facts = model_segments(d, j)
    assert max(f["max_run"] for f in facts) >= 34224 > EOB_RUN_MAX                                   # at least one EOB32767 and a second run behind it
    return d, j


def high_frequency_image():
    img = JC.photo(64, 64, seed=128).astype(float)
    y, x = np.mgrid[0:64, 0:32]
    rng = np.random.default_rng(7)
    img[:, :32] = (128 + 104 * np.cos((2 * x + 1) * 7 * np.pi / 16) * np.cos((2 * y + 1) * 7 * np.pi / 16))[:, :, None] + rng.normal(0, 1.5, (64, 32, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def case_refinement_zrl():
    d = save_jpeg(high_frequency_image(), quality=92, subsampling=0)
    j = J.parse_jpeg(d)
    _, facts = model_segments(d, j)
    assert sum(f["refine_zrl"] for f in facts) >= 1 and sum(f["refine_zrl_repeated"] for f in facts) >= 1      # ZRLs inside refinement scans; several at one position
    return d, j


def case_refinement_q100():
    d = save_jpeg(high_frequency_image(), quality=100, subsampling=2)
    j = J.parse_jpeg(d)
    segs, facts = model_segments(d, j)
    refine = [f for f in facts if f["ah"] and f["ss"]]
    assert any(b"\xff\x00" in s for f in refine for s in segs[f["first_segment"]:f["first_segment"] + f["segments"]])          # stuffed bytes inside refinement data
    return d, j


def case_q5_progressive():
    flat = np.kron(JC.photo(6, 4, seed=9), np.ones((16, 16, 1), np.uint8))                           # the picture of test_jpeg_batch.case_q5
    flat[40:48, 8:24] = JC.photo(16, 8, seed=2)
    d = save_jpeg(flat, quality=5, subsampling=2)
    j = J.parse_jpeg(d)
    _, facts = model_segments(d, j)
    ac = [f for f in facts if f["ss"]]
    assert sum(f["zero_bit_blocks"] for f in ac) > 0.9 * sum(f["blocks"] for f in ac)                # most blocks contribute 0 bits to the AC scans: neighbours share words
    return d, j


def case_many_workgroups():
    d = JC.jpeg_bytes(JC.PROGRESSIVE[4])
    j = J.parse_jpeg(d)
    _, facts = model_segments(d, j)
    assert sum(f["refine_zrl"] for f in facts) > 100 and sum(c.shape[0] * c.shape[1] for c in j.coef) > 64 * B.BLOCKS_PER_WORKGROUP
    return d, j


SHAPES = {
    "grey_8x8": case_grey_one_block,
    "420_9x9": lambda: case_padded(9, 9, 2, [(2, 2), (1, 1), (1, 1)], False),
    "420_17x23": lambda: case_padded(17, 23, 2, [(2, 2), (1, 1), (1, 1)], True),
    "422_50x37": lambda: case_padded(50, 37, 1, [(2, 1), (1, 1), (1, 1)], True),
    "restart_every_mcu": lambda: case_restart(1),
    "restart_short_last": lambda: case_restart(5),
    "gratings": case_gratings,
    "flat_1480": case_flat_1480,
    "refinement_zrl": case_refinement_zrl,
    "refinement_q100_420": case_refinement_q100,
    "q5": case_q5_progressive,
    "300x280": case_many_workgroups,
}


# ---- CPU: the formulation against libjpeg's files -----------------------------------------------------------------------------------------------
def _all_inputs():
    for c in JC.PROGRESSIVE:
        yield "progressive %dx%d" % c[:2], JC.jpeg_bytes(c), None
    for name, make in SHAPES.items():
        if name not in ("gratings", "300x280"):                                                     # (both are PROGRESSIVE files)
            d, j = make()
            yield name, d, j


def test_block_ordered_form_reproduces_the_files():
    for name, data, j in _all_inputs():
        got, _ = model_segments(data, j)
        want = file_segments(data)
        assert len(got) == len(want), name
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == w, "%s: segment %d differs" % (name, k)


def test_lane_form_of_refinement_equals_the_serial_walk():
    checked = zrls = 0
    for data in (JC.jpeg_bytes(JC.PROGRESSIVE[4]), case_refinement_zrl()[0], case_refinement_q100()[0]):
        j = J.parse_jpeg(data)
        for scan, tabs in zip(j.scans, scan_tables(data)):
            if not (scan["ss"] and scan["ah"]):
                continue
            act = tabs["ac"][scan["comps"][0][2]]
            st = dict(refine_zrl=0, refine_zrl_repeated=0)
            for _, _, blk, _, _ in scan_blocks(j, scan)[0]:
                serial = ac_refine_block(blk, scan["ss"], scan["se"], scan["al"], act, st)
                assert refine_lanes(blk, scan["ss"], scan["se"], scan["al"], act) == serial[:2]
                checked += 1
            zrls += st["refine_zrl_repeated"]
    assert checked > 3000 and zrls > 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------
def reconstruct(jx, jxls, on_device=True, host_writer=False):
    b = jx.BatchDecoder()
    if host_writer:
        b.set_option("jpeg_host_writer", 1)
    for d in jxls:
        b.add(d)
    b.reconstruct_jpegs(progressive_on_device=on_device)
    return b, [b.jpeg(i) for i in range(len(jxls))]


def counts(b):
    return tuple(b.info_value(k) for k in ("jpeg_device_images", "jpeg_host_images", "jpeg_device_progressive_images"))


@pytest.fixture(scope="module")
def real_files():
    base = [JC.jpeg_bytes(c) for c in JC.CASES] + [JC.grey_jpeg_bytes(75, 52, 85), JC.grey_jpeg_bytes(41, 30, 70, optimize=True)]
    prog = [JC.jpeg_bytes(c) for c in JC.PROGRESSIVE]
    sample = fixture_bytes("sample.jpg")
    files = base + prog + [sample]                                                                  # the batch of test_jpeg_batch.real_files
    jxls = [J.transcode(d) for d in base + prog] + [fixture_bytes("sample_jpg.jxl")]
    return files, jxls


@pytest.mark.gpu
def test_every_real_file_on_the_device(jx, real_files):
    files, jxls = real_files
    b, out = reconstruct(jx, jxls)
    for i, (got, want) in enumerate(zip(out, files)):
        assert got == want, "image %d differs" % i
    n_prog = sum(1 for d in files if J.parse_jpeg(d).sof == 0xC2)
    assert n_prog >= len(JC.PROGRESSIVE)
    assert counts(b) == (len(files), 0, n_prog)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_progressive_shapes(jx, name):
    data, j = SHAPES[name]()
    assert j.sof == 0xC2
    b, out = reconstruct(jx, [J.transcode(data)])
    assert out[0] == data
    assert counts(b) == (1, 0, 1)


def _without_reset_points(data):
    """The transcode of a file with its reset points dropped from the reconstruction data.  libjpeg's progressive files carry tables made for their own symbols, and
    the longer end-of-band runs need EOBn symbols the file never used: every AC table is replaced by one that has a code (9 or 10 bits) for every symbol."""
    j = J.parse_jpeg(data)
    _, facts = model_segments(data, j, use_reset_points=False)
    assert any(s["reset_points"] for s in j.scans)
    for s in j.scans:
        s["reset_points"] = []
    for h in j.huff:
        if h["is_ac"]:
            h["counts"] = [0] * 8 + [200, 56] + [0] * 6
            h["values"] = list(range(256))
    jxl = J.transcode(data)
    return J.container(J.build_jbrd(j), jxl[jxl.rindex(b"jxlc") + 4:]), max(f["max_span_tail"] for f in facts), j


@pytest.mark.gpu
def test_without_reset_points(jx):
    """Without reset points the canonical writer extends end-of-band runs that libjpeg cut: another, equally valid file.  Below 65473 waiting correction bits the
    device writes it; beyond, the position of the writer's flush depends on the running sum and the image is handed to the host."""
    data = JC.jpeg_bytes(JC.PROGRESSIVE[5])
    jxl, longest, _ = _without_reset_points(data)
    print("gratings 1024x256 without reset points: longest span holds %d tail bits" % longest)
    assert 937 < longest <= TAIL_LIMIT
    b, out = reconstruct(jx, [jxl])
    assert counts(b) == (1, 0, 1)
    _, host = reconstruct(jx, [jxl], host_writer=True)
    assert out[0] == host[0] and out[0] != data
    assert np.array_equal(JC.pil_pixels(out[0]), JC.pil_pixels(data))

    big = save_jpeg(JC.gratings(2048, 1024)[:, :, 0], quality=90)
    jxl, longest, _ = _without_reset_points(big)
    print("grey gratings 2048x1024 without reset points: longest span holds %d tail bits" % longest)
    assert longest > TAIL_LIMIT
    b, out = reconstruct(jx, [jxl])
    assert counts(b) == (0, 1, 0)
    _, host = reconstruct(jx, [jxl], host_writer=True)
    assert out[0] == host[0]
    assert np.array_equal(JC.pil_pixels(out[0]), JC.pil_pixels(big))


@pytest.mark.gpu
def test_failures_and_switches(jx):
    good = JC.jpeg_bytes(JC.PROGRESSIVE[3])                                                         # progressive, restart markers
    baseline = B.colour_jpeg(67, 45, 2, 85)
    jxl, jxl_base = J.transcode(good), J.transcode(baseline)
    jbrd = J.build_jbrd(J.parse_jpeg(good))
    cs = jxl[jxl.rindex(b"jxlc") + 4:]
    assert jxl == J.container(jbrd, cs)
    rng = np.random.default_rng(5)
    mutated = []
    for k in range(5):
        bad = bytearray(cs)
        for pos in rng.integers(len(cs) * 6 // 10, len(cs), 1 + k % 3):
            bad[pos] ^= 1 << int(rng.integers(0, 8))
        mutated.append(J.container(jbrd, bytes(bad)))
    mutated.append(J.container(jbrd, cs[:-40]))
    b = jx.BatchDecoder()
    index = []
    for d in [jxl, jxl_base] + mutated:
        try:
            index.append(b.add(d))
        except jx.DecodeError as e:
            assert str(e)
            index.append(None)
    assert index[:2] == [0, 1]
    b.reconstruct_jpegs(progressive_on_device=True)
    assert b.jpeg(0) == good and b.jpeg(1) == baseline
    for i in index[2:]:
        if i is None:
            continue
        try:
            got = b.jpeg(i)
        except jx.DecodeError as e:
            assert str(e)
            continue
        assert len(got) > 4 and got[:2] == b"\xff\xd8" and got[-2:] == b"\xff\xd9"
    # the switches
    pair = [jxl, jxl_base]
    b_off, out = reconstruct(jx, pair, on_device=False)
    assert out == [good, baseline] and counts(b_off) == (1, 1, 0)                                  # the parent's counts
    b_host, out = reconstruct(jx, pair, host_writer=True)
    assert out == [good, baseline] and counts(b_host) == (0, 2, 0)                                 # jpeg_host_writer overrides the option
    b_on, out = reconstruct(jx, pair)
    assert out == [good, baseline] and counts(b_on) == (2, 0, 1)
    # a pixel decode from the same BatchDecoder, reset
    b_on.reset()

    def pixels(dec):
        for d in pair:
            dec.add(d, num_channels=3)
        dec.prepare(); dec.decode(); dec.finish()
        return [dec.output(i) for i in range(len(pair))]
    again, fresh = pixels(b_on), pixels(jx.BatchDecoder())
    assert all(np.array_equal(a, f) for a, f in zip(again, fresh))
