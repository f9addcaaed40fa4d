"""Extra channels through the frame tail (blending, patches, per-channel upsampling / float conversion, spot colours, un-premultiplied and
non-coalesced output, LF frames, previews), from one channel to nine: the frame tail describes a frame's extra channels by a channel table of any
length (kernels.h EcChanDev), and the streams here are built for channel counts on both sides of four, where an earlier form of the tail changed its path.

How the planes are pinned.  The oracle hands out the colour channels and the FIRST extra channel of type alpha.  A channel's type plays no part
in blending (only its index, the alpha-associated flag of alpha channels and, for the colour, the spot plates do), so extra channel e of a
stream is read from the oracle's decode of the stream's twin in which e is the only channel of type alpha (`relabel=e`: every other channel
becomes `optional`, samples and blending info unchanged).  Lossless samples that no blending touched are pinned against the planes handed to
the synthesiser, which shares nothing with either decoder.

Modes the oracle does not decode (PARITY.md): non-coalesced output and the canvases of an animation's earlier frames are compared with the oracle's decode
of the frame written as an image of its own / of the stream cut behind that frame, as the tests of those modes with fewer channels do.
"""
import ctypes as C
import functools
import numpy as np
import pytest
import oracle_lib as O
import synth_lib as S
import synth_extra as X

W, H, FW, FH, X0, Y0 = 300, 200, 150, 90, 211, -37      # canvas; cropped second frame, partly off the canvas to the right and at the top
OTHER_MODES = [X.REPLACE, X.ADD, X.MULADD, X.MUL, X.BLEND]     # of the channels beside the referred alpha, in turn; that alpha itself blends: all five modes occur from n = 5 on


def _extras(n, relabel=None, alpha_at=5, second_alpha=True, premul_at=None, spots=(), f16_at=None, blend=True, source=1):
    """n channel entries: the alpha that blending refers to at min(alpha_at, n - 1), an unrelated alpha at 0, depth / selection / optional / 16-bit
    channels in between, from n = 5 on every frame-blend mode among them (clamp on for the multiply and one blend channel)."""
    a = min(alpha_at, n - 1)
    out, turn = [], 0
    for k in range(n):
        t = X.ALPHA if k == a or (k == 0 and second_alpha) else (X.DEPTH, X.SELECTION, X.OPTIONAL)[k % 3]
        bits = 16 if k % 4 == 3 else 8
        spot = (0, 0, 0, 0)
        for idx, col in spots:
            if idx == k:
                t, spot = X.SPOT, col
        exp = 0
        if k == f16_at:
            bits, exp, t = 16, 5, X.DEPTH
        mode = X.REPLACE
        if blend and k == a:
            mode = X.BLEND                                  # the alpha channel's own update
        elif blend:
            mode, turn = OTHER_MODES[turn % 5], turn + 1
        premul = 1 if k == premul_at else 0
        if relabel is not None:
            # (a premultiplied alpha keeps its type — the flag is part of the blending arithmetic —, so the twin shows channels up to it only: the oracle hands out the first alpha)
            assert premul_at is None or relabel <= premul_at
            t, spot = (X.ALPHA if k in (relabel, premul_at) else X.OPTIONAL), (0, 0, 0, 0)
        out.append(X.extra(type=t, bits=bits, exp_bits=exp, premultiplied=premul if t == X.ALPHA else 0, mode=mode, alpha=a, clamp=1 if mode == X.MUL or k == 2 else 0,
                           source=source if blend else 0, spot=spot, name=b"ch%d" % k if k % 2 else b""))
    if blend and n >= 5:
        assert {e.blend_mode for e in out} == {0, 1, 2, 3, 4}, "case 4: every frame-blend mode among the extras"
        assert any(e.blend_clamp for e in out if e.blend_mode == X.MUL) and any(e.blend_clamp for e in out if e.blend_mode in (X.BLEND, X.MULADD))
    return out, a


def _planes(n, w, h, seed, extras):
    out = []
    for k in range(n):
        if extras[k].exp_bits:
            out.append(np.float16(X.plane(seed + k, w, h, 8) / 200.0).view(np.uint16).astype(np.int32))
        else:
            out.append(X.plane(seed + k, w, h, extras[k].bits))
    return out


def _as_float(plane, e):
    if e.exp_bits:
        return plane.astype(np.uint16).view(np.float16).astype(np.float32)
    return plane.astype(np.float32) * (np.float32(1.0) / np.float32((1 << e.bits) - 1))


@functools.lru_cache(maxsize=None)
def layered(kind, n, relabel=None, frames=2, upto=None, only=None, premul=False):
    """Two (or three) frames: a full first frame saved as reference 1, then cropped frames blended onto it — colour with mode blend against alpha index min(5, n - 1),
    the extras each with a mode of their own.  upto: the stream cut behind frame `upto` (that frame marked last); only: frame `only` as an image of its own.
    Returns (stream, source planes per frame, extras of the blended frames)."""
    pm = min(5, n - 1) if premul else None            # premul: the alpha that blending refers to is premultiplied
    ex0, a = _extras(n, relabel, blend=False, premul_at=pm)
    ex1, _ = _extras(n, relabel, blend=True, premul_at=pm)
    last = frames - 1 if upto is None else upto
    parts, src = [], []
    for f in range(last + 1):
        fw, fh = (W, H) if f == 0 else (FW, FH)
        img = S.synthetic_image(20 + f, fw, fh)
        ex = ex0 if f == 0 else ex1
        pl = _planes(n, fw, fh, 100 * (f + 1), ex)
        src.append(pl)
        if only is not None and f != only:
            continue
        if only is not None:
            fx = S.frame()
        elif f == 0:
            fx = S.frame(is_last=int(last == 0), save_as_reference=0 if last == 0 else 1, duration=2)
        else:
            fx = S.frame(emit=1, is_last=int(f == last), save_as_reference=0 if f == last else 1, have_crop=1, crop_x0=X0 - 60 * (f - 1), crop_y0=Y0 + 70 * (f - 1), canvas_w=W,
                         canvas_h=H, blend_mode=X.BLEND, blend_source=1, duration=2)
        exf = ex if only is None else _extras(n, relabel, blend=False, premul_at=pm)[0]
        if kind == "vardct":
            parts.append(X.encode_vardct_ec(img, pl, exf, fx, color_alpha=a, seed=3 + f))
        else:
            parts.append(X.encode_modular_ec(img.astype(np.int32), pl, exf, fx, color_alpha=a))
    return b"".join(parts), src, ex1


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


# ---------------------------------------------------------------------------------------------------------------- the C ABI, as a caller drives it
def abi_decode(jx, stream, n, ctype="u8", nch=3, coalescing=True, unpremul=False, spot=True, preview=False):
    """Every frame the decoder delivers: (frame header, blend infos of the extra channels, colour interleave, the n extra-channel planes as f32)."""
    L = jx.libjxl()
    jt, dt = {"u8": (jx.JXL_TYPE_UINT8, np.uint8), "u16": (jx.JXL_TYPE_UINT16, np.uint16), "f32": (jx.JXL_TYPE_FLOAT, np.float32)}[ctype]
    fmt = jx.JxlPixelFormat(nch, jt, jx.JXL_NATIVE_ENDIAN, 0)
    efmt = jx.JxlPixelFormat(1, jx.JXL_TYPE_FLOAT, jx.JXL_NATIVE_ENDIAN, 0)
    data = np.frombuffer(stream, np.uint8)
    dec = L.JxlDecoderCreate(None)
    try:
        ev = jx.JXL_DEC_BASIC_INFO | jx.JXL_DEC_FRAME | (jx.JXL_DEC_PREVIEW_IMAGE if preview else jx.JXL_DEC_FULL_IMAGE)
        assert L.JxlDecoderSubscribeEvents(dec, ev) == 0
        assert L.JxlDecoderSetCoalescing(dec, 1 if coalescing else 0) == 0
        assert L.JxlDecoderSetUnpremultiplyAlpha(dec, 1 if unpremul else 0) == 0
        assert L.JxlDecoderSetRenderSpotcolors(dec, 1 if spot else 0) == 0
        assert L.JxlDecoderSetInput(dec, data.ctypes.data, len(data)) == 0
        L.JxlDecoderCloseInput(dec)
        out, cur, total = [], {}, None      # total: the image's extra channels (n of them are fetched; n = 0: the colour interleave alone)
        while True:
            st = L.JxlDecoderProcessInput(dec)
            if st == jx.JXL_DEC_BASIC_INFO:
                info = jx.JxlBasicInfo()
                assert L.JxlDecoderGetBasicInfo(dec, C.byref(info)) == 0
                total = info.num_extra_channels
                assert n in (0, total)
            elif st == jx.JXL_DEC_FRAME:
                fh = jx.JxlFrameHeader()
                assert L.JxlDecoderGetFrameHeader(dec, C.byref(fh)) == 0
                infos = []
                for k in range(n):
                    bi = jx.JxlBlendInfo()
                    assert L.JxlDecoderGetExtraChannelBlendInfo(dec, k, C.byref(bi)) == 0
                    infos.append((bi.blendmode, bi.source, bi.alpha, bi.clamp))
                bi = jx.JxlBlendInfo()
                assert L.JxlDecoderGetExtraChannelBlendInfo(dec, total, C.byref(bi)) != 0
                cur = {"size": (fh.layer_info.xsize, fh.layer_info.ysize), "infos": infos}
            elif st == jx.JXL_DEC_NEED_PREVIEW_OUT_BUFFER:
                size = C.c_size_t()
                assert L.JxlDecoderPreviewOutBufferSize(dec, C.byref(fmt), C.byref(size)) == 0
                cur["px"] = np.zeros(size.value // np.dtype(dt).itemsize, dt)
                assert L.JxlDecoderSetPreviewOutBuffer(dec, C.byref(fmt), cur["px"].ctypes.data, size.value) == 0
            elif st == jx.JXL_DEC_PREVIEW_IMAGE:
                return [cur]
            elif st == jx.JXL_DEC_NEED_IMAGE_OUT_BUFFER:
                size = C.c_size_t()
                assert L.JxlDecoderImageOutBufferSize(dec, C.byref(fmt), C.byref(size)) == 0
                cur["px"] = np.zeros(size.value // np.dtype(dt).itemsize, dt)
                assert L.JxlDecoderSetImageOutBuffer(dec, C.byref(fmt), cur["px"].ctypes.data, size.value) == 0
                cur["planes"] = []
                for k in range(n):
                    assert L.JxlDecoderExtraChannelBufferSize(dec, C.byref(efmt), C.byref(size), k) == 0, jx.last_error()
                    cur["planes"].append(np.zeros(size.value // 4, np.float32))
                    assert L.JxlDecoderSetExtraChannelBuffer(dec, C.byref(efmt), cur["planes"][k].ctypes.data, size.value, k) == 0
                assert L.JxlDecoderExtraChannelBufferSize(dec, C.byref(efmt), C.byref(size), total) != 0
            elif st == jx.JXL_DEC_FULL_IMAGE:
                out.append(cur)
                cur = dict(cur)
            elif st == jx.JXL_DEC_SUCCESS:
                return out
            else:
                raise jx.DecodeError(jx.last_error())
    finally:
        L.JxlDecoderDestroy(dec)


def assert_colour(got, stream, ctype, nch=3, **okw):
    ref = O.decode(stream)
    if okw.get("unpremul"):
        ref.set_unpremultiply_alpha(True)
    want = ref.pixels(ctype, nch).view(got.dtype)
    assert got.shape == want.shape
    if ctype == "f32":
        gi, wi = got.view(np.int32).astype(np.int64), want.view(np.int32).astype(np.int64)
        gi, wi = np.where(gi < 0, -(gi & 0x7FFFFFFF), gi), np.where(wi < 0, -(wi & 0x7FFFFFFF), wi)
        worst = int(np.abs(gi - wi).max())
        print("colour f32 worst ULP", worst)
        assert worst <= 1
    else:
        print("colour", ctype, "differing samples", int((got != want).sum()))
        assert np.array_equal(got, want)


def oracle_plane(make, e):
    """extra channel e as the oracle decodes it (module docstring: the twin whose only alpha is e)"""
    ref = O.decode(make(e))
    return ref.pixels("f32", 4).view(np.float32).reshape(ref.info.ysize, ref.info.xsize, 4)[..., 3]


def assert_planes(got, make, n):
    for e in range(n):
        want = oracle_plane(make, e)
        g = got[e].reshape(want.shape)
        bad = int((g.view(np.uint32) != want.view(np.uint32)).sum())
        print("plane", e, "differing samples", bad)
        assert bad == 0, (e, bad)


# ---------------------------------------------------------------------------------------------------------------- CPU
NS = [1, 2, 4, 5, 6, 9]


@pytest.mark.parametrize("n", NS)
def test_oracle_decodes_the_streams_and_lossless_planes_are_the_source(n):
    for kind in ("modular", "vardct"):
        stream, src, ex = layered(kind, n, frames=1, upto=0)
        for e in range(n):
            twin, _, _ = layered(kind, n, relabel=e, frames=1, upto=0)
            ref = O.decode(twin)
            assert ref.info.num_extra_channels == n and (ref.info.xsize, ref.info.ysize) == (W, H)
            got = ref.pixels("f32", 4).view(np.float32).reshape(H, W, 4)[..., 3]
            assert np.array_equal(got, _as_float(src[0][e], ex[e])), (kind, e)
        full, _, _ = layered(kind, n)
        assert O.decode(full).info.num_extra_channels == n
    if n != 6:
        return
    # every other stream of the GPU tests below (decoded once, with the n = 6 case), twins included where a twin is what the test reads: (channels, stream)
    makes = [(6, lambda: spot_single(None)), (6, lambda: spot_single(4)), (6, lambda: spot_layered(None)), (6, lambda: spot_layered(1)), (5, lambda: float_stream(None)[0]),
             (5, lambda: float_stream(2)[0]), (5, lambda: upsampled(None)[0]), (5, lambda: upsampled(3)[0]), (5, lambda: xyb_modular(None)), (5, lambda: xyb_modular(4)),
             (6, lambda: patched(None)), (6, lambda: patched(5)), (6, lambda: patched(None, True)), (6, lambda: patched(3, True)), (5, lambda: lf_frame_image(None)),
             (5, lambda: lf_frame_image(2)), (5, lambda: preview_image(None)[0]), (5, lambda: preview_image(None)[1]), (5, lambda: preview_image(1)[0]),
             (6, lambda: premultiplied_image()[0]), (6, lambda: layered("vardct", 6, premul=True)[0]), (6, lambda: layered("vardct", 6, relabel=2, premul=True)[0]),
             (4, lambda: spot_single(None, 4)), (4, lambda: spot_single(2, 4)), (4, lambda: spot_layered(None, 4)), (4, lambda: spot_layered(1, 4)), (4, lambda: float_stream(None, 4)[0]),
             (4, lambda: float_stream(2, 4)[0]), (2, lambda: upsampled(None, 2)[0]), (2, lambda: upsampled(1, 2)[0])]
    for m in PATCHED_NS[:-1]:
        makes += [(m, lambda m=m: patched(None, False, m)), (m, lambda m=m: patched(m - 1, False, m)), (m, lambda m=m: patched(None, True, m)), (m, lambda m=m: patched(0, True, m))]
    for k, (m, make) in enumerate(makes):
        ref = O.decode(make())
        assert ref.info.num_extra_channels == m and ref.info.xsize > 0, k
    S.set_animation(10, 1, 0)
    try:
        layered.cache_clear()
        for f in range(3):
            for e in (None, 0, 5):
                ref = O.decode(layered("modular", 6, relabel=e, frames=3, upto=f)[0])
                assert (ref.info.xsize, ref.info.ysize, ref.info.num_extra_channels) == (W, H, 6)
    finally:
        S.set_animation()
        layered.cache_clear()


@pytest.mark.parametrize("n", NS)
def test_host_parse_reports_every_extra_channel(jxh, n):
    jx = jxh
    L = jx.libjxl()
    spots = ((1, (0.5, 0.25, 1.0, 0.75)), (3, (1.0, 0.0, 0.5, 0.5)))
    ex, a = _extras(n, spots=spots, blend=False)
    stream = X.encode_modular_ec(S.synthetic_image(3, 40, 30).astype(np.int32), _planes(n, 40, 30, 7, ex), ex, color_alpha=a)
    L.JxlHipDebugDescribe.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 16)
    assert L.JxlHipDebugDescribe(stream, len(stream), buf, len(buf)) == 0, jx.last_error()
    lines = buf.value.decode().split("\n")
    assert "extra=%d " % n in lines[0]
    rows = [dict(t.split("=", 1) for t in l.split()[2:]) for l in lines if l.startswith("extra ")]
    assert len(rows) == (n if n > 4 else 0)      # (the description lists the channels one by one from five on; those of images with fewer stay as they always were)
    for k, r in enumerate(rows):
        assert (int(r["type"]), int(r["bits"]), r["name"].encode()) == (ex[k].type, ex[k].bits, ex[k].name), k
        if ex[k].type == X.SPOT:
            assert [float(v) for v in r["spot"].split(",")] == [float(np.float16(v)) for v in ex[k].spot]


def _damaged(stream, lo, hi, count, seed):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(count):
        b = bytearray(stream)
        if i % 4 == 3:
            out.append(bytes(b[:int(rng.randint(lo, hi))]))
        else:
            pos = int(rng.randint(lo, hi))
            b[pos] ^= 1 << int(rng.randint(0, 8))
            out.append(bytes(b))
    return out


def _describe(jx, data):
    L = jx.libjxl()
    L.JxlHipDebugDescribe.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 16)
    return L.JxlHipDebugDescribe(data, len(data), buf, len(buf))


@pytest.mark.parametrize("n", [5, 9])
def test_corrupt_extra_channel_headers_end_cleanly(jxh, n):
    """bit flips / truncations in the image header's extra-channel section (it starts a few bytes in and is 3 - 10 bytes per channel) and in the second
    frame's header with its ec_blend section: an error or a parse, never a crash"""
    first, _, _ = layered("modular", n, frames=1, upto=0)
    full, _, _ = layered("modular", n)
    outcomes = set()
    for bad in _damaged(full, 4, 4 + 10 * n, 24, n) + _damaged(full, len(first), len(first) + 8 + 2 * n, 24, n + 1):
        outcomes.add(_describe(jxh, bad))
    assert outcomes <= {0, 1} and 1 in outcomes


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["vardct", "modular"])
@pytest.mark.parametrize("n", NS)
def test_layered_image_coalesced(jx, kind, n):
    stream, src, ex = layered(kind, n)
    make = lambda e: layered(kind, n, relabel=e)[0]
    for ctype in ("u8", "u16", "f32"):
        (fr,) = abi_decode(jx, stream, n if ctype == "u8" else 0, ctype)
        assert_colour(fr["px"], stream, ctype)
        if ctype == "u8":
            assert fr["size"] == (W, H)
            assert_planes(fr["planes"], make, n)
            # outside the crop no blending touched the first frame's samples
            for e in range(n):
                g = fr["planes"][e].reshape(H, W)
                want = _as_float(src[0][e], ex[e])
                assert np.array_equal(g[H - 40:, :X0], want[H - 40:, :X0]), e


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["vardct", "modular"])
@pytest.mark.parametrize("n", NS)
def test_layered_image_non_coalesced(jx, kind, n):
    stream, src, ex = layered(kind, n)
    frames = abi_decode(jx, stream, n, "u8", coalescing=False)
    assert [f["size"] for f in frames] == [(W, H), (FW, FH)]
    assert frames[1]["infos"] == [(e.blend_mode, e.blend_source, e.blend_alpha if e.blend_mode in (2, 3) else 0, e.blend_clamp if e.blend_mode >= 2 else 0) for e in ex]
    assert frames[0]["infos"] == [(0, 0, 0, 0)] * n
    for f, fr in enumerate(frames):
        alone = layered(kind, n, only=f)[0]
        assert_colour(fr["px"], alone, "u8")
        ex_f = _extras(n, blend=False)[0]
        for e in range(n):                        # frames as coded: lossless samples, the planes handed to the synthesiser
            assert np.array_equal(fr["planes"][e].reshape(fr["size"][1], fr["size"][0]), _as_float(src[f][e], ex_f[e])), (f, e)


PATCHED_NS = [1, 2, 4, 6]
PATCH_REF, PATCH_RECT, PATCH_AT = (64, 48), (2, 2, 40, 35), ((5, 5), (259, 10), (120, 160), (130, 165))      # reference frame; the patch in it (x0, y0, xsize, ysize); its placements


@functools.lru_cache(maxsize=None)
def patched(relabel, premul=False, n=6):
    ex, a = _extras(n, relabel, blend=False, premul_at=min(5, n - 1) if premul else None)
    ref_img, main = S.synthetic_image(41, *PATCH_REF), S.synthetic_image(42, W, H)
    hdr = dict(frame_type=2, is_last=0, save_before_ct=1, have_crop=1, canvas_w=W, canvas_h=H, save_as_reference=1)
    ref = X.encode_vardct_ec(ref_img, _planes(n, *PATCH_REF, 300, ex), ex, S.frame(**hdr), color_alpha=a, seed=3)
    # per placement: colour + six channels; modes 1 - 7 all occur, alpha-reading modes refer to channel 5 (also from channel 5 itself).  With n < 6 channels: the colour,
    # the first n - 1 channels and, as channel a = n - 1, the referred alpha's own entry; the alpha-reading modes refer to a.  The last two placements overlap, and in
    # every placement some channel reads the alpha that the same patch rewrites.
    blends = [[(4, 5, 0), (1, 0, 0), (2, 0, 0), (3, 0, 1), (4, 5, 0), (5, 5, 1), (4, 5, 0)],
              [(5, 5, 1), (6, 5, 0), (7, 5, 1), (0, 0, 0), (1, 0, 0), (2, 0, 0), (5, 5, 0)],
              [(6, 5, 0), (3, 0, 0), (4, 5, 1), (6, 5, 1), (7, 5, 0), (1, 0, 0), (6, 5, 0)],
              [(7, 5, 1), (2, 0, 0), (5, 5, 0), (4, 5, 0), (3, 0, 1), (7, 5, 0), (7, 5, 1)]]
    pos = [(x, y, [(m, a if m >= 4 else 0, c) for m, _, c in modes[:n] + modes[6:]]) for (x, y), modes in zip(PATCH_AT, blends)]
    S.set_features(patches=[(1, *PATCH_RECT, pos)], num_extra=n)
    try:
        return ref + X.encode_vardct_ec(main, _planes(n, W, H, 400, ex), ex, S.frame(emit=1), color_alpha=a, seed=4)
    finally:
        S.set_features()


@pytest.mark.gpu
@pytest.mark.parametrize("premul,n", [pytest.param(pm, n, id=str(pm) + ("" if n == 6 else "-%d" % n)) for n in reversed(PATCHED_NS) for pm in (False, True)])
def test_patches_with_per_channel_modes(jx, premul, n):
    """premul: the alpha the patch blendings refer to (channel min(5, n - 1)) is premultiplied — the other branch of modes 4 / 5"""
    stream = patched(None, premul, n)
    (fr,) = abi_decode(jx, stream, n, "u8")
    assert_colour(fr["px"], stream, "u8")
    assert_planes(fr["planes"], lambda e: patched(e, premul, n), n)
    (fr,) = abi_decode(jx, stream, 0, "f32")
    assert_colour(fr["px"], stream, "f32")


@pytest.mark.gpu
def test_layered_image_blending_against_a_premultiplied_alpha(jx):
    """the alpha at index 5 that colour and extras blend against is premultiplied (mode blend without the division), six channels"""
    stream, src, ex = layered("vardct", 6, premul=True)
    assert ex[5].premultiplied == 1 and ex[5].type == X.ALPHA
    for ctype in ("u8", "f32"):
        (fr,) = abi_decode(jx, stream, 6 if ctype == "u8" else 0, ctype)
        assert_colour(fr["px"], stream, ctype)
        if ctype == "u8":
            assert_planes(fr["planes"], lambda e: layered("vardct", 6, relabel=e, premul=True)[0], 6)


@pytest.mark.gpu
def test_animation_decoded_once_every_canvas(jx):
    n, kind = 6, "modular"
    S.set_animation(10, 1, 0)
    try:
        layered.cache_clear()
        stream = layered(kind, n, frames=3)[0]
        frames = abi_decode(jx, stream, n, "u8")
        assert len(frames) == 3
        for f, fr in enumerate(frames):
            cut = layered(kind, n, frames=3, upto=f)[0]
            assert_colour(fr["px"], cut, "u8")
            assert_planes(fr["planes"], lambda e: layered(kind, n, relabel=e, frames=3, upto=f)[0], n)
        frames = abi_decode(jx, stream, 0, "u8")         # no plane buffers: the kept canvases of one decode (SetOutputAllFrames)
        for f, fr in enumerate(frames):
            assert_colour(fr["px"], layered(kind, n, frames=3, upto=f)[0], "u8")
    finally:
        S.set_animation()
        layered.cache_clear()


@functools.lru_cache(maxsize=None)
def premultiplied_image():
    ex, a = _extras(6, second_alpha=False, alpha_at=2, premul_at=2, blend=False)
    pl = _planes(6, W, H, 500, ex)
    return X.encode_modular_ec(S.synthetic_image(51, W, H).astype(np.int32), pl, ex, S.frame(), color_alpha=a), pl, ex


@pytest.mark.gpu
def test_premultiplied_alpha_unpremultiplied_output(jx):
    n = 6
    stream, pl, ex = premultiplied_image()
    for ctype in ("u8", "f32"):
        (fr,) = abi_decode(jx, stream, n if ctype == "u8" else 0, ctype, nch=4, unpremul=True)
        assert_colour(fr["px"], stream, ctype, nch=4, unpremul=True)
    (fr,) = abi_decode(jx, stream, n, "u8", nch=4, unpremul=True)
    for e in range(n):
        assert np.array_equal(fr["planes"][e].reshape(H, W), _as_float(pl[e], ex[e])), e


def _spots(n):
    """two plates: at 1 and 4 among six channels, at 1 and 2 among four (the referred alpha is channel n - 1 of those)"""
    return ((1, (1.0, 0.25, 0.0, 0.75)), (4 if n == 6 else 2, (0.0, 0.5, 1.0, 0.5)))


@functools.lru_cache(maxsize=None)
def spot_single(relabel, n=6):
    ex, a = _extras(n, relabel, spots=_spots(n), blend=False)
    return X.encode_vardct_ec(S.synthetic_image(61, W, H), _planes(n, W, H, 600, ex), ex, S.frame(), color_alpha=a, seed=6)


@functools.lru_cache(maxsize=None)
def spot_layered(relabel, n=6):
    ex0, a = _extras(n, relabel, spots=_spots(n), blend=False)
    ex1, _ = _extras(n, relabel, spots=_spots(n), blend=True)
    f0 = X.encode_vardct_ec(S.synthetic_image(62, W, H), _planes(n, W, H, 700, ex0), ex0, S.frame(is_last=0, save_as_reference=1), color_alpha=a, seed=7)
    f1 = X.encode_vardct_ec(S.synthetic_image(63, FW, FH), _planes(n, FW, FH, 800, ex1), ex1,
                            S.frame(emit=1, have_crop=1, crop_x0=X0, crop_y0=Y0, canvas_w=W, canvas_h=H, blend_mode=X.BLEND, blend_source=1), color_alpha=a, seed=8)
    return f0 + f1


@pytest.mark.gpu
@pytest.mark.parametrize("render,make,n", [pytest.param(r, m, n, id="%s-%s" % (r, m.__name__) + ("" if n == 6 else "-%d" % n))
                                           for n in (6, 4) for m in (spot_single, spot_layered) for r in (True, False)])
def test_two_spot_plates_in_header_order(jx, make, render, n):
    stream = make(None, n)
    O.set_render_spotcolors(render)
    try:
        for ctype in ("u8", "f32"):
            (fr,) = abi_decode(jx, stream, n if ctype == "u8" else 0, ctype, spot=render)
            assert_colour(fr["px"], stream, ctype)
            if ctype == "u8":
                assert_planes(fr["planes"], lambda e: make(e, n), n)
    finally:
        O.set_render_spotcolors(True)


@functools.lru_cache(maxsize=None)
def float_stream(relabel, n=5):
    ex, a = _extras(n, relabel, f16_at=2, blend=False)
    pl = _planes(n, W, H, 900, ex)
    return X.encode_modular_ec(S.synthetic_image(71, W, H).astype(np.int32), pl, ex, S.frame(), color_alpha=a), pl, ex


@pytest.mark.gpu
def test_float16_extra_channel(jx):
    for n in (5, 4):
        stream, pl, ex = float_stream(None, n)
        (fr,) = abi_decode(jx, stream, n, "u8")
        assert_colour(fr["px"], stream, "u8")
        assert_planes(fr["planes"], lambda e: float_stream(e, n)[0], n)
        for e in range(n):
            assert np.array_equal(fr["planes"][e].reshape(H, W), _as_float(pl[e], ex[e])), (n, e)


@functools.lru_cache(maxsize=None)
def upsampled(relabel, n=5):
    ex, a = _extras(n, relabel, blend=False)
    pl = _planes(n, W // 2, H // 2, 1000, ex)
    pl[1] = np.full_like(pl[1], 77)                  # a flat plane: the one kind of source plane that upsampling hands back unchanged (see the test)
    return X.encode_modular_ec(S.synthetic_image(81, W // 2, H // 2).astype(np.int32), pl, ex, S.frame(), color_alpha=a, upsampling=2), pl, ex


@pytest.mark.gpu
def test_upsampled_modular_frame(jx):
    for n, ctype in ((5, "u8"), (5, "f32"), (2, "u8"), (2, "f32")):
        stream, pl, ex = upsampled(None, n)
        (fr,) = abi_decode(jx, stream, n if ctype == "u8" else 0, ctype)
        assert_colour(fr["px"], stream, ctype)
        if ctype == "u8":
            assert fr["size"] == (W, H)
            assert_planes(fr["planes"], lambda e: upsampled(e, n)[0], n)
            # Source planes: an upsampled sample is a weighted sum of 25 coded samples clamped to their range, so it equals no source sample in general and the
            # planes cannot be pinned against the source the way the unscaled lossless cases are.  A flat plane can: the clamp to [min, max] = [v, v] gives v back.
            assert np.array_equal(fr["planes"][1].reshape(H, W), np.full((H, W), _as_float(pl[1], ex[1])[0, 0], np.float32))


@functools.lru_cache(maxsize=None)
def xyb_modular(relabel):
    ex, a = _extras(5, relabel, blend=False)
    img = S.synthetic_image(91, W, H).astype(np.int32)
    return X.encode_modular_ec(img, _planes(5, W, H, 1100, ex), ex, S.frame(xyb_image=1), color_alpha=a)


@pytest.mark.gpu
def test_xyb_modular_frame(jx):
    stream = xyb_modular(None)
    for ctype in ("u8", "f32"):
        (fr,) = abi_decode(jx, stream, 5 if ctype == "u8" else 0, ctype)
        assert_colour(fr["px"], stream, ctype)
        if ctype == "u8":
            assert_planes(fr["planes"], xyb_modular, 5)


@functools.lru_cache(maxsize=None)
def lf_frame_image(relabel):
    ex, a = _extras(5, relabel, blend=False)
    img = S.synthetic_image(95, W, H)
    lw, lh = (W + 7) // 8, (H + 7) // 8
    small = np.ascontiguousarray(np.pad(img, ((0, lh * 8 - H), (0, lw * 8 - W), (0, 0)), mode="edge").reshape(lh, 8, lw, 8, 3).mean(axis=(1, 3)).astype(np.uint8))
    zero = [np.zeros((lh, lw), np.int32)] * 5
    lf = X.encode_vardct_ec(small, zero, ex, S.frame(frame_type=1, lf_level=1, is_last=0, canvas_w=W, canvas_h=H), color_alpha=a, seed=9)
    return lf + X.encode_vardct_ec(img, _planes(5, W, H, 1200, ex), ex, S.frame(emit=1, use_lf_frame=1), color_alpha=a, seed=10)


@functools.lru_cache(maxsize=None)
def preview_image(relabel):
    ex, a = _extras(5, relabel, blend=False)
    S.set_preview(40, 30)
    try:
        head = X.encode_vardct_ec(S.synthetic_image(96, W, H), _planes(5, W, H, 1300, ex), ex, S.frame(emit=2), color_alpha=a, seed=11)
        prev = X.encode_vardct_ec(S.synthetic_image(97, 40, 30), _planes(5, 40, 30, 1400, ex), ex, S.frame(emit=1), color_alpha=a, seed=12)
        main = X.encode_vardct_ec(S.synthetic_image(96, W, H), _planes(5, W, H, 1300, ex), ex, S.frame(emit=1), color_alpha=a, seed=11)
    finally:
        S.set_preview()
    alone = X.encode_vardct_ec(S.synthetic_image(97, 40, 30), _planes(5, 40, 30, 1400, ex), ex, S.frame(), color_alpha=a, seed=12)
    return head + prev + main, alone


@pytest.mark.gpu
def test_lf_frame_image_and_preview(jx):
    stream = lf_frame_image(None)
    (fr,) = abi_decode(jx, stream, 5, "u8")
    assert_colour(fr["px"], stream, "u8")
    assert_planes(fr["planes"], lf_frame_image, 5)
    stream, alone = preview_image(None)
    (pv,) = abi_decode(jx, stream, 5, "u8", preview=True)
    assert np.array_equal(pv["px"], O.decode(alone).pixels("u8", 3))
    (fr,) = abi_decode(jx, stream, 5, "u8")
    assert_colour(fr["px"], stream, "u8")
    assert_planes(fr["planes"], lambda e: preview_image(e)[0], 5)


@pytest.mark.gpu
def test_pipeline_job_mixing_many_channel_and_plain_images(jx):
    from conftest import fixture_bytes
    many = layered("vardct", 6)[0]
    plain = S.encode_vardct(S.synthetic_image(12, 200, 136), seed=2, alpha=(np.arange(200 * 136) % 256).astype(np.uint8).reshape(136, 200))
    datas = [many, plain, fixture_bytes("sample.jxl")]
    refs = [O.decode(d).pixels("u8", 3) for d in datas]
    p = jx.Pipeline(0, jobs_in_flight=2, lf_streams=2, prepare_threads=1, parse_threads=2, reserve_frames=4, reserve_width=1024, reserve_height=640)
    outs = [jx.PinnedBuffer(r.size) for r in refs]
    t = p.submit(datas, "uint8", 3, host_ptrs=[o.ptr for o in outs], capacities=[r.size for r in refs])
    status, _ = p.wait(t)
    assert status == [0, 0, 0]
    for o, r in zip(outs, refs):
        assert np.array_equal(np.array(o.array), r)
    p.close()


@pytest.mark.gpu
def test_damaged_streams_end_cleanly_and_the_decoder_goes_on(jx):
    stream, _, _ = layered("modular", 5)
    first = len(layered("modular", 5, frames=1, upto=0)[0])
    want = W * H * 3
    for bad in _damaged(stream, first + 12, len(stream) - 4, 6, 5) + [stream[:first + 40], stream[:len(stream) - 9]]:
        try:
            frames = abi_decode(jx, bad, 5, "u8")
        except (jx.DecodeError, AssertionError):
            continue
        assert all(f["px"].size == want and all(p.size == W * H for p in f["planes"]) for f in frames)
    (fr,) = abi_decode(jx, stream, 5, "u8")
    assert_colour(fr["px"], stream, "u8")
