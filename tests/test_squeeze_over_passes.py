"""VarDCT frames whose squeezed extra channel is spread over several passes: a progressive frame with downsampling entries (pass_ds) puts the alpha
sub-channels of shift 2, 1 and 0 into the PassGroup sections of passes 0, 1 and 2 (passes.h GetDownsamplingBracket), behind each pass's AC tokens.
The synthesiser writes them there, the oracle decodes them, the host plans one Modular unit per (pass, group), and on the GPU the SIMT HF kernel
records where each pass's coefficients end so that ModularGroupFastKernel can read that pass's sub-stream."""
import ctypes as C
import hashlib
import threading

import numpy as np
import pytest

import oracle_lib as O
import synth_lib as S

# (name, size, num_passes, LF tree shape): one group (everything in GlobalModular), several groups (PassGroup tails of every shift), wider than an
# LF group (shift >= 3 sub-channels in the LfGroup sections too), and the weighted-predictor LF tree of a default-effort cjxl encode
CASES = [("one_group_p2", (200, 136), 2, 0), ("one_group_p3", (200, 136), 3, 0), ("groups_p2", (700, 560), 2, 0), ("groups_p3", (700, 560), 3, 0),
         ("lf_groups_p2", (2300, 400), 2, 0), ("lf_groups_p3", (2300, 400), 3, 0), ("cjxl_shaped_lf_p3", (700, 560), 3, 1)]


def _alpha(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((np.sin(xx / 23.0) * np.cos(yy / 13.0) * 0.5 + 0.5) * 255).astype(np.uint8)


def _encode(img, al, squeeze, shape=0, **kw):
    S.set_lf_tree_shape(shape)
    S.set_alpha_squeeze(squeeze)
    try:
        return S.encode_vardct(img, seed=4, strategy_mix=2, epf_iters=1, gab=1, alpha=al, **kw)
    finally:
        S.set_alpha_squeeze(False)
        S.set_lf_tree_shape(0)


_streams = {}


def streams():
    """name -> (squeezed over the passes, plain alpha with the same passes, squeezed one-pass twin, alpha plane)"""
    if not _streams:
        for name, (w, h), npasses, shape in CASES:
            img, al = S.synthetic_image(31, w, h), _alpha(w, h)
            sq = _encode(img, al, True, shape, num_passes=npasses, pass_ds=1)
            plain = _encode(img, al, False, shape, num_passes=npasses, pass_ds=1)
            one = _encode(img, al, True, shape)
            _streams[name] = (sq, plain, one, al)
    return _streams


def _describe(jx, data):
    L = jx.libjxl()
    L.JxlHipDebugDescribe.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 16)
    if L.JxlHipDebugDescribe(data, len(data), buf, len(buf)):
        raise jx.GenericError(jx.last_error())
    return buf.value.decode()


# ---- CPU --------------------------------------------------------------------------------------------------------------------------------

# sha256 of streams the synthesiser wrote before it learnt to spread squeezed channels over passes: every parameter set that worked then
# must still give the same bytes (test_synth_roundtrip.squeezed_alpha_streams, and progressive frames with pass_ds without squeeze)
OLD_STREAMS = {
    "one_group": ("e8e0fc6b23d3b65d647861152b54d2987da002d975f001254969b9ae43524c75", "536525716d3be9fcecafc2464f5e53d7b760b2f94ec8b5839ef2ea3d515fc872"),
    "groups": ("57c82bfc6e96b8c63264afbc52b2907aef324b1abd087dd92bea3d6d16199f6c", "09b06484c422883374527273c9927da32023f7fc4998b22747663ff2e07f900d"),
    "lf_groups": ("0f9cc43c2466f1cb7e6b1861259e860b53077ea99af0e7bd72744fccfa774486", "03a239ddd7cae571f64dbdb82a628177dabffadfdb9d38c0f69fea1fec0cca54"),
    "three_passes": ("2c4322504dbb93c04adfe683154d7e012aeda7c79fdebb81992a66b56a9b9210", "76caff674e67156906f8630c12224d7b7e1a819eb1e218373ddaf0788691e363"),
    "cjxl_shaped_lf": ("efcd6449cbbf917aa127750a3f68245466b54982e6a56d15c957a76687f220c9", "6e55dd9f21306c81747f49166563c7294360e53e0a9247a7bf37c6d0fe034c88"),
    "cjxl_shaped_lf_groups": ("d28687f75777b7767cce1085c9e91a31a8b75bad0707c4bab207a616e0efeb37", "3b4ed2aaf666fcb7f84e43745ffea95afe268af8c004cf7ccc292b0f0d06be41"),
}
OLD_PASS_DS = {
    (3, False): "54dd2792248ad438610159e063e621d81a9ca8f9637dec9ffc0d3c46aa6e2554",
    (3, True): "243c18d3dbec308069efb65ad160b0ab9b365667ecb5320724a459e54c30e664",
    (2, True): "ea24cddbfd519af4d9983e66aa38d5ee325081d0b8b3366ce7b2c58848bbf31a",
}


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def test_synthesiser_output_of_earlier_parameter_sets_is_unchanged():
    from test_synth_roundtrip import squeezed_alpha_streams
    got = {name: (_sha(sq), _sha(plain)) for name, sq, plain, _ in squeezed_alpha_streams()}
    assert got == OLD_STREAMS
    img, al = S.synthetic_image(31, 700, 560), _alpha(700, 560)
    for (npasses, with_alpha), want in OLD_PASS_DS.items():
        d = S.encode_vardct(img, seed=4, strategy_mix=2, epf_iters=1, gab=1, num_passes=npasses, pass_ds=1, alpha=al if with_alpha else None)
        assert _sha(d) == want, (npasses, with_alpha)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_oracle_decodes_squeeze_over_passes(name):
    """lossless Squeeze: the alpha comes back exactly; the colour channels do not notice where the alpha sub-streams ride"""
    sq, plain, one, al = streams()[name]
    assert sq != one
    a, b = O.decode(sq).image("u8", 4), O.decode(plain).image("u8", 4)
    assert np.array_equal(a[..., 3], al), name
    assert np.array_equal(a, b), name


@pytest.fixture(scope="module")
def jx_host(built):
    import jpegxl_rs_amd as jx
    return jx


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_host_accepts_squeeze_over_passes(jx_host, name):
    sq, _, _, _ = streams()[name]
    npasses = dict((c[0], c[2]) for c in CASES)[name]
    d = _describe(jx_host, sq)
    assert f"passes={npasses}" in d and "vardct" in d, d


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def jx(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import jpegxl_rs_amd as jx
    return jx


def _check_against_oracle(jx, data, dtype, nch):
    meta, px = jx.decoder_builder(pixel_format=jx.PixelFormat(num_channels=nch)).decode_with(data, dtype)
    kind = {"uint8": "u8", "uint16": "u16", "float32": "f32"}[np.dtype(dtype).name]
    ref = O.decode(data).pixels(kind, nch).view(np.dtype("<" + np.dtype(dtype).str[1:])).astype(dtype)
    assert px.shape == ref.shape
    if np.dtype(dtype) == np.float32:
        a = px.view(np.int32).astype(np.int64); b = ref.view(np.int32).astype(np.int64)
        a = np.where(a < 0, -(a & 0x7FFFFFFF), a); b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
        assert np.abs(a - b).max() <= 1
    else:
        assert np.array_equal(px, ref), f"{int((px != ref).sum())} of {px.size} samples differ"
    return meta, px


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_gpu_matches_oracle(jx, name):
    sq, _, _, al = streams()[name]
    h, w = al.shape
    meta, px = _check_against_oracle(jx, sq, np.uint8, 4)
    assert meta.has_alpha_channel
    assert np.array_equal(px.reshape(h, w, 4)[..., 3], al), name
    _check_against_oracle(jx, sq, np.uint16, 4)
    _check_against_oracle(jx, sq, np.float32, 4)
    _check_against_oracle(jx, sq, np.uint8, 3)


@pytest.mark.gpu
def test_alpha_through_the_extra_channel_buffer(jx):
    L = jx.libjxl()
    sq, _, _, al = streams()["groups_p3"]
    h, w = al.shape
    data = np.frombuffer(sq, np.uint8)
    fmt = jx.JxlPixelFormat(3, jx.JXL_TYPE_UINT8, jx.JXL_NATIVE_ENDIAN, 0)
    efmt = jx.JxlPixelFormat(1, jx.JXL_TYPE_UINT8, jx.JXL_NATIVE_ENDIAN, 0)
    dec = L.JxlDecoderCreate(None)
    try:
        assert L.JxlDecoderSubscribeEvents(dec, jx.JXL_DEC_FULL_IMAGE) == 0
        assert L.JxlDecoderSetInput(dec, data.ctypes.data, len(data)) == 0
        L.JxlDecoderCloseInput(dec)
        px, plane = np.zeros(w * h * 3, np.uint8), np.zeros(w * h, np.uint8)
        while True:
            st = L.JxlDecoderProcessInput(dec)
            if st == jx.JXL_DEC_NEED_IMAGE_OUT_BUFFER:
                assert L.JxlDecoderSetImageOutBuffer(dec, C.byref(fmt), px.ctypes.data, px.size) == 0
                assert L.JxlDecoderSetExtraChannelBuffer(dec, C.byref(efmt), plane.ctypes.data, plane.size, 0) == 0, jx.last_error()
            elif st == jx.JXL_DEC_SUCCESS:
                break
            elif st not in (jx.JXL_DEC_FULL_IMAGE, jx.JXL_DEC_BASIC_INFO, jx.JXL_DEC_FRAME):
                raise AssertionError((st, jx.last_error()))
    finally:
        L.JxlDecoderDestroy(dec)
    assert np.array_equal(plane.reshape(h, w), al)
    assert np.array_equal(px, O.decode(sq).pixels("u8", 3))


@pytest.mark.gpu
def test_batch_beside_one_pass_twins_and_plain_frames(jx):
    """one batch: frames with the alpha squeezed over the passes, their one-pass twins and the same passes with plain alpha, decoded twice"""
    data = streams()
    batch = []
    for name in ("one_group_p3", "groups_p2", "groups_p3", "lf_groups_p3", "cjxl_shaped_lf_p3"):
        sq, plain, one, al = data[name]
        batch += [(name, sq, al), (name + "/one_pass", one, al), (name + "/plain", plain, al)]
    refs = [O.decode(s).pixels("u8", 4) for _, s, _ in batch]
    b = jx.BatchDecoder(0)
    for _, s, _ in batch:
        b.add(s, "uint8", 4)
    b.prepare()
    for _ in range(2):
        b.decode()
        b.finish()
        for i, (name, s, al) in enumerate(batch):
            px = np.asarray(b.output(i))
            assert np.array_equal(px, refs[i]), name
            assert np.array_equal(px.reshape(al.shape + (4,))[..., 3], al), name
    hf = b.info_value("hf_variant")
    assert hf & (4 | 8) and not hf & 2, hf          # the multi-pass SIMT HF kernel (kHfVarSimtAllLds / kHfVarSimtGlobal), not the one-pass form


@pytest.mark.gpu
def test_concurrent_callers(jx):
    """several threads decoding at once: their one-shot decodes go through the scheduler's shared jobs"""
    data = streams()
    names = ["groups_p2", "groups_p3", "lf_groups_p2", "cjxl_shaped_lf_p3"]
    refs = {n: O.decode(data[n][0]).pixels("u8", 4) for n in names}
    errors = []

    def work(k):
        try:
            dec = jx.decoder_builder(pixel_format=jx.PixelFormat(num_channels=4))
            for r in range(3):
                n = names[(k + r) % len(names)]
                _, px = dec.decode_with(data[n][0], np.uint8)
                assert np.array_equal(px, refs[n]), n
        except Exception as e:  # noqa: BLE001 (reported from the main thread)
            errors.append(repr(e))
    threads = [threading.Thread(target=work, args=(k,)) for k in range(6)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
