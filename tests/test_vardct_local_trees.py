"""VarDCT frames whose Modular sub-streams bring MA trees and entropy codes of their own (GroupHeader.use_global_tree = 0), with or without a global
tree.  The synthesiser (jxlsynth_set_vardct_local_trees) writes the same quantised data as its mode-0 twin, only the entropy coding of the sub-streams
changes: mode 1 local LF coefficient and HF metadata streams, mode 2 no global tree at all, mode 3 a global tree that no sub-stream uses.  The host
parses every LfGroup sub-stream's tree and code with the frame (host_parse.cc ParseLfLocalStreams) and LfDecodeLocalKernel decodes them.  Extra
channels behind the AC coefficients of the PassGroup sections under local trees are not taken: those frames fail cleanly."""
import ctypes as C
import hashlib
import threading

import numpy as np
import pytest

import oracle_lib as O
import synth_lib as S

# (name, size, alpha: None / "plain" / "squeezed", num_passes, LF tree shape)
CASES = [("one_group", (200, 136), None, 1, 0), ("groups", (700, 560), None, 1, 0), ("lf_groups", (2300, 400), None, 1, 0),
         ("alpha", (700, 560), "plain", 1, 0), ("one_group_sq_alpha", (200, 136), "squeezed", 1, 0), ("sq_alpha_p3", (700, 560), "squeezed", 3, 0),
         ("lf_groups_sq_alpha", (2300, 400), "squeezed", 1, 0), ("cjxl_shaped_lf", (700, 560), None, 1, 1)]
MODES = (1, 2, 3)
SPEC = {c[0]: c for c in CASES}


def _alpha(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((np.sin(xx / 23.0) * np.cos(yy / 13.0) * 0.5 + 0.5) * 255).astype(np.uint8)


def _encode(name, mode):
    _, (w, h), alpha, npasses, shape = SPEC[name]
    img = S.synthetic_image(31, w, h)
    kw = dict(num_passes=npasses, pass_ds=1) if npasses > 1 else {}
    L = S.lib()
    L.jxlsynth_set_vardct_local_trees.argtypes = [C.c_int]
    S.set_lf_tree_shape(shape)
    S.set_alpha_squeeze(alpha == "squeezed")
    L.jxlsynth_set_vardct_local_trees(mode)
    try:
        return S.encode_vardct(img, seed=4, strategy_mix=2, epf_iters=1, gab=1, alpha=_alpha(w, h) if alpha else None, **kw)
    finally:
        L.jxlsynth_set_vardct_local_trees(0)
        S.set_alpha_squeeze(False)
        S.set_lf_tree_shape(0)


_streams = {}


def stream(name, mode):
    if (name, mode) not in _streams:
        _streams[(name, mode)] = _encode(name, mode)
    return _streams[(name, mode)]


def _multi_group(name):
    w, h = SPEC[name][1]
    return w > 256 or h > 256


def supported(name, mode):
    """refused: extra channels in the PassGroup sections under local trees (modes 2 and 3 with alpha wider than a group), and local LF trees behind a
    global Modular stream that uses the global tree in a one-section frame (mode 1 with alpha in one group)"""
    if SPEC[name][2] and _multi_group(name) and mode >= 2:
        return False
    return not (SPEC[name][2] and not _multi_group(name) and mode == 1)


def _lf_groups(name):
    w, h = SPEC[name][1]
    return ((w + 2047) // 2048) * ((h + 2047) // 2048)


def expected_local_streams(name, mode):
    """LF coefficients + HF metadata of every LF group; modes 2/3 also the global stream of a frame with alpha"""
    return 2 * _lf_groups(name) + (1 if mode >= 2 and SPEC[name][2] else 0)


def _describe(jx, data):
    L = jx.libjxl()
    L.JxlHipDebugDescribe.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 16)
    if L.JxlHipDebugDescribe(data, len(data), buf, len(buf)):
        raise jx.GenericError(jx.last_error())
    return buf.value.decode()


def _sha(b):
    return hashlib.sha256(b).hexdigest()


# ---- CPU --------------------------------------------------------------------------------------------------------------------------------

# sha256 of streams the synthesiser wrote before it learnt local trees (700x560 unless named otherwise)
OLD_STREAMS = {
    "plain": "449b9e7e68b37e04d675ee369d0b3c0b29c8091b504dd3a7fa75e296349a37f8",
    "alpha": "09b06484c422883374527273c9927da32023f7fc4998b22747663ff2e07f900d",
    "squeezed_alpha": "57c82bfc6e96b8c63264afbc52b2907aef324b1abd087dd92bea3d6d16199f6c",
    "three_passes": "cbc9042ef8b3e68c566c874649dcc5b04f8ba3cedf8748274c71b6c2f4a5840c",
    "cjxl_shaped_lf": "ddbd00e96cb91ff64285e59d1b8f84ed837b00a89905c795cabdc18d8c641664",
    "lf_groups": "b89515b327a029d0a71549e9d0e80d668848ec7f8cc47af4a5de4bcb66e5b067",
}


def test_synthesiser_output_of_earlier_parameter_sets_is_unchanged():
    def enc(w, h, al=False, sq=False, shape=0, **kw):
        S.set_lf_tree_shape(shape)
        S.set_alpha_squeeze(sq)
        try:
            return S.encode_vardct(S.synthetic_image(31, w, h), seed=4, strategy_mix=2, epf_iters=1, gab=1, alpha=_alpha(w, h) if al else None, **kw)
        finally:
            S.set_alpha_squeeze(False)
            S.set_lf_tree_shape(0)
    got = {"plain": enc(700, 560), "alpha": enc(700, 560, True), "squeezed_alpha": enc(700, 560, True, True), "three_passes": enc(700, 560, num_passes=3),
           "cjxl_shaped_lf": enc(700, 560, shape=1), "lf_groups": enc(2300, 400)}
    assert {k: _sha(v) for k, v in got.items()} == OLD_STREAMS
    assert stream("groups", 0) == enc(700, 560)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_oracle_decodes_local_trees_like_the_twin(name, mode):
    d, twin = stream(name, mode), stream(name, 0)
    assert d != twin
    for kind in ("u8", "f32"):
        assert np.array_equal(O.decode(d).image(kind, 4), O.decode(twin).image(kind, 4)), (name, mode, kind)


@pytest.fixture(scope="module")
def jx_host(built):
    import jpegxl_rs_amd as jx
    return jx


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_host_accepts_local_trees(jx_host, name, mode):
    d = stream(name, mode)
    if not supported(name, mode):
        # (no global tree: refused by the host; otherwise the frame parses and its decode fails on the device — the GPU test below)
        with pytest.raises(jx_host.GenericError, match="unsupported: VarDCT frame without a global MA tree whose PassGroup") if mode == 2 else _no_raise():
            _describe(jx_host, d)
        return
    desc = _describe(jx_host, d)
    assert "vardct" in desc and f"local_streams={expected_local_streams(name, mode)}" in desc, desc


class _no_raise:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


@pytest.mark.parametrize("name,mode", [("one_group_sq_alpha", 2), ("groups", 1), ("lf_groups", 3), ("cjxl_shaped_lf", 2)])
def test_corrupt_local_trees_end_cleanly(jx_host, name, mode):
    """bit flips and truncations from where the stream starts to differ from its twin (the first local tree or code) on: a parse error or a parse, never a crash"""
    d, twin = stream(name, mode), stream(name, 0)
    first = next(i for i in range(min(len(d), len(twin))) if d[i] != twin[i])
    outcomes = []
    for k in range(24):
        pos = first + k * 11
        if pos >= len(d):
            break
        bad = bytearray(d)
        bad[pos] ^= 1 << (k % 8)
        for data in (bytes(bad), d[:pos]):
            try:
                _describe(jx_host, data)
                outcomes.append("ok")
            except (jx_host.GenericError, jx_host.DecodeError):
                outcomes.append("error")
    assert "error" in outcomes


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
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_gpu_matches_oracle_and_twin(jx, name, mode):
    d = stream(name, mode)
    if not supported(name, mode):
        with pytest.raises((jx.GenericError, jx.DecodeError)):
            jx.decoder_builder(pixel_format=jx.PixelFormat(num_channels=4)).decode_with(d, np.uint8)
        return
    _, px = _check_against_oracle(jx, d, np.uint8, 4)
    _, twin = jx.decoder_builder(pixel_format=jx.PixelFormat(num_channels=4)).decode_with(stream(name, 0), np.uint8)
    assert np.array_equal(px, twin), (name, mode)
    if SPEC[name][2]:
        w, h = SPEC[name][1]
        assert np.array_equal(px.reshape(h, w, 4)[..., 3], _alpha(w, h))
    _check_against_oracle(jx, d, np.uint16, 4)
    _check_against_oracle(jx, d, np.float32, 4)
    _check_against_oracle(jx, d, np.uint8, 3)
    _check_against_oracle(jx, d, np.float32, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", [("alpha", 1), ("one_group_sq_alpha", 3), ("lf_groups_sq_alpha", 1)])
def test_alpha_through_the_extra_channel_buffer(jx, name, mode):
    L = jx.libjxl()
    d = stream(name, mode)
    w, h = SPEC[name][1]
    al = _alpha(w, h)
    data = np.frombuffer(d, np.uint8)
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
    assert np.array_equal(px, O.decode(d).pixels("u8", 3))


@pytest.mark.gpu
def test_batch_beside_twins_and_ordinary_frames(jx):
    """one batch: local-tree frames of every mode beside their mode-0 twins and ordinary frames, prepared once and decoded twice"""
    batch = []
    for name in ("one_group", "groups", "lf_groups", "alpha", "one_group_sq_alpha", "cjxl_shaped_lf"):
        for mode in (0,) + MODES:
            if supported(name, mode):
                batch.append((f"{name}/{mode}", stream(name, mode)))
    batch.append(("ordinary", S.encode_vardct(S.synthetic_image(11, 320, 200), seed=3, strategy_mix=2, epf_iters=1, gab=1)))
    refs = [O.decode(s).pixels("u8", 4) for _, s in batch]
    b = jx.BatchDecoder(0)
    b.set_lane_stride(8, 1)                                # (the streaming pipeline's strides: eligible frames take the SIMT LF kernel)
    for _, s in batch:
        b.add(s, "uint8", 4)
    b.prepare()
    for _ in range(2):
        b.decode()
        b.finish()
        for i, (name, _) in enumerate(batch):
            assert np.array_equal(np.asarray(b.output(i)), refs[i]), name
    lf = b.info_value("lf_variant")
    assert lf & 64, lf                                     # LfDecodeLocalKernel (kLfVarLocal) for the local-tree frames
    assert lf & (1 | 2 | 4 | 8), lf                        # the ordinary frames and the twins still take the SIMT LF kernel


@pytest.mark.gpu
def test_concurrent_callers(jx):
    names = [("groups", 2), ("lf_groups", 1), ("alpha", 1), ("one_group_sq_alpha", 3), ("groups", 0)]
    refs = {k: O.decode(stream(*k)).pixels("u8", 4) for k in names}
    errors = []

    def work(t):
        try:
            dec = jx.decoder_builder(pixel_format=jx.PixelFormat(num_channels=4))
            for r in range(3):
                k = names[(t + r) % len(names)]
                _, px = dec.decode_with(stream(*k), np.uint8)
                assert np.array_equal(px, refs[k]), k
        except Exception as e:  # noqa: BLE001 (reported from the main thread)
            errors.append(repr(e))
    threads = [threading.Thread(target=work, args=(t,)) for t in range(6)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@pytest.mark.gpu
def test_pipeline_mixes_local_tree_frames_with_ordinary_ones(jx):
    """the pipeline decodes local-tree frames and leaves the ordinary frames of the same job bit-exact"""
    datas = [stream("groups", 0), stream("groups", 2), stream("lf_groups", 1), stream("one_group", 3), stream("lf_groups", 0)]
    refs = [O.decode(d).pixels("u8", 3) for d in datas]
    p = jx.Pipeline(0, jobs_in_flight=2, lf_streams=2, prepare_threads=1, parse_threads=2, reserve_frames=8, reserve_width=2304, reserve_height=640)
    try:
        outs = [jx.PinnedBuffer(r.size) for r in refs]
        t = p.submit(datas, "uint8", 3, host_ptrs=[o.ptr for o in outs], capacities=[r.size for r in refs])
        status, _ = p.wait(t, check=False)
        assert list(status) == [0] * len(datas), (status, jx.last_error())
        for k, (o, r) in enumerate(zip(outs, refs)):
            assert np.array_equal(np.array(o.array), r), k
    finally:
        p.close()
