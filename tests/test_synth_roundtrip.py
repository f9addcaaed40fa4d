"""CPU tests: the bit-stream synthesiser (tools/jxlsynth) against the oracle — lossless Modular round trips exactly,
VarDCT round trips within the expected quantisation error for every supported block strategy."""
import numpy as np
import pytest

import os

from conftest import GOLDEN
import oracle_lib as O
import synth_lib as S


def psnr(a, b):
    m = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return 10 * np.log10(255.0 ** 2 / max(m, 1e-12))


@pytest.mark.parametrize("h,w,c,bits,rct", [(50, 40, 3, 8, False), (1, 1, 3, 8, False), (7, 300, 1, 8, False), (300, 520, 4, 8, True),
                                            (64, 64, 1, 16, False), (257, 255, 3, 16, True), (256, 256, 3, 8, True), (513, 10, 2, 8, False)])
def test_modular_lossless_roundtrip(h, w, c, bits, rct):
    base = S.synthetic_image(3, max(w, 8), max(h, 8)).astype(np.int32)[:h, :w]
    img = np.stack([base[..., i % 3] * ((1 << bits) - 1) // 255 for i in range(c)], -1)
    dec = O.decode(S.encode_modular(img, bits, rct))
    assert (dec.info.xsize, dec.info.ysize, dec.info.bits_per_sample) == (w, h, bits)
    out = dec.image("u16" if bits == 16 else "u8", c)
    assert np.array_equal(out, img)


STRATEGIES = {0: "DCT", 1: "IDENTITY", 2: "DCT2X2", 3: "DCT4X4", 4: "DCT16X16", 5: "DCT32X32", 6: "DCT16X8", 7: "DCT8X16", 8: "DCT32X8", 9: "DCT8X32",
              10: "DCT32X16", 11: "DCT16X32", 12: "DCT4X8", 13: "DCT8X4", 18: "DCT64X64", 19: "DCT64X32", 20: "DCT32X64"}


@pytest.mark.parametrize("s", sorted(STRATEGIES))
def test_vardct_every_strategy_roundtrip(s):
    """Forced single strategy at fine quantisation: forward transform (synth) x inverse transform (oracle) must agree."""
    img = S.synthetic_image(7, 256, 128)
    data = S.encode_vardct(img, seed=5, strategy_mix=100 + s, epf_iters=0, gab=0, distance=0.1, skip_lf_smoothing=1)
    out = O.decode(data).image("u8", 3)
    assert psnr(out, img) > 41.0, STRATEGIES[s]


@pytest.mark.parametrize("w,h,mix,epf,gab", [(8, 8, 0, 0, 0), (64, 64, 0, 1, 1), (100, 37, 1, 1, 1), (256, 256, 1, 2, 1), (300, 200, 2, 3, 1), (520, 300, 2, 0, 0)])
def test_vardct_roundtrip_quality(w, h, mix, epf, gab):
    img = S.synthetic_image(11, max(w, 8), max(h, 8))[:h, :w]
    img = np.ascontiguousarray(img)
    dec = O.decode(S.encode_vardct(img, seed=2, strategy_mix=mix, epf_iters=epf, gab=gab))
    assert (dec.info.xsize, dec.info.ysize, dec.info.xyb_encoded) == (w, h, 1)
    assert psnr(dec.image("u8", 3), img) > 33.0
    assert dec.info.tokens_hf > 0 and dec.info.tokens_lf > 0


def test_synth_is_deterministic():
    img = S.synthetic_image(5, 128, 64)
    assert np.array_equal(img, S.synthetic_image(5, 128, 64))
    a = S.encode_vardct(img, seed=1, strategy_mix=2)
    assert a == S.encode_vardct(img, seed=1, strategy_mix=2)
    assert a != S.encode_vardct(img, seed=2, strategy_mix=2)


def test_hdr_float_stream_roundtrip():
    """Config-5 style stream: float32 samples, linear transfer, intensity_target 1000."""
    img = S.synthetic_image(9, 160, 96).astype(np.float32) / 255.0
    lin = (img ** 2.2) * 2.0
    data = S.encode_vardct(lin, seed=4, strategy_mix=1, epf_iters=3, gab=1, out_bits=32, hdr=1)
    dec = O.decode(data)
    assert dec.info.bits_per_sample == 32 and dec.info.exponent_bits == 8 and abs(dec.info.intensity_target - 1000.0) < 1e-3
    out = dec.image("f32", 3)
    assert np.abs(out - lin).mean() < 0.02


# ---- stream features added later in the round: synthesiser x oracle on the CPU (the GPU suite repeats them through the C ABI) --
def _smooth(seed, h, w, c, bits):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = ((np.sin(xx / 37.0) + np.cos(yy / 23.0)) * 0.25 + 0.5) * ((1 << bits) - 1)
    return np.clip(base[..., None] + rng.normal(0, (1 << bits) / 1024.0, (h, w, c)).astype(np.float32), 0, (1 << bits) - 1).astype(np.int32)


@pytest.mark.parametrize("h,w,c,bits,rct,squeeze", [(50, 40, 1, 8, 0, 1), (280, 300, 3, 8, 1, 1), (280, 300, 4, 16, 1, 2), (2070, 2100, 1, 16, 0, 1), (9, 1, 1, 8, 0, 1)])
def test_squeeze_lossless_roundtrip(h, w, c, bits, rct, squeeze):
    """Default Squeeze chain (zero explicit steps in the stream) and explicit chains: residual channels in GlobalModular,
    LfGroup (shift >= 3) and PassGroup sections; the oracle's inverse must return the source samples exactly."""
    img = _smooth(5, h, w, c, bits)
    out = O.decode(S.encode_modular(img, bits, bool(rct), squeeze)).image("u16" if bits == 16 else "u8", c)
    assert np.array_equal(out, img)


@pytest.mark.parametrize("strategy", [21, 22, 23, 24, 25, 26])
def test_dct128_256_family_roundtrip(strategy):
    img = S.synthetic_image(7, 520, 300)
    out = O.decode(S.encode_vardct(img, seed=5, strategy_mix=100 + strategy, epf_iters=0, gab=0, distance=0.1, skip_lf_smoothing=1)).image("u8", 3)
    assert psnr(out, img) > 41.0


def test_alpha_passes_permuted_toc_and_orientation_streams():
    img = S.synthetic_image(42, 600, 400)
    al = (np.add.outer(np.arange(400), np.arange(600)) % 256).astype(np.uint8)
    ref = O.decode(S.encode_vardct(img, seed=3, strategy_mix=2, alpha=al)).image("u8", 4)
    assert np.array_equal(ref[..., 3], al) and psnr(ref[..., :3], img) > 33.0
    for kw in ({"num_passes": 2}, {"num_passes": 3}, {"permute_toc": 7}, {"num_passes": 2, "permute_toc": 9}):
        out = O.decode(S.encode_vardct(img, seed=3, strategy_mix=2, alpha=al, **kw)).image("u8", 4)
        assert np.array_equal(out, ref), kw          # bit planes / section order do not change the decoded picture
    d = O.decode(S.encode_vardct(img, seed=3, strategy_mix=2, orientation=6))
    assert d.info.orientation == 6 and (d.info.xsize, d.info.ysize) == (600, 400)    # the oracle reports the stored raster


def test_set_orientation_reaches_streams_without_an_argument_of_their_own():
    """S.set_orientation: the image header of a Modular stream (plain and frame-controlled) carries the orientation; the samples are the stored raster, untouched"""
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (37, 53, 4)).astype(np.int32)
    plain = S.encode_modular(img, 8, False, 0)
    for o in (1, 5, 8):
        S.set_orientation(o)
        try:
            streams = [S.encode_modular(img, 8, False, 0), S.encode_modular_frame(img, S.frame(), bits=8)]
            vardct = S.encode_vardct(S.synthetic_image(3, 64, 40), seed=3, orientation=3)
        finally:
            S.set_orientation()
        for data in streams:
            d = O.decode(data)
            assert d.info.orientation == o and (d.info.xsize, d.info.ysize) == (53, 37)
            assert np.array_equal(d.image("u8", 4), img)
        assert O.decode(vardct).info.orientation == 3                                # encode_vardct's own argument wins
    assert S.encode_modular(img, 8, False, 0) == plain and O.decode(plain).info.orientation == 1      # and the setting is gone afterwards


@pytest.mark.parametrize("up,custom,floor", [(2, 0, 33.0), (2, 1, 33.0), (4, 1, 28.0), (8, 1, 23.0)])
def test_upsampled_streams_roundtrip(up, custom, floor):
    img = S.synthetic_image(62, 333, 201)
    d = O.decode(S.encode_vardct(img, seed=4, strategy_mix=2, upsampling=up, custom_up_weights=custom))
    assert (d.info.xsize, d.info.ysize) == (333, 201)
    assert psnr(d.image("u8", 3), img) > floor


def test_default_4x_8x_upsampling_weights_decode():
    """Streams that rely on the library-default 4x / 8x kernels (round 1 rejected them; the tables are now restated and
    checked as partitions of unity in test_oracle_goldens.py)."""
    img = S.synthetic_image(3, 96, 64)
    for up, floor in ((4, 24.0), (8, 19.0)):
        d = O.decode(S.encode_vardct(img, upsampling=up, custom_up_weights=0))
        assert (d.info.xsize, d.info.ysize) == (96, 64)
        assert psnr(d.image("u8", 3), img) > floor

# ---- multi-frame images, blending, crops, noise (round 2) ------------------------------------------------------------------------
def _layers():
    img = S.synthetic_image(5, 200, 136)
    small = S.synthetic_image(9, 64, 48)
    return img, small


@pytest.mark.parametrize("mode", [0, 1, 4])
def test_layered_modular_frames_blend_like_the_arithmetic_says(mode):
    """frame_header.cc BlendingInfo / blending.cc: a cropped lossless layer over a saved frame — replace, add, mul."""
    img, small = _layers()
    f0 = S.encode_modular_frame(img, S.frame(is_last=0, save_as_reference=1), bits=8)
    f1 = S.encode_modular_frame(small, S.frame(emit=1, have_crop=1, crop_x0=40, crop_y0=30, canvas_w=200, canvas_h=136, blend_mode=mode, blend_source=1), bits=8)
    px = O.decode(f0 + f1).image("u8", 3).astype(float)
    exp = img.astype(float)
    roi = exp[30:78, 40:104]
    exp[30:78, 40:104] = small if mode == 0 else np.clip(roi + small, 0, 255) if mode == 1 else roi * small / 255.0
    assert np.abs(px - exp).max() <= 0.5


def modular_group_size_streams():
    """(name, stream, samples, bits): Modular frames with group_size_shift 0, 2, 3 (groups of 128, 512, 1024 samples a side; `cjxl -g`), plain and squeezed, RGB / RGBA / grey"""
    from test_gpu_parity import _smooth_image
    out = []
    for shift in (0, 2, 3):
        for (w, h, nch, bits, sq) in [(700, 560, 3, 8, 0), (1300, 1100, 4, 16, 1), (333, 300, 1, 8, 0), (2300, 400, 3, 8, 1)]:
            img = _smooth_image(7 + shift, h, w, nch, bits)
            S.set_modular_group_shift(shift)
            try:
                data = S.encode_modular(img, bits, True, sq)
            finally:
                S.set_modular_group_shift(1)
            out.append((f"shift{shift}_{w}x{h}x{nch}_{bits}b_sq{sq}", data, img, bits))
    return out


def test_modular_group_sizes():
    for name, data, img, bits in modular_group_size_streams():
        out = O.decode(data).image("u8" if bits == 8 else "u16", img.shape[2])
        assert np.array_equal(out.reshape(img.shape), img), name


def block_ctx_map_streams():
    """(name, stream with a BlockCtxMap of its own, default-map twin): thresholds on the quantised LF of X / Y / B and on the quantiser field select among 16 block contexts
    (ac_context.h BlockCtxMap; libjxl's encoder fits one per frame at default effort); the map itself travels MTF- and ANS-coded.  Also with several histogram sets,
    progressive passes, prefix codes, and under an LF frame (no quantised LF of the frame's own: LF index 0)."""
    from_lf = None
    out = []
    for name, (w, h), kw, presets, opt in [("small", (300, 280), {}, 1, None), ("groups", (700, 560), {}, 1, None), ("passes_presets", (520, 300), dict(num_passes=3), 3, None),
                                           ("lf_groups", (2300, 400), {}, 2, None), ("prefix", (700, 560), {}, 1, "prefix")]:
        img = S.synthetic_image(33, w, h)
        if opt == "prefix":
            S.set_prefix(True)
        S.set_hf_presets(presets)
        try:
            one = S.encode_vardct(img, seed=4, strategy_mix=2, epf_iters=1, gab=1, **kw)
            S.set_custom_block_ctx(True)
            many = S.encode_vardct(img, seed=4, strategy_mix=2, epf_iters=1, gab=1, **kw)
        finally:
            S.set_custom_block_ctx(False); S.set_hf_presets(1); S.set_prefix(False)
        out.append((name, many, one))
    img = S.synthetic_image(81, 300, 200)
    parts = {}
    for custom in (False, True):
        S.set_custom_block_ctx(custom)
        try:
            parts[custom] = (S.encode_vardct_frame(img, S.frame(emit=2), seed=3)
                             + S.encode_vardct_frame(_block_means(img), S.frame(emit=1, is_last=0, frame_type=1, lf_level=1), seed=5, distance=0.3, epf_iters=0, gab=0)
                             + S.encode_vardct_frame(img, S.frame(emit=1, use_lf_frame=1), seed=3, strategy_mix=2, epf_iters=1))
        finally:
            S.set_custom_block_ctx(False)
    out.append(("under_lf_frame", parts[True], parts[False]))
    return out


def test_block_context_maps():
    for name, many, one in block_ctx_map_streams():
        assert many != one, name
        assert np.array_equal(O.decode(many).image("u8", 3), O.decode(one).image("u8", 3)), name


def custom_lf_global_streams():
    """(name, stream, source image): frames with their own LfChannelDequantization (LF steps 1 / 2048, 1 / 256, 1 / 128 instead of 1 / 4096, 1 / 512, 1 / 256) and
    LfChannelCorrelation (colour factor 64, base correlations 0.125 / 0.75, LF factors +6 / -10) — libjxl's encoder writes fitted values at default effort"""
    out = []
    for name, (w, h), kw in [("small", (300, 280), {}), ("groups", (700, 560), {}), ("passes", (520, 300), dict(num_passes=3)), ("lf_groups", (2300, 400), {})]:
        img = S.synthetic_image(33, w, h)
        S.set_custom_lf_global(True)
        try:
            data = S.encode_vardct(img, seed=4, strategy_mix=2, epf_iters=1, gab=1, **kw)
        finally:
            S.set_custom_lf_global(False)
        out.append((name, data, img))
    return out


def test_custom_lf_dequantisation_and_colour_correlation():
    for name, data, img in custom_lf_global_streams():
        assert psnr(O.decode(data).image("u8", 3), img) > 37.0, name       # the decoder applies what the encoder assumed (default parameters: 40 dB; the LF steps here are twice as coarse)


def hf_preset_streams():
    """(name, stream with several histogram sets, its one-set twin): HfGlobal num_hf_presets > 1 — libjxl's encoder clusters the groups of a larger picture into several sets of AC
    histograms; every PassGroup names its set, whose contexts follow those of the sets before it.  Single pass, progressive, > 1 LF group, prefix codes, LZ77."""
    out = []
    for name, (w, h), n, kw, opt in [("two_sets", (700, 560), 2, {}, None), ("five_sets_passes", (520, 300), 5, dict(num_passes=3), None), ("three_sets_lf_groups", (2300, 400), 3, {}, None),
                                     ("prefix", (700, 560), 3, {}, "prefix"), ("lz77", (520, 300), 2, {}, "lz77")]:
        img = S.synthetic_image(33, w, h)
        if opt == "prefix":
            S.set_prefix(True)
        if opt == "lz77":
            S.set_lz77_ac(True)
        try:
            one = S.encode_vardct(img, seed=4, strategy_mix=2, epf_iters=1, gab=1, **kw)
            S.set_hf_presets(n)
            many = S.encode_vardct(img, seed=4, strategy_mix=2, epf_iters=1, gab=1, **kw)
        finally:
            S.set_hf_presets(1); S.set_prefix(False); S.set_lz77_ac(False)
        out.append((name, many, one))
    return out


def test_several_hf_histogram_sets():
    for name, many, one in hf_preset_streams():
        assert many != one, name
        assert np.array_equal(O.decode(many).image("u8", 3), O.decode(one).image("u8", 3)), name


def squeezed_alpha_streams():
    """(name, squeezed stream, its unsqueezed twin, alpha plane): the extra channel of a VarDCT frame put through the default Squeeze chain, the way cjxl
    stores a progressive or lossy alpha of an RGBA picture: one-group frame (everything in GlobalModular), several groups (PassGroup tails of every shift), a frame wider than
    an LF group (shift >= 3 sub-channels in the LfGroup sections, between the LF coefficients and the HF metadata), three passes (all of it in the last one)."""
    out = []
    for name, (w, h), shape, kw in [("one_group", (200, 136), 0, {}), ("groups", (700, 560), 0, {}), ("lf_groups", (2300, 400), 0, {}),
                                    ("three_passes", (520, 300), 0, dict(num_passes=3)), ("cjxl_shaped_lf", (700, 560), 1, {}), ("cjxl_shaped_lf_groups", (2100, 300), 1, {})]:
        img = S.synthetic_image(31, w, h)
        yy, xx = np.mgrid[0:h, 0:w]
        al = ((np.sin(xx / 23.0) * np.cos(yy / 13.0) * 0.5 + 0.5) * 255).astype(np.uint8)
        S.set_lf_tree_shape(shape)       # 1: weighted-predictor LF streams, the SIMT LF kernel's case
        try:
            plain = S.encode_vardct(img, seed=4, strategy_mix=2, epf_iters=1, gab=1, alpha=al, **kw)
            S.set_alpha_squeeze(True)
            sq = S.encode_vardct(img, seed=4, strategy_mix=2, epf_iters=1, gab=1, alpha=al, **kw)
        finally:
            S.set_alpha_squeeze(False)
            S.set_lf_tree_shape(0)
        out.append((name, sq, plain, al))
    return out


def test_squeezed_alpha_in_vardct_frames():
    for name, sq, plain, al in squeezed_alpha_streams():
        assert sq != plain, name
        a, b = O.decode(sq).image("u8", 4), O.decode(plain).image("u8", 4)
        assert np.array_equal(a[..., 3], al), name            # Squeeze is lossless
        assert np.array_equal(a, b), name                      # and the colour channels do not notice


def test_layer_partly_outside_the_canvas_and_alpha_blending():
    img, small = _layers()
    f0 = S.encode_modular_frame(img, S.frame(is_last=0, save_as_reference=1), bits=8)
    f1 = S.encode_modular_frame(small, S.frame(emit=1, have_crop=1, crop_x0=-20, crop_y0=100, canvas_w=200, canvas_h=136, blend_source=1), bits=8)
    exp = img.copy(); exp[100:136, 0:44] = small[0:36, 20:64]
    assert np.array_equal(O.decode(f0 + f1).image("u8", 3), exp)
    al = np.full((136, 200, 1), 255, np.uint8)
    f0a = S.encode_modular_frame(np.dstack([img, al]), S.frame(is_last=0, save_as_reference=2), bits=8)
    sa = np.dstack([small, (np.add.outer(np.arange(48), np.arange(64)) * 3 % 256).astype(np.uint8)])
    a = sa[..., 3:4] / 255.0
    for mode in (2, 3):
        f1a = S.encode_modular_frame(sa, S.frame(emit=1, have_crop=1, crop_x0=10, crop_y0=20, canvas_w=200, canvas_h=136, blend_mode=mode, blend_source=2), bits=8)
        px = O.decode(f0a + f1a).image("u8", 4)
        exp = img.astype(float)
        roi = exp[20:68, 10:74]
        exp[20:68, 10:74] = small * a + roi * (1 - a) if mode == 2 else np.clip(roi + small * a, 0, 255)
        assert np.abs(px[..., :3] - exp).max() <= 0.5 and px[..., 3].min() == 255


def test_vardct_layers_and_noise():
    img, small = _layers()
    base = O.decode(S.encode_vardct_frame(img, S.frame(), seed=3)).image("u8", 3)
    ov = O.decode(S.encode_vardct_frame(small, S.frame(), seed=4)).image("u8", 3)
    g0 = S.encode_vardct_frame(img, S.frame(is_last=0, save_as_reference=1), seed=3)
    g1 = S.encode_vardct_frame(small, S.frame(emit=1, have_crop=1, crop_x0=100, crop_y0=60, canvas_w=200, canvas_h=136, blend_source=1), seed=4)
    exp = base.copy(); exp[60:108, 100:164] = ov
    assert np.array_equal(O.decode(g0 + g1).image("u8", 3), exp)
    # noise: zero-mean, strength follows the LUT
    weak = O.decode(S.encode_vardct_frame(img, S.frame(noise_lut=[10] * 8), seed=3)).image("u8", 3).astype(float)
    strong = O.decode(S.encode_vardct_frame(img, S.frame(noise_lut=[120] * 8), seed=3)).image("u8", 3).astype(float)
    assert 0.2 < np.abs(weak - base).mean() < np.abs(strong - base).mean() and abs((weak - base).mean()) < 0.3


def test_free_running_streams_are_stable_under_the_oracle():
    """tools/synth_free.h streams (random MA trees, all predictors / properties, local trees, LZ77, delta palettes): the synthesiser
    is deterministic and the oracle's rendering of them is pinned by hash (tests/golden/free_streams.json, written by this same
    code path) — a change of either shows up here before the GPU parity test compares the HIP path with the oracle."""
    import hashlib
    import json
    from free_cases import FREE_CASES
    man = json.load(open(os.path.join(GOLDEN, "free_streams.json")))
    assert sorted(man) == sorted(FREE_CASES)
    for name, kw in sorted(FREE_CASES.items()):
        kw = dict(kw); kw.setdefault("bits", 16)
        data = S.encode_modular_free(**kw)
        assert hashlib.sha256(data).hexdigest() == man[name]["sha256_stream"], name
        px = O.decode(data).pixels("f32", man[name]["channels"])
        assert hashlib.sha256(px.tobytes()).hexdigest() == man[name]["sha256_f32"], name


def test_prefix_coded_streams_decode_like_their_ans_twins():
    """tools/synth_entropy.h writes prefix (Huffman) codes when asked (length-limited Huffman, Brotli-style code description, canonical codes
    most significant bit first): the oracle must decode such streams to exactly what the ANS-coded twin of the same image gives — VarDCT
    (lossy: same quantised coefficients) and Modular (lossless: the source samples)."""
    import numpy as np
    import oracle_lib as O
    import synth_lib as S
    for seed, (w, h) in enumerate([(320, 200), (64, 48), (520, 300)]):
        img = S.synthetic_image(60 + seed, w, h)
        ans = S.encode_vardct(img, seed=seed, strategy_mix=seed % 3)
        S.set_prefix(True)
        try:
            pfx = S.encode_vardct(img, seed=seed, strategy_mix=seed % 3)
            mod = S.encode_modular(img, bits=8)
        finally:
            S.set_prefix(False)
        assert pfx != ans
        assert np.array_equal(O.decode(pfx).pixels("u8", 3), O.decode(ans).pixels("u8", 3))
        assert np.array_equal(O.decode(mod).pixels("u8", 3), img.reshape(-1))


def preview_streams():
    """(name, stream with a preview frame in front, the same image without): the preview is a frame of the PreviewHeader's size — VarDCT or Modular, also of
    several groups — that a decoder without a JXL_DEC_PREVIEW_IMAGE subscriber steps over"""
    import synth_lib as S
    out = []
    main = S.synthetic_image(71, 300, 200)
    for name, pw, ph, modular in [("vardct_div8", 64, 48, False), ("modular_odd", 37, 23, True), ("vardct_multigroup", 520, 300, False)]:
        prev = S.synthetic_image(72, pw, ph)
        S.set_preview(pw, ph)
        try:
            hdr = S.encode_vardct_frame(main, S.frame(emit=2), seed=3)
        finally:
            S.set_preview(0, 0)
        pf = S.encode_modular_frame(prev, S.frame(emit=1), bits=8) if modular else S.encode_vardct_frame(prev, S.frame(emit=1), seed=5)
        body = S.encode_vardct_frame(main, S.frame(emit=1), seed=3)
        # (the Modular preview of an XYB image is an XYB Modular frame: its samples are read as Y, X, B - Y whatever they were meant to be)
        alone = S.encode_modular_frame(prev, S.frame(emit=0, xyb_image=1), bits=8) if modular else S.encode_vardct_frame(prev, S.frame(emit=0), seed=5)   # the preview as an image of its own
        out.append((name, hdr + pf + body, S.encode_vardct_frame(main, S.frame(emit=0), seed=3), (pw, ph), alone))
    return out


def test_preview_frames_are_stepped_over():
    """headers.cc PreviewHeader + the preview frame (decode.cc): the image decodes to what it decodes to without the preview"""
    import numpy as np
    import oracle_lib as O
    for name, with_preview, plain, _, _ in preview_streams():
        assert len(with_preview) > len(plain)
        assert np.array_equal(O.decode(with_preview).pixels("u8", 3), O.decode(plain).pixels("u8", 3)), name


def _block_means(img):
    """1/8-scale image: the mean of every 8x8 block (edge blocks: of what exists)"""
    import numpy as np
    h, w, c = img.shape
    bh, bw = (h + 7) // 8, (w + 7) // 8
    pad = np.pad(img.astype(np.float64), ((0, bh * 8 - h), (0, bw * 8 - w), (0, 0)), mode="edge")
    return np.clip(np.rint(pad.reshape(bh, 8, bw, 8, c).mean(axis=(1, 3))), 0, 255).astype(np.uint8)


def lf_frame_streams():
    """(name, stream, source image): images whose LF image travels as an LF frame (frame_type 1, `cjxl --progressive_dc`): a 1/8-scale VarDCT or
    Modular frame first, then the frame proper with flag use_lf_frame and no LF coefficients in its LfGroups; also two levels (1/64 -> 1/8 -> 1)."""
    import numpy as np
    import synth_lib as S
    out = []
    for name, (w, h), lf_modular, levels, mix, epf in [("vardct_lf", (300, 200), False, 1, 1, 1), ("modular_lf", (264, 136), True, 1, 2, 2),
                                                       ("two_levels", (2100, 600), False, 2, 1, 1), ("multi_lf_group", (2300, 400), False, 1, 2, 0)]:
        img = S.synthetic_image(81, w, h)
        small = _block_means(img)
        hdr = S.encode_vardct_frame(img, S.frame(emit=2), seed=3)
        parts = [hdr]
        if levels == 2:
            parts.append(S.encode_vardct_frame(_block_means(small), S.frame(emit=1, is_last=0, frame_type=1, lf_level=2), seed=7, distance=0.3, epf_iters=0, gab=0))
        fx = S.frame(emit=1, is_last=0, frame_type=1, lf_level=1, use_lf_frame=1 if levels == 2 else 0, xyb_image=1 if lf_modular else 0)
        if lf_modular:
            # XYB samples as integers (dec_modular.cc: Y, X, B - Y in units of the LF dequantisation steps): any smooth picture will do
            ints = np.stack([small[..., 1].astype(np.int32) * 2, small[..., 0].astype(np.int32) // 8 - 16, small[..., 2].astype(np.int32) // 4 - 32], axis=-1)
            parts.append(S.encode_modular_frame(ints, fx, bits=8))
        else:
            parts.append(S.encode_vardct_frame(small, fx, seed=5, distance=0.3, epf_iters=0, gab=0))
        parts.append(S.encode_vardct_frame(img, S.frame(emit=1, use_lf_frame=1), seed=3, strategy_mix=mix, epf_iters=epf))
        out.append((name, b"".join(parts), img, lf_modular))
    return out


def lf_frame_alpha_streams():
    """(name, stream, twin without the LF frame's detour, alpha): RGBA images whose LF image travels as an LF frame.  Every frame codes the image's extra channels, the LF
    frame too (`cjxl --progressive_dc` on an RGBA picture writes a zero-filled one at 1/8 scale); a decoder reads past them and takes the alpha of the frame proper."""
    import numpy as np
    import synth_lib as S
    out = []
    for name, (w, h), lf_modular, squeeze in [("vardct_lf", (300, 200), False, False), ("modular_lf", (264, 136), True, False), ("vardct_lf_squeezed_alpha", (700, 560), False, True)]:
        img = S.synthetic_image(83, w, h)
        al = (np.add.outer(np.arange(h), np.arange(w)) * 3 % 256).astype(np.uint8)
        small = _block_means(img)
        sal = (np.add.outer(np.arange(small.shape[0]), np.arange(small.shape[1])) * 7 % 256).astype(np.uint8)       # (anything: it is not looked at)
        parts = [S.encode_vardct_frame(img, S.frame(emit=2), seed=3, alpha=al)]
        fx = S.frame(emit=1, is_last=0, frame_type=1, lf_level=1, xyb_image=1 if lf_modular else 0)
        if lf_modular:
            ints = np.stack([small[..., 1].astype(np.int32) * 2, small[..., 0].astype(np.int32) // 8 - 16, small[..., 2].astype(np.int32) // 4 - 32, sal.astype(np.int32)], axis=-1)
            parts.append(S.encode_modular_frame(ints, fx, bits=8))
        else:
            parts.append(S.encode_vardct_frame(small, fx, seed=5, distance=0.3, epf_iters=0, gab=0, alpha=sal))
        S.set_alpha_squeeze(squeeze)
        try:
            parts.append(S.encode_vardct_frame(img, S.frame(emit=1, use_lf_frame=1), seed=3, strategy_mix=2, epf_iters=1, alpha=al))
        finally:
            S.set_alpha_squeeze(False)
        out.append((name, b"".join(parts), al))
    return out


def test_lf_frames_of_images_with_alpha():
    import numpy as np
    import oracle_lib as O
    for name, stream, al in lf_frame_alpha_streams():
        px = O.decode(stream).image("u8", 4)
        assert np.array_equal(px[..., 3], al), name


def test_lf_frames_feed_the_frames_that_refer_to_them():
    """frame_header.cc kLFFrame / kUseLfFrame, dec_cache.cc dc_frames: the decode of an image whose LF image comes from an LF frame is the picture
    (within what a distance-1 VarDCT frame loses whose LF image was made from block means of the sRGB samples and coded at distance 0.3); the Modular LF frame's arbitrary samples show up as
    the picture's low frequencies, i.e. the frame is used at all"""
    import numpy as np
    import oracle_lib as O
    for name, stream, img, lf_modular in lf_frame_streams():
        d = O.decode(stream)
        px = d.pixels("u8", 3).reshape(img.shape).astype(np.int32)
        err = np.abs(px - img.astype(np.int32))
        if lf_modular:
            assert err.mean() > 20, name                      # the low frequencies are someone else's
        else:
            # (a plain distance-1 frame of these pictures: mean 1.7 - 1.9; the LF image here is the block means of the sRGB samples, re-quantised)
            assert err.mean() < 6 and np.percentile(err, 99.9) < 70, (name, float(err.mean()), float(err.max()))


def multipass_modular_streams():
    """(name, stream, source samples, bits): Modular frames in several passes (frame_header.cc Passes; passes.h GetDownsamplingBracket): the squeezed
    channels are spread over the PassGroups of the passes by their shift — "responsive" lossless files"""
    import synth_lib as S
    out = []
    for name, (h, w, c, bits), squeeze, passes, ds in [("three_passes", (300, 520, 3, 8), 1, 3, 1), ("two_passes", (300, 520, 3, 8), 1, 2, 1),
                                                      ("no_entries_explicit_chain", (300, 520, 3, 8), 2, 2, 0), ("grey16_three", (700, 900, 1, 16), 1, 3, 1),
                                                      ("one_group", (100, 90, 3, 8), 1, 3, 1), ("alpha_two", (260, 300, 4, 8), 1, 2, 1), ("unsqueezed", (300, 280, 3, 8), 0, 3, 1)]:
        img = _smooth(5, h, w, c, bits)
        out.append((name, S.encode_modular_frame(img, S.frame(mod_passes=passes, mod_ds=ds), bits=bits, squeeze=squeeze), img, bits))
    return out


def test_multipass_modular_frames_are_lossless():
    import numpy as np
    import oracle_lib as O
    for name, data, img, bits in multipass_modular_streams():
        px = O.decode(data).pixels("u16" if bits > 8 else "u8", img.shape[2])
        px = px.view(np.uint16) if bits > 8 else px
        assert np.array_equal(px.reshape(img.shape), img), name


def lz77_lf_streams():
    """(name, LZ77-coded stream, ANS twin): VarDCT frames whose LF-group Modular streams (LF coefficients, HF metadata) are LZ77-coded — copies of the
    value before (distance 1) and of the row above (special distance 0 = the stream's distance multiplier); flat areas make the runs"""
    import synth_lib as S
    out = []
    for name, seed, (w, h), mix, epf in [("small", 1, (320, 200), 1, 1), ("one_group", 2, (64, 48), 0, 2), ("two_lf_groups", 3, (2300, 400), 2, 0)]:
        img = S.synthetic_image(60 + seed, w, h)
        img[: h // 2, : w // 2] = img[0, 0]
        ans = S.encode_vardct(img, seed=seed, strategy_mix=mix, epf_iters=epf)
        S.set_lz77_lf(True)
        try:
            lz = S.encode_vardct(img, seed=seed, strategy_mix=mix, epf_iters=epf)
        finally:
            S.set_lz77_lf(False)
        out.append((name, lz, ans))
    return out


def test_lz77_coded_lf_streams_decode_like_their_ans_twins():
    import numpy as np
    import oracle_lib as O
    for name, lz, ans in lz77_lf_streams():
        assert lz != ans
        assert np.array_equal(O.decode(lz).pixels("u8", 3), O.decode(ans).pixels("u8", 3)), name


def lz77_ac_streams():
    """(name, stream whose AC coefficient streams are LZ77-coded, ANS twin): runs of zero coefficients, repeating pairs and triples of values become
    copies (distance tokens without special codes: these readers have no distance multiplier); single-pass, progressive (every pass its own code
    and window), with prefix codes under the LZ77 layer, with extra channels whose Modular part follows the coefficients"""
    import numpy as np
    import synth_lib as S
    out = []
    for name, seed, (w, h), kw in [("small", 1, (320, 200), dict(strategy_mix=1, epf_iters=1)), ("one_group", 2, (64, 48), dict(strategy_mix=0, epf_iters=2)),
                                   ("many_groups_big_blocks", 3, (1100, 600), dict(strategy_mix=2, epf_iters=0)), ("three_passes", 4, (520, 300), dict(strategy_mix=2, num_passes=3)),
                                   ("two_passes_permuted", 5, (300, 280), dict(strategy_mix=1, num_passes=2, permute_toc=3)), ("prefix", 6, (320, 200), dict(strategy_mix=1)),
                                   ("alpha", 7, (300, 270), dict(strategy_mix=2))]:
        img = S.synthetic_image(70 + seed, w, h)
        img[: h // 3, : w // 2] = img[0, 0]
        if name == "alpha":
            kw = dict(kw, alpha=(np.arange(w * h, dtype=np.uint32).reshape(h, w) % 251).astype(np.uint8))
        if name == "prefix":
            S.set_prefix(True)
        try:
            ans = S.encode_vardct(img, seed=seed, **kw)
            S.set_lz77_ac(True)
            try:
                lz = S.encode_vardct(img, seed=seed, **kw)
            finally:
                S.set_lz77_ac(False)
        finally:
            S.set_prefix(False)
        out.append((name, lz, ans, 4 if name == "alpha" else 3))
    return out


def test_lz77_coded_ac_streams_decode_like_their_ans_twins():
    import numpy as np
    import oracle_lib as O
    for name, lz, ans, nc in lz77_ac_streams():
        assert lz != ans and len(lz) != len(ans), name
        assert np.array_equal(O.decode(lz).pixels("u8", nc), O.decode(ans).pixels("u8", nc)), name


def prev_channel_streams():
    """(name, stream whose LF-group MA tree splits on previous-channel properties, twin under the plain tree)"""
    import synth_lib as S
    out = []
    for name, seed, (w, h), mix, epf in [("small", 1, (320, 200), 1, 1), ("one_group", 2, (64, 48), 0, 2), ("two_lf_groups", 3, (2300, 400), 2, 0)]:
        img = S.synthetic_image(60 + seed, w, h)
        plain = S.encode_vardct(img, seed=seed, strategy_mix=mix, epf_iters=epf)
        S.set_prev_channel_props(True)
        try:
            pc = S.encode_vardct(img, seed=seed, strategy_mix=mix, epf_iters=epf)
        finally:
            S.set_prev_channel_props(False)
        out.append((name, pc, plain))
    return out


def test_previous_channel_properties_in_lf_streams_decode_like_the_plain_tree():
    """context_predict.h PrecomputeReferences inside the LF-group streams of VarDCT frames (cjxl -E): X conditioned on |Y|, B on X and Y, ytob on ytox"""
    import numpy as np
    import oracle_lib as O
    for name, pc, plain in prev_channel_streams():
        assert pc != plain
        assert np.array_equal(O.decode(pc).pixels("u8", 3), O.decode(plain).pixels("u8", 3)), name


def cjxl_shape_streams():
    """(name, shape, stream under the MA-tree shape of a default-effort cjxl encode, twin under the gradient tree).  Shape 1: weighted-predictor
    leaves under a fixed tree over property 15 for the LF coefficients, the fixed row / N / W tree for the HF metadata, default predictor
    parameters; shape 2: the same with the parameters spelt out (other values) in every LF-group header."""
    import synth_lib as S
    out = []
    for name, seed, (w, h), mix, epf in [("small", 1, (320, 200), 1, 1), ("one_group", 2, (64, 48), 0, 2), ("two_lf_groups", 3, (2300, 400), 2, 0), ("tall", 4, (136, 2200), 1, 1)]:
        img = S.synthetic_image(80 + seed, w, h)
        plain = S.encode_vardct(img, seed=seed, strategy_mix=mix, epf_iters=epf)
        for shape in (1, 2):
            S.set_lf_tree_shape(shape)
            try:
                out.append((name, shape, S.encode_vardct(img, seed=seed, strategy_mix=mix, epf_iters=epf), plain))
            finally:
                S.set_lf_tree_shape(0)
    return out


def test_cjxl_shaped_lf_trees_decode_like_the_gradient_tree():
    """The weighted predictor inside LF-group streams (what cjxl writes at its default effort): the synthesiser's encoder-side simulation of the
    predictor (written from the format's definition) and the oracle's decoder agree — same pixels as the twin whose LF coefficients ride under
    the gradient tree; explicit predictor parameters in the group headers included."""
    import numpy as np
    import oracle_lib as O
    for name, shape, cj, plain in cjxl_shape_streams():
        assert cj != plain
        assert np.array_equal(O.decode(cj).pixels("u8", 3), O.decode(plain).pixels("u8", 3)), (name, shape)
