"""CPU tests of the synthesiser's entropy-code shape controls (synth_lib.set_code_shape): the codes it writes have the clusters, log_alpha and hybrid-uint
configurations asked for (JxlHipDebugDescribe, host-only), the oracle decodes them to the same pixels as the synthesiser's own shape, and with the
controls at their defaults the output is byte for byte what it was before they existed."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import oracle_lib as O
import synth_lib as S


def psnr(a, b):
    m = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return 10 * np.log10(255.0 ** 2 / max(m, 1e-12))


@pytest.fixture(scope="module")
def describe(built):
    import jpegxl_rs_amd as jx
    L = jx.libjxl()
    L.JxlHipDebugDescribe.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]

    def run(data):
        buf = C.create_string_buffer(1 << 16)
        assert L.JxlHipDebugDescribe(data, len(data), buf, len(buf)) == 0, jx.last_error()
        return [dict([("which", l.split()[0])] + [t.split("=") for t in l.split() if "=" in t])
                for l in buf.value.decode().split("\n") if l.startswith(("  lf_code", "  ac_code"))]
    return run


IMG = (41, 400, 260)


def _streams(**shape):
    """plain, 4 HF presets, 2 passes, 4:2:0 YCbCr, LZ77 AC — one VarDCT frame each under `shape`"""
    img = S.synthetic_image(*IMG)
    S.set_code_shape(**shape)
    try:
        out = {"plain": S.encode_vardct(img, seed=3, strategy_mix=2, distance=0.5)}
        S.set_hf_presets(4)
        try:
            out["presets4"] = S.encode_vardct(img, seed=3, strategy_mix=2, distance=0.5)
        finally:
            S.set_hf_presets(1)
        out["passes2"] = S.encode_vardct(img, seed=3, num_passes=2)
        out["ycbcr420"] = S.encode_ycbcr(img, "420", seed=3)
        S.set_lz77_ac(True)
        try:
            out["lz77_ac"] = S.encode_vardct(img, seed=3)
        finally:
            S.set_lz77_ac(False)
    finally:
        S.set_code_shape()
    return out


SHAPES = [dict(min_clusters=256, uint_configs="mixed", seed=1), dict(min_log_alpha=8, uint_configs="mixed", seed=2), dict(uint_configs=[(0, 0, 0)]),
          dict(max_clusters=4, min_log_alpha=7), dict(min_clusters=256, min_log_alpha=7, which="ac"), dict(uint_configs="mixed", which="lf", seed=5)]


@pytest.mark.parametrize("shape", SHAPES, ids=[",".join(f"{k}={v}" for k, v in s.items()) for s in SHAPES])
def test_codes_have_the_shape_asked_for(describe, shape):
    which = shape.get("which", "both")
    for kind, data in _streams(**shape).items():
        for c in describe(data):
            applies = which == "both" or (which == "ac") == (c["which"] == "ac_code")
            n, la, uni = int(c["clusters"]), int(c["log_alpha"]), c["uniform_cfg"]
            if not applies:       # the synthesiser's own shape
                assert uni == "1" and n <= 96, (kind, c)
                continue
            if shape.get("min_clusters"):
                # (one cluster per non-empty context: every AC code here has more than 256 of them, the LF codes fewer than their 58 contexts but more than the 32 clusters
                # of the synthesiser's own shape)
                assert n == 256 if c["which"] == "ac_code" else 32 < n <= int(c["contexts"]), (kind, c)
            if shape.get("max_clusters"):
                assert n <= shape["max_clusters"], (kind, c)
            lz77_ac = kind == "lz77_ac" and c["which"] == "ac_code"
            if shape.get("min_log_alpha"):
                assert la >= shape["min_log_alpha"], (kind, c)
            if shape.get("uint_configs") == [(0, 0, 0)] and not lz77_ac:
                assert la == 5, (kind, c)             # tokens of {0, 0, 0} are 1 + floor(log2(v)): 32 slots hold them
            assert uni == ("0" if shape.get("uint_configs") == "mixed" else "1"), (kind, c)


@pytest.mark.parametrize("shape", SHAPES[:4], ids=["c256_mixed", "la8_mixed", "uniform_000", "few_la7"])
def test_oracle_decodes_shaped_codes_like_the_default_ones(shape):
    """the code's shape changes how the coefficients are coded, not which: the oracle's pixels are those of the default-shape stream, close to the source"""
    img = S.synthetic_image(*IMG)
    ref = _streams()
    for kind, data in _streams(**shape).items():
        assert data != ref[kind], kind
        out = O.decode(data).image("u8", 3)
        assert np.array_equal(out, O.decode(ref[kind]).image("u8", 3)), kind
        assert psnr(out, img) > 33.0, kind


@pytest.mark.parametrize("shape", SHAPES[:3], ids=["c256_mixed", "la8_mixed", "uniform_000"])
def test_free_modular_codes_take_the_shape(shape):
    """encode_modular_free: the pixels are what a decoder makes of the token stream — the same tokens under another code give the same pixels"""
    kw = dict(seed=19, w=300, h=200, nchan=3, bits=8, tree_flags=S.TREE_WP | S.TREE_PREV_CHANNELS, tree_depth=7)
    ref = S.encode_modular_free(**kw)
    S.set_code_shape(**shape)
    try:
        data = S.encode_modular_free(**kw)
    finally:
        S.set_code_shape()
    assert data != ref
    assert np.array_equal(O.decode(data).image("u8", 3), O.decode(ref).image("u8", 3))


# sha256 (first 32 hex digits) of streams written before the shape controls existed
DEFAULT_HASHES = {
    "vardct_smoke": "8c46a8ee337a8de3d5bc9c00580bf4e3",
    "vardct_d03": "a2350ff056eabbc6edbec2ab9402ad27",
    "presets4": "28d2b4286cf37b0be350d8a1c2245bf4",
    "passes2": "4aa30e98829ad390c00f8bbf44cd3948",
    "ycbcr420": "5af1faf7194934547d9c37a0c90a55ae",
    "lz77_ac": "d2f066e33b6df744390a5335b609bd14",
    "modular_free": "28d3f6c2e6f43c785efa5d24edeeeae9",
    "modular": "792ec40040bd28277c3e30b56f276fc4",
}


def test_default_shape_is_byte_identical():
    """with the controls at their defaults — never set, or set and cleared again — the synthesiser writes exactly what it wrote before"""
    def encode_all():
        out = {"vardct_smoke": S.encode_vardct(S.synthetic_image(11, 320, 200), seed=3, strategy_mix=2, epf_iters=1, gab=1),
               "vardct_d03": S.encode_vardct(S.synthetic_image(21, 520, 300), seed=4, strategy_mix=2, distance=0.3)}
        S.set_hf_presets(4)
        try:
            out["presets4"] = S.encode_vardct(S.synthetic_image(22, 520, 300), seed=5, strategy_mix=1)
        finally:
            S.set_hf_presets(1)
        out["passes2"] = S.encode_vardct(S.synthetic_image(23, 400, 300), seed=6, num_passes=2)
        out["ycbcr420"] = S.encode_ycbcr(S.synthetic_image(24, 300, 200), "420", seed=7)
        S.set_lz77_ac(True)
        try:
            out["lz77_ac"] = S.encode_vardct(S.synthetic_image(25, 300, 200), seed=8)
        finally:
            S.set_lz77_ac(False)
        out["modular_free"] = S.encode_modular_free(seed=9, w=200, h=150, tree_flags=31, tree_depth=6)
        out["modular"] = S.encode_modular(S.synthetic_image(26, 200, 100).astype(np.int32), 8, True)
        return {k: hashlib.sha256(v).hexdigest()[:32] for k, v in out.items()}
    assert encode_all() == DEFAULT_HASHES
    S.set_code_shape(min_clusters=256, min_log_alpha=8, uint_configs="mixed", seed=7)
    S.set_code_shape()
    assert encode_all() == DEFAULT_HASHES
