"""The weighted predictor of the LF-group streams against its definition (PARITY.md "Modular integer stages").

Two links that carry the restatement of test_modular_formulas.py to the LF kernels (SIMT lanes, QUAD form, wave-wide decoders), which only ever see streams
written by the synthesiser's own encoder-side simulation of the predictor:

  CPU   the synthesiser's LF tokeniser (the ModularTokens that frame encoding calls, synth_lib.lf_residuals) gives residuals; the RESTATED tree walk and
        predictor, given those residuals, must give the planes back.  With the round trips HIP == oracle == gradient-tree twin of test_synth_roundtrip /
        test_gpu_parity / test_round6_wave, the simulation — and every decoder that undoes it — is pinned to the format's text, not to each other.
  GPU   cjxl-shaped VarDCT frames at the smallest geometries (one LF sample, one row, one column, a second LF group one block wide) through the three LF paths."""
import numpy as np
import pytest

import oracle_lib as O
import synth_lib as S
import test_modular_formulas as F


@pytest.fixture(scope="module")
def jx(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import jpegxl_rs_amd as jx
    return jx


LF_HEADERS = {1: F.WP_DEFAULT, 2: F.WP_SHAPE2}
LF_TREE = F.cutoff_tree(15, F.LF_CUTOFFS, 6)


def lf_planes(seed, w, h):
    """Three planes shaped like quantised LF coefficients: smooth, plus noise of about +-600 (so the true errors, in eighths, cross the +-500 cut-offs)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for c in range(3):
        smooth = 900 * np.sin(xx / 9.0 + c) * np.cos(yy / 6.0) + 40 * c
        noise = rng.integers(-600, 601, (h, w)) * (rng.integers(0, 4, (h, w)) == 0) + rng.integers(-3, 4, (h, w))
        out.append(np.rint(smooth + noise).astype(np.int64))
    return out


@pytest.mark.parametrize("shape", (1, 2))
def test_lf_tokeniser_residuals_decode_to_the_planes_under_the_restated_predictor(shape):
    """Widths 1, 2, 3, 37, 256 x heights 1, 2, 23: residuals from the synthesiser's tokeniser, decoded by the restatement alone"""
    reached, stats = set(), F.WpStats()
    for w in (1, 2, 3, 37, 256):
        for h in (1, 2, 23):
            planes = lf_planes(100 * w + h + shape, w, h)
            res = S.lf_residuals(planes, shape)
            assert res.shape == (3, h, w)
            st, branch = F.Stats(), {}
            got = F.decode_stream([(w, h, False)] * 3, [r for r in res], LF_TREE, 1, st.peak, branch, (LF_HEADERS[shape], st.wp))
            for c in range(3):
                assert np.array_equal(got[c], planes[c]), (shape, w, h, c, np.argwhere(got[c] != planes[c])[:3])
            assert st.wp.n["samples"] == 3 * w * h and st.wp.stored < 1 << 31
            reached |= {n for n, k in branch.items() if k}
            stats.add(st.wp)
    assert set(F._extreme_leaves(LF_TREE)) <= reached and len(reached) >= 25, len(reached)      # property 15 beyond +-500 and between most cut-offs
    assert all(stats.n[k] > 0 for k in F.WP_CLASSES), stats.n


# ---- LF kernels at the smallest geometries ------------------------------------------------------------------------------------------------------------
EDGE_SIZES = ((8, 8), (16, 8), (8, 24), (24, 16), (2056, 16))                   # LF images of 1x1, 2x1, 1x3, 3x2 and 257x2: the last has a second LF group one block wide
_edge = {}


def edge_streams():
    """[(w, h, shape, cjxl-shaped stream, the oracle's u8 decode of its gradient-tree twin)], made once"""
    if not _edge:
        items = []
        for k, (w, h) in enumerate(EDGE_SIZES):
            img = S.synthetic_image(90 + k, w, h)
            plain = S.encode_vardct(img, seed=5 + k, strategy_mix=k % 3, epf_iters=k % 2)
            ref = O.decode(plain).pixels("u8", 3)
            ref.setflags(write=False)
            for shape in (1, 2):
                S.set_lf_tree_shape(shape)
                try:
                    cj = S.encode_vardct(img, seed=5 + k, strategy_mix=k % 3, epf_iters=k % 2)
                finally:
                    S.set_lf_tree_shape(0)
                assert cj != plain
                items.append((w, h, shape, cj, ref))
        _edge["items"] = items
    return _edge["items"]


def test_oracle_decodes_edge_geometries_like_the_gradient_twin():
    for w, h, shape, cj, ref in edge_streams():
        assert np.array_equal(O.decode(cj).pixels("u8", 3), ref), (w, h, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", (1, 2))
def test_lf_weighted_predictor_kernels_at_edge_geometries(jx, shape):
    """Single-image decode (one wavefront per stream), a SIMT batch at lane stride 4, and the wide first launch: the oracle's pixels of the gradient-tree twin"""
    mine = [(w, h, cj, ref) for w, h, sh, cj, ref in edge_streams() if sh == shape]
    for w, h, cj, ref in mine:
        _, px = jx.decoder_builder().decode_with(cj, np.uint8)
        assert np.array_equal(px.reshape(-1), ref.reshape(-1)), ("single", w, h)
    for wide in (0, 1):
        b = jx.BatchDecoder(0)
        b.set_lane_stride(4, 1)
        b.add_many([cj for _, _, cj, _ in mine], "uint8", 3)
        b.prepare()
        assert b.info_value("lf_simt_frames") == len(mine) and b.info_value("lf_simt_wp") == 1
        if wide:
            b.set_option("lf_wide_once", 1)
        b.decode(); b.finish()
        for i, (w, h, _, ref) in enumerate(mine):
            assert np.array_equal(b.output(i).reshape(-1), ref.reshape(-1)), ("wide" if wide else "simt", w, h)
