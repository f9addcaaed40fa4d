"""GPU parity tests (-m gpu) of the candidate lanes of the SIMT LF decode (kernels.hip LfDecodeSimtKernel SPEC, LaunchCfg::lf_spec_lanes): G adjacent lanes carry one
LF-group stream, each reads the alias slot of a candidate cluster beside the class-table read, a sample whose cluster is no candidate takes the one-lane form's dependent
read.  No sample may depend on G: every case runs at lane strides 8, 4 and 1 (G = 8, 4 and 1), with lf_spec_lanes = 2 and with lf_spec_lanes = 1 (the one-lane kernel),
and every frame is compared with the CPU oracle, bit-exact.  The cases reach: rows wider than G in all seven channels; LF groups one block wide / high (rows under four
samples, channels without a next row to prefetch); codes with more clusters than a group has candidates (misses, replacement); codes of one cluster (no miss after the
first); a hybrid-integer configuration per cluster (the candidate carries it); log_alpha 8; lanes that decode several streams of frames with different codes one after the
other (candidates of the frame before must not survive the stream start)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import synth_lib as S

pytestmark = pytest.mark.gpu

kLfVarSimtLean, kLfVarSimtGen = 1, 2

# (lane_stride_lf, lf_spec_lanes, lanes per stream the launch must report)
CONFIGS = [(8, 0, 8), (4, 0, 4), (1, 0, 1), (8, 2, 2), (8, 1, 1)]


@pytest.fixture(scope="module")
def jx(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import jpegxl_rs_amd as jx
    return jx


def _encode(img, frame_seed, **shape):
    if shape:
        S.set_code_shape(which="lf", **shape)
    try:
        return S.encode_vardct(img, seed=frame_seed, strategy_mix=2, epf_iters=1, gab=1)
    finally:
        S.set_code_shape()


def _lf_code(jx, data):
    """{clusters, log_alpha, uniform_cfg} of the stream's global-tree Modular code (JxlHipDebugDescribe; host only)"""
    L = jx.libjxl()
    L.JxlHipDebugDescribe.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 16)
    assert L.JxlHipDebugDescribe(data, len(data), buf, len(buf)) == 0, jx.last_error()
    lines = [dict(t.split("=") for t in l.split() if "=" in t) for l in buf.value.decode().split("\n") if l.startswith("  lf_code")]
    assert lines, buf.value.decode()
    return {k: int(lines[0][k]) for k in ("clusters", "log_alpha", "uniform_cfg")}


@pytest.fixture(scope="module")
def cases(jx):
    """{id: [(stream, oracle u8 pixels), ...]}: the streams of one batch each, encoded and decoded by the oracle once"""
    def one(img, frame_seed, **shape):
        d = _encode(img, frame_seed, **shape)
        return d, O.decode(d).pixels("u8", 3)
    small = S.synthetic_image(71, 264, 136)
    mid = S.synthetic_image(72, 520, 300)
    out = {
        "one_group": [one(small, 3)],
        "group_one_block_wide": [one(S.synthetic_image(73, 2056, 24), 4)],
        "group_one_block_high": [one(S.synthetic_image(74, 24, 2056), 5)],
        "min_clusters_40": [one(mid, 6, min_clusters=40)],
        "max_clusters_1": [one(mid, 7, max_clusters=1)],
        "mixed_uint_configs": [one(mid, 8, uint_configs="mixed")],
        "log_alpha_8": [one(mid, 9, min_log_alpha=8)],
    }
    # one lane, several streams, alternating codes: the second LF group of the wide frame and the six small frames share a lane (decoder.cc PackLanes)
    chain = [one(S.synthetic_image(80, 2100, 1100), 10, min_clusters=40)]
    for i in range(6):
        chain.append(one(S.synthetic_image(81 + i, 136, 136), 11 + i, min_clusters=2 if i % 2 == 0 else 40))
    out["chained_streams"] = chain
    # the same chain with a configuration per cluster, picked differently in every frame: a candidate left over from the stream before would bring the wrong one along
    chain = [one(S.synthetic_image(80, 2100, 1100), 20, min_clusters=40, uint_configs="mixed", seed=1)]
    for i in range(6):
        chain.append(one(S.synthetic_image(81 + i, 136, 136), 21 + i, min_clusters=2 if i % 2 == 0 else 40, uint_configs="mixed", seed=2 + i))
    out["chained_streams_mixed_configs"] = chain
    return out


def batch_decode(jx, streams, lf_stride, hf_stride, options):
    b = jx.BatchDecoder(0)
    b.add_many(streams, "uint8", 3, threads=4)
    b.set_lane_stride(lf_stride, hf_stride)
    b.prepare()
    for k, v in options.items():
        b.set_option(k, v)
    b.decode(); b.finish()
    info = {k: b.info_value(k) for k in ("lf_variant", "lf_spec_lanes", "lf_simt_lanes", "lf_simt_streams", "lf_simt_frames")}
    return [b.output(i) for i in range(len(streams))], info


def test_streams_carry_the_codes_the_cases_name(jx, cases):
    """what the synthesiser wrote is what the cases mean to reach (host only)"""
    assert _lf_code(jx, cases["min_clusters_40"][0][0])["clusters"] > 24      # (one per non-empty context at most: 36 of the 58 here; three times a group's candidates)
    assert _lf_code(jx, cases["max_clusters_1"][0][0])["clusters"] == 1
    assert _lf_code(jx, cases["mixed_uint_configs"][0][0])["uniform_cfg"] == 0
    assert _lf_code(jx, cases["log_alpha_8"][0][0])["log_alpha"] == 8
    assert _lf_code(jx, cases["one_group"][0][0])["uniform_cfg"] == 1
    chain = [_lf_code(jx, d)["clusters"] for d, _ in cases["chained_streams"]]
    assert chain[0] > 24 and max(chain[1::2]) < min(chain[2::2]), chain       # (neighbours on the lane: codes of different sizes)
    assert all(_lf_code(jx, d)["uniform_cfg"] == 0 for d, _ in cases["chained_streams_mixed_configs"])


@pytest.mark.parametrize("lf_stride,spec_lanes,group", CONFIGS)
@pytest.mark.parametrize("case", ["one_group", "group_one_block_wide", "group_one_block_high", "min_clusters_40", "max_clusters_1", "mixed_uint_configs", "log_alpha_8",
                                  "chained_streams", "chained_streams_mixed_configs"])
def test_candidate_lanes_match_oracle(jx, cases, case, lf_stride, spec_lanes, group):
    frames = cases[case]
    got, info = batch_decode(jx, [d for d, _ in frames], lf_stride, 1, {"lf_spec_lanes": spec_lanes})
    assert info["lf_simt_frames"] == len(frames) and info["lf_variant"] in (kLfVarSimtLean, kLfVarSimtGen), info      # the SIMT kernel without the weighted predictor, nothing else
    assert info["lf_spec_lanes"] == group, info
    if case.startswith("chained_streams"):
        assert info["lf_simt_streams"] > info["lf_simt_lanes"], info                                             # some lane got more than one stream
    for i, ((d, ref), px) in enumerate(zip(frames, got)):
        px = px.reshape(ref.shape)
        assert np.array_equal(px, ref), f"{case} frame {i}, stride {lf_stride}, lf_spec_lanes {spec_lanes}: {int((px != ref).sum())} of {px.size} samples differ"
