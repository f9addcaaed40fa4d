"""GPU tests (-m gpu) of grouped SIMT LF launches: one LfDecodeSimtKernel launch decodes the LF-group streams of several prepared batches (kernels.h LaunchLfSimtGroup — a
wavefront finds its part of the by-value table from its wave index), as the pipeline's LF issuer enqueues it for jobs that are ready together (pipeline.cc) and as
JxlHipBatchDecodeLfGrouped enqueues it for a list of batches.  Everything runs at lane_stride_lf = 8.  Frames are small but have two or more LF groups (2056x64, 64x2056: two;
2056x2056: four unequal ones) beside one-group frames (64x64, 520x264), so that lanes carry several streams and parts end in the middle of a wavefront.  Every frame is
compared with the CPU oracle, byte for byte, and with the same batch decoded alone."""
import numpy as np
import pytest

import oracle_lib as O
import synth_lib as S

pytestmark = pytest.mark.gpu

kLfVarSimtLean, kLfVarSimtGen, kLfVarSimtWpQuad = 1, 2, 8
INFOS = ("lf_variant", "lf_spec_lanes", "lf_simt_lanes", "lf_simt_streams", "lf_simt_frames", "lf_simt_waves", "lf_wide_bytes", "lf_wide_only")
SIZES = {"wide": (2056, 64), "tall": (64, 2056), "quad": (2056, 2056), "tiny": (64, 64), "mid": (520, 264)}


@pytest.fixture(scope="module")
def jx(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import jpegxl_rs_amd as jx
    return jx


@pytest.fixture(scope="module")
def pool():
    """{name: (stream, oracle u8 pixels)}: encoded and decoded by the oracle once, shared by every test (never modified)"""
    out = {}
    def add(name, kind, seed, tree_shape=0):
        w, h = SIZES[kind]
        S.set_lf_tree_shape(tree_shape)
        try:
            d = S.encode_vardct(S.synthetic_image(seed, w, h), seed=seed, strategy_mix=2, epf_iters=1, gab=1)
        finally:
            S.set_lf_tree_shape(0)
        out[name] = (d, O.decode(d).pixels("u8", 3))
    for i in range(3):
        add(f"wide{i}", "wide", 300 + i)
        add(f"tall{i}", "tall", 310 + i)
        add(f"tiny{i}", "tiny", 320 + i)
        add(f"mid{i}", "mid", 330 + i)
    add("quad0", "quad", 340)
    add("wp_wide", "wide", 350, tree_shape=1)
    add("wp_mid", "mid", 351, tree_shape=1)
    # tree shape 3 (tools/jxl_synth.cc MakeGlobalTree): gradient trees for the LF coefficients, tables over W and N for the HF metadata, no weighted predictor —
    # what only the general instantiation LfDecodeSimtKernel<false, true> decodes
    add("gen_wide", "wide", 352, tree_shape=3)
    add("gen_mid", "mid", 353, tree_shape=3)
    add("gen_tall", "tall", 354, tree_shape=3)
    return out


# the three batches of the first case: 1, 3 and 9 frames of mixed sizes (the 9-frame one: 2 + 2 + 4 + five single LF-group streams over eight lanes a wavefront)
BATCH_1 = ["wide0"]
BATCH_3 = ["tall0", "tiny0", "mid0"]
BATCH_9 = ["wide1", "tiny1", "quad0", "mid1", "tall1", "tiny2", "mid2", "wide2", "tall2"]


def prepared(jx, pool, names):
    b = jx.BatchDecoder(0)
    b.add_many([pool[n][0] for n in names], "uint8", 3, threads=4)
    b.set_lane_stride(8, 1)
    b.prepare()
    return b


def finish(b):
    """the pieces behind the LF decode: LF post-processing, then HF decode, IDCT and pixels"""
    b.decode_part(6); b.decode_part(2); b.finish()


def check(pool, names, b, what):
    for i, n in enumerate(names):
        ref = pool[n][1]
        px = b.output(i).reshape(ref.shape)
        assert np.array_equal(px, ref), f"{what}: frame {i} ({n}): {int((px != ref).sum())} of {px.size} samples differ from the oracle"


def infos(b):
    return {k: b.info_value(k) for k in INFOS}


def alone(jx, pool, names):
    """the batch decoded on its own through decode_part: (outputs, infos)"""
    b = prepared(jx, pool, names)
    b.decode_part(5); finish(b)
    check(pool, names, b, "decoded alone")
    return [b.output(i) for i in range(len(names))], infos(b)


def grouped(jx, pool, lists, what):
    """the batches' LF decodes through one JxlHipBatchDecodeLfGrouped call, everything else batch by batch; every frame against the oracle.  -> the batches"""
    bs = [prepared(jx, pool, names) for names in lists]
    jx.decode_lf_grouped(bs)
    for b in bs:
        finish(b)
    for k, (names, b) in enumerate(zip(lists, bs)):
        check(pool, names, b, f"{what}, batch {k}")
    return bs


def test_three_batches_share_one_launch(jx, pool):
    lists = [BATCH_1, BATCH_3, BATCH_9]
    bs = grouped(jx, pool, lists, "1 + 3 + 9 frames")
    for names, b in zip(lists, bs):
        outs, info = alone(jx, pool, names)
        assert infos(b) == info, (infos(b), info)
        assert info["lf_variant"] == kLfVarSimtLean and info["lf_simt_frames"] == len(names), info
        for i, o in enumerate(outs):
            assert np.array_equal(b.output(i), o), f"batch of {len(names)}, frame {i}: grouped and alone differ"
    # (parts end inside a wavefront and lanes carry several streams: the 9-frame batch has more streams than a wavefront has lanes at stride 8)
    assert bs[2].info_value("lf_simt_streams") > 8 and bs[0].info_value("lf_simt_lanes") < 8


@pytest.mark.parametrize("count", [8, 9])
def test_full_table_and_one_more(jx, pool, count):
    """eight batches fill the table of one launch; nine are split into 8 + 1"""
    names = ["wide0", "tiny0", "tall0", "mid0", "tiny1", "wide1", "mid1", "tall1", "tiny2"]
    lists = [[names[k], names[(k + 3) % 9]] if k % 2 else [names[k]] for k in range(count)]
    grouped(jx, pool, lists, f"{count} batches")


def test_weighted_predictor_batch_between_gradient_batches(jx, pool):
    """different kernels never share a launch: gradient trees | weighted predictor | gradient trees -> the launches of each alone"""
    lists = [["wide0", "tiny0"], ["wp_wide", "wp_mid"], ["tall0", "mid0"]]
    bs = grouped(jx, pool, lists, "lean | weighted predictor | lean")
    assert [b.info_value("lf_variant") & 15 for b in bs] == [kLfVarSimtLean, kLfVarSimtWpQuad, kLfVarSimtLean]
    for names, b in zip(lists, bs):
        assert infos(b) == alone(jx, pool, names)[1]


def test_weighted_predictor_batches_share_a_launch(jx, pool):
    """the weighted-predictor quads take the table as well"""
    lists = [["wp_wide"], ["wp_mid", "wp_wide"]]
    bs = grouped(jx, pool, lists, "two weighted-predictor batches")
    assert all(b.info_value("lf_variant") & kLfVarSimtWpQuad for b in bs)


def test_general_instantiation_beside_lean_batches(jx, pool):
    """batches whose frames need the general instantiation (tables over W / N, no weighted predictor) share a launch of it, the lean ones around them theirs"""
    lists = [["wide0", "tiny0"], ["gen_wide", "gen_mid"], ["gen_tall"], ["gen_mid", "gen_tall", "gen_wide"], ["tall0", "mid0"], ["tiny1"]]
    bs = grouped(jx, pool, lists, "lean | general x 3 | lean x 2")
    assert [b.info_value("lf_variant") for b in bs] == [kLfVarSimtLean] + [kLfVarSimtGen] * 3 + [kLfVarSimtLean] * 2
    for names, b in zip(lists, bs):
        outs, info = alone(jx, pool, names)
        assert infos(b) == info, (infos(b), info)
        for i, o in enumerate(outs):
            assert np.array_equal(b.output(i), o)
    # a batch that mixes the two kinds of frames takes the general instantiation as a whole and groups with general batches
    lists = [["gen_mid"], ["wide1", "gen_tall", "tiny2"]]
    bs = grouped(jx, pool, lists, "general | mixed")
    assert [b.info_value("lf_variant") for b in bs] == [kLfVarSimtGen] * 2


def _damaged(jx, data):
    """the stream with the last 48 bytes of its LF part (the end of its last LF groups' sections) zeroed: headers, TOC and every section's place stay as they are, so
    the parser takes it and the LF kernel is the first to meet the damage (the ANS state a stream ends in is checked)"""
    end = jx.lf_part_size(data)
    assert 200 < end < len(data)
    return data[:end - 48] + bytes(48) + data[end:]


def test_damaged_lf_stream_beside_healthy_batches(jx, pool):
    """a part of the table whose stream fails on the device: that image fails alone, with the message the batch gives when decoded on its own; the other images of its
    batch and the batches that shared the launch are exact"""
    local = dict(pool)
    local["bad"] = (_damaged(jx, pool["wide1"][0]), None)
    lists = [["tall0", "tiny0"], ["mid0", "bad", "wide2"], ["tiny1", "wide0", "mid1"]]
    bs = [prepared(jx, local, names) for names in lists]
    jx.decode_lf_grouped(bs)
    for b in bs:
        b.decode_part(6); b.decode_part(2)
    bs[0].finish(); bs[2].finish()
    with pytest.raises(jx.DecodeError, match=r"corrupt stream \(device status \d+, frame 1\)") as grouped_error:
        bs[1].finish()
    for k, names in enumerate(lists):
        for i, n in enumerate(names):
            if n == "bad":
                continue
            ref = pool[n][1]
            px = bs[k].output(i).reshape(ref.shape)
            assert np.array_equal(px, ref), f"batch {k}, frame {i} ({n}) beside the damaged stream: {int((px != ref).sum())} samples differ"
    b = prepared(jx, local, lists[1])
    b.decode_part(5); b.decode_part(6); b.decode_part(2)
    with pytest.raises(jx.DecodeError) as alone_error:
        b.finish()
    assert str(alone_error.value) == str(grouped_error.value)


def test_group_of_one_is_decode_part(jx, pool):
    b = grouped(jx, pool, [BATCH_9], "a group of one")[0]
    outs, info = alone(jx, pool, BATCH_9)
    assert infos(b) == info
    for i, o in enumerate(outs):
        assert np.array_equal(b.output(i), o)


def _jobs(pool, k):
    """eight jobs of 2 - 4 small frames"""
    names = ["wide0", "tiny0", "tall0", "mid0", "tiny1", "wide1", "mid1", "tall1", "tiny2", "mid2", "wide2", "tall2"]
    return [[names[(3 * j + i) % len(names)] for i in range(2 + j % 3)] for j in range(k)]


def _run_jobs(jx, pool, p, jobs, expect_failed=()):
    bufs, tickets = [], []
    for names in jobs:
        outs = [jx.PinnedBuffer(max(1, pool[n][1].size)) for n in names]
        bufs.append(outs)
        tickets.append(p.submit([pool[n][0] for n in names], "uint8", 3, host_ptrs=[o.ptr for o in outs], capacities=[pool[n][1].size for n in names]))
    for j, (names, outs, t) in enumerate(zip(jobs, bufs, tickets)):
        status, _ = p.wait(t, check=False)
        for i, (n, o) in enumerate(zip(names, outs)):
            if (j, i) in expect_failed:
                assert status[i] == 1 and "truncated" in jx.last_error(), (j, i, list(status), jx.last_error())
                continue
            assert status[i] == 0, (j, i, list(status), jx.last_error())
            assert np.array_equal(np.array(o.array).reshape(-1)[:pool[n][1].size], pool[n][1].reshape(-1)), f"job {j}, frame {i} ({n}) differs from the oracle"


@pytest.mark.parametrize("group_max", [4, 1])
def test_pipeline_groups_jobs_that_are_ready_together(jx, pool, group_max):
    """one LF stream, eight jobs back to back: whatever groups form (that depends on timing), every job is exact and every job is counted once"""
    p = jx.Pipeline(0, jobs_in_flight=8, lf_streams=2, hf_streams=2, prepare_threads=2, parse_threads=2, wide_first=0, reserve_frames=4, reserve_width=2056, reserve_height=2056)
    try:
        p.set_option("lf_streams_effective", 1); p.set_option("lf_group_max", group_max)
        assert p.info("lf_streams_effective") == 1 and p.info("lf_group_max") == group_max
        _run_jobs(jx, pool, p, _jobs(pool, 8))
        assert p.info("lf_grouped_jobs") == 8
        assert 1 <= p.info("lf_groups") <= 8 and 1 <= p.info("lf_group_largest") <= group_max
        if group_max == 1:
            assert p.info("lf_groups") == 8
    finally:
        p.close()


def test_pipeline_job_with_a_truncated_stream_beside_healthy_jobs(jx, pool):
    """the truncated image fails alone, with the parser's message; every other image of its job and of the jobs around it is exact"""
    cut = dict(pool)
    d = pool["wide1"][0]
    cut["cut"] = (d[:len(d) * 2 // 3], pool["wide1"][1])
    p = jx.Pipeline(0, jobs_in_flight=4, lf_streams=2, hf_streams=2, prepare_threads=2, parse_threads=2, wide_first=0, reserve_frames=4, reserve_width=2056, reserve_height=2056)
    try:
        p.set_option("lf_streams_effective", 1)
        _run_jobs(jx, cut, p, [["wide0", "tiny0"], ["tall0", "cut", "mid0"], ["tiny1", "wide2"], ["mid1", "tall1"]], expect_failed={(1, 1)})
        assert p.info("lf_grouped_jobs") == 4
    finally:
        p.close()


def test_small_job_then_larger_job_on_a_cold_pipeline(jx, pool):
    """small_job_frames = 8: a 4-frame job, then a 16-frame job within the first wide_first submits of a fresh pipeline.  The larger job's cold-start chain names the
    ticket before it, which is no chained job: the LF issuer goes through the jobs in ticket order and chains on the device only behind a job that really took the wide
    launch, so nothing waits on the host for a ticket that never reports."""
    small = ["tiny0", "mid0", "wide0", "tall0"]
    large = ["tiny1", "mid1", "wide1", "tall1"] * 4
    p = jx.Pipeline(0, jobs_in_flight=4, lf_streams=2, hf_streams=2, prepare_threads=2, parse_threads=2, small_job_frames=8, reserve_frames=16, reserve_width=2056, reserve_height=264)
    try:
        _run_jobs(jx, pool, p, [small, large])
    finally:
        p.close()
