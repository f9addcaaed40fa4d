"""GPU parity tests (-m gpu) of the entropy decoders on codes shaped like a real encoder's output (synth_lib.set_code_shape): few / 96 / 256 clusters,
log_alpha 5 / 7 / 8, one hybrid-uint configuration for every cluster or one per cluster.  The synthesiser's own codes all have one shape (96 clusters,
log_alpha 6, one configuration), so the kernel paths that only other shapes take — per-cluster configurations in the wave-wide decoders, the
UCFG=false chunk decoder, alias tables in global memory, partial staging of a code too large for the LDS budget, the wave-wide HF kernel's fall-back —
are exercised here, each through every launch shape, against the CPU oracle (bit-exact for integer output, 1 ULP for f32).  The launch trace of
Batch::Info (hf_variant / lf_variant, kernels.h kHfVar* / kLfVar*) shows which kernel ran; test_every_decode_variant_is_taken asserts each was reached."""
import ctypes as C
import itertools

import numpy as np
import pytest

import oracle_lib as O
import synth_lib as S

pytestmark = pytest.mark.gpu

HF_VARIANTS = {1: "HfDecodeWaveKernel", 2: "HfDecodeSimtKernel<true,false,false> (plain)", 4: "HfDecodeSimtKernel<true,true,true> (all-LDS general)",
               8: "HfDecodeSimtKernel<false,true,true> (tables in global memory)", 16: "HfDecodeKernel (lane-stride batch)",
               32: "HfDecodeKernel beside the SIMT kernel (LZ77 / prefix AC codes)"}
LF_VARIANTS = {1: "LfDecodeSimtKernel<false,false>", 2: "LfDecodeSimtKernel<false,true>", 4: "LfDecodeSimtKernel<true,true>", 8: "LfDecodeSimtKernel<true,true,true>",
               16: "LfDecodeKernel<true> (four groups per workgroup)", 32: "LfDecodeKernel<false>"}

# code shapes: clusters {few, 96, 256} x log_alpha {5, 7, 8} x configurations {uniform, per cluster}
CLUSTERS, ALPHAS, CFGS = ("few", "c96", "c256"), ("la5", "la7", "la8"), ("uniform", "mixed")
KINDS = ("plain", "presets4", "passes2", "ycbcr420", "lz77_ac", "modular_free")


def shape_kwargs(name):
    """set_code_shape arguments of a shape name such as "c256_la7_mixed" (uniform at log_alpha 5: every cluster under {0, 0, 0}, whose alphabet fits 32 slots)"""
    cl, la, cfg = name.split("_")
    kw = {"few": dict(max_clusters=5), "c96": {}, "c256": dict(min_clusters=256)}[cl]
    kw = dict(kw, min_log_alpha=int(la[2:]))
    if cfg == "mixed":
        kw.update(uint_configs="mixed", seed=sum(map(ord, name)))
    elif la == "la5":
        kw.update(uint_configs=[(0, 0, 0)])
    return kw


def _cover():
    """(kind, shape) rows, a pairwise cover of the four factors: per kind one shape per cluster count, the log_alpha values permuted differently for every
    kind, the configuration alternating"""
    rows = []
    for k, (kind, perm) in enumerate(zip(KINDS, itertools.permutations(ALPHAS))):
        for r, cl in enumerate(CLUSTERS):
            rows.append((kind, f"{cl}_{perm[r]}_{CFGS[(r + k) % 2]}"))
    return rows


# the cover, plus plain frames with the two codes the coverage test needs (per-cluster configurations small enough for the wave-wide HF kernel; an alias
# table of 196 KB) whatever the cover gives the plain kind
ROWS = _cover() + [("plain", "c256_la5_mixed"), ("plain", "c96_la8_mixed")]


def _encode(kind, shape, seed):
    img = S.synthetic_image(300 + seed, 520 - 40 * (seed % 3), 300 - 24 * (seed % 4))
    S.set_code_shape(**shape_kwargs(shape))
    try:
        if kind == "plain":
            return S.encode_vardct(img, seed=seed, strategy_mix=2, distance=0.5, epf_iters=1, gab=1)
        if kind == "presets4":
            S.set_hf_presets(4)
            try:
                return S.encode_vardct(img, seed=seed, strategy_mix=1, distance=0.7)
            finally:
                S.set_hf_presets(1)
        if kind == "passes2":
            return S.encode_vardct(img, seed=seed, num_passes=2, strategy_mix=2)
        if kind == "ycbcr420":
            return S.encode_ycbcr(img, "420", seed=seed)
        if kind == "lz77_ac":
            S.set_lz77_ac(True)
            try:
                return S.encode_vardct(img, seed=seed, strategy_mix=1)
            finally:
                S.set_lz77_ac(False)
        return S.encode_modular_free(seed=seed, w=300, h=260, nchan=3, bits=8, tree_flags=S.TREE_WP | S.TREE_PREV_CHANNELS, tree_depth=7)
    finally:
        S.set_code_shape()


@pytest.fixture(scope="module")
def jx(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import jpegxl_rs_amd as jx
    return jx


@pytest.fixture(scope="module")
def cases(jx):
    """{id: (stream, oracle u8 pixels)} for every row of the cover, plus one frame of two LF groups and one under a weighted-predictor LF tree"""
    out = {}
    for i, (kind, shape) in enumerate(ROWS):
        d = _encode(kind, shape, 11 + i)
        out[f"{kind}-{shape}"] = (d, O.decode(d).pixels("u8", 3))
    img = S.synthetic_image(390, 2100, 300)
    S.set_code_shape(**shape_kwargs("c256_la7_mixed"))
    try:
        d = S.encode_vardct(img, seed=39, strategy_mix=2, distance=0.5)
    finally:
        S.set_code_shape()
    out["two_lf_groups-c256_la7_mixed"] = (d, O.decode(d).pixels("u8", 3))
    S.set_code_shape(**shape_kwargs("c256_la5_mixed")); S.set_lf_tree_shape(1)     # (the weighted-predictor LF tree of a default-effort cjxl encode)
    try:
        d = S.encode_vardct(S.synthetic_image(391, 520, 300), seed=40, strategy_mix=2, distance=0.5)
    finally:
        S.set_code_shape(); S.set_lf_tree_shape(0)
    out["wp_lf_tree-c256_la5_mixed"] = (d, O.decode(d).pixels("u8", 3))
    return out


def _describe(jx, data):
    L = jx.libjxl()
    L.JxlHipDebugDescribe.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 16)
    assert L.JxlHipDebugDescribe(data, len(data), buf, len(buf)) == 0, jx.last_error()
    return [dict(t.split("=") for t in l.split() if "=" in t) for l in buf.value.decode().split("\n") if l.startswith(("  lf_code", "  ac_code"))]


def batch_decode(jx, streams, strides=(64, 1), trace=None, **options):
    """decodes `streams` in one batch; trace: a list that gets one dict of the launch-trace values"""
    b = jx.BatchDecoder(0)
    b.add_many(streams, "uint8", 3, threads=4)
    b.set_lane_stride(*strides)
    b.prepare()
    for k, v in options.items():
        b.set_option(k, v)
    b.decode(); b.finish()
    if trace is not None:
        trace.append({k: b.info_value(k) for k in ("hf_variant", "lf_variant", "lf_wide_bytes", "lf_wide_only", "ac_cfg_uniform", "mod_cfg_uniform",
                                                    "ac_code_bytes", "ac_code_bytes_compact", "mod_code_bytes")})
    return [b.output(i) for i in range(len(streams))]


def _same(px, ref, what):
    px = px.reshape(ref.shape)
    assert np.array_equal(px, ref), f"{what}: {int((px != ref).sum())} of {px.size} samples differ"


def test_shapes_are_what_the_cover_asks_for(jx, cases):
    """the streams carry the codes their names promise (JxlHipDebugDescribe)"""
    for cid, (d, _) in cases.items():
        kind, shape = cid.split("-")
        if kind == "modular_free":
            continue
        ac = [c for c in _describe(jx, d) if "pass" in c]
        cl, la, cfg = shape.split("_")
        for c in ac:
            n = int(c["clusters"])
            assert (n <= 6) if cl == "few" else (n > 200) if cl == "c256" else (40 <= n <= 96), (cid, c)
            if kind != "lz77_ac":            # (LZ77 length symbols start at 224: log_alpha 8 whatever was asked)
                assert int(c["log_alpha"]) == int(la[2:]), (cid, c)
            assert c["uniform_cfg"] == ("1" if cfg == "uniform" else "0"), (cid, c)


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32"])
def test_latency_path_matches_oracle(jx, cases, dtype):
    """decode_with (the latency path: wave-wide HF and LF decoders where they apply) — u8 / u16 bit-exact, f32 within 1 ULP"""
    kind_of = {"uint8": "u8", "uint16": "u16", "float32": "f32"}
    ids = sorted(cases) if dtype == "uint8" else sorted(cases)[::3]
    for cid in ids:
        d = cases[cid][0]
        meta, px = jx.decoder_builder(pixel_format=jx.PixelFormat(num_channels=3)).decode_with(d, np.dtype(dtype))
        ref = O.decode(d).pixels(kind_of[dtype], 3)
        ref = ref.view(np.dtype("<" + np.dtype(dtype).str[1:])).astype(dtype)
        px = px.reshape(ref.shape)
        if dtype == "float32":
            a = px.view(np.int32).astype(np.int64); b = ref.view(np.int32).astype(np.int64)
            a = np.where(a < 0, -(a & 0x7FFFFFFF), a); b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
            assert np.abs(a - b).max() <= 1, cid
        else:
            _same(px, ref, cid)


LAUNCHES = [("hf_lanes_per_wave=1", (64, 1), {"hf_lanes_per_wave": 1}), ("hf_lanes_per_wave=4", (64, 1), {"hf_lanes_per_wave": 4}),
            ("hf_lanes_per_wave=0", (64, 1), {"hf_lanes_per_wave": 0}), ("lf_force_big=1", (64, 1), {"lf_force_big": 1}),
            ("lf_force_big=2", (64, 1), {"lf_force_big": 2}), ("lf_force_big=-1", (64, 1), {"lf_force_big": -1}),
            ("simt_lf", (4, 1), {}), ("lf_wide_once", (4, 1), {"lf_wide_once": 1}),
            ("hf_block_threads=128", (64, 64), {"hf_block_threads": 128}), ("hf_block_threads=512", (64, 64), {"hf_block_threads": 512})]


@pytest.mark.parametrize("launch", LAUNCHES, ids=[l[0] for l in LAUNCHES])
def test_launch_shapes_match_oracle(jx, cases, launch):
    """every code through every launch shape of the batch API, one stream per batch (so that the kernel choice is the stream's own), and all of them in
    one batch"""
    name, strides, options = launch
    for cid, (d, ref) in sorted(cases.items()):
        _same(batch_decode(jx, [d], strides, **options)[0], ref, f"{name} {cid}")
    ids = sorted(cases)
    got = batch_decode(jx, [cases[c][0] for c in ids], strides, **options)
    for cid, px in zip(ids, got):
        _same(px, cases[cid][1], f"{name} {cid} (whole batch)")


def _budgets(info, code_lines):
    """every StageCode boundary of the AC and the Modular code (config; + context map; + plain alias table; + wide copy; compact form), 1 byte below and at it, and 0"""
    out = {0}
    ac = [c for c in code_lines if "pass" in c]
    lf = [c for c in code_lines if "pass" not in c]
    bounds = set()
    for c in ac:
        cfg = (int(c["clusters"]) * 4 + 15) & ~15
        bounds |= {cfg, cfg + ((int(c["contexts"]) + 15) & ~15)}
    for c in lf:
        bounds.add((int(c["clusters"]) * 4 + 15) & ~15)
    a, m = info["ac_code_bytes"], info["mod_code_bytes"]
    bounds |= {a, a * 5 // 4 + 64, info["ac_code_bytes_compact"], m, m * 9 // 4 + 64}
    for b in bounds:
        out |= {b - 1, b}
    return sorted(v for v in out if 0 <= v <= 128 * 1024)


@pytest.mark.parametrize("strides,options", [((64, 1), {"hf_lanes_per_wave": 0}), ((4, 64), {"lf_wide_once": 1})], ids=["simt_hf", "lane_stride_hf+wide_lf"])
def test_lds_code_budget_sweep(jx, cases, strides, options):
    """lds_code_budget 1 byte below and exactly at every staging boundary of the batch's codes, and 0: every partial-staging outcome of StageCode"""
    picks = [c for c in sorted(cases) if c.split("-")[0] in ("plain", "passes2", "ycbcr420", "presets4")][::2]
    assert len(picks) >= 4
    for cid in picks:
        d, ref = cases[cid]
        tr = []
        batch_decode(jx, [d], strides, trace=tr, **options)
        for budget in _budgets(tr[0], _describe(jx, d)):
            _same(batch_decode(jx, [d], strides, lds_code_budget=budget, **options)[0], ref, f"{cid} lds_code_budget={budget}")


def test_pipeline_job_of_shaped_frames(jx, cases):
    """one pipeline job of every VarDCT case (the throughput path) — the same pixels"""
    ids = [c for c in sorted(cases) if not c.startswith("modular_free")]
    assert len(ids) >= 16
    p = jx.Pipeline(0, jobs_in_flight=2, lf_streams=2, prepare_threads=2, parse_threads=2)
    try:
        outs = [jx.PinnedBuffer(cases[c][1].size) for c in ids]
        t = p.submit([cases[c][0] for c in ids], "uint8", 3, host_ptrs=[o.ptr for o in outs], capacities=[cases[c][1].size for c in ids])
        status, _ = p.wait(t)
        assert status == [0] * len(ids)
        for cid, o in zip(ids, outs):
            _same(np.array(o.array), cases[cid][1], f"pipeline {cid}")
    finally:
        p.close()


# variants no stream of any shape reaches through the batch API's options, and why
UNREACHABLE = {("lf", 4): "LfDecodeSimtKernel<true,true> (one lane per weighted-predictor stream) runs only under the JXL_HIP_LF_NOQUAD A/B switch; the "
                          "production launch of weighted-predictor trees is the four-lanes-per-stream instantiation"}


def test_every_decode_variant_is_taken(jx, cases):
    """self-contained: decodes that between them must take every HF and LF entropy-decode kernel at the default LDS budget, per-cluster configurations
    in the wave-wide HF and LF decoders, and the fall-backs that only large codes reach.  With the synthesiser's own code shape alone, several of these
    are never reached — the failure message names them."""
    def first(pred):
        return next(c for c in sorted(cases) if pred(c))
    plan = [
        ("plain, small code, one stream per wavefront", first(lambda c: c.startswith("plain-few")), (64, 1), {"hf_lanes_per_wave": 1}),
        ("plain, per-cluster configurations, wave-wide HF", "plain-c256_la5_mixed", (64, 1), {"hf_lanes_per_wave": 1}),
        ("plain, dense SIMT", first(lambda c: c.startswith("plain-few")), (64, 1), {"hf_lanes_per_wave": 0}),
        ("progressive, SIMT general", first(lambda c: c.startswith("passes2-few")), (64, 1), {"hf_lanes_per_wave": 0}),
        ("alias tables beyond the budget: global memory", "plain-c96_la8_mixed", (64, 1), {"hf_lanes_per_wave": 0}),
        ("code over 150 KB: the wave-wide HF kernel hands over", "two_lf_groups-c256_la7_mixed", (64, 1), {"hf_lanes_per_wave": 1}),
        ("lane-stride batch", first(lambda c: c.startswith("plain-")), (64, 64), {"hf_block_threads": 128}),
        ("LZ77 AC code", first(lambda c: c.startswith("lz77_ac")), (64, 1), {}),
        ("LF big", first(lambda c: c.startswith("plain-")), (64, 1), {"lf_force_big": 1}),
        ("LF small", first(lambda c: c.startswith("plain-")), (64, 1), {"lf_force_big": -1}),
        ("LF SIMT", first(lambda c: c.startswith("plain-")), (4, 1), {}),
        ("LF SIMT, weighted-predictor tree", "wp_lf_tree-c256_la5_mixed", (4, 1), {}),
        ("LF wide once, per-cluster Modular configurations", "plain-c256_la5_mixed", (4, 1), {"lf_wide_once": 1}),
        ("LF code too large for the wide copy", "plain-c96_la8_mixed", (64, 1), {}),
    ]
    hf_seen, lf_seen, facts = {}, {}, {}
    for what, cid, strides, options in plan:
        d, ref = cases[cid]
        tr = []
        _same(batch_decode(jx, [d], strides, trace=tr, **options)[0], ref, what)
        t = tr[0]
        for bit in HF_VARIANTS:
            if t["hf_variant"] & bit:
                hf_seen.setdefault(bit, what)
        for bit in LF_VARIANTS:
            if t["lf_variant"] & bit:
                lf_seen.setdefault(bit, what)
        if t["hf_variant"] & 1 and t["ac_cfg_uniform"] == 0:
            facts.setdefault("per-cluster AC configurations in HfDecodeWaveKernel", what)
        if options.get("hf_lanes_per_wave") == 1 and not t["hf_variant"] & 1:
            facts.setdefault("HfDecodeWaveKernel's fall-back for a code over 150 KB", what)
        if t["lf_variant"] & 48 and t["lf_wide_bytes"] > 0 and t["mod_cfg_uniform"] == 0:
            facts.setdefault("per-cluster Modular configurations in the wave-wide LF decoder", what)
        if t["lf_variant"] & 48 and t["lf_wide_bytes"] == 0:
            facts.setdefault("LfDecodeKernel's lane-0 serial path without the wide copy", what)
        if t["lf_wide_only"]:
            facts.setdefault("the wide layout alone (LdAliasAt)", what)
        if t["hf_variant"] & 8 and t["ac_code_bytes"] > 64 * 1024:
            facts.setdefault("an AC code over the default LDS budget", what)
    lf_simt = {1, 2} & set(lf_seen)
    missing = [HF_VARIANTS[b] for b in HF_VARIANTS if b not in hf_seen]
    missing += [LF_VARIANTS[b] for b in LF_VARIANTS if b not in lf_seen and ("lf", b) not in UNREACHABLE and b not in (1, 2)]
    if not lf_simt:
        missing.append("LfDecodeSimtKernel<false,false> or <false,true>")
    missing += [f for f in ("per-cluster AC configurations in HfDecodeWaveKernel", "HfDecodeWaveKernel's fall-back for a code over 150 KB",
                            "per-cluster Modular configurations in the wave-wide LF decoder", "LfDecodeKernel's lane-0 serial path without the wide copy",
                            "the wide layout alone (LdAliasAt)", "an AC code over the default LDS budget") if f not in facts]
    for key, why in UNREACHABLE.items():
        assert key[1] not in (lf_seen if key[0] == "lf" else hf_seen), f"listed as unreachable but taken: {why}"
    print("taken:", {HF_VARIANTS[b]: w for b, w in hf_seen.items()}, {LF_VARIANTS[b]: w for b, w in lf_seen.items()}, facts)
    print("not reachable:", list(UNREACHABLE.values()))
    assert not missing, "variants not reached: " + "; ".join(missing)


def test_corrupted_shaped_streams_fail_cleanly_or_decode(jx, cases):
    """bit flips / truncation in a per-cluster-configuration stream and in a stream whose alias tables stay in global memory: a DecodeError or a decode of the
    right size, never a crash; the clean streams decode bit-exactly afterwards"""
    rng = np.random.default_rng(1606)
    mixed = cases["plain-c256_la5_mixed"]
    glob = cases["plain-c96_la8_mixed"]
    outcomes = {"error": 0, "decoded": 0}
    for (data, _), trials in ((mixed, 14), (glob, 14)):
        for trial in range(trials):
            bad = bytearray(data)
            for pos in rng.integers(len(bad) // 8, len(bad), 1 + trial % 4):
                bad[pos] ^= 1 << int(rng.integers(0, 8))
            if trial % 6 == 5:
                bad = bad[: int(rng.integers(len(bad) // 2, len(bad)))]
            try:
                meta, px = jx.decoder_builder().decode_with(bytes(bad), np.uint8)
                assert len(px) == meta.width * meta.height * (4 if meta.has_alpha_channel else 3)
                outcomes["decoded"] += 1
            except jx.DecodeError:
                outcomes["error"] += 1
    assert outcomes["error"] > 0 and sum(outcomes.values()) == 28
    for d, ref in (mixed, glob):
        meta, px = jx.decoder_builder().decode_with(d, np.uint8)
        _same(px, ref, "clean stream after the corrupted ones")
