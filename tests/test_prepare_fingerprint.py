"""What Batch::Prepare lays out, pinned as numbers: for each case a BatchDecoder is filled and prepared (nothing is decoded) and the sizes of its arenas and the
facts about its plan are compared with tests/golden/prepare_fingerprint.json.

  device_bytes   constant arena + work arena + coefficient and pixel planes: every table put into the constant arena and every buffer taken from the others
  stage_bytes    the algorithmic bytes per stage
  info_value     lf_simt_frames, lf_legacy_frames, lf_simt_lanes, lf_simt_waves, lf_simt_wp (the SIMT LF plan: eligible frames, lane packing, instantiation),
                 ac_code_bytes, ac_code_bytes_compact, mod_code_bytes, mod_group_lds_bytes (the LDS sizing)

Every stream is prepared twice: with the library's lane strides (LF 64: no SIMT plan) and with the throughput pipeline's (LF 8, HF 1: the SIMT plan is built).

The expected values were recorded with the build of the commit before Prepare was split into phases and are not to be regenerated from later code: they are what says
that a restructuring of Prepare changed no layout.  A case is added by running, on a GPU, with a build that is known to be right,

    python tests/test_prepare_fingerprint.py --record

which writes the file anew (review the diff: only the new case may appear).
"""
import functools
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FIXTURES = os.path.join(HERE, "fixtures")
EXPECTED = os.path.join(GOLDEN, "prepare_fingerprint.json")
INFOS = ("lf_simt_frames", "lf_legacy_frames", "lf_simt_lanes", "lf_simt_waves", "lf_simt_wp", "ac_code_bytes", "ac_code_bytes_compact", "mod_code_bytes", "mod_group_lds_bytes")
GOLDEN_STREAMS = sorted(f for f in os.listdir(GOLDEN) if f.endswith(".jxl"))
FIXTURE_STREAMS = ["sample.jxl", "sample_grey.jxl", "2bit.jxl", "sample_jpg.jxl"]
SEEDED = ["layered_modular_n2", "layered_vardct_n2", "patched_n2", "spot_layered_n4", "upsampled_n2"]
MIXED = ["vardct_300x200_mix2_epf2.jxl", "vardct2_520x300_ups2_default.jxl", "vardct_272x264_mix2_epf3.jxl"]
STRIDES = {"default": None, "simt": (8, 1)}


def _read(folder, name):
    with open(os.path.join(folder, name), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def stream(name):
    if name in GOLDEN_STREAMS:
        return _read(GOLDEN, name)
    if name in FIXTURE_STREAMS:
        return _read(FIXTURES, name)
    import test_many_extra_channels as M      # the 300 x 200 seeded streams of that module
    return {"layered_modular_n2": lambda: M.layered("modular", 2)[0], "layered_vardct_n2": lambda: M.layered("vardct", 2)[0], "patched_n2": lambda: M.patched(None, False, 2),
            "spot_layered_n4": lambda: M.spot_layered(None, 4), "upsampled_n2": lambda: M.upsampled(None, 2)[0]}[name]()


def fingerprint(b):
    out = {"device_bytes": int(b.device_bytes), "stage_bytes": b.stage_bytes}
    out.update({k: b.info_value(k) for k in INFOS})
    return out


def prepared(jx, names, strides=None, **spec):
    b = jx.BatchDecoder()
    if strides:
        b.set_lane_stride(*strides)
    for name in names:
        b.add(stream(name), **spec)
    b.prepare()
    return b


def _plain(name, strides):
    return lambda jx: fingerprint(prepared(jx, [name], STRIDES[strides]))


def _mixed_refilled(jx):
    """three VarDCT streams in one batch (quant tables shared between frames), then the same object reset, filled in another order and prepared again"""
    b = prepared(jx, MIXED, (8, 1))
    first = fingerprint(b)
    b.reset()
    for name in reversed(MIXED):
        b.add(stream(name))
    b.prepare()
    return {"first": first, "refilled": fingerprint(b)}


CASES = {}
for _name in GOLDEN_STREAMS + FIXTURE_STREAMS + SEEDED:
    for _s in STRIDES:
        CASES["%s-%s" % (_name, _s)] = _plain(_name, _s)
CASES["mixed_batch_refilled"] = _mixed_refilled
CASES["downscale8"] = lambda jx: fingerprint(prepared(jx, ["vardct_300x200_mix2_epf2.jxl"], (8, 1), downscale=8))
CASES["resize_37x23_crop"] = lambda jx: fingerprint(prepared(jx, ["vardct_300x200_mix2_epf2.jxl"], (8, 1), dtype="float32", num_channels=3, resize=(37, 23), crop=(11, 7, 200, 150)))
CASES["lf_stride_64_forced"] = lambda jx: fingerprint(prepared(jx, ["vardct_272x264_mix2_epf3.jxl"], (64, 1)))
CASES["one_group_prerun"] = lambda jx: fingerprint(prepared(jx, ["vardct_64x64_dct8.jxl"], (8, 1)))


@pytest.fixture(scope="module")
def jx(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import jpegxl_rs_amd as jx
    return jx


@pytest.fixture(scope="module")
def expected():
    with open(EXPECTED) as f:
        return json.load(f)


def test_every_case_has_a_recorded_fingerprint(expected):
    assert sorted(expected) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_prepare_fingerprint(jx, expected, case):
    got = CASES[case](jx)
    print(case, json.dumps(got, sort_keys=True))
    assert got == expected[case]


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import __graft_entry__ as g
    g.build()
    import jpegxl_rs_amd
    record = {case: CASES[case](jpegxl_rs_amd) for case in sorted(CASES)}
    with open(EXPECTED, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases in %s" % (len(record), EXPECTED))
