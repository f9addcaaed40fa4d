"""What Batch::PlanPostOps records for the frame tail of multi-frame and feature images, pinned as numbers: for each case a BatchDecoder is filled and prepared (nothing is
decoded) and two facts about its plan are compared with tests/golden/frame_tail_plan.json.

  post_ops        the number of recorded ops (one kernel launch or copy each), those of the batch that decodes the image's LF frames included
  post_ops_hash   FNV-1a, 63 bits, over the names of their stages in order ("chroma upsampling", "int to float", "patches", "splines", "upsampling", "noise",
                  "LF-frame hand-over", "colour transform", "own-frame output", "blending", "delivery"), each with its terminating zero; the ops of the LF frames' batch come first

The expected values were recorded with the build of the commit before the frame tail was split into stage functions, with nothing added to it but the names beside the
recorded ops (and the two testing options this file sets), and are not to be regenerated from later code: they are what says that a restructuring of the frame tail
plans the same ops in the same order.  A case is added by running, on a GPU, with a build that is known to be right,

    python tests/test_frame_tail_plan.py --record

which writes the file anew (review the diff: only the new case may appear).
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EXPECTED = os.path.join(HERE, "golden", "frame_tail_plan.json")
SEEDED = ["layered_modular_n2", "layered_vardct_n2", "patched_n2", "spot_layered_n4", "upsampled_n2"]


def _seeded(name):
    from test_prepare_fingerprint import stream
    return stream(name)


def _animation():
    """the three-frame animation of test_many_extra_channels.test_animation_decoded_once_every_canvas"""
    import synth_lib as S
    import test_many_extra_channels as M
    S.set_animation(10, 1, 0)
    try:
        M.layered.cache_clear()
        return M.layered("modular", 6, frames=3)[0]
    finally:
        S.set_animation()
        M.layered.cache_clear()


def _noise():
    """the strong-noise stream of test_synth_roundtrip.test_vardct_layers_and_noise"""
    import synth_lib as S
    return S.encode_vardct_frame(S.synthetic_image(5, 200, 136), S.frame(noise_lut=[120] * 8), seed=3)


def _lf_frame():
    import test_many_extra_channels as M
    return M.lf_frame_image(None)


def _splines():
    with open(os.path.join(HERE, "fixtures", "2bit.jxl"), "rb") as f:
        return f.read()


# case -> (the stream, batch options set before it is added)
CASES = {name: (lambda name=name: _seeded(name), {}) for name in SEEDED}
CASES["layered_vardct_n2_frame1_not_coalesced"] = (lambda: _seeded("layered_vardct_n2"), {"output_only_frame": 1})
CASES["animation_every_frame"] = (_animation, {"output_all_frames": 1})
CASES["splines_2bit"] = (_splines, {})
CASES["noise"] = (_noise, {})
CASES["lf_frame"] = (_lf_frame, {})


def plan_of(jx, case):
    make, options = CASES[case]
    b = jx.BatchDecoder()
    for k, v in options.items():
        b.set_option(k, v)
    b.add(make())
    b.prepare()
    return {"post_ops": b.info_value("post_ops"), "post_ops_hash": b.info_value("post_ops_hash")}


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


def test_every_case_has_a_recorded_plan(expected):
    assert sorted(expected) == sorted(CASES)
    assert all(e["post_ops"] > 0 for e in expected.values())


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_frame_tail_plan(jx, expected, case):
    got = plan_of(jx, case)
    print(case, json.dumps(got, sort_keys=True))
    assert got == expected[case]


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import __graft_entry__ as g
    g.build()
    import jpegxl_rs_amd
    record = {case: plan_of(jpegxl_rs_amd, case) for case in sorted(CASES)}
    with open(EXPECTED, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases in %s" % (len(record), EXPECTED))
