#!/usr/bin/env python3
"""Throughput of the lossless batch encoder (jx.LosslessEncoder, include/jxl_hip.h JxlHipEncoderEncodeLossless): `--images` frames of `--width` x `--height` RGB u8 that
already sit in device memory (the synthesiser's picture, rolled by a different offset per frame so that no two frames are equal), encoded in one call; `--warmup` calls,
then `--steps` timed ones.

Reported (one JSON line): Mpixel/s at the median call; ms per phase of the median call (upload, tokenise + histogram readback, host code build, count + scans + size
readback, pack, copy back, splice); bytes per frame against the synthesiser's prefix-coded Modular stream of frame 0 (same model class); the synthesiser's single-core
Mpixel/s on the same box, the only other encoder here.  `--check` decodes frame 0 with the CPU oracle and compares it with the source.
Kernel resources (VGPRs, scratch): tools/scripts/kernel_resources.sh."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.append(ROOT)
sys.path.append(os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import jpegxl_rs_amd as jx
    import synth_lib as S
    base = S.synthetic_image(3, a.width, a.height)
    S.set_prefix(True)
    try:
        t0 = time.perf_counter()
        ref = S.encode_modular(base, bits=8, rct=True)
        synth_s = time.perf_counter() - t0
    finally:
        S.set_prefix(False)
    dev = torch.from_numpy(base).cuda()
    frames = [dev] + [torch.roll(dev, shifts=(17 * k, 29 * k), dims=(0, 1)).contiguous() for k in range(1, a.images)]
    torch.cuda.synchronize()
    enc = jx.LosslessEncoder(0)
    calls = []
    for step in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        out = enc.encode(frames)
        dt = time.perf_counter() - t0
        if step >= a.warmup:
            calls.append((dt, enc.phase_times()))
    calls.sort(key=lambda c: c[0])
    dt, phases = calls[len(calls) // 2]
    mpix = a.images * a.width * a.height / 1e6
    res = {"images": a.images, "width": a.width, "height": a.height, "call_ms": round(dt * 1e3, 2), "mpixel_per_s": round(mpix / dt, 1),
           "phase_ms": {k: round(v, 2) for k, v in phases.items()}, "bytes_frame0": len(out[0]), "bytes_mean": int(np.mean([len(o) for o in out])),
           "share_of_raw_frame0": round(len(out[0]) / base.nbytes, 4), "synth_bytes_frame0": len(ref), "bytes_vs_synth": round(len(out[0]) / len(ref), 4),
           "synth_mpixel_per_s": round(a.width * a.height / 1e6 / synth_s, 2)}
    if a.check:
        import oracle_lib as O
        res["frame0_round_trip"] = bool(np.array_equal(O.decode(out[0]).image("u8"), base))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
