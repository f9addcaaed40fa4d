#!/usr/bin/env python3
"""Throughput, latency and device memory of the 1:8 decode (JxlHipPipelineSubmitScaled / JxlHipBatchSetOutputScaled) beside the full decode, on the frames of
bench.py's headline (3840x2160, distance 1, gaborish + one EPF pass; `--distinct` seeded frames cycled to fill jobs of `--batch`).

  pipeline legs   a scaled and an unscaled jx.Pipeline at the same jobs_in_flight: --warmup jobs, then --steps jobs; the step is the distance between the end times
                  (GPU clock, JxlHipPipelineWait end_ms) of consecutive jobs; reported: median, 10th / 90th percentile, frames/s at the median, device_bytes
  single image    one frame through a BatchDecoder (add, prepare, decode, finish, pixels to the host), median of --reps, scaled against unscaled

Prints one JSON line.  --legs unscaled runs nothing of the new interface: with PYTHONPATH pointing at another build of the package the same script measures that
build (the unscaled numbers of two commits on one machine)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.append(ROOT)                     # (behind PYTHONPATH: another build of the package may be measured with this script)
sys.path.append(os.path.join(ROOT, "tests"))


def percentile(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def pipeline_leg(jx, torch, streams, batch, steps, warmup, in_flight, W, H, downscale):
    ow, oh = (-(-W // 8), -(-H // 8)) if downscale == 8 else (W, H)
    frame_bytes = ow * oh * 3
    kw = {} if downscale == 8 else dict(reserve_frames=batch, reserve_width=W, reserve_height=H)
    p = jx.Pipeline(0, jobs_in_flight=in_flight, lf_streams=in_flight, **kw)
    outs = [torch.empty((batch, oh, ow, 3), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    lag = max(0, p.info("slots") - 2)
    extra = dict(downscale=8) if downscale == 8 else {}

    def run(njobs, first):
        p.reset_clock()
        tickets, ends = [], []
        for k in range(njobs):
            off = ((first + k) * 37) % len(streams)
            frames = [streams[(off + i) % len(streams)] for i in range(batch)]
            base = outs[k % 2].data_ptr()
            tickets.append(p.submit(frames, "uint8", 3, device_ptrs=[base + i * frame_bytes for i in range(batch)], **extra))
            if k >= lag:
                ends.append(p.wait(tickets[k - lag])[1])
        for k in range(max(0, njobs - lag), njobs):
            ends.append(p.wait(tickets[k])[1])
        return ends

    t0 = time.perf_counter()
    ends = run(warmup + steps + 1, 0)
    wall = time.perf_counter() - t0
    gaps = [b - a for a, b in zip(ends[warmup:], ends[warmup + 1:])]
    med = percentile(gaps, 0.5)
    res = {"step_ms_median": round(med, 2), "step_ms_p10": round(percentile(gaps, 0.1), 2), "step_ms_p90": round(percentile(gaps, 0.9), 2), "steps": len(gaps),
           "frames_per_s": round(batch / med * 1e3, 1), "device_bytes": int(p.info("device_bytes")), "wall_s": round(wall, 2), "first_job_end_ms": round(ends[0], 1)}
    p.close()
    return res


def single_leg(jx, data, reps, downscale):
    extra = dict(downscale=8) if downscale == 8 else {}
    times = []
    for _ in range(reps + 2):
        t0 = time.perf_counter()
        b = jx.BatchDecoder(0)
        b.add(data, "uint8", 3, **extra)
        b.prepare(); b.decode(); b.finish()
        px = b.output(0)
        times.append((time.perf_counter() - t0) * 1e3)
        dev = int(b.device_bytes)
        del b
    times = times[2:]
    return {"ms_median": round(percentile(times, 0.5), 2), "ms_min": round(min(times), 2), "ms_max": round(max(times), 2), "device_bytes": dev, "output_bytes": int(px.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--in-flight", type=int, default=11)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--legs", default="unscaled,scaled")
    args = ap.parse_args()
    import torch
    import bench
    import jpegxl_rs_amd as jx
    streams = bench.make_streams(args.distinct, args.width, args.height, 1)
    out = {"what": "1:8 decode beside the full decode", "frames_per_job": args.batch, "distinct": args.distinct, "size": [args.width, args.height], "jobs_in_flight": args.in_flight,
           "package": os.path.dirname(os.path.abspath(jx.__file__))}
    for leg in args.legs.split(","):
        ds = 8 if leg == "scaled" else 1
        out["pipeline_" + leg] = pipeline_leg(jx, torch, streams, args.batch, args.steps, args.warmup, args.in_flight, args.width, args.height, ds)
        out["single_" + leg] = single_leg(jx, streams[0], args.reps, ds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
