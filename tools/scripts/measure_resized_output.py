#!/usr/bin/env python3
"""Step time of the throughput pipeline with resized output (JxlHipPipelineSubmitResized) beside what a consumer does without it, on the frames of bench.py's headline
(3840x2160, distance 1, gaborish + one EPF pass; `--distinct` seeded frames cycled to fill jobs of `--batch`).  One jx.Pipeline per leg at the same jobs_in_flight,
--warmup jobs, then --steps jobs; the step is the distance between the end times (GPU clock, JxlHipPipelineWait end_ms) of consecutive jobs; reported: median, 10th /
90th percentile, frames/s at the median, the pipeline's device_bytes.

  interleaved     u8 RGB at full size, [N, H, W, 3] — the decode alone
  resized         float16 planes of --target x --target pixels with a per-channel scale and bias, [N, 3, T, T] = (resize(v) - mean) / std, straight from the decode
  resampled       the resized leg with what a training input pipeline asks of every image (JxlHipPipelineSubmitResampled): a random-resized-crop rectangle of its own (area
                  0.08 - 1 of the picture, aspect ratio 3/4 - 4/3, log-uniform; seed 7), the bicubic filter, and a mirror on every second image
  consumer        what a consumer of that tensor does without the resize: the interleaved leg, plus — for every job, on a stream of the consumer's own, as soon as the job has
                  left the pipeline — torch's interpolate(mode="bilinear", antialias=True) of the job's output (permuted to [N, 3, H, W], float16) to the target, then scale and
                  bias.  The step is the distance between the ends of that second pass (torch events), which is when the consumer has its tensor.

Prints one JSON line."""
import argparse
import json
import math
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.append(ROOT)                     # (behind PYTHONPATH: another build of the package may be measured with this script)
sys.path.append(os.path.join(ROOT, "tests"))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def percentile(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def random_resized_crop(rng, W, H):
    """torchvision's RandomResizedCrop.get_params: area 0.08 - 1 of the picture, log-uniform aspect ratio 3/4 - 4/3, ten tries, else the whole picture"""
    for _ in range(10):
        area = W * H * rng.uniform(0.08, 1.0)
        ratio = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
        w, h = int(round(math.sqrt(area * ratio))), int(round(math.sqrt(area / ratio)))
        if 0 < w <= W and 0 < h <= H:
            return (rng.randint(0, W - w), rng.randint(0, H - h), w, h)
    return (0, 0, W, H)


def leg(jx, torch, streams, name, batch, steps, warmup, in_flight, W, H, T, chunk):
    # (the f32 picture a resized output is filtered from lives among the pixel planes the jobs of a pipeline share: leg `resized` reserves a second set and a margin for the
    # horizontally filtered rows, so that no job falls back to planes of its own)
    reserve = dict(reserve_frames=batch + (batch + 7) // 8, reserve_plane_sets=2) if name in ("resized", "resampled") else dict(reserve_frames=batch)
    p = jx.Pipeline(0, jobs_in_flight=in_flight, lf_streams=in_flight, reserve_width=W, reserve_height=H, **reserve)
    lag = max(0, p.info("slots") - 2)
    nbuf = 2                                        # (destinations rotate over two buffers, as in measure_planar_output.py)
    scale_l, bias_l = [1.0 / s for s in STD], [-m / s for m, s in zip(MEAN, STD)]
    rng = random.Random(7)
    if name in ("resized", "resampled"):
        dtype, shape, tdtype = "float16", (batch, 3, T, T), torch.float16
        extra = dict(planar=True, scale=scale_l, bias=bias_l, resize=(T, T))
    else:
        dtype, shape, tdtype, extra = "uint8", (batch, H, W, 3), torch.uint8, {}
    outs = [torch.empty(shape, dtype=tdtype, device="cuda:0") for _ in range(nbuf)]
    frame_bytes = outs[0][0].numel() * outs[0].element_size()
    consumer = name == "consumer"
    if consumer:
        side = torch.cuda.Stream(device="cuda:0")
        dst = [torch.empty((batch, 3, T, T), dtype=torch.float16, device="cuda:0") for _ in range(2)]
        scale = torch.tensor(scale_l, dtype=torch.float16, device="cuda:0").view(1, 3, 1, 1)
        bias = torch.tensor(bias_l, dtype=torch.float16, device="cuda:0").view(1, 3, 1, 1)
        first_event = torch.cuda.Event(enable_timing=True)
        events = []

    def second_pass(k):
        # (the pipeline has written the job: wait() returned; the pass runs beside the decode of the jobs behind it, `chunk` images at a time so that the float16 copy
        # of the full-size pictures stays small)
        with torch.cuda.stream(side):
            if not events:
                first_event.record(side)
            d = dst[k % 2]
            src = outs[k % nbuf]
            for i in range(0, batch, chunk):
                x = src[i:i + chunk].permute(0, 3, 1, 2).to(torch.float16)
                y = torch.nn.functional.interpolate(x, size=(T, T), mode="bilinear", antialias=True, align_corners=False)
                torch.mul(y, scale / 255.0, out=d[i:i + chunk])
            d.add_(bias)
            e = torch.cuda.Event(enable_timing=True)
            e.record(side)
            events.append(e)

    def run(njobs):
        p.reset_clock()
        tickets, ends = [], []
        for k in range(njobs):
            off = (k * 37) % len(streams)
            frames = [streams[(off + i) % len(streams)] for i in range(batch)]
            base = outs[k % nbuf].data_ptr()
            own = {}
            if name == "resampled":
                own = dict(crop=[random_resized_crop(rng, W, H) for _ in range(batch)], filter="bicubic", mirror=[i % 2 == 1 for i in range(batch)])
            tickets.append(p.submit(frames, dtype, 3, device_ptrs=[base + i * frame_bytes for i in range(batch)], **extra, **own))
            if k >= lag:
                ends.append(p.wait(tickets[k - lag])[1])
                if consumer:
                    second_pass(k - lag)
        for k in range(max(0, njobs - lag), njobs):
            ends.append(p.wait(tickets[k])[1])
            if consumer:
                second_pass(k)
        return ends

    t0 = time.perf_counter()
    ends = run(warmup + steps + 1)
    if consumer:
        torch.cuda.synchronize()
        ends = [first_event.elapsed_time(e) for e in events]
    wall = time.perf_counter() - t0
    gaps = [b - a for a, b in zip(ends[warmup:], ends[warmup + 1:])]
    med = percentile(gaps, 0.5)
    res = {"step_ms_median": round(med, 2), "step_ms_p10": round(percentile(gaps, 0.1), 2), "step_ms_p90": round(percentile(gaps, 0.9), 2), "steps": len(gaps),
           "frames_per_s": round(batch / med * 1e3, 1), "gpixel_per_s": round(batch * W * H / med / 1e6, 2), "output_bytes_per_job": int(batch * frame_bytes),
           "device_bytes": int(p.info("device_bytes")), "private_plane_jobs": int(p.info("private_plane_jobs")), "wall_s": round(wall, 2)}
    p.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--in-flight", type=int, default=11)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--target", type=int, default=224)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--legs", default="interleaved,resized,consumer")
    args = ap.parse_args()
    import torch
    import bench
    import jpegxl_rs_amd as jx
    streams = bench.make_streams(args.distinct, args.width, args.height, 1)
    out = {"what": "resized planar float16 output beside the interleaved decode and a consumer's interpolate pass", "frames_per_job": args.batch, "distinct": args.distinct,
           "size": [args.width, args.height], "target": args.target, "jobs_in_flight": args.in_flight, "package": os.path.dirname(os.path.abspath(jx.__file__))}
    for name in args.legs.split(","):
        out[name] = leg(jx, torch, streams, name, args.batch, args.steps, args.warmup, args.in_flight, args.width, args.height, args.target, args.chunk)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
