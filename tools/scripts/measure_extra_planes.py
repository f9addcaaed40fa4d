#!/usr/bin/env python3
"""The price of extra-channel planes on the batch path: one simple (single-frame, no features) RGB image with four lossless extra channels, decoded

  fused   without planes: three-channel planar f16, the fused tile kernels of simple images,
  planes  as one [3 + 4, H, W] planar f16 block (BatchDecoder.add extra_planes=[0, 1, 2, 3]): the image takes the frame tail, EcPlanesOutKernel writes the four planes,

each prepared once and decoded --decodes times behind --warmup decodes: a host clock around decode() + finish(), which ends in a device synchronise.  The legs alternate,
decode by decode, so that what else the machine does falls on all of them alike.  Prints one JSON line: the median, the minimum and max - min per leg in ms, and the
bytes of each destination.  Needs a GPU; it does not fall back."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.append(ROOT)
sys.path.append(os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--kind", default="vardct", choices=("vardct", "modular"))
    ap.add_argument("--decodes", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    import jpegxl_rs_amd as jx
    import synth_lib as S
    import synth_extra as X
    w, h = (int(v) for v in args.size.split("x"))
    extras = [X.extra(type=X.DEPTH if k else X.ALPHA, bits=8) for k in range(4)]
    planes = [X.plane(50 + k, w, h, 8) for k in range(4)]
    img = S.synthetic_image(9, w, h)
    data = X.encode_vardct_ec(img, planes, extras, S.frame(), seed=4) if args.kind == "vardct" else X.encode_modular_ec(img.astype(np.int32), planes, extras, S.frame())
    fmt = dict(dtype="float16", num_channels=3, planar=True)
    legs = {"fused": dict(fmt), "planes": dict(fmt, extra_planes=[0, 1, 2, 3])}
    batches, bufs, sizes = {}, {}, {}
    for name, kw in legs.items():
        b = jx.BatchDecoder(0)
        sizes[name] = jx.image_out_size(data, **kw)[1]
        bufs[name] = torch.empty(sizes[name], dtype=torch.uint8, device="cuda:0")
        b.add(data, device_ptr=bufs[name].data_ptr(), **kw)
        b.prepare()
        batches[name] = b
    times = {name: [] for name in legs}
    for k in range(args.warmup + args.decodes):
        for name, b in batches.items():
            t0 = time.perf_counter()
            b.decode(); b.finish()
            if k >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    # the colour planes of the two legs hold the same picture to within the last bit (fused tile kernels against the frame tail: test_extra_planes.py pins both against the oracle)
    a = bufs["fused"][:3 * w * h * 2].cpu().numpy().view(np.float16).astype(np.float32)
    c = bufs["planes"][:3 * w * h * 2].cpu().numpy().view(np.float16).astype(np.float32)
    res = {"what": "batch decode of one %s %dx%d RGB + 4 extra channels, planar f16" % (args.kind, w, h), "stream_bytes": len(data), "decodes": args.decodes,
           "plane_outputs": batches["planes"].info_value("plane_outputs"), "colour_max_abs_diff": float(np.abs(a - c).max()), "out_bytes": sizes,
           "ms": {name: {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "spread": round(max(t) - min(t), 3)} for name, t in times.items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
