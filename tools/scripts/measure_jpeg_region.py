#!/usr/bin/env python3
"""Same-box A/B of Pipeline.set_option("jpeg_region", 0 | 1): libjpeg-exact jobs of RandomResizedCrop crops with every group decoded, and with only the groups a crop needs.

Input: --files transcodes of --width x --height 4:2:0 JPEGs written at run time by Pillow from tests/jpeg_cases.photo (--distinct different pictures, cycled; quality
--quality), turned into JPEG XL by tests/jpeg_tools.transcode.  Every image of a job has its own crop, drawn as torchvision's RandomResizedCrop draws it — area fraction
uniform in [0.08, 1] (--area), aspect ratio log-uniform in [3/4, 4/3], ten tries, then the central crop — from numpy's default_rng(--seed); the target is --target x --target,
u8 RGB, resize_u8, bilinear, into device memory.  The crops are the same for both settings.

One pipeline (timed), the option toggled between runs: a run is --jobs jobs submitted before the first wait.  --pairs pairs of (off, on) after one warm-up pair; per run
one JSON line {"region", "ms_per_job", "images_per_s", "stage_ms" (the pipeline's HIP-event brackets per job), "hf_groups_decoded", "hf_groups_total"}, then a summary
line with the range of every figure over the pairs and the mean share of groups decoded.  The first job of the first pair is compared between the settings, byte for byte.
--cache DIR keeps the transcodes (the parser of tests/jpeg_tools.py is plain Python and slow on large files); --fill-cache only writes them."""
import argparse
import json
import math
import os
import pickle
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.append(ROOT)
sys.path.append(os.path.join(ROOT, "tests"))


def random_resized_crop(rng, w, h, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """torchvision.transforms.RandomResizedCrop.get_params -> (x0, y0, cw, ch)"""
    area = w * h
    for _ in range(10):
        target = area * rng.uniform(scale[0], scale[1])
        aspect = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
        cw, ch = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
        if 0 < cw <= w and 0 < ch <= h:
            return int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch
    r = w / h
    if r < ratio[0]:
        cw, ch = w, int(round(w / ratio[0]))
    elif r > ratio[1]:
        cw, ch = int(round(h * ratio[1])), h
    else:
        cw, ch = w, h
    return (w - cw) // 2, (h - ch) // 2, cw, ch


def transcodes(a):
    import io
    from PIL import Image
    import jpeg_cases as JC
    import jpeg_tools as J
    path = os.path.join(a.cache, "region_%dx%d_q%d_%d.pkl" % (a.width, a.height, a.quality, a.distinct)) if a.cache else None
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    out = []
    for k in range(a.distinct):
        buf = io.BytesIO()
        Image.fromarray(JC.photo(a.width, a.height, seed=500 + k)).save(buf, "JPEG", quality=a.quality, subsampling=2)
        out.append(J.transcode(buf.getvalue()))
    if path:
        os.makedirs(a.cache, exist_ok=True)
        with open(path, "wb") as f:
            pickle.dump(out, f)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--height", type=int, default=1536)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--target", type=int, default=224)
    ap.add_argument("--jobs", type=int, default=6)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--area", default="0.08,1", help="range of the crops' area fraction (RandomResizedCrop's scale)")
    ap.add_argument("--cache", default=None)
    ap.add_argument("--fill-cache", action="store_true")
    a = ap.parse_args()
    pool = transcodes(a)
    if a.fill_cache:
        return
    import numpy as np
    import torch
    import jpegxl_rs_amd as jx
    rng = np.random.default_rng(a.seed)
    datas = [pool[k % len(pool)] for k in range(a.files)]
    area = tuple(float(v) for v in a.area.split(","))
    crops = [[random_resized_crop(rng, a.width, a.height, scale=area) for _ in range(a.files)] for _ in range(a.jobs)]
    one = a.target * a.target * 3
    outs = [torch.zeros((a.files, one), dtype=torch.uint8, device="cuda:0") for _ in range(a.jobs)]
    p = jx.Pipeline(0, jobs_in_flight=3, timed=True)
    first = {}

    def run(on):
        p.set_option("jpeg_region", on)
        p.collect_times()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tickets = [p.submit(datas, "uint8", 3, device_ptrs=[outs[j][k].data_ptr() for k in range(a.files)], capacities=[one] * a.files, jpeg_pixels=True, resize_u8=True,
                            resize=(a.target, a.target), crop=crops[j], filter="bilinear") for j in range(a.jobs)]
        for t in tickets:
            st, _ = p.wait(t)
            assert st == [0] * a.files
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        times, runs = p.collect_times()
        if on not in first:
            first[on] = outs[0].cpu().numpy().copy()
        return {"region": on, "ms_per_job": round(wall * 1e3 / a.jobs, 3), "images_per_s": round(a.files * a.jobs / wall, 1),
                "stage_ms": {k.replace("_ms", ""): round(v / max(runs, 1), 3) for k, v in times.items()},
                "hf_groups_decoded": p.info("hf_groups_decoded"), "hf_groups_total": p.info("hf_groups_total")}

    try:
        run(0); run(1)                                            # warm-up pair
        assert np.array_equal(first[0], first[1]), "the option changed the bytes"
        lines = []
        for _ in range(a.pairs):
            for on in (0, 1):
                lines.append(run(on))
                print(json.dumps(lines[-1]), flush=True)
    finally:
        p.close()
    # (hf_groups_* of a line are those of the job prepared last; the mean share over all jobs of a run is asked of a host-only batch: BatchDecoder.jpeg_region)
    cdiv = lambda x, y: -(-x // y)
    per_image = cdiv(cdiv(a.width, 16) * 2, 32) * cdiv(cdiv(a.height, 16) * 2, 32)
    host = jx.BatchDecoder(-1)
    decoded = 0
    for j in range(a.jobs):
        for d, c in zip(datas, crops[j]):
            g = host.jpeg_region(host.add(d, num_channels=3, resize=(a.target, a.target), crop=c, resize_u8=True))
            decoded += per_image if g is None else (g[2] - g[0]) * (g[3] - g[1])
    summary = {"width": a.width, "height": a.height, "files": a.files, "jobs": a.jobs, "pairs": a.pairs, "target": a.target, "area": a.area, "groups_per_image": per_image,
               "mean_groups_share": round(decoded / (per_image * a.files * a.jobs), 4)}
    for on in (0, 1):
        sel = [x for x in lines if x["region"] == on]
        tag = "on" if on else "off"
        summary[tag] = {"images_per_s": [min(x["images_per_s"] for x in sel), max(x["images_per_s"] for x in sel)],
                        **{k: [min(x["stage_ms"][k] for x in sel), max(x["stage_ms"][k] for x in sel)] for k in ("hf", "idct", "out")},
                        "groups_share_last_job": round(sel[-1]["hf_groups_decoded"] / max(1, sel[-1]["hf_groups_total"]), 4)}
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
