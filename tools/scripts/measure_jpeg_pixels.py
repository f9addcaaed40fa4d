#!/usr/bin/env python3
"""Milliseconds per batch and Mpixel/s of the ways from a batch of JPEG transcodes to the pixels of the original JPEG files.

Input: --files baseline JPEGs (--sampling 444 | 422 | 420 | grey, default 420) of --width x --height, written at run time by Pillow from tests/jpeg_cases.photo (--distinct different pictures, cycled) and
turned into JPEG XL by tests/jpeg_tools.transcode.  Output of the two device legs: u8 RGB in device memory (one caller-owned buffer per image).  Legs (--legs):

  pixels       BatchDecoder.decode_jpeg_pixels() of a prepared batch: the entropy stages, then the integer pixel path (csrc/jpeg_pixels.hip); the call waits for the result
  decode       decode() + finish() of the same prepared batch: libjxl's rendering through the float VarDCT pipeline — the pixel path these files had before
               decode_jpeg_pixels existed.  It runs nothing of the new interface: with PYTHONPATH pointing at a build of an earlier commit the same script measures that build
  reconstruct  what a user needs without the new call to get libjpeg's samples: reconstruct_jpegs(), the files fetched to the host, Pillow decoding them on --threads
               host threads (reported whole and in its two parts)
  pipeline     --jobs jobs of the same --files transcodes through Pipeline.submit(jpeg_pixels=True), all submitted before the first wait: the entropy stages of later jobs
               overlap the integer pixel path of earlier ones.  ms_per_batch is the wall time from the first submit to the last wait over --jobs; "stages_ms_per_job" are
               the pipeline's own HIP-event brackets (the `timed` option, JxlHipPipelineCollectTimes) per job: the largest of them is the step of the schedule
               --resize W,H: every image of the jobs comes out W x H (the triangle filter); --jpeg_scale 2 | 4 | 8: libjpeg's scaled decode (Pipeline.submit(jpeg_scale=)),
               the source of that resize.  With either, the pixels are not compared with Pillow here (tests/test_jpeg_scaled_pixels.py does); "pixel_half_ms_per_job" is
               idct_ms + out_ms of the brackets: integer IDCT, colour-out and the resizes
               --resize_u8 (with --resize): the resample in Pillow's 8-bit arithmetic over a u8 intermediate (Pipeline.submit(resize_u8=True)); the first image of the first
               job is compared with PIL's resize of the source file (after draft() for --jpeg_scale), byte for byte
               --prefix (with --jpeg_scale 8 and a sampling that is decoded from the DC terms alone: 444, 422, grey): every file is submitted cut at lf_part_size(),
               the bytes that hold the LF part of its frame; "submitted_bytes" / "file_bytes" say what a loader read and what the files hold.  "dc_only_images": images
               of the last job written by JpegDcOutKernel (a build without that path reports None)
  pipeline_float  the same jobs without jpeg_pixels: libjxl's rendering through the float tail — what a loader of these files gets from a Pipeline otherwise

Every leg runs --reps times after --warmup; the median is reported.  The first run of a leg is checked: pixels and reconstruct equal Pillow's decode of the source
file exactly, decode is reported with its largest difference from it.  Prints one JSON line.
--cache DIR keeps the input files and their transcodes (the parser of tests/jpeg_tools.py is plain Python and slow on large files) for the next run; --legs "" only fills it."""
import argparse
import io
import json
import os
import pickle
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.append(ROOT)                     # (behind PYTHONPATH: another build of the package may be measured with this script)
sys.path.append(os.path.join(ROOT, "tests"))


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--legs", default="pixels,decode,reconstruct")
    ap.add_argument("--cache", default=None)
    ap.add_argument("--jobs", type=int, default=6, help="pipeline legs: jobs per repetition")
    ap.add_argument("--resize", default=None, help="pipeline legs: W,H of every output")
    ap.add_argument("--jpeg_scale", type=int, default=1, help="pipeline leg: libjpeg's scaled decode (2, 4, 8)")
    ap.add_argument("--resize_u8", action="store_true", help="pipeline leg: the integer resample (needs --resize)")
    ap.add_argument("--sampling", default="420", choices=("444", "422", "420", "grey"), help="chroma sampling of the source files")
    ap.add_argument("--prefix", action="store_true", help="pipeline leg at --jpeg_scale 8: submit each file cut at lf_part_size()")
    args = ap.parse_args()
    import numpy as np
    from PIL import Image
    import jpeg_cases as JC
    import jpeg_tools as J
    tag = "" if args.sampling == "420" else "_" + args.sampling
    cached = args.cache and os.path.join(args.cache, "jpeg_pixels_%dx%d_q%d_n%d%s.pickle" % (args.width, args.height, args.quality, args.distinct, tag))
    if cached and os.path.exists(cached):
        with open(cached, "rb") as f:
            jpegs, jxls = pickle.load(f)
    else:
        jpegs = []
        for k in range(args.distinct):
            buf = io.BytesIO()
            img = JC.photo(args.width, args.height, seed=100 + k)
            if args.sampling == "grey":
                Image.fromarray(np.ascontiguousarray(img[:, :, 0])).save(buf, "JPEG", quality=args.quality)
            else:
                Image.fromarray(img).save(buf, "JPEG", quality=args.quality, subsampling={"444": 0, "422": 1, "420": 2}[args.sampling])
            jpegs.append(buf.getvalue())
        jxls = [J.transcode(d) for d in jpegs]
        if cached:
            os.makedirs(args.cache, exist_ok=True)
            with open(cached, "wb") as f:
                pickle.dump((jpegs, jxls), f)
    legs = [leg for leg in args.legs.split(",") if leg]
    if not legs:
        return
    import torch
    import jpegxl_rs_amd as jx
    files = [jpegs[k % args.distinct] for k in range(args.files)]
    inputs = [jxls[k % args.distinct] for k in range(args.files)]
    w, h = args.width, args.height
    mpix = args.files * w * h / 1e6
    want = [np.asarray(Image.open(io.BytesIO(d)).convert("RGB")) for d in jpegs]
    out = {"what": "pixels of JPEG transcodes, u8 RGB", "files": args.files, "distinct": args.distinct, "size": [w, h], "quality": args.quality, "megapixels": round(mpix, 1), "sampling": args.sampling,
           "jpeg_bytes": sum(len(f) for f in files), "package": os.path.dirname(os.path.abspath(jx.__file__))}

    def report(times):
        ms = median(times[args.warmup:])
        return {"ms_per_batch": round(ms, 2), "mpixel_per_s": round(mpix / ms * 1e3, 1), "ms_min": round(min(times[args.warmup:]), 2)}

    def prepared_batch():
        b = jx.BatchDecoder(0)
        bufs = [torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda:0") for _ in inputs]
        for d, t in zip(inputs, bufs):
            b.add(d, num_channels=3, device_ptr=t.data_ptr())
        b.prepare()
        return b, bufs

    for leg in legs:
        times = []
        if leg in ("pixels", "decode"):
            b, bufs = prepared_batch()
            if leg == "pixels" and not hasattr(b, "decode_jpeg_pixels"):
                out[leg] = "this build has no decode_jpeg_pixels"
                continue
            for r in range(args.warmup + args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if leg == "pixels":
                    errs = b.decode_jpeg_pixels()
                else:
                    b.decode(); b.finish()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
                if r == 0:
                    got = [bufs[k].cpu().numpy().reshape(h, w, 3) for k in range(args.distinct)]
                    diff = max(int(np.abs(g.astype(int) - x.astype(int)).max()) for g, x in zip(got, want))
                    if leg == "pixels":
                        assert errs == [None] * len(inputs), errs
                        assert diff == 0, "pixels differ from Pillow's decode of the source files"
            out[leg] = report(times)
            out[leg]["max_difference_from_pillow"] = diff
            if leg == "pixels":
                out[leg]["pixel_launches"] = b.info_value("jpeg_pixel_launches")
            del b, bufs
        elif leg in ("pipeline", "pipeline_float"):
            exact = leg == "pipeline"
            if exact and "jpeg_pixels" not in jx.Pipeline.submit.__code__.co_varnames:
                out[leg] = "this build has no Pipeline.submit(jpeg_pixels=True)"
                continue
            p = jx.Pipeline(0, timed=1, reserve_frames=args.files, reserve_width=w, reserve_height=h)
            resize = tuple(int(v) for v in args.resize.split(",")) if args.resize else None
            scaled = exact and args.jpeg_scale != 1
            if scaled and "jpeg_scale" not in jx.Pipeline.submit.__code__.co_varnames:
                out[leg] = "this build has no Pipeline.submit(jpeg_scale=)"
                p.close()
                continue
            ow, oh = resize if resize else (-(-w // args.jpeg_scale), -(-h // args.jpeg_scale)) if scaled else (w, h)
            bufs = [[torch.zeros(ow * oh * 3, dtype=torch.uint8, device="cuda:0") for _ in inputs] for _ in range(min(args.jobs, 3))]
            kw = dict(jpeg_pixels=True) if exact else {}
            if resize:
                kw["resize"] = resize
            if scaled:
                kw["jpeg_scale"] = args.jpeg_scale
            u8 = exact and args.resize_u8
            if u8 and (not resize or "resize_u8" not in jx.Pipeline.submit.__code__.co_varnames):
                out[leg] = "--resize_u8 needs --resize and a build with Pipeline.submit(resize_u8=)"
                p.close()
                continue
            if u8:
                kw["resize_u8"] = True
            submitted = inputs
            if exact and args.prefix:
                if args.jpeg_scale != 8 or not hasattr(jx, "lf_part_size"):
                    out[leg] = "--prefix needs --jpeg_scale 8 and a build with lf_part_size()"
                    p.close()
                    continue
                submitted = [d[:jx.lf_part_size(d)] for d in inputs]
            stages = None
            for r in range(args.warmup + args.reps):
                if r == args.warmup:
                    p.collect_times()                      # (the brackets of the warm-up jobs are dropped)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tickets = [p.submit(submitted, "uint8", 3, device_ptrs=[t.data_ptr() for t in bufs[k % len(bufs)]], **kw) for k in range(args.jobs)]
                for t in tickets:
                    st, _ = p.wait(t)
                    assert st == [0] * len(inputs), st
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3 / args.jobs)
                if r == 0 and u8:
                    im = Image.open(io.BytesIO(files[0]))
                    if scaled:
                        im.draft(im.mode, (w // args.jpeg_scale, h // args.jpeg_scale))
                    ref = np.asarray(im.resize(resize, Image.BILINEAR).convert("RGB"))
                    diff = int(np.abs(bufs[0][0].cpu().numpy().reshape(ref.shape).astype(int) - ref).max())
                    assert diff == 0, "the integer resample differs from PIL's resize of the source file"
                elif r == 0 and (resize or scaled):
                    diff = None
                elif r == 0:
                    got = [bufs[0][k].cpu().numpy().reshape(h, w, 3) for k in range(args.distinct)]
                    diff = max(int(np.abs(g.astype(int) - x.astype(int)).max()) for g, x in zip(got, want))
                    assert not exact or diff == 0, "pixels differ from Pillow's decode of the source files"
            st, runs = p.collect_times()
            stages = {k: round(v / max(runs, 1), 2) for k, v in st.items()}
            out[leg] = report(times)
            out[leg].update(jobs_per_rep=args.jobs, max_difference_from_pillow=diff, stages_ms_per_job=stages, timed_jobs=runs, private_plane_jobs=p.info("private_plane_jobs"))
            out[leg].update(output_size=[ow, oh], device_bytes=p.info("device_bytes"), pixel_half_ms_per_job=round(stages.get("idct_ms", 0) + stages.get("out_ms", 0), 3))
            if exact:
                out[leg].update(pixel_launches=p.info("jpeg_pixel_launches"), jpeg_scale=args.jpeg_scale, resize_u8=bool(u8))
                dc = p.info("jpeg_dc_only_images")
                out[leg].update(dc_only_images=dc if dc >= 0 else None, hf_nonzeros=p.info("hf_nonzeros"), prefix=bool(args.prefix), submitted_bytes=sum(len(d) for d in submitted),
                                file_bytes=sum(len(d) for d in inputs))
            p.close()
            del p, bufs
        elif leg == "reconstruct":
            parts = []
            pool = ThreadPoolExecutor(args.threads)
            for r in range(args.warmup + args.reps):
                b = jx.BatchDecoder(0)
                for d in inputs:
                    b.add(d)
                t0 = time.perf_counter()
                b.reconstruct_jpegs()
                got = [b.jpeg(i) for i in range(len(inputs))]
                t1 = time.perf_counter()
                px = list(pool.map(lambda d: np.asarray(Image.open(io.BytesIO(d))), got))
                t2 = time.perf_counter()
                times.append((t2 - t0) * 1e3)
                parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
                if r == 0:
                    assert got == files, "bytes differ from the source files"
                    assert all(np.array_equal(px[k], want[k]) for k in range(args.distinct))
                del b
            pool.shutdown()
            out[leg] = report(times)
            out[leg]["reconstruct_ms"] = round(median([p[0] for p in parts[args.warmup:]]), 2)
            out[leg]["host_decode_ms"] = round(median([p[1] for p in parts[args.warmup:]]), 2)
            out[leg]["host_threads"] = args.threads
        else:
            raise SystemExit("unknown leg " + leg)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
