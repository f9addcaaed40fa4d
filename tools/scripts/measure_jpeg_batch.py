#!/usr/bin/env python3
"""Files per second of JPEG reconstruction: the batch call with the device writer, the same call with the host writer, and a loop of single reconstruct() calls.

Input: --files baseline 4:2:0 JPEGs of --width x --height, written at run time by Pillow from tests/jpeg_cases.photo (--distinct different pictures, cycled) and
turned into JPEG XL by tests/jpeg_tools.transcode.  Legs (--legs, comma separated):

  device   BatchDecoder.reconstruct_jpegs(): one entropy run, sequential scans entropy-coded on the GPU (progressive files: on the host)
  device_progressive   reconstruct_jpegs(progressive_on_device=True), i.e. JxlHipBatchSetOption("jpeg_device_progressive", 1): progressive scans entropy-coded on the GPU as well
  host     the same call with JxlHipBatchSetOption("jpeg_host_writer", 1): one entropy run, every file Huffman-coded on one host thread
  single   decoder_builder().reconstruct() file by file
  pipeline the same files as reconstruction jobs of --job-files (16) through one Pipeline with its default options (Pipeline.submit_jpegs), all submitted, then waited
           for in order: the pack pass, the copies and the host splice of job k run beside the entropy stages of the jobs behind it.  It is judged against leg `device`
           of a build of the parent commit (PYTHONPATH, --legs device) on the same machine in the same call.

Every leg adds the files to its decoder, reconstructs and fetches the bytes, --reps times after --warmup; the median is reported as ms per batch and files/s, and
the bytes are compared with the source files once.  Prints one JSON line.  --legs single runs nothing of the batch interface: with PYTHONPATH pointing at a build
of an earlier commit the same script measures that build — the baseline the batch call is judged against.

--progressive: the input files are progressive (Pillow's default scan script: ten scans, spectral selection and successive approximation).  The baseline of the
device_progressive leg is the device leg of the parent build (PYTHONPATH, --legs device), whose batch call codes these files on the host.
--cache DIR keeps the input files and their transcodes (the parser of tests/jpeg_tools.py is plain Python and slow on large files) for the next run."""
import argparse
import io
import json
import os
import pickle
import sys
import time

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
    ap.add_argument("--legs", default="device,host,single")
    ap.add_argument("--progressive", action="store_true")
    ap.add_argument("--cache", default=None)
    ap.add_argument("--job-files", type=int, default=16)
    args = ap.parse_args()
    from PIL import Image
    import jpeg_cases as JC
    import jpeg_tools as J
    import jpegxl_rs_amd as jx
    cached = args.cache and os.path.join(args.cache, "jpeg_batch_%dx%d_q%d_n%d%s.pickle" % (args.width, args.height, args.quality, args.distinct, "_progressive" if args.progressive else ""))
    if cached and os.path.exists(cached):
        with open(cached, "rb") as f:
            jpegs, jxls = pickle.load(f)
    else:
        jpegs = []
        for k in range(args.distinct):
            buf = io.BytesIO()
            Image.fromarray(JC.photo(args.width, args.height, seed=100 + k)).save(buf, "JPEG", quality=args.quality, subsampling=2, progressive=args.progressive)
            jpegs.append(buf.getvalue())
        jxls = [J.transcode(d) for d in jpegs]
        if cached:
            os.makedirs(args.cache, exist_ok=True)
            with open(cached, "wb") as f:
                pickle.dump((jpegs, jxls), f)
    files = [jpegs[k % args.distinct] for k in range(args.files)]
    inputs = [jxls[k % args.distinct] for k in range(args.files)]
    out = {"what": "JPEG reconstruction, files per second", "files": args.files, "distinct": args.distinct, "size": [args.width, args.height], "quality": args.quality, "progressive": args.progressive,
           "jpeg_bytes": sum(len(f) for f in files), "package": os.path.dirname(os.path.abspath(jx.__file__))}

    def batch_leg(host_writer, progressive_on_device=False):
        b = jx.BatchDecoder(0)
        if host_writer:
            b.set_option("jpeg_host_writer", 1)
        for d in inputs:
            b.add(d)
        if progressive_on_device:
            b.reconstruct_jpegs(progressive_on_device=True)
        else:
            b.reconstruct_jpegs()
        got = [b.jpeg(i) for i in range(len(inputs))]
        counts = (b.info_value("jpeg_device_images"), b.info_value("jpeg_host_images"))
        del b
        return got, counts

    def single_leg():
        dec = jx.decoder_builder()
        return [dec.reconstruct(d)[1][1] for d in inputs], None

    def pipeline_leg():
        p = jx.Pipeline(0)
        try:
            tickets = [p.submit_jpegs(inputs[k:k + args.job_files], progressive_on_device=args.progressive) for k in range(0, len(inputs), args.job_files)]
            got, dev, host = [], 0, 0
            for t in tickets:
                files, errors, _ = p.wait_jpegs(t)
                assert errors == [None] * len(files), errors
                got += files
                dev += p.info("jpeg_device_images"); host += p.info("jpeg_host_images")
        finally:
            p.close()
        return got, (dev, host)

    for leg in args.legs.split(","):
        run = single_leg if leg == "single" else pipeline_leg if leg == "pipeline" else (lambda h=(leg == "host"), p=(leg == "device_progressive"): batch_leg(h, p))
        times, counts = [], None
        for r in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            got, counts = run()
            times.append((time.perf_counter() - t0) * 1e3)
            if r == 0:
                assert got == files, leg + ": bytes differ from the source files"
        ms = median(times[args.warmup:])
        out[leg] = {"ms_per_batch": round(ms, 2), "files_per_s": round(args.files / ms * 1e3, 1), "ms_min": round(min(times[args.warmup:]), 2)}
        if counts:
            out[leg]["device_images"], out[leg]["host_images"] = counts
    print(json.dumps(out))


if __name__ == "__main__":
    main()
