#!/usr/bin/env python3
"""Output digests and decode times of the frame tail's extra-channel paths, on the seeded streams of tests/test_many_extra_channels.py with 1, 2 and 4 extra channels:
layered (a cropped frame blended onto a reference frame) as VarDCT and as Modular, patched (overlapping placements, per-channel modes), upsampled (2 and 4 channels) and —
four channels — spot-layered.  Every stream is decoded through the C ABI as u8 and as f32 with every extra-channel plane requested; each output buffer (the colour interleave, then the
planes) gives one SHA-256.  The u8 decode is timed as a whole — a host clock around the ABI calls, which return once the device has been synchronised and the buffers
are filled — after one warm-up decode: the median of --decodes decodes per stream and size.

Sizes: the tests' 300x200 canvas, where the number of launches decides, and a larger one with the streams' geometry (crop, patch source and placements) scaled along.
--cache DIR keeps the synthesised streams (the Python synthesiser takes seconds per stream at the larger size): built once, read by every later run.

Prints one JSON line.  With PYTHONPATH pointing at another build of the package the same script measures that build.  --against DIR does that itself: it runs this
script (after it has built the streams, into a temporary directory unless --cache names one) --reps times with PYTHONPATH=DIR (the reference build) and --reps times without, in turn, one fresh process each, and reports per stream and size
  ref_ms / new_ms   the median over the runs of each run's median,
  ref_spread_ms     max - min of the reference build's run medians — the resolution of the machine,
  slower            new_ms > ref_ms + ref_spread_ms,
and whether every digest of the two builds is equal.  A run that fails ends the comparison at once (exit status 1)."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.append(ROOT)                     # (behind PYTHONPATH: another build of the package may be measured with this script)
sys.path.append(os.path.join(ROOT, "tests"))

NS = (1, 2, 4)


def stream_makers(T):
    out = {}
    for n in NS:
        out["layered_vardct_n%d" % n] = (n, lambda n=n: T.layered("vardct", n)[0])
        out["layered_modular_n%d" % n] = (n, lambda n=n: T.layered("modular", n)[0])
        out["patched_n%d" % n] = (n, lambda n=n: T.patched(None, False, n))
        if n > 1:                   # (the upsampled stream pins its channel 1)
            out["upsampled_n%d" % n] = (n, lambda n=n: T.upsampled(None, n)[0])
    out["spot_layered_n4"] = (4, lambda: T.spot_layered(None, 4))
    return out


def set_geometry(T, w, h):
    """the test module's canvas, crop and patch geometry, scaled from its 300x200 to w x h"""
    fx, fy = w / 300.0, h / 200.0
    T.W, T.H, T.FW, T.FH, T.X0, T.Y0 = w, h, int(150 * fx), int(90 * fy), int(211 * fx), int(-37 * fy)
    T.PATCH_REF, T.PATCH_RECT = (int(64 * fx), int(48 * fy)), (2, 2, int(40 * fx), int(35 * fy))
    T.PATCH_AT = tuple((int(x * fx), int(y * fy)) for x, y in ((5, 5), (259, 10), (120, 160), (130, 165)))
    for f in (T.layered, T.patched, T.upsampled, T.spot_layered):
        f.cache_clear()


def streams_of(T, w, h, cache):
    set_geometry(T, w, h)
    out = {}
    for name, (n, make) in stream_makers(T).items():
        path = os.path.join(cache, "%s_%dx%d.jxl" % (name, w, h)) if cache else None
        if path and os.path.exists(path):
            data = open(path, "rb").read()
        else:
            t0 = time.perf_counter()
            data = make()
            print("built %s %dx%d in %.1f s" % (name, w, h, time.perf_counter() - t0), file=sys.stderr)
            if path:
                os.makedirs(cache, exist_ok=True)
                open(path, "wb").write(data)
        out[name] = (n, data)
    return out


def measure(args):
    import jpegxl_rs_amd as jx
    import test_many_extra_channels as T
    res = {"what": "frame tail with 1, 2 and 4 extra channels", "package": os.path.dirname(os.path.abspath(jx.__file__)), "digests": {}, "ms": {}, "patch_tmp_bytes": {}}
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        for name, (n, data) in streams_of(T, w, h, args.cache).items():
            key = "%s@%s" % (name, size)
            for ctype in ("u8", "f32"):
                (fr,) = T.abi_decode(jx, data, n, ctype)               # (also the warm-up of the timed decodes)
                res["digests"]["%s/%s" % (key, ctype)] = [hashlib.sha256(b.tobytes()).hexdigest() for b in [fr["px"]] + fr["planes"]]
            times = []
            for _ in range(args.decodes):
                t0 = time.perf_counter()
                T.abi_decode(jx, data, n, "u8")
                times.append((time.perf_counter() - t0) * 1e3)
            res["ms"][key] = round(statistics.median(times), 3)
            if name.startswith("patched"):      # the planes the patch kernel parks new values in: one of the coded size per extra channel
                res["patch_tmp_bytes"][key] = n * w * h * 4
    print(json.dumps(res))


def compare(args):
    import test_many_extra_channels as T
    cache = args.cache or tempfile.mkdtemp(prefix="frame_tail_streams_")
    for size in args.sizes.split(","):
        streams_of(T, *(int(v) for v in size.split("x")), cache)
    cmd = [sys.executable, os.path.abspath(__file__), "--sizes", args.sizes, "--decodes", str(args.decodes), "--cache", cache]
    runs = {"ref": [], "new": []}
    for rep in range(args.reps):
        for leg in ("ref", "new"):
            env = dict(os.environ)
            if leg == "ref":
                env["PYTHONPATH"] = os.path.abspath(args.against) + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.run_timeout)
            if p.returncode != 0:
                print(json.dumps({"failed": leg, "rep": rep, "status": p.returncode}))
                return 1
            runs[leg].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print("%s run %d done" % (leg, rep), file=sys.stderr)
    assert runs["ref"][0]["package"] != runs["new"][0]["package"], "both legs measured the same build"
    differing = sorted({k for leg in runs for r in runs[leg] for k, d in r["digests"].items() if d != runs["ref"][0]["digests"][k]})
    table = {}
    for key in runs["ref"][0]["ms"]:
        ref, new = [r["ms"][key] for r in runs["ref"]], [r["ms"][key] for r in runs["new"]]
        row = {"ref_ms": round(statistics.median(ref), 3), "ref_spread_ms": round(max(ref) - min(ref), 3), "new_ms": round(statistics.median(new), 3), "new_spread_ms": round(max(new) - min(new), 3)}
        row["slower"] = row["new_ms"] > row["ref_ms"] + row["ref_spread_ms"]
        table[key] = row
    print(json.dumps({"what": runs["new"][0]["what"], "ref": runs["ref"][0]["package"], "new": runs["new"][0]["package"], "reps": args.reps, "decodes": args.decodes,
                      "buffers_hashed": sum(len(d) for d in runs["ref"][0]["digests"].values()), "digests_equal": not differing, "differing": differing,
                      "slower": sorted(k for k, r in table.items() if r["slower"]), "ms": table, "patch_tmp_bytes": runs["new"][0]["patch_tmp_bytes"]}))
    return 0 if not differing and not any(r["slower"] for r in table.values()) else 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="300x200,1920x1080")
    ap.add_argument("--decodes", type=int, default=5, help="timed decodes per stream and size, behind one warm-up decode")
    ap.add_argument("--cache", default=None, help="directory that keeps the synthesised streams")
    ap.add_argument("--against", default=None, help="PYTHONPATH of the reference build: alternate the two builds and compare")
    ap.add_argument("--reps", type=int, default=5, help="with --against: runs of each build")
    ap.add_argument("--run-timeout", type=float, default=300, help="with --against: seconds one run may take")
    args = ap.parse_args()
    sys.exit(compare(args) if args.against else measure(args))


if __name__ == "__main__":
    main()
