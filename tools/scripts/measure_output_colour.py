"""What an image that is not XYB pays for a converting output colour ("Output colour"): one 3840x2160 lossless Modular image with a Display-P3 header, u8 output,
with and without output_color="srgb", convert_non_xyb=True, through JxlHipBatchDecodeTimed, seven decodes each, alternating.  Prints the median, minimum and maximum of total_ms."""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import jpegxl_rs_amd as jx
import synth_lib as S

img = S.synthetic_image(7, 3840, 2160).astype(np.int32)
S.set_color(white_point=1, primaries=11, tf=13)
try:
    data = S.encode_modular(img, 8)
finally:
    S.set_color()
print("stream bytes", len(data), flush=True)
batches = {}
for name, kw in (("plain", {}), ("converted", dict(output_color="srgb", convert_non_xyb=True))):
    b = jx.BatchDecoder(0)
    b.add(data, "uint8", 3, **kw)
    b.prepare(); b.decode(); b.finish()
    batches[name] = b
times = {k: [] for k in batches}
for r in range(7):
    for name, b in batches.items():
        b.decode_timed(); b.finish()
        t, runs = b.collect_times()
        times[name].append(t["total_ms"] / max(1, runs))
for name, v in times.items():
    print(name, "total_ms median %.3f min %.3f max %.3f" % (statistics.median(v), min(v), max(v)), ["%.3f" % x for x in v], flush=True)
a, c = batches["plain"].output(0), batches["converted"].output(0)
print("outputs differ:", int((a != c).sum()), "of", a.size)
