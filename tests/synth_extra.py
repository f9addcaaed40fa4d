"""ctypes binding of the synthesiser's entry points for images with a list of extra channels (tools/jxl_synth.cc jxlsynth_modular_ec /
jxlsynth_vardct_ec), and the picture material the tests of such images share."""
import ctypes as C
import numpy as np
import synth_lib as S

ALPHA, DEPTH, SPOT, SELECTION, OPTIONAL = 0, 1, 2, 3, 16
REPLACE, ADD, BLEND, MULADD, MUL = 0, 1, 2, 3, 4


class Extra(C.Structure):
    """tools/jxl_synth.cc jxlsynth_extra"""
    _fields_ = [(n, C.c_int32) for n in ("type", "bits", "exp_bits", "premultiplied", "blend_mode", "blend_alpha", "blend_clamp", "blend_source")] + [
        ("spot", C.c_float * 4), ("name", C.c_char * 16)]


def extra(type=ALPHA, bits=8, exp_bits=0, premultiplied=0, mode=REPLACE, alpha=0, clamp=0, source=0, spot=(0, 0, 0, 0), name=b""):
    return Extra(type, bits, exp_bits, premultiplied, mode, alpha, clamp, source, (C.c_float * 4)(*spot), name)


def _lib():
    L = S.lib()
    L.jxlsynth_modular_ec.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(Extra), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(S.Frame),
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.jxlsynth_vardct_ec.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(Extra), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(S.Params), C.POINTER(S.Frame),
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    return L


def _planes(arrs):
    keep = [np.ascontiguousarray(a, dtype=np.int32) for a in arrs]
    return keep, (C.c_void_p * len(keep))(*[a.ctypes.data for a in keep])


def encode_modular_ec(color, planes, extras, fx=None, bits=8, color_alpha=0, upsampling=1):
    """Lossless Modular frame: color (h, w, 1 | 3) integers, planes: one (h, w) integer array per entry of `extras`."""
    L = _lib()
    h, w, nc = color.shape
    keep, arr = _planes([color[..., c] for c in range(nc)] + list(planes))
    ec = (Extra * len(extras))(*extras)
    out = C.c_void_p(); n = C.c_size_t()
    fx = fx if fx is not None else S.frame()
    if L.jxlsynth_modular_ec(arr, nc, ec, len(extras), color_alpha, w, h, bits, upsampling, C.byref(fx), C.byref(out), C.byref(n)):
        raise RuntimeError(L.jxlsynth_last_error().decode())
    return S._take(out, n)


def encode_vardct_ec(rgb, planes, extras, fx=None, color_alpha=0, seed=1, distance=1.0, epf_iters=1, gab=1, strategy_mix=1):
    """VarDCT frame (rgb (h, w, 3) uint8 sRGB) with lossless extra channels."""
    L = _lib()
    h, w = rgb.shape[:2]
    keep, arr = _planes(planes)
    ec = (Extra * len(extras))(*extras)
    p = S.Params(seed=seed, distance=distance, epf_iters=epf_iters, gab=gab, strategy_mix=strategy_mix, out_bits=8, orientation=1, upsampling=1, num_passes=1)
    a = np.ascontiguousarray(rgb, dtype=np.uint8)
    out = C.c_void_p(); n = C.c_size_t()
    fx = fx if fx is not None else S.frame()
    if L.jxlsynth_vardct_ec(a.ctypes.data, arr, ec, len(extras), color_alpha, w, h, C.byref(p), C.byref(fx), C.byref(out), C.byref(n)):
        raise RuntimeError(L.jxlsynth_last_error().decode())
    return S._take(out, n)


def plane(seed, w, h, bits=8):
    """A deterministic sample plane with smooth and busy parts, full range of `bits`."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = (np.sin(x / (7.0 + seed % 5)) + np.cos(y / (5.0 + seed % 3))) * 0.25 + 0.5 + rng.uniform(-0.08, 0.08, (h, w))
    return np.clip(np.rint(v * ((1 << bits) - 1)), 0, (1 << bits) - 1).astype(np.int32)
