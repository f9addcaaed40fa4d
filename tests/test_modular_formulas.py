"""The integer half of the Modular path against its definitions (PARITY.md "Modular integer stages").

`restate(script)` below is a Modular decoder without entropy coding, written from the format's definitions (ISO/IEC 18181-1: the MA-tree properties, the
predictors, the reversible colour transforms, the palette with its implicit entries, the delta-palette scan) in Python integers / int64 numpy.  It imports
nothing from oracle/ and nothing from the product.  The streams come from the scripted writer (tools/synth_script.h, synth_lib.encode_modular_scripted): the
caller decides the transforms, the tree and the value of every token, so the restatement knows what the image has to be — exactly.

Two layers over the same cases:  CPU (unmarked)  oracle == restate;   gpu-marked  product == restate.
Results are read off the f32 decode (samples are not clamped there): integer = rint(float64(x) * (2^bits - 1)), exact because every test asserts |sample| <= 2^20;
and every test asserts that no intermediate value reaches 2^28, so no case depends on overflow behaviour.  Every case asserts that its input holds the classes it
claims (index ranges, edge fall-backs, both branches) before anything is compared.

Not restated (NotImplementedError): predictor 6 and property 15 (the weighted predictor) — pinned by the synthesiser's lossless round trip and by bench.jxl —
and Squeeze (pinned by the lossless round trip)."""
import numpy as np
import pytest

import oracle_lib as O
import synth_lib as S


@pytest.fixture(scope="module")
def jx(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import jpegxl_rs_amd as jx
    return jx


# =====================================================================================================================================================
# The restatement
# =====================================================================================================================================================
# Table of the implicit delta-palette entries (negative indices), as the format lists it
DELTA = np.array([
    (0, 0, 0), (4, 4, 4), (11, 0, 0), (0, 0, -13), (0, -12, 0), (-10, -10, -10), (-18, -18, -18), (-27, -27, -27),
    (-18, -18, 0), (0, 0, -32), (-32, 0, 0), (-37, -37, -37), (0, -32, -32), (24, 24, 45), (50, 50, 50), (-45, -24, -24),
    (-24, -45, -45), (0, -24, -24), (-34, -34, 0), (-24, 0, -24), (-45, -45, -24), (64, 64, 64), (-32, 0, -32), (0, -32, 0),
    (-32, 0, 32), (-24, -45, -24), (45, 24, 45), (24, -24, -45), (-45, -24, 24), (80, 80, 80), (64, 0, 0), (0, 0, -64),
    (0, -64, -64), (-24, -24, 45), (96, 96, 96), (64, 64, 0), (45, -24, -24), (34, -34, 0), (112, 112, 112), (24, -45, -45),
    (45, 45, -24), (0, -32, 32), (24, -24, 45), (0, 96, 96), (45, -24, 24), (24, -45, -24), (-24, -45, 24), (0, -64, 0),
    (96, 0, 0), (128, 128, 128), (64, 0, 64), (144, 144, 144), (96, 96, 0), (-36, -36, 36), (45, -24, -45), (45, -45, -24),
    (0, 0, -96), (0, 128, 128), (0, 96, 0), (45, 24, -45), (-128, 0, 0), (24, -45, 24), (-45, 24, -45), (64, 0, -64),
    (64, -64, -64), (96, 0, 96), (45, -45, 24), (24, 45, -45), (64, 64, -64), (128, 128, 0), (0, 0, -128), (-24, 45, -45)], np.int64)
assert DELTA.shape == (72, 3)
# Where the three results of an inverse RCT go, per permutation (rct_type // 7): (first, second, third) -> channel
PERMUTATION = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (1, 0, 2), (2, 1, 0))
PREDICTORS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13)      # all but the weighted one


class Peak:
    """Largest magnitude any stage has seen.  Every intermediate of the restatement is a stage value or a sum of stage values with weights adding up to at
    most 20 (predictor 13: 6 + 2 + 7 + 1 + 1 + 3, plus 8), so `intermediate_bound()` bounds them all."""

    def __init__(self):
        self.v = 0

    def see(self, a):
        a = np.asarray(a)
        if a.size:
            self.v = max(self.v, int(np.abs(a).max()))
        return a

    def intermediate_bound(self):
        return 20 * self.v + 8


def idiv(a, b):
    """Integer division that truncates towards zero (the format's predictors divide like that)"""
    q = abs(a) // b
    return q if a >= 0 else -q


def neighbours(rows, x, y, w):
    """W, N, NW, NE, NN, WW, NEE of sample (x, y) of a channel `w` wide whose rows so far are `rows`, with the format's fall-backs at the edges"""
    row = rows[y]
    up = rows[y - 1] if y > 0 else None
    W = row[x - 1] if x > 0 else (up[x] if y > 0 else 0)
    N = up[x] if y > 0 else W
    NW = up[x - 1] if (x > 0 and y > 0) else W
    NE = up[x + 1] if (y > 0 and x + 1 < w) else N
    NN = rows[y - 2][x] if y > 1 else N
    WW = row[x - 2] if x > 1 else W
    NEE = up[x + 2] if (y > 0 and x + 2 < w) else NE
    return W, N, NW, NE, NN, WW, NEE


def clamped_gradient(W, N, NW):
    return min(max(W + N - NW, min(W, N)), max(W, N))


def predict(p, W, N, NW, NE, NN, WW, NEE):
    if p == 0: return 0
    if p == 1: return W
    if p == 2: return N
    if p == 3: return idiv(W + N, 2)
    if p == 4: return W if abs(N - NW) < abs(W - NW) else N              # Select: the neighbour closer to W + N - NW (|g - W| = |N - NW|, |g - N| = |W - NW|)
    if p == 5: return clamped_gradient(W, N, NW)
    if p == 7: return NE
    if p == 8: return NW
    if p == 9: return WW
    if p == 10: return idiv(W + NW, 2)
    if p == 11: return idiv(N + NW, 2)
    if p == 12: return idiv(N + NE, 2)
    if p == 13: return idiv(6 * N - 2 * NN + 7 * W + WW + NEE + 3 * NE + 8, 16)
    raise NotImplementedError("predictor %d" % p)                          # 6: the weighted predictor


def property_value(p, chan, stream_id, x, y, W, N, NW, NE, NN, WW, prev_gradient, refs):
    if p == 0: return chan
    if p == 1: return stream_id
    if p == 2: return y
    if p == 3: return x
    if p == 4: return abs(N)
    if p == 5: return abs(W)
    if p == 6: return N
    if p == 7: return W
    if p == 8: return W - prev_gradient                                     # prev_gradient: property 9 of the sample to the left (0 in column 0)
    if p == 9: return W + N - NW
    if p == 10: return W - NW
    if p == 11: return NW - N
    if p == 12: return N - NE
    if p == 13: return N - NN
    if p == 14: return W - WW
    if p == 15: raise NotImplementedError("property 15")
    k, which = divmod(p - 16, 4)                                            # the k-th previous channel of the same size in this stream, nearest first
    if k >= len(refs):
        return 0
    r = refs[k]
    rC = r[y][x]
    rW = r[y][x - 1] if x > 0 else 0
    rN = r[y - 1][x] if y > 0 else rW
    rNW = r[y - 1][x - 1] if (x > 0 and y > 0) else rW
    d = rC - clamped_gradient(rW, rN, rNW)
    return (abs(rC), rC, abs(d), d)[which]


def scan_channel(chan, w, h, tokens, tree, stream_id, refs, branch_count):
    """Raster scan of one channel: tree walk on the properties, value = token * multiplier + offset + prediction"""
    T = tokens.tolist()
    R = [r.tolist() for r in refs]
    rows = []
    for y in range(h):
        row = [0] * w
        rows.append(row)
        trow = T[y]
        prev_gradient = 0
        for x in range(w):
            W, N, NW, NE, NN, WW, NEE = neighbours(rows, x, y, w)
            n = 0
            while tree[n][0] >= 0:
                prop, val, left, right, _ = tree[n]
                n = left if property_value(prop, chan, stream_id, x, y, W, N, NW, NE, NN, WW, prev_gradient, R) > val else right
            _, pred, offset, mul_log, mul_bits = tree[n]
            branch_count[n] = branch_count.get(n, 0) + 1
            row[x] = trow[x] * ((mul_bits + 1) << mul_log) + offset + predict(pred, W, N, NW, NE, NN, WW, NEE)
            prev_gradient = W + N - NW
    return np.array(rows, np.int64).reshape(h, w)


def decode_stream(dims, tokens, tree, stream_id, peak, branch_count):
    """dims: (w, h, is_meta) per channel of the stream; tokens: one (h, w) int64 array each -> the decoded channels"""
    out = []
    max_mul = max((n[4] + 1) << n[3] for n in tree if n[0] < 0)
    for c, (w, h, meta) in enumerate(dims):
        tok = tokens[c]
        assert tok.shape == (h, w), (tok.shape, (h, w))
        peak.see(tok * max_mul)
        if len(tree) == 1 and tree[0][1] == 0:                               # a single Zero leaf: no neighbour takes part
            out.append(peak.see(tok * ((tree[0][4] + 1) << tree[0][3]) + tree[0][2]))
            continue
        refs = [out[j] for j in range(c - 1, -1, -1) if dims[j] == dims[c]]   # (a palette never has the geometry of an image channel: is_meta is part of it)
        out.append(peak.see(scan_channel(c, w, h, tok, tree, stream_id, refs, branch_count)))
    return out


def meta_apply(dims, t):
    """What a transform does to the channel list before decoding: a palette replaces its num_c channels by one index channel and puts itself in front"""
    if t[0] == 1:
        _, begin_c, num_c, nb_colors, _, _ = t
        del dims[begin_c + 1:begin_c + num_c]
        dims.insert(0, (nb_colors, num_c, True))


def inverse_rct(chs, begin_c, rct_type, peak):
    a, b, c = chs[begin_c:begin_c + 3]
    permutation, kind = divmod(rct_type, 7)
    if kind == 6:                                                            # YCgCo-R: a = Y, b = Co, c = Cg
        tmp = a - (c >> 1)
        second = c + tmp
        third = tmp - (b >> 1)
        first = third + b
        peak.see(tmp)
    else:
        first = a
        third = c + a if kind & 1 else c
        second = b + a if kind >> 1 == 1 else (b + ((first + third) >> 1) if kind >> 1 == 2 else b)
        peak.see(first + third)
    for v, pos in zip((first, second, third), PERMUTATION[permutation]):
        chs[begin_c + pos] = peak.see(v)


def forward_rct(c0, c1, c2, rct_type):
    """Test-side: the three coded channels whose inverse RCT gives (c0, c1, c2)"""
    permutation, kind = divmod(rct_type, 7)
    src = (c0, c1, c2)
    first, second, third = (src[pos] for pos in PERMUTATION[permutation])
    if kind == 6:
        co = first - third
        tmp = third + (co >> 1)
        cg = second - tmp
        return tmp + (cg >> 1), co, cg
    b = second - first if kind >> 1 == 1 else (second - ((first + third) >> 1) if kind >> 1 == 2 else second)
    c = third - first if kind & 1 else third
    return first, b, c


def palette_value(pal, index, c, bits):
    """The palette's value for channel c at every index of the array `index`: explicit entries, then the 4x4x4 and the 5x5x5 cube, negative = implicit deltas"""
    nb = pal.shape[1]
    out = np.zeros(index.shape, np.int64)
    explicit = (index >= 0) & (index < nb)
    out[explicit] = pal[c][index[explicit]]
    if c >= 3:
        return out                                                           # implicit entries have three channels; a fourth reads 0
    neg = index < 0
    i = (-(index[neg] + 1)) % 143
    out[neg] = DELTA[(i + 1) >> 1, c] * np.where(i & 1, 1, -1) * (1 << max(0, bits - 8))
    small = (index >= nb) & (index < nb + 64)
    i = (index[small] - nb) >> (2 * c)
    out[small] = (i % 4) * ((1 << bits) - 1) // 4 + (1 << max(0, bits - 3))
    large = index >= nb + 64
    i = (index[large] - nb - 64) // 5 ** c
    out[large] = (i % 5) * ((1 << bits) - 1) // 4
    return out


def inverse_palette(chs, t, bits, peak):
    _, begin_c, num_c, nb_colors, nb_deltas, predictor = t
    pal, index = chs[0], chs[begin_c + 1]
    assert pal.shape == (num_c, nb_colors)
    h, w = index.shape
    outs = []
    for c in range(num_c):
        val = peak.see(palette_value(pal, index, c, min(bits, 24)))
        if nb_deltas == 0 and predictor == 0:
            outs.append(val)
            continue
        V, I, rows = val.tolist(), index.tolist(), []                          # the delta scan: entries below nb_deltas (the negative ones too) add to a prediction
        for y in range(h):
            rows.append([0] * w)
            for x in range(w):
                v = V[y][x]
                if I[y][x] < nb_deltas:
                    v += predict(predictor, *neighbours(rows, x, y, w))
                rows[y][x] = v
        outs.append(peak.see(np.array(rows, np.int64).reshape(h, w)))
    chs[:] = chs[1:begin_c + 1] + outs + chs[begin_c + 2:]


def undo(chs, transforms, bits, peak):
    for t in reversed(transforms):
        if t[0] == 0:
            inverse_rct(chs, t[1], t[2], peak)
        else:
            inverse_palette(chs, t, bits, peak)


def restate(sc):
    """-> (image (h, w, channels) int64, Peak, {tree node: samples that ended in that leaf})"""
    w, h, bits = sc["w"], sc["h"], sc["bits"]
    tree = sc.get("tree", (S.leaf(),))
    gt, lt = list(sc.get("gt", ())), list(sc.get("lt", ()))
    gd = 128 << sc.get("shift", 1)
    xg, yg = -(-w // gd), -(-h // gd)
    num_lf_groups = (-(-w // (8 * gd))) * (-(-h // (8 * gd)))
    ntot = sc["nchan"] + (1 if sc.get("has_alpha") else 0)
    peak, branch = Peak(), {}
    planes = [np.asarray(p).astype(np.int64) for p in sc["planes"]]
    glist = [(w, h, False)] * ntot
    for t in gt:
        meta_apply(glist, t)
    nglobal = 0                                                              # GlobalModular: every meta channel, then every channel that fits a group
    while nglobal < len(glist) and (glist[nglobal][2] or (glist[nglobal][0] <= gd and glist[nglobal][1] <= gd)):
        nglobal += 1
    chs = decode_stream(glist[:nglobal], planes[:nglobal], tree, 0, peak, branch)
    nrest = len(glist) - nglobal
    chs += [np.zeros((h, w), np.int64) for _ in range(nrest)]
    for g in range(xg * yg if nrest else 0):                                 # each group rectangle is a stream of its own
        x0, y0 = (g % xg) * gd, (g // xg) * gd
        rw, rh = min(gd, w - x0), min(gd, h - y0)
        ldims = [(rw, rh, False)] * nrest
        for t in lt:
            meta_apply(ldims, t)
        toks = [planes[nglobal + c] if d[2] else planes[nglobal + c][y0:y0 + rh, x0:x0 + rw] for c, d in enumerate(ldims)]
        vals = decode_stream(ldims, toks, tree, 1 + 3 * num_lf_groups + 17 + g, peak, branch)
        undo(vals, lt, bits, peak)
        assert len(vals) == nrest
        for k, v in enumerate(vals):
            chs[nglobal + k][y0:y0 + rh, x0:x0 + rw] = v
    undo(chs, gt, bits, peak)
    assert len(chs) == ntot
    return np.stack(chs, axis=-1), peak, branch


# =====================================================================================================================================================
# Cases: name -> list of (tag, script).  A case asserts that its inputs hold the classes it is there for.
# =====================================================================================================================================================
CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def script(w, h, planes, bits=8, nchan=3, has_alpha=False, shift=1, gt=(), lt=(), tree=(S.leaf(),), local_tree=False):
    return dict(w=w, h=h, planes=planes, bits=bits, nchan=nchan, has_alpha=has_alpha, shift=shift, gt=tuple(gt), lt=tuple(lt), tree=tuple(tree), local_tree=local_tree)


def encode(sc):
    return S.encode_modular_scripted(sc["w"], sc["h"], sc["planes"], bits=sc["bits"], nchan=sc["nchan"], has_alpha=sc["has_alpha"], group_shift=sc["shift"],
                                     global_transforms=sc["gt"], local_transforms=sc["lt"], tree=sc["tree"], local_tree=sc["local_tree"])


def final_image(seed, w, h, nch):
    """An image for the RCT cases: signed, odd and even, so that every `>> 1` of a transform floors a negative somewhere"""
    return [p for p in np.random.default_rng(seed).integers(-700, 1500, (nch, h, w)).astype(np.int64)]


def assert_rct_classes(coded, rct_type, tag):
    a, b, c = coded
    kind = rct_type % 7
    if kind == 6:
        assert ((b < 0) & (b & 1 == 1)).any() and ((c < 0) & (c & 1 == 1)).any(), (tag, "no negative odd chroma")
    if kind in (4, 5):
        s = a + (c + a if kind & 1 else c)
        assert ((s < 0) & (s & 1 == 1)).any(), (tag, "no negative odd first + third")
    assert (b < 0).any() and (c < 0).any(), tag


def rct_scripts(w, h, shift, where, types=range(42), alpha=False):
    out = []
    img = final_image(w * 1000 + h, w, h, 4 if alpha else 3)
    for t in types:
        m = 1 if alpha else 0
        coded = forward_rct(img[m], img[m + 1], img[m + 2], t)
        assert_rct_classes(coded, t, (where, t))
        planes = img[:m] + list(coded)
        kw = dict(gt=[S.rct(m, t)]) if where == "global" else dict(lt=[S.rct(m, t)])
        out.append(("type%d" % t, script(w, h, planes, has_alpha=alpha, shift=shift, **kw)))
    return out


@case
def rct_global_5x3():
    return rct_scripts(5, 3, 1, "global")


@case
def rct_global_four_groups():
    return rct_scripts(150, 140, 0, "global")


@case
def rct_local_four_groups():
    return rct_scripts(150, 140, 0, "local")


@case
def rct_global_begin1_over_g_b_alpha():
    return rct_scripts(37, 23, 1, "global", alpha=True)


@case
def rct_grid_stride_1100x1000():
    assert 1100 * 1000 > 4096 * 256                                          # more samples than ModRctKernel's largest grid has threads: a second trip
    return rct_scripts(1100, 1000, 1, "global", types=(6, 13, 32))           # 32 = permutation 4, kind 4


# ---- palettes ---------------------------------------------------------------------------------------------------------------------------------------
NB = 11                                                                        # explicit colours of the plain-palette cases
PALETTE_KINDS = {"grey": (1, False, 0, 1), "rgb": (3, False, 0, 3), "rgba": (3, True, 0, 4), "alpha_only": (3, True, 3, 1)}   # nchan, alpha, begin_c, num_c


def index_classes(nb):
    return np.array(list(range(nb)) + list(range(nb, nb + 64 + 125 + 3)) + list(range(-1, -144, -1)) + [-144, -300], np.int64)


def index_plane(w, h, nb, seed):
    cls = index_classes(nb)
    assert w * h >= cls.size
    idx = np.resize(cls, w * h)
    return np.random.default_rng(seed).permutation(idx).reshape(h, w)


def assert_index_classes(idx, nb, tag):
    have = set(np.unique(idx).tolist())
    assert set(range(nb)) <= have, (tag, "explicit indices")
    assert set(range(nb, nb + 64)) <= have and set(range(nb + 64, nb + 189)) <= have and set(range(nb + 189, nb + 192)) <= have, (tag, "cube indices")
    assert set(range(-143, 0)) <= have and {-144, -300} <= have, (tag, "negative indices")


def palette_entries(nb, num_c, bits, seed):
    return np.random.default_rng(seed).integers(-50, (1 << bits) + 50, (num_c, nb)).astype(np.int64)


def palette_scripts(w, h, shift, where, kinds=PALETTE_KINDS, depths=(2, 8, 12, 16)):
    out = []
    for kind in kinds:
        nchan, alpha, begin_c, num_c = PALETTE_KINDS[kind]
        for bits in depths:
            rng = np.random.default_rng(bits * 10 + num_c)
            idx = index_plane(w, h, NB, bits + num_c)
            assert_index_classes(idx, NB, (kind, bits))
            others = [p for p in rng.integers(-40, 1 << bits, (begin_c, h, w)).astype(np.int64)]      # the channels in front of the palette's
            planes = [palette_entries(NB, num_c, bits, bits)] + others + [idx]
            kw = dict(gt=[S.palette(begin_c, num_c, NB)]) if where == "global" else dict(lt=[S.palette(begin_c, num_c, NB)])
            out.append(("%s_%dbit" % (kind, bits), script(w, h, planes, bits=bits, nchan=nchan, has_alpha=alpha, shift=shift, **kw)))
    return out


@case
def palette_global_64x40():
    return palette_scripts(64, 40, 1, "global")


@case
def palette_global_four_groups():
    return palette_scripts(150, 140, 0, "global")                             # the palette rides in GlobalModular, the index channel in the sections


@case
def palette_local_four_groups():
    return palette_scripts(150, 140, 0, "local")


@case
def palette_grid_stride_1100x1000():
    assert 1100 * 1000 > 4096 * 256                                          # ModPaletteKernel's grid-stride loop takes a second trip
    return palette_scripts(1100, 1000, 1, "global", kinds=("rgb",), depths=(8,))


DELTA_SIZES = ((37, 23), (1, 9), (9, 1), (2, 5), (3, 5))


def delta_palette_scripts(num_c, bits):
    nb, nb_deltas = 12, 5
    out = []
    for w, h in DELTA_SIZES:
        rng = np.random.default_rng(w * 100 + h + num_c)
        pal = rng.integers(0, 1 << bits, (num_c, nb)).astype(np.int64)
        pal[:, :nb_deltas] = rng.integers(-4, 5, (num_c, nb_deltas))
        pick = rng.integers(0, 100, (h, w))
        idx = np.where(pick < 45, rng.integers(0, nb_deltas, (h, w)), np.where(pick < 70, -rng.integers(1, 150, (h, w)), np.where(pick < 90, rng.integers(nb_deltas, nb, (h, w)), nb + rng.integers(0, 189, (h, w)))))
        idx = idx.astype(np.int64)
        idx[0, 0], idx[-1, -1] = 1, -3                                        # the first sample predicted (from nothing), the last one too
        delta = idx < nb_deltas
        assert (idx < 0).any() and delta.any() and (~delta).any(), (w, h)
        if (w, h) == (37, 23):                                               # a predicted sample at every place where a neighbour falls back
            for name, m in (("first row", delta[0, 2:-2]), ("second row", delta[1, 2:-2]), ("x = 0", delta[2:, 0]), ("x = 1", delta[2:, 1]), ("x = w - 1", delta[2:, -1]), ("x = w - 2", delta[2:, -2]),
                            ("corner", delta[0, :1]), ("inside", delta[2:, 2:-2])):
                assert m.any(), name
        for p in PREDICTORS:
            out.append(("%dx%d_pred%d" % (w, h, p), script(w, h, [pal, idx], bits=bits, nchan=3, has_alpha=num_c == 4, gt=[S.palette(0, num_c, nb, nb_deltas, p)])))
    assert {w for w, h in DELTA_SIZES} >= {1, 2, 3} and 1 in {h for w, h in DELTA_SIZES}    # no W / WW / NE / NEE at all, NE without NEE, one row
    return out


@case
def palette_delta_three_channels():
    return delta_palette_scripts(3, 8)


@case
def palette_delta_four_channels():
    return delta_palette_scripts(4, 12)


@case
def transform_chains():
    out = []
    rng = np.random.default_rng(77)
    nb = 9
    for t in (6, 10, 19, 26, 40):
        # RCT, then a palette over the transformed channels: the inverse palette feeds the inverse RCT
        w, h = 64, 40
        idx = index_plane(w, h, nb, t)
        out.append(("rct%d_then_palette" % t, script(w, h, [palette_entries(nb, 3, 8, t), idx], gt=[S.rct(0, t), S.palette(0, 3, nb)])))
        # the same chain inside the sections, and a global RCT over what a local palette gives
        w, h = 150, 140
        idx = index_plane(w, h, nb, t + 1)
        out.append(("local_rct%d_behind_local_palette" % t, script(w, h, [palette_entries(nb, 3, 8, t + 1), idx], shift=0, lt=[S.rct(0, t), S.palette(0, 3, nb)])))
        out.append(("global_rct%d_local_palette" % t, script(w, h, [palette_entries(nb, 3, 8, t + 2), idx], shift=0, gt=[S.rct(0, t)], lt=[S.palette(0, 3, nb)])))
    # two palettes in one list: RGB, then alpha (channel 2 of the list the first one leaves: its palette, its index channel, alpha)
    for w, h, shift in ((64, 40, 1), (150, 140, 0)):
        nb2 = 7
        planes = [palette_entries(nb2, 1, 8, 5), palette_entries(nb, 3, 8, 6), index_plane(w, h, nb, 7), rng.integers(0, nb2, (h, w)).astype(np.int64)]
        out.append(("two_palettes_%dx%d" % (w, h), script(w, h, planes, has_alpha=True, shift=shift, gt=[S.palette(0, 3, nb), S.palette(2, 1, nb2)])))
    return out


# ---- predictors -------------------------------------------------------------------------------------------------------------------------------------
MULTIPLIERS = ((1, 0, 0), (2, 1, 0), (3, 0, 2), (4, 2, 0), (6, 1, 2))          # multiplier, mul_log, mul_bits


def predictor_tree(setting, p, h):
    if setting == "single_leaf":
        return (S.leaf(p),)
    if setting == "two_level":                                               # channel > 0 ? (row > h/3 ? p : other) : (row > h/2 ? other : p)
        other = 5 if p != 5 else 1
        return (S.split(0, 0, 1, 2), S.split(2, h // 3, 3, 4), S.split(2, h // 2, 5, 6), S.leaf(p), S.leaf(other), S.leaf(other), S.leaf(p))
    # five bands of rows, each with another multiplier and offset
    nodes = []
    for k in range(4):
        nodes.append(S.split(2, h * (4 - k) // 5 - 1, 2 * k + 1, 2 * k + 2))    # node 2k: row > cut ? leaf 2k + 1 : node 2k + 2
        nodes.append(None)
    nodes.append(None)
    for k, (mul, mul_log, mul_bits) in enumerate(MULTIPLIERS):
        assert (mul_bits + 1) << mul_log == mul
        nodes[2 * k + 1 if k < 4 else 8] = S.leaf(p, offset=(-3, 5, -1, 2, 7)[k], mul_log=mul_log, mul_bits=mul_bits)
    return tuple(nodes)


def predictor_scripts(setting, sizes, shift):
    out = []
    nchan, alpha = (1, True) if setting == "two_level" else (1, False)
    for w, h in sizes:
        tok = [p for p in np.random.default_rng(w * 31 + h).integers(-3, 4, (nchan + alpha, h, w)).astype(np.int64)]
        assert (tok[0] < 0).any() and (tok[0] > 0).any()
        for p in PREDICTORS:
            out.append(("%dx%d_pred%d" % (w, h, p), script(w, h, tok, bits=16, nchan=nchan, has_alpha=alpha, shift=shift, tree=predictor_tree(setting, p, min(h, 128 << shift)))))
    return out


PREDICTOR_GEOMETRIES = {"37x23": (((37, 23),), 1), "four_groups": (((150, 140),), 0), "narrow": (((1, 11), (2, 10), (3, 10)), 1)}
for _setting in ("single_leaf", "two_level", "multipliers"):
    for _geo, (_sizes, _shift) in PREDICTOR_GEOMETRIES.items():
        CASES["predictors_%s_%s" % (_setting, _geo)] = (lambda s=_setting, z=_sizes, sh=_shift: predictor_scripts(s, z, sh))


# ---- property probes --------------------------------------------------------------------------------------------------------------------------------
def probe_threshold(p, w, h):
    """Tokens are uniform in [-20000, 20000] and a leaf adds 0 or 4096, so a sample is roughly uniform around 2048, a difference of samples is symmetric
    around 0 and a magnitude is spread over [0, 24096]: these thresholds sit near the medians."""
    if p == 2: return h // 2 - 1
    if p == 3: return w // 2 - 1
    if p in (4, 5, 16): return 10000
    if p in (6, 7, 17): return 2048
    if p == 18: return 9000
    return 0


def probe_scripts(w, h, shift, props, nchan):
    out = []
    tok = [p for p in np.random.default_rng(w + h).integers(-20000, 20001, (nchan, h, w)).astype(np.int64)]
    for p in props:
        hh, ww = min(h, 128 << shift), min(w, 128 << shift)
        tree = (S.split(p, probe_threshold(p, ww, hh), 1, 2), S.leaf(0, offset=4096), S.leaf(0, offset=0))
        out.append(("prop%d" % p, script(w, h, tok, bits=16, nchan=nchan, shift=shift, tree=tree)))
    return out


@case
def properties_2_to_14_37x23():
    return probe_scripts(37, 23, 1, range(2, 15), 1)


@case
def properties_2_to_14_four_groups():
    return probe_scripts(150, 140, 0, range(2, 15), 1)


@case
def properties_16_to_19_37x23():
    return probe_scripts(37, 23, 1, range(16, 20), 3)


@case
def properties_16_to_19_four_groups():
    return probe_scripts(150, 140, 0, range(16, 20), 3)


# =====================================================================================================================================================
# The two layers
# =====================================================================================================================================================
_prepared = {}


def prepared(name):
    """[(tag, script, codestream, restated image)] of a case, computed once for both layers and left unchanged"""
    if name not in _prepared:
        items = []
        for tag, sc in CASES[name]():
            want, peak, branch = restate(sc)
            assert np.abs(want).max() <= 1 << 20, (name, tag, "samples must stay within 2^20 for the f32 read-out to be exact")
            assert peak.intermediate_bound() < 1 << 28, (name, tag, "an intermediate value reaches 2^28")
            if name.startswith("properties_"):                               # both branches of the probe taken on at least 20 % of the samples each
                total = sum(branch.values())
                assert total == want.size and min(branch.get(1, 0), branch.get(2, 0)) >= 0.2 * total, (name, tag, branch)
            if name.startswith("predictors_two_level") or name.startswith("predictors_multipliers"):
                assert all(branch.get(n, 0) > 0 for n, node in enumerate(sc["tree"]) if node[0] < 0), (name, tag, "a leaf is never reached", branch)
            want.setflags(write=False)
            items.append((tag, sc, encode(sc), want))
        _prepared[name] = items
    return _prepared[name]


def to_ints(px, sc):
    nch = sc["nchan"] + (1 if sc["has_alpha"] else 0)
    return np.rint(np.asarray(px, np.float32).astype(np.float64) * ((1 << sc["bits"]) - 1)).astype(np.int64).reshape(sc["h"], sc["w"], nch)


def compare(name, tag, got, want, who):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        y, x, c = bad[0]
        raise AssertionError("%s / %s: %s differs from the restatement in %d of %d samples, first at (x %d, y %d, channel %d): %d, restated %d"
                             % (name, tag, who, len(bad), want.size, x, y, c, got[y, x, c], want[y, x, c]))


def test_inverse_rct_undoes_forward_rct():
    """All 42 types: the restatement's inverse RCT gives back what the test's forward RCT was given (signed, odd and even samples)"""
    img = final_image(3, 19, 7, 3)
    for t in range(42):
        chs = list(forward_rct(img[0], img[1], img[2], t))
        inverse_rct(chs, 0, t, Peak())
        assert all(np.array_equal(a, b) for a, b in zip(chs, img)), t
    assert len({tuple(np.concatenate(forward_rct(img[0], img[1], img[2], t)).ravel().tolist()) for t in range(42)}) == 42      # 42 different transforms


def test_writer_refuses_planes_that_do_not_match():
    """The scripted writer derives the coded channel list itself and says what is wrong with planes that do not fit it"""
    idx = np.zeros((40, 64), np.int64)
    with pytest.raises(RuntimeError, match="2 channels, 1 planes"):
        S.encode_modular_scripted(64, 40, [idx], global_transforms=[S.palette(0, 3, 5)])
    with pytest.raises(RuntimeError, match="plane 0 is 4x3, the coded channel is 5x3"):
        S.encode_modular_scripted(64, 40, [np.zeros((3, 4), np.int64), idx], global_transforms=[S.palette(0, 3, 5)])
    with pytest.raises(RuntimeError, match="local palette must be plain"):
        S.encode_modular_scripted(150, 140, [np.zeros((3, 5), np.int64), np.zeros((140, 150), np.int64)], group_shift=0, local_transforms=[S.palette(0, 3, 5, 2, 1)])
    with pytest.raises(RuntimeError, match="need channels in the section streams"):
        S.encode_modular_scripted(64, 40, [idx] * 3, local_transforms=[S.rct(0, 6)])


def test_restatement_leaves_the_weighted_predictor_out():
    for tree in ((S.leaf(6),), (S.split(15, 0, 1, 2), S.leaf(1), S.leaf(1))):
        with pytest.raises(NotImplementedError):
            restate(script(4, 4, [np.ones((4, 4), np.int64)], nchan=1, tree=tree))


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_restatement(name):
    """CPU layer: the oracle's decode of every stream of the case is the restated image, sample for sample"""
    for tag, sc, data, want in prepared(name):
        nch = want.shape[2]
        got = to_ints(O.decode(data).pixels("f32", nch).view(np.float32), sc)
        compare(name, tag, got, want, "the oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_product_equals_restatement(jx, name):
    """GPU layer: the HIP decode of every stream of the case — one batch — is the restated image, sample for sample"""
    items = prepared(name)
    b = jx.BatchDecoder(0)
    for tag, sc, data, want in items:
        b.add(data, "float32", want.shape[2])
    b.prepare(); b.decode(); b.finish()
    for i, (tag, sc, data, want) in enumerate(items):
        compare(name, tag, to_ints(b.output(i), sc), want, "the HIP decode")
