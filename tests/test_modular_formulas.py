"""The integer half of the Modular path against its definitions (PARITY.md "Modular integer stages").

`restate(script)` below is a Modular decoder without entropy coding, written from the format's definitions (ISO/IEC 18181-1: the MA-tree properties, the
predictors, the weighted predictor, the reversible colour transforms, the palette with its implicit entries, the delta-palette scan, Squeeze) in Python integers / int64 numpy.  It imports
nothing from oracle/ and nothing from the product.  The streams come from the scripted writer (tools/synth_script.h, synth_lib.encode_modular_scripted): the
caller decides the transforms, the tree and the value of every token, so the restatement knows what the image has to be — exactly.

Two layers over the same cases:  CPU (unmarked)  oracle == restate;   gpu-marked  product == restate.
Results are read off the f32 decode (samples are not clamped there): integer = rint(float64(x) * (2^bits - 1)), exact because every test asserts |sample| <= 2^20;
and every test asserts that no intermediate value reaches 2^28, so no case depends on overflow behaviour.  Every case asserts that its input holds the classes it
claims (index ranges, edge fall-backs, both branches) before anything is compared.

The weighted (self-correcting) predictor — predictor 6, property 15, its header — and Squeeze are restated too.  The writer takes tokens, so where a case wants
certain SAMPLES (within the nominal range, straddling +-4095, +-2^20) the restatement runs forward on the test side first (restate(forward=True): the token nearest to each
wanted sample); a wrong restatement then yields tokens whose decode by the oracle and the product is another image.  The predictor keeps two peaks of its own (WpStats):
what a decoder stores from sample to sample stays below 2^31 in every case (beyond that the format's 32-bit storage decides); the other intermediates may and, in one case, must
exceed 2^31.  Squeeze cases are squeezed on the test side with the same tendency function; what pins the function is that oracle and product, given those residuals, must
reconstruct the image the restatement reconstructs — a forward and an inverse that share a wrong tendency would agree with each other, not with them.

Not restated: LZ77, predictor 6 as the predictor of a delta palette, Squeeze whose channels ride in the section streams."""
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
PREDICTORS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13)      # all but the weighted one (which has cases of its own)


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
    raise NotImplementedError("predictor %d" % p)                          # 6, the weighted predictor, needs its state: scan_channel / Weighted


# ---- the weighted (self-correcting) predictor ---------------------------------------------------------------------------------------------------------
WP_DEFAULT = dict(p1=16, p2=10, p3=(7, 7, 7, 0, 0), w=(13, 12, 12, 12))
WP_SHAPE2 = dict(p1=20, p2=8, p3=(5, 9, 6, 3, 2), w=(10, 14, 9, 13))           # what the synthesiser's LF tree shape 2 spells out
WP_ZERO = dict(p1=0, p2=0, p3=(0, 0, 0, 0, 0), w=(0, 0, 0, 0))
WP_MAX = dict(p1=31, p2=31, p3=(31, 31, 31, 31, 31), w=(15, 15, 15, 15))
DIVIDE = tuple((1 << 24) // (i + 1) for i in range(64))


def floor_log2(v):
    assert v > 0
    return v.bit_length() - 1


class WpStats:
    """What the weighted predictor met in one script.  Two peaks: `stored` — true errors and accumulated error magnitudes, what a decoder keeps in 32-bit
    storage from sample to sample; `other` — every other intermediate up to the weighted sum (neighbours * 8, the four sub-predictions, the sums in front
    of their `>> 5`, the weighted sum in front of its product with the division table; that product itself takes 64 bits in any implementation and is left out)."""

    def __init__(self):
        self.stored = self.other = 0
        self.n = dict.fromkeys(("samples", "clamp", "no_clamp", "eshift0", "eshift_pos", "rshift0", "rshift_pos", "negative_average", "p15_pos", "p15_neg", "p15_zero"), 0)
        self.weights = set()

    def add(self, other):
        self.stored, self.other = max(self.stored, other.stored), max(self.other, other.other)
        for k in self.n:
            self.n[k] += other.n[k]
        self.weights |= other.weights
        return self


class Weighted:
    """State of one channel: the true errors of the row above and of this row, and per sub-predictor the error magnitudes of the same two rows, width + 2 each"""

    def __init__(self, header, w, stats):
        self.hd, self.w, self.st = header, w, stats
        self.err = [[0] * (w + 2) for _ in range(2)]
        self.sub = [[[0] * (w + 2) for _ in range(2)] for _ in range(4)]
        self.pred = [0, 0, 0, 0]
        self.avg = 0

    def predict(self, x, y, W, N, NE, NW, NN):
        """-> (the prediction in eighths, property 15)"""
        hd, st, n = self.hd, self.st, self.st.n
        cur, up = y & 1, (y & 1) ^ 1
        ne, nw = (x + 1 if x + 1 < self.w else x), (x - 1 if x > 0 else x)
        wt = []
        for i in range(4):
            rows = self.sub[i][up]
            e = rows[x] + rows[ne] + rows[nw]
            shift = max(0, floor_log2(e + 1) - 5)
            n["eshift_pos" if shift else "eshift0"] += 1
            wt.append(4 + ((hd["w"][i] * DIVIDE[e >> shift]) >> shift))
        st.weights.add(tuple(wt))
        W, N, NE, NW, NN = 8 * W, 8 * N, 8 * NE, 8 * NW, 8 * NN
        eW = self.err[cur][x - 1] if x > 0 else 0
        eN, eNW, eNE = self.err[up][x], self.err[up][nw], self.err[up][ne]
        p15 = eW
        for e in (eN, eNW, eNE):                                             # the largest magnitude, the first of equals
            if abs(e) > abs(p15):
                p15 = e
        n["p15_pos" if p15 > 0 else ("p15_neg" if p15 < 0 else "p15_zero")] += 1
        p3 = hd["p3"]
        inner = ((eW + eN + eNE) * hd["p1"], (eW + eN + eNW) * hd["p2"], eNW * p3[0] + eN * p3[1] + eNE * p3[2] + (NN - N) * p3[3] + (NW - W) * p3[4])
        self.pred = [W + NE - N, N - (inner[0] >> 5), W - (inner[1] >> 5), N - (inner[2] >> 5)]
        rshift = floor_log2(sum(wt)) - 4
        n["rshift_pos" if rshift else "rshift0"] += 1
        wt = [v >> rshift for v in wt]
        total = sum(wt)
        acc = (total >> 1) - 1 + sum(p * v for p, v in zip(self.pred, wt))
        avg = (acc * DIVIDE[total - 1]) >> 24
        st.other = max(st.other, abs(acc), max(abs(v) for v in inner), max(abs(v) for v in self.pred), max(abs(v) for v in (W, N, NE, NW, NN)))
        if ((eN ^ eW) | (eN ^ eNW)) <= 0:                                    # the three true errors do not share a sign
            avg = max(min(W, N, NE), min(max(W, N, NE), avg))
            n["clamp"] += 1
        else:
            n["no_clamp"] += 1
        if avg < 0:
            n["negative_average"] += 1
        n["samples"] += 1
        self.avg = avg
        return avg, p15

    def update(self, x, y, value):
        cur, up = y & 1, (y & 1) ^ 1
        value *= 8
        self.err[cur][x] = self.avg - value
        st = self.st
        st.stored = max(st.stored, abs(self.avg - value))
        for i in range(4):
            e = (abs(self.pred[i] - value) + 3) >> 3
            self.sub[i][cur][x] = e                                            # stored here, and added to the entry up and to the right
            self.sub[i][up][x + 1] += e
            st.stored = max(st.stored, self.sub[i][up][x + 1])


def uses_weighted(tree):
    return any(n[0] == 15 or (n[0] < 0 and n[1] == 6) for n in tree)


def property_value(p, chan, stream_id, x, y, W, N, NW, NE, NN, WW, prev_gradient, refs, max_error=0):
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
    if p == 15: return max_error                                           # the weighted predictor's largest neighbouring true error (0 in a stream without it)
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


def scan_channel(chan, w, h, tokens, tree, stream_id, refs, branch_count, wp=None, forward=None):
    """Raster scan of one channel: tree walk on the properties, value = token * multiplier + offset + prediction.  wp: (header, WpStats) when the stream's tree
    uses the weighted predictor — its state starts afresh with the channel and takes in every sample, whatever leaf the sample lands in.
    forward: test side — `tokens` holds the samples one would like; the token nearest to each is chosen and written into the array `forward`."""
    T = tokens.tolist()
    R = [r.tolist() for r in refs]
    state = Weighted(wp[0], w, wp[1]) if wp else None
    rows = []
    for y in range(h):
        row = [0] * w
        rows.append(row)
        trow = T[y]
        prev_gradient = 0
        for x in range(w):
            W, N, NW, NE, NN, WW, NEE = neighbours(rows, x, y, w)
            eighths, max_error = state.predict(x, y, W, N, NE, NW, NN) if state else (0, 0)
            n = 0
            while tree[n][0] >= 0:
                prop, val, left, right, _ = tree[n]
                n = left if property_value(prop, chan, stream_id, x, y, W, N, NW, NE, NN, WW, prev_gradient, R, max_error) > val else right
            _, pred, offset, mul_log, mul_bits = tree[n]
            branch_count[n] = branch_count.get(n, 0) + 1
            guess = (eighths + 3) >> 3 if pred == 6 else predict(pred, W, N, NW, NE, NN, WW, NEE)
            token = trow[x]
            if forward is not None:
                token = idiv(trow[x] - offset - guess, (mul_bits + 1) << mul_log)
                forward[y, x] = token
            row[x] = token * ((mul_bits + 1) << mul_log) + offset + guess
            if state:
                state.update(x, y, row[x])
            prev_gradient = W + N - NW
    return np.array(rows, np.int64).reshape(h, w)


def decode_stream(dims, tokens, tree, stream_id, peak, branch_count, wp=None, forward=None):
    """dims: (w, h, is_meta) per channel of the stream; tokens: one (h, w) int64 array each -> the decoded channels.  wp: (header, WpStats); forward: a list
    that takes the chosen tokens, one array per channel (test side, see scan_channel)"""
    out = []
    wp = wp if uses_weighted(tree) else None
    max_mul = max((n[4] + 1) << n[3] for n in tree if n[0] < 0)
    for c, (w, h, meta) in enumerate(dims):
        tok = tokens[c]
        assert tok.shape == (h, w), (tok.shape, (h, w))
        refs = [out[j] for j in range(c - 1, -1, -1) if dims[j] == dims[c]]   # (a palette never has the geometry of an image channel: is_meta is part of it)
        if forward is not None:
            forward.append(np.zeros((h, w), np.int64))
            out.append(peak.see(scan_channel(c, w, h, tok, tree, stream_id, refs, branch_count, wp, forward[-1])))
            continue
        peak.see(tok * max_mul)
        if len(tree) == 1 and tree[0][1] == 0:                               # a single Zero leaf: no neighbour takes part
            out.append(peak.see(tok * ((tree[0][4] + 1) << tree[0][3]) + tree[0][2]))
            continue
        out.append(peak.see(scan_channel(c, w, h, tok, tree, stream_id, refs, branch_count, wp)))
    return out


# ---- Squeeze ----------------------------------------------------------------------------------------------------------------------------------------------
class SqueezeStats:
    """Per direction ("h" / "v"): how often the tendency took each of its seven ways out — (branch, clamp) with branch "falling" (prev >= avg >= next),
    "rising" (prev <= avg <= next) and clamp "none", "first" (the first alone), "second" (the second, whatever the first did), or ("zero", "none") —
    the classes of diff (residual + tendency), and the last pairs whose `next` had to be their own average"""

    def __init__(self):
        self.n = {}

    def count(self, *key):
        self.n[key] = self.n.get(key, 0) + 1

    def add(self, other):
        for k, v in other.n.items():
            self.n[k] = self.n.get(k, 0) + v
        return self


TENDENCY_OUTCOMES = tuple((b, c) for b in ("falling", "rising") for c in ("none", "first", "second")) + (("zero", "none"),)


def smooth_tendency(prev, avg, nxt, stats=None, direction=None):
    outcome = ("zero", "none")
    diff = 0
    if prev >= avg >= nxt:
        diff = idiv(4 * prev - 3 * nxt - avg + 6, 12)
        first = diff - (diff & 1) > 2 * (prev - avg)
        if first:
            diff = 2 * (prev - avg) + 1
        second = diff + (diff & 1) > 2 * (avg - nxt)
        if second:
            diff = 2 * (avg - nxt)
        outcome = ("falling", "second" if second else ("first" if first else "none"))
    elif prev <= avg <= nxt:
        diff = idiv(4 * prev - 3 * nxt - avg - 6, 12)
        first = diff + (diff & 1) < 2 * (prev - avg)
        if first:
            diff = 2 * (prev - avg) - 1
        second = diff - (diff & 1) < 2 * (avg - nxt)
        if second:
            diff = 2 * (avg - nxt)
        outcome = ("rising", "second" if second else ("first" if first else "none"))
    if stats is not None:
        stats.count(direction, "tendency", *outcome)
    return diff


def unsqueeze_line(avg, res, stats=None, direction=None):
    """One row (or column) of averages and one of residuals -> the samples, pair by pair"""
    aw, rw = len(avg), len(res)
    assert aw in (rw, rw + 1)
    out = []
    for x in range(rw):
        a = avg[x]
        nxt = avg[x + 1] if x + 1 < aw else a                                 # the following average; the last pair of an even line has none
        prev = out[2 * x - 1] if x else a                                     # the second sample of the pair before, as reconstructed
        if stats is not None and x + 1 >= aw:
            stats.count(direction, "last pair without a next average")
        diff = res[x] + smooth_tendency(prev, a, nxt, stats, direction)
        if stats is not None:
            stats.count(direction, "diff", "even" if diff % 2 == 0 else ("positive odd" if diff > 0 else "negative odd"))
        first = a + idiv(diff, 2)                                             # avg = (first + second + (first > second)) >> 1: diff / 2 rounds towards zero
        out += [first, first - diff]
    if aw > rw:
        out.append(avg[rw])                                                   # odd length: the last sample was its own average
    return out


def squeeze_line(line):
    """Test side: the forward step that unsqueeze_line undoes (same tendency function)"""
    rw, aw = len(line) // 2, (len(line) + 1) // 2
    avg = [(line[2 * x] + line[2 * x + 1] + (line[2 * x] > line[2 * x + 1])) >> 1 for x in range(rw)] + line[2 * rw:]
    res = []
    for x in range(rw):
        nxt = avg[x + 1] if x + 1 < aw else avg[x]
        prev = line[2 * x - 1] if x else avg[x]
        res.append(line[2 * x] - line[2 * x + 1] - smooth_tendency(prev, avg[x], nxt))
    return avg, res


def unsqueeze(avg, res, horizontal, stats=None):
    """(h, aw) averages and (h, rw) residuals -> (h, aw + rw) samples; the vertical step is the same on columns"""
    if not horizontal:
        return unsqueeze(avg.T, res.T, True, stats if stats is None else _Vertical(stats)).T
    lines = [unsqueeze_line(a, r, stats, "h") for a, r in zip(avg.tolist(), res.tolist())]
    return np.array(lines, np.int64).reshape(avg.shape[0], avg.shape[1] + res.shape[1])


class _Vertical:
    def __init__(self, stats):
        self.stats = stats

    def count(self, direction, *key):
        self.stats.count("v", *key)


def squeeze(plane, horizontal):
    """Test side: (h, w) samples -> (averages, residuals)"""
    if not horizontal:
        a, r = squeeze(plane.T, True)
        return a.T, r.T
    h, w = plane.shape
    pairs = [squeeze_line(row) for row in plane.tolist()]
    return np.array([p[0] for p in pairs], np.int64).reshape(h, (w + 1) // 2), np.array([p[1] for p in pairs], np.int64).reshape(h, w // 2)


def default_squeeze_steps(dims):
    """The chain a stream with zero explicit steps stands for, from the channel list (no meta channels): chroma first when the first two channels are of one
    size, then all channels in place, alternating until neither side exceeds 8 — starting with a vertical step unless the image is wider than high"""
    nb = len(dims)
    (w, h) = dims[0][:2]
    steps = []
    if nb > 2 and dims[1][:2] == (w, h):
        steps += [(True, False, 1, 2), (False, False, 1, 2)]
    if not w > h and h > 8:
        steps.append((False, True, 0, nb))
        h = (h + 1) // 2
    while w > 8 or h > 8:
        if w > 8:
            steps.append((True, True, 0, nb))
            w = (w + 1) // 2
        if h > 8:
            steps.append((False, True, 0, nb))
            h = (h + 1) // 2
    return steps


def squeeze_meta(dims, steps):
    """Channel-list bookkeeping of a Squeeze: every channel of a step shrinks to its averages; the residual channels go right behind the step's channels
    (in_place) or to the end of the list"""
    for horizontal, in_place, begin_c, num_c in steps:
        end_c = begin_c + num_c - 1
        assert 0 <= begin_c and end_c < len(dims)
        offset = end_c + 1 if in_place else len(dims)
        for c in range(begin_c, end_c + 1):
            w, h, meta = dims[c]
            assert not meta and w > 0 and h > 0
            dims[c] = ((w + 1) // 2, h, False) if horizontal else (w, (h + 1) // 2, False)
            dims.insert(offset + c - begin_c, (w // 2, h, False) if horizontal else (w, h // 2, False))


def inverse_squeeze(chs, steps, peak, stats):
    for horizontal, in_place, begin_c, num_c in reversed(steps):
        offset = begin_c + num_c if in_place else len(chs) - num_c
        for c in range(begin_c, begin_c + num_c):
            chs[c] = peak.see(unsqueeze(chs[c], chs[offset + c - begin_c], horizontal, stats))
        del chs[offset:offset + num_c]


def forward_squeeze(chs, steps):
    """Test side: the coded channel list (arrays) whose inverse Squeeze gives `chs`"""
    chs = list(chs)
    for horizontal, in_place, begin_c, num_c in steps:
        offset = begin_c + num_c if in_place else len(chs)
        for c in range(begin_c, begin_c + num_c):
            chs[c], res = squeeze(chs[c], horizontal)
            chs.insert(offset + c - begin_c, res)
    return chs


def transform_list(entries):
    """The writer's flat entries -> transforms: a run of Squeeze entries (synth_lib.squeeze) is one transform (2, steps), steps None for the default chain"""
    out = []
    for t in entries:
        if t[0] != 2:
            out.append(t)
        elif t[2] == 0:
            out.append((2, None))
        elif t[5] == 1:
            out[-1][1].append((bool(t[3]), bool(t[4]), t[1], t[2]))
        else:
            out.append((2, [(bool(t[3]), bool(t[4]), t[1], t[2])]))
    return out


def meta_apply(dims, t):
    """What a transform does to the channel list before decoding: a palette replaces its num_c channels by one index channel and puts itself in front"""
    if t[0] == 1:
        _, begin_c, num_c, nb_colors, _, _ = t
        del dims[begin_c + 1:begin_c + num_c]
        dims.insert(0, (nb_colors, num_c, True))
    if t[0] == 2:                                                            # a Squeeze: with the default chain the steps are fixed here, from the list as it stands
        if t[1] is None:
            t = (2, default_squeeze_steps(dims))
        squeeze_meta(dims, t[1])
    return t


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


def undo(chs, transforms, bits, peak, squeeze_stats=None):
    for t in reversed(transforms):
        if t[0] == 0:
            inverse_rct(chs, t[1], t[2], peak)
        elif t[0] == 2:
            inverse_squeeze(chs, t[1], peak, squeeze_stats)
        else:
            inverse_palette(chs, t, bits, peak)


class Stats:
    """What restate() met besides the samples: Peak, the samples per tree leaf, the weighted predictor's and the Squeeze's classes"""

    def __init__(self):
        self.peak, self.branch, self.wp, self.squeeze = Peak(), {}, WpStats(), SqueezeStats()


def restate(sc, forward=False):
    """-> (image (h, w, channels) int64, Peak, {tree node: samples that ended in that leaf}, Stats).
    forward=True (test side): sc["planes"] holds the SAMPLES one would like the coded channels to have -> the token planes that come nearest (see scan_channel)"""
    w, h, bits = sc["w"], sc["h"], sc["bits"]
    tree = sc.get("tree", (S.leaf(),))
    gt, lt = transform_list(sc.get("gt", ())), transform_list(sc.get("lt", ()))
    gwp, swp = sc.get("gwp") or WP_DEFAULT, sc.get("swp") or WP_DEFAULT
    gd = 128 << sc.get("shift", 1)
    xg, yg = -(-w // gd), -(-h // gd)
    num_lf_groups = (-(-w // (8 * gd))) * (-(-h // (8 * gd)))
    ntot = sc["nchan"] + (1 if sc.get("has_alpha") else 0)
    st = Stats()
    peak, branch = st.peak, st.branch
    planes = [np.asarray(p).astype(np.int64) for p in sc["planes"]]
    glist = [(w, h, False)] * ntot
    gt = [meta_apply(glist, t) for t in gt]
    nglobal = 0                                                              # GlobalModular: every meta channel, then every channel that fits a group
    while nglobal < len(glist) and (glist[nglobal][2] or (glist[nglobal][0] <= gd and glist[nglobal][1] <= gd)):
        nglobal += 1
    assert nglobal == len(glist) or not any(t[0] == 2 for t in gt), "squeezed channels in the sections: not restated"
    tokens = [] if forward else None
    chs = decode_stream(glist[:nglobal], planes[:nglobal], tree, 0, peak, branch, (gwp, st.wp), tokens)
    nrest = len(glist) - nglobal
    chs += [np.zeros((h, w), np.int64) for _ in range(nrest)]
    if forward:
        tokens += [np.zeros(p.shape, np.int64) for p in planes[nglobal:]]
    for g in range(xg * yg if nrest else 0):                                 # each group rectangle is a stream of its own
        x0, y0 = (g % xg) * gd, (g // xg) * gd
        rw, rh = min(gd, w - x0), min(gd, h - y0)
        ldims = [(rw, rh, False)] * nrest
        for t in lt:
            meta_apply(ldims, t)
        toks = [planes[nglobal + c] if d[2] else planes[nglobal + c][y0:y0 + rh, x0:x0 + rw] for c, d in enumerate(ldims)]
        chosen = [] if forward else None
        vals = decode_stream(ldims, toks, tree, 1 + 3 * num_lf_groups + 17 + g, peak, branch, (swp, st.wp), chosen)
        if forward:
            for c, d in enumerate(ldims):
                if d[2]:
                    tokens[nglobal + c][:] = chosen[c]
                else:
                    tokens[nglobal + c][y0:y0 + rh, x0:x0 + rw] = chosen[c]
            continue
        undo(vals, lt, bits, peak)
        assert len(vals) == nrest
        for k, v in enumerate(vals):
            chs[nglobal + k][y0:y0 + rh, x0:x0 + rw] = v
    if forward:
        return tokens
    undo(chs, gt, bits, peak, st.squeeze)
    assert len(chs) == ntot
    return np.stack(chs, axis=-1), peak, branch, st


# =====================================================================================================================================================
# Cases: name -> list of (tag, script).  A case asserts that its inputs hold the classes it is there for.
# =====================================================================================================================================================
CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def script(w, h, planes, bits=8, nchan=3, has_alpha=False, shift=1, gt=(), lt=(), tree=(S.leaf(),), local_tree=False, gwp=None, swp=None):
    """gwp / swp: weighted-predictor header (a dict like WP_DEFAULT) of the GlobalModular stream / of the section streams; None: the stream says it is the default one"""
    return dict(w=w, h=h, planes=planes, bits=bits, nchan=nchan, has_alpha=has_alpha, shift=shift, gt=tuple(gt), lt=tuple(lt), tree=tuple(tree), local_tree=local_tree,
                gwp=gwp, swp=swp)


def encode(sc):
    return S.encode_modular_scripted(sc["w"], sc["h"], sc["planes"], bits=sc["bits"], nchan=sc["nchan"], has_alpha=sc["has_alpha"], group_shift=sc["shift"],
                                     global_transforms=sc["gt"], local_transforms=sc["lt"], tree=sc["tree"], local_tree=sc["local_tree"],
                                     global_wp=sc["gwp"] and S.wp_header(**sc["gwp"]), section_wp=sc["swp"] and S.wp_header(**sc["swp"]))


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


# ---- the weighted predictor -----------------------------------------------------------------------------------------------------------------------------
CHECKS = {}                                                                    # case name -> check([(tag, script, Stats)]): the classes the case is there for
LF_CUTOFFS = (-500, -392, -255, -191, -127, -95, -63, -47, -31, -23, -15, -11, -7, -4, -3, -1, 0, 1, 3, 5, 7, 11, 15, 23, 31, 47, 63, 95, 127, 191, 255, 392, 500)
assert len(LF_CUTOFFS) == 33                                                   # the cut-offs on property 15 of a default-effort encoder's LF tree


def cutoff_tree(prop, cuts, predictor):
    """A balanced tree over `cuts` on one property, every leaf the same predictor"""
    nodes = []

    def build(lo, hi):
        me = len(nodes)
        nodes.append(None)
        if lo >= hi:
            nodes[me] = S.leaf(predictor)
        else:
            mid = (lo + hi) // 2
            left = build(mid + 1, hi)
            right = build(lo, mid)
            nodes[me] = S.split(prop, cuts[mid], left, right)
        return me
    build(0, len(cuts))
    return tuple(nodes)


WP_TREES = {
    "leaf6": (S.leaf(6),),
    "p15_over_6_and_5": (S.split(15, 0, 1, 2), S.leaf(6), S.leaf(5)),             # the state advances under the gradient leaf too
    "p15_over_5_and_1": (S.split(15, 0, 1, 2), S.leaf(5), S.leaf(1)),             # the predictor runs for the property alone
    "lf33": cutoff_tree(15, LF_CUTOFFS, 6),
    "offset_multiplier": (S.leaf(6, offset=-3, mul_log=1, mul_bits=2),),         # value = 6 * token - 3 + prediction
}


def wp_samples(seed, w, h, nch, kind, bits=8):
    """Samples one would like the channels to have.  "nominal": within [0, 2^bits), smooth + noise + a flat patch (small errors: error-weight shift 0);
    "signed": the same around 0; "straddle": +-4094 .. +-4097, both signs; "extreme": -2^20 or +2^20"""
    rng = np.random.default_rng(seed)
    top = (1 << bits) - 1
    if kind == "extreme":
        return [np.where(rng.integers(0, 2, (h, w)) == 1, 1 << 20, -(1 << 20)).astype(np.int64) for _ in range(nch)]
    if kind == "straddle":
        out = [(rng.integers(4094, 4098, (h, w)) * np.where(np.cumsum(rng.integers(0, 8, (h, w)) == 0, axis=1) % 2 == 1, -1, 1)).astype(np.int64) for _ in range(nch)]
        for v in out:
            v[0, :3] = np.clip(v[0, :3], -4095, 4095)                         # a channel begins within +-4095 and leaves that range later
        return out
    out = []
    for c in range(nch):
        yy, xx = np.mgrid[0:h, 0:w]
        smooth = top * (0.5 + 0.3 * np.sin(xx / 5.0 + c) * np.cos(yy / 7.0)) + rng.integers(-top // 6, top // 6 + 1, (h, w)) * (rng.integers(0, 3, (h, w)) > 0)
        v = np.clip(np.rint(smooth), 0, top).astype(np.int64)
        v[h // 2:h // 2 + 6, w // 3:w // 3 + 12] = top // 3 + c                # the flat patch
        out.append(v - top // 2 if kind == "signed" else v)
    return out


def wp_script(tag, w, h, kind, bits=8, nchan=1, alpha=True, shift=1, tree="leaf6", gwp=None, swp=None, seed=0):
    nch = nchan + (1 if alpha else 0)
    sc = script(w, h, wp_samples(seed + w * 7 + h, w, h, nch, kind, bits), bits=bits, nchan=nchan, has_alpha=alpha, shift=shift, tree=WP_TREES[tree], gwp=gwp, swp=swp)
    sc["planes"] = restate(sc, forward=True)                                  # the tokens that give those samples (the nearest ones under a multiplier)
    return (tag, sc)


WP_CLASSES = ("clamp", "no_clamp", "eshift0", "eshift_pos", "rshift_pos", "negative_average", "p15_pos", "p15_neg", "p15_zero")


def wp_union(items):
    total = WpStats()
    for _, _, st in items:
        total.add(st.wp)
    return total


def assert_wp_classes(items, classes=WP_CLASSES, share=()):
    """Over the case: every class met; per script named in `share`: the clamp taken and not taken on at least 5 % of the samples each"""
    total = wp_union(items)
    assert all(total.n[k] > 0 for k in classes), total.n
    for tag, sc, st in items:
        if tag in share:
            n = st.wp.n
            assert min(n["clamp"], n["no_clamp"]) >= 0.05 * n["samples"] > 0, (tag, n)
    for _, _, st in items:
        assert st.wp.stored < 1 << 31, "a stored error reaches 2^31: the result is not defined"


@case
def wp_geometries():
    return [wp_script("%dx%d" % (w, h), w, h, "signed", nchan=3) for w, h in ((1, 1), (1, 9), (9, 1), (2, 7), (37, 23))]


def _check_geometries(items):
    assert_wp_classes(items, share=("37x23",))
    sizes = {(sc["w"], sc["h"]) for _, sc, _ in items}
    assert {w for w, h in sizes} >= {1, 2} and {h for w, h in sizes} >= {1} and max(h for w, h in sizes) >= 3      # x = 0 = w - 1; rows 0, 1 and later ones
    assert all(st.wp.n["samples"] == sc["w"] * sc["h"] * 4 for _, sc, st in items)


CHECKS["wp_geometries"] = _check_geometries


@case
def wp_trees_37x23():
    return [wp_script("%s_%dbit" % (t, bits), 37, 23, "nominal", bits=bits, tree=t, seed=bits) for t in WP_TREES for bits in (8, 12, 16)]


def _check_trees(items):
    assert_wp_classes(items, classes=[k for k in WP_CLASSES if k != "negative_average"], share=[tag for tag, _, _ in items if tag.startswith("leaf6")])
    for tag, sc, st in items:
        leaves = [n for n, node in enumerate(sc["tree"]) if node[0] < 0]
        reached = [n for n in leaves if st.branch.get(n, 0) > 0]
        if tag.startswith("lf33"):
            assert len(leaves) == 34 and len(reached) >= (20 if sc["bits"] == 8 else 2), (tag, len(reached))              # 8 bits: property 15 on both sides of most cut-offs,
            assert all(st.branch.get(n, 0) > 0 for n in _extreme_leaves(sc["tree"])), tag                                 # beyond the outermost ones too
        else:
            assert reached == leaves and min(st.branch[n] for n in leaves) >= 0.05 * st.wp.n["samples"], (tag, st.branch)
        assert st.wp.n["samples"] == 37 * 23 * 2                              # the state advanced under every leaf


def _extreme_leaves(tree):
    """The leaves of a cutoff tree reached by always going left (property above every cut-off) and always right"""
    out = []
    for side in (2, 3):
        n = 0
        while tree[n][0] >= 0:
            n = tree[n][side]
        out.append(n)
    return out


CHECKS["wp_trees_37x23"] = _check_trees


@case
def wp_headers_37x23():
    headers = (("default", None), ("shape2", WP_SHAPE2), ("zero", WP_ZERO), ("maximum", WP_MAX))
    return [wp_script("%s_%dbit" % (name, bits), 37, 23, "signed", bits=bits, tree="p15_over_6_and_5", gwp=hd, seed=bits) for name, hd in headers for bits in (8, 16)]


def _check_headers(items):
    assert_wp_classes(items, share=("default_8bit", "shape2_8bit"))
    for tag, sc, st in items:
        if tag.startswith("zero"):
            assert st.wp.n["rshift_pos"] == 0 and st.wp.n["rshift0"] > 0 and st.wp.weights == {(4, 4, 4, 4)}, tag      # the only header whose weights add up to less than 32
        else:
            assert st.wp.n["rshift_pos"] > 0, tag


CHECKS["wp_headers_37x23"] = _check_headers


@case
def wp_four_groups():
    """150 x 140 in groups of 128: four section streams, each with the section header — which is not the global one"""
    return [wp_script("lf33_8bit_straddle", 150, 140, "straddle", bits=8, alpha=False, shift=0, tree="lf33", gwp=WP_MAX, swp=WP_SHAPE2),
            wp_script("p15_12bit", 150, 140, "nominal", bits=12, alpha=True, shift=0, tree="p15_over_6_and_5", gwp=WP_SHAPE2, swp=WP_MAX),
            wp_script("leaf6_16bit", 150, 140, "signed", bits=16, alpha=False, shift=0, tree="leaf6", gwp=WP_ZERO, swp=None)]


def _check_four_groups(items):
    assert_wp_classes(items, share=("p15_12bit", "leaf6_16bit"))
    for tag, sc, st in items:
        assert sc["gwp"] != sc["swp"] and st.wp.n["samples"] == 150 * 140 * (2 if sc["has_alpha"] else 1), tag
        other = restate(dict(sc, swp=sc["gwp"]))[0]                           # decoded with the global header the image is another one
        assert not np.array_equal(other, restate(sc)[0]), tag


CHECKS["wp_four_groups"] = _check_four_groups


@case
def wp_magnitudes():
    out = []
    for bits in (8, 12):
        out.append(wp_script("nominal_%dbit" % bits, 37, 23, "nominal", bits=bits, nchan=3, seed=1))
        out.append(wp_script("straddle_4095_%dbit" % bits, 37, 23, "straddle", bits=bits, nchan=3, seed=2))
        out.append(wp_script("straddle_4095_lf33_%dbit" % bits, 37, 23, "straddle", bits=bits, tree="lf33", gwp=WP_SHAPE2, seed=3))
        out.append(wp_script("extreme_maximum_header_%dbit" % bits, 37, 23, "extreme", bits=bits, gwp=WP_MAX, seed=4))
        out.append(wp_script("extreme_default_header_%dbit" % bits, 37, 23, "extreme", bits=bits, seed=5))
    return out


def _check_magnitudes(items):
    assert_wp_classes(items, share=[tag for tag, _, _ in items if tag.startswith("nominal")])
    for tag, sc, st in items:
        img = restate(sc)[0]
        if tag.startswith("nominal"):
            assert img.min() >= 0 and img.max() < 1 << sc["bits"], tag
        if tag.startswith("straddle"):
            assert set(np.unique(np.abs(img)).tolist()) == {4094, 4095, 4096, 4097} and (img < 0).any() and (img > 0).any(), tag
            first = min(int(np.argmax(np.abs(img[:, :, c]).ravel() > 4095)) for c in range(img.shape[2]))
            assert 3 <= first < 37, (tag, first)                              # the first sample beyond +-4095 comes after the channel has begun
        if tag.startswith("extreme"):
            assert set(np.unique(img).tolist()) == {-(1 << 20), 1 << 20}, tag
        if tag.startswith("extreme_maximum"):                                 # beyond 32 bits on the way, within them in what is kept
            assert st.wp.other >= 1 << 31 and st.wp.stored < 1 << 31, (tag, st.wp.other, st.wp.stored)


CHECKS["wp_magnitudes"] = _check_magnitudes


# ---- Squeeze --------------------------------------------------------------------------------------------------------------------------------------------
def squeeze_field(seed, w, h, nch):
    """Images for the Squeeze cases: monotone stretches, steps and noise in both directions (every way out of the tendency function), signed"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nch):
        gx = np.cumsum(rng.integers(-3, 9, (h, w)) * rng.choice((1, 1, 1, 40, -25), (h, w)), axis=1)
        gy = np.cumsum(rng.integers(-3, 9, (h, w)) * rng.choice((1, 1, 1, 40, -25), (h, w)), axis=0)
        out.append((gx + gy + rng.integers(-2, 3, (h, w)) - 300).astype(np.int64))
    return out


def squeeze_script(tag, w, h, steps, nchan=1, alpha=False, shift=1, rct_type=None, tree=(S.leaf(),), seed=0):
    """steps: explicit list or None (default chain).  The image is squeezed on the test side; with a tree that predicts, the tokens are chosen to give those channels"""
    nch = nchan + (1 if alpha else 0)
    img = squeeze_field(seed + 13 * w + h, w, h, nch)
    gt = []
    if rct_type is not None:
        img[:3] = forward_rct(img[0], img[1], img[2], rct_type)
        gt.append(S.rct(0, rct_type))
    resolved = steps if steps is not None else default_squeeze_steps([(w, h, False)] * nch)
    sc = script(w, h, forward_squeeze(img, resolved), bits=16, nchan=nchan, has_alpha=alpha, shift=shift, gt=gt + S.squeeze(steps), tree=tree)
    if tree != (S.leaf(),):
        sc["planes"] = restate(sc, forward=True)
    return (tag, sc)


SQUEEZE_LENGTHS = (1, 2, 3, 16, 17, 18, 19, 37)                                 # residual lengths 0, 1, 8, 9, 18; averages as long as the residuals and one longer


def assert_squeeze_classes(items, directions):
    total = SqueezeStats()
    for _, _, st in items:
        total.add(st.squeeze)
    for d in directions:
        for o in TENDENCY_OUTCOMES:
            assert total.n.get((d, "tendency") + o, 0) > 0, (d, o, total.n)
        for k in ("even", "positive odd", "negative odd"):
            assert total.n.get((d, "diff", k), 0) > 0, (d, k, total.n)
        assert total.n.get((d, "last pair without a next average"), 0) > 0, (d, total.n)
    return total


@case
def squeeze_lengths_horizontal():
    return [squeeze_script("w%d" % n, n, 6, [(True, True, 0, 1)]) for n in SQUEEZE_LENGTHS]


@case
def squeeze_lengths_vertical():
    return [squeeze_script("h%d" % n, 6, n, [(False, True, 0, 1)]) for n in SQUEEZE_LENGTHS]


CHECKS["squeeze_lengths_horizontal"] = lambda items: assert_squeeze_classes(items, "h")
CHECKS["squeeze_lengths_vertical"] = lambda items: assert_squeeze_classes(items, "v")


@case
def squeeze_chains():
    return [squeeze_script("h_v_h_on_the_averages", 37, 23, [(True, True, 0, 1), (False, True, 0, 1), (True, True, 0, 1)]),
            squeeze_script("three_channels_in_place", 37, 23, [(True, True, 0, 3), (False, True, 0, 3)], nchan=3),
            squeeze_script("three_channels_appended", 37, 23, [(True, False, 0, 3), (False, False, 0, 3)], nchan=3),
            squeeze_script("under_rct", 37, 23, [(True, True, 0, 3), (False, False, 1, 2)], nchan=3, rct_type=6),
            squeeze_script("under_rct_17", 19, 18, [(False, True, 0, 3), (True, True, 0, 3)], nchan=3, rct_type=17),
            squeeze_script("alpha_only", 37, 23, [(True, True, 3, 1), (False, True, 3, 1)], nchan=3, alpha=True),
            squeeze_script("default_chain_37x23", 37, 23, None, nchan=3),
            squeeze_script("default_chain_grey_alpha_23x37", 23, 37, None, nchan=1, alpha=True),
            squeeze_script("default_chain_300x280", 300, 280, None, nchan=1, shift=3)]


def _check_chains(items):
    assert_squeeze_classes(items, "hv")
    for tag, sc, st in items:
        if tag.startswith("default_chain"):
            nch = sc["nchan"] + (1 if sc["has_alpha"] else 0)
            steps = default_squeeze_steps([(sc["w"], sc["h"], False)] * nch)
            assert (steps[0] == (True, False, 1, 2)) == (nch > 2) and steps[2 if nch > 2 else 0][0] == (sc["w"] > sc["h"]), (tag, steps)
            assert len(sc["planes"]) == nch + sum(s[3] for s in steps) and max(sc["planes"][0].shape) <= 8, tag


CHECKS["squeeze_chains"] = _check_chains


@case
def squeeze_under_the_weighted_predictor():
    return [squeeze_script("leaf6", 37, 23, [(True, True, 0, 2), (False, True, 0, 2)], alpha=True, tree=WP_TREES["leaf6"]),
            squeeze_script("lf33_default_chain", 37, 23, None, nchan=3, tree=WP_TREES["lf33"])]


def _check_squeeze_wp(items):
    assert_squeeze_classes(items, "hv")
    assert_wp_classes(items)


CHECKS["squeeze_under_the_weighted_predictor"] = _check_squeeze_wp


# =====================================================================================================================================================
# The two layers
# =====================================================================================================================================================
_prepared = {}


def prepared(name):
    """[(tag, script, codestream, restated image)] of a case, computed once for both layers and left unchanged"""
    if name not in _prepared:
        items, met = [], []
        for tag, sc in CASES[name]():
            want, peak, branch, stats = restate(sc)
            assert np.abs(want).max() <= 1 << 20, (name, tag, "samples must stay within 2^20 for the f32 read-out to be exact")
            assert peak.intermediate_bound() < 1 << 28, (name, tag, "an intermediate value reaches 2^28")
            if name.startswith("properties_"):                               # both branches of the probe taken on at least 20 % of the samples each
                total = sum(branch.values())
                assert total == want.size and min(branch.get(1, 0), branch.get(2, 0)) >= 0.2 * total, (name, tag, branch)
            if name.startswith("predictors_two_level") or name.startswith("predictors_multipliers"):
                assert all(branch.get(n, 0) > 0 for n, node in enumerate(sc["tree"]) if node[0] < 0), (name, tag, "a leaf is never reached", branch)
            want.setflags(write=False)
            items.append((tag, sc, encode(sc), want))
            met.append((tag, sc, stats))
        if name in CHECKS:
            CHECKS[name](met)
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
    big = np.zeros((140, 150), np.int64)
    with pytest.raises(RuntimeError, match="Squeeze needs an image of at most one group"):
        S.encode_modular_scripted(150, 140, [big[:, :75], big[:, :75]], nchan=1, group_shift=0, global_transforms=S.squeeze([(True, True, 0, 1)]))
    with pytest.raises(RuntimeError, match="Squeeze in a section stream"):
        S.encode_modular_scripted(150, 140, [big[:, :75], big[:, :75]], nchan=1, group_shift=0, local_transforms=S.squeeze([(True, True, 0, 1)]))
    with pytest.raises(RuntimeError, match="plane 1 is 32x40, the coded channel is 0x40"):
        S.encode_modular_scripted(1, 40, [idx[:, :1], idx[:, :32]], nchan=1, global_transforms=S.squeeze([(True, True, 0, 1)]))
    with pytest.raises(RuntimeError, match="Squeeze of an empty channel"):
        S.encode_modular_scripted(1, 40, [idx[:, :1], idx[:, :0], idx[:, :0]], nchan=1, global_transforms=S.squeeze([(True, True, 0, 1), (True, True, 1, 1)]))
    with pytest.raises(RuntimeError, match="weights must be 0..15"):
        S.encode_modular_scripted(64, 40, [idx], nchan=1, global_wp=S.wp_header(w=(16, 0, 0, 0)))


def test_weights_are_four_when_every_maximum_weight_is_zero():
    """weight = 4 + ((max weight * table entry) >> shift): nothing but the 4 is left of it, whatever the errors"""
    rng = np.random.default_rng(1)
    sc = script(9, 7, [rng.integers(-300, 300, (7, 9))], nchan=1, tree=(S.leaf(6),), gwp=WP_ZERO)
    _, _, _, st = restate(sc)
    assert st.wp.weights == {(4, 4, 4, 4)} and st.wp.n["samples"] == 63 and st.wp.n["rshift0"] == 63      # 16 = 2^4: the weights are not scaled down
    _, _, _, st = restate(dict(sc, gwp=None))
    assert (4, 4, 4, 4) not in st.wp.weights and st.wp.n["rshift_pos"] == 63


@pytest.mark.parametrize("header", (WP_DEFAULT, WP_SHAPE2, WP_ZERO, WP_MAX))
def test_a_constant_channel_predicts_itself_from_the_second_row_on(header):
    """Sample (0, 0) is predicted 0 and leaves the true error -8 * value.  For a value >= 0 that error is negative or zero, every other true error is zero, so the
    three errors a later sample looks at never share a sign: the average is clamped to min / max of W, N, NE, all of them the constant — whatever the header.
    (A negative constant leaves a positive error, 0 and a positive number do share a sign by the format's test, and the average goes unclamped: checked as a round trip.)"""
    for value in (0, 1, 77, 4096, 1 << 20):
        want = np.full((6, 8), value, np.int64)
        sc = script(8, 6, [want], bits=16, nchan=1, tree=(S.leaf(6),), gwp=header)
        tokens = restate(sc, forward=True)[0]
        assert tokens[0, 0] == value and not tokens[1:].any() and not tokens[0, 1:].any(), (header, value, tokens)
    for value in (-5, -4096):
        want = np.full((6, 8), value, np.int64)
        sc = script(8, 6, [want], bits=16, nchan=1, tree=(S.leaf(6),), gwp=header)
        tokens = restate(sc, forward=True)
        got, _, _, st = restate(dict(sc, planes=tokens))
        assert np.array_equal(got[:, :, 0], want) and st.wp.n["no_clamp"] > 0


def test_inverse_squeeze_undoes_forward_squeeze():
    """Lengths 1 .. 19, both directions: the restated inverse gives back what the test's forward step (same tendency function) was given; steep, flat
    and monotone stretches, so that all seven ways out of the tendency function are taken"""
    rng = np.random.default_rng(5)
    stats = SqueezeStats()
    for n in range(1, 20):
        for horizontal in (True, False):
            walk = np.cumsum(rng.integers(-3, 9, (5, n)) * rng.choice((1, 1, 1, 40, -25), (5, n)), axis=1) + rng.integers(-2, 3, (5, n))
            plane = walk if horizontal else walk.T.copy()
            avg, res = squeeze(plane, horizontal)
            assert avg.shape[1 if horizontal else 0] == (n + 1) // 2 and res.shape[1 if horizontal else 0] == n // 2
            assert np.array_equal(unsqueeze(avg, res, horizontal, stats), plane), (n, horizontal)
    for d in "hv":
        assert all(stats.n.get((d, "tendency") + o, 0) > 0 for o in TENDENCY_OUTCOMES), stats.n
    chs = [rng.integers(-100, 100, (7, 11)) for _ in range(3)]
    steps = [(True, True, 0, 3), (False, False, 1, 2), (True, True, 0, 1)]
    coded = forward_squeeze(chs, steps)
    dims = [(11, 7, False)] * 3
    squeeze_meta(dims, steps)
    assert [(c.shape[1], c.shape[0]) for c in coded] == [d[:2] for d in dims] == [(3, 7), (3, 7), (6, 4), (6, 4), (5, 7), (5, 7), (5, 7), (6, 3), (6, 3)]
    inverse_squeeze(coded, steps, Peak(), None)
    assert len(coded) == 3 and all(np.array_equal(a, b) for a, b in zip(coded, chs))


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
