"""The step between the tokens of a PassGroup section and the quantised coefficient planes, pinned to its DEFINITION: block context map with LF and
quantiser thresholds, predicted number of non-zeros, the 37 + 458 contexts per block context, natural and custom coefficient orders, histogram sets
("HF presets") and the shifts of several passes.

The restatement below (`tokens()` and what it calls) is plain Python and numpy integers written from the format's definitions; it imports nothing from
oracle/, the product or tools/.  A scripted writer (tools/synth_script_hf.h, synth_lib.encode_vardct_scripted) that computes no context, no order and
no count codes the (context, value) pairs `tokens()` says a set of coefficients must be coded as; every decoder then has to read those coefficients back.
Every case runs under two context maps of the AC code, context mod 256 and context div 256 (two distinct contexts differ under at least one), with
pseudo-counts that make the codes of any two clusters in use differ: a decoder that confuses two contexts reads another code.

Layers, all exact: the restatement reproduces the oracle's token trace of the two VarDCT streams libjxl itself wrote (the only link to the real
encoder: their ANS final-state check vouches for the trace); oracle == restatement per case (CPU); named wrong variants of the restatement are seen by
the case built for each (CPU); product == restatement per case and HF kernel (-m gpu).

The two 64-entry tables of the coefficient context model are DATA nothing here can re-derive: they are typed below as literals and asserted equal to the
oracle's copy (which was typed from the same source); what can be derived is asserted too (non-decreasing, every feasible context below 458).

Reachability, worked out from the definition: a block stores (nz + cx*cy - 1) >> log2(cx*cy) with nz <= 64*cx*cy - cx*cy, which is at most 63, and the first
block of a group predicts 32 — so a prediction never exceeds 63, the cap at 64 never acts and slot 36 of the 37 is unreachable in a valid stream.
The `counts` case asserts the 36 reachable slots (predictions 0 .. 63).

Case table (kernel = the HF kernel forced / the one asserted to have run; every case: two context maps = two streams per frame):
  every_strategy   27 frames, one strategy each                          wave, SIMT plain, SIMT tables-in-global, lane stride; SIMT all-LDS with the companion
  mixed_520x300    3x2 ragged groups, tall / wide / 64x64 at group edges  all five (SIMT all-LDS: see companion)
  counts           empty / full blocks, nz around size/16, predictions    all five
  magnitudes       +-1 .. +-32767 (64-symbol alphabets, 256 clusters)     the AC code is over the wave kernel's 150 KB and over the 64 KB LDS budget: SIMT tables-in-global runs; lane stride
  block_contexts   nctx 16, thresholds 1 / 2 / 1 and two on hf_mul        all five
  orders           every bucket custom, 32768 / 65536-entry tables        all five
  passes           two and three passes, own orders per pass             wave, SIMT plain and lane stride decline several passes: SIMT all-LDS runs; SIMT tables-in-global
  presets          two histogram sets over four groups, per pass          as passes (two passes)
"SIMT all-LDS" (HfDecodeSimtKernel<true, true, true>) is the launch's choice only when a frame of the batch has several passes or subsampled chroma: a
single-pass case reaches it with a COMPANION in its batch, a tiny two-pass scripted frame (checked like the others)."""
import itertools

import numpy as np
import pytest

import oracle_lib as O
import synth_lib as S
from conftest import fixture_bytes

# ---- the format's tables -----------------------------------------------------------------------------------------------------------------------------
# strategy -> (cx, cy): 8x8 blocks covered horizontally / vertically
COVERED = [(1, 1), (1, 1), (1, 1), (1, 1), (2, 2), (4, 4), (1, 2), (2, 1), (1, 4), (4, 1), (2, 4), (4, 2), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1),
           (8, 8), (4, 8), (8, 4), (16, 16), (8, 16), (16, 8), (32, 32), (16, 32), (32, 16)]
# strategy -> order bucket: one per transform shape up to transposition; all 8x8 transforms that are not a plain DCT share bucket 1
BUCKET = [0, 1, 1, 1, 2, 3, 4, 4, 5, 5, 6, 6, 1, 1, 1, 1, 1, 1, 7, 8, 8, 9, 10, 10, 11, 12, 12]
BUCKET_SHAPE = [(1, 1), (1, 1), (2, 2), (4, 4), (2, 1), (4, 1), (4, 2), (8, 8), (8, 4), (16, 16), (16, 8), (32, 32), (32, 16)]     # (longer, shorter) side in blocks
DEFAULT_BLOCK_CTX = [0, 1, 2, 2, 3, 3, 4, 5, 6, 6, 6, 6, 6, 7, 8, 9, 9, 10, 11, 12, 13, 14, 14, 14, 14, 14, 7, 8, 9, 9, 10, 11, 12, 13, 14, 14, 14, 14, 14]
# index 0 of both is never read (position 0 is an LF position; a scan with nothing left has ended)
FREQ_CTX = np.array([0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 15, 16, 16, 17, 17, 18, 18, 19, 19, 20, 20, 21, 21, 22, 22, 23, 23, 23, 23, 24, 24, 24, 24,
                     25, 25, 25, 25, 26, 26, 26, 26, 27, 27, 27, 27, 28, 28, 28, 28, 29, 29, 29, 29, 30, 30, 30, 30], np.int64)
NUM_NONZERO_CTX = np.array([0, 0, 31, 62, 62, 93, 93, 93, 93, 123, 123, 123, 123, 152, 152, 152, 152, 152, 152, 152, 152, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180, 180,
                            180, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206, 206,
                            206, 206], np.int64)


def log2(n):
    assert n & (n - 1) == 0
    return n.bit_length() - 1


def natural_order(long_blocks, short_blocks):
    """scan position -> coefficient position of a transform of long x short blocks, the longer side horizontal: the long * short lowest frequencies in row-major order,
    then the zig-zag over the square of the longer side of which only rows at a multiple of the side ratio exist.  Position = row * (8 * long) + column."""
    n, ratio = 8 * long_blocks, long_blocks // short_blocks
    llf, rest = {}, []
    for d in range(2 * n - 1):
        xs = range(max(0, d - n + 1), min(d, n - 1) + 1)
        for x in (xs if d % 2 == 0 else reversed(xs)):
            y = d - x
            if y % ratio:
                continue
            y //= ratio
            if x < long_blocks and y < short_blocks:
                llf[y * long_blocks + x] = y * n + x
            else:
                rest.append(y * n + x)
    return np.array([llf[i] for i in range(long_blocks * short_blocks)] + rest, np.int64)


_natural = {}


def natural_of_bucket(b):
    if b not in _natural:
        _natural[b] = natural_order(*BUCKET_SHAPE[b])
    return _natural[b]


def lehmer_to_permutation(code, skip, size):
    """code[i] (i >= skip, zero beyond the code's end) picks the code[i]-th smallest value not used yet"""
    left, perm = list(range(size)), []
    for i in range(size):
        perm.append(left.pop(code[i] if i >= skip and i < len(code) else 0))
    return perm


def block_ctx_parts(sc):
    if sc.get("block_ctx") is None:
        return [[], [], []], [], DEFAULT_BLOCK_CTX, 15
    tx, ty, tb, tq, m, nctx = sc["block_ctx"]
    return [list(tx), list(ty), list(tb)], list(tq), list(m), nctx


def groups_of(sc):
    return (sc["w"] + 255) // 256, (sc["h"] + 255) // 256


WRONG = ("prediction_without_plus_one", "thresholds_greater_or_equal", "prev_starts_flipped", "stored_count_rounded_down", "tall_not_transposed",
         "x_and_b_swapped_in_order_lookup", "shift_ignored")


def tokens(sc, wrong=None):
    """script -> (tok[pass][group] = (contexts, values), expected[varblock index] = (3, size) coefficients by coefficient position (X, Y, B), stats).
    sc["values"][pass][varblock index][channel X / Y / B]: dict scan position -> value, or a dense array over scan positions (None: all zero)."""
    assert wrong is None or wrong in WRONG
    lf_thr, qf_thr, bmap, nctx = block_ctx_parts(sc)
    num_lf = (len(lf_thr[0]) + 1) * (len(lf_thr[1]) + 1) * (len(lf_thr[2]) + 1)
    xg, yg = groups_of(sc)
    shifts = list(sc.get("shifts", ())) + [0]
    lfq = np.asarray(sc["lfq"])
    vbs = sc["varblocks"]
    by_group = {}
    for vi in sorted(range(len(vbs)), key=lambda i: (vbs[i][0], vbs[i][1])):                  # raster order of the top-left blocks
        by_group.setdefault((vbs[vi][0] // 32) * xg + vbs[vi][1] // 32, []).append(vi)
    expected = [np.zeros((3, 64 * COVERED[s][0] * COVERED[s][1]), np.int64) for _, _, s, _ in vbs]
    stats = dict(slots=set(), coef_ctx={}, cells=set(), predictions=set(), custom_buckets=set(), prev_start=set())
    above = (lambda v, t: v >= t) if wrong == "thresholds_greater_or_equal" else (lambda v, t: v > t)
    tok = []
    for ps, shift in enumerate(shifts):
        orders = (sc.get("orders") or [{}] * len(shifts))[ps] or {}
        presets = sc.get("presets")
        per_group = []
        for g in range(xg * yg):
            offset = 495 * nctx * (presets[ps][g] if presets is not None else 0)
            stored = np.zeros((3, 32, 32), np.int64)
            ctxs, vals = [], []
            for vi in by_group.get(g, []):
                by, bx, s, hf_mul = vbs[vi]
                cx, cy = COVERED[s]
                covered, size, bucket = cx * cy, 64 * cx * cy, BUCKET[s]
                l2 = log2(covered)
                gy, gx = by % 32, bx % 32
                b3 = [sum(above(int(lfq[c, by, bx]), t) for t in lf_thr[c]) for c in range(3)]
                lf_idx = (b3[0] * (len(lf_thr[2]) + 1) + b3[2]) * (len(lf_thr[1]) + 1) + b3[1]
                qf_idx = sum(above(hf_mul, t) for t in qf_thr)
                stats["cells"].add((qf_idx, lf_idx))
                for c in (1, 0, 2):                                                           # Y, X, B
                    slot_c = (0, 1, 2)[(1, 0, 2).index(c)]                                    # Y -> 0, X -> 1, B -> 2
                    block_ctx = bmap[((slot_c * 13 + bucket) * (len(qf_thr) + 1) + qf_idx) * num_lf + lf_idx]
                    # ---- the order of this pass, bucket and channel
                    oc = {0: 2, 1: 1, 2: 0}[c] if wrong == "x_and_b_swapped_in_order_lookup" else c
                    order = natural_of_bucket(bucket)
                    if wrong == "tall_not_transposed" and cy > cx:
                        rows, cols = 8 * cx, 8 * cy                                           # (the stored layout of the wide twin) read as if it were the tall one's
                        order = (order % cols) * rows + order // cols
                    if bucket in orders:
                        order = order[np.asarray(orders[bucket][oc], np.int64)]
                        stats["custom_buckets"].add((ps, bucket))
                    # ---- values over scan positions
                    given = sc["values"][ps][vi][c] if sc["values"][ps][vi] is not None else None
                    v = np.zeros(size, np.int64)
                    if isinstance(given, dict):
                        for k, val in given.items():
                            v[k] = val
                    elif given is not None:
                        v[:] = given
                    assert not v[:covered].any(), "the lowest frequencies are not coded here"
                    hit = np.flatnonzero(v)
                    nz = hit.size
                    # ---- predicted count
                    if gx == 0:
                        pred = 32 if gy == 0 else int(stored[c, gy - 1, gx])
                    elif gy == 0:
                        pred = int(stored[c, gy, gx - 1])
                    else:
                        pred = (int(stored[c, gy - 1, gx]) + int(stored[c, gy, gx - 1]) + (0 if wrong == "prediction_without_plus_one" else 1)) >> 1
                    stats["predictions"].add(pred)
                    pred = min(pred, 64)
                    slot = pred if pred < 8 else 4 + pred // 2
                    stats["slots"].add(slot)
                    ctxs.append(np.array([offset + block_ctx + nctx * slot])); vals.append(np.array([nz]))
                    stored[c, gy:gy + cy, gx:gx + cx] = (nz >> l2) if wrong == "stored_count_rounded_down" else (nz + covered - 1) >> l2
                    if nz:
                        last = int(hit[-1])
                        vv = v[covered:last + 1]
                        nonzero = (vv != 0).astype(np.int64)
                        left = nz - (np.cumsum(nonzero) - nonzero)
                        k = np.arange(covered, last + 1)
                        prev = np.empty_like(nonzero)
                        start = 1 if nz <= size // 16 else 0
                        prev[0] = 1 - start if wrong == "prev_starts_flipped" else start
                        prev[1:] = nonzero[:-1]
                        stats["prev_start"].add((size, int(prev[0])))
                        local = (NUM_NONZERO_CTX[(left + covered - 1) >> l2] + FREQ_CTX[k >> l2]) * 2 + prev
                        for u in np.unique(local):
                            stats["coef_ctx"].setdefault(size, set()).add(int(u))
                        ctxs.append(offset + 37 * nctx + 458 * block_ctx + local)
                        vals.append(np.where(vv >= 0, 2 * vv, -2 * vv - 1))
                        expected[vi][c][order[k]] += vv << (0 if wrong == "shift_ignored" else shift)
            per_group.append((np.concatenate(ctxs) if ctxs else np.zeros(0, np.int64), np.concatenate(vals) if vals else np.zeros(0, np.int64)))
        tok.append(per_group)
    return tok, expected, stats


def feasible_contexts(size):
    """{coefficient context (below 458): one (nz_left, k, prev) that yields it} over every state a scan of a transform of `size` coefficients can be in: at its first
    position prev is decided by the count, later both values occur; never more non-zeros left than positions"""
    covered = size // 64
    l2 = log2(covered)
    out = {}
    for k in range(covered, size):
        for left in range(1, size - k + 1):
            prevs = (1 if left <= size // 16 else 0,) if k == covered else (0, 1)
            for prev in prevs:
                ctx = int(NUM_NONZERO_CTX[(left + covered - 1) >> l2] + FREQ_CTX[k >> l2]) * 2 + prev
                out.setdefault(ctx, (left, k, prev))
    return out


def planes_of(sc, expected, coef_off=None):
    """(3, groups * 65536) planes: coefficient position p of varblock v lands at group * 65536 + coef_off + p.  coef_off: per varblock (the device's), or None: the
    varblocks of a group back to back in raster order of their top-left blocks (how the oracle's dump lays them out)."""
    xg, yg = groups_of(sc)
    vbs = sc["varblocks"]
    planes = np.zeros((3, xg * yg * 65536), np.int64)
    used = {}
    for vi in sorted(range(len(vbs)), key=lambda i: (vbs[i][0], vbs[i][1])):
        g = (vbs[vi][0] // 32) * xg + vbs[vi][1] // 32
        n = expected[vi].shape[1]
        off = used.get(g, 0) if coef_off is None else int(coef_off[vi])
        used[g] = used.get(g, 0) + n
        planes[:, g * 65536 + off:g * 65536 + off + n] = expected[vi]
    return planes


# ---- writing a script ---------------------------------------------------------------------------------------------------------------------------------
CONTEXT_MAPS = ("mod256", "div256")


def stream_of(sc, tok, which):
    _, _, _, nctx = block_ctx_parts(sc)
    n = 495 * nctx * sc.get("num_presets", 1)
    ctx = np.arange(n)
    cmap = ctx % 256 if which == "mod256" else ctx // 256
    # cluster c: one count on symbol 8 + c % 16, two on symbol 8 + c // 16 — a pair no other cluster has, below 32 so that the alias tables stay at 32 slots
    pseudo = [[(8 + c % 16, 1), (8 + c // 16, 2)] for c in range(int(cmap.max()) + 1)]
    data, dist = S.encode_vardct_scripted(sc["w"], sc["h"], sc["varblocks"], sc["lfq"], tok, cmap, block_ctx=sc.get("block_ctx"), shifts=sc.get("shifts", ()),
                                          orders=sc.get("orders"), num_presets=sc.get("num_presets", 1), presets=sc.get("presets"), pseudo_counts=pseudo)
    # no two clusters in use (in the same pass) share a distribution
    for ps, per_group in enumerate(tok):
        used = np.unique(cmap[np.concatenate([c for c, _ in per_group])])
        rows = {dist[ps, c].tobytes() for c in used}
        assert len(rows) == used.size, (which, ps, used.size, len(rows))
    return data, dist


# ---- scripts --------------------------------------------------------------------------------------------------------------------------------------------
def tiling(bw, bh, placed, rng=None, fill=(0,)):
    """`placed` (by, bx, strategy) + the rest of the grid filled greedily with strategies of `fill` (the first that fits, drawn by rng; 8x8 ones always fit)"""
    taken = np.zeros((bh, bw), bool)
    out = []

    def fits(by, bx, s):
        cx, cy = COVERED[s]
        return bx + cx <= bw and by + cy <= bh and bx % 32 + cx <= 32 and by % 32 + cy <= 32 and not taken[by:by + cy, bx:bx + cx].any()
    for by, bx, s in placed:
        assert fits(by, bx, s), (by, bx, s)
        taken[by:by + COVERED[s][1], bx:bx + COVERED[s][0]] = True
        out.append((by, bx, s))
    for by in range(bh):
        for bx in range(bw):
            if taken[by, bx]:
                continue
            cand = list(fill) if rng is None else [fill[i] for i in rng.permutation(len(fill))]
            s = next((s for s in cand if fits(by, bx, s)), 0)
            taken[by:by + COVERED[s][1], bx:bx + COVERED[s][0]] = True
            out.append((by, bx, s))
    return out


def sparse_values(rng, vbs, density=0.02, amplitude=3, cap=200):
    vals = []
    for _, _, s, _ in vbs:
        covered, size = COVERED[s][0] * COVERED[s][1], 64 * COVERED[s][0] * COVERED[s][1]
        per = []
        for c in range(3):
            n = min(cap, int(rng.binomial(size - covered, density)))
            ks = covered + rng.choice(size - covered, n, replace=False)
            v = rng.integers(1, amplitude + 1, n) * rng.choice([-1, 1], n)
            per.append({int(k): int(x) for k, x in zip(ks, v)})
        vals.append(per)
    return vals


def script(w, h, placed, rng, fill=(0,), hf=lambda rng: int(rng.integers(1, 41)), **kw):
    bw, bh = (w + 7) // 8, (h + 7) // 8
    vbs = [(by, bx, s, hf(rng)) for by, bx, s in tiling(bw, bh, placed, rng, fill)]
    sc = dict(w=w, h=h, varblocks=vbs, lfq=rng.integers(-40, 41, (3, bh, bw)), **kw)
    return sc


def case_every_strategy():
    out = []
    for s in range(27):
        rng = np.random.default_rng(100 + s)
        side = 64 if max(COVERED[s]) <= 4 else 256
        sc = script(side, side, [], rng, fill=(s,))
        assert all(v[2] == s for v in sc["varblocks"])
        sc["values"] = [sparse_values(rng, sc["varblocks"], 0.03 if side == 64 else 0.004)]
        out.append(sc)
    return out


def case_mixed():
    rng = np.random.default_rng(7)
    placed = [(24, 24, 18), (0, 28, 19), (28, 32, 20), (0, 0, 18), (8, 56, 19), (32, 0, 20), (32, 56, 20), (34, 28, 10)]      # 64x64, tall 32x64, wide 64x32 at group edges
    sc = script(520, 300, placed, rng, fill=(0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17))
    sc["values"] = [sparse_values(rng, sc["varblocks"], 0.05)]
    return [sc]


def witness_block(size, left, k, prev):
    """a scan that passes through (left non-zeros left at position k with `prev`)"""
    covered = size // 64
    v = {}
    if k > covered and prev == 1:
        v[k - 1] = 1
    for i in range(left):
        v[k + i] = -1 if i % 2 else 2
    return v


def case_counts():
    rng = np.random.default_rng(11)
    # groups 0 and 1: rows of DCT8 blocks whose counts grow with the row — first column predicts the row above, the rest (above + left + 1) >> 1: 0 .. 63 all occur
    # groups 2 and 3: a witness block for every feasible coefficient context of 64-, 128- and 256-coefficient transforms; empty blocks fill the rest
    wit = {size: list(feasible_contexts(size).values()) for size in (64, 128, 256)}
    extra = {size: [(size // 16, size // 64, None), (size // 16 + 1, size // 64, None), (size - size // 64, size // 64, None)] for size in (64, 128, 256)}    # both sides of size / 16, full
    strat = {64: 0, 128: 6, 256: 4}
    placed, want = [], {}
    cursor = {2: [0, 0], 3: [0, 0]}

    def put(group, s):
        cx, cy = COVERED[s]
        cur = cursor[group]
        if cur[1] + cx > 32:
            cur[0] += 2; cur[1] = 0
        by, bx = cur[0], group * 32 + cur[1]
        cur[1] += cx
        assert by + cy <= 32
        placed.append((by, bx, s))
        return by, bx
    for size, group in ((64, 2), (128, 2), (256, 3)):
        items = wit[size] + extra[size]
        for i in range(0, len(items), 3):
            want[put(group, strat[size])] = (size, items[i:i + 3])
    sc = script(1024, 256, placed, rng)
    vals = []
    for by, bx, s, _ in sc["varblocks"]:
        if (by, bx) in want:
            size, items = want[(by, bx)]
            per = [{}, {}, {}]
            for c, (left, k, prev) in zip((1, 0, 2), items):
                per[c] = witness_block(size, left, k, 0 if prev is None else prev)
            vals.append(per)
        elif bx < 64:
            nz = by + (32 if bx >= 32 else 0)
            vals.append([{1 + i: 1 + (i + c) % 2 for i in range(nz)} for c in range(3)])
        else:
            vals.append(None)
    sc["values"] = [vals]
    return [sc]


def case_magnitudes():
    rng = np.random.default_rng(13)
    sc = script(64, 64, [(0, 0, 4), (0, 2, 5)], rng, fill=(0, 6, 7))
    vals = sparse_values(rng, sc["varblocks"], 0.1, amplitude=2)
    big = [1, -1, 2, -2, 255, -256, 4095, -4096, 32767, -32767]
    for i, per in enumerate(vals):
        size = 64 * COVERED[sc["varblocks"][i][2]][0] * COVERED[sc["varblocks"][i][2]][1]
        for c in range(3):
            per[c][size - 1 - c] = big[(i + c) % len(big)]                      # a run of zeros in front of it: both values of prev
            per[c][size // 64 + (i % 5)] = big[(i + 2 * c + 3) % len(big)]
    sc["values"] = [vals]
    return [sc]


def case_block_contexts():
    rng = np.random.default_rng(17)
    tx, ty, tb, tq = [-2], [-1, 3], [0], [5, 100]
    n = 39 * 12 * 3
    bmap = [(7 * i + i // 16) % 16 for i in range(n)]
    combos = list(itertools.product((-3, -2, -1), (-2, -1, 0, 2, 3, 4), (-1, 0, 1), (4, 5, 6, 99, 100, 101)))       # each threshold: one below, at it, one above
    sc = script(256, 256, [], rng, fill=(0, 0, 0, 0, 1, 4, 6, 7, 12))
    sc["block_ctx"] = (tx, ty, tb, tq, bmap, 16)
    vbs = []
    for i, (by, bx, s, _) in enumerate(sc["varblocks"]):
        x, y, b, hf = combos[i % len(combos)]
        sc["lfq"][:, by, bx] = (x, y, b)
        vbs.append((by, bx, s, hf))
    sc["varblocks"] = vbs
    sc["values"] = [sparse_values(rng, vbs, 0.05)]
    return [sc]


def order_permutations(rng, bucket, kinds):
    size = S.ORDER_BUCKET_SIZE[bucket]
    skip = size // 64
    head = min(size, 64 if skip < 64 else skip + 64)
    out = []
    for kind in kinds:
        p = np.arange(size)
        if kind == "reversed":                     # the largest Lehmer codes
            p[skip:] = p[skip:][::-1]
        elif kind == "head":                       # swaps inside the first 64 scan positions only (the 64 behind the lowest frequencies where those fill the first 64)
            p[skip:head] = skip + rng.permutation(head - skip)
        elif kind == "tail":                       # swaps beyond them only
            hi = min(size, head + 900)
            if hi > head:
                p[head:hi] = head + rng.permutation(hi - head)
            else:
                p[skip:] = p[skip:][::-1]
        elif kind == "cut":                        # identity from some point on: the code's end is cut short
            p[skip:skip + 9] = p[skip:skip + 9][::-1]
        elif kind == "shuffled":
            p[skip:] = skip + rng.permutation(size - skip)
        out.append(p)
    return tuple(out)


def case_orders():
    rng = np.random.default_rng(19)
    # frame A: every bucket but the two largest, one mask with buckets 0, 2, 5 natural and the others custom; frame B: the 65536- and 32768-entry orders (swaps near
    # the front and a cut end only: a quadratic Lehmer decode of a long code costs seconds)
    placed = [(0, 0, 21), (0, 16, 22), (0, 24, 22), (16, 0, 23), (24, 0, 23), (16, 16, 18), (16, 24, 19), (16, 28, 19), (24, 16, 20), (28, 16, 20), (24, 24, 5), (24, 28, 10),
              (24, 30, 8), (24, 31, 8), (28, 24, 11), (30, 24, 9), (31, 24, 9), (28, 28, 4), (28, 30, 6), (28, 31, 6), (30, 28, 7), (30, 30, 7), (31, 28, 1), (31, 29, 12),
              (31, 30, 14), (31, 31, 0)]
    a = script(256, 256, placed, rng)
    kinds = {1: ("reversed", "head", "cut"), 3: ("tail", "reversed", "shuffled"), 4: ("head", "tail", "reversed"), 6: ("shuffled", "cut", "tail"),
             7: ("reversed", "tail", "head"), 8: ("tail", "shuffled", "cut"), 9: ("tail", "head", "cut"), 10: ("cut", "tail", "head")}
    a["orders"] = [{b: order_permutations(rng, b, k) for b, k in kinds.items()}]
    a["values"] = [sparse_values(rng, a["varblocks"], 0.01)]
    b = script(768, 272, [(0, 0, 24), (0, 32, 25), (0, 48, 25), (0, 64, 26), (16, 64, 26)], rng, fill=(0, 4, 9))
    b["orders"] = [{0: order_permutations(rng, 0, ("reversed", "shuffled", "head")), 2: order_permutations(rng, 2, ("shuffled", "reversed", "tail")),
                    5: order_permutations(rng, 5, ("reversed", "cut", "shuffled")),
                    11: order_permutations(rng, 11, ("head", "tail", "cut")), 12: order_permutations(rng, 12, ("tail", "cut", "head"))}]
    b["values"] = [sparse_values(rng, b["varblocks"], 0.003)]
    for sc in (a, b):                               # and something at the very end of every scan
        for i, (_, _, s, _) in enumerate(sc["varblocks"]):
            size = 64 * COVERED[s][0] * COVERED[s][1]
            for c in range(3):
                sc["values"][0][i][c][size - 1 - c] = 1 + c
    return [a, b]


def case_passes():
    out = []
    for shifts, seed in (((2,), 23), ((3, 1), 29)):
        rng = np.random.default_rng(seed)
        sc = script(264, 72, [(0, 0, 5), (0, 4, 10), (0, 6, 11), (4, 4, 4), (4, 6, 6), (4, 7, 7), (0, 32, 2)], rng, fill=(0, 0, 1, 4, 6, 7, 13))
        sc["shifts"] = shifts
        sc["orders"], sc["values"] = [], []
        for ps in range(len(shifts) + 1):
            buckets = [(0, 2, 4), (1, 3, 4, 6), (0, 1)][ps]
            sc["orders"].append({b: order_permutations(rng, b, [("shuffled", "reversed", "tail"), ("head", "shuffled", "cut"), ("reversed", "tail", "shuffled")][ps]) for b in buckets})
            vals = sparse_values(rng, sc["varblocks"], 0.06)
            for i, per in enumerate(vals):
                for c in range(3):
                    per[c].pop(63, None)
                    if ps == len(shifts):
                        per[c][63] = -3 - c                    # scan position 63 is touched by the last pass only
            sc["values"].append(vals)
        out.append(sc)
    return out


def case_presets():
    rng = np.random.default_rng(31)
    sc = script(512, 512, [], rng, fill=(5, 5, 18, 4))
    sc["shifts"] = (1,)
    sc["num_presets"] = 2
    sc["presets"] = [[0, 1, 1, 0], [1, 1, 0, 1]]
    sc["values"] = [sparse_values(rng, sc["varblocks"], 0.01) for _ in range(2)]
    return [sc]


def companion():
    """the tiny two-pass frame that makes a batch's HF launch take the several-passes instantiation"""
    rng = np.random.default_rng(37)
    sc = script(16, 8, [], rng)
    sc["shifts"] = (1,)
    sc["values"] = [sparse_values(rng, sc["varblocks"], 0.2) for _ in range(2)]
    return sc


# case -> (builder, several passes?, AC code too large for the wave kernel and the default LDS budget?)
CASES = {"every_strategy": (case_every_strategy, False, False), "mixed_520x300": (case_mixed, False, False), "counts": (case_counts, False, False),
         "magnitudes": (case_magnitudes, False, True), "block_contexts": (case_block_contexts, False, False), "orders": (case_orders, False, False),
         "passes": (case_passes, True, False), "presets": (case_presets, True, False)}
_built = {}


def built_case(name):
    """[(script, expected per varblock, stats, {map: stream})]"""
    if name not in _built:
        out = []
        for sc in (CASES[name][0]() if name != "companion" else [companion()]):
            tok, expected, stats = tokens(sc)
            streams = {}
            for which in CONTEXT_MAPS:
                streams[which], dist = stream_of(sc, tok, which)
                stats["alphabet"] = max(stats.get("alphabet", 0), int(np.flatnonzero(dist.any(axis=(0, 1))).max()) + 1)
            out.append((sc, tok, expected, stats, streams))
        _built[name] = out
    return _built[name]


def merged(name, key):
    out = set()
    for _, _, _, stats, _ in built_case(name):
        v = stats[key]
        out |= set().union(*v.values()) if isinstance(v, dict) else v
    return out


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------------------
def test_context_tables_are_the_oracles_and_what_can_be_derived_holds():
    freq, nzc = O.coeff_context_tables()
    assert np.array_equal(freq[1:], FREQ_CTX[1:]) and np.array_equal(nzc[1:], NUM_NONZERO_CTX[1:])       # (entry 0 is never read: the oracle keeps a poison value there)
    assert (np.diff(FREQ_CTX[1:]) >= 0).all() and (np.diff(NUM_NONZERO_CTX[1:]) >= 0).all()
    # every transform size: never more non-zeros left than positions, so with n' = ceil(left / covered) and k' = k >> log2(covered): n' <= 64 - k' (and <= 63)
    reachable = max(int(NUM_NONZERO_CTX[n] + FREQ_CTX[k]) * 2 + 1 for k in range(1, 64) for n in range(1, min(63, 64 - k) + 1))
    assert reachable < 458, reachable
    for size in (64, 128, 256, 512):
        f = feasible_contexts(size)
        assert 0 <= min(f) and max(f) <= reachable, (size, max(f))
    assert len(COVERED) == len(BUCKET) == 27 and sorted(set(BUCKET)) == list(range(13))
    for s in range(27):
        assert sorted(COVERED[s], reverse=True) == list(BUCKET_SHAPE[BUCKET[s]])
    for b in range(13):
        n = natural_of_bucket(b)
        assert n.size == S.ORDER_BUCKET_SIZE[b] and np.array_equal(np.sort(n), np.arange(n.size))
    assert lehmer_to_permutation([0, 0, 2, 0, 1], 1, 6) == [0, 1, 4, 2, 5, 3]


# ---- libjxl's own streams -------------------------------------------------------------------------------------------------------------------------------
# what the two files contain: (order buckets of the strategies present, used_orders mask of the one pass, block contexts)
LIBJXL_FIXTURES = {"sample_grey.jxl": ({0, 1, 4}, 0b10, 15), "sample_jpg.jxl": ({0}, 0b1, 2)}


@pytest.mark.parametrize("name", sorted(LIBJXL_FIXTURES))
def test_restatement_reproduces_the_trace_of_libjxl_written_streams(name):
    """tokens() on the coefficients and metadata the oracle dumped of a stream libjxl wrote gives the very (context, value) pairs the oracle read — and those
    are right because the ANS state of every section ended where libjxl's encoder started it"""
    d = O.decode(fixture_bytes(name), dump=True)
    w, h = d.info.xsize, d.info.ysize
    bw, bh = (w + 7) // 8, (h + 7) // 8
    st, hm = d.ints("strategy").reshape(bh, bw), d.ints("hf_mul").reshape(bh, bw)
    vbs = [(by, bx, int(st[by, bx]), int(hm[by, bx])) for by in range(bh) for bx in range(bw) if st[by, bx] >= 0]
    nctx, lf_thr, qf_thr, bmap = O.block_ctx_map(d)
    (used, orders), = O.custom_orders(d)
    buckets, mask, want_nctx = LIBJXL_FIXTURES[name]
    assert ({BUCKET[v[2]] for v in vbs}, used, nctx) == (buckets, mask, want_nctx)
    sc = dict(w=w, h=h, varblocks=vbs, lfq=np.stack([d.ints("lfq%d" % c).reshape(bh, bw) for c in range(3)]), block_ctx=(lf_thr[0], lf_thr[1], lf_thr[2], qf_thr, bmap, nctx))
    perms = {}
    for b in range(13):
        if used >> b & 1:
            where = np.empty(S.ORDER_BUCKET_SIZE[b], np.int64)
            where[natural_of_bucket(b)] = np.arange(where.size)
            perms[b] = tuple(where[orders[(b, c)]] for c in range(3))                 # order = natural[perm]  <=>  perm = natural^-1[order]
            assert all(np.array_equal(p[:where.size // 64], np.arange(where.size // 64)) for p in perms[b])
    sc["orders"] = [perms]
    coeff = [d.ints("coeff%d" % c).astype(np.int64) for c in range(3)]
    vals, off = [], 0
    for _, _, s, _ in vbs:                                                           # one group: varblocks back to back
        size = 64 * COVERED[s][0] * COVERED[s][1]
        order = natural_of_bucket(BUCKET[s])
        per = []
        for c in range(3):
            o = order[perms[BUCKET[s]][c]] if BUCKET[s] in perms else order
            v = coeff[c][off + o]
            assert not v[:size // 64].any()
            per.append(v)
        vals.append(per)
        off += size
    sc["values"] = [vals]
    tok, expected, _ = tokens(sc)
    preset, ctxs, values = O.hf_trace(d)[(0, 0)]
    assert preset == 0 and np.array_equal(tok[0][0][0], ctxs) and np.array_equal(tok[0][0][1], values), name
    assert np.array_equal(planes_of(sc, expected), np.stack(coeff))


# ---- oracle == restatement ------------------------------------------------------------------------------------------------------------------------------
def oracle_planes(data, sc):
    d = O.decode(data, dump=True)
    bw, bh = (sc["w"] + 7) // 8, (sc["h"] + 7) // 8
    st, hm = d.ints("strategy").reshape(bh, bw), d.ints("hf_mul").reshape(bh, bw)
    for by, bx, s, hf in sc["varblocks"]:
        assert (st[by, bx], hm[by, bx]) == (s, hf)
        cx, cy = COVERED[s]
        assert (hm[by:by + cy, bx:bx + cx] == hf).all() and (np.where(st < 0, -1 - st, st)[by:by + cy, bx:bx + cx] == s).all()
    assert (st >= 0).sum() == len(sc["varblocks"])
    assert np.array_equal(np.stack([d.ints("lfq%d" % c).reshape(bh, bw) for c in range(3)]), sc["lfq"])
    return np.stack([d.ints("coeff%d" % c).astype(np.int64) for c in range(3)]), d


@pytest.mark.parametrize("case", sorted(CASES) + ["companion"])
def test_oracle_equals_restatement(case):
    for sc, tok, expected, stats, streams in built_case(case):
        want = planes_of(sc, expected)
        for which in CONTEXT_MAPS:
            got, d = oracle_planes(streams[which], sc)
            assert np.array_equal(got, want), (case, which, int((got != want).sum()))
            trace = O.hf_trace(d)
            xg, yg = groups_of(sc)
            for ps in range(len(tok)):
                for g in range(xg * yg):
                    assert np.array_equal(trace[(ps, g)][1], tok[ps][g][0]) and np.array_equal(trace[(ps, g)][2], tok[ps][g][1])
    if case != "companion":
        assert (stats["alphabet"] > 32) == CASES[case][2], stats["alphabet"]


def test_the_cases_reach_their_classes():
    """the classes PARITY.md counts per case"""
    assert len(built_case("every_strategy")) == 27
    # counts: the 36 reachable slots (module docstring), predictions 7, 8, 9, 63 among 0 .. 63, every feasible coefficient context of the three sizes, both starts of prev per size
    assert merged("counts", "predictions") == set(range(64))
    assert merged("counts", "slots") == set(range(36))
    stats = built_case("counts")[0][3]
    for size in (64, 128, 256):
        assert stats["coef_ctx"][size] == set(feasible_contexts(size)), size
        assert {(size, 0), (size, 1)} <= stats["prev_start"]
    sc = built_case("counts")[0][0]
    counts = {}
    for (_, _, s, _), per in zip(sc["varblocks"], sc["values"][0]):
        size = 64 * COVERED[s][0] * COVERED[s][1]
        for c in range(3):
            counts.setdefault(size, set()).add(0 if per is None else len(per[c]))
    for size in (64, 128, 256):
        assert {size // 16, size // 16 + 1, size - size // 64} <= counts[size] and 0 in counts[64]
    # block contexts: every (quantiser cell, LF cell)
    assert merged("block_contexts", "cells") == set(itertools.product(range(3), range(12)))
    # orders: every bucket carries a custom order somewhere; passes: the masks differ from pass to pass
    assert {b for _, b in merged("orders", "custom_buckets")} == set(range(13))
    for sc, *_ in built_case("passes"):
        masks = [sorted(o) for o in sc["orders"]]
        assert all(a != b for a, b in zip(masks, masks[1:]))
    assert len({tuple(p) for p in built_case("presets")[0][0]["presets"]}) == 2
    # mixed: the prediction is fed by 8x8 blocks and by multi-block transforms, both first-row / first-column and interior
    strategies = {v[2] for v in built_case("mixed_520x300")[0][0]["varblocks"]}
    assert {18, 19, 20} <= strategies and len(strategies) >= 15


# ---- the cases see every rule ---------------------------------------------------------------------------------------------------------------------------
DISCRIMINATED_BY = {"prediction_without_plus_one": "counts", "thresholds_greater_or_equal": "block_contexts", "prev_starts_flipped": "counts",
                    "stored_count_rounded_down": "mixed_520x300", "tall_not_transposed": "every_strategy", "x_and_b_swapped_in_order_lookup": "orders",
                    "shift_ignored": "passes"}


@pytest.mark.parametrize("wrong", WRONG)
def test_the_cases_discriminate(wrong):
    """a stream written from a wrong variant of the restatement: the oracle fails on it, or does not return what the variant expects, under at least one of the two maps"""
    seen = False
    for sc, _, _, _, _ in built_case(DISCRIMINATED_BY[wrong]):
        tok, expected, _ = tokens(sc, wrong)
        want = planes_of(sc, expected)
        for which in CONTEXT_MAPS:
            try:
                data, _ = stream_of(sc, tok, which)
                got, _ = oracle_planes(data, sc)
            except (O.OracleError, RuntimeError):
                seen = True
                continue
            seen |= not np.array_equal(got, want)
    assert seen, wrong


@pytest.mark.parametrize("shape", ["prefix", "lz77", "mixed_uint_configs", "log_alpha_8"])
def test_the_writers_code_shapes_keep_their_meaning(shape):
    """set_prefix, set_lz77_ac and set_code_shape(which="ac") apply to the scripted AC code as they do to the synthesiser's: the same pairs under another code, the same planes"""
    (sc, tok, expected, _, _), = built_case("magnitudes")
    try:
        if shape == "prefix":
            S.set_prefix(True)
        elif shape == "lz77":
            S.set_lz77_ac(True)
        elif shape == "mixed_uint_configs":
            S.set_code_shape(uint_configs="mixed", which="ac", seed=3)
        else:
            S.set_code_shape(min_log_alpha=8, which="ac")
        data, dist = S.encode_vardct_scripted(sc["w"], sc["h"], sc["varblocks"], sc["lfq"], tok, np.arange(495 * 15) // 256)
    finally:
        S.set_prefix(False); S.set_lz77_ac(False); S.set_code_shape()
    got, _ = oracle_planes(data, sc)
    assert np.array_equal(got, planes_of(sc, expected)) and (dist.sum(axis=2) == 4096).all()


# ---- the synthesiser's custom_orders parameter ------------------------------------------------------------------------------------------------------------
def test_custom_orders_parameter_defaults_to_natural_orders_and_sorts_by_frequency():
    import hashlib
    import json
    import os
    from conftest import GOLDEN
    manifest = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    data = S.encode_vardct(S.synthetic_image(42, 300, 200), seed=9, strategy_mix=2, epf_iters=2, gab=1)
    assert hashlib.sha256(data).hexdigest() == manifest["vardct_300x200_mix2_epf2"]["sha256_stream"]          # the default writes the bytes it always wrote
    img = S.synthetic_image(13, 520, 300)
    plain = O.decode(S.encode_vardct(img, seed=13, strategy_mix=2, epf_iters=0, gab=0, num_passes=2), dump=True)
    custom = O.decode(S.encode_vardct(img, seed=13, strategy_mix=2, epf_iters=0, gab=0, num_passes=2, custom_orders=1), dump=True)
    for c in range(3):
        assert np.array_equal(plain.ints("coeff%d" % c), custom.ints("coeff%d" % c))
    assert [u for u, _ in O.custom_orders(plain)] == [0, 0]
    per_pass = O.custom_orders(custom)
    assert len(per_pass) == 2 and all(u != 0 for u, _ in per_pass)
    assert any(not np.array_equal(per_pass[0][1][k], per_pass[1][1][k]) for k in per_pass[0][1])                 # each pass sorts by its own statistics
    assert custom.info.tokens_hf < plain.info.tokens_hf                                                            # a better order ends the scans earlier


# ---- product == restatement -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jx(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import jpegxl_rs_amd as jx
    return jx


# kernels.h kHfVar*: HfDecodeWaveKernel, HfDecodeSimtKernel<true, false, false> / <true, true, true> / <false, true, true>, HfDecodeKernel (lane stride).
# name -> (variant bit, setup, needs a several-passes frame in the batch)
HF_KERNELS = {
    "wave": (1, lambda b: (b.set_lane_stride(8, 1), b.set_option("hf_lanes_per_wave", 1)), False),
    "simt_plain": (2, lambda b: b.set_lane_stride(8, 1), False),
    "simt_all_lds": (4, lambda b: b.set_lane_stride(8, 1), True),
    "simt_global": (8, lambda b: (b.set_lane_stride(8, 1), b.set_option("lds_code_budget", 0)), False),
    "lane_stride": (16, lambda b: b.set_lane_stride(8, 64), False),
}


def variant_that_runs(kernel, several_passes, b):
    """which kernel LaunchHfDecode takes for the batch (kernels.hip), from the sizes of the largest AC code of the batch: the wave kernel and the lane-stride kernel
    decline several passes (decoder.cc: only the SIMT kernel walks the passes), the wave kernel a code over 150 KB in its layout (10 bytes an alias slot: the cases here
    are far from that limit on either side), the plain SIMT instantiation several passes, both all-LDS instantiations a code over the LDS budget (64 KB by default)"""
    if kernel == "lane_stride" and not several_passes:
        return 16
    if kernel == "wave" and not several_passes and b.info_value("ac_code_bytes") * 5 // 4 <= 140 * 1024:
        return 1
    if kernel == "simt_global" or b.info_value("ac_code_bytes_compact") > 64 * 1024:
        return 8
    return 4 if several_passes else 2


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", sorted(HF_KERNELS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_product_equals_restatement(jx, case, kernel):
    variant, setup, wants_passes = HF_KERNELS[kernel]
    _, several_passes, big_code = CASES[case]
    items = [(sc, expected, streams[which]) for sc, _, expected, _, streams in built_case(case) for which in CONTEXT_MAPS]
    if wants_passes and not several_passes:
        items += [(sc, expected, streams[which]) for sc, _, expected, _, streams in built_case("companion") for which in CONTEXT_MAPS]
        several_passes = True
    b = jx.BatchDecoder(0)
    for _, _, data in items:
        b.add(data, "float32", 3)
    setup(b)
    b.prepare()
    first = None
    for run in range(2):                                            # the same resident batch twice
        b.decode_part(1); b.decode_part(3); b.finish()
        ran = b.info_value("hf_variant")
        assert ran == variant_that_runs(kernel, several_passes, b), (case, kernel, ran)
        if big_code and kernel != "lane_stride":
            assert ran == 8, (case, kernel, ran)                    # 256 clusters of 64 slots: over the LDS budget and over the wave kernel's limit
        if case in ("mixed_520x300", "counts", "block_contexts", "orders"):
            assert ran == variant, (case, kernel, ran)              # these four reach all five
        planes = [np.stack([b.debug_read(i, "coeff", c, dtype=np.int32) for c in range(3)]) for i in range(len(items))]
        if first is None:
            first = planes
            for i, (sc, expected, _) in enumerate(items):
                bw, bh = (sc["w"] + 7) // 8, (sc["h"] + 7) // 8
                info = b.debug_read(i, "blk_info", dtype=np.uint32).reshape(bh, bw)
                coef_off = b.debug_read(i, "coef_off", dtype=np.uint32).reshape(bh, bw)
                offs = []
                for by, bx, s, hf in sc["varblocks"]:
                    word = int(info[by, bx])
                    assert (word & 31, (word >> 5) & 1, ((word >> 8) & 0xFF) + 1) == (s, 1, hf), (case, by, bx, word)
                    offs.append(int(coef_off[by, bx]))
                want = planes_of(sc, expected, offs)
                assert want.any()
                assert planes[i].shape == want.shape and np.array_equal(planes[i], want), (case, kernel, i, int((planes[i] != want).sum()))
        else:
            assert all(np.array_equal(p, q) for p, q in zip(first, planes)), (case, kernel, "second decode")


@pytest.mark.gpu
def test_custom_orders_of_the_synthesiser_decode_like_the_oracle(jx):
    """encode_vardct(custom_orders=1): 520x300, large and exotic transforms, two passes with orders of their own — u8 pixels through the batch and through one pipeline job"""
    data = S.encode_vardct(S.synthetic_image(13, 520, 300), seed=13, strategy_mix=2, epf_iters=1, gab=1, num_passes=2, custom_orders=1)
    d = O.decode(data, dump=True)
    assert all(u != 0 for u, _ in O.custom_orders(d))
    want = d.pixels("u8", 3)
    b = jx.BatchDecoder(0)
    b.add(data, "uint8", 3)
    b.prepare(); b.decode(); b.finish()
    assert np.array_equal(b.output(0).reshape(-1), want)
    p = jx.Pipeline(0, jobs_in_flight=1, reserve_frames=1, reserve_width=520, reserve_height=300)
    out = jx.PinnedBuffer(want.size)
    status, _ = p.wait(p.submit([data], "uint8", 3, host_ptrs=[out.ptr], capacities=[want.size]))
    assert status == [0] and np.array_equal(np.array(out.array), want)
    p.close()
