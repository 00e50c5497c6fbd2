"""Plain-numpy restatement of the adaptive-sampling calls (include/rt_abi.h: rt_sample_pixels, rt_sample_priority,
rt_sample_plan, rt_sample_resolve) for tests/test_adaptive_cpu.py and tests/test_gpu_adaptive.py.

rt_sample_pixels' yardstick is radiance_ref's: the oracle's oracle_sample_table gives, for a pixel and its initial
state, the colour and the number of draws of one camera sample started at every even draw offset.  A pixel that has
received N samples holds the fp32 sum, in order, of the N table rows of the chain o_0 = 0, o_{j+1} = o_j + draws(o_j),
and its state is the initial one advanced by o_N (chain_sums).  The planner's integer part is restated with Python ints.
"""
import numpy as np

import radiance_ref as R

F32, U32 = np.float32, np.uint32
LUM = (F32(0.2126), F32(0.7152), F32(0.0722))


def table_entries(max_total, bounces):
    """Table entries that hold every chain of max_total samples: a sample draws at most 2 + 4 * bounces numbers."""
    return 1 + (max_total * (2 + 4 * bounces) + 1) // 2


_CHAIN_TABLES = {}


def chain_tables(key, oracle_scene, w, h, bounces, states, max_total):
    """radiance_ref.frame_tables with only the entries a pixel's chain visits in its first max_total samples filled in
    (the others NaN: a chain that strays poisons what it sums): float32 [h * w, table_entries(max_total, bounces), 8].
    Each entry is oracle_sample_table's own row 0 for the pixel's state advanced to the entry's offset, so a filled
    entry is the full table's (tests/test_adaptive_cpu.py checks it) at 1 / 13 of the oracle's work for six bounces.
    Computed once per (key, max_total) and shared (never modified by a test)."""
    got = _CHAIN_TABLES.get((key, max_total))
    if got is None:
        P = w * h
        got = np.full((P, table_entries(max_total, bounces), 8), np.nan, dtype=F32)
        st = np.array(states, dtype=U32, copy=True).reshape(P, 6)
        off = np.zeros(P, dtype=np.int64)
        rows = np.arange(P)
        for _ in range(max_total):
            for p in range(P):
                got[p, off[p] // 2] = R.sample_table(oracle_scene, w, h, p % w, p // w, bounces, st[p], 1)[0]
            draws = got[rows, off // 2, 3].astype(np.int64)
            st = R.xorwow_advance(st, draws)
            off += draws
        got.setflags(write=False)
        _CHAIN_TABLES[(key, max_total)] = got
    return got


def lum(c):
    """rt_moments' lum of float32 [..., 3] colours."""
    c = np.asarray(c, dtype=F32)
    return ((LUM[0] * c[..., 0] + LUM[1] * c[..., 1]).astype(F32) + LUM[2] * c[..., 2]).astype(F32)


def chain_sums(tables, counts, bounces, offsets=None, accum=None, moments=None):
    """Per pixel p, counts[p] more samples of the chain through tables ([P, n, 8], radiance_ref.frame_tables) from draw
    offset offsets[p] (default 0), added to accum (float32 [P, 4]: sum rgb, count; default 0) and moments (float32
    [P, 2]: sum l, sum l*l; default 0) one sample at a time in fp32.  Returns new (accum, moments, offsets int64 [P])."""
    P, n, _ = tables.shape
    counts = np.asarray(counts, dtype=np.int64).reshape(P)
    off = np.zeros(P, dtype=np.int64) if offsets is None else np.array(offsets, dtype=np.int64)
    acc = np.zeros((P, 4), dtype=F32) if accum is None else np.array(accum, dtype=F32)
    mom = np.zeros((P, 2), dtype=F32) if moments is None else np.array(moments, dtype=F32)
    worst = int((off + counts * (2 + 4 * bounces)).max(initial=0))  # the last draw any chain can reach
    assert n >= 1 + (worst + 1) // 2, "the table is too short for the chain"
    for k in range(int(counts.max(initial=0))):
        rows = np.flatnonzero(counts > k)
        assert (off[rows] % 2 == 0).all() and (off[rows] // 2 < n).all(), "the table is too short for the chain"
        row = tables[rows, off[rows] // 2]
        c = row[:, 0:3]
        acc[rows, 0:3] = (acc[rows, 0:3] + c).astype(F32)
        acc[rows, 3] = (acc[rows, 3] + F32(1.0)).astype(F32)
        l = lum(c)
        mom[rows, 0] = (mom[rows, 0] + l).astype(F32)
        mom[rows, 1] = (mom[rows, 1] + (l * l).astype(F32)).astype(F32)
        off[rows] += row[:, 3].astype(np.int64)
    return acc, mom, off


def priority(accum, moments):
    """rt_sample_priority: float32 [P] from accum [P, 4] and moments [P, 2]."""
    accum, moments = np.asarray(accum, dtype=F32), np.asarray(moments, dtype=F32)
    n, mx, my = accum[:, 3], moments[:, 0], moments[:, 1]
    out = np.full(n.shape, np.inf, dtype=F32)
    with np.errstate(all="ignore"):
        known = (n >= F32(2.0)) & np.isfinite(mx) & np.isfinite(my)
        nk = n[known]
        m1, m2 = (mx[known] / nk).astype(F32), (my[known] / nk).astype(F32)
        var = (np.maximum(F32(0.0), (m2 - (m1 * m1).astype(F32)).astype(F32)) / nk).astype(F32)
        out[known] = (var / ((m1 * m1).astype(F32) + F32(1e-4)).astype(F32)).astype(F32)
    return out


def resolve(accum):
    """rt_sample_resolve: float32 [P, 4] from accum [P, 4]."""
    accum = np.asarray(accum, dtype=F32)
    out = np.zeros(accum.shape, dtype=F32)
    out[:, 3] = 1.0
    with np.errstate(all="ignore"):
        some = accum[:, 3] >= F32(1.0)
        out[some, 0:3] = (accum[some, 0:3] / accum[some, 3:4]).astype(F32)
    return out


def subtile_order(w, h):
    """The pixel indices y * w + x in 8x8 sub-tile order: sub-tiles row-major, row-major inside a sub-tile, positions
    outside the image left out."""
    out = []
    for ty in range((h + 7) // 8):
        for tx in range((w + 7) // 8):
            for y in range(8 * ty, min(8 * ty + 8, h)):
                for x in range(8 * tx, min(8 * tx + 8, w)):
                    out.append(y * w + x)
    return np.array(out, dtype=np.int32)


def quantise(prio, scale):
    """q_p of rt_sample_plan as a list of Python ints."""
    with np.errstate(all="ignore"):
        t = (np.asarray(prio, dtype=F32) * F32(scale)).astype(F32)
    return [65535 if not (v < F32(65535.0)) else (int(v) if v > 0 else 0) for v in t]


def plan(prio, w, h, budget, min_samples, max_samples, scale):
    """rt_sample_plan: (pixels int32 [P], samples uint16 [P], total int)."""
    P = w * h
    assert 1 <= max_samples <= 4095 and 0 <= min_samples <= max_samples and budget >= min_samples * P
    q = quantise(np.asarray(prio).reshape(-1)[:P], scale)
    Q = sum(q)
    B = budget - min_samples * P
    n = [min(max_samples, min_samples + (qp * B // Q if Q else 0)) for qp in q]
    order = subtile_order(w, h)
    keyed = sorted(range(P), key=lambda e: -n[order[e]])  # sorted() is stable
    pixels = order[keyed]
    samples = np.array([n[p] for p in pixels], dtype=np.uint16)
    return pixels.astype(np.int32), samples, sum(n)


# ----------------------------------------------------------------------------------------------------------------------
# the planner's test inputs, shared by the CPU self-checks and the GPU comparison
# ----------------------------------------------------------------------------------------------------------------------
def priorities(kind, P, seed=7):
    r = np.random.default_rng(seed)
    if kind == "random":
        return (r.random(P) ** 4 * 3.0).astype(F32)
    if kind == "zero":
        return np.zeros(P, dtype=F32)
    if kind == "inf":
        return np.full(P, np.inf, dtype=F32)
    if kind == "hot":
        out = np.zeros(P, dtype=F32)
        out[P // 2] = 3.0
        return out
    assert kind == "mixed"  # NaN, negative, -inf, +inf, huge, denormal among random ones
    out = (r.random(P) * 2.0 - 0.5).astype(F32)
    special = np.array([np.nan, -1.0, -np.inf, np.inf, 3e38, 1e-42, -0.0, 65535.0, 65534.99], dtype=F32)
    out[r.permutation(P)[:min(P, special.size)]] = special[:min(P, special.size)]
    return out


KINDS = ["random", "zero", "inf", "hot", "mixed"]
PLANS = [dict(budget_spp=4, min_samples=0, max_samples=64, scale=64.0), dict(budget_spp=2, min_samples=1, max_samples=3, scale=1000.0),
         dict(budget_spp=1.5, min_samples=0, max_samples=4095, scale=1.0), dict(budget_spp=5000, min_samples=2, max_samples=4095, scale=0.5)]
