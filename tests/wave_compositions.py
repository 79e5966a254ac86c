"""Who shares a wave with whom: row orders for the query entries (DESIGN.md "What the wave compositions show").  Not a test module.

k_query_closest / k_query_visible hand rows [64 t, 64 t + 64) of a call to one wave, and shade_rays on a path-traced scene starts row i in slot i, so
the caller's row order is the wave composition.  Each builder below takes the number N of base items (or arrays over them) and returns

    src     int64 [M]: the base item of each row, -1 for a filler row (a degenerate ray or segment: a lane that never enters the trace)
    pairs   int64 [K, 2]: (row, base item) for every row whose answer is compared with the base item's answer in natural order

Plain numpy; tests/test_wave_compositions.py checks the builders themselves, tests/test_gpu_wave_composition.py uses them."""
import numpy as np

TILE = 64                   # rows per wave
FILL = -1
TRUNCATED_SIZES = (1, 63, 64, 65, 255, 257)


def _pairs(src):
    rows = np.flatnonzero(src >= 0)
    return np.stack([rows, src[rows]], axis=1).astype(np.int64)


def natural(n):
    src = np.arange(n, dtype=np.int64)
    return src, _pairs(src)


def alone_at(n, lane):
    """item j alone in tile j, at `lane`: every vote on the device has one voter"""
    assert 0 <= lane < TILE
    src = np.full(TILE * n, FILL, np.int64)
    src[TILE * np.arange(n) + lane] = np.arange(n)
    return src, _pairs(src)


def alone(n):
    return alone_at(n, 0)


def permuted(n, seed):
    src = np.random.default_rng(seed).permutation(n).astype(np.int64)
    return src, _pairs(src)


def grouped(labels):
    """a stable sort by label: coherent waves, which take the wave-uniform exits"""
    src = np.argsort(np.asarray(labels), kind="stable").astype(np.int64)
    return src, _pairs(src)


def replicated(n):
    """each item 64 times: tile j is item j in every lane"""
    src = np.repeat(np.arange(n, dtype=np.int64), TILE)
    return src, _pairs(src)


def one_odd(n, P, Q, seed, tiles=None):
    """`tiles` tiles of 63 copies of one p of P with one q of Q at a seeded lane, then as many of 63 copies of one q with one p; tile i takes P[i % |P|]
    and a seeded member of Q (the mirror: Q[i % |Q|] and a seeded member of P), so with tiles >= max(|P|, |Q|), the default, every member of either
    class is the majority of a tile.  Base items that no tile holds follow in natural order from the next tile boundary.  Every row is compared."""
    P, Q = np.asarray(P, np.int64), np.asarray(Q, np.int64)
    assert len(P) and len(Q) and not np.intersect1d(P, Q).size
    tiles = max(len(P), len(Q)) if tiles is None else int(tiles)
    rng = np.random.default_rng(seed)
    src = np.empty((2 * tiles, TILE), np.int64)
    t = np.arange(tiles)
    for half, (major, minor) in enumerate(((P, Q), (Q, P))):
        block = src[half * tiles:(half + 1) * tiles]
        block[:] = major[t % len(major)][:, None]
        block[t, rng.integers(0, TILE, tiles)] = minor[rng.integers(0, len(minor), tiles)]
    src = src.ravel()
    rest = np.setdiff1d(np.arange(n, dtype=np.int64), src)
    src = np.concatenate([src, rest])
    return src, _pairs(src)


def truncated(n, m):
    """the first m rows: the last tile's lanes past m idle"""
    assert 0 < m <= n
    src = np.arange(m, dtype=np.int64)
    return src, _pairs(src)


def dead_interleaved(n, seed):
    """natural order with a seeded third of the rows replaced by filler; then natural order again, the rows that were filler live and a seeded third
    of the others filler, so that every item is compared"""
    rng = np.random.default_rng(seed)
    first = np.arange(n, dtype=np.int64)
    dead = rng.random(n) < 1.0 / 3.0
    if n > 1 and not dead.any():
        dead[rng.integers(0, n)] = True
    first[dead] = FILL
    second = np.arange(n, dtype=np.int64)
    second[~dead & (rng.random(n) < 1.0 / 3.0)] = FILL
    src = np.concatenate([first, second])
    return src, _pairs(src)


def gather(src, *arrays, fill):
    """rows of each array in `src` order; filler rows take `fill` (one row per array)"""
    out = []
    for x, f in zip(arrays, fill):
        x = np.asarray(x)
        y = x[np.maximum(src, 0)].copy()
        y[src < 0] = f
        out.append(np.ascontiguousarray(y))
    return out
