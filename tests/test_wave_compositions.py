"""The row orders of tests/wave_compositions.py, checked on their own (no GPU): every base item is compared, src maps back, tiles fall where stated."""
import numpy as np
import pytest

import wave_compositions as wc

SIZES = [1, 63, 64, 65, 257, 1000]


def compositions(n):
    labels = np.random.default_rng(n).integers(-2, 5, n)
    half = np.arange(n) % 3 == 0
    out = {"natural": wc.natural(n), "alone": wc.alone(n), "alone_at17": wc.alone_at(n, 17), "alone_at63": wc.alone_at(n, 63), "permuted1": wc.permuted(n, 1),
           "permuted2": wc.permuted(n, 2), "grouped": wc.grouped(labels), "replicated": wc.replicated(n), "dead_interleaved": wc.dead_interleaved(n, 5)}
    if half.any() and not half.all():
        out["one_odd"] = wc.one_odd(n, np.flatnonzero(half), np.flatnonzero(~half), 7)
    return out, labels


@pytest.mark.parametrize("n", SIZES)
def test_every_item_is_compared_and_src_maps_back(n):
    comps, _ = compositions(n)
    for name, (src, pairs) in comps.items():
        assert src.dtype == np.int64 and src.ndim == 1 and pairs.shape[1] == 2, name
        assert ((src >= 0) | (src == wc.FILL)).all() and (src < n).all(), name
        rows, base = pairs[:, 0], pairs[:, 1]
        assert len(np.unique(rows)) == len(rows) and (rows >= 0).all() and (rows < len(src)).all(), name
        assert np.array_equal(src[rows], base), name                                  # a compared row holds the item it is compared with
        assert np.array_equal(np.sort(rows), np.flatnonzero(src >= 0)), name          # and every live row is compared
        assert np.array_equal(np.unique(base), np.arange(n)), (name, "a base item is never compared")


@pytest.mark.parametrize("n", SIZES)
def test_shapes_and_tile_boundaries(n):
    comps, labels = compositions(n)
    src, _ = comps["natural"]
    assert np.array_equal(src, np.arange(n))
    for name, lane in (("alone", 0), ("alone_at17", 17), ("alone_at63", 63)):
        src, _ = comps[name]
        tiles = src.reshape(n, wc.TILE)
        assert (np.sum(tiles >= 0, axis=1) == 1).all(), name                           # no tile holds two live rows
        assert np.array_equal(tiles[:, lane], np.arange(n)), name
    for name in ("permuted1", "permuted2"):
        src, _ = comps[name]
        assert np.array_equal(np.sort(src), np.arange(n))
    if n > 64:
        assert not np.array_equal(comps["permuted1"][0], comps["permuted2"][0]) and not np.array_equal(comps["permuted1"][0], np.arange(n))
    assert np.array_equal(wc.permuted(n, 1)[0], comps["permuted1"][0])                # seeded: the same order every time
    src, _ = comps["grouped"]
    assert np.array_equal(np.sort(src), np.arange(n)) and (np.diff(labels[src]) >= 0).all()
    same = np.diff(labels[src]) == 0
    assert (np.diff(src)[same] > 0).all()                                              # stable within a label
    src, _ = comps["replicated"]
    assert np.array_equal(src.reshape(n, wc.TILE), np.repeat(np.arange(n), wc.TILE).reshape(n, wc.TILE))
    src, _ = comps["dead_interleaved"]
    assert len(src) == 2 * n
    first, second = src[:n], src[n:]
    for part in (first, second):
        live = part >= 0
        assert np.array_equal(part[live], np.arange(n)[live])                         # natural order where live
    assert ((first >= 0) | (second >= 0)).all()
    if n >= 63:
        assert 0.15 < (first < 0).mean() < 0.55 and (second < 0).any()


@pytest.mark.parametrize("n,tiles", [(65, None), (257, None), (1000, None), (1000, 40)])
def test_one_odd_tiles_hold_63_and_1(n, tiles):
    inP = np.arange(n) % 3 == 0
    P, Q = np.flatnonzero(inP), np.flatnonzero(~inP)
    src, pairs = wc.one_odd(n, P, Q, 11, tiles=tiles)
    T = max(len(P), len(Q)) if tiles is None else tiles
    body = src[:2 * T * wc.TILE].reshape(2 * T, wc.TILE)
    for half, major_is_P in ((body[:T], True), (body[T:], False)):
        for tile in half:
            vals, counts = np.unique(tile, return_counts=True)
            assert sorted(counts) == [1, 63]
            major, minor = vals[np.argmax(counts)], vals[np.argmin(counts)]
            assert inP[major] == major_is_P and inP[minor] != major_is_P
    lanes = np.array([np.flatnonzero(t != np.bincount(t).argmax())[0] for t in body])
    assert len(np.unique(lanes)) > 8                                                  # the odd one's lane is seeded, not fixed
    rest = src[2 * T * wc.TILE:]
    assert np.array_equal(rest, np.setdiff1d(np.arange(n), body))                     # what no tile holds follows, from a tile boundary
    if tiles is None:
        assert len(rest) == 0
        assert set(body[:T, :].ravel()) >= set(P) and set(body[T:, :].ravel()) >= set(Q)
    assert len(pairs) == len(src)                                                     # every row is compared


@pytest.mark.parametrize("m", wc.TRUNCATED_SIZES)
def test_truncated(m):
    src, pairs = wc.truncated(1000, m)
    assert np.array_equal(src, np.arange(m)) and np.array_equal(pairs, np.stack([np.arange(m)] * 2, axis=1))
    assert (len(src) + wc.TILE - 1) // wc.TILE * wc.TILE - len(src) == (-m) % wc.TILE           # idle lanes of the last tile


def test_gather_fills_filler_rows():
    o = np.arange(12.0).reshape(4, 3)
    keys = np.arange(4, dtype=np.uint32)
    src = np.array([2, wc.FILL, 0, 3, wc.FILL], np.int64)
    go, gk = wc.gather(src, o, keys, fill=(np.nan, 0))
    assert np.array_equal(go[[0, 2, 3]], o[[2, 0, 3]]) and np.isnan(go[[1, 4]]).all()
    assert gk.dtype == np.uint32 and np.array_equal(gk, [2, 0, 0, 3, 0])
    assert np.array_equal(o, np.arange(12.0).reshape(4, 3))                           # the base arrays are left as they were
