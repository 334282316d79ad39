"""Streams made of a handful of distinct vectors, with the query's answer worked out from those
vectors alone (test infrastructure, like the oracle: never the thing under test).

A stream whose tuples repeat a few mutually non-dominating vectors keeps almost every tuple in
the skyline, so the expected ids, |L_k| and survivors_k follow from brute-force dominance over
the distinct vectors and the list of tuples that carry each: no quadratic BNL over the tuples.
tests/test_cpu_stream_cases.py pins expected() to the oracle's BNL job at a small size."""
import numpy as np

# three mutually non-dominating 2-D vectors (MR-Angle, P = 8: three different partitions) ...
A, B, C = (1.0, 3.0), (2.0, 2.0), (3.0, 1.0)
VECTORS = np.array([A, B, C], np.float64)
MIX = (0.5, 0.3, 0.2)                      # ... drawn with these odds
B_KILLER = 0.99 * np.array(B)              # dominates B alone; meant to share B's partition


def draw(rng, n, among=(0, 1, 2)):
    """Vector index of each of n tuples: a seeded, non-uniform mix of the vectors `among`."""
    odds = np.asarray(MIX, np.float64)[list(among)]
    return np.asarray(among)[rng.choice(len(among), size=n, p=odds / odds.sum())]


def members(which, m):
    """Per-vector tuple lists from the vector index of every tuple in arrival order: the tuples'
    arrival positions (= their ids when the ids are 0..n-1)."""
    return [np.nonzero(which == i)[0].astype(np.int64) for i in range(m)]


def expected(vectors, tuples, keys, K):
    """vectors [m, D] distinct; tuples[i]: ids of the tuples that carry vector i (ids increase along
    the stream, so arrival order is id order); keys[i]: vector i's partition, in [0, K).
    -> (ids of the global skyline in arrival order, |L_k| [K], survivors_k [K]): a tuple is in L_k
    when no vector of its partition dominates its vector, and survives the merge of the L_k when
    no vector of any L_j does (ServiceTuple.dominates: <= everywhere and < somewhere)."""
    v = np.asarray(vectors, np.float64)
    keys = np.asarray(keys)
    m = len(v)
    assert len(tuples) == m and len(keys) == m
    assert len({tuple(r) for r in v.tolist()}) == m, "the vectors must be distinct"
    assert ((keys >= 0) & (keys < K)).all()
    dom = (v[:, None, :] <= v[None, :, :]).all(-1) & (v[:, None, :] < v[None, :, :]).any(-1)   # [i, j]: i dominates j
    dom &= np.array([len(t) > 0 for t in tuples])[:, None]      # a vector nobody carries dominates nothing
    same = keys[:, None] == keys[None, :]
    in_local = ~(dom & same).any(0)
    in_global = in_local & ~(dom & in_local[:, None]).any(0)
    ls = np.zeros(K, np.int64)
    sv = np.zeros(K, np.int64)
    for i in range(m):
        if in_local[i]:
            ls[keys[i]] += len(tuples[i])
        if in_global[i]:
            sv[keys[i]] += len(tuples[i])
    parts = [np.asarray(tuples[i], np.int64) for i in range(m) if in_global[i]]
    ids = np.sort(np.concatenate(parts)) if parts else np.zeros(0, np.int64)
    return ids, ls, sv
