"""tests/stream_cases.py against the oracle: the analytic answer for a stream of a few distinct
vectors (brute-force dominance over the vectors only) equals the oracle's BNL job over every
tuple, before any GPU stream test relies on it."""
import numpy as np

import stream_cases as sc


def test_expected_equals_oracle_bnl(oracle):
    P_ = 8
    rng = np.random.default_rng(2000)
    vectors = np.vstack([sc.VECTORS, sc.B_KILLER])
    keys = oracle.keys("angle", vectors, P_)
    assert len(set(keys[:3].tolist())) == 3 and keys[3] == keys[1]
    # 2000 tuples of the mix, the row that dominates B, then A and C rows only
    which = np.concatenate([sc.draw(rng, 2000), [3], sc.draw(rng, 500, among=(0, 2))])
    assert all((which == i).sum() > 100 for i in range(3))
    vals = vectors[which]
    ids = np.arange(len(which), dtype=np.int64)
    for n in (1, 2000, 2001, len(which)):       # one tuple; all in the skyline; B's gone; more behind them
        m = 4 if n > 2000 else 3
        ids_e, ls_e, sv_e = sc.expected(vectors[:m], sc.members(which[:n], m), keys[:m], P_)
        got, _, ls, sv = oracle.query_bnl("angle", vals[:n], ids[:n], P_)
        np.testing.assert_array_equal(ids_e, np.sort(got))
        np.testing.assert_array_equal(ls_e, ls)
        np.testing.assert_array_equal(sv_e, sv)
        if n == 2000:
            assert len(ids_e) == 2000
        if n > 2000:                            # the B tuples left L_k and the output, the new row is in
            assert len(ids_e) == (which[:n] != 1).sum() and ls_e[keys[1]] == 1
