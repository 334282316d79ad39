"""The small-set route's dense all-pairs kernels run alone (sky_profile_pairs_dev): every row
against every row, ServiceTuple.dominates (ServiceTuple.java:67-77) over all pairs as the BNL
loops of FlinkSkyline.java:424-441 / :548-566 would evaluate them.  k_brute16_pairs (integer
rows, packed u16, the x chunk ordered by partition in LDS), k_brute_pairs<float> and <double>
must give every row exactly the fates of a numpy brute force: bit 0 = a row of its partition
dominates it, bit 1 = some row does.  The same kernels serve every query whose slots take the
brute route (C1-C4), which the configuration tests check end to end against the oracle.

Beyond the 9000-row cases: the large u16 tile shape (two y per lane, 512-row chunks), which the
launcher takes from 32257 rows and no query's slots reach, checked against the same compare in
torch f64 on the device; every kernel at one row and around its tile edges; odd dimension
counts; and the ends of the u16 range, with 65536 or a fraction turning the rows into f32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def numpy_fates(vals, keys, block=512):
    n = len(vals)
    out = np.zeros(n, np.uint32)
    for i0 in range(0, n, block):
        y = vals[i0:i0 + block]                                   # [b, D]
        le = (vals[None, :, :] <= y[:, None, :]).all(-1)         # x_j <= y_i everywhere
        lt = (vals[None, :, :] < y[:, None, :]).any(-1)
        dom = le & lt                                             # [b, n]
        same = keys[None, :] == keys[i0:i0 + block, None]
        out[i0:i0 + block] = (dom & same).any(1).astype(np.uint32) | (dom.any(1).astype(np.uint32) << 1)
    return out


def run(eng, vals, keys):
    dv = torch.from_numpy(np.ascontiguousarray(vals)).cuda()
    dk = torch.from_numpy(np.ascontiguousarray(keys, np.int32)).cuda()
    df = torch.empty(len(vals), dtype=torch.int32, device="cuda")
    kind, ms = eng.profile_pairs_dev(dv, dk, df)
    eng.sync()
    return kind, df.cpu().numpy().astype(np.uint32)


CASES = ["u16_std_anti", "u16_dups_many_parts", "u16_one_part", "f32_negative", "f64_inexact", "u16_16d"]


def case_inputs(case, oracle):
    """-> (D, P, rows, keys, the kind the rows must take)"""
    rng = np.random.default_rng(sum(map(ord, case)))
    D, n, P = 8, 9000, 16
    if case == "u16_std_anti":
        vals = oracle.synth(3, D, n, seed=5)
        keys = rng.integers(0, P, n)
        want = 0
    elif case == "u16_dups_many_parts":
        vals = rng.integers(0, 6, size=(n, D)).astype(np.float64)   # many duplicates and ties
        keys = rng.integers(0, 200, n)
        want = 0
    elif case == "u16_one_part":
        vals = oracle.synth(2, D, n, seed=6)
        keys = np.zeros(n, np.int64)
        want = 0
    elif case == "f32_negative":
        vals = (rng.integers(-50, 50, size=(n, 4)) * 0.25).astype(np.float64)
        D = 4
        keys = rng.integers(0, P, n)
        want = 1
    elif case == "f64_inexact":
        vals = rng.integers(0, 40, size=(n, 5)).astype(np.float64) + 0.1
        D = 5
        keys = rng.integers(0, P, n)
        want = 2
    else:
        D = 16
        vals = oracle.synth(3, D, 4000, seed=7)
        keys = rng.integers(0, P, len(vals))
        want = 0
    return D, P, vals, keys, want


_CASE_FATES = {}


def case_fates(case, vals, keys):
    """numpy_fates of a case's rows, computed once for the tests that share the case."""
    if case not in _CASE_FATES:
        _CASE_FATES[case] = numpy_fates(vals, keys)
    return _CASE_FATES[case]


@pytest.mark.parametrize("case", CASES)
def test_dense_pairs_equal_numpy(case, gpu_engine_factory, oracle):
    D, P, vals, keys, want = case_inputs(case, oracle)
    eng = gpu_engine_factory(D, P)
    kind, got = run(eng, vals, keys)
    eng.close()
    assert kind == want
    np.testing.assert_array_equal(got, case_fates(case, vals, keys))


# ---- the large u16 tile shape, partial tiles, dimension counts, the u16 value limits ----------
def torch_fates(vals, keys, block=512):
    """numpy_fates' blocked broadcast compare in torch f64 on the device (no project call): the
    reference for sizes at which numpy takes tens of seconds."""
    v = torch.from_numpy(np.ascontiguousarray(vals, np.float64)).cuda()
    k = torch.from_numpy(np.ascontiguousarray(keys, np.int64)).cuda()
    n = len(v)
    out = torch.zeros(n, dtype=torch.int64, device="cuda")
    for i0 in range(0, n, block):
        y = v[i0:i0 + block]
        le = (v[None, :, :] <= y[:, None, :]).all(-1)
        lt = (v[None, :, :] < y[:, None, :]).any(-1)
        dom = le & lt
        same = k[None, :] == k[i0:i0 + block, None]
        out[i0:i0 + block] = (dom & same).any(1).to(torch.int64) | (dom.any(1).to(torch.int64) << 1)
    return out.cpu().numpy().astype(np.uint32)


def expected_kind(vals):
    """The compare type sky_profile_pairs_dev documents: f64 (2) once a value is no f32; packed u16
    (0) for integers in [0, 65535] (no -0.0) whose score key has no ties, i.e. every row's f64 sum
    in dimension order is exact (values clamped to +-1e300) and is an f32; else f32 (1)."""
    v = np.asarray(vals, np.float64)
    if (v.astype(np.float32).astype(np.float64) != v).any():
        return 2
    s = np.zeros(len(v))
    inexact = np.zeros(len(v), bool)
    for d in range(v.shape[1]):
        x = np.clip(v[:, d], -1e300, 1e300)
        sn = s + x
        bb = sn - s
        inexact |= (x != v[:, d]) | (((s - (sn - bb)) + (x - bb)) != 0.0)
        s = sn
    inexact |= s.astype(np.float32).astype(np.float64) != s
    ints = ((v >= 0) & (v <= 65535) & (v == np.floor(v)) & ~np.signbit(v)).all()
    return 0 if ints and not inexact.any() else 1


def corr_ints(rng, n, D):
    """Integer rows with a shared per-row base: most rows dominated, some not (unlike the std-anti
    rows, of which a few per cent are)."""
    return (rng.integers(0, 800, (n, 1)) + rng.integers(0, 200, (n, D))).astype(np.float64)


@pytest.mark.parametrize("case", ["u16_std_anti", "u16_dups_many_parts", "f32_negative"])
def test_torch_fates_equal_numpy_fates(case, oracle):
    """The device reference of the large cases equals the numpy one on the 9000-row inputs above."""
    _, _, vals, keys, _ = case_inputs(case, oracle)
    ref = case_fates(case, vals, keys)
    assert (ref == 0).any() and (ref == 2).any() and (ref == 3).any()
    np.testing.assert_array_equal(torch_fates(vals, keys), ref)


def large_keys(rng, n, P=16):
    """Partition runs as a query's sorted slots have them, a quarter of the rows re-drawn at random
    (many short runs in every x chunk), and the last 300 rows cycling over three partitions: the
    last chunks hold rows of more than one partition, whatever n leaves in the very last one."""
    i = np.arange(n)
    keys = (i * P) // n
    redraw = rng.random(n) < 0.25
    keys[redraw] = rng.integers(0, P, int(redraw.sum()))
    keys[n - 300:] = P - 3 + i[n - 300:] % 3
    return keys


# the launcher takes the large shape (two y per lane, 512-row chunks) from ceil(n / 512)^2 >= 4096
LARGE_FROM = 63 * 512 + 1
LARGE_CASES = [("std_anti", 8, LARGE_FROM - 1),      # the last size on the small shape
               ("std_anti", 8, LARGE_FROM),          # one row in the last y block and the last x chunk
               ("std_anti", 8, 32768),               # whole blocks and chunks only
               ("std_anti", 8, 32769),
               ("std_anti", 16, LARGE_FROM),         # the eight-word rows
               ("corr", 8, 32769),                   # rows of which most are dominated
               ("corr", 16, LARGE_FROM)]


@pytest.mark.parametrize("rows,D,n", LARGE_CASES, ids=lambda x: str(x))
def test_dense_u16_large_shape(rows, D, n, gpu_engine_factory, oracle):
    """k_brute16_pairs at the sizes around the switch to its large tile shape, which no query's
    brute route reaches (at most ~16k slots) but the bench's 64k dense line runs."""
    assert LARGE_FROM == 32257
    rng = np.random.default_rng(n + D)
    vals = oracle.synth(3, D, n, seed=n) if rows == "std_anti" else corr_ints(rng, n, D)
    keys = large_keys(rng, n)
    eng = gpu_engine_factory(D, 16)
    kind, got = run(eng, vals, keys)
    eng.close()
    assert kind == 0
    ref = torch_fates(vals, keys)
    if rows == "corr":
        assert (ref == 0).any() and (ref == 2).any() and (ref == 3).any()
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513])
@pytest.mark.parametrize("rows", ["u16", "f32_negative", "f64_inexact"])
def test_dense_partial_tiles(rows, n, gpu_engine_factory):
    """One row, and sizes one below, at and one above the tile edges of the three kernels (64-row
    tiles of k_brute_pairs, 128-row chunks and 256-row y blocks of the small u16 shape)."""
    rng = np.random.default_rng(1000 * n + len(rows))
    if rows == "u16":
        D, vals = 8, corr_ints(rng, n, 8)
    elif rows == "f32_negative":
        D, vals = 4, rng.integers(-50, 50, size=(n, 4)) * 0.25
    else:
        D, vals = 5, rng.integers(0, 40, size=(n, 5)).astype(np.float64) + 0.1
    keys = rng.integers(0, 4, n)
    want = expected_kind(vals)
    if n >= 63:                                   # (one or two f32_negative rows can be u16 rows)
        assert want == {"u16": 0, "f32_negative": 1, "f64_inexact": 2}[rows]
    ref = numpy_fates(vals, keys)
    if n >= 63:
        assert (ref == 0).any() and (ref == 2).any() and (ref == 3).any()
    eng = gpu_engine_factory(D, 16)
    kind, got = run(eng, vals, keys)
    eng.close()
    assert kind == want
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("D", [1, 3, 7, 9, 15])
def test_dense_u16_dimension_counts(D, gpu_engine_factory):
    """Odd dimension counts (a half-filled last word, zero-padded words) and the first count that
    takes the eight-word rows."""
    rng = np.random.default_rng(D)
    n = 1000
    vals = corr_ints(rng, n, D)
    keys = rng.integers(0, 16, n)
    ref = numpy_fates(vals, keys)
    assert (ref == 0).any() and (ref == 2).any() and (ref == 3).any()
    eng = gpu_engine_factory(D, 16)
    kind, got = run(eng, vals, keys)
    eng.close()
    assert kind == 0
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("D", [8, 16])
@pytest.mark.parametrize("case", ["limits", "one_65536", "one_half"])
def test_dense_u16_value_limits(case, D, gpu_engine_factory):
    """Rows of {0, 1, 65534, 65535}: the saturating subtracts at both ends of the u16 range and, at
    16 dimensions, the largest row sum (16 * 65535, still an exact f32: no score tie, so u16).
    One value of 65536 or of 0.5 anywhere must move the whole set to the f32 kernel."""
    rng = np.random.default_rng(D)
    n = 1000
    vals = rng.choice(np.array([0.0, 1.0, 65534.0, 65535.0]), size=(n, D))
    vals[17] = 65535.0                            # the largest sum is there
    keys = rng.integers(0, 16, n)
    if case == "one_65536":
        vals[n // 2, D - 1] = 65536.0
    elif case == "one_half":
        vals[n // 3, 0] = 0.5
    want = expected_kind(vals)
    assert want == (0 if case == "limits" else 1)
    ref = numpy_fates(vals, keys)
    assert (ref == 0).any() and (ref == 2).any() and (ref == 3).any()
    eng = gpu_engine_factory(D, 16)
    kind, got = run(eng, vals, keys)
    eng.close()
    assert kind == want
    np.testing.assert_array_equal(got, ref)
