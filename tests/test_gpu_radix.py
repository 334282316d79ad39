"""The pipeline's onesweep radix sort (k_radix.hip, radix_sort_pairs) run alone below the sizes of
test_radix_sort_at_scale: (u64 key, u32 value) pairs through sky_profile_sort_dev against a stable
torch sort of the keys taken as unsigned 64-bit (torch sorts int64 as signed: bit 63 is flipped
first).  Keys sorted, values in the reference's order (so ties keep index order), and the pass
count the launcher's rule gives for the keys' OR and AND, worked out here.

Sizes: the early exits (0, 1 keys), one and two 1024-key tiles, an exact multiple of the tile and
one past it, the switch to 6144-key tiles at 1 << 22 and the first exact multiple of that tile
past the switch.  Patterns: no varying bit, one varying bit (0, 31, 63), one varying byte (one
pass, the result copied back from the alt buffers), three raw bytes, two far bits compressed to
one pass, nine runs of one bit (more runs than the compression takes: raw bytes), heavy ties."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SWITCH = 1 << 22            # radix_sort_pairs: 6144-key tiles from here on
BIG_TILE = 6144
BIT63 = -(1 << 63)          # the int64 whose only set bit is bit 63


def expected_passes(keys):
    """radix_sort_pairs' rule from the OR and the AND of the keys: no pass for at most one key or no
    varying bit; else min(bytes holding a varying bit, ceil(varying bits / 8)), and the byte count
    when the varying bits make more than 8 runs."""
    if keys.numel() <= 1:
        return 0
    varying = 0
    for b in range(64):
        bit = (keys >> b) & 1
        if int(bit.max()) != int(bit.min()):
            varying |= 1 << b
    if varying == 0:
        return 0
    nbits = bin(varying).count("1")
    nbytes = sum(1 for byte in range(8) if (varying >> (8 * byte)) & 0xff)
    runs = sum(1 for b in range(64) if (varying >> b) & 1 and not (b and (varying >> (b - 1)) & 1))
    return nbytes if runs > 8 else min(nbytes, (nbits + 7) // 8)


def rand_bits(n, mask, gen):
    """n int64 keys with independent random bits where `mask` (a 64-bit pattern) has a one."""
    lo = torch.randint(0, 1 << 32, (n,), device="cuda", dtype=torch.int64, generator=gen)
    hi = torch.randint(0, 1 << 32, (n,), device="cuda", dtype=torch.int64, generator=gen)
    m = mask - (1 << 64) if mask >> 63 else mask
    return (lo | (hi << 32)) & m


def sort_and_check(eng, keys, want_passes=None):
    n = keys.numel()
    vals = torch.arange(n, dtype=torch.int32, device="cuda")
    _, order = torch.sort(keys ^ BIT63, stable=True)        # unsigned order, ties by index
    skeys = keys[order]
    exp = expected_passes(keys)
    if want_passes is not None:
        assert exp == want_passes, "the pattern does not vary the bits it is meant to"
    k = keys.clone()
    if n:
        passes, _ = eng.profile_sort_dev(k, vals)
    else:
        # an empty tensor has no address and the ABI takes no null pointer: n = 0 on one-word buffers
        from skyline._abi import check, lib
        kb = torch.zeros(1, dtype=torch.int64, device="cuda")
        vb = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        p = ctypes.c_int32(-1)
        ms = ctypes.c_double(0)
        check(lib().sky_profile_sort_dev(eng.h, ctypes.c_void_p(kb.data_ptr()), ctypes.c_void_p(vb.data_ptr()), 0,
                                         ctypes.byref(p), ctypes.byref(ms)))
        passes = p.value
        eng.sync()
        assert int(kb[0]) == 0 and int(vb[0]) == 0
    eng.sync()
    assert passes == exp
    assert torch.equal(k, skeys)
    assert torch.equal(vals.to(torch.int64), order)
    if exp == 0:                                            # nothing to do: both arrays as they came
        assert torch.equal(k, keys)
        assert torch.equal(vals, torch.arange(n, dtype=torch.int32, device="cuda"))


@pytest.fixture(scope="module")
def eng(gpu_engine_factory):
    e = gpu_engine_factory(2, 4)
    yield e
    e.close()


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 2049, 65537])
def test_radix_small_sizes_full_keys(n, eng):
    """One partial tile, one whole tile, two tiles, an exact multiple and one past it, 65 tiles: full
    62-bit keys (8 raw-byte passes once enough keys vary every byte; the rule decides below that)."""
    g = torch.Generator(device="cuda")
    g.manual_seed(100 + n)
    sort_and_check(eng, rand_bits(n, (1 << 62) - 1, g))


@pytest.mark.parametrize("n", [SWITCH - 1, SWITCH, SWITCH + 1, BIG_TILE * 683, BIG_TILE * 683 + 1])
@pytest.mark.parametrize("pattern", ["full", "compressed"])
def test_radix_tile_switch(pattern, n, eng):
    """The last size on 1024-key tiles, the first sizes on 6144-key tiles, and the first exact
    multiple of the large tile past the switch (683 tiles) and one key more (684, the last with
    one key).  'compressed': 16 varying bits in two runs over three bytes -> two dense passes."""
    assert BIG_TILE * 682 < SWITCH < BIG_TILE * 683
    g = torch.Generator(device="cuda")
    g.manual_seed(n % 1000 + len(pattern))
    if pattern == "full":
        sort_and_check(eng, rand_bits(n, (1 << 62) - 1, g), 8)
    else:
        sort_and_check(eng, rand_bits(n, (0xfff << 4) | (0xf << 40), g) | (1 << 62) | 3, 2)


PATTERNS = {
    # name: (varying mask, constant bits, passes)
    "all_equal": (0, 0x0123456789abcdef, 0),
    "bit0": (1, 0x5a5a5a00, 1),
    "bit31": (1 << 31, 0x1234, 1),
    "bit63": (1 << 63, 0x00ff00ff00ff00ff, 1),
    "byte2": (0xff << 16, 1 << 40, 1),              # not compressed, odd pass count: copied back
    "bits8_24": (0xffffff << 8, 0, 3),              # three raw bytes, not compressed
    "bits0_56": (1 | (1 << 56), 0xff00, 1),         # two bytes, two bits: compressed to one pass
    "nine_runs": (0x15555, 1 << 50, 3),             # more than 8 runs: raw bytes 0, 1, 2
}


@pytest.mark.parametrize("n", [65537, SWITCH + 1])
@pytest.mark.parametrize("pattern", list(PATTERNS) + ["four_keys"])
def test_radix_bit_patterns(pattern, n, eng):
    """Each route through radix_sort_pairs' pass plan, on both tile sizes.  'four_keys': four
    distinct keys spread over the whole word, so nearly every compare is a tie and the values
    show whether each pass kept index order."""
    g = torch.Generator(device="cuda")
    g.manual_seed(7 * n + sum(map(ord, pattern)))
    if pattern == "four_keys":
        table = torch.tensor([3, (1 << 62) | 3, (1 << 33) | 1, BIT63 | (1 << 20)], dtype=torch.int64, device="cuda")
        keys = table[torch.randint(0, 4, (n,), device="cuda", generator=g)]
        sort_and_check(eng, keys)
        return
    mask, const, passes = PATTERNS[pattern]
    assert mask & const == 0
    keys = rand_bits(n, mask, g) | const
    sort_and_check(eng, keys, passes)
