"""The wide packing-rows kernel on the MI355X (pytest -m gpu): thfhe_mk_pack_boxes with mk_pack_rows_wide_kernel forced
(threshold 1) and with the direct mk_pack_rows_kernel forced (threshold 0), the kernel's name asserted each time, both word for word against each
other and against the numpy model (tests/mk_pack_reference.py): every ring degree, both key shapes (D = P n and D = N), the digit shapes of
tests/test_gpu_mk_pack_shapes.py, record counts around the wide kernel's group of 32, an all-zero-digit record, a zero mask word, the words whose
rounding carry wraps, and slices against the uncut call.  Every key is random words: only word equality is asserted."""
import numpy as np
import pytest

import mk_pack_reference as MP
from support import differing, words

pytestmark = pytest.mark.gpu

GW = 32   # kMkPackWideGroup of thfhe_mk_pack.h: records per workgroup of mk_pack_rows_wide_kernel
EXTREME = np.array([0x7FFFFFFF, -0x80000000, -1, 1, 0x7FFFFFFE], np.int64).astype(np.int32)   # 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF: the carry wraps
WIDE, DIRECT = "mk_pack_rows_wide_kernel", "mk_pack_rows_kernel"
DEFAULT = 4096   # kMkPackWideDefault of thfhe_mk_pack.h: the threshold a context starts with, restored after a test has forced a kernel


def _ctx(O, name, seed, **over):
    """a context of the reduced set on random key words (no packing call touches the bootstrapping or key-switch key)"""
    import thfhe
    p = O.make_params(name, **over)
    rng = np.random.default_rng(seed)
    bk = rng.integers(-2**63, 2**63, O.mk_bk_shape(p), dtype=np.int64)
    return p, thfhe.MKCloudKey(thfhe.make_params(**p.as_dict()), bk, words(rng, *O.mk_ksk_shape(p)), device=0)


def _key(rng, D, t, basebit, N):
    return rng.integers(-2**63, 2**63, (D, t, (1 << basebit) - 1, 2, N), dtype=np.int64)


def _records(rng, count, D, sparse=False):
    """sparse (the D = N keys of the larger rings, whose model sums are slow): non-zero mask words only at the ends of the record and on either
    side of the kernel's 256-word chunk seams, so that every index range still meets its ends"""
    recs = words(rng, count, D + 1)
    if sparse:
        keep = np.zeros(D + 1, bool)
        keep[D] = True
        for c in range(0, D + 1, 256):
            keep[max(c - 6, 0):min(c + 6, D)] = True
        recs[:, ~keep] = 0
    recs[0, :D] = 0                                  # every digit zero: the record's sum is (0, b 2^32)
    if count > 1:
        recs[1, 0] = 0                               # a zero mask word among others
        k = min(D - 1, len(EXTREME))
        recs[1, 1:1 + k] = EXTREME[:k]
        recs[count - 1, D - k:D] = EXTREME[:k]       # ... and on the last record of the last group
    return recs


def _counts(p):
    """GW - p, GW, GW + p and 3 GW + p records, each rounded up to a whole number of tables of p records (p = 64: 64, 128, 192): one short of a
    group, a full group, a group and a partial one, three groups and a partial one"""
    return sorted({-(-c // p) * p for c in (GW - p, GW, GW + p, 3 * GW + p) if c > 0})


def _both(ck, recs, p):
    """the call through the wide kernel and through the direct one, the dispatch asserted by name"""
    n = recs.shape[0]
    ck.set_pack_wide_threshold(1)
    try:
        assert ck.pack_kernel_name(n) == WIDE
        wide = ck.pack_boxes(recs, p)
        ck.set_pack_wide_threshold(0)
        assert ck.pack_kernel_name(n) == DIRECT
        direct = ck.pack_boxes(recs, p)
    finally:
        ck.set_pack_wide_threshold(DEFAULT)
    return wide, direct


def _check(ck, pk, t, basebit, p, count, rng, sparse=False):
    D = pk.shape[0]
    recs = _records(rng, count, D, sparse)
    (wa, wb), (da, db) = _both(ck, recs, p)
    tag = (D, t, basebit, p, count)
    assert wa.shape == wb.shape == (count // p, pk.shape[-1])
    assert np.array_equal(wa, da), (tag, differing(wa, da))
    assert np.array_equal(wb, db), (tag, differing(wb, db))
    ra, rb = MP.pack(recs, pk, t, basebit, p)
    assert np.array_equal(wa, ra), (tag, differing(wa, ra))
    assert np.array_equal(wb, rb), (tag, differing(wb, rb))
    return recs, (wa, wb)


@pytest.fixture(scope="module")
def mk2(O):
    p, ck = _ctx(O, "MK2", 903, n=30)
    yield p, ck
    ck.close()


@pytest.mark.parametrize("t,basebit", [(8, 2), (4, 3), (16, 2), (5, 1)])
def test_n1024_lwe_key_shapes(O, mk2, t, basebit):
    p, ck = mk2
    rng = np.random.default_rng(3000 + 10 * t + basebit)
    pk = _key(rng, p.parties * p.n, t, basebit, p.N)     # D = 60: no multiple of the 256-word chunk
    ck.pack_key_set(pk, t, basebit)
    for pp in (2, 4, 64):
        for count in _counts(pp):
            _check(ck, pk, t, basebit, pp, count, rng)


@pytest.mark.parametrize("t,basebit,pp", [(5, 1, 4), (8, 2, 2)])
def test_n1024_ring_key_shape(O, mk2, t, basebit, pp):
    # D = N, the tree's key: four chunks of mask words per record
    p, ck = mk2
    rng = np.random.default_rng(4000 + t)
    pk = _key(rng, p.N, t, basebit, p.N)
    ck.pack_key_set(pk, t, basebit)
    for count in (GW - pp, GW + pp):
        _check(ck, pk, t, basebit, pp, count, rng)


@pytest.mark.parametrize("name,over,lwe_shape,ring_shape", [
    ("MK4-N2048", dict(n=10, parties=2), (8, 2), (2, 2)),
    ("MK64-fft", dict(n=4, parties=2), (4, 3), (1, 1)),   # one-bit digits: a 256 MiB D = N key; this ring's multi-bit digits come with the D = P n key
])
def test_larger_rings(O, name, over, lwe_shape, ring_shape):
    p, ck = _ctx(O, name, 904, **over)
    try:
        rng = np.random.default_rng(p.N + 1)
        t, basebit = lwe_shape
        pk = _key(rng, p.parties * p.n, t, basebit, p.N)
        ck.pack_key_set(pk, t, basebit)
        # few tables of small p here: the model multiplies N / p monomials per table; every (p, count) pair runs at N = 1024 above
        for pp, count in ((4, GW - 4), (2, 2), (64, 128), (8, 3 * GW + 8)):
            _check(ck, pk, t, basebit, pp, count, rng)
        t, basebit = ring_shape
        pk = _key(rng, p.N, t, basebit, p.N)
        ck.pack_key_set(pk, t, basebit)
        for pp, count in ((8, GW - 8), (4, GW + 4)):
            _check(ck, pk, t, basebit, pp, count, rng, sparse=True)
    finally:
        ck.close()


def test_slices_thresholds_and_names(O, mk2):
    import thfhe
    p, ck = mk2
    rng = np.random.default_rng(78)
    D = p.parties * p.n
    pk = _key(rng, D, 8, 2, p.N)
    ck.pack_key_set(pk, 8, 2)
    recs, whole = _check(ck, pk, 8, 2, 4, 3 * GW + 4, rng)
    assert [ck.pack_kernel_name(n) for n in (DEFAULT - 1, DEFAULT)] == [DIRECT, WIDE]      # the default a context starts with and _both restores
    try:
        # slices of two groups, of one group and of one table give the words of the uncut call, through either kernel
        for slice_, thr in ((2 * GW, 1), (GW, 1), (4, 1), (GW, 0), (GW, GW), (GW + 4, GW + 4)):
            ck.set_tree_slice(slice_)
            ck.set_pack_wide_threshold(thr)
            parts = ck.pack_boxes(recs, 4)
            assert np.array_equal(whole[0], parts[0]) and np.array_equal(whole[1], parts[1]), (slice_, thr)
        # the threshold is a record count: at it and above the wide kernel, below it the direct one; 0 is never
        ck.set_pack_wide_threshold(GW)
        assert [ck.pack_kernel_name(n) for n in (0, GW - 1, GW, GW + 1, 1 << 20)] == [DIRECT, DIRECT, WIDE, WIDE, WIDE]
        ck.set_pack_wide_threshold(0)
        assert [ck.pack_kernel_name(n) for n in (0, 1, 1 << 20)] == [DIRECT] * 3
    finally:
        ck.set_tree_slice(16384)
        ck.set_pack_wide_threshold(DEFAULT)
    assert ck.pack_boxes(recs[:0], 4)[0].shape == (0, p.N)
    with pytest.raises(thfhe.ThfheError):
        ck.pack_boxes(recs[:10], 4)                          # a refused call leaves the dispatch as it was
    again = ck.pack_boxes(recs, 4)
    assert np.array_equal(whole[0], again[0]) and np.array_equal(whole[1], again[1])
