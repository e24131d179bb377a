"""The multi-key packing key switch on the MI355X (pytest -m gpu): thfhe_mk_pack_boxes word for word against the numpy
model (tests/mk_pack_reference.py) at every ring degree, for both key shapes (D = P n and D = N), several digit shapes, table sizes and counts
around the row kernel's record group, on all-zero digits, zero mask words and the words whose rounding carry wraps.  Every key here is random
words: only word equality is asserted, so nothing is generated or decrypted."""
import numpy as np
import pytest

import mk_pack_reference as MP
from support import differing, words

pytestmark = pytest.mark.gpu

GROUP = 4   # kMkPackGroup of thfhe_mk_pack.h: records per workgroup of mk_pack_rows_kernel
EXTREME = np.array([0x7FFFFFFF, -0x80000000, -1, 1, 0x7FFFFFFE], np.int64).astype(np.int32)   # 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF: the carry wraps


def _ctx(O, name, seed, **over):
    """a context of the reduced set on random key words (no packing call touches the bootstrapping or key-switch key)"""
    import thfhe
    p = O.make_params(name, **over)
    rng = np.random.default_rng(seed)
    bk = rng.integers(-2**63, 2**63, O.mk_bk_shape(p), dtype=np.int64)
    return p, thfhe.MKCloudKey(thfhe.make_params(**p.as_dict()), bk, words(rng, *O.mk_ksk_shape(p)), device=0)


def _key(rng, D, t, basebit, N):
    return rng.integers(-2**63, 2**63, (D, t, (1 << basebit) - 1, 2, N), dtype=np.int64)


def _records(rng, count, D):
    recs = words(rng, count, D + 1)
    recs[0, :D] = 0                                  # every digit zero: the record's sum is (0, b 2^32)
    if count > 1:
        recs[1, 0] = 0                               # a zero mask word among others
        k = min(D - 1, len(EXTREME))
        recs[1, 1:1 + k] = EXTREME[:k]
    return recs


def _check(ck, pk, t, basebit, p, count, rng):
    D = pk.shape[0]
    recs = _records(rng, count, D)
    ta, tb = ck.pack_boxes(recs, p)
    ra, rb = MP.pack(recs, pk, t, basebit, p)
    assert ta.shape == tb.shape == (count // p, pk.shape[-1])
    assert np.array_equal(ta, ra), (D, t, basebit, p, count, differing(ta, ra))
    assert np.array_equal(tb, rb), (D, t, basebit, p, count, differing(tb, rb))


def _counts(p):
    # one table, three, and a count that fills one record group and leaves a partial one: tables are made of an even number of records, so a
    # partial group holds two (p = 2: 6 records = one group of four and two more); GROUP p + p crosses the group size at every p
    return sorted({p, 3 * p, GROUP * p + p})


@pytest.fixture(scope="module")
def mk2(O):
    p, ck = _ctx(O, "MK2", 901, n=30)
    yield p, ck
    ck.close()


@pytest.mark.parametrize("t,basebit", [(8, 2), (4, 3), (16, 2), (5, 1)])
def test_n1024_lwe_key_shapes(O, mk2, t, basebit):
    p, ck = mk2
    rng = np.random.default_rng(1000 + 10 * t + basebit)
    pk = _key(rng, p.parties * p.n, t, basebit, p.N)
    ck.pack_key_set(pk, t, basebit)
    for pp in (2, 4, 64):
        for count in _counts(pp):
            _check(ck, pk, t, basebit, pp, count, rng)


@pytest.mark.parametrize("t,basebit,pp", [(5, 1, 4), (8, 2, 2)])
def test_n1024_ring_key_shape_and_key_replacement(O, mk2, t, basebit, pp):
    # D = N (the tree's key: 1 024 mask words per record); then a second pack_key_set replaces it, and a third brings it back
    p, ck = mk2
    rng = np.random.default_rng(2000 + t)
    pk = _key(rng, p.N, t, basebit, p.N)
    ck.pack_key_set(pk, t, basebit)
    for count in _counts(pp):
        _check(ck, pk, t, basebit, pp, count, rng)
    recs = _records(rng, 2 * pp, p.N)
    first = ck.pack_boxes(recs, pp)
    other = _key(rng, p.parties * p.n, 3, 2, p.N)
    ck.pack_key_set(other, 3, 2)
    _check(ck, other, 3, 2, 64, 64, rng)
    ck.pack_key_set(pk, t, basebit)
    again = ck.pack_boxes(recs, pp)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


@pytest.mark.parametrize("name,over,lwe_shape,ring_shape", [
    ("MK4-N2048", dict(n=10, parties=2), (8, 2), (2, 2)),
    ("MK64-fft", dict(n=4, parties=2), (4, 3), (1, 2)),
])
def test_larger_rings(O, name, over, lwe_shape, ring_shape):
    p, ck = _ctx(O, name, 902, **over)
    try:
        rng = np.random.default_rng(p.N)
        for D, (t, basebit), cases in ((p.parties * p.n, lwe_shape, [(2, 2), (4, 12), (64, 64), (2, 10)]), (p.N, ring_shape, [(2, 6), (4, 4)])):   # p = 64 meets these rings with the small key: the box kernel never sees the key
            pk = _key(rng, D, t, basebit, p.N)
            ck.pack_key_set(pk, t, basebit)
            for pp, count in cases:
                _check(ck, pk, t, basebit, pp, count, rng)
    finally:
        ck.close()


def test_trivial_records_slices_and_refusals(O, mk2):
    import thfhe
    from thfhe import lut
    p, ck = mk2
    rng = np.random.default_rng(77)
    D = p.parties * p.n
    pk = _key(rng, D, 8, 2, p.N)
    ck.pack_key_set(pk, 8, 2)
    recs = np.zeros((8, D + 1), np.int32)
    recs[:, D] = words(rng, 8)
    ta, tb = ck.pack_boxes(recs, 4)
    assert not ta.any()
    for g in range(2):
        assert np.array_equal(tb[g], lut.test_vector(recs[4 * g:4 * g + 4, D].astype(np.int64) << 32, 4, N=p.N, torus_bits=64))
    # slices of one table each give the same words as one slice
    recs = _records(rng, 12, D)
    whole = ck.pack_boxes(recs, 4)
    ck.set_tree_slice(4)
    try:
        parts = ck.pack_boxes(recs, 4)
    finally:
        ck.set_tree_slice(16384)
    assert np.array_equal(whole[0], parts[0]) and np.array_equal(whole[1], parts[1])
    for bad_p, count in ((3, 12), (128, 128), (4, 10)):
        with pytest.raises(thfhe.ThfheError):
            ck.pack_boxes(recs[:count] if count <= 12 else np.zeros((count, D + 1), np.int32), bad_p)
    with pytest.raises(thfhe.ThfheError):
        ck.pack_key_set(_key(rng, 7, 2, 2, p.N), 2, 2)          # D is neither N nor P n
    assert ck.pack_boxes(recs[:0], 4)[0].shape == (0, p.N)
    again = ck.pack_boxes(recs, 4)                                # the refused key left the old one in place
    assert np.array_equal(whole[0], again[0]) and np.array_equal(whole[1], again[1])
