"""thfhe_pack_boxes at the box counts and packing-key shapes that tests/test_gpu_tree_lut.py leaves out (pytest -m gpu; DESIGN.md section
4.11): p = 4 .. 256, where the window of N/p coefficients crosses different strides of pack_boxes_kernel's prefix scan; calls below
kPackMfmaMinSamples = 8 samples (the plain packing key switch) and from 8 on (the matrix cores, where the key has int8 planes: 2-bit digits,
t = 4 or 8); packing keys with a small odd n, n = 500 (not a multiple of 64 or 128) and n = 1024.  Every word against
tree_lut_reference.pack_boxes.  Keys and records are random words: the contract is word equality, not decryption."""
import numpy as np
import pytest

import tree_lut_reference as TR

pytestmark = pytest.mark.gpu

N = 1024
KEYS = [  # (n, t, basebit)
    (7, 8, 2),      # small odd n, matrix cores from 8 samples on
    (9, 5, 3),      # 3-bit digits: no int8 planes, the plain key switch at every size
    (500, 8, 2),    # SK-80's n: padded to 512
    (1024, 4, 2),   # SK-lib's n, the four-digit matrix-core shape
]
BOXES = [  # (p, outputs): 4 samples take the plain key switch, everything else has 8 or more
    (4, 1), (4, 3), (32, 2), (64, 1), (128, 3), (256, 1),
]


@pytest.fixture(scope="module")
def contexts():
    """(n, t, basebit) -> (PolyContext, key), one context per key shape"""
    from thfhe import threshold as T
    made = {}

    def get(shape):
        if shape not in made:
            n, t, bb = shape
            rng = np.random.default_rng(31 * n + t)
            pk = rng.integers(-2**31, 2**31, size=(n, t, (1 << bb) - 1, 2, N), dtype=np.int64).astype(np.int32)
            pc = T.PolyContext(0)
            pc.set_pack_key(pk, t, bb)
            made[shape] = (pc, pk)
        return made[shape]
    yield get
    for pc, _ in made.values():
        pc.close()


@pytest.mark.parametrize("p_box,outs", BOXES, ids=["p%d-x%d" % b for b in BOXES])
@pytest.mark.parametrize("key", KEYS, ids=["n%d-ks%dx%d" % k for k in KEYS])
def test_pack_boxes_every_word(contexts, key, p_box, outs):
    from thfhe import threshold as T
    n, t, bb = key
    pc, pk = contexts(key)
    count = p_box * outs
    assert (count < 8) == (p_box == 4 and outs == 1)
    rng = np.random.default_rng(1000 * n + 10 * p_box + outs)
    lwe = rng.integers(-2**31, 2**31, size=(count, n + 1), dtype=np.int64).astype(np.int32)
    lwe[0, :n], lwe[-1, :n] = -2**31, 2**31 - 1                 # the extreme mask words
    a, b = T.PackBoxes(pc, lwe, p_box)
    ra, rb = TR.pack_boxes(lwe, pk, t, bb, p_box)
    assert a.shape == ra.shape == (outs, N) and b.shape == rb.shape
    assert np.array_equal(a, ra), np.argwhere(a != ra)[:6].tolist()
    assert np.array_equal(b, rb), np.argwhere(b != rb)[:6].tolist()
