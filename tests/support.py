"""Shared scaffolding of the GPU test families (tests/test_gpu_*.py): constants, the parameter shapes and kernel-name table of the shape sweeps,
small helpers, and the generators behind the `ck`, `pack` and `env` fixtures.  A plain module, not a conftest: the fixtures stay declared in the
test modules, as one-line delegations, so scope, name and lifetime are visible where a test reads them.  Only numpy is imported here; thfhe and
the reference models are imported inside the functions that need them, so importing this module never loads the HIP library."""
import numpy as np

N = 1024
SIGMA = 2.0**-15      # fresh-ciphertext noise of SK-128
SIGMA_BK = 2.0**-25   # its ring noise: encrypted tables and the packing key
# the launch thresholds a context starts with: thfhe_ctx.coop_max_jobs and thfhe_ctx.ring4_max_jobs in thfhe_sk.hip
DEFAULT_COOP = 768
DEFAULT_RING4 = 1024

SHAPES = [  # (n, l, Bgbit, ks_t, ks_basebit): l = 1 .. 4, digits up to SK-80's 10 bits, n = 1, n off the mask padding (37, 33), several key-switch shapes
    (24, 1, 8, 8, 2), (24, 2, 10, 8, 2), (37, 3, 7, 8, 2), (16, 4, 8, 5, 3), (33, 3, 6, 3, 5), (1, 2, 7, 15, 1), (64, 4, 4, 4, 4),
]
KERNELS = [  # (id, coop threshold, ring4 threshold, kernel that does most of a batch below 2 048)
    ("ring8", 0, 0, "sk_blind_rotate_ring_kernel<{l}>"),
    ("ring4", 0, 1024, "sk_blind_rotate_ring_kernel<{l}, 4 waves>"),
    ("coop", 1 << 20, 1024, "sk_blind_rotate_coop_kernel<{l}>"),
    ("split", 6, 6, "sk_blind_rotate_ring_kernel<{l}, 4 waves>"),   # launch_br: 6 rotations on the four-wave ring + the rest cooperative
]


def shape_id(s):
    return "n%d-l%d-Bg%d-ks%dx%d" % s


class thresholds:
    """the kernel choice of a case, restored on the way out"""
    def __init__(self, ck, coop, ring4):
        self.ck, self.coop, self.ring4 = ck, coop, ring4

    def __enter__(self):
        self.ck.set_coop_threshold(self.coop)
        self.ck.set_ring4_threshold(self.ring4)

    def __exit__(self, *exc):
        self.ck.set_coop_threshold(DEFAULT_COOP)
        self.ck.set_ring4_threshold(DEFAULT_RING4)


def pmap(fn, items):
    """independent model jobs on Python threads (ctypes and numpy drop the GIL)"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(fn, items))


def words(rng, *shape):
    """uniform int32 words"""
    return rng.integers(-2**31, 2**31, size=shape, dtype=np.int64).astype(np.int32)


def differing(got, ref):
    """(job, output, word) of the first mismatches, for the assertion message"""
    return np.argwhere(got != ref)[:6].tolist()


def spread_index(rng, count, n_tables):
    """a per-sample table index that uses every table and differs between the two launches of the split case"""
    idx = rng.permutation(np.arange(count) % n_tables).astype(np.int32)
    assert len(set(idx.tolist())) == n_tables
    return idx


def enc_int(K, m, p, seed, sigma=SIGMA):
    import lut_reference as R
    from thfhe import lut
    return R.encrypt_words(K, lut.encode(np.asarray(m), p), sigma, seed)


def dec_int(K, recs, p):
    from thfhe import lut
    return lut.decode(K.phases(recs), p)


def mk_rotate_dev(ck, p, x, mu):
    """thfhe_mk_rotate_partial_dev on the records x: the raw Torus64 accumulators int64[count][2][N] (barb = 0)."""
    import oracle_lib as OL
    import thfhe
    count, words = x.shape[0], p.parties * p.n
    bara = np.array([[OL.lib().oracle_modswitch(int(v), p.N) for v in r[:words]] for r in x], np.int32)
    db, dbb, dacc = thfhe.DeviceBuffer(ck, bara.nbytes), thfhe.DeviceBuffer(ck, 4 * count), thfhe.DeviceBuffer(ck, 16 * count * p.N)
    try:
        db.upload(bara)
        dbb.upload(np.zeros(count, np.int32))
        thfhe._check(thfhe.lib().thfhe_mk_rotate_partial_dev(ck.h, db.ptr, dbb.ptr, int(mu), None, dacc.ptr, count))
        ck.sync()
        return dacc.download((count, 2, p.N), np.int64)
    finally:
        for b in (db, dbb, dacc):
            b.free()


# ---- the generators behind the fixtures: `yield from` them in a fixture of the scope the module wants --------------------------------------

def sk128_cloud_key(sk128):
    """the SK-128 CloudKey on conftest.sk128's key material, closed afterwards"""
    import thfhe
    p, K, orc = sk128
    c = thfhe.CloudKey(thfhe.make_params("SK-128"), K.bk, K.ksk, device=0)
    yield c
    c.close()


def make_pack(K, p, seed, sigma=SIGMA_BK):
    """(PolyContext, packing key): LWE key -> the BOOTSTRAPPING ring key of the same key set."""
    from thfhe import keygen
    from thfhe import threshold as T
    pk = keygen.gen_pack_key(np.random.default_rng(seed), K.lwe_key, K.rlwe_key[0], p.ks_t, p.ks_basebit, sigma)
    pc = T.PolyContext(0)
    pc.set_pack_key(pk, p.ks_t, p.ks_basebit)
    return pc, pk


def sk128_pack(sk128):
    p, K, orc = sk128
    pc, pk = make_pack(K, p, 0x7EE0001)
    yield pc, pk
    pc.close()


def shape_env(O, with_pack=False):
    """shape -> (params, keys, oracle, CloudKey), with_pack: + (PolyContext, packing key); built once per shape, every context closed at the end"""
    import thfhe
    made = {}

    def get(shape):
        if shape not in made:
            n, l, Bgbit, t, bb = shape
            kw = dict(n=n, N=N, k=1, l=l, Bgbit=Bgbit, ks_t=t, ks_basebit=bb, torus_bits=32, parties=1)
            p = O.make_params(**kw)
            K = O.SKKeys(p, 3000 + 7 * n + l, 2.0**-25, 2.0**-15)
            made[shape] = (p, K, O.Oracle(p, K.bk, K.ksk), thfhe.CloudKey(thfhe.make_params(**kw), K.bk, K.ksk, device=0))
            if with_pack:
                made[shape] += make_pack(K, p, 5000 + n)
        return made[shape]
    yield get
    for v in made.values():
        v[3].close()
        if with_pack:
            v[4].close()
