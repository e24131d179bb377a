"""The opening of a CMux -- X^a acc - acc cut into gadget digits -- over the rotation amounts on the 3-gen multi-key rotation kernels of the MI355X
(pytest -m gpu): the sets and the kernel table of test_gpu_mk_rotation_ends.py at n = 1 and two parties, so that a record (a_0, a_1, b) runs at most
one CMux per party, through lut_bootstrap_enc_wo_keyswitch at theta = 1 with b chosen so that barb = 0: the accumulator entering the first CMux is the
caller's table, word for word -- the Torus64 edge tables of tests/decomp_edges.py (every digit edge at every amount, the 9-bit part split of the tlev
and r4k kernels included; asserted on the CPU by test_decomp_edges_host.py) and one uniform random table.

The N = 1024 kernels (coop, pair) take EVERY amount, the N = 2048 and N = 4096 kernels the structured set (every lane residue, every register, the
neighbours of 0, N/2, N and 3N/2, 2N - 1, and 64 random amounts).  Each amount runs on party 0 alone and on party 1 alone (on the edge table that
decomp_edges.tables_at gives it: the condition the host test asserts) and on both parties with different amounts (the random table; the second CMux
then reads what the first wrote), which reaches the key rows of both parties and the skipped step of each.  Every call has an odd job count and
stays on the kernel the table names; every output word equals the reference composed from the CPU oracle's CMux (mk_pack_reference's
lut_enc_wo_keyswitch step by step; its word-by-word extraction mk_lut_reference.extract_at is applied in the vectorised form
conv_edges.extract_at64, and held against it and against mk_pack_reference.lut_bootstrap_enc on a sample of the jobs).

The CCS and KMS engines' own CMux kernels are out of reach of this recipe -- no call sets their accumulator, so a job there runs many steps (see the
docstring of test_gpu_mk_rotation_ends.py) -- and remain covered by random words only."""
import numpy as np
import pytest

import conv_edges as E
import decomp_edges as D
import mk_lut_reference as R
import mk_pack_reference as MP
from support import pmap
from test_gpu_mk_rotation_ends import KERNELS, SETS, odd_calls

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(O):
    """kernel id -> (params, oracle, context, case) with the id's pair threshold set: test_gpu_mk_rotation_ends.env at n = 1, two parties, plus the
    oracle on the same keys and the set's jobs with their reference, computed once for the kernels that share a set; contexts closed at the end"""
    import thfhe
    made = {}

    def get(kid):
        name, threshold = KERNELS[kid][:2]
        if name not in made:
            p = O.make_params(name, **dict(SETS[name], n=1, parties=2))
            s = O.SIGMAS[name]
            K = O.MKKeys(p, 0xC3050000 + len(made), s["bk"], s["ks"])
            orc = O.MKOracle(p, K.bk, K.ksk)
            made[name] = (p, orc, thfhe.MKCloudKey(thfhe.make_params(**p.as_dict()), K.bk, K.ksk, device=0), case(p, orc))
        made[name][2].set_pair_threshold(threshold)
        return made[name]
    yield get
    for v in made.values():
        v[2].close()


def amounts_of(N, rng):
    if N == 1024:
        return np.arange(2 * N)
    S = D.structured_amounts(N, rng)
    assert D.structured_members(N) <= set(S.tolist()) and {int(v) % 64 for v in S} == set(range(64)) and len(S) >= 2 * N // 64 + 120
    return S


def case(p, orc):
    """(amount pairs int[jobs][2], records, table index, (tv_a, tv_b), reference int32[jobs][1][N+1]) of a parameter set"""
    N = p.N
    rng = np.random.default_rng([0x3C, N, p.l, p.Bgbit])
    S = amounts_of(N, rng)
    other = np.roll(S, len(S) // 3)                                  # the amount party 1 takes where both work
    assert not np.any(other == S)
    edge = D.edge_tables(64, N, p.l, p.Bgbit)
    rnd = rng.integers(-2**63, 2**63, (2, N), dtype=np.int64)
    tv_a, tv_b = np.stack([t[0] for t in edge] + [rnd[0]]), np.stack([t[1] for t in edge] + [rnd[1]])
    jobs = [(a, 0, k) for a in S for k in D.tables_at(a, N)] + [(0, a, k) for a in S for k in D.tables_at(a, N)]
    jobs += [(a, b, D.TABLES) for a, b in zip(S, other)]
    jobs = np.array(jobs)[rng.permutation(len(jobs))]                # neighbouring jobs of a workgroup get unrelated amounts and parties
    pairs, idx = jobs[:, :2], jobs[:, 2].astype(np.int32)
    x = np.concatenate([D.amount_word(pairs, N, rng), D.amount_word(np.zeros(len(pairs), np.int64), N, rng)[:, None]], axis=1)
    for g in rng.integers(0, len(x), 64):
        assert [b % (2 * N) for b in R.bars(x[g], N, 1)] == pairs[g].tolist() + [0]

    def rotate(g):
        acc = MP.acc_start_enc(tv_a[idx[g]], tv_b[idx[g]], 0)
        for q in range(2):
            if pairs[g, q]:
                acc = orc.mux_rotate(q, 0, int(pairs[g, q]), acc)
        return acc
    accs = np.stack(pmap(rotate, range(len(x))))
    ref = E.extract_at64(accs, 0, N)
    for g in rng.integers(0, len(x), 16):
        assert np.array_equal(ref[g], R.extract_at(accs[g], 0, N))
        assert np.array_equal(ref[g], MP.lut_bootstrap_enc(orc, [x[g]], (1,), 0, tv_a[idx[g]], tv_b[idx[g]], 1, keyswitch=False)[0])
    return pairs, x, idx, (tv_a, tv_b), ref[:, None, :], S


@pytest.mark.parametrize("kid", list(KERNELS))
def test_amounts_on_every_party(env, kid):
    p, orc, ck, (pairs, x, idx, (tv_a, tv_b), ref, S) = env(kid)
    name, limit, N = KERNELS[kid][2], KERNELS[kid][3], p.N
    covered = [set(), set()]
    for sl in odd_calls(len(x), limit):
        count = sl.stop - sl.start
        assert count % 2 == 1 and ck.rotation_kernel_name(count) == name
        u = ck.lut_bootstrap_enc_wo_keyswitch(tv_a, tv_b, x[sl], theta=1, lut_index=idx[sl])
        assert u.shape == ref[sl].shape == (count, 1, N + 1)
        bad = np.argwhere(u != ref[sl])
        assert bad.size == 0, ("amounts (party 0, party 1), table, word of the first mismatches",
                               [(pairs[sl.start + g].tolist(), int(idx[sl.start + g]), int(q)) for g, _, q in bad[:6]])
        for q in range(2):
            covered[q] |= set(pairs[sl, q].tolist())
    want = set(S.tolist()) | {0}
    assert covered[0] == covered[1] == want and (N != 1024 or want == set(range(2 * N)))
    alone = [{int(a) for a, b in pairs if not b}, {int(b) for a, b in pairs if not a}]
    assert alone[0] >= set(S.tolist()) and alone[1] >= set(S.tolist())      # ... and each party met every amount while the other skipped its step
