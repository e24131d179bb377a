"""Engine contexts called from two host threads on the MI355X (pytest -m gpu).  DevCtx::mu serialises the calls on a
context and every call makes the context's device current on its own thread; ctypes drops the GIL, so two Python threads really are inside the
library together.  The ops and references are those of tests/ctx_sequence.py: each thread runs its own half of a catalogue three times and every
output word must equal the op's CPU reference -- on one single-key context, on one 3-gen multi-key context, and on one context of each kind at once.

Two threads, one process.  They are daemon threads joined with a timeout: a deadlock fails the test, it does not hold the session."""
import threading

import pytest

import ctx_sequence as CS

pytestmark = pytest.mark.gpu

ROUNDS = 3
JOIN_SECONDS = 120


@pytest.fixture(scope="module")
def engines(O):
    sk = CS.SkEnv(O)
    mk = CS.MkEnv(O, "MK2")
    made = {"sk": (sk, CS.sk_catalogue(sk)), "mk": (mk, CS.mk_catalogue(mk))}
    for env, cat in made.values():
        CS.references(env, cat)
    return made


def worker(ck, dev, ops, errors, done, tag):
    """ROUNDS passes over ops; the first mismatch or error ends the thread and is reported by the test"""
    try:
        prev = "thread start"
        for r in range(ROUNDS):
            for pos, op in enumerate(ops):
                CS.check(op.run(ck, dev), op.reference(dev), op, prev, r * len(ops) + pos)
                prev = op.name
        done.append(tag)
    except BaseException as e:   # noqa: BLE001 -- carried to the main thread
        errors.append((tag, e))


def run_threads(jobs):
    """jobs: two (context, device side, ops); both threads must finish within JOIN_SECONDS with no mismatch"""
    errors, done = [], []
    threads = [threading.Thread(target=worker, args=(ck, dev, ops, errors, done, i), daemon=True) for i, (ck, dev, ops) in enumerate(jobs)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_SECONDS)
    alive = [i for i, t in enumerate(threads) if t.is_alive()]
    assert not alive, "threads %s did not finish within %d s (deadlock?); finished: %s, errors: %s" % (alive, JOIN_SECONDS, done, errors)
    assert not errors, errors
    assert sorted(done) == [0, 1]


def halves(cat):
    """two halves with different families in each, both with small and large ops"""
    fam = CS.families(cat)
    return [[op for op in cat if fam.index(op.family) % 2 == h] for h in range(2)]


@pytest.mark.parametrize("engine", ["sk", "mk"])
def test_two_threads_on_one_context(engines, engine):
    env, cat = engines[engine]
    ck = env.cloud_key()
    dev = env.open(ck)
    try:
        a, b = halves(cat)
        assert a and b and not {op.family for op in a} & {op.family for op in b}
        run_threads([(ck, dev, a), (ck, dev, b)])
        # ... and the context still serves one thread afterwards
        CS.check(cat[0].run(ck, dev), cat[0].reference(dev), cat[0], "the threads", 0)
    finally:
        dev.close()
        ck.close()


def test_two_contexts_on_two_threads(engines):
    (sk, sk_cat), (mk, mk_cat) = engines["sk"], engines["mk"]
    ck_sk, ck_mk = sk.cloud_key(), mk.cloud_key()
    dev_sk, dev_mk = sk.open(ck_sk), mk.open(ck_mk)
    try:
        run_threads([(ck_sk, dev_sk, CS.alternating(sk_cat)[::2] + CS.alternating(sk_cat)[1::2]), (ck_mk, dev_mk, CS.big_then_small(mk_cat))])
    finally:
        dev_sk.close()
        dev_mk.close()
        ck_sk.close()
        ck_mk.close()
