"""The order and the wording of the host refusals of the leveled CMux and lookup entries of both engines (no GPU; DESIGN.md sections 4.15, 4.26):
a call that breaks two rules is answered by the earlier one, the d_rot bound is the ring's log2 N, and the 3-gen texts carry "mk " where the
single-key ones do not.  Every call has a null context; where a set is needed it is a pointer that is never dereferenced."""
import ctypes as C
import itertools

import numpy as np
import pytest

# (symbol prefix, text prefix, ctypes word, largest d_rot)
ENGINES = {"sk": ("thfhe_", "", C.c_int32, 10), "mk": ("thfhe_mk_", "mk ", C.c_int64, 11)}
FAKE = 8   # a set pointer that is never dereferenced: every refusal asked for here comes before the set is looked at


def _entry(engine, name):
    import thfhe
    sym, text, word, rot_max = ENGINES[engine]
    L = thfhe.lib()
    w, o32 = np.zeros(16, np.int64), np.zeros(16, np.int32)
    return getattr(L, sym + name), (lambda: L.thfhe_last_error().decode()), text, w.ctypes.data_as(C.POINTER(word)), thfhe._p32(o32), rot_max, (w, o32)


@pytest.mark.parametrize("engine", ENGINES)
def test_cmux_answers_with_the_earlier_rule(engine):
    """null argument, then bit, then null set"""
    fn, err, text, p, _, _, _keep = _entry(engine, "lhe_cmux")
    rules = [("null argument", dict(d0_b=None)), (text + "lhe_cmux: bit must be 0 .. d-1", dict(bit=16)), ("null tgsw set", dict(set_=None))]
    ok = dict(set_=C.c_void_p(FAKE), bit=0, d1_a=p, d1_b=p, d0_a=p, d0_b=p, out_a=p, out_b=p)
    for (want, first), (_, second) in itertools.combinations(rules, 2):
        v = dict(ok, **second, **first)
        assert fn(None, v["set_"], v["bit"], v["d1_a"], v["d1_b"], v["d0_a"], v["d0_b"], v["out_a"], v["out_b"], 1) == -1
        assert err() == want, (first, second)
    assert fn(None, C.c_void_p(FAKE), -1, p, p, p, p, p, p, 1) == -1 and err() == text + "lhe_cmux: bit must be 0 .. d-1"
    assert ("mk " in err()) == (engine == "mk")


@pytest.mark.parametrize("name", ["lhe_lookup", "lhe_lookup_wo_keyswitch"])
@pytest.mark.parametrize("engine", ENGINES)
def test_lookup_answers_with_the_earlier_rule(engine, name):
    """null argument, then d_tree, d_rot, theta, box, n_tables, table_index, then null set"""
    import thfhe
    fn, err, text, p, q, rot_max, _keep = _entry(engine, name)
    idx = np.array([0, 1, 2, 0], np.int32)
    pre = text + "lhe_lookup: "
    rules = [("null argument", dict(tab_b=None)),
             (pre + "d_tree must be 0 .. 6", dict(d_tree=7)),
             (pre + f"d_rot must be 0 .. {rot_max}", dict(d_rot=12)),
             (pre + "theta must be 1, 2 or 4", dict(theta=3)),
             (pre + "theta must not exceed box = N >> d_rot", dict(d_rot=rot_max, theta=2)),   # box = 1
             (pre + "n_tables 2^d_tree must be 1 .. 262144", dict(n_tables=0)),
             ("table_index out of range (0 .. n_tables-1)", dict(count=4, n_tables=2, index=thfhe._p32(idx))),
             ("null tgsw set", dict(set_=None))]
    ok = dict(set_=C.c_void_p(FAKE), first=0, count=1, d_tree=1, d_rot=2, theta=1, tab_a=None, tab_b=p, n_tables=1, index=None, out=q)

    def call(**kw):
        v = dict(ok, **kw)
        return fn(None, v["set_"], v["first"], v["count"], v["d_tree"], v["d_rot"], v["theta"], v["tab_a"], v["tab_b"], v["n_tables"], v["index"], v["out"])
    for (want, first), (_, second) in itertools.combinations(rules, 2):
        assert call(**dict(second, **first)) == -1   # where both rules set one argument, the earlier rule's value breaks the later rule too
        assert err() == want, (first, second)
    # the d_rot bound is the ring's: 10 is refused on neither engine, 11 on the single-key one alone, 12 on both.  With a null set behind it, a
    # d_rot that passes is answered by "null tgsw set"
    for d_rot, refused in ((10, False), (11, engine == "sk"), (12, True)):
        assert call(d_rot=d_rot, set_=None) == -1
        assert err() == (pre + f"d_rot must be 0 .. {rot_max}" if refused else "null tgsw set"), d_rot
    assert call(d_tree=-1) == -1 and err().startswith("mk ") == (engine == "mk")


@pytest.mark.parametrize("engine", ENGINES)
def test_set_create_answers_with_the_earlier_rule(engine):
    """null argument, then d, then count, then null ctx; the texts word for word"""
    fn, err, text, p, _, _, _keep = _entry(engine, "tgsw_set_create")
    h = C.c_void_p()
    rules = [("null argument", dict(tgsw=None)), (text + "tgsw set: d must be 1 .. 16", dict(d=17)),
             (text + "tgsw set: count must be 1 .. 2^24", dict(count=0)), ("null ctx", {})]
    for (want, first), (_, second) in itertools.combinations(rules, 2):
        v = dict(dict(tgsw=p, count=1, d=3), **second, **first)
        assert fn(None, v["tgsw"], v["count"], v["d"], C.byref(h)) == -1
        assert err() == want and not h.value, (first, second)
