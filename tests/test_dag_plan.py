"""The gate-DAG planner (torus-fhe_amd/csrc/thfhe_dag.h) on the CPU, under AddressSanitizer + UBSan: tests/cpp/dag_plan_dump plans a corpus of node
lists -- the valid lists of tests/test_dag_*_host.py and fixed-seed generated ones under each of the seven flavours of entry -- and prints every plan
whole (launch groups in order, index table, sizing figures, stats) or the refusal.  tests/golden/dag_plans.txt is that output as recorded from the
planner before it was given one family record and one node-kind table; the plans must not change."""
import collections
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dag_plans.txt")
FLAVOURS = ["sk4", "mk4", "lut", "mk_lut", "tree", "mv", "lhe"]


def _lists(text):
    """[(flavour, name, 'rc ...' line, lines of the list)]"""
    out = []
    for line in text.splitlines():
        if line.startswith("list "):
            _, flavour, name = line.split()[:3]
            out.append([flavour, name, None, []])
        elif line.startswith(" rc "):
            out[-1][2] = line.strip()
        out[-1][3].append(line)
    return out


def test_the_golden_corpus_accepts_and_refuses_enough():
    lists = _lists(open(GOLDEN).read())
    gen = [l for l in lists if l[1].startswith("gen_")]
    for flavour in FLAVOURS:
        mine = [l for l in gen if l[0] == flavour]
        ok = sum(l[2] == "rc 0" for l in mine)
        assert len(mine) >= 40 and 3 * ok >= len(mine) and 3 * (len(mine) - ok) >= len(mine), (flavour, ok, len(mine))
        assert all(len([r for r in l[3] if r.startswith(" row ")]) <= 12 for l in mine)
    assert len({l[2] for l in gen if l[2] != "rc 0"}) >= 8
    # the hand-written lists: the kinds of plan that must occur among the accepted ones
    hand = {(l[0], l[1]): l[3] for l in lists if not l[1].startswith("gen_") and l[2] == "rc 0"}
    batches = lambda key: [tuple(int(v) for v in r.split()[1:]) for r in hand[key] if r.startswith(" batch ")]   # (depth, sub, cls, count, tree)
    assert {(1, 0, 0), (1, 1, 2), (1, 2, 2), (1, 3, 2)} <= {b[:3] for b in batches(("sk4", "gates"))}           # a NOT reading a NOT of the same depth
    assert any(b[2] == 1 for b in batches(("sk4", "gates")))                                                  # a MUX
    assert any(b[2] == 3 for b in batches(("mk4", "gates")))                                                  # AND3 of the multi-key engine
    assert any(b[2] == 6 for b in batches(("lut", "lut_host_theta_4")))                                       # a LUT with theta 4
    assert any(b[2] == 14 and b[4] == 1 for b in batches(("mv", "mv_host_OK_ROWS")))                          # a TREE_MV with k = 2 (mvs[1])
    lhe = batches(("lhe", "lhe_host_GOOD"))
    assert [b[0] for b in lhe if b[2] == 16] == [1, 2] and [b[0] for b in lhe if b[2] == 15] == [1, 1]        # a GATHER above a LOOKUP
    assert len(collections.Counter(b[2] for b in batches(("lhe", "one_level_every_kind")))) == 16             # every launch class of the single-key engine


def test_the_planner_reproduces_the_golden_plans_under_asan_and_ubsan():
    d = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-s", "-C", d, "dag_plan_dump"], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(d, "dag_plan_dump")], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    want = open(GOLDEN).read()
    if r.stdout != want:
        got, ref = _lists(r.stdout), _lists(want)
        assert len(got) == len(ref), (len(got), len(ref))
        for g, w in zip(got, ref):
            assert g[3] == w[3], "\n".join(["got:"] + g[3] + ["golden:"] + w[3])
    assert r.stdout == want
