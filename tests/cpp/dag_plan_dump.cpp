// dag_plan_dump -- prints what the gate-DAG planner (torus-fhe_amd/csrc/thfhe_dag.h) makes of a corpus of node lists: for every list either the
// return code and message of the refusal, or the whole plan (launch groups in order, index table, sizing figures, the four stats).  Host code only:
// no HIP call, no GPU.  tests/test_dag_plan.py builds it under AddressSanitizer + UBSan and compares the output with tests/golden/dag_plans.txt.
//   (a) hand-written lists: the valid node lists of tests/test_dag_*_host.py with the families of those files, some gate lists, and a few refusals
//       of the family checks;
//   (b) generated lists: a fixed-seed generator, at most 12 rows over 8 inputs, under each of the seven flavours of entry; a row is drawn valid for
//       its flavour or, at a small rate, with one field perturbed.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../torus-fhe_amd/csrc/thfhe_dag.h"

static std::string g_msg;
namespace thfhe {
int thfhe_fail(int code, const char *msg) {
    g_msg = msg ? msg : "";
    return code;
}
int thfhe_fail_hip(hipError_t, const char *what) {
    g_msg = std::string("HIP error in ") + (what ? what : "?");
    return THFHE_E_HIP;
}
}  // namespace thfhe

namespace {

enum Flavour { SK4, MK4, SK_LUT, MK_LUT, TREE, MV, LHE, N_FLAVOURS };
const char *const kFlavourName[N_FLAVOURS] = {"sk4", "mk4", "lut", "mk_lut", "tree", "mv", "lhe"};

// the engines' gate classes (thfhe_sk.hip: sk_dag_classify, thfhe_mk.hip: mk_dag_classify)
int sk_classify(int op) { return op == THFHE_NOT || op == THFHE_COPY ? 2 : (op == THFHE_MUX ? 1 : (op >= THFHE_NAND && op <= THFHE_ORYN ? 0 : -1)); }
int mk_classify(int op) {
    if (op == THFHE_NOT || op == THFHE_COPY) return 2;
    if (op == THFHE_MUX) return 1;
    if (op == THFHE_AND3) return 3;
    return op == THFHE_NAND || op == THFHE_OR || op == THFHE_AND || op == THFHE_XOR ? 0 : -1;
}

// The table families of a call.  The planner reads the spec arrays and the word pool; of every other family only whether its pointer is null.
struct Fam {
    std::vector<thfhe_lut_spec> specs;
    int n_specs = -1;   // -1: specs.size()
    bool tv = true;
    int n_luts = 2;
    bool enc_a = false, enc_b = false;
    int n_enc = 0;
    std::vector<thfhe_tree_spec> trees;
    bool tv1 = false;
    int n_tv1_rows = 0;
    std::vector<thfhe_mv_spec> mvs;
    bool tv0 = false, fac = false;
    int n_bases = 0;
    size_t n_factor_words = 0;
    bool lhe = false;
    int n_sets = 0;
    std::vector<thfhe_dag_lhe_spec> lks;
    bool tab = false, fin = false;
    int n_tab_rows = 0, n_fin_rows = 0;
    std::vector<thfhe_dag_wfa_spec> wfas;
    std::vector<int32_t> pool;
};

const thfhe_lut_spec ONE{1, {1, 0, 0}, 0, 1}, ONE2{1, {1, 0, 0}, 0, 2}, TWO{2, {1, 1, 0}, 0, 1}, TWO_MV{2, {1, 2, 0}, 0, 1};
const std::vector<thfhe_lut_spec> SPECS = {{1, {1, 0, 0}, 0, 1}, {2, {1, 1, 0}, 0, 2}, {3, {1, 1, 1}, 0, 4}};
const std::vector<thfhe_tree_spec> TREES = {{ONE, ONE, 4}, {ONE2, TWO, 4}, {TWO, TWO, 8}};   // trees[2]: four operands
// (lo, hi, p, q, k, base, factors_off, n_tables): an MV spec with q = 3 and two tables, a TREE_MV spec with k = 2 outputs of p_hi = 4, an MV spec at q = 1
const std::vector<thfhe_mv_spec> MVS = {{TWO_MV, ONE, 8, 3, 1, 0, 0, 2}, {ONE, TWO_MV, 4, 4, 2, 1, 48, 1}, {ONE, ONE, 2, 1, 1, 1, 80, 1}};
// (set, d_tree, d_rot, theta): a lookup spec with theta = 2, a gather spec at d = 1 + 2, a lookup-only spec (d_rot = 0)
const std::vector<thfhe_dag_lhe_spec> LKS = {{0, 1, 2, 2}, {1, 1, 2, 1}, {0, 2, 0, 1}};
const std::vector<thfhe_dag_wfa_spec> WFAS = {{2, 3, 2, 2, 0, 2, 0, 12, 14}};
const std::vector<int32_t> POOL = {1, 2, 2, 0, 0, 1, 0, 0, 2, 1, 1, 2, 16, 1, 2, 0};

Fam fam_lut() {   // tests/test_dag_lut_host.py
    Fam F;
    F.specs = SPECS;
    return F;
}
Fam fam_tree() {   // tests/test_dag_tree_host.py
    Fam F = fam_lut();
    F.enc_a = F.enc_b = true, F.n_enc = 2;
    F.trees = TREES;
    F.tv1 = true, F.n_tv1_rows = 6;
    return F;
}
Fam fam_mv() {   // tests/test_dag_mv_host.py
    Fam F;
    F.specs = {ONE};
    F.trees = {{ONE, ONE, 4}};
    F.tv1 = true, F.n_tv1_rows = 4;
    F.mvs = MVS;
    F.tv0 = F.fac = true, F.n_bases = 2, F.n_factor_words = 82;
    return F;
}
Fam fam_lhe() {   // tests/test_dag_lhe_host.py
    Fam F;
    F.specs = {ONE};
    F.lhe = true, F.n_sets = 2;
    F.lks = LKS, F.wfas = WFAS, F.pool = POOL;
    F.tab = F.fin = true, F.n_tab_rows = 6, F.n_fin_rows = 4;
    return F;
}
Fam fam_all() {   // the generated lists: every family of the three files above
    Fam F = fam_tree(), L = fam_lhe();
    F.mvs = MVS;
    F.tv0 = F.fac = true, F.n_bases = 2, F.n_factor_words = 82;
    F.lhe = true, F.n_sets = 2;
    F.lks = L.lks, F.wfas = L.wfas, F.pool = L.pool;
    F.tab = F.fin = true, F.n_tab_rows = 6, F.n_fin_rows = 4;
    return F;
}

using Rows = std::vector<std::vector<int32_t>>;

// ---- the calls of the planner: one per flavour of entry ----
int plan_list(Flavour fl, const Fam &F, size_t n_inputs, const Rows &rows, const std::vector<int32_t> &out_wires, DagPlan &plan) {
    static int32_t word = 0;   // what a non-null host array points to: the planner does not read it
    static const thfhe_tgsw_set *const no_sets[64] = {};
    const size_t stride = fl == SK4 || fl == MK4 ? 4 : 6;
    std::vector<int32_t> nodes;
    for (const auto &r : rows) nodes.insert(nodes.end(), r.begin(), r.begin() + stride);
    auto ptr = [](bool have) { return have ? &word : nullptr; };
    const DagCall A{&word, n_inputs, nodes.data(), rows.size(), out_wires.data(), out_wires.size(), &word};
    if (fl == SK4) return dag_plan(A, DagFamilies{}, sk_classify, plan);
    if (fl == MK4) return dag_plan(A, DagFamilies{}, mk_classify, plan);
    // each entry fills the families it has, as thfhe_sk.hip and thfhe_mk.hip do
    DagFamilies T{kDagGenLut, F.specs.empty() ? nullptr : F.specs.data(), F.n_specs < 0 ? (int)F.specs.size() : F.n_specs, ptr(F.tv), F.n_luts};
    if (fl == SK_LUT) return dag_checked_plan(A, T, sk_classify, plan);
    if (fl == MK_LUT) return dag_checked_plan(A, T, mk_classify, plan);
    T.gens |= kDagGenTree, T.tv = ptr(F.tv && F.n_luts);
    T.enc_a = ptr(F.enc_a), T.enc_b = ptr(F.enc_b), T.n_enc = F.n_enc;
    T.trees = F.trees.empty() ? nullptr : F.trees.data(), T.n_trees = (int)F.trees.size(), T.tv1 = ptr(F.tv1), T.n_tv1_rows = F.n_tv1_rows;
    if (fl >= MV) {
        T.gens |= kDagGenMv, T.mvs = F.mvs.empty() ? nullptr : F.mvs.data(), T.n_mvs = (int)F.mvs.size();
        T.mv_tv0 = ptr(F.tv0), T.n_bases = F.n_bases, T.mv_factors = ptr(F.fac), T.n_factor_words = F.n_factor_words;
    }
    const thfhe_dag_lhe_families lhe{F.n_sets ? no_sets : nullptr, F.n_sets, F.lks.empty() ? nullptr : F.lks.data(), (int32_t)F.lks.size(), nullptr,
                                     ptr(F.tab), F.n_tab_rows, F.wfas.empty() ? nullptr : F.wfas.data(), (int32_t)F.wfas.size(),
                                     F.pool.empty() ? nullptr : F.pool.data(), F.pool.size(), nullptr, ptr(F.fin), F.n_fin_rows};
    if (fl == LHE && F.lhe) T.gens |= kDagGenLhe, T.lhe = &lhe;
    return dag_checked_plan(A, T, sk_classify, plan);
}

void dump(const char *name, Flavour fl, const Fam &F, size_t n_inputs, const Rows &rows, const std::vector<int32_t> &out_wires = {}) {
    const size_t stride = fl == SK4 || fl == MK4 ? 4 : 6;
    std::printf("list %s %s n_inputs=%zu n_rows=%zu\n", kFlavourName[fl], name, n_inputs, rows.size());
    for (const auto &r : rows) {
        std::printf(" row");
        for (size_t q = 0; q < stride; q++) std::printf(" %d", r[q]);
        std::printf("\n");
    }
    DagPlan plan;
    g_msg.clear();
    const int rc = plan_list(fl, F, n_inputs, rows, out_wires, plan);
    if (rc) {
        std::printf(" rc %d: %s\n", rc, g_msg.c_str());
        return;
    }
    std::printf(" rc 0\n");
    for (const DagBatch &b : plan.batches) std::printf(" batch %d %d %d %zu %d\n", b.depth, b.sub, b.cls, b.count, b.tree);
    std::printf(" tab");
    for (int32_t v : plan.tab) std::printf(" %d", v);
    std::printf("\n max_width %zu max_rot %zu max_theta %d rotations %lld max_depth %d\n", plan.max_width, plan.max_rot, plan.max_theta,
                (long long)plan.rotations, plan.max_depth);
    int64_t st[4] = {-1, -1, -1, -1};
    plan.fill_stats(st);
    std::printf(" stats %lld %lld %lld %lld\n", (long long)st[0], (long long)st[1], (long long)st[2], (long long)st[3]);
}

constexpr int32_t NAND = THFHE_NAND, XOR = THFHE_XOR, ORYN = THFHE_ORYN, MUX = THFHE_MUX, NOT = THFHE_NOT, COPY = THFHE_COPY, AND3 = THFHE_AND3,
                  LUT = THFHE_LUT, LUT_ENC = THFHE_LUT_ENC, SELECT = THFHE_SELECT, TREE_ = THFHE_TREE, MV_ = THFHE_MV, TREE_MV = THFHE_TREE_MV,
                  LOOKUP = THFHE_LHE_LOOKUP, GATHER = THFHE_LHE_GATHER, WFA = THFHE_LHE_WFA;
std::vector<int32_t> OUT(int32_t head) { return {THFHE_LUT_OUT, head, -1, -1, -1, -1}; }

void hand_written() {
    // gate lists: a NOT reading a NOT of the same depth (and a COPY reading that), a MUX, linear gates on an input; AND3 for the multi-key engine
    const Rows gates = {{NAND, 0, 1, -1, -1, -1}, {NOT, 3, -1, -1, -1, -1}, {NOT, 4, -1, -1, -1, -1}, {COPY, 5, -1, -1, -1, -1}, {MUX, 0, 4, 6, -1, -1},
                        {XOR, 6, 7, -1, -1, -1},  {NOT, 2, -1, -1, -1, -1}, {NAND, 9, 5, -1, -1, -1}, {NOT, 10, -1, -1, -1, -1}};
    Rows gates_sk = gates, gates_mk = gates;
    gates_sk.push_back({ORYN, 8, 11, -1, -1, -1});
    gates_mk.push_back({AND3, 8, 11, 2, -1, -1});
    for (Flavour fl : {SK4, SK_LUT, TREE, MV, LHE}) dump("gates", fl, fam_all(), 3, gates_sk);
    for (Flavour fl : {MK4, MK_LUT}) dump("gates", fl, fam_all(), 3, gates_mk);
    dump("gates_of_the_other_engine", SK4, fam_all(), 3, gates_mk);
    dump("gates_of_the_other_engine", MK_LUT, fam_all(), 3, gates_sk);
    dump("empty", SK4, fam_all(), 3, {});
    dump("empty", LHE, fam_all(), 0, {});
    // tests/test_dag_lut_host.py: OK_ROWS, and the rows of test_lut_node_rows_wires_and_dedup (a LUT with theta 4)
    const Rows lut_ok = {{LUT, 0, 1, -1, 1, 0}, OUT(3), {NAND, 3, 4, -1, -1, -1}, {LUT, 2, -1, -1, 0, 1}, {NOT, 6, -1, -1, -1, -1}};
    for (Flavour fl : {SK_LUT, MK_LUT, TREE}) dump("lut_host_OK_ROWS", fl, fam_lut(), 3, lut_ok);
    dump("lut_host_OK_ROWS_out_wires", SK_LUT, fam_lut(), 3, lut_ok, {0, 7, 3});
    dump("lut_host_OK_ROWS_out_wires", SK_LUT, fam_lut(), 3, lut_ok, {0, 8});
    Fam dedup = fam_lut();
    dedup.specs = {{2, {1, 1, 0}, 0, 2}, {1, {1, 0, 0}, 0, 4}, {3, {1, -2, 3}, -5, 1}};
    const Rows lut_dedup = {{LUT, 0, 1, -1, 0, 0}, OUT(3), {NAND, 3, 2, -1, -1, -1}, {LUT, 2, -1, -1, 1, 1}, OUT(6), OUT(6), OUT(6), {LUT, 1, 2, -1, 0, 0}, OUT(10),
                            {LUT, 0, 1, 5, 2, 1}};
    for (Flavour fl : {SK_LUT, MK_LUT, MV}) dump("lut_host_theta_4", fl, dedup, 3, lut_dedup);
    // tests/test_dag_tree_host.py: OK_ROWS, and the two lists of test_circuits_without_new_nodes_are_unchanged
    const Rows tree_ok = {{LUT, 0, 1, -1, 1, 0}, OUT(4), {NAND, 4, 5, -1, -1, -1}, {LUT_ENC, 0, 1, 2, 2, 1}, OUT(7), OUT(7), OUT(7), {SELECT, 3, -1, -1, 0, 7},
                          {TREE_, 0, 1, 2, 1, 4}, {TREE_, 11, 12, -1, 0, 2}, {NOT, 13, -1, -1, -1, -1}};
    for (Flavour fl : {TREE, MV, LHE, SK_LUT}) dump("tree_host_OK_ROWS", fl, fam_tree(), 4, tree_ok);
    Fam adder = fam_lut();
    adder.specs = {{2, {1, 1, 0}, 0, 2}, {3, {1, 1, 1}, 0, 2}, {1, {1, 0, 0}, 0, 1}};
    dump("tree_host_lut_adder", TREE, adder, 4, {{LUT, 0, 2, -1, 0, 0}, OUT(4), {LUT, 1, 3, 5, 1, 0}, OUT(6), {LUT, 7, -1, -1, 2, 1}, {NOT, 8, -1, -1, -1, -1}});
    Fam none;
    none.tv = false, none.n_luts = 0;
    dump("tree_host_no_family", TREE, none, 2, {{NAND, 0, 1, -1, -1, -1}});
    dump("tree_host_no_family", LHE, none, 2, {{NAND, 0, 1, -1, -1, -1}});
    // tests/test_dag_mv_host.py: OK_ROWS (a TREE_MV with k = 2), its first four rows, and the TREE list without the multi-value families
    const Rows mv_ok = {{MV_, 0, 1, -1, 0, 1}, OUT(4), OUT(4), {NAND, 0, 1, -1, -1, -1}, {TREE_MV, 2, 0, 1, 1, 0}, OUT(8), {MV_, 3, -1, -1, 2, 0},
                        {LUT, 4, -1, -1, 0, 1}, {SELECT, 10, -1, -1, 0, 4}, {TREE_MV, 8, 9, 12, 1, 0}, OUT(13), {NOT, 13, -1, -1, -1, -1}};
    for (Flavour fl : {MV, LHE, TREE}) dump("mv_host_OK_ROWS", fl, fam_mv(), 4, mv_ok);
    dump("mv_host_OK_ROWS_head", MV, fam_mv(), 4, Rows(mv_ok.begin(), mv_ok.begin() + 4));
    Fam no_mv = fam_mv();
    no_mv.mvs.clear(), no_mv.tv0 = no_mv.fac = false, no_mv.n_bases = 0, no_mv.n_factor_words = 0;
    for (Flavour fl : {MV, TREE}) dump("mv_host_tree_without_mv_families", fl, no_mv, 4, {{NAND, 0, 1, -1, -1, -1}, {TREE_, 0, 1, -1, 0, 0}});
    // tests/test_dag_lhe_host.py: GOOD (a GATHER above a LOOKUP)
    auto LK = [](int32_t lk, int32_t row0) { return std::vector<int32_t>{LOOKUP, -1, -1, -1, lk, row0}; };
    auto GA = [](int32_t lk, int32_t first) { return std::vector<int32_t>{GATHER, -1, -1, -1, lk, first}; };
    auto WF = [](int32_t wfa, int32_t fin0) { return std::vector<int32_t>{WFA, -1, -1, -1, wfa, fin0}; };
    const Rows lhe_good = {LK(0, 4), OUT(8), GA(1, 0), WF(0, 1), OUT(11), OUT(11), OUT(11), LK(2, 2), GA(1, 3)};
    for (Flavour fl : {LHE, MV}) dump("lhe_host_GOOD", fl, fam_lhe(), 8, lhe_good);
    Fam no_lhe = fam_lhe();
    no_lhe.lhe = false;
    dump("lhe_host_GOOD_without_lhe", LHE, no_lhe, 8, lhe_good);
    // every kind on one level and two groups of a kind: the order of the groups of a level
    const Rows level = {WF(0, 0), OUT(8), OUT(8), OUT(8), GA(1, 0), LK(2, 0), LK(0, 0), OUT(14), {TREE_MV, 0, 1, 2, 1, 0}, OUT(16), {MV_, 3, -1, -1, 2, 0},
                        {MV_, 0, 1, -1, 0, 0}, OUT(19), OUT(19), {TREE_, 0, 1, 2, 1, 0}, {TREE_, 4, 5, -1, 0, 0}, {SELECT, 0, 1, -1, 1, 0}, {SELECT, 6, -1, -1, 0, 4},
                        {LUT_ENC, 0, 1, 2, 2, 0}, OUT(26), OUT(26), OUT(26), {LUT_ENC, 1, 2, -1, 1, 1}, OUT(30), {LUT_ENC, 7, -1, -1, 0, 0}, {LUT, 0, 1, 2, 2, 0},
                        OUT(33), OUT(33), OUT(33), {LUT, 1, 2, -1, 1, 1}, OUT(37), {LUT, 7, -1, -1, 0, 0}, {MUX, 0, 1, 2, -1, -1}, {NAND, 0, 1, -1, -1, -1},
                        {NOT, 0, -1, -1, -1, -1}, LK(2, 1), {MV_, 5, -1, -1, 2, 0}, {NAND, 41, 3, -1, -1, -1}};
    dump("one_level_every_kind", LHE, fam_all(), 8, level);
    // the family checks, one refusal each
    Fam F = fam_all();
    const Rows nand = {{NAND, 0, 1, -1, -1, -1}};
    F.tv = false;
    dump("family_tv_null", SK_LUT, F, 2, nand);
    dump("family_tv_null", TREE, F, 2, nand);
    F = fam_all(), F.n_specs = 0;
    dump("family_n_specs_0", MK_LUT, F, 2, nand);
    dump("family_n_specs_0", TREE, F, 2, nand);
    F = fam_all(), F.n_luts = 1025;
    dump("family_n_luts", SK_LUT, F, 2, nand);
    dump("family_n_luts", MV, F, 2, nand);
    F = fam_all(), F.enc_b = false;
    dump("family_enc_b_null", TREE, F, 2, nand);
    F = fam_all(), F.n_enc = (1 << 18) + 1;
    dump("family_n_enc", LHE, F, 2, nand);
    F = fam_all(), F.trees[0].p_hi = 6;
    dump("family_p_hi", TREE, F, 2, nand);
    F = fam_all(), F.specs[1].theta = 3;
    dump("family_spec_theta", SK_LUT, F, 2, nand);
    dump("family_spec_theta", MV, F, 2, nand);
    F = fam_all(), F.n_tv1_rows = -1;
    dump("family_n_tv1_rows", TREE, F, 2, nand);
    F = fam_all(), F.tv0 = false;
    dump("family_tv0_null", MV, F, 2, nand);
    dump("family_tv0_null", TREE, F, 2, nand);   // an entry without the family does not look at it
    F = fam_all(), F.n_factor_words = ((size_t)1 << 28) + 1;
    dump("family_n_factor_words", LHE, F, 2, nand);
    F = fam_all(), F.tab = false;
    dump("family_tab_b_null", LHE, F, 2, nand);
    dump("family_tab_b_null", MV, F, 2, nand);
    F = fam_all(), F.n_sets = 65;
    dump("family_n_sets", LHE, F, 2, nand);
    F = fam_all(), F.pool.clear();
    dump("family_no_pool", LHE, F, 8, {WF(0, 0), OUT(8), OUT(8), OUT(8)});
    F = fam_all(), F.enc_a = F.enc_b = false, F.n_enc = 0;
    dump("family_no_enc", TREE, F, 2, {{LUT_ENC, 0, -1, -1, 0, 0}});
    F = fam_all(), F.tv1 = false, F.n_tv1_rows = 0;
    dump("family_no_tv1", MV, F, 2, {{TREE_, 0, 1, -1, 0, 0}});
    F = fam_all(), F.tv0 = false, F.n_bases = 0;
    dump("family_no_bases", MV, F, 2, {{MV_, 0, -1, -1, 2, 0}});
    dump("output_wire", TREE, fam_all(), 2, nand, {3});
}

// ---- (b) the generator ----
struct Rng {   // splitmix64: the same sequence everywhere
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    int32_t below(int32_t n) { return (int32_t)(next() % (uint64_t)n); }   // 0 .. n-1
};

constexpr int kGenInputs = 8, kGenMaxRows = 12, kGenLists = 48, kPerturbPercent = 18;

// One node drawn valid for the flavour over the families of fam_all(), with the LUT_OUT rows it needs; `room` rows are left.
void draw_node(Rng &R, Flavour fl, int32_t w, int room, Rows &rows) {
    auto wire = [&] { return R.below(w); };
    auto push = [&](std::vector<int32_t> head, int outs) {
        rows.push_back(head);
        for (int j = 0; j < outs; j++) rows.push_back(OUT(w));
    };
    const bool mk = fl == MK4 || fl == MK_LUT;
    const int kinds = fl == SK4 || fl == MK4 ? 1 : (fl == SK_LUT || fl == MK_LUT ? 2 : (fl == TREE ? 5 : (fl == MV ? 7 : 10)));
    for (;;) {
        const int kind = R.below(kinds + 1) % kinds;   // gates twice as often as any other kind
        switch (kind) {
        case 0: {   // a gate of the engine
            const int g = R.below(mk ? 8 : 13);
            if (mk) {
                static const int32_t ops[8] = {THFHE_NAND, THFHE_OR, THFHE_AND, THFHE_XOR, THFHE_MUX, THFHE_NOT, THFHE_COPY, THFHE_AND3};
                const int32_t op = ops[g];
                const int nin = op == THFHE_NOT || op == THFHE_COPY ? 1 : (op == THFHE_MUX || op == THFHE_AND3 ? 3 : 2);
                return push({op, wire(), nin > 1 ? wire() : -1, nin > 2 ? wire() : -1, -1, -1}, 0);
            }
            const int nin = g == THFHE_NOT || g == THFHE_COPY ? 1 : (g == THFHE_MUX ? 3 : 2);
            return push({g, wire(), nin > 1 ? wire() : -1, nin > 2 ? wire() : -1, -1, -1}, 0);
        }
        case 1:     // LUT: specs[s] has s + 1 operands and theta 1 << s
        case 2: {   // LUT_ENC
            const int s = R.below(3);
            if ((1 << s) > room) continue;
            return push({kind == 1 ? LUT : LUT_ENC, wire(), s > 0 ? wire() : -1, s > 1 ? wire() : -1, s, R.below(2)}, (1 << s) - 1);
        }
        case 3: {   // SELECT on trees[t]: t + 1 index operands, p_hi = 4, 4, 8 candidates
            const int t = R.below(3), p = t == 2 ? 8 : 4;
            return push({SELECT, wire(), t > 0 ? wire() : -1, -1, t, R.below(w - p + 1)}, 0);
        }
        case 4: {   // TREE on trees[0] (1 + 1 operands, R = 4 of the 6 rows) or trees[1] (1 + 2 operands, R = 2)
            const int t = R.below(2);
            return push({TREE_, wire(), wire(), t ? wire() : -1, t, R.below(t ? 5 : 3)}, 0);
        }
        case 5: {   // MV on mvs[0] (two operands, q = 3, two tables) or mvs[2] (one operand, q = 1)
            const int m = R.below(2) * 2;
            if (m == 0 && room < 3) continue;
            return push({MV_, wire(), m == 0 ? wire() : -1, -1, m, m == 0 ? R.below(2) : 0}, m == 0 ? 2 : 0);
        }
        case 6:     // TREE_MV on mvs[1]: 1 + 2 operands, k = 2
            if (room < 2) continue;
            return push({TREE_MV, wire(), wire(), wire(), 1, 0}, 1);
        case 7: {   // LOOKUP on lks[l]: 2^d_tree = 2, 2, 4 of the 6 rows, theta = 2, 1, 1
            const int l = R.below(3);
            if (l == 0 && room < 2) continue;
            return push({LOOKUP, -1, -1, -1, l, R.below(l == 2 ? 3 : 5)}, l == 0 ? 1 : 0);
        }
        case 8:     // GATHER on lks[1]: 8 candidates
            return push({GATHER, -1, -1, -1, 1, R.below(w - 8 + 1)}, 0);
        default:    // WFA on wfas[0]: 3 of the 4 final rows, n_out theta = 4 wires
            if (room < 4) continue;
            return push({WFA, -1, -1, -1, 0, R.below(2)}, 3);
        }
    }
}

void generated() {
    const Fam F = fam_all();
    for (int fl = 0; fl < N_FLAVOURS; fl++) {
        Rng R{0x5EEDDA60000ull + (uint64_t)fl};
        for (int i = 0; i < kGenLists; i++) {
            const int n_rows = 1 + R.below(kGenMaxRows);
            Rows rows;
            while ((int)rows.size() < n_rows) {
                const size_t first = rows.size();
                draw_node(R, (Flavour)fl, (int32_t)(kGenInputs + first), n_rows - (int)first, rows);
                for (size_t r = first; r < rows.size(); r++) {
                    if (R.below(100) >= kPerturbPercent) continue;
                    static const int32_t values[10] = {-1, -2, 0, 1, 3, 7, 12, 19, 64, 100000};
                    const int field = R.below(fl == SK4 || fl == MK4 ? 4 : 6);
                    rows[r][field] = field == 0 ? R.below(26) - 1 : values[R.below(10)];   // an opcode -1 .. 24, or a value that is often out of range
                }
            }
            char name[32];
            std::snprintf(name, sizeof name, "gen_%02d", i);
            dump(name, (Flavour)fl, F, kGenInputs, rows);
        }
    }
}

}  // namespace

int main() {
    hand_written();
    generated();
    return 0;
}
