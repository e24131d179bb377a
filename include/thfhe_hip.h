/*
 * thfhe_hip.h -- C ABI of libthfhe_hip.so, the MI355X-native gate-bootstrapping engine.
 *
 * Drop-in boundary for ONE hot path of Animesh005/Torus-FHE: bootstrapped gate evaluation
 * (blind rotate = n x CMux, sample extraction, key switching).  Reference interfaces replaced
 * (paths relative to the reference tree, J/ = 3-gen-mk-tfhe/src/):
 *
 *   thfhe_gates                      <- gate_nand/or/and/xor/xnor/nor/andny/andyn/orny/oryn/mux/not  J/gates.jl:15-177
 *                                       == libtfhe's extern "C" bootsNAND/AND/OR/XOR/.../MUX/NOT that the C++ side
 *                                       calls (src/KNN_medical_data.cpp:130,142-151,227,388-396; src/Convert.cpp:31)
 *   thfhe_bootstrap                  <- bootstrap(bk, ks, mu, x)                    J/bootstrap.jl:98-101
 *   thfhe_bootstrap_wo_keyswitch     <- bootstrap_wo_keyswitch(bk, mu, x)           J/bootstrap.jl:75-88
 *   thfhe_keyswitch                  <- keyswitch(ks, sample)                       J/keyswitch.jl:45-80
 *   thfhe_ctx_create                 <- BootstrapKey(...) forward_transform step    J/bootstrap.jl:6-15 (key -> transformed key)
 *                                       + KeyswitchKey table upload                 J/keyswitch.jl:7-42
 *   thfhe_mk_*                       <- mk_bootstrap_3gen / mk_gate_*_3gen          J/3gen_mk_internals.jl:99-116, J/3gen_mk_gates.jl:8-150
 *   bootsNAND ... (tfhe_shim.h)      <- the libtfhe symbols themselves (struct-compatible shims)
 *
 * All entry points are plain C: pointers + sizes, no C++/torch types.  Return value: 0 on success,
 * negative THFHE_E_* on failure (thfhe_last_error() gives a message).  There is NO CPU fallback: if
 * no HIP device is usable every compute call fails with THFHE_E_NO_DEVICE.
 *
 * Data layouts (little-endian, row-major, innermost last):
 *   LWE record                  int32[n+1]   = a[0..n), b                       (LweSample, J/lwe.jl:21-29)
 *   extracted LWE record        int32[N+1]
 *   bk_coeff  (single key)      int32[n][(k+1)l][k+1][N], row r = j*l + p (block j, level p) -- libtfhe's
 *                               TGswSample.all_sample order; coefficient domain (Torus32)
 *   ksk       (single key)      int32[N][t][base-1][n+1], entry (i, j, h-1) = KS[h, j, i]    (J/keyswitch.jl:35-38)
 *   MK record (P parties)       int32[P*n+1] = a[p*n + i], b                     (MKLweSample, J/mk_internals.jl:23-37)
 *   mk bk_coeff                 int64[P][n][4][l][N]  (part_1..part_4, level)    (TGswSample_3gen, J/tgsw_3gen.jl:3-20)
 *   mk ksk                      int32[P][N][t][base-1][n+1]
 */
#ifndef THFHE_HIP_H
#define THFHE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct thfhe_params {
    int32_t n;          /* LWE dimension                (lwe_size, J/api.jl:4-21)                     */
    int32_t N;          /* ring degree                  (rlwe_polynomial_degree); 1024 supported      */
    int32_t k;          /* RLWE mask size; 1 supported                                                 */
    int32_t l;          /* gadget decomposition length  (bs_decomp_length); 1..4                       */
    int32_t Bgbit;      /* log2 gadget base             (bs_log2_base); l*Bgbit <= 32, Bgbit <= 10     */
    int32_t ks_t;       /* key-switch length            (ks_decomp_length)                             */
    int32_t ks_basebit; /* key-switch log2 base         (ks_log2_base)                                 */
    int32_t torus_bits; /* 32 = Torus32 ring (single key), 64 = Torus64 ring (3-gen multi-key)         */
    int32_t parties;    /* 1 = single key                                                              */
} thfhe_params;

/* gate opcodes (J/gates.jl; J/3gen_mk_gates.jl for AND3) */
enum thfhe_gate {
    THFHE_NAND = 0, THFHE_OR = 1, THFHE_AND = 2, THFHE_XOR = 3, THFHE_XNOR = 4, THFHE_NOR = 5,
    THFHE_ANDNY = 6, THFHE_ANDYN = 7, THFHE_ORNY = 8, THFHE_ORYN = 9, THFHE_MUX = 10,
    THFHE_NOT = 11, THFHE_COPY = 12, THFHE_AND3 = 13,
    THFHE_LUT = 14,     /* gate-DAG node: programmable bootstrap, output 0 (thfhe_dag_run_lut_batch only) */
    THFHE_LUT_OUT = 15, /* output j > 0 of the LUT node j rows above (thfhe_dag_run_lut_batch, thfhe_dag_run_tree_batch) */
    THFHE_LUT_ENC = 16, /* gate-DAG node: programmable bootstrap of an ENCRYPTED table (thfhe_dag_run_tree_batch only) */
    THFHE_SELECT = 17,  /* gate-DAG node: oblivious pick among p consecutive earlier wires (thfhe_dag_run_tree_batch only) */
    THFHE_TREE = 18,    /* gate-DAG node: two-digit tree PBS (thfhe_dag_run_tree_batch, thfhe_dag_run_mv_batch) */
    THFHE_MV = 19,      /* gate-DAG node: multi-value bootstrap, q outputs of one rotation (thfhe_dag_run_mv_batch only) */
    THFHE_TREE_MV = 20, /* gate-DAG node: two-digit tree with a multi-value level 1 and k outputs (thfhe_dag_run_mv_batch, thfhe_dag_run_lhe_batch) */
    THFHE_LHE_LOOKUP = 21,  /* gate-DAG node: leveled lookup of a table of the run at a TGSW-encrypted address (thfhe_dag_run_lhe_batch only) */
    THFHE_LHE_GATHER = 22,  /* gate-DAG node: leveled pick among 2^d computed wires at a TGSW-encrypted index (thfhe_dag_run_lhe_batch only) */
    THFHE_LHE_WFA = 23,     /* gate-DAG node: layered automaton on TGSW-encrypted bits (thfhe_dag_run_lhe_batch only) */
    THFHE_CB = 24,          /* gate-DAG node: wires -> a computed TGSW set by circuit bootstrapping (thfhe_dag_run_cb_batch only); in
                               THFHE_CB_ONE_ROTATION mode the operand wires must be gate-encoded (+-1/8): the caller's responsibility */
    THFHE_DENSE = 25        /* gate-DAG node: an encrypted dense layer, M theta outputs from K operand wires (thfhe_dag_run_dense_batch,
                               thfhe_mk_dag_run_dense_batch only) */
};

enum thfhe_error {
    THFHE_OK = 0, THFHE_E_INVALID = -1, THFHE_E_UNSUPPORTED = -2, THFHE_E_NO_DEVICE = -3,
    THFHE_E_HIP = -4, THFHE_E_NOMEM = -5
};

typedef struct thfhe_ctx thfhe_ctx;

const char *thfhe_last_error(void);
int thfhe_device_count(void);
/* PCI bus id ("0000:c1:00.0") of HIP device `device` as this process sees it: bench.py prints it per rank so that a multi-GPU record
 * shows N ranks on N different devices. */
int thfhe_device_pci_bus_id(int device, char *buf, int len);

/* Upload + transform the keys to device `device`.  bk_coeff / ksk are HOST pointers, borrowed only
 * for the duration of the call. */
int thfhe_ctx_create(const thfhe_params *params, const int32_t *bk_coeff, const int32_t *ksk, int device,
                     thfhe_ctx **out);
void thfhe_ctx_destroy(thfhe_ctx *ctx);
int thfhe_ctx_params(const thfhe_ctx *ctx, thfhe_params *out);

/* ---- host-buffer API: the drop-in level.  in0/in1/in2/out are HOST arrays of `count` records.  `out` may alias
 * an input (the reference's callers do, src/KNN_medical_data.cpp:256,395).  Thread-safe per ctx. */
int thfhe_gates(thfhe_ctx *ctx, int op, const int32_t *in0, const int32_t *in1, const int32_t *in2,
                int32_t *out, size_t count);
/* One launch for a level of a gate DAG: gate g applies ops[g] (any two-input bootstrapped gate NAND..ORYN) to
 * (in0[g], in1[g]).  ops is a HOST array of `count` opcodes. */
int thfhe_gates_mixed(thfhe_ctx *ctx, const int32_t *ops, const int32_t *in0, const int32_t *in1, int32_t *out, size_t count);
/* Gate-DAG evaluation: the levelising scheduler + device-resident executor for the reference's circuits (FullAdder / difference /
 * distance / sort_with_distance ..., src/KNN_medical_data.cpp:127-489, issued there as sequential boots* calls).
 *   wires  HOST table int32[n_inputs + n_gates][n+1]: rows [0, n_inputs) hold the input ciphertexts, row n_inputs + g receives gate g
 *   gates  HOST int32[n_gates][4] = (opcode, in0, in1, in2), topological order, operands are earlier wire ids (unused = -1);
 *          opcodes: the two-input bootstrapped gates, THFHE_MUX, THFHE_NOT, THFHE_COPY
 * Gates are scheduled ASAP into levels; each level is ONE blind-rotate launch per gate class (two-input with per-gate opcodes, MUX);
 * the wire table stays in HBM and the host is not synchronised between levels.
 * stats (optional) int64[4] = {levels, bootstrap launches, blind rotations, widest level}. */
int thfhe_dag_run(thfhe_ctx *ctx, int32_t *wires, size_t n_inputs, const int32_t *gates, size_t n_gates, int64_t *stats);
/* `instances` independent evaluations of ONE gate list, level by level: a level's launch holds instances x its gates.  This is the
 * reference's loop over test records around one circuit (`for i < test_row_size`, src/KNN_medical_data.cpp:676-691): the deep, narrow
 * part of a decision (a ripple carry holds 1-3 gates per level) fills the chip only when many records walk it side by side.
 *   inputs     HOST int32[instances][n_inputs][n+1]
 *   out_wires  HOST wire ids to return (n_out of them); NULL: every gate wire, i.e. n_inputs .. n_inputs + n_gates - 1
 *   outputs    HOST int32[instances][n_out (or n_gates)][n+1]
 * Gate outputs are deterministic functions of their operands, so instance q's wires equal thfhe_dag_run on inputs[q] bit for bit. */
int thfhe_dag_run_batch(thfhe_ctx *ctx, const int32_t *inputs, size_t n_inputs, const int32_t *gates, size_t n_gates, size_t instances,
                        const int32_t *out_wires, size_t n_out, int32_t *outputs, int64_t *stats);
/* A level whose instances x gates exceed `max_gates` runs as several launches of at most that many gates (default 28 672 = 14 rounds of the
 * throughput kernel; bounds the staging memory and the launch grid).  1 .. 32 767. */
int thfhe_set_dag_slice(thfhe_ctx *ctx, size_t max_gates);
int thfhe_bootstrap(thfhe_ctx *ctx, int32_t mu, const int32_t *x, int32_t *out, size_t count);
int thfhe_bootstrap_wo_keyswitch(thfhe_ctx *ctx, int32_t mu, const int32_t *x, int32_t *out_N1, size_t count);
int thfhe_keyswitch(thfhe_ctx *ctx, const int32_t *in_N1, int32_t *out, size_t count);

/* ---- programmable bootstrapping (PBS): a lookup table on a small encrypted integer, evaluated during the blind rotation.
 *
 * Integer encoding (padding bit): m in [0, p), p a power of two, is the Torus32 word m * 2^32 / (2p); the phase stays in [0, 1/2) and
 * the negacyclic wrap never inverts a valid input.
 * Prologue: x = w0*in0 + w1*in1 + w2*in2 + (0, ..., 0, bias), word-wise mod 2^32 over the first n_inputs inputs; the bias is added to the
 *   body only.  With w = (p_b, 1) a two-input function f(a, b) is a one-input table on p_b*a + b.
 * Mod-switch with theta outputs (many-LUT), theta in {1, 2, 4}: every word of x is rounded to a multiple of theta in Z_2N,
 *   bar = modswitch_{2N/theta}(word) * theta  (theta = 1: the mod-switch of thfhe_bootstrap, bit for bit).
 * Accumulator: (0, X^{-barb} * tv), tv = the sample's test vector of N Torus32 words; the blind rotation is the one of thfhe_bootstrap
 *   (same CMux chain, same skip of mask words with bara == 0).
 * Extraction: for every j < theta, coefficient j of the accumulator becomes an LWE(N) record: a'_i = a_{j-i} for i <= j,
 *   a'_i = -a_{N+j-i} for i > j, b' = body_j.  thfhe_lut_bootstrap then key-switches the count*theta records.
 * Test-vector layout (built on the host, e.g. thfhe.lut.test_vector): message m occupies the box of N/p coefficients centred on m*N/p;
 *   inside the box entry i holds f_{i mod theta}(m); the lower half-box of m = 0 wraps to the top of tv with its sign negated.
 *   tv = (mu, ..., mu), theta = 1, w = (1), bias = 0 is exactly thfhe_bootstrap(mu).
 * tv: HOST int32[n_luts][N], 1 <= n_luts <= 1024.  lut_index: HOST int32[count] table of each sample, or NULL (every sample uses table 0).
 * in0/in1/in2: HOST records int32[count][n+1] (in1, in2 may be NULL when n_inputs does not name them).
 * out: HOST int32[count][theta][n+1] (thfhe_lut_bootstrap) or int32[count][theta][N+1] (thfhe_lut_bootstrap_wo_keyswitch).
 * Arguments are checked on the host before any device work (THFHE_E_INVALID): null pointers, n_inputs outside 1..3, theta not in
 * {1, 2, 4}, n_luts outside 1..1024, any lut_index entry outside 0..n_luts-1.  count 0 returns THFHE_OK.  Single key, N = 1024. */
typedef struct thfhe_lut_spec {
    int32_t n_inputs;   /* 1..3 */
    int32_t weights[3]; /* integer weights of in0, in1, in2 */
    int32_t bias;       /* Torus32 constant added to the body */
    int32_t theta;      /* outputs per rotation: 1, 2 or 4 */
} thfhe_lut_spec;

int thfhe_lut_bootstrap(thfhe_ctx *ctx, const thfhe_lut_spec *spec, const int32_t *tv, int n_luts, const int32_t *lut_index,
                        const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out, size_t count);
int thfhe_lut_bootstrap_wo_keyswitch(thfhe_ctx *ctx, const thfhe_lut_spec *spec, const int32_t *tv, int n_luts, const int32_t *lut_index,
                                     const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out_N1, size_t count);

/* ---- LUT nodes in the gate-DAG executor: thfhe_dag_run_batch with programmable bootstraps among the gates.
 * nodes: HOST int32[n_nodes][6] = (opcode, in0, in1, in2, spec, lut); row g defines wire n_inputs + g, topological order.
 *   Gate row:  an opcode of thfhe_dag_run_batch, spec = lut = -1.
 *   LUT node:  (THFHE_LUT, in0, in1, in2, spec, lut): specs[spec] gives n_inputs, weights, bias and theta; operands beyond n_inputs are -1;
 *              tv[lut] is the node's test vector.  It is followed by exactly theta - 1 rows (THFHE_LUT_OUT, head, -1, -1, -1, -1), head =
 *              the LUT row's wire id; wire head + j holds output j, the record thfhe_lut_bootstrap(specs[spec], tv[lut], operands) returns
 *              at [0][j], bit for bit (key switch included).
 * specs: HOST thfhe_lut_spec[n_specs], 1 <= n_specs <= 1024; tv: HOST int32[n_luts][N], 1 <= n_luts <= 1024.  Every instance shares them;
 *   they are uploaded once per call.
 * Scheduling: a LUT node costs one level, like a bootstrapped gate; the LUT nodes of a level run as one launch group per theta (the spec and
 *   the table vary per node).  LUT_OUT wires sit on their head's level, so NOT / COPY may read them at once.
 * stats: a LUT node counts one rotation whatever its theta, a LUT_OUT row nothing; launches counts each LUT launch group.
 * inputs / instances / out_wires / outputs / stats: the contract of thfhe_dag_run_batch.
 * Checks, on the host before any device work and before the context is looked at (THFHE_E_INVALID): null pointers, n_specs / n_luts out of
 *   range, an invalid spec (the rules of thfhe_lut_bootstrap), a spec or table index out of range, operands that do not match the spec's
 *   n_inputs, a missing, extra or misplaced LUT_OUT row or one naming the wrong head, spec / lut not -1 on a gate row, operands that are not
 *   earlier wires, opcodes the engine does not define.  thfhe_dag_run(_batch) and thfhe_mk_dag_run(_batch) reject THFHE_LUT and THFHE_LUT_OUT. */
int thfhe_dag_run_lut_batch(thfhe_ctx *ctx, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes, const thfhe_lut_spec *specs,
                            int n_specs, const int32_t *tv, int n_luts, size_t instances, const int32_t *out_wires, size_t n_out, int32_t *outputs,
                            int64_t *stats);

/* ---- device-buffer API: records already resident in HBM (what bench.py times).  Pointers come from
 * thfhe_dev_alloc (or any hipMalloc in this process).  Calls enqueue on the context's stream and
 * return; thfhe_sync waits. */
void *thfhe_dev_alloc(thfhe_ctx *ctx, size_t bytes);
void thfhe_dev_free(thfhe_ctx *ctx, void *p);
int thfhe_copy_h2d(thfhe_ctx *ctx, void *dst, const void *src, size_t bytes);
int thfhe_copy_d2h(thfhe_ctx *ctx, void *dst, const void *src, size_t bytes);
int thfhe_reserve(thfhe_ctx *ctx, size_t max_count); /* pre-size the workspace (no allocation afterwards) */
int thfhe_gates_dev(thfhe_ctx *ctx, int op, const int32_t *d_in0, const int32_t *d_in1, const int32_t *d_in2,
                    int32_t *d_out, size_t count);
int thfhe_sync(thfhe_ctx *ctx);

/* Kernel choice for a batch of rotations (gates; a MUX is two).  Whole rounds of 2 048 rotations (eight per CU of an MI355X) run on the
 * LDS-ring throughput kernel, eight gates per workgroup.  The remainder r runs on the cooperative latency kernel (one workgroup per gate) if
 * r <= the cooperative threshold (default 768), on the four-wave shape of the ring kernel (four gates per workgroup, one wave per SIMD) if
 * r <= the ring4 threshold (default 1 024), on both if r <= ring4 + 256, else on one more eight-wave round.  Both thresholds 0: everything
 * on the eight-wave kernel.  Every shape computes the same words. */
int thfhe_set_coop_threshold(thfhe_ctx *ctx, int max_jobs);
int thfhe_set_ring4_threshold(thfhe_ctx *ctx, int max_jobs);
/* The name of the blind-rotation kernel that a batch of `rotations` runs on under the context's thresholds, as a C string in buf (for
 * profiles and coverage checks; where a batch is cut in pieces, the kernel of its first and largest).  The answer comes from the rule the
 * launcher itself follows (csrc/thfhe_launch_plan.h); no device work.  A buffer shorter than the name is THFHE_E_INVALID; 64 bytes hold
 * every name.  thfhe_mk_ / thfhe_kms_ / thfhe_ccs_rotation_kernel_name answer for the other engines. */
int thfhe_rotation_kernel_name(const thfhe_ctx *ctx, size_t rotations, char *buf, int len);

/* Per-kernel device timing: when enabled, every *_dev call brackets each kernel with HIP events on the
 * context's stream.  After thfhe_sync, thfhe_last_timings returns milliseconds of the most recent call:
 * ms[0] = prologue (linear part + mod-switch), ms[1] = blind rotate, ms[2] = key switch, ms[3] = total. */
int thfhe_set_profiling(thfhe_ctx *ctx, int enabled);
int thfhe_last_timings(thfhe_ctx *ctx, float ms[4]);

/* ---- 3-gen multi-key (Torus64 ring) --------------------------------------------------------------- */
typedef struct thfhe_mk_ctx thfhe_mk_ctx;
/* Ring degrees: N = 1024 (l <= 4, Bgbit <= 10), N = 2048 (l <= 3; bases of 11 .. 27 bit are cut into balanced 9-bit digit parts: the 16 .. 256-party
 * sets of J/mk_api.jl:214-310), N = 4096 (at most six digit rows: the 64-party "for fft" and the 512-party set, J/mk_api.jl:277-283, 316-322).
 * bk_coeff int64[P][n][4][l][N] (part_1 .. part_4 of MKBootstrapKeyPart_3gen), ksk int32[P][N][t][base-1][n+1]. */
int thfhe_mk_ctx_create(const thfhe_params *params, const int64_t *bk_coeff, const int32_t *ksk, int device,
                        thfhe_mk_ctx **out);
void thfhe_mk_ctx_destroy(thfhe_mk_ctx *ctx);
int thfhe_mk_gates(thfhe_mk_ctx *ctx, int op, const int32_t *in0, const int32_t *in1, const int32_t *in2,
                   int32_t *out, size_t count);
/* one launch for a DAG level of two-input 3-gen gates (NAND / OR / AND / XOR), per-gate opcodes in the HOST array ops */
int thfhe_mk_gates_mixed(thfhe_mk_ctx *ctx, const int32_t *ops, const int32_t *in0, const int32_t *in1, int32_t *out, size_t count);
/* Batches of at most `max_single_jobs` rotations run one gate per workgroup (latency), larger ones two gates per workgroup sharing
 * every key chunk (throughput; l <= 3 on the ring of degree 1024, every set on the ring of degree 2048).  Default 256 = one workgroup per CU of an MI355X. */
int thfhe_mk_set_pair_threshold(thfhe_mk_ctx *ctx, long max_single_jobs);
int thfhe_mk_rotation_kernel_name(const thfhe_mk_ctx *ctx, size_t rotations, char *buf, int len);   /* see thfhe_rotation_kernel_name */
/* Gate-DAG evaluation for the 3-gen scheme (same contract as thfhe_dag_run; records of P*n+1 words): the reference's multi-key integer
 * circuits mk_add_3gen ... mk_int_mul_3gen (J/3gen_mk_gates.jl:183-362).  Opcodes: NAND / OR / AND / XOR, AND3, MUX, NOT, COPY. */
int thfhe_mk_dag_run(thfhe_mk_ctx *ctx, int32_t *wires, size_t n_inputs, const int32_t *gates, size_t n_gates, int64_t *stats);
/* `instances` evaluations of one 3-gen gate list side by side (same contract as thfhe_dag_run_batch; records of P*n+1 words) */
int thfhe_mk_dag_run_batch(thfhe_mk_ctx *ctx, const int32_t *inputs, size_t n_inputs, const int32_t *gates, size_t n_gates, size_t instances,
                           const int32_t *out_wires, size_t n_out, int32_t *outputs, int64_t *stats);
int thfhe_mk_set_dag_slice(thfhe_mk_ctx *ctx, size_t max_gates); /* default 8 192 */
int thfhe_mk_bootstrap(thfhe_mk_ctx *ctx, int64_t mu, const int32_t *x, int32_t *out, size_t count);
/* Multi-key programmable bootstrap: the contract of thfhe_lut_bootstrap on the 3-gen scheme, every parameter family.
 * in0/in1/in2: HOST records int32[count][P*n+1] (padding-bit encoding m * 2^32 / (2p)).  The prologue and the theta-rounded mod-switch
 *   run over all P*n+1 words; the CMux chain is mk_bootstrap_3gen's (party-major, mask words with bara == 0 skipped).
 * tv: HOST int64[n_luts][N] Torus64 test vectors (N = the context's ring degree; layout of thfhe_lut_bootstrap, e.g.
 *   thfhe.lut.test_vector(..., torus_bits=64)).  Accumulator (0, X^{-barb} * tv[lut_index[s]]); record j < theta of sample s is
 *   coefficient j extracted with t64tot32: a'_i = t64tot32(a_{j-i}) (i <= j), t64tot32(-a_{N+j-i}) (i > j), b' = t64tot32(body_j).
 *   tv = (mu, ..., mu), theta = 1, w = (1), bias = 0 is exactly thfhe_mk_bootstrap(mu).
 * out: HOST int32[count][theta][P*n+1] (key-switched) or int32[count][theta][N+1] (_wo_keyswitch).
 * Argument checks as thfhe_lut_bootstrap, on the host before any device work and before the context is looked at. */
int thfhe_mk_lut_bootstrap(thfhe_mk_ctx *ctx, const thfhe_lut_spec *spec, const int64_t *tv, int n_luts, const int32_t *lut_index,
                           const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out, size_t count);
int thfhe_mk_lut_bootstrap_wo_keyswitch(thfhe_mk_ctx *ctx, const thfhe_lut_spec *spec, const int64_t *tv, int n_luts, const int32_t *lut_index,
                                        const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out_N1, size_t count);
/* LUT nodes in the 3-gen gate-DAG executor: the contract of thfhe_dag_run_lut_batch with the gate opcodes of thfhe_mk_dag_run_batch, records of
 * P*n+1 words and Torus64 tables tv: HOST int64[n_luts][N] (N = the context's ring degree).  A LUT node equals thfhe_mk_lut_bootstrap bit for bit. */
int thfhe_mk_dag_run_lut_batch(thfhe_mk_ctx *ctx, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes,
                               const thfhe_lut_spec *specs, int n_specs, const int64_t *tv, int n_luts, size_t instances, const int32_t *out_wires,
                               size_t n_out, int32_t *outputs, int64_t *stats);
/* Party-sharded building blocks (optional mode: a rank holds only the keys of a contiguous block of m
 * parties, i.e. a context created with parties = m from those parties' key parts; m = 1 is one rank per party).  Below
 * nb = m * n (the block's mask words) and P = the key set's total party count.  All pointers are DEVICE pointers; calls enqueue
 * on the context's stream.  The accumulator travels between ranks as int64[count][2][N] (mask polynomial, body polynomial).
 *   prologue       : the gate's linear part (J/3gen_mk_gates.jl; op = -1: identity, i.e. plain mk_bootstrap_3gen of in0; which = 0 / 1
 *                    selects the first / second AND of the 3-gen MUX) + mod-switch (J/numeric-functions.jl:70-73) of this block's nb
 *                    mask words [first_word, first_word + nb) of records with rec_words = P*n + 1 words, and of b.
 *   rotate_partial : run this context's nb CMuxes (J/3gen_mk_internals.jl:66-84, party-major) on every accumulator.  d_bara =
 *                    int32[count][nb] mod-switched mask words of this block; d_acc_in == NULL starts from X^{-barb} * mu (first block).
 *   extract        : rlwe_extract_sample_64 (J/rlwe.jl:70-74) -> int32[count][N+1]
 *   keyswitch      : keyswitch of the extracted samples with this context's key(s) -> int32[count][nb+1]      */
int thfhe_mk_prologue_dev(thfhe_mk_ctx *ctx, int op, int which, const int32_t *d_in0, const int32_t *d_in1, const int32_t *d_in2,
                          int rec_words, int first_word, int32_t *d_bara, int32_t *d_barb, size_t count);
int thfhe_mk_rotate_partial_dev(thfhe_mk_ctx *ctx, const int32_t *d_bara, const int32_t *d_barb, int64_t mu,
                                const int64_t *d_acc_in, int64_t *d_acc_out, size_t count);
int thfhe_mk_extract_dev(thfhe_mk_ctx *ctx, const int64_t *d_acc, int32_t *d_u, size_t count);
int thfhe_mk_keyswitch_dev(thfhe_mk_ctx *ctx, const int32_t *d_u, int32_t *d_out, size_t count);
/* Enqueue every later call on the caller's HIP stream (e.g. the stream the caller's RCCL communicator synchronises with);
 * NULL returns to the context's own stream.  Waits for work already enqueued. */
int thfhe_mk_set_stream(thfhe_mk_ctx *ctx, void *hip_stream);
void *thfhe_mk_dev_alloc(thfhe_mk_ctx *ctx, size_t bytes);
void thfhe_mk_dev_free(thfhe_mk_ctx *ctx, void *p);
int thfhe_mk_copy_h2d(thfhe_mk_ctx *ctx, void *dst, const void *src, size_t bytes);
int thfhe_mk_copy_d2h(thfhe_mk_ctx *ctx, void *dst, const void *src, size_t bytes);
int thfhe_mk_reserve(thfhe_mk_ctx *ctx, size_t max_count);
int thfhe_mk_gates_dev(thfhe_mk_ctx *ctx, int op, const int32_t *d_in0, const int32_t *d_in1,
                       const int32_t *d_in2, int32_t *d_out, size_t count);
int thfhe_mk_sync(thfhe_mk_ctx *ctx);
int thfhe_mk_set_profiling(thfhe_mk_ctx *ctx, int enabled);
int thfhe_mk_last_timings(thfhe_mk_ctx *ctx, float ms[4]);

/* ---- CCS multi-key scheme: the reference's `mk_bootstrap` / `mk_gate_nand` ---------------------------------
 *   thfhe_ccs_gates      <- mk_gate_nand(ck, x, y)            J/mk_gates.jl:7-13 (AND / OR / XOR share the bootstrap with their own linear part)
 *   thfhe_ccs_bootstrap  <- mk_bootstrap(bk, ks, mu, x)       J/mk_internals.jl:855-858 (UniProduct_old :477-536, mk_keyswitch :714-728)
 *   thfhe_ccs_ctx_create <- MKBootstrapKey(parts, shared_key) J/mk_internals.jl:778-802 (forward_transform of every key polynomial)
 * Torus32, N = 1024, k = 1.  HOST tables, coefficient domain:
 *   bk  int32[P][n][3][l][N]   d1, f0, f1 of every MKTGswUESample (J/mk_internals.jl:338-448)
 *   pk  int32[P][l][N]         PublicKey.b;    crs int32[l][N]  SharedKey.a;    ksk int32[P][N][t][base-1][n+1]
 * Records: int32[P*n+1] = a[p*n + i], b (MKLweSample). */
typedef struct thfhe_ccs_ctx thfhe_ccs_ctx;
int thfhe_ccs_ctx_create(const thfhe_params *params, const int32_t *bk, const int32_t *pk, const int32_t *crs, const int32_t *ksk, int device,
                         thfhe_ccs_ctx **out);
void thfhe_ccs_ctx_destroy(thfhe_ccs_ctx *ctx);
int thfhe_ccs_gates(thfhe_ccs_ctx *ctx, int op, const int32_t *in0, const int32_t *in1, int32_t *out, size_t count);
int thfhe_ccs_bootstrap(thfhe_ccs_ctx *ctx, int32_t mu, const int32_t *x, int32_t *out, size_t count);
/* the context's blind-rotation kernel (more than 8 parties or 8 levels take the wide one); see thfhe_rotation_kernel_name */
int thfhe_ccs_rotation_kernel_name(const thfhe_ccs_ctx *ctx, char *buf, int len);

/* ---- LWE -> TLWE conversion and threshold partial / final decryption: the step after the gate path in the reference's C++
 * applications.  k = 1, N = 1024; all pointers are HOST arrays.
 *   thfhe_tlwe_from_lwe     <- TLweFromLwe(ring_cipher, cipher, tlwe_params)       src/libthfhe.cpp:340-348, src/KNN_medical_data.cpp:492-500
 *                              lwe int32[count][N+1] -> tlwe_a int32[count][N] (a'[0] = a[0], a'[i] = -a[N-i]), tlwe_b int32[count][N] (b'[0] = b)
 *   thfhe_partial_decrypt   <- ThFHEKeyShare::PartialDecrypt / partialDecrypt       src/libthfhe.cpp:270-293, src/threshold_decryption_functions.cpp:441-480
 *                              partial[c] = key_share (*) tlwe_a[c] + noise[c]; (*) exact negacyclic product mod 2^32 (torusPolynomialAddMulR);
 *                              key_share int32[N] with |s| <= 512; noise (the caller's smudging Gaussian) may be NULL
 *   thfhe_final_decrypt     <- finalDecrypt                                          src/libthfhe.cpp:296-315
 *                              result[c] = tlwe_b[c] - partials[0][c] + sum_{i>=1} partials[i][c]; bits[c] = result[c][0] > 0; result may be NULL
 *   thfhe_pack_key_set      the LWE -> TLWE packing key (the reference's TODO at src/Convert.cpp:103):
 *                              pk int32[n][t][2^basebit - 1][2][N], row (j, p, v) a TLWE sample (alpha, beta) under the ring key z with
 *                              beta = alpha (*) z + e + v s_j 2^(32 - (p+1) basebit) on the constant coefficient.  Uploads it (with the
 *                              matrix-core planes for basebit 2, t = 4 or 8) and replaces any earlier key.  THFHE_E_INVALID for n < 1, t < 1
 *                              or t basebit > 32; THFHE_E_UNSUPPORTED for basebit > 4 or n > 2048; an allocation failure leaves no key set
 *   thfhe_pack_lwe          lwe int32[count][n+1] -> tlwe_a, tlwe_b int32[ceil(count / slots)][N]: sample g slots + i is key-switched
 *                              with its LWE key switch's digits into T = (0, b X^0) - sum PK[j][p][digit - 1] and lands at X^i:
 *                              output g = sum_i X^i T_{g slots + i} mod X^N + 1.  Coefficient i of its phase (b - a (*) z) is sample i's
 *                              phase plus rounding and key noise; the output feeds thfhe_partial_decrypt / thfhe_final_decrypt unchanged.
 *                              THFHE_E_INVALID without a key or for slots outside 1 .. N.  Bit-exact: integer sums mod 2^32 */
typedef struct thfhe_poly_ctx thfhe_poly_ctx;
int thfhe_poly_ctx_create(int device, int N, thfhe_poly_ctx **out);
void thfhe_poly_ctx_destroy(thfhe_poly_ctx *ctx);
int thfhe_tlwe_from_lwe(thfhe_poly_ctx *ctx, const int32_t *lwe, int32_t *tlwe_a, int32_t *tlwe_b, size_t count);
int thfhe_partial_decrypt(thfhe_poly_ctx *ctx, const int32_t *key_share, const int32_t *tlwe_a, const int32_t *noise, int32_t *partial, size_t count);
int thfhe_final_decrypt(thfhe_poly_ctx *ctx, const int32_t *tlwe_b, const int32_t *partials /*[t][count][N]*/, int t, int32_t *result, int32_t *bits,
                        size_t count);
int thfhe_pack_key_set(thfhe_poly_ctx *ctx, const int32_t *pk, int n, int t, int basebit);
int thfhe_pack_lwe(thfhe_poly_ctx *ctx, const int32_t *lwe /*[count][n+1]*/, size_t count, int slots, int32_t *tlwe_a, int32_t *tlwe_b /*[ceil(count/slots)][N]*/);

/* ---- encrypted lookup tables and two-digit tree PBS (single key, N = 1024, k = 1).  Phase convention everywhere: beta - alpha (*) z.
 *
 * thfhe_lut_bootstrap_enc(_wo_keyswitch): the contract of thfhe_lut_bootstrap(_wo_keyswitch) with ENCRYPTED tables.  Table t is a TLWE sample
 *   (tv_a[t], tv_b[t]) under the context's bootstrapping ring key, whose phase is a test vector in the layout of thfhe_lut_bootstrap (e.g.
 *   thfhe.lut.encrypt_table, or an output of thfhe_pack_boxes).  tv_a, tv_b: HOST int32[n_luts][N], 1 <= n_luts <= 262 144 (every sample may bring
 *   its own table).  Accumulator (X^{-barb} * tv_a[t], X^{-barb} * tv_b[t]), t = lut_index[s], or table 0 when lut_index is NULL.  Prologue, theta in
 *   {1, 2, 4}, the theta-rounded mod-switch, the skip of mask words with bara == 0, extraction at coefficients 0 .. theta-1, the key switch, the
 *   output shapes and the argument checks (on the host, before the context is looked at) are those of thfhe_lut_bootstrap.  tv_a = 0, tv_b = tv gives
 *   the words of thfhe_lut_bootstrap(tv).  The table's noise adds to the output's.
 *
 * thfhe_pack_boxes: p LWE samples -> ONE encrypted test vector.  lwe: HOST int32[count][n+1] (n = the packing key's dimension), p a power of two,
 *   2 <= p <= N/2, count a multiple of p -> tlwe_a, tlwe_b HOST int32[count / p][N].  With T_i the per-sample key-switch result of thfhe_pack_lwe,
 *   output g = U(X) * sum_{i < p} X^(i N/p) T_(g p + i) mod X^N + 1 on both polynomials, U(X) = X^(-N/(2p)) (1 + X + ... + X^(N/p - 1)): candidate i
 *   fills the N/p coefficients centred on i N/p, the lower half-box of candidate 0 wraps to the top negated -- the layout of thfhe.lut.test_vector at
 *   theta = 1.  Noiseless trivial inputs (a = 0, b = v_i) under an all-zero key give exactly (0, test_vector(v, p)).  Bit-exact: integer sums mod 2^32.
 *   THFHE_E_INVALID without a key, for a bad p, or a count that is not a multiple of p.
 *
 * thfhe_tree_lut_bootstrap: out[s] = f_table[s](hi, lo) for two encrypted digits, as level-1 many-LUT rotations on `lo`, box packing, and one
 *   rotation of the packed (encrypted) table on `hi`; nothing between the stages visits the host.
 *   spec_lo: 1 .. 3 weighted inputs lo0..2, theta1 in {1, 2, 4}.  spec_hi: inputs hi0..2, theta must be 1.  p_hi: a power of two, 2 <= p_hi <= N/2,
 *   theta1 | p_hi; R = p_hi / theta1.  tv1: HOST int32[n_tables][R][N], row r = the many-LUT test vector of f(r theta1 + j, .), j < theta1 (e.g.
 *   thfhe.lut.tree_test_vectors); 1 <= n_tables, n_tables R <= 262 144.  table_index: HOST int32[count] or NULL (table 0).  lo*, hi*: HOST records
 *   int32[count][n+1]; out: HOST int32[count][n+1], which must not alias an input.
 *   The result equals, word for word, thfhe_lut_bootstrap(spec_lo, tv1 rows, lut_index = table R + r) on every sample's inputs repeated R times ->
 *   thfhe_pack_boxes(p = p_hi) -> thfhe_lut_bootstrap_enc(spec_hi, table s for sample s).
 *   ctx_pack must hold a packing key (thfhe_pack_key_set) from the gate key set's LWE key to its BOOTSTRAPPING RING key -- the key the encrypted
 *   table must be under for the second rotation (thfhe.keygen.gen_pack_key(rng, K.lwe_key, K.rlwe_key, t, basebit, sigma_bk)).  The library cannot
 *   check which ring key a packing key targets: with any other key the call succeeds and the results do not decrypt.
 *   THFHE_E_INVALID, before any device work: null pointers, an invalid spec, spec_hi theta != 1, a bad p_hi, theta1 not dividing p_hi, n_tables or a
 *   table_index entry out of range (these on the host, before the contexts are looked at); then the two contexts on different devices, no packing
 *   key, a packing key whose n differs from the gate context's.
 *   The batch runs in slices of at most max_candidates / p_hi samples (thfhe_set_tree_slice, default 65 536 candidates, 1 .. 2^20): the packing
 *   scratch is 8 KiB per candidate.  All work of a call is enqueued on the gate context's stream while both contexts are locked; the packing
 *   context's own stream is drained first.  With profiling on, thfhe_last_timings gives ms[0] = level 1, ms[1] = packing, ms[2] = level 2 of the
 *   LAST slice and ms[3] = the whole call. */
int thfhe_lut_bootstrap_enc(thfhe_ctx *ctx, const thfhe_lut_spec *spec, const int32_t *tv_a, const int32_t *tv_b, int n_luts, const int32_t *lut_index,
                            const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out, size_t count);
int thfhe_lut_bootstrap_enc_wo_keyswitch(thfhe_ctx *ctx, const thfhe_lut_spec *spec, const int32_t *tv_a, const int32_t *tv_b, int n_luts,
                                         const int32_t *lut_index, const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out_N1,
                                         size_t count);
int thfhe_pack_boxes(thfhe_poly_ctx *ctx, const int32_t *lwe /*[count][n+1]*/, size_t count, int p, int32_t *tlwe_a, int32_t *tlwe_b /*[count/p][N]*/);
int thfhe_tree_lut_bootstrap(thfhe_ctx *ctx, thfhe_poly_ctx *ctx_pack, const thfhe_lut_spec *spec_lo, const thfhe_lut_spec *spec_hi, int p_hi,
                             const int32_t *tv1, int n_tables, const int32_t *table_index, const int32_t *lo0, const int32_t *lo1, const int32_t *lo2,
                             const int32_t *hi0, const int32_t *hi1, const int32_t *hi2, int32_t *out, size_t count);
int thfhe_set_tree_slice(thfhe_ctx *ctx, size_t max_candidates);

/* ---- multi-value bootstrapping with factored test vectors (single key, N = 1024): q functions of one encrypted digit from ONE
 * blind rotation, whatever q is (Carpov - Izabachene - Mollimard; Guimaraes - Borin - Aranha).
 *
 * thfhe_mv_lut_bootstrap(_wo_keyswitch): spec must have theta 1; prologue, mod-switch, CMux chain and the skip of mask words with bara == 0 are
 *   those of thfhe_lut_bootstrap at theta = 1.  tv0: HOST int32[N], any words: the accumulator starts at (0, X^{-barb} * tv0).
 *   factors: HOST int32[n_tables][q][p], p a power of two, 2 <= p <= 64, 1 <= q <= 64, 1 <= n_tables <= 1024.  table_index: HOST int32[count], or
 *   NULL (table 0).  With box = N/p and F_{t,j}(X) = sum_{k<p} factors[t][j][k] X^(box/2 + k box), output (s, j) is the extraction at coefficient 0
 *   of ACC_s * F_{t,j} mod (X^N + 1, 2^32), t = table_index[s]: word-wise, - sum_k factors[t][j][k] * extract_at(ACC_s, N - box/2 - k box), an exact
 *   integer combination of p extractions.  With tv0 = (u, ..., u), step = 2u, and factors c_k = f(k+1) - f(k) (k < p-1), c_{p-1} = -(f(0) + f(p-1))
 *   (thfhe.lut.mv_base / mv_factors) tv0 * F is the test vector of the words f(m) * step: output j carries f_j(m) * step.  The rotation's noise
 *   reaches output j multiplied by the 2-norm of its factor.
 *   out: HOST int32[count][q][n+1] (thfhe_mv_lut_bootstrap) or int32[count][q][N+1] (_wo_keyswitch).
 *   THFHE_E_INVALID on the host, before the context is looked at: the checks of thfhe_lut_bootstrap (tv0 and n_tables in the places of tv and
 *   n_luts), a null factors, theta != 1, a bad p, q or n_tables, a table_index entry out of range.  count 0 returns THFHE_OK.  The batch runs in
 *   slices of at most max_candidates (thfhe_set_tree_slice) output records, 4.1 KiB of workspace each.
 *
 * thfhe_tree_lut_bootstrap_mv: thfhe_tree_lut_bootstrap with level 1 replaced by one multi-value rotation per sample on `lo` (p = p_lo taps,
 *   q = p_hi outputs: candidate h of sample s is output h), then the key switch of the count p_hi candidates, the box packing and the selection
 *   rotation on `hi` as there: 1 + 1 rotations per sample.  factors: HOST int32[n_tables][p_hi][p_lo] (thfhe.lut.tree_mv_factors).  The result
 *   equals, word for word, thfhe_mv_lut_bootstrap(spec_lo, q = p_hi) -> thfhe_pack_boxes(p = p_hi) -> thfhe_lut_bootstrap_enc(spec_hi, table s for
 *   sample s).  Checks, contexts, locking, stream, slicing and timings are those of thfhe_tree_lut_bootstrap, plus the checks above (spec_lo theta
 *   1, p_lo as p, p_hi as q: 2 .. 64).
 *
 * thfhe_tree_lut_bootstrap_mvk: thfhe_tree_lut_bootstrap_mv with k tables per sample, out[s][j] = f_{t,j}(hi_s, lo_s) for j < k, in
 *   1 + k rotations per sample; nothing between the stages visits the host.  factors: HOST int32[n_tables][k][p_hi][p_lo] (thfhe.lut.tree_mvk_factors);
 *   out: HOST int32[count][k][n+1].  p_lo and p_hi powers of two in 2 .. 64, 1 <= k, k p_hi <= 64 (the multi-value rotation's q limit), 1 <= n_tables
 *   <= 1024, both specs' theta 1.  Per slice: one multi-value rotation per sample on `lo` with q = k p_hi outputs, output j p_hi + h = candidate h of
 *   table j; the key switch of the S k p_hi candidates; the box packing (p = p_hi) into S k encrypted tables -- the candidate order makes table (s, j)
 *   the packed sample s k + j; S k selection rotations, job s k + j on sample s's `hi` operands and its own table s k + j; the key switch into out.
 *   The result equals, word for word, thfhe_mv_lut_bootstrap(spec_lo, q = k p_hi) -> thfhe_pack_boxes(p = p_hi) -> thfhe_lut_bootstrap_enc(spec_hi,
 *   ...) with each sample's `hi` operands repeated k times and lut_index = 0 .. count k - 1; at k = 1 it equals thfhe_tree_lut_bootstrap_mv word for
 *   word.  Host checks, before either context is looked at: those of thfhe_tree_lut_bootstrap_mv, then k and k p_hi; then the context checks of
 *   thfhe_tree_lut_bootstrap; count 0 returns THFHE_OK once those have passed (with a NULL context it is THFHE_E_INVALID, as in the older tree entries).  A
 *   slice is at most max(1, max_candidates / (k p_hi)) samples (thfhe_set_tree_slice).  Contexts, locking, the single stream, the drain of the packing
 *   context's stream and the timing slots are those of thfhe_tree_lut_bootstrap. */
int thfhe_mv_lut_bootstrap(thfhe_ctx *ctx, const thfhe_lut_spec *spec, const int32_t *tv0, const int32_t *factors /*[n_tables][q][p]*/, int p, int q,
                           int n_tables, const int32_t *table_index, const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out,
                           size_t count);
int thfhe_mv_lut_bootstrap_wo_keyswitch(thfhe_ctx *ctx, const thfhe_lut_spec *spec, const int32_t *tv0, const int32_t *factors /*[n_tables][q][p]*/,
                                        int p, int q, int n_tables, const int32_t *table_index, const int32_t *in0, const int32_t *in1,
                                        const int32_t *in2, int32_t *out_N1, size_t count);
int thfhe_tree_lut_bootstrap_mv(thfhe_ctx *ctx, thfhe_poly_ctx *ctx_pack, const thfhe_lut_spec *spec_lo, const thfhe_lut_spec *spec_hi, int p_hi,
                                int p_lo, const int32_t *tv0, const int32_t *factors /*[n_tables][p_hi][p_lo]*/, int n_tables,
                                const int32_t *table_index, const int32_t *lo0, const int32_t *lo1, const int32_t *lo2, const int32_t *hi0,
                                const int32_t *hi1, const int32_t *hi2, int32_t *out, size_t count);
int thfhe_tree_lut_bootstrap_mvk(thfhe_ctx *ctx, thfhe_poly_ctx *ctx_pack, const thfhe_lut_spec *spec_lo, const thfhe_lut_spec *spec_hi, int p_hi,
                                 int p_lo, int k, const int32_t *tv0, const int32_t *factors /*[n_tables][k][p_hi][p_lo]*/, int n_tables,
                                 const int32_t *table_index, const int32_t *lo0, const int32_t *lo1, const int32_t *lo2, const int32_t *hi0,
                                 const int32_t *hi1, const int32_t *hi2, int32_t *out /*[count][k][n+1]*/, size_t count);

/* ---- leveled table lookup on TGSW-encrypted address bits (single key, N = 1024): the external product TGSW (.) TLWE on user data.
 * With the d address bits of a sample encrypted as TGSW samples under the ring key, a 2^d-entry table costs d CMuxes instead of a blind rotation.
 *
 * thfhe_tgsw_set_create: tgsw: HOST int32[count][d][2l][2][N], the layout of the bootstrapping key (thfhe.keygen.SecretKeySet.tgsw_encrypt): row
 *   (j, level) of a sample is a TLWE encryption of zero plus bit * 2^(32 - (level+1) Bgbit) on coefficient 0 of polynomial j.  The samples are
 *   uploaded in slices, transformed on the device and kept as spectra, count d 2l 32 KiB; that size is checked against the free device memory
 *   before anything is allocated (THFHE_E_NOMEM), and a failed create leaves nothing behind.  1 <= d <= 16, 1 <= count <= 2^24.  The set belongs to
 *   ctx: destroy it before the context.  thfhe_tgsw_set_destroy(NULL) is a no-op.
 *
 * thfhe_lhe_cmux: out[s] = d0[s] + C_(s,bit) (.) (d1[s] - d0[s]) for the samples s = 0 .. count-1 of the set: d1 where the bit is 1, d0 where it is
 *   0.  d1_a, d1_b, d0_a, d0_b, out_a, out_b: HOST int32[count][N] (masks, bodies of TLWE samples under the ring key, phase b - a (*) z).  Exact
 *   integers: every word equals the reference's decomposition and product.
 *
 * thfhe_lhe_lookup(_wo_keyswitch): samples first .. first+count-1 of the set; d_tree + d_rot must equal the set's d, 0 <= d_tree <= 6,
 *   0 <= d_rot <= 10, box = N >> d_rot, theta in {1, 2, 4} and theta <= box.  Address bits 0 .. d_rot-1 are the low bits, bits d_rot .. d-1 pick the
 *   polynomial.  tab_b: HOST int32[n_tables][2^d_tree][N]; tab_a: the masks, or NULL for a public table (trivial samples (0, tab_b)); n_tables
 *   2^d_tree <= 262144.  table_index: HOST int32[count] or NULL (table 0).  Entry e of function j of a table sits at coefficient e * box + j of
 *   polynomial e >> d_rot (thfhe.lut.lhe_table).  Per sample: a CMux tree over the 2^d_tree polynomials, level t pairing neighbours on bit d_rot + t;
 *   then for i = 0 .. d_rot-1  ACC += C_(s,i) (.) (X^(2N - box 2^i) ACC - ACC); then the extraction of coefficients 0 .. theta-1.
 *   out: HOST int32[count][theta][n+1] (key-switched) or int32[count][theta][N+1] (_wo_keyswitch).  The batch runs in slices of at most
 *   max_candidates / 2^(d_tree-1) samples (thfhe_set_tree_slice; the tree workspace is 2^(d_tree-1) TLWE samples per sample) and 65 535 samples.
 *
 * All checks run on the host before the context is looked at (THFHE_E_INVALID): null pointers, the ranges above, a table_index entry out of range,
 * samples outside the set; then a NULL context or a set of another context.  count 0 returns THFHE_OK once those have passed. */
typedef struct thfhe_tgsw_set thfhe_tgsw_set;
int thfhe_tgsw_set_create(thfhe_ctx *ctx, const int32_t *tgsw /*[count][d][2l][2][N]*/, size_t count, int d, thfhe_tgsw_set **out);
void thfhe_tgsw_set_destroy(thfhe_tgsw_set *set);
int thfhe_lhe_cmux(thfhe_ctx *ctx, const thfhe_tgsw_set *set, int bit, const int32_t *d1_a, const int32_t *d1_b, const int32_t *d0_a,
                   const int32_t *d0_b /*[count][N]*/, int32_t *out_a, int32_t *out_b, size_t count);
int thfhe_lhe_lookup(thfhe_ctx *ctx, const thfhe_tgsw_set *set, size_t first, size_t count, int d_tree, int d_rot, int theta, const int32_t *tab_a,
                     const int32_t *tab_b /*[n_tables][2^d_tree][N]*/, int n_tables, const int32_t *table_index, int32_t *out);
int thfhe_lhe_lookup_wo_keyswitch(thfhe_ctx *ctx, const thfhe_tgsw_set *set, size_t first, size_t count, int d_tree, int d_rot, int theta,
                                  const int32_t *tab_a, const int32_t *tab_b /*[n_tables][2^d_tree][N]*/, int n_tables, const int32_t *table_index,
                                  int32_t *out_N1);

/* ---- layered automata on TGSW-encrypted bits (single key, N = 1024): one CMux per state and input bit, whatever the number of bits.
 * A deterministic automaton (or a layered decision diagram) of n_states <= 64 states reads n_steps <= 4096 encrypted bits; its final weights are
 * TLWE samples.  Noise grows as sqrt(steps) sigma_1, so comparisons, equality and threshold tests of wide numbers and pattern matches over some
 * hundred bits need no bootstrap.
 *
 * thfhe_lhe_wfa(_wo_keyswitch): sets: HOST array of n_sets (1 .. 64) sets of ONE context and ONE count (thfhe_tgsw_set_create; each holds at most 16
 *   bits per sample, the array is what reaches past 16); the samples first .. first+count-1 of every set are read.
 *   trans: HOST int32[n_steps][n_states][2], entries in 0 .. n_states-1: trans[j][q][b] is the state that q moves to when the bit of step j is b.
 *   step_bit: HOST int32[n_steps]: step j reads bit (step_bit[j] & 15) of set (step_bit[j] >> 4); any order, any bit more than once.
 *   fin_b: HOST int32[n_tables][n_states][N], the final weight of every state (thfhe.lut.wfa_finals); fin_a: their masks, or NULL for trivial
 *   samples (0, fin_b); n_tables n_states <= 262144; table_index: HOST int32[count] or NULL (table 0).  start: HOST int32[n_out], 1 <= n_out <= 64.
 *   Per sample s, with V_(n_steps)[q] = final weight q of its table, for j = n_steps-1 .. 0:
 *       V_j[q] = V_(j+1)[t0] + C_(s, step_bit[j]) (.) (V_(j+1)[t1] - V_(j+1)[t0]),   (t0, t1) = trans[j][q]
 *   -- thfhe_lhe_cmux's d0 + C (.) (d1 - d0), the same decomposition, words and transforms; where t0 == t1 the state is copied: no product, no noise.
 *   Output (s, o, j) is the extraction of V_0[start[o]] at coefficient j < theta, theta in {1, 2, 4}.  Exact integers, as thfhe_lhe_cmux.
 *   out: HOST int32[count][n_out][theta][n+1] (key-switched) or int32[count][n_out][theta][N+1] (_wo_keyswitch).
 *   One kernel launch per step; the batch runs in slices of at most max(1, max_candidates / (2 n_states)) samples (thfhe_set_tree_slice: two layers
 *   of n_states TLWE samples per sample), at most max(1, max_candidates / (n_out theta)) samples (the output records of a slice) and 65 535 samples.
 *   THFHE_E_INVALID, in this order: on the host, before any set or context is looked at, null pointers, the limits above, a trans, start or
 *   table_index entry out of range; then a null set, a step_bit naming a set >= n_sets or a bit >= that set's d, sets of differing count or
 *   context, samples outside the sets; then a NULL context or a set of another context.  count 0 returns THFHE_OK once those have passed.
 *
 * thfhe_set_wfa_chunk: states per workgroup of a step, 1 .. 64, or 0 (the default): the largest number for which the launch still gives every
 *   compute unit a workgroup.  A workgroup loads the spectra of its sample's bit once for all its states (l <= 3; at l = 4 per state, from the
 *   lines it has just read).  No output word depends on it. */
int thfhe_lhe_wfa(thfhe_ctx *ctx, const thfhe_tgsw_set *const *sets, int n_sets, size_t first, size_t count, int n_steps, int n_states,
                  const int32_t *trans /*[n_steps][n_states][2]*/, const int32_t *step_bit /*[n_steps]*/, const int32_t *fin_a,
                  const int32_t *fin_b /*[n_tables][n_states][N]*/, int n_tables, const int32_t *table_index, int theta, const int32_t *start /*[n_out]*/,
                  int n_out, int32_t *out);
int thfhe_lhe_wfa_wo_keyswitch(thfhe_ctx *ctx, const thfhe_tgsw_set *const *sets, int n_sets, size_t first, size_t count, int n_steps, int n_states,
                               const int32_t *trans, const int32_t *step_bit, const int32_t *fin_a, const int32_t *fin_b, int n_tables,
                               const int32_t *table_index, int theta, const int32_t *start, int n_out, int32_t *out_N1);
int thfhe_set_wfa_chunk(thfhe_ctx *ctx, int g);

/* ---- leveled scatter: demux trees that write at TGSW-encrypted addresses (single key, N = 1024): the other half of the leveled
 * memory.  thfhe_lhe_lookup reads a table at an encrypted address; thfhe_lhe_scatter adds values into tables at encrypted addresses (scatter-add,
 * histograms, one-hot encodings) and returns the tables as TLWE samples in the layout thfhe_lhe_lookup reads (tab_a non-NULL), so a write and a read
 * compose with nothing in between.  A TGSW sample is used once; nothing is bootstrapped.
 *
 * thfhe_lhe_demux: for the samples s = 0 .. count-1 of the set, out1[s] = C_(s,bit) (.) x[s] -- thfhe_lhe_cmux with d0 = 0 and d1 = x, the same
 *   decomposition, words and transforms -- and out0[s] = x[s] - out1[s] word-wise mod 2^32: out1 carries x where the bit is 1, out0 where it is 0, the
 *   other child encrypts zero.  x_a, x_b, out0_a, out0_b, out1_a, out1_b: HOST int32[count][N]; x_a NULL: the trivial samples (0, x_b).
 *
 * thfhe_lhe_scatter: samples first .. first+count-1 of the set; d_tree + d_rot must equal the set's d, 0 <= d_tree <= 6, 0 <= d_rot <= 10,
 *   box = N >> d_rot.  val_b: HOST int32[n_vals][N], val_a: the masks, or NULL for trivial samples (0, val_b); 1 <= n_vals <= 2^24.  Sample s writes the
 *   value val_index[s] (HOST int32[count]); with val_index NULL it writes value s when n_vals == count and value 0 when n_vals == 1 (any other n_vals is
 *   invalid).  table_index: HOST int32[count] or NULL (table 0); n_tables 2^d_tree <= 262144.  Per sample, with v its value:
 *     1. ACC = v; for i = 0 .. d_rot-1  ACC += C_(s,i) (.) (X^(box 2^i) ACC - ACC) -- the mirror of the lookup's X^(2N - box 2^i); the largest shift is
 *        N - box, so nothing wraps;
 *     2. a demux tree, top down over bits d-1 .. d_rot: the node at depth k splits on bit d-1-k, child 1 = C (.) x, child 0 = x - child 1
 *        (thfhe_lhe_demux); leaf P = sum_t bit_(d_rot+t) 2^t carries ACC, the other 2^d_tree - 1 leaves encrypt zero;
 *     3. leaf P is added into polynomial P of the sample's table, word-wise mod 2^32, masks and bodies.  Tables start from zero.
 *   With f_j at coefficient j < box of v, the table ends with f_j at coefficient (addr mod 2^d_rot) box + j of polynomial addr >> d_rot, the layout of
 *   thfhe.lut.lhe_table.  What v means is not looked at: coefficients >= box spill into the neighbouring entries, unchecked.
 *   tab_a, tab_b: OUT, HOST int32[n_tables][2^d_tree][N].  Exact integers, as thfhe_lhe_cmux; sums of integers do not depend on their order.
 *   d_rot + 2^d_tree - 1 external products per sample; every leaf carries the d products of its path.  The batch runs in slices of at most
 *   max(1, max_candidates / 2^d_tree) samples (thfhe_set_tree_slice; the workspace is 2^d_tree TLWE samples per sample) and 65 535 samples; the tables
 *   stay on the device across the slices and come down once.
 *
 * THFHE_E_INVALID, in the order of thfhe_lhe_lookup: on the host, before the set or the context is looked at, null pointers, the ranges above and
 * every val_index and table_index entry; then samples outside the set (and d_tree + d_rot against its d); then a NULL context or a set of another
 * context.  count 0 returns THFHE_OK once those have passed, with the tables zeroed. */
int thfhe_lhe_demux(thfhe_ctx *ctx, const thfhe_tgsw_set *set, int bit, const int32_t *x_a, const int32_t *x_b /*[count][N]*/, int32_t *out0_a,
                    int32_t *out0_b, int32_t *out1_a, int32_t *out1_b /*[count][N]*/, size_t count);
int thfhe_lhe_scatter(thfhe_ctx *ctx, const thfhe_tgsw_set *set, size_t first, size_t count, int d_tree, int d_rot, const int32_t *val_a,
                      const int32_t *val_b /*[n_vals][N]*/, int n_vals, const int32_t *val_index /*[count]*/, int n_tables,
                      const int32_t *table_index /*[count]*/, int32_t *tab_a, int32_t *tab_b /*[n_tables][2^d_tree][N]*/);

/* ---- circuit bootstrapping (single key, N = 1024): LWE gate outputs -> device-resident TGSW samples, so that bits the circuit
 * computed drive thfhe_lhe_cmux / _lookup / _wfa / _demux / _scatter and the leveled DAG entry.  Level 1 is `ctx` (ring key z, decomposition (l, Bgbit),
 * LWE key s of dimension n); level 2 is a 3-gen context with parties = 1, THE SAME LWE key s and a ternary ring key z2 of degree D = 2048.
 *
 * thfhe_cb_key_set: the private key-switching key pks HOST int32[2][D][t][2][N] (thfhe.keygen.gen_cb_key): row (f, i, p) is a TLWE encryption of zero
 *   under z with z2[i] 2^(32 - (p+1) basebit) added to coefficient 0 of the body (f = 1) or of the mask (f = 0).  1 <= D <= 2048, t >= 1,
 *   1 <= basebit <= 8, t basebit <= 32 (THFHE_E_INVALID, checked before the context is looked at).  The key stays on the device twice, as rows and
 *   as byte planes: 2 x 2 D t 8 KiB (D = 2048, t = 7: 2 x 224 MiB); THFHE_E_NOMEM if that does not fit (no key is set then).  A second call
 *   replaces the key.
 *
 * thfhe_cb_private_keyswitch: stage B alone.  lwe2: HOST int32[count][l][D+1], record (s, j) an LWE sample (a, b) under z2 -> tgsw HOST
 *   int32[count][2l][2][N]: row j = (b X^0, 0) - sum_(i,p) d_ip K[0][i][p], row l + j = (0, b X^0) - sum_(i,p) d_ip K[1][i][p], d_ip in [-B/2, B/2) the
 *   balanced base-2^basebit digits of a_i rounded to t basebit bits (sum_p d_ip 2^(32 - (p+1) basebit) = the rounded word mod 2^32).  Exact
 *   integers.  thfhe_cb_set_batch_threshold: inputs (count l per launch) from which the matrix-core kernel runs instead of the plain one; 0
 *   restores the default.  No output word depends on it.
 *
 * thfhe_circuit_bootstrap: lwe HOST int32[count][d][n+1], gate-encoded records (+-1/8) under s -> *out, a set of `count` samples of d bits for the
 *   calls of section 4.15 - 4.18, and, with tgsw_words != NULL, its rows HOST int32[count][d][2l][2][N] (the layout of thfhe_tgsw_set_create).
 *   Per bit and gadget level j < l: the level-2 gate bootstrap with mu_j = 2^(63 - (j+1) Bgbit), extraction of coefficient 0, the engine's Torus64 ->
 *   Torus32 conversion, + 2^(31 - (j+1) Bgbit) on the body; then the private key switch and the key transform.  Nothing leaves the device between
 *   the stages; the batch runs in slices of 2048 bits.  1 <= d <= 16, 1 <= count <= 2^24.  THFHE_E_INVALID: null pointers and those ranges (before
 *   the contexts are looked at), then a null context, no key, contexts on different devices, a level-2 context without parties = 1, n = ctx's n and
 *   ring degree = the key's D.  THFHE_E_NOMEM (before anything is allocated) if spectra and workspace exceed the free device memory.  With profiling
 *   on, thfhe_last_timings gives ms[0] = stage A, ms[1] = stage B, ms[2] = transform of the LAST slice.  The library cannot check that the two
 *   contexts share s or that the key is from z2 to z: with other keys the call succeeds and the set does not decrypt.
 * thfhe_circuit_bootstrap_mode: thfhe_circuit_bootstrap with stage A chosen by `mode`; THFHE_CB_PER_LEVEL is thfhe_circuit_bootstrap, word for word.
 *   THFHE_CB_ONE_ROTATION takes the l records of a bit from ONE level-2 rotation (many-LUT with the l constants mu_j as the functions): with
 *   theta = the smallest power of two >= l, the record's n + 1 words are mod-switched to multiples of theta, bar = modswitch_{2D/theta}(word) theta
 *   (the prologue of thfhe_mk_lut_bootstrap with one input, weight 1, bias 0); the accumulator starts at (0, X^{-barb} tv), tv[q] = mu_(q mod theta)
 *   for q mod theta < l and 0 otherwise; the CMux chain is the gate bootstrap's; record (bit, j) is the extraction at coefficient j (mask word i
 *   t64tot32(a_{j-i}) for i <= j, t64tot32(-a_{D+j-i}) above, negated mod 2^64 first) with 2^(31 - (j+1) Bgbit) added to the body.  barb is a
 *   multiple of theta and j < theta, so coefficient j is +-mu_j with the sign of coefficient 0.  Stages B and C are the same.  The mode gives OTHER
 *   words than the default (another mod-switch) with the same rotation noise; its price is a theta times coarser mod-switch of the INPUT, which the
 *   gate encoding +-1/8 absorbs (DESIGN 4.21 has the margins) -- an input with a smaller box is the caller's risk.  THFHE_E_INVALID for an unknown
 *   mode, with the null pointers, before the contexts are looked at; THFHE_E_UNSUPPORTED for l > 4 (the engines' theta stops at 4).  The security
 *   caveat of the default mode (sigma_pks near 2^-31) is unchanged.
 * thfhe_cb_stage_a: stage A alone on host buffers, the counterpart of thfhe_cb_private_keyswitch: lwe HOST int32[count][n+1] -> lwe2_out HOST
 *   int32[count][l][D+1], in either mode, in the slices and on the lent stream of thfhe_circuit_bootstrap.  count <= 2^24; count 0 returns THFHE_OK
 *   once the checks have passed.
 * thfhe_mk_lut_rotate_dev (3-gen engine, DEVICE pointers, on the context's stream): d_recs int32[count][P*n+1] -> the theta-rounded prologue of the
 *   records themselves, the accumulator start (0, X^{-barb} d_tv) from the ONE table d_tv int64[N], and the rotation in place in d_acc
 *   int64[count][2][N].  The caller extracts.  theta is 1, 2 or 4; arguments are checked before the context is looked at.
 * thfhe_mk_ctx_info: the parameters and the device of a 3-gen context. */
enum { THFHE_CB_PER_LEVEL = 0, THFHE_CB_ONE_ROTATION = 1 };
int thfhe_cb_key_set(thfhe_ctx *ctx, const int32_t *pks /*[2][D][t][2][N]*/, int D, int t, int basebit);
int thfhe_cb_private_keyswitch(thfhe_ctx *ctx, const int32_t *lwe2 /*[count][l][D+1]*/, size_t count, int32_t *tgsw /*[count][2l][2][N]*/);
int thfhe_cb_set_batch_threshold(thfhe_ctx *ctx, long min_inputs);
int thfhe_circuit_bootstrap(thfhe_ctx *ctx, thfhe_mk_ctx *level2, const int32_t *lwe /*[count][d][n+1]*/, size_t count, int d, int32_t *tgsw_words,
                            thfhe_tgsw_set **out);
int thfhe_circuit_bootstrap_mode(thfhe_ctx *ctx, thfhe_mk_ctx *level2, const int32_t *lwe /*[count][d][n+1]*/, size_t count, int d, int mode,
                                 int32_t *tgsw_words, thfhe_tgsw_set **out);
int thfhe_cb_stage_a(thfhe_ctx *ctx, thfhe_mk_ctx *level2, const int32_t *lwe /*[count][n+1]*/, size_t count, int mode,
                     int32_t *lwe2_out /*[count][l][D+1]*/);
int thfhe_mk_lut_rotate_dev(thfhe_mk_ctx *ctx, const int32_t *d_recs /*[count][P*n+1]*/, int theta, const int64_t *d_tv /*[N]*/,
                            int64_t *d_acc /*[count][2][N]*/, size_t count);
int thfhe_mk_ctx_info(const thfhe_mk_ctx *ctx, thfhe_params *params, int *device);

/* ---- encrypted-table, select and tree nodes in the gate-DAG executor (single key): thfhe_dag_run_lut_batch with three more node
 * kinds, so that a circuit needing a private table, an oblivious pick or a 6-bit -> 3-bit function does not leave the device-resident wire table.
 * nodes: HOST int32[n_nodes][6] = (opcode, in0, in1, in2, x, y); row g defines wire n_inputs + g.  Gate rows, THFHE_LUT and THFHE_LUT_OUT rows mean
 *   exactly what they mean in thfhe_dag_run_lut_batch.  New rows:
 *   (THFHE_LUT_ENC, in0, in1, in2, spec, etab), followed by theta - 1 THFHE_LUT_OUT rows: wire head + j is the record
 *       thfhe_lut_bootstrap_enc(specs[spec], enc_a[etab], enc_b[etab], operands) returns at [0][j], word for word.
 *   (THFHE_SELECT, in0, in1, in2, tree, first): the candidate among the p = trees[tree].p_hi consecutive EARLIER wires first .. first + p - 1 that the
 *       encrypted digit trees[tree].hi forms from the operands points at: thfhe_pack_boxes(candidate records, p) then
 *       thfhe_lut_bootstrap_enc(trees[tree].hi, that table), word for word.  trees[tree].lo is ignored.  The outputs of a many-LUT node (its row and
 *       its LUT_OUT rows) are consecutive wires and serve as candidates directly.
 *   (THFHE_TREE, op0, op1, op2, tree, row0): the first lo.n_inputs operands belong to trees[tree].lo, the next hi.n_inputs to .hi, at most three
 *       together, unused fields -1; level-1 rows tv1[row0 .. row0 + R - 1].  The result is thfhe_tree_lut_bootstrap(ctx, ctx_pack, &lo, &hi, p_hi,
 *       tv1 + row0 N, 1, NULL, operands ...), word for word.
 * specs / tv (as thfhe_dag_run_lut_batch) may both be absent (NULL, 0); enc_a, enc_b: HOST int32[n_enc][N] encrypted tables or NULL, 0, shared by all
 *   instances and uploaded once per call; trees: HOST thfhe_tree_spec[n_trees] (at most 1024); tv1: HOST int32[n_tv1_rows][N] or NULL, 0.
 * Scheduling: every new node costs one level (a SELECT's depth counts its candidates too).  A level's LUT_ENC nodes run as one launch group per
 *   theta, its SELECT and its TREE nodes as one group per distinct trees[] index, after the gate and LUT groups.  A TREE group runs its whole chain
 *   -- level-1 rotations, key switch, box packing, selection rotation, key switch, scatter -- inside its level on the gate context's stream.  A group
 *   is cut into slices of at most thfhe_set_dag_slice nodes over all instances, SELECT / TREE groups also of at most thfhe_set_tree_slice / p_hi.
 * stats: a TREE node counts R + 1 rotations and its group two launches, a LUT_ENC or SELECT node one rotation, their groups one launch.
 * Checks, on the host before any device work and before either context is looked at (THFHE_E_INVALID): those of thfhe_dag_run_lut_batch; etab, tree
 *   or row0 + R out of range; n_enc outside 1 .. 262 144 with a LUT_ENC row present; a tree spec thfhe_tree_lut_bootstrap would refuse; operand counts
 *   that do not match the specs or exceed three; SELECT candidates that are not all earlier wires; a table family that is NULL while a row refers to
 *   it.  Then, when the plan holds a SELECT or TREE node, the context checks of thfhe_tree_lut_bootstrap (same device, a packing key, its n equal to
 *   the gate context's); ctx_pack may be NULL otherwise.  thfhe_dag_run(_batch), thfhe_dag_run_lut_batch and every thfhe_mk_dag_* entry reject the
 *   three opcodes. */
typedef struct thfhe_tree_spec {
    thfhe_lut_spec lo;   /* level 1 (TREE only): 1..3 inputs, theta1 in {1,2,4} */
    thfhe_lut_spec hi;   /* selection rotation: theta must be 1 */
    int32_t p_hi;        /* power of two, 2..N/2; TREE: theta1 | p_hi, R = p_hi / theta1 */
} thfhe_tree_spec;

int thfhe_dag_run_tree_batch(thfhe_ctx *ctx, thfhe_poly_ctx *ctx_pack, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes,
                             const thfhe_lut_spec *specs, int n_specs, const int32_t *tv, int n_luts, const int32_t *enc_a, const int32_t *enc_b, int n_enc,
                             const thfhe_tree_spec *trees, int n_trees, const int32_t *tv1, int n_tv1_rows, size_t instances, const int32_t *out_wires,
                             size_t n_out, int32_t *outputs, int64_t *stats);

/* ---- multi-value nodes in the gate-DAG executor (single key): thfhe_dag_run_tree_batch with two more node kinds and their table
 * families, so that a circuit can hold multi-value rotations.  Every row of thfhe_dag_run_tree_batch means what it means there.  New rows:
 *   (THFHE_MV, in0, in1, in2, mv, t), followed by q - 1 THFHE_LUT_OUT rows (q = mvs[mv].q): wire head + j is the record
 *       thfhe_mv_lut_bootstrap(mvs[mv].lo, mv_tv0[base], table t of the spec, p, q, operands) returns at [0][j], word for word.  The q wires are
 *       consecutive: a later THFHE_SELECT takes them as its candidates directly.  mvs[mv].k must be 1, .hi is ignored.
 *   (THFHE_TREE_MV, op0, op1, op2, mv, t), followed by k - 1 THFHE_LUT_OUT rows: the operands are split between .lo and .hi as a THFHE_TREE row
 *       splits them, at most three together; wire head + j is thfhe_tree_lut_bootstrap_mvk(&lo, &hi, p_hi = q, p_lo = p, k, mv_tv0[base], table t,
 *       operands)[0][j], word for word.
 * mvs: HOST thfhe_mv_spec[n_mvs] (at most 1024) or NULL, 0; mv_tv0: HOST int32[n_bases][N] base vectors (at most 1024) or NULL, 0; mv_factors: HOST
 *   int32[n_factor_words], the taps of every spec: table t of spec m starts at word factors_off + t k q p (k = 1 for MV).  All are uploaded once
 *   per call.  With the three families absent the call is thfhe_dag_run_tree_batch.
 * Scheduling: every new node costs one level.  A level's MV nodes run as one launch group per distinct mvs[] index (one rotation launch: p, q and
 *   the base vector are per launch, the table per job), their outputs scattered q per node; its TREE_MV nodes as one group per mvs[] index, the whole
 *   chain of thfhe_tree_lut_bootstrap_mvk with both prologues reading the wire table.  Slices: at most thfhe_set_dag_slice nodes over all instances;
 *   MV groups also at most thfhe_set_tree_slice / q nodes, TREE_MV groups at most thfhe_set_tree_slice / (k q).
 * stats: an MV node counts one rotation and its group one launch; a TREE_MV node 1 + k rotations and its group two launches.
 * Checks, on the host before any device work and before either context is looked at (THFHE_E_INVALID): those of thfhe_dag_run_tree_batch; mv, t,
 *   base or factors_off + n_tables k q p out of range; a spec the flat entries would refuse (theta != 1, p, q, k, k q > 64, n_tables; an MV row on
 *   a spec with k != 1); a wrong number of LUT_OUT rows after a head; operand counts that do not match the specs or exceed three; a family that is
 *   NULL while a row refers to it.  The context checks of thfhe_tree_lut_bootstrap apply when the plan holds a SELECT, TREE or TREE_MV node; ctx_pack
 *   may be NULL otherwise.  Every other thfhe_dag_* and thfhe_mk_dag_* entry rejects the two opcodes, but thfhe_mk_dag_run_mv_batch (below), which
 *   takes THFHE_MV rows. */
typedef struct thfhe_mv_spec {
    thfhe_lut_spec lo;      /* the multi-value rotation's inputs, theta 1 */
    thfhe_lut_spec hi;      /* TREE_MV: selection inputs, theta 1; ignored by MV */
    int32_t p;              /* taps (p_lo), power of two 2..64 */
    int32_t q;              /* MV: outputs 1..64.  TREE_MV: p_hi, power of two 2..64 */
    int32_t k;              /* TREE_MV: outputs, k q <= 64; MV: must be 1 */
    int32_t base;           /* row of mv_tv0[n_bases][N] */
    int32_t factors_off;    /* word offset of this spec's table 0 in mv_factors; table t at + t k q p */
    int32_t n_tables;
} thfhe_mv_spec;

int thfhe_dag_run_mv_batch(thfhe_ctx *ctx, thfhe_poly_ctx *ctx_pack, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes,
                           const thfhe_lut_spec *specs, int n_specs, const int32_t *tv, int n_luts, const int32_t *enc_a, const int32_t *enc_b, int n_enc,
                           const thfhe_tree_spec *trees, int n_trees, const int32_t *tv1, int n_tv1_rows, const thfhe_mv_spec *mvs, int n_mvs,
                           const int32_t *mv_tv0, int n_bases, const int32_t *mv_factors, size_t n_factor_words, size_t instances,
                           const int32_t *out_wires, size_t n_out, int32_t *outputs, int64_t *stats);

/* ---- multi-value bootstrapping on the 3-gen multi-key engine: the contract of thfhe_mv_lut_bootstrap restated on Torus64, every
 * parameter family (N = the context's ring degree: 1024, 2048 or 4096).  q <= 64 functions of one encrypted digit from ONE blind rotation.
 *
 * thfhe_mk_mv_lut_bootstrap(_wo_keyswitch): spec must have theta 1; prologue, mod-switch, the accumulator start (0, X^{-barb} * tv0), the party-major
 *   CMux chain and the skip of mask words with bara == 0 are those of thfhe_mk_lut_bootstrap at theta = 1.  tv0: HOST int64[N], any words.
 *   factors: HOST int32[n_tables][q][p], p a power of two, 2 <= p <= 64, 1 <= q <= 64, 1 <= n_tables <= 1024; table_index: HOST int32[count] or NULL
 *   (table 0).  With box = N/p, J_k = N - box/2 - k box and E(ACC, J) the UNCONVERTED extraction over int64 (e_i = a_{J-i} for i <= J,
 *   -a_{N+J-i} for i > J, e_N = body_J; negations mod 2^64), record (s, j) is t64tot32, word by word, of
 *       - sum_k factors[t][j][k] * E(ACC_s, J_k)   (+ out_bias on the body word),   t = table_index[s],
 *   all sums mod 2^64, taps sign-extended.  The combination happens in Torus64 BEFORE the one conversion of each word: t64tot32 truncates toward
 *   zero and is not linear, so converting the p extractions first gives other words.  With tv0 = (u, ..., u), step = 2u, and the factors of
 *   thfhe.lut.mv_factors, output j carries f_j(m) * step (+ out_bias) on Torus64; the rotation's noise reaches it times the 2-norm of its taps.
 *   out_bias: one Torus64 word for every output; 0/1 tables at step 2^62 with out_bias = -2^61 leave the rotation in the 3-gen gates' encoding
 *   +-2^61 (thfhe.lut.mv_bool_factors) with half the taps -- and half the rotation noise -- of +-1 tables at step 2^61.
 *   out: HOST int32[count][q][P*n+1] after the multi-key key switch of the count q records, or int32[count][q][N+1] (_wo_keyswitch).
 *   THFHE_E_INVALID on the host, before the context is looked at: the checks of thfhe_mk_lut_bootstrap (tv0 and n_tables in the places of tv and
 *   n_luts), a null factors, theta != 1, a bad p, q or n_tables, a table_index entry out of range.  count 0 returns THFHE_OK.  The batch runs in
 *   slices of at most max_records (thfhe_mk_set_mv_slice, default 4 096, 1 .. 2^20) output records and at least one sample: (N + 1) x 4 B of
 *   workspace per record; only a slice's inputs go up and only its records come down.  thfhe_mk_last_timings: the last slice, prologue | accumulator
 *   start | rotation + multi-value epilogue | key switch on the boundaries of thfhe_mk_lut_bootstrap.
 *
 * thfhe_mk_dag_run_mv_batch: thfhe_mk_dag_run_lut_batch with one more node kind.  New rows: (THFHE_MV, in0, in1, in2, mv, t) followed by q - 1
 *   THFHE_LUT_OUT rows (q = mvs[mv].q), the rows of thfhe_dag_run_mv_batch with the same meaning: wire head + j is the record
 *   thfhe_mk_mv_lut_bootstrap(mvs[mv].lo, mv_tv0[base], table t of the spec, p, q, out_bias = mv_out_bias[mv], operands) returns at [0][j], word for
 *   word.  mvs[mv].k must be 1, .hi is ignored.  mv_tv0: HOST int64[n_bases][N]; mv_factors as in thfhe_dag_run_mv_batch; mv_out_bias: HOST
 *   int64[n_mvs] or NULL (0 for every spec).  specs / tv may be NULL, 0 when no LUT row needs them; with mvs, mv_tv0 and mv_factors all absent the
 *   call is thfhe_mk_dag_run_lut_batch.  THFHE_TREE_MV, THFHE_SELECT, THFHE_TREE and the encrypted-table rows are refused as undefined opcodes: the
 *   flat entries exist, their rows in this executor do not.  One launch group per distinct mvs[] index and level; slices of at most thfhe_mk_set_dag_slice nodes over all
 *   instances and at most max_records / q of them.  stats: an MV node counts one rotation and its group one launch.  Checks as
 *   thfhe_dag_run_mv_batch's for these rows, on the host before the context is looked at. */
int thfhe_mk_mv_lut_bootstrap(thfhe_mk_ctx *ctx, const thfhe_lut_spec *spec, const int64_t *tv0, const int32_t *factors /*[n_tables][q][p]*/, int p,
                              int q, int n_tables, const int32_t *table_index, int64_t out_bias, const int32_t *in0, const int32_t *in1,
                              const int32_t *in2, int32_t *out, size_t count);
int thfhe_mk_mv_lut_bootstrap_wo_keyswitch(thfhe_mk_ctx *ctx, const thfhe_lut_spec *spec, const int64_t *tv0, const int32_t *factors /*[n_tables][q][p]*/,
                                           int p, int q, int n_tables, const int32_t *table_index, int64_t out_bias, const int32_t *in0,
                                           const int32_t *in1, const int32_t *in2, int32_t *out_N1, size_t count);
int thfhe_mk_set_mv_slice(thfhe_mk_ctx *ctx, size_t max_records);
int thfhe_mk_dag_run_mv_batch(thfhe_mk_ctx *ctx, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes,
                              const thfhe_lut_spec *specs, int n_specs, const int64_t *tv, int n_luts, const thfhe_mv_spec *mvs, int n_mvs,
                              const int64_t *mv_tv0, int n_bases, const int32_t *mv_factors, size_t n_factor_words, const int64_t *mv_out_bias,
                              size_t instances, const int32_t *out_wires, size_t n_out, int32_t *outputs, int64_t *stats);

/* ---- multi-key packing key switch, encrypted tables and the two-digit tree on the 3-gen engine: thfhe_pack_boxes,
 * thfhe_lut_bootstrap_enc and thfhe_tree_lut_bootstrap restated on Torus64, every parameter family (N = the context's ring degree).  Phases are
 * beta - alpha (*) Z with Z = sum_q z_q the summed ring key; all arithmetic is integer and wrapping.
 *
 * thfhe_mk_pack_key_set: pk HOST int64[D][t][R][2][N], R = 2^basebit - 1 (thfhe.keygen.gen_mk_pack_key).  D = P*n: the key takes the concatenated
 *   LWE keys (it packs key-switched records and gate outputs); D = N: it takes the coefficients of Z (it packs _wo_keyswitch records; the tree's
 *   key).  1 <= basebit <= 4, t >= 1, t basebit <= 32 (checked before the context is looked at), D one of the two.  A second call replaces the
 *   key.  The key stays on the device: D t R 2N x 8 B (N = 1024, D = N, t = 12, basebit = 1: 192 MiB).  THFHE_E_NOMEM if it does not fit (no key is set then).
 *
 * thfhe_mk_pack_boxes: p records -> ONE encrypted test vector.  recs: HOST int32[count][D+1] (D = the key's), p a power of two, 2 <= p <= 64, count
 *   a multiple of p -> tv_a, tv_b HOST int64[count / p][N].  Digits are the LWE key switch's: abar = a + 2^(31 - t basebit) (nothing at t basebit
 *   = 32; the sum wraps), d_jp = (abar_j >> (32 - (p+1) basebit)) & R, a zero digit contributes nothing.
 *   T_i = (0, (int64) b_i 2^32 on X^0) - sum_{j, p: d != 0} pk[j][p][d - 1] mod 2^64 on both polynomials;
 *   output g = U(X) * sum_{i < p} X^(i N/p) T_(g p + i) mod X^N + 1, U(X) = X^(-N/(2p)) (1 + X + ... + X^(N/p - 1)) -- the layout of thfhe_pack_boxes.
 *   Records with a zero mask give exactly (0, thfhe.lut.test_vector(b 2^32, p, N=N, torus_bits=64)) whatever the key is.  Bit-exact: integer sums.
 *   THFHE_E_INVALID: null pointers, a bad p, a count that is no multiple of p (on the host, before the context is looked at); no key.  count 0
 *   returns THFHE_OK.  The batch runs in slices of at most max_candidates records (thfhe_mk_set_tree_slice).
 *
 * thfhe_mk_lut_bootstrap_enc(_wo_keyswitch): the contract of thfhe_mk_lut_bootstrap(_wo_keyswitch) with ENCRYPTED tables.  Table t is the RLWE
 *   sample (tv_a[t], tv_b[t]) under Z whose phase is a test vector (thfhe.lut.encrypt_table(..., torus_bits=64), or an output of thfhe_mk_pack_boxes).
 *   tv_a, tv_b: HOST int64[n_luts][N], 1 <= n_luts <= 262 144.  Accumulator (X^{-barb} * tv_a[t], X^{-barb} * tv_b[t]), t = lut_index[s], or table 0
 *   when lut_index is NULL; everything else, the argument checks included, is thfhe_mk_lut_bootstrap's.  tv_a = 0, tv_b = tv gives the words of
 *   thfhe_mk_lut_bootstrap(tv).
 *
 * thfhe_mk_tree_lut_bootstrap: out[s] = f_table[s](hi, lo) for two encrypted digits: level-1 many-LUT rotations on `lo` without a key switch, box
 *   packing of their [N+1] records with the D = N key, one rotation of the packed table on `hi`, extraction at coefficient 0 and the multi-key key
 *   switch; three stages per slice on the context's stream, nothing between them visits the host.  spec_lo: 1 .. 3 weighted inputs lo0..2, theta1 in
 *   {1, 2, 4}.  spec_hi: inputs hi0..2, theta must be 1.  p_hi: a power of two, 2 <= p_hi <= 64, theta1 | p_hi; R = p_hi / theta1.  tv1: HOST
 *   int64[n_tables][R][N] (thfhe.lut.tree_test_vectors(..., torus_bits=64)); 1 <= n_tables, n_tables R <= 262 144.  table_index: HOST int32[count] or
 *   NULL (table 0).  lo*, hi*: HOST int32[count][P*n+1]; out: HOST int32[count][P*n+1], which must not alias an input.
 *   The result equals, word for word, thfhe_mk_lut_bootstrap_wo_keyswitch(spec_lo, tv1 rows, lut_index = table R + r) on every sample's inputs repeated
 *   R times -> thfhe_mk_pack_boxes(p = p_hi) -> thfhe_mk_lut_bootstrap_enc(spec_hi, table s for sample s).
 *   THFHE_E_INVALID, before any device work: null pointers, an invalid spec, spec_hi theta != 1, a bad p_hi, theta1 not dividing p_hi, n_tables or a
 *   table_index entry out of range (on the host, before the context is looked at); then no packing key, a packing key with D != N.
 *   The batch runs in slices of at most max_candidates / p_hi samples (thfhe_mk_set_tree_slice, default 16 384 candidates, 1 .. 2^18).  Per candidate
 *   the workspace holds its sum T, 2N x 8 B (16 / 32 / 64 KiB at N = 1024 / 2048 / 4096), its record of (N + 1) x 4 B and, per level-1 rotation, an
 *   accumulator of 2N x 8 B.  With profiling on, thfhe_mk_last_timings gives ms[0] = level 1, ms[1] = packing, ms[2] = selection of the LAST slice
 *   and ms[3] = the three together. */
int thfhe_mk_pack_key_set(thfhe_mk_ctx *ctx, const int64_t *pk, int D, int t, int basebit);
int thfhe_mk_pack_boxes(thfhe_mk_ctx *ctx, const int32_t *recs /*[count][D+1]*/, size_t count, int p, int64_t *tv_a, int64_t *tv_b /*[count/p][N]*/);
int thfhe_mk_lut_bootstrap_enc(thfhe_mk_ctx *ctx, const thfhe_lut_spec *spec, const int64_t *tv_a, const int64_t *tv_b, int n_luts,
                               const int32_t *lut_index, const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out, size_t count);
int thfhe_mk_lut_bootstrap_enc_wo_keyswitch(thfhe_mk_ctx *ctx, const thfhe_lut_spec *spec, const int64_t *tv_a, const int64_t *tv_b, int n_luts,
                                            const int32_t *lut_index, const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out_N1,
                                            size_t count);
int thfhe_mk_tree_lut_bootstrap(thfhe_mk_ctx *ctx, const thfhe_lut_spec *spec_lo, const thfhe_lut_spec *spec_hi, int p_hi,
                                const int64_t *tv1 /*[n_tables][p_hi/theta_lo][N]*/, int n_tables, const int32_t *table_index, const int32_t *lo0,
                                const int32_t *lo1, const int32_t *lo2, const int32_t *hi0, const int32_t *hi1, const int32_t *hi2,
                                int32_t *out /*[count][P*n+1]*/, size_t count);
int thfhe_mk_set_tree_slice(thfhe_mk_ctx *ctx, size_t max_candidates);

/* ---- encrypted dense layers: an integer matrix times a vector of LWE records, fused into the programmable bootstrap.
 *
 * A PBS prologue combines at most three records; a dense layer combines K.  rec = the words of a record of the context (n + 1 single key,
 * P n + 1 on the 3-gen engine), word rec - 1 the body.  For sample s < count, output m < M, word i < rec:
 *     x[s][m][i] = ( sum_{k<K} W[m][k] * in[s][k][i]  +  (i == rec - 1 ? bias[m] : 0) )  mod 2^32
 * Exact integer arithmetic, independent of the order of summation.  With the padding-bit encoding of the PBS every reachable sum of
 * messages sum_k W[m][k] m_k + bias must stay inside [0, p): that is the caller's duty (thfhe.circuits.dense_bias).
 * W: HOST int32[M][K], any int32 values (the products wrap); one matrix serves all samples of a call.  bias: HOST int32[M] Torus32
 * words, or NULL (zero).  in: HOST int32[count][K][rec].  1 <= M, K <= 65536.
 *
 * thfhe_lwe_linear:            out = HOST int32[count][M][rec] = x.
 * thfhe_linear_lut_bootstrap:  out = HOST int32[count][M][theta][rec]: every x[s][m] bootstrapped on table tv[lut_index[m]] (table 0 with a
 *   NULL lut_index), theta in {1, 2, 4} records each.  lut_index: HOST int32[M], the table of OUTPUT m, the same for every sample.  Word for
 *   word the result of thfhe_lwe_linear followed by thfhe_lut_bootstrap(spec = {1, {1}, 0, theta}, tv, n_luts, lut_index'[s M + m] =
 *   lut_index[m], in0 = x); x stays on the device and nothing visits the host between the two stages.
 * thfhe_linear_lut_bootstrap_wo_keyswitch: the same without the key switch, out = HOST int32[count][M][theta][N+1].
 * thfhe_mk_*: the same on a 3-gen context, tv HOST int64[n_luts][N] as in thfhe_mk_lut_bootstrap.
 * thfhe_set_linear_slice / thfhe_mk_set_linear_slice: the most PBS jobs (sample x output) of one slice, 1 .. 2^20, default 4096.  A call runs
 *   in slices of whole samples, at least one sample each (a sample with M above the cap runs alone): only a slice's inputs go up and only its
 *   records come down.  The result does not depend on the setting.
 * thfhe_linear_last_timings / thfhe_mk_linear_last_timings: with profiling on (thfhe_set_profiling), ms[3] = {input upload, linear kernel, upload
 *   start .. end of the key switch} of the last slice of the last dense-layer call, by device events; a call without a key switch ends ms[2] at
 *   the kernel's end.  thfhe_last_timings keeps answering for the PBS stages of that slice.  THFHE_E_INVALID before any profiled call.
 * thfhe_linear_tile: the kernel's output tile and reduction tile (tests place their edges there).
 * Checks, on the host before a context or a device is touched (THFHE_E_INVALID): null W, in, out (or tv), M or K outside 1 .. 65536, theta
 * not in {1, 2, 4}, n_luts outside 1 .. 1024, a lut_index entry outside 0 .. n_luts-1.  count 0 returns THFHE_OK.  in and out must not overlap. */
int thfhe_lwe_linear(thfhe_ctx *ctx, const int32_t *W, const int32_t *bias, int M, int K, const int32_t *in, int32_t *out, size_t count);
int thfhe_linear_lut_bootstrap(thfhe_ctx *ctx, const int32_t *W, const int32_t *bias, int M, int K, int theta, const int32_t *tv, int n_luts,
                               const int32_t *lut_index, const int32_t *in, int32_t *out, size_t count);
int thfhe_linear_lut_bootstrap_wo_keyswitch(thfhe_ctx *ctx, const int32_t *W, const int32_t *bias, int M, int K, int theta, const int32_t *tv,
                                            int n_luts, const int32_t *lut_index, const int32_t *in, int32_t *out_N1, size_t count);
int thfhe_set_linear_slice(thfhe_ctx *ctx, size_t jobs);
int thfhe_linear_last_timings(thfhe_ctx *ctx, float ms[3]);
int thfhe_linear_tile(int *tile_m, int *tile_k);
int thfhe_mk_lwe_linear(thfhe_mk_ctx *ctx, const int32_t *W, const int32_t *bias, int M, int K, const int32_t *in, int32_t *out, size_t count);
int thfhe_mk_linear_lut_bootstrap(thfhe_mk_ctx *ctx, const int32_t *W, const int32_t *bias, int M, int K, int theta, const int64_t *tv, int n_luts,
                                  const int32_t *lut_index, const int32_t *in, int32_t *out, size_t count);
int thfhe_mk_linear_lut_bootstrap_wo_keyswitch(thfhe_mk_ctx *ctx, const int32_t *W, const int32_t *bias, int M, int K, int theta, const int64_t *tv,
                                               int n_luts, const int32_t *lut_index, const int32_t *in, int32_t *out_N1, size_t count);
int thfhe_mk_set_linear_slice(thfhe_mk_ctx *ctx, size_t jobs);
int thfhe_mk_linear_last_timings(thfhe_mk_ctx *ctx, float ms[3]);

/* ---- multi-value two-digit trees on the 3-gen engine: thfhe_tree_lut_bootstrap_mvk restated on Torus64, every parameter family.
 *
 * thfhe_mk_tree_lut_bootstrap_mvk: out[s][j] = f_{t,j}(hi_s, lo_s), j < k, t = table_index[s], in 1 + k rotations per sample.  Three stages per slice
 *   on the context's stream, nothing between them visits the host: ONE multi-value rotation on `lo` with q = k p_hi outputs (output j p_hi + h is
 *   candidate h of table j; out_bias, a Torus64 word, is added to every body word before its conversion), no key switch; the box packing of the
 *   [N+1] records with p = p_hi and the D = N key (table (s, j) is packed sample s k + j); k theta = 1 rotations per sample on `hi`, extraction at
 *   coefficient 0 and the multi-key key switch.  Both specs theta = 1; p_lo, p_hi powers of two in 2 .. 64; 1 <= k, k p_hi <= 64; tv0 HOST int64[N]
 *   (thfhe.lut.tree_mvk_factors(..., torus_bits=64)); factors HOST int32[n_tables][k][p_hi][p_lo], 1 <= n_tables <= 1024; table_index HOST
 *   int32[count] or NULL; lo*, hi* HOST int32[count][P*n+1]; out HOST int32[count][k][P*n+1], which must not alias an input.
 *   The result equals, word for word, thfhe_mk_mv_lut_bootstrap_wo_keyswitch(spec_lo, tv0, factors, p = p_lo, q = k p_hi, ..., out_bias) ->
 *   thfhe_mk_pack_boxes(p = p_hi) -> thfhe_mk_lut_bootstrap_enc(spec_hi) with each sample's `hi` operands repeated k times and lut_index = 0 ..
 *   count k - 1.  THFHE_E_INVALID, on the host before the context is looked at: null pointers, an invalid spec, a theta != 1, a bad p_lo, p_hi, k or
 *   n_tables, a table_index entry out of range, out aliasing an input; then no packing key, a packing key with D != N.  count 0 returns THFHE_OK
 *   after those.  Slices of max(1, max_candidates / (k p_hi)) samples (thfhe_mk_set_tree_slice); per slice one level-1 accumulator per sample, per
 *   candidate its record and its sum, S k tables.  With profiling on, thfhe_mk_last_timings gives ms[0] = level 1 with its epilogue, ms[1] =
 *   packing, ms[2] = selection of the LAST slice and ms[3] = the three together.
 *
 * thfhe_mk_set_pack_wide_threshold: packing calls of at least min_records records (per slice; thfhe_mk_pack_boxes and both trees) run
 *   mk_pack_rows_wide_kernel, which fetches a key row once per 32 records; smaller ones the direct mk_pack_rows_kernel.  0 = never; default 4096, the
 *   smallest measured size from which the wide kernel is the faster on every measured key.  Both kernels give the same words.  thfhe_mk_pack_kernel_name: the rows kernel a packing of `count` records runs, see thfhe_rotation_kernel_name. */
int thfhe_mk_tree_lut_bootstrap_mvk(thfhe_mk_ctx *ctx, const thfhe_lut_spec *spec_lo, const thfhe_lut_spec *spec_hi, int p_hi, int p_lo, int k,
                                    const int64_t *tv0 /*[N]*/, const int32_t *factors /*[n_tables][k][p_hi][p_lo]*/, int n_tables,
                                    const int32_t *table_index, int64_t out_bias, const int32_t *lo0, const int32_t *lo1, const int32_t *lo2,
                                    const int32_t *hi0, const int32_t *hi1, const int32_t *hi2, int32_t *out /*[count][k][P*n+1]*/, size_t count);
/* thfhe_mk_dag_run_tree_batch: thfhe_mk_dag_run_mv_batch plus three node kinds, the rows meaning what they mean in
 *   thfhe_dag_run_tree_batch / thfhe_dag_run_mv_batch, restated on Torus64.  (THFHE_LUT_ENC, in0, in1, in2, spec, etab) + theta - 1 LUT_OUT rows:
 *   thfhe_mk_lut_bootstrap_enc(specs[spec], enc_a[etab], enc_b[etab]); enc_a, enc_b HOST int64[n_enc][N], shared by all instances and uploaded
 *   once.  (THFHE_TREE, op0, op1, op2, tree, row0): thfhe_mk_tree_lut_bootstrap on tv1[row0 .. row0 + R - 1], tv1 HOST int64[n_tv1_rows][N], p_hi <= 64.
 *   (THFHE_TREE_MV, op0, op1, op2, mv, t) + k - 1 LUT_OUT rows: thfhe_mk_tree_lut_bootstrap_mvk with mv_out_bias[mv]; wire head + j is its record
 *   [0][j].  THFHE_SELECT is refused with a message of its own (its candidates would need the D = P*n packing key next to the trees' D = N key,
 *   and a context holds one).  One level per node; LUT_ENC groups per theta, TREE groups per trees[] index, TREE_MV groups per mvs[] index; both
 *   prologues read the wire table.  Slices: thfhe_mk_set_dag_slice nodes over all instances and at most max_candidates / p_hi (TREE), max_candidates
 *   / (k p_hi) (TREE_MV) of them (thfhe_mk_set_tree_slice).  stats (written before the context is looked at): a TREE node counts R + 1 rotations, a
 *   TREE_MV node 1 + k, each group two launches; a LUT_ENC node one rotation, its group one launch.  Checks before any device work: those of the
 *   single-key entries for these rows; then, only when the plan holds a TREE or TREE_MV group, a packing key with D = N.  Every other
 *   thfhe_mk_dag_* entry keeps refusing these opcodes. */
int thfhe_mk_dag_run_tree_batch(thfhe_mk_ctx *ctx, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes,
                                const thfhe_lut_spec *specs, int n_specs, const int64_t *tv, int n_luts, const int64_t *enc_a, const int64_t *enc_b,
                                int n_enc, const thfhe_tree_spec *trees, int n_trees, const int64_t *tv1, int n_tv1_rows, const thfhe_mv_spec *mvs,
                                int n_mvs, const int64_t *mv_tv0, int n_bases, const int32_t *mv_factors, size_t n_factor_words,
                                const int64_t *mv_out_bias, size_t instances, const int32_t *out_wires, size_t n_out, int32_t *outputs, int64_t *stats);
int thfhe_mk_set_pack_wide_threshold(thfhe_mk_ctx *ctx, size_t min_records);
int thfhe_mk_pack_kernel_name(const thfhe_mk_ctx *ctx, size_t count, char *buf, int len);

/* ---- leveled CMux and table lookup on the 64-bit ring of degree 2048: thfhe_tgsw_set_create / thfhe_lhe_cmux / thfhe_lhe_lookup on a
 * one-party 3-gen context, whose external product is the ordinary TGSW (.) TLWE product.  Supported contexts have parties = 1, N = 2048 and run
 * the batched rotation (l x digit parts > 3: the CB sets, l = 2, Bgbit = 18); on any other thfhe_mk_tgsw_set_create returns THFHE_E_UNSUPPORTED and
 * says which condition failed.  Ring samples are (mask a, body b) of Torus64 polynomials, phase b - a (*) z under the context's ring key.
 *
 * thfhe_mk_tgsw_set_create: tgsw: HOST int64[count][d][4][l][N], the layout of a one-party bootstrapping key with n = d
 *   (thfhe.keygen.MKSecretKeySet.tgsw_encrypt): bit i of sample s is part_1 .. part_4 of a TGswSample_3gen, the gadget value
 *   bit * 2^(64 - (level+1) Bgbit) on coefficient 0 of part_1 and part_3.  The samples are uploaded one at a time, transformed on the device and kept as
 *   spectra in the batched path's key layout, count d (2 l parts) 128 KiB (1 MiB per bit on the CB sets); that size is checked against the free
 *   device memory before anything is allocated (THFHE_E_NOMEM), and a failed create leaves nothing behind.  1 <= d <= 16, 1 <= count <= 2^24.  The
 *   set belongs to ctx: destroy it before the context.  thfhe_mk_tgsw_set_destroy(NULL) is a no-op.
 *
 * thfhe_mk_lhe_cmux: out[s] = d0[s] + C_(s,bit) (.) (d1[s] - d0[s]) for the samples s = 0 .. count-1 of the set.  d1_a, d1_b, d0_a, d0_b, out_a,
 *   out_b: HOST int64[count][N].  Exact integers: every word equals the 64-bit decomposition (v = D + offset; digit = ((v >> shift) & mask) - Bg/2,
 *   cut into balanced parts, as the rotation kernels do) and product.
 *
 * thfhe_mk_lhe_lookup(_wo_keyswitch): the contract of thfhe_lhe_lookup on this ring: samples first .. first+count-1 of the set, d_tree + d_rot = d,
 *   0 <= d_tree <= 6, 0 <= d_rot <= 11, box = N >> d_rot, theta in {1, 2, 4} and theta <= box.  tab_b: HOST int64[n_tables][2^d_tree][N]; tab_a: the
 *   masks, or NULL for a public table; n_tables 2^d_tree <= 262144; table_index: HOST int32[count] or NULL (table 0).  Entry e of function j sits at
 *   coefficient e * box + j of polynomial e >> d_rot (thfhe.lut.lhe_table with N = 2048, torus_bits = 64).  Per sample: the CMux tree, level t pairing
 *   neighbours on bit d_rot + t; then for i = 0 .. d_rot-1  ACC += C_(s,i) (.) (X^(2N - box 2^i) ACC - ACC); then coefficients 0 .. theta-1 extracted and
 *   converted to Torus32 as the engine's programmable bootstrap does; then, for the key-switched entry, the context's key switch.
 *   out: HOST int32[count][theta][n+1] or int32[count][theta][N+1] (_wo_keyswitch).  Slices of at most max_candidates / 2^(d_tree-1) samples
 *   (thfhe_mk_set_tree_slice; the tree workspace is 2^(d_tree-1) accumulators of 32 KiB per sample) and 65 535 samples.
 *
 * All checks run on the host before the context is looked at (THFHE_E_INVALID), in the order of thfhe_lhe_lookup: null pointers, the ranges above, a
 * table_index entry out of range, samples outside the set; then a NULL context or a set of another context.  count 0 returns THFHE_OK once those
 * have passed. */
typedef struct thfhe_mk_tgsw_set thfhe_mk_tgsw_set;
int thfhe_mk_tgsw_set_create(thfhe_mk_ctx *ctx, const int64_t *tgsw /*[count][d][4][l][N]*/, size_t count, int d, thfhe_mk_tgsw_set **out);
void thfhe_mk_tgsw_set_destroy(thfhe_mk_tgsw_set *set);
int thfhe_mk_lhe_cmux(thfhe_mk_ctx *ctx, const thfhe_mk_tgsw_set *set, int bit, const int64_t *d1_a, const int64_t *d1_b, const int64_t *d0_a,
                      const int64_t *d0_b /*[count][N]*/, int64_t *out_a, int64_t *out_b, size_t count);
int thfhe_mk_lhe_lookup(thfhe_mk_ctx *ctx, const thfhe_mk_tgsw_set *set, size_t first, size_t count, int d_tree, int d_rot, int theta,
                        const int64_t *tab_a, const int64_t *tab_b /*[n_tables][2^d_tree][N]*/, int n_tables, const int32_t *table_index, int32_t *out);
int thfhe_mk_lhe_lookup_wo_keyswitch(thfhe_mk_ctx *ctx, const thfhe_mk_tgsw_set *set, size_t first, size_t count, int d_tree, int d_rot, int theta,
                                     const int64_t *tab_a, const int64_t *tab_b /*[n_tables][2^d_tree][N]*/, int n_tables, const int32_t *table_index,
                                     int32_t *out_N1);

/* ---- leveled nodes in the gate-DAG executor (single key): thfhe_dag_run_mv_batch with three more node kinds that read the client's
 * TGSW-encrypted bits, so that a leveled lookup, a leveled pick among COMPUTED wires and a layered automaton run between gates on the device-resident
 * wire table.  Every argument before `lhe` means what it means in thfhe_dag_run_mv_batch; with lhe = NULL the call is that call.  Instance q of the
 * run reads sample q of every set.  New rows (operand fields -1):
 *   (THFHE_LHE_LOOKUP, -1, -1, -1, lk, row0), followed by theta - 1 THFHE_LUT_OUT rows: wire head + j of instance q is the record
 *       thfhe_lhe_lookup(ctx, sets[lks[lk].set], q, 1, d_tree, d_rot, theta, tab_a + row0 N, tab_b + row0 N, 1, NULL) returns at [0][j], word for
 *       word; it reads rows row0 .. row0 + 2^d_tree - 1 of the run's table polynomials.
 *   (THFHE_LHE_GATHER, -1, -1, -1, lk, first): one output, lks[lk].theta = 1, 1 <= d_rot <= 9 (the range of p of thfhe_pack_boxes), d_tree <= 6.  The
 *       candidates are the 2^d (d = d_tree + d_rot) consecutive EARLIER wires first .. first + 2^d - 1, candidate e = wire first + e.  The wire equals
 *       thfhe_pack_boxes(ctx_pack, candidate records, 2^d, p = 2^d_rot) -> 2^d_tree TLWE samples -> thfhe_lhe_lookup(.., d_tree, d_rot, 1, those
 *       samples as tab_a / tab_b, 1, NULL), word for word: the box packer's output is a theta = 1 leveled table.
 *   (THFHE_LHE_WFA, -1, -1, -1, wfa, fin_row0), followed by n_out theta - 1 THFHE_LUT_OUT rows: wire head + o theta + j of instance q is
 *       thfhe_lhe_wfa(ctx, sets + set0, n_sets, q, 1, n_steps, n_states, trans, step_bit, fin_a + fin_row0 N, fin_b + fin_row0 N, 1, NULL, theta,
 *       start, n_out) at [0][o][j]; it reads n_states rows from fin_row0.  trans (int32[n_steps][n_states][2]), step_bit (int32[n_steps]) and start
 *       (int32[n_out]) lie in the pool wfa_words at the spec's offsets.
 * Scheduling: every new node costs one level; a GATHER's depth counts its candidates, LOOKUP and WFA nodes have no wire operands and sit on the
 *   first level.  A level's leveled nodes run as one launch group per distinct lks[] / wfas[] index, after the other groups, on the gate context's
 *   stream with no host synchronisation between levels.  The leveled kernels address the TGSW sample by the job number, so a group runs the flat
 *   entry's launch chain once per node with count = the instances of the slice.  Slices: at most thfhe_set_dag_slice instances; LOOKUP and WFA
 *   groups also follow the flat entries' thfhe_set_tree_slice rules, a GATHER slice holds at most thfhe_set_tree_slice / 2^d jobs.
 * stats: a leveled node counts no rotation.  stats[1] counts launch GROUPS, one per group of a level: a leveled group of cnt nodes issues cnt launch
 *   chains per slice (each d_tree CMux launches, a rotation, a key switch and a scatter; a GATHER also its gather and packing), so the kernel
 *   launches of a leveled group are not that figure.
 * thfhe_dag_last_group_ms: with profiling on (thfhe_set_profiling), *ms = the device time of the LAST SELECT / TREE / MV / TREE_MV / leveled group
 *   of the context's last thfhe_dag_run_lut_batch / _tree_batch / _mv_batch / _lhe_batch, first launch to last scatter: a pair of events of its own
 *   on the gate context's stream, no copy inside, which gate levels and the stages' events do not touch; thfhe_last_timings is not changed by it.
 *   THFHE_E_INVALID when profiling is off or that run had no such group.
 * Checks, on the host before any device work and before either context or any set is looked at (THFHE_E_INVALID): those of thfhe_dag_run_mv_batch; a
 *   spec the flat entry would refuse; lk, wfa, row0 + 2^d_tree or fin_row0 + n_states out of range; pool offsets past n_wfa_words; a wrong number of
 *   LUT_OUT rows; operand fields that are not -1; GATHER candidates that are not all earlier wires; GATHER with theta != 1 or d_rot outside 1 .. 9; a
 *   family that is NULL while a row refers to it.  Then: null sets, a set of another context, a set count below `instances`, d_tree + d_rot against
 *   the set's d, step_bit against the spec's sets.  The context checks of thfhe_tree_lut_bootstrap apply when the plan holds a SELECT, TREE, TREE_MV
 *   or GATHER node; ctx_pack may be NULL otherwise.  Every other thfhe_dag_* and thfhe_mk_dag_* entry rejects the three opcodes. */
typedef struct thfhe_dag_lhe_spec {
    int32_t set;      /* index into sets[] */
    int32_t d_tree;   /* 0 .. 6 */
    int32_t d_rot;    /* LOOKUP: 0 .. 10; GATHER: 1 .. 9 */
    int32_t theta;    /* LOOKUP: 1, 2 or 4, at most N >> d_rot; GATHER: 1 */
} thfhe_dag_lhe_spec;

typedef struct thfhe_dag_wfa_spec {
    int32_t n_steps, n_states, theta, n_out;
    int32_t set0, n_sets;   /* the automaton's sets are sets[set0 .. set0 + n_sets - 1]; step_bit = 16 set + bit names set0 + set */
    int32_t trans_off;      /* int32[n_steps][n_states][2] in wfa_words */
    int32_t step_off;       /* int32[n_steps] in wfa_words */
    int32_t start_off;      /* int32[n_out] in wfa_words */
} thfhe_dag_wfa_spec;

typedef struct thfhe_dag_lhe_families {
    const thfhe_tgsw_set *const *sets;   /* HOST array of 1 .. 64 sets of the gate context, each of at least `instances` samples */
    int32_t n_sets;
    const thfhe_dag_lhe_spec *lks;       /* at most 1024, or NULL, 0 */
    int32_t n_lks;
    const int32_t *tab_a, *tab_b;        /* HOST int32[n_tab_rows][N]; tab_a NULL: public tables.  Uploaded once, shared by all instances */
    int32_t n_tab_rows;
    const thfhe_dag_wfa_spec *wfas;      /* at most 1024, or NULL, 0 */
    int32_t n_wfas;
    const int32_t *wfa_words;            /* HOST int32[n_wfa_words] */
    size_t n_wfa_words;
    const int32_t *fin_a, *fin_b;        /* HOST int32[n_fin_rows][N] final weights; fin_a NULL: public */
    int32_t n_fin_rows;
} thfhe_dag_lhe_families;

int thfhe_dag_run_lhe_batch(thfhe_ctx *ctx, thfhe_poly_ctx *ctx_pack, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes,
                            const thfhe_lut_spec *specs, int n_specs, const int32_t *tv, int n_luts, const int32_t *enc_a, const int32_t *enc_b, int n_enc,
                            const thfhe_tree_spec *trees, int n_trees, const int32_t *tv1, int n_tv1_rows, const thfhe_mv_spec *mvs, int n_mvs,
                            const int32_t *mv_tv0, int n_bases, const int32_t *mv_factors, size_t n_factor_words, const thfhe_dag_lhe_families *lhe,
                            size_t instances, const int32_t *out_wires, size_t n_out, int32_t *outputs, int64_t *stats);
int thfhe_dag_last_group_ms(thfhe_ctx *ctx, float *ms);
/* thfhe_dag_last_stage_ms: with profiling on, ms = the device-event times of the three stages of the context's last six-column run
 *   (thfhe_dag_run_lut_batch ... thfhe_dag_run_dense_batch): {the uploads -- input records into the wire table, the plan's index table, the output
 *   wire list --, the levels (every launch group and scatter), the output gather and the download}, events on the gate context's stream.  The host
 *   work before them (checks, plan, workspace, the table families' upload) is the call's wall clock less their sum.  THFHE_E_INVALID when profiling
 *   is off or no such run was made since it went on. */
int thfhe_dag_last_stage_ms(thfhe_ctx *ctx, float ms[3]);

/* ---- circuit-bootstrap nodes in the gate-DAG executor (single key): thfhe_dag_run_lhe_batch with one more node kind, which turns
 * d wires of the run into the d TGSW bits of a COMPUTED set that later leveled rows read, so that an index computed by gates is converted, used by a
 * LOOKUP / GATHER / WFA node and its result fed back into gates in ONE run on the device-resident wire table.  Every argument before `cb` means what
 * it means in thfhe_dag_run_lhe_batch; with cb = NULL the call is that call (level2 may then be NULL; stats[4] = 0).
 *   Row: (THFHE_CB, -1, -1, -1, cbset, -1), exactly one per computed set.  Its operands are the d wires cb_wires[wire_off .. wire_off + d - 1] of
 *       sets[cbset]: earlier wires (inputs too), not necessarily consecutive; they count for the depth as a GATHER's candidates do, the node costs one
 *       level, and its own wire is a word-for-word copy of the wire of bit 0.
 *   Reading: in lks[].set and in a WFA spec's set0 .. set0 + n_sets - 1 an index >= lhe->n_sets names computed set index - lhe->n_sets (lhe->sets may
 *       be NULL with count 0 when every set is computed; a WFA spec may mix the two kinds).  A leveled row that reads a computed set comes after the
 *       set's THFHE_CB row and sits at least one level above it.
 *   Contract: computed set c of a run equals, word for word, what thfhe_circuit_bootstrap_mode(ctx, level2, the operand wires' records as
 *       int32[instances][d][n+1], instances, d, mode, words[c], &set) makes, its rows (cb->words) included; every leveled wire that reads it equals the
 *       flat thfhe_lhe_lookup / thfhe_pack_boxes + thfhe_lhe_lookup / thfhe_lhe_wfa on that set.  THFHE_CB_ONE_ROTATION keeps its caveat: it assumes
 *       gate-encoded (+-1/8) operands.  The security caveat of the private key-switching key's noise is unchanged.
 *   Scheduling: all CB nodes of a level form ONE launch group, run before the level's leveled groups as one batch in slices of
 *       S = min(instances, thfhe_set_dag_slice, 2048 / sum of d) instances: a gather of the operand wires, stage A on S sum-d bits, stage B, one key
 *       transform per node into its set's spectra.  The run lends the gate context's stream to level2 and hands it back whatever happens.
 *   Ownership: the computed sets belong to ctx, grow only, are reused by the next run, and are freed by thfhe_dag_cb_release and with the context.
 *       Before any device work the spectra (instances d 2l 32 KiB per set) not yet held and the slice workspace are checked against the free device
 *       memory: THFHE_E_NOMEM with nothing run.
 *   stats[0..3]: as thfhe_dag_run_lhe_batch; a CB node adds a level, one launch group per level that has CB nodes and no level-1 rotation.
 *       stats[4]: level-2 rotations per instance, sum of d in one-rotation mode (a plan figure), sum of d x l per level (written once ctx is known;
 *       0 when the call is refused before).  thfhe_dag_last_group_ms also answers for a CB group.
 *   Checks, on the host before either context or any set is looked at (THFHE_E_INVALID): those of thfhe_dag_run_lhe_batch; an unknown mode; n_sets
 *       outside 1 .. 64 or client + computed sets above 64; d outside 1 .. 16; wire_off + d past the pool; a pool wire that is not earlier than the
 *       CB row; cbset out of range; a set with no CB row or with two; a leveled row that reads a computed set before its CB row; operand fields or
 *       field 5 not -1; d_tree + d_rot != the computed set's d.  Then the null level2, then the checks of thfhe_circuit_bootstrap on the two contexts.
 *   Every other thfhe_dag_* and thfhe_mk_dag_* entry rejects THFHE_CB. */
typedef struct thfhe_dag_cb_spec {
    int32_t d;          /* 1 .. 16 */
    int32_t wire_off;   /* bit i of sample q = wire cb_wires[wire_off + i] of instance q */
} thfhe_dag_cb_spec;

typedef struct thfhe_dag_cb_families {
    const thfhe_dag_cb_spec *sets;   /* computed sets, 1 .. 64; client sets + computed sets <= 64 */
    int32_t n_sets;
    const int32_t *cb_wires;         /* HOST pool of wire ids */
    size_t n_cb_wires;
    int32_t mode;                    /* THFHE_CB_PER_LEVEL | THFHE_CB_ONE_ROTATION */
    int32_t *const *words;           /* NULL, or per computed set NULL or HOST int32[instances][d][2l][2][N]: the rows of stage B */
} thfhe_dag_cb_families;

int thfhe_dag_run_cb_batch(thfhe_ctx *ctx, thfhe_poly_ctx *ctx_pack, thfhe_mk_ctx *level2, const int32_t *inputs, size_t n_inputs, const int32_t *nodes,
                           size_t n_nodes, const thfhe_lut_spec *specs, int n_specs, const int32_t *tv, int n_luts, const int32_t *enc_a,
                           const int32_t *enc_b, int n_enc, const thfhe_tree_spec *trees, int n_trees, const int32_t *tv1, int n_tv1_rows,
                           const thfhe_mv_spec *mvs, int n_mvs, const int32_t *mv_tv0, int n_bases, const int32_t *mv_factors, size_t n_factor_words,
                           const thfhe_dag_lhe_families *lhe, const thfhe_dag_cb_families *cb, size_t instances, const int32_t *out_wires, size_t n_out,
                           int32_t *outputs, int64_t *stats /*[5]*/);
int thfhe_dag_cb_release(thfhe_ctx *ctx);

/* ---- dense-layer nodes in the gate-DAG executor (both engines): thfhe_dag_run_cb_batch / thfhe_mk_dag_run_tree_batch with one more
 * node kind, an encrypted dense layer (thfhe_linear_lut_bootstrap) whose K operands are wires of the run and whose M theta records go
 * back into wires, so that a quantised network and the gates, tables and lookups around it are ONE run on the device-resident wire table.  Every
 * argument before `dense` means what it means in the entry named; with dense = NULL the call is that call (stats stays [5] / [4]).
 *   Row: (THFHE_DENSE, wire_off, -1, -1, layer, -1), followed by exactly M theta - 1 THFHE_LUT_OUT rows that name its head.  Its operands are the K
 *       wires wires[wire_off .. wire_off + K - 1] of the pool: earlier wires (inputs too), in any order, repeats allowed; they count for the depth as
 *       a CB row's list does, and the node costs one level.  Several rows may name one layers[] entry with different wire_off (a convolution window
 *       at several positions, one comparator on several operand sets).
 *   Contract: wire head + m theta + t of instance q is record [0][m][t] of thfhe_linear_lut_bootstrap(ctx, W, bias, M, K, theta, tv, n_luts,
 *       lut_index, in = the K operand wires' records of instance q, out, 1) -- thfhe_mk_linear_lut_bootstrap on the 3-gen engine, int64 tables and
 *       records of P n + 1 words --, key switch included, word for word.  W = words[w_off ..], bias = words[bias_off ..] (or none), lut_index =
 *       words[lut_off ..] (or table 0 for every output); tv is the run's table family.  The noise rule is the flat call's: the
 *       library cannot see a sum that left [0, p).
 *   Scheduling: the DENSE rows of a level that share a layers[] entry form one launch group; LUT_OUT wires sit on the head's level.  A group runs in
 *       slices of S whole samples (a sample = one node of one instance), S = min(nodes x instances, thfhe_set_dag_slice, max(1,
 *       thfhe_set_linear_slice / M)): the dense kernel reads the operand records in place from the wire table into S M sums, the engine's PBS stage
 *       and key switch run on those, and the S M theta records are scattered into the wires.  A slice may begin and end inside an instance.
 *   stats: a DENSE node counts M rotations and one level, its group one launch.
 *   Checks, on the host before any context is looked at (THFHE_E_INVALID): those of the underlying entry; a family count without its pointer;
 *       n_layers outside 1 .. 1024, n_words outside 1 .. 2^28; M or K outside 1 .. 65 536, theta not 1, 2 or 4; w_off + M K, bias_off + M or
 *       lut_off + M past n_words; a lut_off entry outside 0 .. n_luts - 1 (once per entry a row uses); layer out of range; wire_off + K past the wire
 *       pool; a pool wire that is not earlier than the row; operand fields 2, 3 or field 5 not -1; a missing, extra or misplaced LUT_OUT run; a
 *       DENSE row with no tv.
 *   Every other thfhe_dag_* and thfhe_mk_dag_* entry rejects THFHE_DENSE. */
typedef struct thfhe_dag_dense_spec {
    int32_t M, K;       /* outputs and operands of the layer, 1 .. 65 536 each (the limits of thfhe_lwe_linear) */
    int32_t theta;      /* 1, 2 or 4 records per output */
    int32_t w_off;      /* W = words[w_off .. w_off + M K), int32[M][K] row-major, any int32 values */
    int32_t bias_off;   /* bias = words[bias_off .. + M) Torus32 words, or -1: none */
    int32_t lut_off;    /* table of output m = tv[words[lut_off + m]], or -1: tv[0] for every output */
} thfhe_dag_dense_spec;

typedef struct thfhe_dag_dense_families {
    const thfhe_dag_dense_spec *layers;   /* 1 .. 1024 */
    int32_t n_layers;
    const int32_t *words;                 /* HOST pool: weights, biases, table indices; 1 .. 2^28 words */
    size_t n_words;
    const int32_t *wires;                 /* HOST pool of operand wire ids */
    size_t n_wires;
} thfhe_dag_dense_families;

int thfhe_dag_run_dense_batch(thfhe_ctx *ctx, thfhe_poly_ctx *ctx_pack, thfhe_mk_ctx *level2, const int32_t *inputs, size_t n_inputs, const int32_t *nodes,
                              size_t n_nodes, const thfhe_lut_spec *specs, int n_specs, const int32_t *tv, int n_luts, const int32_t *enc_a,
                              const int32_t *enc_b, int n_enc, const thfhe_tree_spec *trees, int n_trees, const int32_t *tv1, int n_tv1_rows,
                              const thfhe_mv_spec *mvs, int n_mvs, const int32_t *mv_tv0, int n_bases, const int32_t *mv_factors, size_t n_factor_words,
                              const thfhe_dag_lhe_families *lhe, const thfhe_dag_cb_families *cb, const thfhe_dag_dense_families *dense, size_t instances,
                              const int32_t *out_wires, size_t n_out, int32_t *outputs, int64_t *stats /*[5]*/);
int thfhe_mk_dag_run_dense_batch(thfhe_mk_ctx *ctx, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes,
                                 const thfhe_lut_spec *specs, int n_specs, const int64_t *tv, int n_luts, const int64_t *enc_a, const int64_t *enc_b,
                                 int n_enc, const thfhe_tree_spec *trees, int n_trees, const int64_t *tv1, int n_tv1_rows, const thfhe_mv_spec *mvs,
                                 int n_mvs, const int64_t *mv_tv0, int n_bases, const int32_t *mv_factors, size_t n_factor_words,
                                 const int64_t *mv_out_bias, const thfhe_dag_dense_families *dense, size_t instances, const int32_t *out_wires,
                                 size_t n_out, int32_t *outputs, int64_t *stats);

/* ---- multi-key KEY GENERATION arithmetic on the device --------------------------------------------------------------
 * Exact multiply-accumulate of small-coefficient polynomials with torus polynomials, the only non-trivial arithmetic of
 *   tgsw_encrypt_3gen                3-gen-mk-tfhe/src/tgsw_3gen.jl:41-95     part_1..4 = r1 (*) B, r2 (*) B, r2 (*) A, r1 (*) A  (+ m g + e)
 *   PublicKey / CommonPubKey_3gen    3-gen-mk-tfhe/src/mk_internals.jl:266-345 b = z (*) a + e ; B = sum of the parties' b
 *   mk_tgsw_encrypt (CCS)            3-gen-mk-tfhe/src/mk_internals.jl:390-446 d1 = r (*) a + m g + e ; f0 = s (*) f1 + r g + e
 * The randomness (keys, masks, Gaussian noise) is an INPUT, so the device result equals the host key generation bit for bit.
 *   out[j] = addend[j] + sum over the terms (j, s, t, sign) of sign * small[s] (*) torus[t]     mod X^N + 1, mod 2^torus_bits
 *   small  int32[n_small][N], |coefficient| <= 4096;  torus / addend / out  int32 or int64 [.][N] by torus_bits;
 *   terms  int32[n_terms][4] = (out, small, torus, +1 | -1), outputs in ascending order; addend may be NULL.
 * N = 1024 (torus_bits 32 or 64) and N = 2048 (torus_bits 64). */
typedef struct thfhe_pm_ctx thfhe_pm_ctx;
int thfhe_pm_ctx_create(int device, int N, int torus_bits, thfhe_pm_ctx **out);
void thfhe_pm_ctx_destroy(thfhe_pm_ctx *ctx);
int thfhe_pm_mac(thfhe_pm_ctx *ctx, const int32_t *small, size_t n_small, const void *torus, size_t n_torus, const int32_t *terms, size_t n_terms,
                 const void *addend, void *out, size_t n_out);

/* ---- KMS multi-key scheme: mk_bootstrap_new / mk_gate_nand_new ----------------------------------------------
 * reference: 3-gen-mk-tfhe/src/new_mk_internals.jl (mk_ith_blind_rotate :210-225, mk_lev_rlwe_mul :185-207, UniProduct_new :85-127,
 * mk_bootstrap_new :321-325), tlev.jl, new_mk_gates.jl:1-7, parameter sets mk_api.jl:12-30,64-82,120-138 (ring degree 2048, Torus64).
 * The context holds the parties' TGSW bootstrapping keys (spectral, device) and key-switch keys:
 *   gsw  int64[P][n][2 l_gsw][2][N]  row = block * l_gsw + level, column 0 = mask, 1 = body (coefficient domain)
 *   ksk  int32[P][N][t][base-1][n+1]
 * thfhe_kms_tlev_rotate   <- mk_ith_blind_rotate: for `count` gates, party `party`: bara int32[count][n] (the party's mod-switched mask
 *                            words) -> lev int64[count][l_lev][2][N], the rotated TLev accumulator (mask, body per level)
 * thfhe_kms_rlwe_rotate   <- mk_single_blind_rotate (new_mk_internals.jl:226-238, the fast_boot route :255-269): acc int64[count][2][N]
 *                            (mask, body), rotated in place by the party's n TGSW-encrypted key bits
 * thfhe_kms_keyswitch     <- mk_keyswitch (mk_internals.jl:714-728): u int32[count][P N + 1] -> out int32[count][P n + 1]
 * thfhe_kms_set_relin_keys <- the rest of MKBootstrapKey_new (mk_api.jl:440-455): uni int64[P][3][l_uni][N] (d, f0, f1 of every party's
 *                            uni-encryption), pk int64[P][l_uni][N] (public keys), crs int64[l_uni][N] (shared key); transformed once
 * thfhe_kms_lev_rlwe_mul  <- mk_lev_rlwe_mul (new_mk_internals.jl:185-207 = tlev_extern_mul + UniProduct_new :85-127): accum
 *                            int64[count][P+1][N] (a_0 .. a_{P-1}, b) in place, lev int64[count][l_lev][2][N]
 * thfhe_kms_bootstrap     <- mk_bootstrap_new (new_mk_internals.jl:315-325) / mk_bootstrap_wo_keyswitch_new (:302-313): x int32[count][P n+1]
 *                            -> u int32[count][P N + 1] (before the key switch; may be null) and / or out int32[count][P n + 1] (may be null);
 *                            fast_boot != 0 selects mk_blind_rotate_new_v2 (:255-269)
 * thfhe_kms_gates         <- mk_gate_nand_new (new_mk_gates.jl:1-7) and the other two-input gates of gates.jl on the same bootstrap
 * Between the gate's linear part and the key switch everything stays in HBM: prologue, per party the TLev rotation, gadget
 * decompositions and exact polynomial multiply-accumulates of the relinearisation, extraction. */
typedef struct {
    int32_t n, N, parties;
    int32_t l_gsw, bg_gsw;
    int32_t l_lev, bg_lev;
    int32_t l_uni, bg_uni;
    int32_t ks_t, ks_basebit;
} thfhe_kms_params;
typedef struct thfhe_kms_ctx thfhe_kms_ctx;
int thfhe_kms_ctx_create(const thfhe_kms_params *p, const int64_t *gsw, const int32_t *ksk, int device, thfhe_kms_ctx **out);
void thfhe_kms_ctx_destroy(thfhe_kms_ctx *ctx);
int thfhe_kms_tlev_rotate(thfhe_kms_ctx *ctx, int party, const int32_t *bara, int64_t *lev, size_t count);
int thfhe_kms_rlwe_rotate(thfhe_kms_ctx *ctx, int party, const int32_t *bara, int64_t *acc, size_t count);
int thfhe_kms_keyswitch(thfhe_kms_ctx *ctx, const int32_t *u, int32_t *out, size_t count);
int thfhe_kms_set_relin_keys(thfhe_kms_ctx *ctx, const int64_t *uni, const int64_t *pk, const int64_t *crs);
int thfhe_kms_lev_rlwe_mul(thfhe_kms_ctx *ctx, int party, int64_t *accum, const int64_t *lev, size_t count);
int thfhe_kms_bootstrap(thfhe_kms_ctx *ctx, int64_t mu, const int32_t *x, int32_t *u, int32_t *out, size_t count, int fast_boot);
int thfhe_kms_gates(thfhe_kms_ctx *ctx, int op, const int32_t *x, const int32_t *y, int32_t *out, size_t count, int fast_boot);
/* Party-sharded KMS evaluation, device-resident (thfhe/kms_sharded.py): in mk_blind_rotate_new the per-party TLev rotations read nothing the
 * relinearisation writes (new_mk_internals.jl:241-252), so ranks rotate disjoint blocks of parties, exchange the TLev accumulators once
 * (RCCL all-gather on device tensors) and finish replicated.  All pointers are DEVICE pointers; op = opcode NAND .. ORYN or -1 (plain
 * mk_bootstrap_new of x, mu = 1/8).
 *   rotate_parties_dev : gate linear part + mod-switch, then mk_ith_blind_rotate for parties [first_party, first_party + n_parties)
 *                        -> d_lev int64[n_parties][count][l_lev][2][N]                                   (returns after enqueueing)
 *   finish_dev         : trivial accumulator, mk_lev_rlwe_mul for p = 0 .. P-1 with d_lev_all int64[P][count][l_lev][2][N], extraction,
 *                        key switch -> d_out int32[count][P n + 1]                                        (returns after the digit-range check)
 *   set_stream         : enqueue on the caller's HIP stream (NULL: the context's own)                                                    */
int thfhe_kms_rotate_parties_dev(thfhe_kms_ctx *ctx, int op, const int32_t *d_x, const int32_t *d_y, int first_party, int n_parties, int64_t *d_lev,
                                 size_t count);
int thfhe_kms_finish_dev(thfhe_kms_ctx *ctx, int op, const int32_t *d_x, const int32_t *d_y, const int64_t *d_lev_all, int32_t *d_out, size_t count);
int thfhe_kms_set_stream(thfhe_kms_ctx *ctx, void *hip_stream);
/* Launches of at most `max_single_jobs` TLev / RLWE rotations run one job per workgroup, larger ones two jobs per workgroup that share
 * every key chunk (kms_tlev_rotate_pair_kernel).  Default 256 = one workgroup per CU of an MI355X. */
int thfhe_kms_set_pair_threshold(thfhe_kms_ctx *ctx, long max_single_jobs);
int thfhe_kms_rotation_kernel_name(const thfhe_kms_ctx *ctx, size_t rotations, char *buf, int len);   /* see thfhe_rotation_kernel_name */

#ifdef __cplusplus
}
#endif
#endif /* THFHE_HIP_H */
