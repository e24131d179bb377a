"""Gate-DAG front end: the reference's circuits as static gate lists + a levelising evaluator.

The reference's applications issue long dependent streams of two-input gates, one `boots*` call at a time
(FullAdder / difference / distance / distance_bw_data, src/KNN_medical_data.cpp:127-263; mk_add_3gen,
3gen_mk_gates.jl:183-220).  Here the same wiring is recorded as a DAG, scheduled ASAP into levels, and every level is
evaluated as ONE batched launch (thfhe_gates_mixed for the two-input gates, thfhe_gates for the MUXes) so that the
independent gates of a level -- and of independent sub-circuits placed in the same DAG -- fill the GPU.

Bit vectors are MSB-first lists of wire ids, as in the reference (index nbits-1 = least significant bit,
src/bootstrap_modules.cpp:95).

LUT nodes (Circuit.lut): a programmable bootstrap among the gates -- one rotation, one level, theta outputs on consecutive wires
(a THFHE_LUT row, then theta - 1 THFHE_LUT_OUT rows).  Circuits that hold them run on thfhe_dag_run_lut_batch / thfhe_mk_dag_run_lut_batch;
lut_ripple_add, from_gate_bit and to_gate_bit build integer arithmetic from them.

Encrypted-table, select and tree nodes (Circuit.lut_enc / select / tree; single key): a programmable bootstrap of an encrypted
table, an oblivious pick among p consecutive wires, and the two-digit tree PBS, each one level.  Circuits that hold them run on
thfhe_dag_run_tree_batch with the packing context (`pack`); tree_mul_digits multiplies two 3-bit digits with two TREE nodes.

Multi-value nodes (Circuit.mv / tree_mv; single key): q functions of one digit from one rotation on q consecutive wires, and k functions
of two digits in 1 + k rotations on k consecutive wires, each one level.  Circuits that hold them run on thfhe_dag_run_mv_batch; sbox_digits looks a
6-bit -> 4-bit table up in one TREE_MV node.

On the 3-gen multi-key engine LUT_ENC, TREE and TREE_MV nodes on Torus64 tables (int64 enc_table / tree_rows / mv_base, tree_mv's
out_bias) run on thfhe_mk_dag_run_tree_batch with the context's own D = N packing key; SELECT and the leveled nodes stay single-key.

Leveled nodes (Circuit.lhe_lookup / lhe_gather / lhe_wfa; single key): a table lookup, a pick among 2^d computed wires and a layered
automaton on the client's TGSW-encrypted bits (`tgsw_sets`: instance q reads sample q of every set), each one level and no blind rotation.  Circuits
that hold them run on thfhe_dag_run_lhe_batch; lhe_array_read reads an array of computed wires at the client's index, wfa_mux_max takes the larger
of two numbers with one automaton and `width` MUX gates.

Circuit-bootstrap nodes (Circuit.cb_set; single key): d wires of the circuit become the d TGSW bits of a COMPUTED set, whose id the
leveled nodes accept in place of a client set id, one level and d l (or d) level-2 rotations.  Circuits that hold them run on thfhe_dag_run_cb_batch
(`level2`: the level-2 key, default the one CloudKey.cb_key_set named); cb_lookup_dag reads a table at an address the circuit computed, cb_array_read
an array of computed wires at a computed index, cb_mux_max takes the larger of two numbers the circuit holds as gate bits only.

Dense-layer nodes (Circuit.dense_layer / dense; both engines): an encrypted dense layer (CloudKey.linear_lut_bootstrap)
whose K operands are wires and whose M theta records come back as wires, one level and M rotations.  Circuits that hold them run on
thfhe_dag_run_dense_batch / thfhe_mk_dag_run_dense_batch; dense_network chains layers, dense_argmax puts a LUT and gate tail on the last one.
"""
import time

import numpy as np

from . import AND, CB, COPY, DENSE, LHE_GATHER, LHE_LOOKUP, LHE_WFA, LUT, LUT_ENC, LUT_OUT, MUX, MV, NOT, OR, SELECT, TREE, TREE_MV, XOR, _wrap32

_LHE_OPS = (LHE_LOOKUP, LHE_GATHER, LHE_WFA)
CB_SET_BASE = 1 << 16   # Circuit.cb_set returns CB_SET_BASE + c for computed set c; ids below it are the client's sets


class Circuit:
    """A static gate list.  Wires are integers; inputs are declared first, every gate defines one new wire."""

    def __init__(self):
        self.n_inputs = 0
        self.gates = []   # (op, a, b, c) ; c = -1 unless MUX ; output wire id = n_inputs + index
        self.outputs = {}
        self.tables = []      # test vectors of the LUT nodes (table ids index this list)
        self.specs = []       # (n_inputs, (w0, w1, w2), bias, theta) of the LUT nodes, deduplicated
        self.lut_rows = {}    # gate index of a LUT node -> (spec id, table id)
        self.enc_tables = []  # (tv_a, tv_b, plaintext test vector or None) of the LUT_ENC nodes (the plaintext serves simulate only)
        self.tree_specs = []  # (lo spec or None, hi spec, p_hi) of the SELECT / TREE launch groups, deduplicated
        self.tv1 = []         # level-1 rows int32[N] of the TREE nodes, blocks of R registered by tree_rows
        self.ext_rows = {}    # gate index of a LUT_ENC / SELECT / TREE node -> (spec id, etab) / (tree id, first) / (tree id, row0)
        self.mv_bases = []    # base vectors int32[N] of the MV / TREE_MV nodes
        self.mv_specs = []    # [lo spec, hi spec or None, p, q, k, base id, [factor tables int32[k][q][p]]] of the MV / TREE_MV launch groups
        self.mv_rows = {}     # gate index of an MV / TREE_MV node -> (mv id, table t of that spec)
        self.mv_out_bias = {} # mv id -> the Torus64 word added to every output of its MV nodes (multi-key engine only; absent: 0)
        self.lhe_tab = []     # table polynomials of the LHE_LOOKUP nodes: (body int32[N], mask or None, plaintext polynomial or None), rows of lhe_table
        self.lhe_fin = []     # final weights of the LHE_WFA nodes, the same triples, rows of lhe_finals
        self.lhe_specs = []   # (set, d_tree, d_rot, theta) of the LHE_LOOKUP / LHE_GATHER launch groups, deduplicated
        self.wfa_specs = []   # (trans, step_bit, start, theta, set0, n_sets) of the LHE_WFA launch groups
        self.lhe_rows = {}    # gate index of a leveled node -> (lk, row0) / (lk, first) / (wfa, fin_row0)
        self.cb_specs = []    # the operand wires (bit 0 first) of every computed set, in the order of cb_set
        self.cb_rows = {}     # gate index of a CB node -> (computed set, -1)
        self.dense_specs = [] # (W int32[M][K], bias int32[M] or None, table ids int32[M] or None, theta) of the DENSE launch groups, deduplicated
        self.dense_wires = [] # the pool of operand wire ids of the DENSE nodes; a node's gate tuple is (DENSE, wire_off, -1, -1)
        self.dense_rows = {}  # gate index of a DENSE node -> (layer, -1)
        self._ids = {}

    def inputs(self, count):
        assert not self.gates, "declare all inputs before the first gate"
        ids = list(range(self.n_inputs, self.n_inputs + count))
        self.n_inputs += count
        return ids

    def gate(self, op, a=-1, b=-1, c=-1):
        self.gates.append((op, a, b, c))
        return self.n_inputs + len(self.gates) - 1

    def table(self, tv):
        """Register a test vector (thfhe.lut.test_vector: int32[N] for the single-key engine, int64[N] with torus_bits=64 for the 3-gen one);
        returns its table id.  Equal tables share one id."""
        tv = np.ascontiguousarray(tv)
        key = ("table", tv.dtype.str, tv.tobytes())
        if key not in self._ids:
            self._ids[key] = len(self.tables)
            self.tables.append(tv)
        return self._ids[key]

    def lut(self, table_id, inputs, weights=(1,), bias=0, theta=1):
        """A LUT node: programmable bootstrap of x = sum_q weights[q] * inputs[q] + (0, bias) through table `table_id`, theta outputs from one
        rotation.  Returns the theta output wire ids (consecutive: the node's row, then theta - 1 LUT_OUT rows)."""
        inputs = list(inputs)
        if not 1 <= len(inputs) <= 3 or len(weights) != len(inputs):
            raise ValueError("a LUT node takes 1 to 3 inputs and one weight per input")
        if theta not in (1, 2, 4):
            raise ValueError("theta must be 1, 2 or 4")
        if not 0 <= table_id < len(self.tables):
            raise ValueError(f"unknown table id {table_id}")
        spec = (len(inputs), tuple(_wrap32(w) for w in list(weights) + [0] * (3 - len(weights))), _wrap32(bias), int(theta))
        key = ("spec",) + spec
        if key not in self._ids:
            self._ids[key] = len(self.specs)
            self.specs.append(spec)
        head = self.gate(LUT, *(inputs + [-1] * (3 - len(inputs))))
        self.lut_rows[len(self.gates) - 1] = (self._ids[key], int(table_id))
        return [head] + [self.gate(LUT_OUT, head) for _ in range(theta - 1)]

    def _spec_id(self, n_in, weights, bias, theta):
        spec = (n_in, tuple(_wrap32(w) for w in list(weights) + [0] * (3 - len(weights))), _wrap32(bias), int(theta))
        key = ("spec",) + spec
        if key not in self._ids:
            self._ids[key] = len(self.specs)
            self.specs.append(spec)
        return self._ids[key]

    def _tree_id(self, lo, hi, p):
        if p < 2 or p > 512 or p & (p - 1):
            raise ValueError("p must be a power of two in 2 .. 512")
        key = ("tree", lo, hi, int(p))
        if key not in self._ids:
            self._ids[key] = len(self.tree_specs)
            self.tree_specs.append((lo, hi, int(p)))
        return self._ids[key]

    def enc_table(self, tv_a, tv_b, plain=None):
        """Register an encrypted table: the TLWE sample (tv_a, tv_b) int32[N] under the bootstrapping ring key (thfhe.lut.encrypt_table, or
        PackBoxes' output); returns its id.  Equal samples share one id.  plain: its plaintext test vector, carried for simulate only.  int64 arrays
        are kept as the Torus64 RLWE sample of a circuit for the 3-gen multi-key engine (thfhe.lut.encrypt_table(..., torus_bits=64))."""
        dt = np.int64 if np.asarray(tv_b).dtype == np.int64 else np.int32
        a, b = np.ascontiguousarray(tv_a, dt).reshape(-1), np.ascontiguousarray(tv_b, dt).reshape(-1)
        if a.shape != b.shape:
            raise ValueError("tv_a and tv_b differ in shape")
        key = ("enc", a.tobytes(), b.tobytes())
        if key not in self._ids:
            self._ids[key] = len(self.enc_tables)
            self.enc_tables.append((a, b, None if plain is None else np.ascontiguousarray(plain, dt).reshape(-1)))
        return self._ids[key]

    def lut_enc(self, etab, inputs, weights=(1,), bias=0, theta=1):
        """A LUT_ENC node: Circuit.lut on the encrypted table `etab` (enc_table).  Returns the theta output wire ids (consecutive)."""
        inputs = list(inputs)
        if not 1 <= len(inputs) <= 3 or len(weights) != len(inputs):
            raise ValueError("a LUT_ENC node takes 1 to 3 inputs and one weight per input")
        if theta not in (1, 2, 4):
            raise ValueError("theta must be 1, 2 or 4")
        if not 0 <= etab < len(self.enc_tables):
            raise ValueError(f"unknown encrypted table id {etab}")
        si = self._spec_id(len(inputs), weights, bias, theta)
        head = self.gate(LUT_ENC, *(inputs + [-1] * (3 - len(inputs))))
        self.ext_rows[len(self.gates) - 1] = (si, int(etab))
        return [head] + [self.gate(LUT_OUT, head) for _ in range(theta - 1)]

    def tree_rows(self, rows):
        """Register the R level-1 rows int32[R][N] of a tree function (thfhe.lut.tree_test_vectors); returns row0, the index of the first.  Equal row
        blocks share one row0.  int64 rows (thfhe.lut.tree_test_vectors(..., torus_bits=64)) are kept as the Torus64 rows of a circuit for the 3-gen
        multi-key engine."""
        rows = np.asarray(rows)
        rows = np.ascontiguousarray(rows, np.int64 if rows.dtype == np.int64 else np.int32)
        if rows.ndim != 2 or rows.shape[0] < 1:
            raise ValueError("tree_rows: expected int32[R][N]")
        key = ("tv1", rows.dtype.str, rows.shape, rows.tobytes())
        if key not in self._ids:
            self._ids[key] = len(self.tv1)
            self.tv1.extend(rows)
        return self._ids[key]

    def tree(self, row0, lo_inputs, hi_inputs, p_hi, lo_weights=None, hi_weights=None, lo_bias=0, hi_bias=0, theta1=1):
        """A TREE node: f(hi, lo) of two encrypted digits by the two-digit tree PBS (R = p_hi / theta1 level-1 rotations of the rows row0 .. row0 + R - 1
        on the `lo` digit, box packing, one rotation of the packed table on the `hi` digit), one level, one output wire.  lo_inputs and hi_inputs
        number at most three together; the weights default to ones."""
        lo_inputs, hi_inputs = list(lo_inputs), list(hi_inputs)
        lo_weights = (1,) * len(lo_inputs) if lo_weights is None else tuple(lo_weights)
        hi_weights = (1,) * len(hi_inputs) if hi_weights is None else tuple(hi_weights)
        if not lo_inputs or not hi_inputs or len(lo_inputs) + len(hi_inputs) > 3:
            raise ValueError("a TREE node takes at least one lo and one hi input, at most three together")
        if len(lo_weights) != len(lo_inputs) or len(hi_weights) != len(hi_inputs):
            raise ValueError("one weight per input")
        if theta1 not in (1, 2, 4) or p_hi % theta1:
            raise ValueError("theta1 must be 1, 2 or 4 and divide p_hi")
        if not 0 <= row0 or row0 + p_hi // theta1 > len(self.tv1):
            raise ValueError("row0 + R exceeds the registered level-1 rows (tree_rows)")
        lo = (len(lo_inputs), tuple(_wrap32(w) for w in list(lo_weights) + [0] * (3 - len(lo_weights))), _wrap32(lo_bias), int(theta1))
        hi = (len(hi_inputs), tuple(_wrap32(w) for w in list(hi_weights) + [0] * (3 - len(hi_weights))), _wrap32(hi_bias), 1)
        ti = self._tree_id(lo, hi, p_hi)
        ops = lo_inputs + hi_inputs
        w = self.gate(TREE, *(ops + [-1] * (3 - len(ops))))
        self.ext_rows[len(self.gates) - 1] = (ti, int(row0))
        return w

    def select(self, index_inputs, first, p, weights=None, bias=0):
        """A SELECT node: the wire among first .. first + p - 1 (all defined above) that the encrypted digit sum_q weights[q] * index_inputs[q] + (0, bias)
        points at, obliviously: box packing of the p candidates and one rotation of the packed table.  One level, one output wire."""
        index_inputs = list(index_inputs)
        weights = (1,) * len(index_inputs) if weights is None else tuple(weights)
        if not 1 <= len(index_inputs) <= 3 or len(weights) != len(index_inputs):
            raise ValueError("a SELECT node takes 1 to 3 index inputs and one weight per input")
        hi = (len(index_inputs), tuple(_wrap32(w) for w in list(weights) + [0] * (3 - len(weights))), _wrap32(bias), 1)
        if first < 0 or first + p > self.n_wires():
            raise ValueError("the candidates first .. first + p - 1 must be wires defined above the node")
        ti = self._tree_id(None, hi, p)
        w = self.gate(SELECT, *(index_inputs + [-1] * (3 - len(index_inputs))))
        self.ext_rows[len(self.gates) - 1] = (ti, int(first))
        return w

    def mv_base(self, tv0):
        """Register the base vector int32[N] of multi-value rotations (thfhe.lut.mv_base, or the first result of tree_mv_factors / tree_mvk_factors);
        returns its id.  Equal vectors share one id.  An int64 array is kept as the Torus64 base vector of a circuit for the multi-key engine
        (thfhe.lut.mv_base(step, N, torus_bits=64))."""
        tv0 = np.asarray(tv0)
        tv0 = np.ascontiguousarray(tv0, np.int64 if tv0.dtype == np.int64 else np.int32).reshape(-1)
        key = ("mv_base", tv0.dtype.str, tv0.tobytes())
        if key not in self._ids:
            self._ids[key] = len(self.mv_bases)
            self.mv_bases.append(tv0)
        return self._ids[key]

    def _mv_row(self, op, lo, hi, base, w, operands, out_bias=0):
        """An MV / TREE_MV row on the factor table w int32[k][q][p]: its launch group's spec (one per distinct prologues, shape and base) and the
        table's index in it; the head wire and its LUT_OUT rows."""
        k, q, p = w.shape
        if not 0 <= base < len(self.mv_bases):
            raise ValueError(f"unknown base vector id {base}")
        if p < 2 or p > 64 or p & (p - 1) or k * q > 64:
            raise ValueError("p must be a power of two in 2 .. 64 and the node's rotation has at most 64 outputs")
        key = ("mv", lo, hi, p, q, k, int(base)) + ((int(out_bias),) if out_bias else ())
        if key not in self._ids:
            self._ids[key] = len(self.mv_specs)
            self.mv_specs.append([lo, hi, p, q, k, int(base), []])
            if out_bias:
                self.mv_out_bias[self._ids[key]] = int(out_bias)
        mi = self._ids[key]
        tabs = self.mv_specs[mi][6]
        t = next((i for i, x in enumerate(tabs) if np.array_equal(x, w)), len(tabs))
        if t == len(tabs):
            tabs.append(w)
        head = self.gate(op, *(operands + [-1] * (3 - len(operands))))
        self.mv_rows[len(self.gates) - 1] = (mi, t)
        return [head] + [self.gate(LUT_OUT, head) for _ in range((k if op == TREE_MV else q) - 1)]

    def mv(self, base, factors, inputs, weights=(1,), bias=0, out_bias=0):
        """An MV node: q functions of the digit x = sum_q weights[q] * inputs[q] + (0, bias) from ONE rotation of the base vector `base` (mv_base),
        function j through the taps factors[j] (thfhe.lut.mv_factors: int32[q][p]).  Returns the q output wire ids (consecutive: a SELECT can take
        them as its candidates).  out_bias: the Torus64 word the multi-key engine adds to every output (thfhe.lut.mv_bool_factors); the single-key
        engine has none."""
        inputs = list(inputs)
        if not 1 <= len(inputs) <= 3 or len(weights) != len(inputs):
            raise ValueError("an MV node takes 1 to 3 inputs and one weight per input")
        w = np.ascontiguousarray(factors, np.int32)
        if w.ndim != 2:
            raise ValueError("factors: expected int32[q][p]")
        lo = (len(inputs), tuple(_wrap32(v) for v in list(weights) + [0] * (3 - len(weights))), _wrap32(bias), 1)
        return self._mv_row(MV, lo, None, base, w[None], inputs, out_bias)

    def tree_mv(self, base, factors, lo_inputs, hi_inputs, lo_weights=None, hi_weights=None, lo_bias=0, hi_bias=0, out_bias=0):
        """A TREE_MV node: k functions f_j(hi, lo) of two encrypted digits in 1 + k rotations (one multi-value rotation of the base vector `base` on
        the `lo` digit with k p_hi outputs, box packing, k selection rotations on the `hi` digit), one level.  factors: int32[k][p_hi][p_lo]
        (thfhe.lut.tree_mvk_factors).  lo_inputs and hi_inputs number at most three together.  Returns the k output wire ids (consecutive).
        out_bias: the Torus64 word the multi-key engine adds to every level-1 candidate (thfhe.lut.tree_mvk_bool_factors, on a Torus64 base); the
        single-key engine has none."""
        lo_inputs, hi_inputs = list(lo_inputs), list(hi_inputs)
        lo_weights = (1,) * len(lo_inputs) if lo_weights is None else tuple(lo_weights)
        hi_weights = (1,) * len(hi_inputs) if hi_weights is None else tuple(hi_weights)
        if not lo_inputs or not hi_inputs or len(lo_inputs) + len(hi_inputs) > 3:
            raise ValueError("a TREE_MV node takes at least one lo and one hi input, at most three together")
        if len(lo_weights) != len(lo_inputs) or len(hi_weights) != len(hi_inputs):
            raise ValueError("one weight per input")
        w = np.ascontiguousarray(factors, np.int32)
        if w.ndim != 3 or w.shape[1] < 2 or w.shape[1] & (w.shape[1] - 1):
            raise ValueError("factors: expected int32[k][p_hi][p_lo], p_hi a power of two")
        lo = (len(lo_inputs), tuple(_wrap32(v) for v in list(lo_weights) + [0] * (3 - len(lo_weights))), _wrap32(lo_bias), 1)
        hi = (len(hi_inputs), tuple(_wrap32(v) for v in list(hi_weights) + [0] * (3 - len(hi_weights))), _wrap32(hi_bias), 1)
        return self._mv_row(TREE_MV, lo, hi, base, w, lo_inputs + hi_inputs, out_bias)

    def _lhe_rows(self, store, rows_b, rows_a, plain, what):
        b = np.ascontiguousarray(rows_b, np.int32)
        b = b[None] if b.ndim == 1 else b
        if b.ndim != 2 or b.shape[0] < 1:
            raise ValueError(f"{what}: expected int32[rows][N]")
        a = None if rows_a is None else np.ascontiguousarray(rows_a, np.int32).reshape(b.shape)
        pl = None if plain is None else np.ascontiguousarray(plain, np.int32).reshape(b.shape)
        if a is None and pl is None:
            pl = b   # a public polynomial is its own plaintext
        row0 = len(store)
        store.extend((b[i], None if a is None else a[i], None if pl is None else pl[i]) for i in range(b.shape[0]))
        return row0

    def lhe_table(self, rows_b, rows_a=None, plain=None):
        """Register table polynomials int32[rows][N] of the LHE_LOOKUP nodes (thfhe.lut.lhe_table: 2^d_tree per table; rows_a: the masks of an
        encrypted table, None: public); returns row0, the index of the first.  plain: the plaintext polynomials of an encrypted table, for simulate."""
        return self._lhe_rows(self.lhe_tab, rows_b, rows_a, plain, "lhe_table")

    def lhe_finals(self, rows_b, rows_a=None, plain=None):
        """Register the n_states final weights int32[n_states][N] of an automaton (thfhe.lut.wfa_finals); returns fin_row0.  As lhe_table."""
        return self._lhe_rows(self.lhe_fin, rows_b, rows_a, plain, "lhe_finals")

    def _lk_id(self, set_id, d_tree, d_rot, theta):
        key = ("lk", int(set_id), int(d_tree), int(d_rot), int(theta))
        if set_id < 0 or not 0 <= d_tree <= 6 or not 0 <= d_rot <= 10 or theta not in (1, 2, 4) or theta > (1024 >> d_rot):
            raise ValueError("leveled node: set_id >= 0, d_tree 0 .. 6, d_rot 0 .. 10, theta 1, 2 or 4 and at most N >> d_rot")
        if key not in self._ids:
            self._ids[key] = len(self.lhe_specs)
            self.lhe_specs.append(key[1:])
        return self._ids[key]

    def lhe_lookup(self, set_id, row0, d_tree, d_rot, theta=1):
        """An LHE_LOOKUP node: the table of 2^d_tree polynomials from row0 (lhe_table) read at the address the instance's sample of TGSW set `set_id`
        encrypts (d_tree + d_rot bits, low bits rotate, high bits pick the polynomial): theta consecutive coefficients from addr_lo N / 2^d_rot.  One
        level, no rotation key.  Returns the theta output wire ids (consecutive)."""
        lk = self._lk_id(set_id, d_tree, d_rot, theta)
        if self._set_d(set_id) not in (None, d_tree + d_rot):
            raise ValueError("d_tree + d_rot must equal the computed set's d")
        if row0 < 0 or row0 + (1 << d_tree) > len(self.lhe_tab):
            raise ValueError("row0 + 2^d_tree exceeds the registered table polynomials (lhe_table)")
        head = self.gate(LHE_LOOKUP)
        self.lhe_rows[len(self.gates) - 1] = (lk, int(row0))
        return [head] + [self.gate(LUT_OUT, head) for _ in range(theta - 1)]

    def lhe_gather(self, set_id, first, d_tree, d_rot):
        """An LHE_GATHER node: the wire among first .. first + 2^d - 1 (d = d_tree + d_rot, all defined above) at the index the instance's sample of
        TGSW set `set_id` encrypts: box packing of the candidates into 2^d_tree samples and d CMuxes.  1 <= d_rot <= 9.  One level, one output wire."""
        if not 1 <= d_rot <= 9:
            raise ValueError("lhe_gather: d_rot must be 1 .. 9")
        lk = self._lk_id(set_id, d_tree, d_rot, 1)
        if self._set_d(set_id) not in (None, d_tree + d_rot):
            raise ValueError("d_tree + d_rot must equal the computed set's d")
        if first < 0 or first + (1 << (d_tree + d_rot)) > self.n_wires():
            raise ValueError("the candidates first .. first + 2^d - 1 must be wires defined above the node")
        w = self.gate(LHE_GATHER)
        self.lhe_rows[len(self.gates) - 1] = (lk, int(first))
        return w

    def lhe_wfa(self, automaton, set_ids, finals_row0, theta=1):
        """An LHE_WFA node: the layered automaton (trans, step_bit, finals, start) -- what wfa_less_than and friends return -- on the consecutive TGSW
        sets set_ids (step_bit = 16 set + bit counts within them), its final weights the n_states rows from finals_row0 (lhe_finals).  One level.
        Returns the n_out theta output wire ids (consecutive, output-major)."""
        trans, step_bit, _, start = automaton
        trans = np.ascontiguousarray(trans, np.int32)
        step_bit, start = np.ascontiguousarray(step_bit, np.int32).reshape(-1), np.ascontiguousarray(start, np.int32).reshape(-1)
        set_ids = [int(v) for v in set_ids]
        if trans.ndim != 3 or trans.shape[2] != 2 or step_bit.shape[0] != trans.shape[0] or not start.shape[0]:
            raise ValueError("automaton: expected (trans int32[n_steps][n_states][2], step_bit int32[n_steps], finals, start int32[n_out])")
        if not set_ids or set_ids[0] < 0 or set_ids != list(range(set_ids[0], set_ids[0] + len(set_ids))):
            raise ValueError("lhe_wfa: set_ids must be consecutive set ids")
        if set_ids[0] < CB_SET_BASE <= set_ids[-1] or (set_ids[0] >= CB_SET_BASE and self._set_d(set_ids[-1]) is None):
            raise ValueError("lhe_wfa: set_ids must be all client sets or all computed sets (the C entry alone mixes the two)")
        if theta not in (1, 2, 4):
            raise ValueError("theta must be 1, 2 or 4")
        if finals_row0 < 0 or finals_row0 + trans.shape[1] > len(self.lhe_fin):
            raise ValueError("finals_row0 + n_states exceeds the registered final weights (lhe_finals)")
        key = ("wfa", trans.shape, trans.tobytes(), step_bit.tobytes(), start.tobytes(), int(theta), set_ids[0], len(set_ids))
        if key not in self._ids:
            self._ids[key] = len(self.wfa_specs)
            self.wfa_specs.append((trans, step_bit, start, int(theta), set_ids[0], len(set_ids)))
        head = self.gate(LHE_WFA)
        self.lhe_rows[len(self.gates) - 1] = (self._ids[key], int(finals_row0))
        return [head] + [self.gate(LUT_OUT, head) for _ in range(start.shape[0] * theta - 1)]

    def cb_set(self, wires):
        """A CB node: circuit bootstrapping of the 1 .. 16 wires `wires` (bit 0 first; inputs too, not necessarily consecutive; gate-encoded in
        one-rotation mode) into the TGSW bits of a computed set.  One level.  Returns the set id that lhe_lookup / lhe_gather / lhe_wfa accept in
        place of a client set id; the node's own wire (a copy of bit 0's) is n_wires() - 1 right after the call."""
        wires = [int(w) for w in wires]
        if not 1 <= len(wires) <= 16 or any(w < 0 or w >= self.n_wires() for w in wires):
            raise ValueError("cb_set: expected 1 .. 16 wires defined above the node")
        self.gate(CB)
        self.cb_rows[len(self.gates) - 1] = (len(self.cb_specs), -1)
        self.cb_specs.append(wires)
        return CB_SET_BASE + len(self.cb_specs) - 1

    def dense_layer(self, W, bias=None, table_ids=None, theta=1):
        """Register a dense layer: W int[M][K] (any int32 values), bias M Torus32 words or None, table_ids the table (Circuit.table) of every output or
        None (table 0 for all), theta records per output.  Returns its layer id; equal layers share one id."""
        W = np.ascontiguousarray(np.asarray(W, np.int64), np.int64)
        if W.ndim != 2 or W.size == 0 or max(W.shape) > 65536:
            raise ValueError("dense_layer: W must be int[M][K] with 1 <= M, K <= 65536")
        if theta not in (1, 2, 4):
            raise ValueError("theta must be 1, 2 or 4")
        W = (W & 0xFFFFFFFF).astype(np.uint32).view(np.int32)   # any integer, taken mod 2^32 as _wrap32 does
        b = None if bias is None else np.array([_wrap32(v) for v in np.asarray(bias).reshape(-1)], np.int32)
        t = None if table_ids is None else np.ascontiguousarray(table_ids, np.int32).reshape(-1)
        if (b is not None and b.shape[0] != W.shape[0]) or (t is not None and t.shape[0] != W.shape[0]):
            raise ValueError("dense_layer: bias and table_ids hold one entry per output")
        if t is not None and (t.min() < 0 or t.max() >= len(self.tables)):
            raise ValueError("dense_layer: unknown table id")
        key = ("dense", W.shape, W.tobytes(), None if b is None else b.tobytes(), None if t is None else t.tobytes(), int(theta))
        if key not in self._ids:
            self._ids[key] = len(self.dense_specs)
            self.dense_specs.append((W, b, t, int(theta)))
        return self._ids[key]

    def dense(self, layer, inputs):
        """A DENSE node: layer `layer` (dense_layer) on the K wires `inputs` (any earlier wires, in any order, repeats allowed).  One level, M
        rotations.  Returns M lists of theta wire ids (consecutive: the node's row, then M theta - 1 LUT_OUT rows)."""
        if not 0 <= layer < len(self.dense_specs):
            raise ValueError(f"unknown dense layer {layer}")
        W, _, _, theta = self.dense_specs[layer]
        inputs = [int(w) for w in inputs]
        if len(inputs) != W.shape[1] or any(w < 0 or w >= self.n_wires() for w in inputs):
            raise ValueError(f"dense: expected {W.shape[1]} wires defined above the node")
        head = self.gate(DENSE, len(self.dense_wires))
        self.dense_rows[len(self.gates) - 1] = (int(layer), -1)
        self.dense_wires += inputs
        for _ in range(W.shape[0] * theta - 1):
            self.gate(LUT_OUT, head)
        return [[head + m * theta + t for t in range(theta)] for m in range(W.shape[0])]

    def has_dense_nodes(self):
        """Whether the circuit holds a DENSE node (it then runs on thfhe_dag_run_dense_batch / thfhe_mk_dag_run_dense_batch)."""
        return bool(self.dense_rows)

    def dense_families(self):
        """The dense_layers, dense_words and dense_wires keyword arguments of dag_run_dense_batch: (M, K, theta, w_off, bias_off, lut_off) per layer,
        the pool of their weights, bias words and table ids laid end to end, and the pool of operand wires."""
        layers, words, off = [], [], 0
        for W, b, t, theta in self.dense_specs:
            w_off, off = off, off + W.size
            b_off = -1 if b is None else off
            off += 0 if b is None else b.size
            t_off = -1 if t is None else off
            off += 0 if t is None else t.size
            layers.append((W.shape[0], W.shape[1], theta, w_off, b_off, t_off))
            words += [W.reshape(-1)] + [a for a in (b, t) if a is not None]
        return dict(dense_layers=layers, dense_words=np.concatenate(words) if words else None, dense_wires=np.array(self.dense_wires, np.int32))

    def _dense_operands(self, gi):
        """the operand wires of the DENSE node at gate index gi"""
        off = self.gates[gi][1]
        return self.dense_wires[off:off + self.dense_specs[self.dense_rows[gi][0]][0].shape[1]]

    def has_cb_nodes(self):
        """Whether the circuit holds a CB node (it then runs on thfhe_dag_run_cb_batch)."""
        return bool(self.cb_rows)

    def cb_families(self):
        """The cb_sets and cb_wires keyword arguments of CloudKey.dag_run_cb_batch: (d, wire_off) per computed set and the pool of their wires."""
        sets, pool = [], []
        for wires in self.cb_specs:
            sets.append((len(wires), len(pool)))
            pool += wires
        return dict(cb_sets=sets, cb_wires=np.array(pool, np.int32))

    def _set_index(self, set_id):
        """The index the entry knows set `set_id` by: the client's sets first, then the computed ones."""
        return set_id if set_id < CB_SET_BASE else self.n_lhe_sets() + set_id - CB_SET_BASE

    def _set_d(self, set_id):
        """d of a computed set, None for a client set (the circuit does not know it)."""
        if set_id < CB_SET_BASE:
            return None
        if set_id - CB_SET_BASE >= len(self.cb_specs):
            raise ValueError("set id: no such computed set (cb_set)")
        return len(self.cb_specs[set_id - CB_SET_BASE])

    def has_lhe_nodes(self):
        """Whether the circuit holds an LHE_LOOKUP, LHE_GATHER or LHE_WFA node (it then runs on thfhe_dag_run_lhe_batch)."""
        return bool(self.lhe_rows)

    def n_lhe_sets(self):
        """TGSW sets the leveled nodes name: one more than the largest set id."""
        return max([k[0] + 1 for k in self.lhe_specs if k[0] < CB_SET_BASE] + [a[4] + a[5] for a in self.wfa_specs if a[4] < CB_SET_BASE] + [0])

    def lhe_families(self):
        """The leveled keyword arguments of CloudKey.dag_run_lhe_batch but the sets: lks, tab_b, tab_a, wfas, wfa_words, fin_b, fin_a.  A family with
        any encrypted row carries zero masks for its public rows."""
        def rows(store):
            if not store:
                return None, None
            enc = any(r[1] is not None for r in store)
            return np.stack([r[0] for r in store]), (np.stack([np.zeros_like(r[0]) if r[1] is None else r[1] for r in store]) if enc else None)
        wfas, words, off = [], [], 0
        for trans, step_bit, start, theta, set0, n_sets in self.wfa_specs:
            wfas.append((trans.shape[0], trans.shape[1], theta, start.shape[0], self._set_index(set0), n_sets, off, off + trans.size, off + trans.size + step_bit.size))
            words += [trans.reshape(-1), step_bit, start]
            off += trans.size + step_bit.size + start.size
        tab_b, tab_a = rows(self.lhe_tab)
        fin_b, fin_a = rows(self.lhe_fin)
        return dict(lks=[(self._set_index(k[0]),) + k[1:] for k in self.lhe_specs], tab_b=tab_b, tab_a=tab_a, wfas=wfas, wfa_words=np.concatenate(words) if words else None, fin_b=fin_b, fin_a=fin_a)

    def has_mv_nodes(self):
        """Whether the circuit holds an MV or TREE_MV node (it then runs on thfhe_dag_run_mv_batch)."""
        return bool(self.mv_rows)

    def mv_families(self):
        """(mvs, mv_tv0, mv_factors) of thfhe_dag_run_mv_batch: (lo, hi, p, q, k, base, factors_off, n_tables) per spec, the base vectors
        int32[n_bases][N] and the specs' tables laid end to end."""
        mvs, words, off = [], [], 0
        for lo, hi, p, q, k, base, tabs in self.mv_specs:
            mvs.append((lo, hi, p, q, k, base, off, len(tabs)))
            words += [t.reshape(-1) for t in tabs]
            off += len(tabs) * k * q * p
        return mvs, (np.stack(self.mv_bases) if self.mv_bases else None), (np.concatenate(words) if words else None)

    def has_luts(self):
        return bool(self.lut_rows)

    def has_tree_nodes(self):
        """Whether the circuit holds a LUT_ENC, SELECT or TREE node (it then runs on thfhe_dag_run_tree_batch)."""
        return bool(self.ext_rows)

    def nodes(self):
        """int32[n_gates][6] = (op, in0, in1, in2, spec, lut): the rows of thfhe_dag_run_lut_batch (spec = lut = -1 on gate rows); LUT_ENC, SELECT and
        TREE rows (thfhe_dag_run_tree_batch) carry (spec, etab), (tree, first), (tree, row0); MV and TREE_MV rows (thfhe_dag_run_mv_batch) (mv, t);
        LHE_LOOKUP, LHE_GATHER and LHE_WFA rows (thfhe_dag_run_lhe_batch) (lk, row0), (lk, first), (wfa, fin_row0); CB rows (thfhe_dag_run_cb_batch)
        (cbset, -1); DENSE rows (thfhe_dag_run_dense_batch) hold wire_off in the first operand field and carry (layer, -1)."""
        rows = [tuple(g) + (self.lut_rows.get(i) or self.ext_rows.get(i) or self.mv_rows.get(i) or self.cb_rows.get(i) or self.dense_rows.get(i) or self.lhe_rows.get(i, (-1, -1)))
                for i, g in enumerate(self.gates)]
        return np.array(rows, np.int32).reshape(-1, 6)

    def n_wires(self):
        return self.n_inputs + len(self.gates)

    def levels(self):
        """ASAP schedule: list of lists of gate indices; NOT costs no level (it is not bootstrapped, gates.jl:76-79).  A LUT node costs one
        level; its LUT_OUT rows join its level."""
        depth = np.zeros(self.n_wires(), np.int64)
        lv = {}
        set_depth = {}   # computed set -> the depth of its CB node: a leveled node that reads it sits above
        reads = lambda ids: max([set_depth[s] for s in ids if s >= CB_SET_BASE] + [0])
        for gi, (op, a, b, c) in enumerate(self.gates):
            if op == LUT_OUT:
                d = depth[a]
            else:
                ops = self._dense_operands(gi) if op == DENSE else (a, b, c)   # a DENSE node's first field is its slice of the wire pool
                d = max([depth[w] for w in ops if w >= 0] + [0])   # a leveled node has no wire operands
                if op == SELECT:   # its candidates count too
                    ti, first = self.ext_rows[gi]
                    d = max(d, depth[first:first + self.tree_specs[ti][2]].max())
                if op == LHE_GATHER:
                    lk, first = self.lhe_rows[gi]
                    d = max(d, depth[first:first + (1 << (self.lhe_specs[lk][1] + self.lhe_specs[lk][2]))].max())
                if op in (LHE_LOOKUP, LHE_GATHER):
                    d = max(d, reads([self.lhe_specs[self.lhe_rows[gi][0]][0]]))
                if op == LHE_WFA:
                    spec = self.wfa_specs[self.lhe_rows[gi][0]]
                    d = max(d, reads(range(spec[4], spec[4] + spec[5])))
                if op == CB:
                    d = max(depth[w] for w in self.cb_specs[self.cb_rows[gi][0]])
                    set_depth[CB_SET_BASE + self.cb_rows[gi][0]] = d + 1
                if op not in (NOT, COPY):
                    d += 1
            depth[self.n_inputs + gi] = d
            lv.setdefault((int(d), op in (NOT, COPY)), []).append(gi)
        keys = sorted(lv)  # (depth, is_not): bootstrapped gates of depth d first, then the free NOTs that read them
        return [lv[k] for k in keys]

    def census(self):
        ops = [g[0] for g in self.gates]
        boot = sum(1 for o in ops if o not in (NOT, COPY, LUT_OUT, CB) + _LHE_OPS)   # a leveled node takes no blind rotation, a CB node level-2 ones
        c = dict(gates=len(ops), bootstrapped=boot, mux=ops.count(MUX), rotations=boot + ops.count(MUX),
                 depth=len([l for l in self.levels() if self.gates[l[0]][0] not in (NOT, COPY)]))
        if self.lut_rows:
            c["luts"] = ops.count(LUT)
        if self.ext_rows:   # a TREE node: R level-1 rotations + the selection rotation
            extra = sum(self.tree_specs[self.ext_rows[i][0]][2] // self.tree_specs[self.ext_rows[i][0]][0][3] for i, o in enumerate(ops) if o == TREE)
            c.update(rotations=c["rotations"] + extra, luts_enc=ops.count(LUT_ENC), selects=ops.count(SELECT), trees=ops.count(TREE))
        if self.mv_rows:    # a TREE_MV node: one multi-value rotation + k selection rotations
            extra = sum(self.mv_specs[self.mv_rows[i][0]][4] for i, o in enumerate(ops) if o == TREE_MV)
            c.update(rotations=c["rotations"] + extra, mvs=ops.count(MV), tree_mvs=ops.count(TREE_MV))
        if self.lhe_rows:
            c.update(lhe_lookups=ops.count(LHE_LOOKUP), lhe_gathers=ops.count(LHE_GATHER), lhe_wfas=ops.count(LHE_WFA))
        if self.cb_rows:
            c.update(cbs=ops.count(CB), cb_bits=sum(len(w) for w in self.cb_specs))
        if self.dense_rows:   # a DENSE node: one rotation per output
            extra = sum(self.dense_specs[l][0].shape[0] - 1 for l, _ in self.dense_rows.values())
            c.update(rotations=c["rotations"] + extra, denses=ops.count(DENSE))
        return c


# ---- the reference's building blocks (src/KNN_medical_data.cpp) ---------------------------------------------------
def ones_comp(cir, all_one, x):
    """onesComp, :127-132."""
    return [cir.gate(XOR, all_one[i], x[i]) for i in range(len(x))]


def full_adder(cir, a, b, carry_in):
    """FullAdder, :134-157 (same wiring as src/bootstrap_modules.cpp:20-44).  Returns (sum, carry) MSB-first; carry[nb-1] = carry_in."""
    nb = len(a)
    sum2 = [None] * nb
    carry = [None] * nb
    carry[nb - 1] = carry_in
    for i in range(nb - 1, -1, -1):
        s1 = cir.gate(XOR, a[i], b[i])
        c1 = cir.gate(AND, a[i], b[i])
        sum2[i] = cir.gate(XOR, s1, carry[i])
        c2 = cir.gate(AND, s1, carry[i])
        if i != 0:
            carry[i - 1] = cir.gate(OR, c1, c2)
    return sum2, carry


def difference(cir, x, y, all_one, lsb_one, zero):
    """difference = x - y via two's complement, :161-213."""
    ones = ones_comp(cir, all_one, y)
    twos, _ = full_adder(cir, ones, lsb_one, zero)
    diff, _ = full_adder(cir, x, twos, zero)
    return diff


def distance(cir, x, y, all_one, lsb_one, zero):
    """|x - y|: dist[i] = MUX(d1[0], d2[i], d1[i]), :217-236."""
    d1 = difference(cir, x, y, all_one, lsb_one, zero)
    d2 = difference(cir, y, x, all_one, lsb_one, zero)
    return [cir.gate(MUX, d1[0], d2[i], d1[i]) for i in range(len(x))]


def distance_bw_data(cir, row_a, row_b, all_zero, all_one, lsb_one, zero):
    """Manhattan distance of two records, columns 1..end, :239-263."""
    result = list(all_zero)
    for col in range(1, len(row_a)):
        dist = distance(cir, row_a[col], row_b[col], all_one, lsb_one, zero)
        result, _ = full_adder(cir, result, dist, zero)
    return result


def copy_through_mux(cir, all_one, x):
    """The reference copies a word with bootsMUX(allOne[l], x[l], x[l]), :685-689 (a bootstrapped refresh)."""
    return [cir.gate(MUX, all_one[i], x[i], x[i]) for i in range(len(x))]


def compare_swap(cir, key_a, key_b, payload_a, payload_b, all_zero, all_one, lsb_one, zero):
    """One step of sort_with_distance, :443-481: diff = key_a - key_b; its sign bit routes the smaller key (and its
    payload words) to position a and the bigger to position b through MUXes; every routed bit is then refreshed with
    XOR(., allZero).  Returns (key_a', key_b', payload_a', payload_b')."""
    diff = difference(cir, key_a, key_b, all_one, lsb_one, zero)
    s = diff[0]
    nb = len(key_a)
    big = [cir.gate(MUX, s, key_b[j], key_a[j]) for j in range(nb)]
    small = [cir.gate(MUX, s, key_a[j], key_b[j]) for j in range(nb)]
    pay_big = [[cir.gate(MUX, s, wb[j], wa[j]) for j in range(nb)] for wa, wb in zip(payload_a, payload_b)]
    pay_small = [[cir.gate(MUX, s, wa[j], wb[j]) for j in range(nb)] for wa, wb in zip(payload_a, payload_b)]
    refresh = lambda w: [cir.gate(XOR, w[j], all_zero[j]) for j in range(nb)]
    return refresh(small), refresh(big), [refresh(w) for w in pay_small], [refresh(w) for w in pay_big]


def sort_with_distance(cir, rows, dists, all_zero, all_one, lsb_one, zero):
    """sort_with_distance, :410-489: n passes of adjacent compare-swaps (bubble sort) on the distances, the train records
    moving with them.  rows[i] = list of words, dists[i] = word.  Returns (rows, dists) sorted by ascending distance."""
    rows, dists = [list(r) for r in rows], list(dists)
    n = len(dists)
    for _ in range(n):
        for i in range(1, n):
            dists[i - 1], dists[i], rows[i - 1], rows[i] = compare_swap(cir, dists[i - 1], dists[i], rows[i - 1], rows[i],
                                                                        all_zero, all_one, lsb_one, zero)
    return rows, dists


def knn_classify(cir, test_row, train_rows, threshold, all_zero, all_one, lsb_one, lsb_zero_carry, zero, K=None):
    """The reference's KNN decision for one test record, :676-732: Manhattan distances to every train row (columns
    1..col_size-2), a MUX copy of the train rows, sort by distance, count = sum of the label column of the K nearest,
    decision = XOR(sign(threshold - count), 0).  Returns (decision_wire, count_word, sorted_dists)."""
    ncol = len(test_row)
    n = len(train_rows)
    K = n if K is None else K
    dists = [distance_bw_data(cir, test_row[:ncol - 1], tr[:ncol - 1], all_zero, all_one, lsb_one, zero) for tr in train_rows]
    copies = [[copy_through_mux(cir, all_one, w) for w in tr] for tr in train_rows]
    srows, sdists = sort_with_distance(cir, copies, dists, all_zero, all_one, lsb_one, zero)
    count = list(all_zero)
    for j in range(K):
        count, _ = full_adder(cir, count, srows[j][ncol - 1], lsb_zero_carry)
    diff = difference(cir, threshold, count, all_one, lsb_one, zero)
    return cir.gate(XOR, diff[0], all_zero[0]), count, sdists


# ---- the KNN decision sharded over ranks (BASELINE.json configs[3]; src/KNN_medical_data.cpp:676-732) ------------------------------
class KnnPlan:
    """The reference's KNN decision for one test record, cut the way its `#pragma omp parallel for` over train rows (:681-691) cuts it:
      phase 1  per train row: distance_bw_data to the test record + the MUX copy of the row -- independent rows, sharded over ranks;
      phase 2  sort_with_distance, vote over the label column of the K = n_train nearest, decision bit -- one sequential chain,
               evaluated by every rank on the gathered rows (replicated keys; 855 of its levels hold 1-3 gates, nothing to shard).
    Inputs (MSB-first bit records): the test record, the train rows, and the constants (threshold, allZero, allOne, lsbOne, zero).
    One rank (world = 1) evaluates the very same two DAGs, so the sharded result equals the single-rank result bit for bit."""

    def __init__(self, nb, ncol, ntrain):
        self.nb, self.ncol, self.ntrain = nb, ncol, ntrain

    def phase1(self, n_rows):
        """DAG for n_rows train rows: inputs = test[ncol], rows[n_rows][ncol], allZero, allOne, lsbOne, zero."""
        c = Circuit()
        test = [c.inputs(self.nb) for _ in range(self.ncol)]
        rows = [[c.inputs(self.nb) for _ in range(self.ncol)] for _ in range(n_rows)]
        all_zero, all_one, lsb_one = c.inputs(self.nb), c.inputs(self.nb), c.inputs(self.nb)
        zero = c.inputs(1)[0]
        dist = [distance_bw_data(c, test[:self.ncol - 1], r[:self.ncol - 1], all_zero, all_one, lsb_one, zero) for r in rows]
        copies = [[copy_through_mux(c, all_one, w) for w in r] for r in rows]
        return c, dist, copies

    def phase1_distances(self, n_rows):
        """phase1 without the MUX copies (they do not depend on the test record): inputs as phase1."""
        c = Circuit()
        test = [c.inputs(self.nb) for _ in range(self.ncol)]
        rows = [[c.inputs(self.nb) for _ in range(self.ncol)] for _ in range(n_rows)]
        all_zero, all_one, lsb_one = c.inputs(self.nb), c.inputs(self.nb), c.inputs(self.nb)
        zero = c.inputs(1)[0]
        dist = [distance_bw_data(c, test[:self.ncol - 1], r[:self.ncol - 1], all_zero, all_one, lsb_one, zero) for r in rows]
        return c, dist

    def copies(self, n_rows):
        """The MUX copy of the train rows alone (src/KNN_medical_data.cpp:685-689): inputs = rows[n_rows][ncol], allOne."""
        c = Circuit()
        rows = [[c.inputs(self.nb) for _ in range(self.ncol)] for _ in range(n_rows)]
        all_one = c.inputs(self.nb)
        return c, [[copy_through_mux(c, all_one, w) for w in r] for r in rows]

    def phase2(self):
        """DAG on the gathered rows: inputs = rows[ntrain][ncol], dists[ntrain], threshold, allZero, allOne, lsbOne, zero."""
        c = Circuit()
        rows = [[c.inputs(self.nb) for _ in range(self.ncol)] for _ in range(self.ntrain)]
        dists = [c.inputs(self.nb) for _ in range(self.ntrain)]
        thr, all_zero, all_one, lsb_one = (c.inputs(self.nb) for _ in range(4))
        zero = c.inputs(1)[0]
        srows, sdists = sort_with_distance(c, rows, dists, all_zero, all_one, lsb_one, zero)
        count = list(all_zero)
        for j in range(self.ntrain):
            count, _ = full_adder(c, count, srows[j][self.ncol - 1], zero)
        diff = difference(c, thr, count, all_one, lsb_one, zero)
        decision = c.gate(XOR, diff[0], all_zero[0])
        return c, decision, count, sdists, srows


def knn_decision_sharded(ck, plan, test, train, threshold, all_zero, all_one, lsb_one, zero, rank=0, world=1, all_reduce=None, stats=None):
    """Evaluate the KNN decision with the train rows of phase 1 dealt round-robin over `world` ranks (every rank holds the keys).
    test: int32[ncol][nb][words]; train: int32[ntrain][ncol][nb][words]; threshold / all_zero / all_one / lsb_one: int32[nb][words];
    zero: int32[words].  all_reduce(np.ndarray) -> np.ndarray sums an int32 array over the ranks (torch.distributed all_reduce over
    RCCL or gloo; every row is produced by exactly one rank, so the sum IS the gather); None is allowed only for world = 1.
    Returns dict(decision=record, count=records[nb], sorted_dists=records[ntrain][nb], dists=records[ntrain][nb])."""
    nb, ncol, ntrain = plan.nb, plan.ncol, plan.ntrain
    words = ck.words
    test = np.asarray(test, np.int32).reshape(ncol, nb, words)
    train = np.asarray(train, np.int32).reshape(ntrain, ncol, nb, words)
    consts = [np.asarray(v, np.int32).reshape(nb, words) for v in (all_zero, all_one, lsb_one)]
    zero = np.asarray(zero, np.int32).reshape(1, words)
    mine = [j for j in range(ntrain) if j % world == rank]
    gathered = np.zeros((ntrain, ncol + 1, nb, words), np.int32)   # [row][its ncol words, then its distance]
    st1 = {}
    if mine:
        c1, dist, copies = plan.phase1(len(mine))
        in1 = np.concatenate([test.reshape(-1, words), train[mine].reshape(-1, words)] + consts + [zero])
        _t = time.perf_counter()
        v1 = evaluate(ck, c1, in1, st1)
        st1["seconds"] = st1.get("seconds", 0.0) + time.perf_counter() - _t
        for q, j in enumerate(mine):
            for col in range(ncol):
                gathered[j, col] = v1[copies[q][col]]
            gathered[j, ncol] = v1[dist[q]]
    if world > 1:
        if all_reduce is None:
            raise ValueError("knn_decision_sharded: world > 1 needs an all_reduce callable")
        gathered = np.asarray(all_reduce(gathered), np.int32).reshape(gathered.shape)
    c2, decision, count, sdists, _ = plan.phase2()
    thr = np.asarray(threshold, np.int32).reshape(nb, words)
    in2 = np.concatenate([gathered[:, :ncol].reshape(-1, words), gathered[:, ncol].reshape(-1, words), thr] + consts + [zero])
    st2 = {}
    _t = time.perf_counter()
    v2 = evaluate(ck, c2, in2, st2)
    st2["seconds"] = time.perf_counter() - _t
    if stats is not None:
        stats.update(phase1=st1, phase2=st2, my_rows=mine)
    return dict(decision=v2[decision], count=v2[count], sorted_dists=np.stack([v2[w] for w in sdists]), dists=gathered[:, ncol])


def knn_decisions_batched(ck, plan, tests, train, threshold, all_zero, all_one, lsb_one, zero, rank=0, world=1, all_reduce=None, stats=None):
    """The reference's loop over test records (`for i < test_row_size`, src/KNN_medical_data.cpp:676-691) as ONE batched evaluation:
    every test record is an instance of the same two DAGs (KnnPlan.phase1 over all train rows, KnnPlan.phase2) and the instances walk
    the levels side by side (dag_run_batch), so that the 879 levels of the sort / vote chain that hold 1-3 gates per decision hold
    Q-3Q gates per launch.  Sharding is BY QUERY: rank r evaluates the test records q with q % world == r, both phases, with no
    exchange in between; one all_reduce at the end gathers the results (every record is produced by exactly one rank, so the sum is
    the gather).  Gates are deterministic, so record q's result equals knn_decision_sharded on tests[q] bit for bit.
    tests: int32[Q][ncol][nb][words]; the other arguments as in knn_decision_sharded.
    Returns dict(decision=[Q][words], count=[Q][nb][words], sorted_dists=[Q][ntrain][nb][words], dists=[Q][ntrain][nb][words])."""
    nb, ncol, ntrain = plan.nb, plan.ncol, plan.ntrain
    words = ck.words
    tests = np.asarray(tests, np.int32)
    tests = tests.reshape(-1, ncol, nb, words)
    Q = tests.shape[0]
    train = np.asarray(train, np.int32).reshape(ntrain, ncol, nb, words)
    consts = [np.asarray(v, np.int32).reshape(nb, words) for v in (all_zero, all_one, lsb_one)]
    zero = np.asarray(zero, np.int32).reshape(1, words)
    thr = np.asarray(threshold, np.int32).reshape(nb, words)
    mine = [q for q in range(Q) if q % world == rank]
    per = 1 + nb + 2 * ntrain * nb                       # decision | count | sorted distances | distances
    result = np.zeros((Q, per, words), np.int32)
    st1, st2 = {}, {}
    if mine:
        # the MUX copies of the train rows (:685-689) do not depend on the test record and a bootstrapped gate is a deterministic function of its
        # operands: evaluated ONCE per rank, they are the very ciphertexts the reference recomputes for every test record (3.6 % of its rotations)
        cc, copy_w = plan.copies(ntrain)
        stc = {}
        _t = time.perf_counter()
        oc = evaluate_batch(ck, cc, np.concatenate([train.reshape(-1, words), consts[1]])[None], [w for r in copy_w for col in r for w in col], stc)[0]
        c1, dist = plan.phase1_distances(ntrain)
        shared = np.concatenate([train.reshape(-1, words)] + consts + [zero])
        in1 = np.stack([np.concatenate([tests[q].reshape(-1, words), shared]) for q in mine])
        od = evaluate_batch(ck, c1, in1, [w for r in range(ntrain) for w in dist[r]], st1)
        st1["rotations"] = st1.get("rotations", 0) + stc.get("rotations", 0)
        st1["copies_once"] = dict(rotations=stc.get("rotations"), launches=stc.get("launches"))
        st1["seconds"] = time.perf_counter() - _t
        o1 = np.concatenate([np.broadcast_to(oc, (len(mine),) + oc.shape), od], axis=1)   # rows' copies | distances, the layout of phase 2's inputs
        del in1
        c2, decision, count, sdists, _ = plan.phase2()
        tail = np.concatenate([thr] + consts + [zero])
        in2 = np.concatenate([o1, np.broadcast_to(tail, (len(mine),) + tail.shape)], axis=1)   # rows, dists | thr, constants, zero
        sel2 = [decision] + list(count) + [w for d in sdists for w in d]
        _t = time.perf_counter()
        o2 = evaluate_batch(ck, c2, in2, sel2, st2)
        st2["seconds"] = time.perf_counter() - _t
        result[mine, :1 + nb + ntrain * nb] = o2
        result[mine, 1 + nb + ntrain * nb:] = o1[:, ntrain * ncol * nb:]
    if world > 1:
        if all_reduce is None:
            raise ValueError("knn_decisions_batched: world > 1 needs an all_reduce callable")
        result = np.asarray(all_reduce(result), np.int32).reshape(result.shape)
    if stats is not None:
        stats.update(phase1=st1, phase2=st2, my_queries=mine)
    a, b = 1 + nb, 1 + nb + ntrain * nb
    return dict(decision=result[:, 0], count=result[:, 1:a], sorted_dists=result[:, a:b].reshape(Q, ntrain, nb, words),
                dists=result[:, b:].reshape(Q, ntrain, nb, words))


def torch_all_reduce(device=None):
    """all_reduce callable for knn_decision_sharded over torch.distributed (backend nccl = RCCL: pass the rank's cuda device)."""
    import torch
    import torch.distributed as dist

    def f(a):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if device is not None:
            t = t.to(device)
        dist.all_reduce(t)
        return t.cpu().numpy()
    return f


# ---- the reference's multi-key integer circuits (3gen_mk_gates.jl; bit vectors LSB-first, mk_api.jl:563-576) ----------
def mk_add_3gen(cir, a, b, cin):
    """mk_add_3gen / mk_add_3gen_v2, 3gen_mk_gates.jl:183-220."""
    out = []
    for i in range(len(a)):
        t1 = cir.gate(XOR, a[i], b[i])
        t2 = cir.gate(AND, a[i], b[i])
        out.append(cir.gate(XOR, t1, cin))
        t3 = cir.gate(AND, t1, cin)
        cin = cir.gate(OR, t2, t3)
    return out


def mk_inv_3gen(cir, a, one):
    """:223-233."""
    return [cir.gate(XOR, x, one) for x in a]


def mk_sub_3gen(cir, a, b, one):
    """a - b = a + ~b + 1, :236-244."""
    return mk_add_3gen(cir, a, mk_inv_3gen(cir, b, one), one)


def mk_less_3gen(cir, a, b, one):
    """sign bit of a - b, :247-255."""
    return mk_sub_3gen(cir, a, b, one)[-1]


def mk_grt_3gen(cir, a, b, one):
    """a > b: sign bit of b - a, copied, :258-266."""
    return cir.gate(COPY, mk_sub_3gen(cir, b, a, one)[-1])


def mk_leq_3gen(cir, a, b, one):
    """:269-277."""
    return cir.gate(XOR, mk_grt_3gen(cir, a, b, one), one)


def mk_geq_3gen(cir, a, b, one):
    """:280-288."""
    return cir.gate(XOR, mk_less_3gen(cir, a, b, one), one)


def mk_int_add_with_carry_3gen(cir, a, b, cin):
    """WIDTH sum bits + the carry out, :291-310."""
    out = []
    for i in range(len(a)):
        t1 = cir.gate(XOR, a[i], b[i])
        t2 = cir.gate(AND, a[i], b[i])
        out.append(cir.gate(XOR, t1, cin))
        t3 = cir.gate(AND, t1, cin)
        cin = cir.gate(OR, t2, t3)
    return out + [cin]


def mk_int_mul_3gen(cir, a, b, zero):
    """Shift-and-add multiplier, low WIDTH bits, :312-362 -- the reference's dataflow verbatim, including its last addition of
    partial-product row `ctr` (= WIDTH-1, not WIDTH) and its mk_copy_3gen refreshes."""
    W = len(a)
    cp = lambda w: cir.gate(COPY, w)
    BArr = [[cir.gate(AND, a[j], b[i]) for j in range(W)] for i in range(W)]
    result = [None] * (2 * W + 1)
    result[0] = cp(BArr[0][0])
    tmp_in = [cp(BArr[0][i + 1]) for i in range(W - 1)] + [cp(zero)]
    ctr = 1
    for i in range(2, W):                      # Julia i = 2 .. WIDTH-1 (1-based row i)
        t = mk_int_add_with_carry_3gen(cir, tmp_in, BArr[i - 1], zero)
        result[i - 1] = cp(t[0])
        tmp_in = [cp(t[j + 1]) for j in range(W)]
        ctr = i
    t = mk_int_add_with_carry_3gen(cir, tmp_in, BArr[ctr - 1], zero)
    for i in range(W + 1):
        result[i + ctr] = cp(t[i])
    return [cp(result[i]) for i in range(W)]


# ---- integer arithmetic from LUT nodes -------------------------------------------------------------------------------------
# Integer bits use the padding-bit encoding of thfhe.lut at p = 4 (bit m = m * 2^32 / 8); gate bits are the gates' +-1/8.  Tables are built
# for the ring of degree N, Torus32 (single key) or torus_bits=64 (3-gen multi-key), unless a table id is given.
def adder_table(N=1024, torus_bits=32):
    """theta = 2 test vector of a full-adder bit at p = 4: output 0 = parity (sum), output 1 = majority (carry) of a + b + c."""
    from . import lut
    return lut.test_vector([lut.int_outputs(lambda m: m & 1, 4, torus_bits=torus_bits), lut.int_outputs(lambda m: m >= 2, 4, torus_bits=torus_bits)],
                           4, theta=2, N=N, torus_bits=torus_bits)


def lut_ripple_add(cir, a_bits, b_bits, table_id=None, carry_in=None, N=1024, torus_bits=32):
    """a + b on LSB-first p = 4 integer bits: one theta = 2 LUT node per bit (the node of bit i reads a_i, b_i and the carry of bit i-1).
    Returns (sum bits LSB-first, carry out).  table_id: an adder_table registered in cir (None: registered here)."""
    if table_id is None:
        table_id = cir.table(adder_table(N, torus_bits))
    carry, sums = carry_in, []
    for a, b in zip(a_bits, b_bits):
        if carry is None:
            s, carry = cir.lut(table_id, [a, b], weights=(1, 1), theta=2)
        else:
            s, carry = cir.lut(table_id, [a, b, carry], weights=(1, 1, 1), theta=2)
        sums.append(s)
    return sums, carry


def from_gate_bit(cir, w, table_id=None, N=1024, torus_bits=32):
    """Gate bit (+-1/8) -> p = 4 integer bit, one theta = 1 LUT node: with weight 1 and bias +1/8 the gate bit is the p = 2 message 0 or 1."""
    from . import lut
    if table_id is None:
        table_id = cir.table(lut.test_vector(lut.int_outputs(lambda m: m, 4, p=2, torus_bits=torus_bits), 2, N=N, torus_bits=torus_bits))
    return cir.lut(table_id, [w], weights=(1,), bias=1 << 29)[0]


def to_gate_bit(cir, w, table_id=None, N=1024, torus_bits=32):
    """p = 4 integer bit -> gate bit (+-1/8 on Torus32; the 3-gen gates read the same Torus32 records), one theta = 1 LUT node."""
    from . import lut
    if table_id is None:
        table_id = cir.table(lut.test_vector(lut.bool_outputs(lambda m: m & 1, 4, torus_bits=torus_bits), 4, N=N, torus_bits=torus_bits))
    return cir.lut(table_id, [w])[0]


def tree_mul_digits(cir, a, b, N=1024, torus_bits=32):
    """The product of two 3-bit digits (p = 8 wires a, b) as its low and high 3-bit digits: two TREE nodes with p_hi = p_lo = p_out = 8 and
    theta1 = 2 (4 + 1 rotations each; a shape of DESIGN 4.11's supported set), a on the level-1 digit, b on the selection digit.  Returns (low, high).
    torus_bits=64 with the context's N: int64 rows for the 3-gen multi-key engine."""
    from . import lut
    lo_rows = cir.tree_rows(lut.tree_test_vectors(lambda h, l: (h * l) % 8, 8, 8, 8, theta=2, N=N, torus_bits=torus_bits))
    hi_rows = cir.tree_rows(lut.tree_test_vectors(lambda h, l: (h * l) // 8, 8, 8, 8, theta=2, N=N, torus_bits=torus_bits))
    return cir.tree(lo_rows, [a], [b], 8, theta1=2), cir.tree(hi_rows, [a], [b], 8, theta1=2)


def sbox_digits(cir, hi, lo, table, N=1024, torus_bits=32):
    """A 64-entry table of 4-bit values (a DES S-box: table[8 hi + lo]) on two p = 8 digit wires, as its four bits LSB-first in the p_out = 2 encoding
    of thfhe.lut: ONE TREE_MV node with k = 4, p_hi = p_lo = 8 (1 + 4 rotations; bit-valued outputs, the shape DESIGN 4.13's noise table supports on
    the named parameter sets).  Returns the four bit wires.  torus_bits=64 with the context's N: the Torus64 base vector of the 3-gen multi-key engine."""
    from . import lut
    table = [int(v) for v in table]
    if len(table) != 64 or any(not 0 <= v < 16 for v in table):
        raise ValueError("sbox_digits: expected 64 values in 0 .. 15")
    tv0, w = lut.tree_mvk_factors([lambda h, l, j=j: (table[8 * h + l] >> j) & 1 for j in range(4)], 8, 8, 2, N=N, torus_bits=torus_bits)
    return cir.tree_mv(cir.mv_base(tv0), w, [lo], [hi])


def lhe_sbox(ck, tset, table, p_out=8):
    """A 16-bit -> 4-bit S-box by leveled lookup (thfhe_lhe_lookup), not a circuit of gates: `table` holds 2^16 integers in [0, 16), `tset`
    the TGSW samples of the 16 address bits of every sample (CloudKey.tgsw_set, d = 16).  A 16-bit address needs (d_tree, d_rot) = (6, 10), where
    box = N >> 10 = 1 leaves room for ONE function per polynomial, so theta = 4 does not fit; the four output bits are four lookups at (6, 10, 1) on
    the same set, 4 x 73 CMuxes per sample (about half a bootstrap).  The other layout the issue of four functions allows, theta = 4 at d_rot = 8,
    serves 14-bit addresses only.  Returns int32[count, 4, n+1]: record j of a sample is bit j of its entry at modulus p_out (thfhe.lut.encode)."""
    from . import lut
    t = np.asarray(table, np.int64).reshape(-1)
    if t.shape[0] != 1 << 16 or np.any((t < 0) | (t > 15)):
        raise ValueError("table: expected 2^16 integers in [0, 16)")
    if tset.d != 16:
        raise ValueError("tset: expected 16 address bits per sample")
    outs = [ck.lhe_lookup(tset, lut.lhe_table((t >> j) & 1, 6, 10, encode=lambda v: lut.encode(v, p_out)), d_tree=6, d_rot=10)[:, 0] for j in range(4)]
    return np.stack(outs, axis=1)


def cb_lookup(ck, a_recs, b_recs, table, p_out=8, one_rotation=False):
    """A table read at an address the circuit computed (circuit bootstrapping): a_recs, b_recs int32[count * d][n+1] hold the gate-encoded
    bits of two d-bit numbers per sample (sample-major, low bit first; d = log2(len(table)), 1 <= d <= 10), the address is a XOR b -- d XOR gates
    per sample --, CloudKey.circuit_bootstrap turns the gate outputs into TGSW address bits and lhe_lookup reads `table` (integers in [0, p_out)) with
    d CMuxes.  `ck` holds a circuit-bootstrap key (cb_key_set).  one_rotation: CloudKey.circuit_bootstrap's (the XOR outputs are gate-encoded, as
    it needs).  Returns int32[count, n+1]: the entry at modulus p_out (thfhe.lut.encode)."""
    from . import lut
    t = np.asarray(table, np.int64).reshape(-1)
    d = t.shape[0].bit_length() - 1
    if not 1 <= d <= 10 or t.shape[0] != 1 << d or np.any((t < 0) | (t >= p_out)):
        raise ValueError("table: expected 2^d integers in [0, p_out), 1 <= d <= 10")
    addr = ck.gates(XOR, a_recs, b_recs)
    with ck.circuit_bootstrap(addr, d, one_rotation=one_rotation) as tset:
        return ck.lhe_lookup(tset, lut.lhe_table(t, 0, d, encode=lambda v: lut.encode(v, p_out)), d_tree=0, d_rot=d)[:, 0]


def cb_lookup_plain(a, b, table):
    """The plain-integer twin of cb_lookup: table[a XOR b]."""
    return np.asarray(table, np.int64).reshape(-1)[np.asarray(a, np.int64) ^ np.asarray(b, np.int64)]


def lhe_histogram(ck, tset, p_out, d_tree, d_rot):
    """A histogram of encrypted addresses by leveled scatter (thfhe_lhe_scatter): every sample of `tset` adds the trivial value
    2^32 / (2 p_out) -- the message 1 at modulus p_out (thfhe.lut.encode) -- at its address, so entry e of the returned table (tab_a, tab_b)
    int32[1][2^d_tree][N] encrypts the number of samples whose address is e: decrypt with lut.decode(lut.lhe_table_entries(phases, d_tree, d_rot), p_out).
    Counts must stay below p_out, and the noise of an entry grows with the number of samples, hit or not (DESIGN 4.17 tabulates it)."""
    from . import lut
    one = lut.lhe_value([1], encode=lambda v: lut.encode(v, p_out), N=ck.params.N)
    return ck.lhe_scatter(tset, one, d_tree=d_tree, d_rot=d_rot)


def lhe_scatter_plain(addresses, values, d_tree, d_rot, val_index=None, n_tables=1, table_index=None, N=1024):
    """The plain model of thfhe_lhe_scatter: int32[n_tables][2^d_tree][N], the table polynomials after sample s has added X^((a mod 2^d_rot) box)
    times its value polynomial -- values int[n_vals][N] words, value val_index[s], or value s when n_vals == len(addresses), or the one value --
    into polynomial a >> d_rot of table table_index[s] (None: table 0), a = addresses[s], box = N >> d_rot; sums mod 2^32."""
    addr = np.asarray(addresses, np.int64).reshape(-1)
    vals = np.asarray(values, np.int64).reshape(-1, N)
    if not (0 <= d_tree <= 6 and 0 <= d_rot <= 10) or np.any((addr < 0) | (addr >= 1 << (d_tree + d_rot))):
        raise ValueError("d_tree must be 0 .. 6, d_rot 0 .. 10 and the addresses in [0, 2^(d_tree + d_rot))")
    if val_index is None:
        if vals.shape[0] not in (1, addr.shape[0]):
            raise ValueError("without val_index there must be one value or one per address")
        val_index = np.arange(addr.shape[0]) if vals.shape[0] > 1 else np.zeros(addr.shape[0], np.int64)
    table_index = np.zeros(addr.shape[0], np.int64) if table_index is None else np.asarray(table_index, np.int64).reshape(-1)
    box = N >> d_rot
    tab = np.zeros((n_tables, 1 << d_tree, N), np.int64)
    for a, vi, ti in zip(addr, np.asarray(val_index, np.int64).reshape(-1), table_index):
        shift = int(a & ((1 << d_rot) - 1)) * box
        v = vals[vi]
        tab[ti, a >> d_rot] += np.concatenate([-v[N - shift:], v[:N - shift]])   # X^shift v mod X^N + 1
    return (tab & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


# ---- layered automata for thfhe_lhe_wfa ------------------------------------------------------------------------------------------
# An automaton is (trans int32[n_steps][n_states][2], step_bit int32[n_steps], finals int[1][n_states], start int32[n_out]): step j reads bit
# step_bit[j] & 15 of TGSW set step_bit[j] >> 4 and moves state q to trans[j][q][bit]; the output is finals[:, state after the last step].  Sets hold
# at most 16 bits, so the operands are dealt over sets in 16-bit chunks (wfa_pair_bits, wfa_text_bits).

def wfa_pair_bits(a, b, width):
    """The bits of two `width`-bit operands per sample in the layout of wfa_less_than / wfa_equal: chunk c (bits 16c .. 16c+15) of a is set 2c,
    of b set 2c+1 -> a list of int32[count][bits of the chunk], low bit first (each goes through SecretKeySet.tgsw_encrypt to CloudKey.tgsw_set)."""
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    if not 1 <= width <= 62 or a.shape != b.shape or np.any((a < 0) | (a >> width != 0) | (b < 0) | (b >> width != 0)):
        raise ValueError(f"expected two arrays of one length with values in [0, 2^{width}), 1 <= width <= 62")
    sets = []
    for lo in range(0, width, 16):
        d = min(16, width - lo)
        for v in (a, b):
            sets.append((((v >> lo)[:, None] >> np.arange(d)[None, :]) & 1).astype(np.int32))
    return sets


def wfa_text_bits(bits):
    """The bits int[count][n] of a text in the layout of wfa_match: bit i is bit i % 16 of set i // 16 -> a list of int32[count][<= 16]."""
    t = np.asarray(bits, np.int32)
    t = t[None] if t.ndim == 1 else t
    return [np.ascontiguousarray(t[:, lo:lo + 16]) for lo in range(0, t.shape[1], 16)]


def _wfa_pair_steps(width):
    bit = lambda operand, i: 16 * (2 * (i // 16) + operand) + i % 16
    return np.array([bit(j & 1, j >> 1) for j in range(2 * width)], np.int32)


def wfa_less_than(width):
    """a < b for two `width`-bit numbers (wfa_pair_bits), low bit first: 2 width steps, 4 states.  Even steps read a_i in state lt (0 / 1) and
    move to 2 lt + a_i; odd steps read b_i: lt' = 1 if a_i < b_i, 0 if a_i > b_i, else lt -- half of the odd steps' states are copies.
    finals: 1 in state 1."""
    if not 1 <= width <= 62:
        raise ValueError("1 <= width <= 62")
    even = [[0, 1], [2, 3], [2, 2], [3, 3]]              # states 2, 3 are not reached at an even step
    odd = [[0, 1], [0, 0], [1, 1], [0, 1]]               # (lt, a_i) = (0, 0), (0, 1), (1, 0), (1, 1)
    trans = np.array([even, odd] * width, np.int32)
    return trans, _wfa_pair_steps(width), np.array([[0, 1, 0, 0]]), np.array([0], np.int32)


def wfa_equal(width):
    """a == b for two `width`-bit numbers (wfa_pair_bits): 2 width steps, 4 states -- 0 equal so far, 1 different (absorbing: copies), 2 + a_i
    after an even step.  finals: 1 in state 0."""
    if not 1 <= width <= 62:
        raise ValueError("1 <= width <= 62")
    even = [[2, 3], [1, 1], [2, 2], [3, 3]]
    odd = [[0, 0], [1, 1], [0, 1], [1, 0]]
    trans = np.array([even, odd] * width, np.int32)
    return trans, _wfa_pair_steps(width), np.array([[1, 0, 0, 0]]), np.array([0], np.int32)


def wfa_match(pattern_bits, text_bits=None):
    """Does the public bit pattern occur in an encrypted text of text_bits bits (wfa_text_bits; default: the pattern's length, i.e. equality with
    the pattern)?  The Knuth-Morris-Pratt automaton: state q = length of the longest prefix of the pattern that ends here, state m = found
    (absorbing); m + 1 <= 64 states, one step per text bit.  finals: 1 in state m."""
    pat = [int(v) for v in np.asarray(pattern_bits).reshape(-1)]
    m = len(pat)
    n = m if text_bits is None else int(text_bits)
    if not 1 <= m <= 63 or any(v not in (0, 1) for v in pat) or not m <= n <= 4096:
        raise ValueError("expected 1 .. 63 pattern bits in {0, 1} and len(pattern) <= text_bits <= 4096")
    delta = np.zeros((m + 1, 2), np.int32)
    for q in range(m):
        for b in (0, 1):
            seen = pat[:q] + [b]
            k = min(m, q + 1)
            while k and seen[len(seen) - k:] != pat[:k]:
                k -= 1
            delta[q, b] = k
    delta[m] = m
    trans = np.repeat(delta[None], n, axis=0)
    step_bit = np.array([16 * (i // 16) + i % 16 for i in range(n)], np.int32)
    fin = np.zeros((1, m + 1), np.int64)
    fin[0, m] = 1
    return trans, step_bit, fin, np.array([0], np.int32)


def wfa_run_plain(automaton, bits):
    """The automaton on plain bits: bits is the list of sets (int[count][d] each, as wfa_pair_bits / wfa_text_bits return them) -> int[count][n_out]
    [theta], finals[:, state] of the state each start state ends in."""
    trans, step_bit, finals, start = automaton
    trans, finals = np.asarray(trans), np.asarray(finals)
    sets = [np.asarray(b).reshape(len(b), -1) for b in bits]
    count = sets[0].shape[0]
    state = np.tile(np.asarray(start, np.int64)[None], (count, 1))
    for j, sb in enumerate(np.asarray(step_bit)):
        b = sets[sb >> 4][:, sb & 15]
        state = trans[j][state, b[:, None]]
    return np.moveaxis(finals[:, state], 0, -1)


def wfa_noise_steps(automaton, bits):
    """Non-copy steps on the path of every (sample, output): the CMuxes whose noise the output carries -> int[count][n_out]."""
    trans, step_bit, finals, start = automaton
    trans = np.asarray(trans)
    sets = [np.asarray(b).reshape(len(b), -1) for b in bits]
    state = np.tile(np.asarray(start, np.int64)[None], (sets[0].shape[0], 1))
    steps = np.zeros_like(state)
    for j, sb in enumerate(np.asarray(step_bit)):
        steps += trans[j][state, 0] != trans[j][state, 1]
        state = trans[j][state, sets[sb >> 4][:, sb & 15][:, None]]
    return steps


# ---- leveled nodes among gates ---------------------------------------------------------------------------------------------------
def lhe_array_read(cir, wires, set_id, d_tree, d_rot):
    """Read an array of computed wires at the client's index: wires[addr] for the address the instance's sample of TGSW set `set_id` encrypts
    (d_tree + d_rot bits, len(wires) = 2^(d_tree + d_rot)).  A GATHER takes consecutive wires, so wires that are not consecutive are copied
    first (COPY costs no bootstrap).  Returns the output wire."""
    wires = [int(w) for w in wires]
    if len(wires) != 1 << (d_tree + d_rot):
        raise ValueError("lhe_array_read: expected 2^(d_tree + d_rot) wires")
    if wires != list(range(wires[0], wires[0] + len(wires))):
        wires = [cir.gate(COPY, w) for w in wires]
    return cir.lhe_gather(set_id, wires[0], d_tree, d_rot)


def wfa_mux_max(cir, a_wires, b_wires, set_ids, width, N=1024):
    """max(a, b) of two `width`-bit numbers the circuit holds as gate bits (MSB first) and the client also sent as TGSW bits (wfa_pair_bits over the
    consecutive sets set_ids): a < b comes from the leveled automaton wfa_less_than with no bootstrap -- its final weights are the gate bits
    +-1/8 as trivial samples, 1/8 in the accepting state -- and drives `width` bootstrapped MUX gates over the LWE bits.  Returns the wires of the
    maximum, MSB first."""
    a_wires, b_wires = list(a_wires), list(b_wires)
    if len(a_wires) != width or len(b_wires) != width:
        raise ValueError("wfa_mux_max: expected `width` wires per number")
    aut = wfa_less_than(width)
    fin = np.zeros((aut[0].shape[1], N), np.int32)
    fin[:, 0] = np.where(np.asarray(aut[2])[0] == 1, 1 << 29, -(1 << 29))
    lt = cir.lhe_wfa(aut, set_ids, cir.lhe_finals(fin))[0]
    return [cir.gate(MUX, lt, b, a) for a, b in zip(a_wires, b_wires)]


# ---- circuit-bootstrap nodes among gates -------------------------------------------------------------------------------------------
def cb_lookup_dag(cir, a_wires, b_wires, table, p_out=8, d_tree=0, encode=None):
    """cb_lookup as one circuit: a_wires, b_wires hold the gate bits of two d-bit numbers (low bit first; d = log2(len(table))), the address is
    a XOR b -- d XOR gates --, a CB node turns the XOR outputs into TGSW bits and an LHE_LOOKUP node at (d_tree, d - d_tree) reads `table`
    (integers in [0, p_out); encode: integers -> Torus32 words, default thfhe.lut.encode at modulus p_out).  Returns the output wire; the plain twin
    is cb_lookup_plain."""
    from . import lut
    t = np.asarray(table, np.int64).reshape(-1)
    d = t.shape[0].bit_length() - 1
    a_wires, b_wires = list(a_wires), list(b_wires)
    if not 1 <= d <= 16 or t.shape[0] != 1 << d or len(a_wires) != d or len(b_wires) != d or not 0 <= d_tree <= min(d, 6) or d - d_tree > 10:
        raise ValueError("table: expected 2^d entries, d wires per operand, 0 <= d_tree <= 6 and d - d_tree <= 10")
    addr = [cir.gate(XOR, a, b) for a, b in zip(a_wires, b_wires)]
    tset = cir.cb_set(addr)
    row0 = cir.lhe_table(lut.lhe_table(t, d_tree, d - d_tree, encode=encode or (lambda v: lut.encode(v, p_out))))
    return cir.lhe_lookup(tset, row0, d_tree, d - d_tree)[0]


def cb_array_read(cir, wires, index_wires, d_tree, d_rot):
    """lhe_array_read at an index the circuit computed: wires[index] for the index whose gate bits are index_wires (low bit first,
    d_tree + d_rot of them, len(wires) = 2^(d_tree + d_rot)); a CB node makes the TGSW bits.  Returns the output wire."""
    index_wires = list(index_wires)
    if len(index_wires) != d_tree + d_rot:
        raise ValueError("cb_array_read: expected d_tree + d_rot index wires")
    wires = [int(w) for w in wires]
    if wires != list(range(wires[0], wires[0] + len(wires))):   # before the CB node, so that it shares their level
        wires = [cir.gate(COPY, w) for w in wires]
    return lhe_array_read(cir, wires, cir.cb_set(index_wires), d_tree, d_rot)


def cb_mux_max(cir, a_wires, b_wires, width, N=1024):
    """wfa_mux_max without the client's TGSW copy of the operands: max(a, b) of two `width`-bit numbers the circuit holds as gate bits (MSB first,
    width <= 8): ONE CB node makes a computed set of 2 width bits (a's low bit first, then b's), the automaton wfa_less_than reads it and drives
    `width` MUX gates.  Returns the wires of the maximum, MSB first."""
    a_wires, b_wires = list(a_wires), list(b_wires)
    if not 1 <= width <= 8 or len(a_wires) != width or len(b_wires) != width:
        raise ValueError("cb_mux_max: expected `width` <= 8 wires per number")
    tset = cir.cb_set(a_wires[::-1] + b_wires[::-1])
    trans, _, finals, start = wfa_less_than(width)
    step_bit = np.array([(j & 1) * width + (j >> 1) for j in range(2 * width)], np.int32)   # a_i, b_i, low bit first, all in the one set
    fin = np.zeros((trans.shape[1], N), np.int32)
    fin[:, 0] = np.where(np.asarray(finals)[0] == 1, 1 << 29, -(1 << 29))
    lt = cir.lhe_wfa((trans, step_bit, finals, start), [tset], cir.lhe_finals(fin))[0]
    return [cir.gate(MUX, lt, b, a) for a, b in zip(a_wires, b_wires)]


def _lhe_plain_bits(lhe_bits, set_id, instance, computed=None):
    if set_id >= CB_SET_BASE:   # a computed set: the bits simulate derived from the wires
        return computed[set_id - CB_SET_BASE]
    if lhe_bits is None or set_id >= len(lhe_bits):
        raise ValueError("simulate: the circuit holds leveled nodes; lhe_bits must give the plain bits of every set")
    b = np.asarray(lhe_bits[set_id], np.int64)
    return b[instance] if b.ndim == 2 else b


def _tables(ck, cir):
    return np.stack([np.asarray(t, ck._tv_dtype).reshape(ck.params.N) for t in cir.tables])


def _rotate_noiseless(x, tv, theta):
    """Coefficients 0 .. theta-1 of X^{-bar} tv for the noiseless phase word x: what a programmable bootstrap of table tv returns on it."""
    N = tv.shape[0]
    steps = 2 * N // theta
    shift = 32 - (steps.bit_length() - 1)
    bar = ((((int(x) & 0xFFFFFFFF) + (1 << (shift - 1))) >> shift) % steps) * theta
    out = []
    for j in range(theta):
        k = (bar + j) % (2 * N)
        out.append(int(tv[k]) if k < N else -int(tv[k - N]))
    return out


def _tv32(tv):
    """a test vector as Torus32 words: an int64 table of the 3-gen engine rounded to its top 32 bits, what the key-switched record carries"""
    tv = np.asarray(tv)
    if tv.dtype != np.int64:
        return tv
    return (((tv.astype(object) + (1 << 31)) >> 32) % (1 << 32)).astype(np.int64)


def _mv_test_vector(tv0, taps):
    """tv0 * F mod (X^N + 1, 2^32) for the factor F = sum_k taps[k] X^(box/2 + k box), box = N / p: the test vector a multi-value output equals a
    plain rotation of (thfhe_mv_lut_bootstrap)."""
    tv0 = np.asarray(tv0, np.int64)
    N, p = tv0.shape[0], len(taps)
    box = N // p
    acc = np.zeros(N, np.int64)
    for k, c in enumerate(taps):
        e = box // 2 + k * box
        acc += int(c) * np.concatenate([-tv0[N - e:], tv0[:N - e]])
    return ((acc + (1 << 31)) % (1 << 32)) - (1 << 31)


def _simulate_words(cir, input_words, lhe_bits=None, instance=0):
    """simulate for circuits with LUT-type nodes: noiseless Torus32 phase words in (thfhe.lut.encode of the digits; +-2^29 for gate bits), the
    noiseless phase word of every wire out (thfhe.lut.decode gives the digits)."""
    from . import lut
    N = len(cir.tables[0]) if cir.tables else (len(cir.tv1[0]) if cir.tv1 else (len(cir.mv_bases[0]) if cir.mv_bases else 1024))
    v = np.zeros(cir.n_wires(), np.int64)
    v[:cir.n_inputs] = np.asarray(input_words, np.int64)
    wrap = lambda t: ((int(t) + (1 << 31)) % (1 << 32)) - (1 << 31)
    lin = lambda spec, ws: wrap(sum(int(w) * int(v[i]) for w, i in zip(spec[1], ws)) + spec[2])
    gates_only = Circuit()
    computed = {}   # computed set -> its plain bits, from the gate-encoded wires
    for gi, (op, a, b, c) in enumerate(cir.gates):
        o = cir.n_inputs + gi
        if op == LUT_OUT:
            continue
        if op == CB:
            wires = cir.cb_specs[cir.cb_rows[gi][0]]
            computed[cir.cb_rows[gi][0]] = np.array([int(v[w] > 0) for w in wires], np.int64)
            v[o] = v[wires[0]]
            continue
        if op == DENSE:   # x_m = sum_k W[m][k] v_k + bias[m] (dense_plain on the messages), then output m's table
            W, bias, tids, theta = cir.dense_specs[cir.dense_rows[gi][0]]
            ws = cir._dense_operands(gi)
            for m in range(W.shape[0]):
                x = wrap(sum(int(W[m, k]) * int(v[w]) for k, w in enumerate(ws)) + (0 if bias is None else int(bias[m])))
                outs = _rotate_noiseless(x, _tv32(cir.tables[0 if tids is None else tids[m]]), theta)
                v[o + m * theta:o + (m + 1) * theta] = [wrap(t) for t in outs]
            continue
        if op in (LUT, LUT_ENC):
            si, ti = cir.lut_rows[gi] if op == LUT else cir.ext_rows[gi]
            tv = cir.tables[ti] if op == LUT else cir.enc_tables[ti][2]
            if tv is None:
                raise ValueError("simulate: the encrypted table was registered without its plaintext")
            spec = cir.specs[si]
            outs = _rotate_noiseless(lin(spec, (a, b, c)[:spec[0]]), np.asarray(tv), spec[3])
            v[o:o + spec[3]] = [wrap(t) for t in outs]
        elif op == SELECT:
            ti, first = cir.ext_rows[gi]
            _, hi, p = cir.tree_specs[ti]
            tv = lut.test_vector(lut._to_i32(v[first:first + p]), p, N=N)
            v[o] = wrap(_rotate_noiseless(lin(hi, (a, b, c)[:hi[0]]), tv, 1)[0])
        elif op == TREE:
            ti, row0 = cir.ext_rows[gi]
            lo, hi, p = cir.tree_specs[ti]
            ops = (a, b, c)
            x = lin(lo, ops[:lo[0]])
            cands = [wrap(t) for r in range(p // lo[3]) for t in _rotate_noiseless(x, np.asarray(cir.tv1[row0 + r]), lo[3])]
            tv = lut.test_vector(lut._to_i32(np.array(cands, np.int64)), p, N=N)
            v[o] = wrap(_rotate_noiseless(lin(hi, ops[lo[0]:lo[0] + hi[0]]), tv, 1)[0])
        elif op in (MV, TREE_MV):
            mi, t = cir.mv_rows[gi]
            lo, hi, p, q, k, base, tabs = cir.mv_specs[mi]
            ops = (a, b, c)
            x = lin(lo, ops[:lo[0]])
            outs = [[wrap(_rotate_noiseless(x, _mv_test_vector(cir.mv_bases[base], tabs[t][j][h]), 1)[0]) for h in range(q)] for j in range(k)]
            if op == MV:
                v[o:o + q] = outs[0]
            else:
                y = lin(hi, ops[lo[0]:lo[0] + hi[0]])
                v[o:o + k] = [wrap(_rotate_noiseless(y, lut.test_vector(lut._to_i32(np.array(cands, np.int64)), q, N=N), 1)[0]) for cands in outs]
        elif op in (LHE_LOOKUP, LHE_GATHER):
            lk, y = cir.lhe_rows[gi]
            set_id, d_tree, d_rot, theta = cir.lhe_specs[lk]
            bits = _lhe_plain_bits(lhe_bits, set_id, instance, computed)[:d_tree + d_rot]
            addr = int(sum(int(bit) << i for i, bit in enumerate(bits)))
            if op == LHE_GATHER:
                v[o] = v[y + addr]
            else:
                poly = cir.lhe_tab[y + (addr >> d_rot)][2]
                if poly is None:
                    raise ValueError("simulate: the encrypted table polynomial was registered without its plaintext")
                at = (addr & ((1 << d_rot) - 1)) * (len(poly) >> d_rot)
                v[o:o + theta] = poly[at:at + theta]
        elif op == LHE_WFA:
            wi, y = cir.lhe_rows[gi]
            trans, step_bit, start, theta, set0, n_sets = cir.wfa_specs[wi]
            state = np.array(start, np.int64)
            for j, sb in enumerate(step_bit):
                state = trans[j][state, int(_lhe_plain_bits(lhe_bits, set0 + (sb >> 4), instance, computed)[sb & 15])]
            for k, q in enumerate(state):
                poly = cir.lhe_fin[y + int(q)][2]
                if poly is None:
                    raise ValueError("simulate: the encrypted final weight was registered without its plaintext")
                v[o + k * theta:o + (k + 1) * theta] = poly[:theta]
        elif op == NOT:
            v[o] = wrap(-int(v[a]))
        elif op == COPY:
            v[o] = v[a]
        else:   # a bootstrapped gate on the signs of its operands
            gates_only.n_inputs, gates_only.gates = o, [(op, a, b, c)]
            v[o] = (1 << 29) if simulate(gates_only, v[:o] > 0)[o] else -(1 << 29)
    return lut._to_i32(v)


def simulate(cir, input_bits, lhe_bits=None, instance=0):
    """Plaintext evaluation of the DAG (wiring check): bool[n_inputs] -> bool[n_wires].  Circuits with LUT, LUT_ENC, SELECT, TREE, multi-value or
    leveled nodes work on integer digits in their torus encoding: int32[n_inputs] noiseless phase words (thfhe.lut.encode(digit, p); +-2^29 for gate
    bits) -> the noiseless phase word int32[n_wires] of every wire, which thfhe.lut.decode turns into digits.  lhe_bits (circuits with leveled
    nodes): the plain bits of every CLIENT TGSW set, low bit first -- int[d] per set, or int[instances][d] of which row `instance` is read; a computed
    set's bits (Circuit.cb_set) come from its wires, a positive phase word reading as 1."""
    from . import ANDNY, ANDYN, NAND, NOR, ORNY, ORYN, XNOR
    if cir.lut_rows or cir.ext_rows or cir.mv_rows or cir.lhe_rows or cir.cb_rows or cir.dense_rows:
        return _simulate_words(cir, input_bits, lhe_bits, instance)
    v = np.zeros(cir.n_wires(), bool)
    v[:cir.n_inputs] = np.asarray(input_bits, bool)
    f = {NAND: lambda a, b: not (a and b), OR: lambda a, b: a or b, AND: lambda a, b: a and b, XOR: lambda a, b: a != b,
         XNOR: lambda a, b: a == b, NOR: lambda a, b: not (a or b), ANDNY: lambda a, b: (not a) and b,
         ANDYN: lambda a, b: a and (not b), ORNY: lambda a, b: (not a) or b, ORYN: lambda a, b: a or (not b)}
    for gi, (op, a, b, c) in enumerate(cir.gates):
        o = cir.n_inputs + gi
        if op == NOT:
            v[o] = not v[a]
        elif op == COPY:
            v[o] = v[a]
        elif op == MUX:
            v[o] = v[b] if v[a] else v[c]
        else:
            v[o] = f[op](bool(v[a]), bool(v[b]))
    return v


simulate_ext = simulate


def simulate_mk(cir, input_bits):
    """simulate() plus the 3-gen three-input AND exactly as the reference defines it (3gen_mk_gates.jl:55-64): bootstrap of
    -1/4 + x + y + z.  Three false operands give the phase -5/8 = +3/8 (mod 1), so the reference's gate answers TRUE there -- it is a
    correct AND only when at least one operand is true.  The simulation mirrors the gate, not the name."""
    from . import AND3
    if cir.dense_rows:   # phase words, as simulate: the DENSE nodes through dense_plain's arithmetic on the tables' top 32 bits
        if any(g[0] == AND3 for g in cir.gates):
            raise ValueError("simulate_mk: a circuit with DENSE nodes is simulated on phase words, which has no AND3")
        return _simulate_words(cir, input_bits)
    v = np.zeros(cir.n_wires(), bool)
    v[:cir.n_inputs] = np.asarray(input_bits, bool)
    for gi, (op, a, b, c) in enumerate(cir.gates):
        o = cir.n_inputs + gi
        if op == AND3:
            v[o] = (v[a] and v[b] and v[c]) or not (v[a] or v[b] or v[c])
        else:
            one = Circuit()
            one.n_inputs = o
            one.gates = [(op, a, b, c)]
            v[o] = simulate(one, v[:o])[o]
    return v


# ---- evaluator --------------------------------------------------------------------------------------------------------
def _run_tree_batch(ck, cir, x, sel, pack, tgsw_sets=None, level2=None, one_rotation=False):
    if ck._tv_dtype == np.int64:   # the 3-gen multi-key engine: thfhe_mk_dag_run_mv_batch, with tree rows thfhe_mk_dag_run_tree_batch
        if cir.has_lhe_nodes() or cir.has_cb_nodes():
            raise ValueError("the multi-key executor runs gate, LUT, MV, LUT_ENC, TREE and TREE_MV nodes only (no leveled nodes)")
        if any(g[0] == SELECT for g in cir.gates):
            raise ValueError("the multi-key executor runs no SELECT node: its candidates are key-switched records and need the D = P n packing key, "
                             "trees the D = N key, and a context holds one key")
        mvs, tv0, fac = cir.mv_families()
        bias = [cir.mv_out_bias.get(i, 0) for i in range(len(mvs))]
        if cir.has_dense_nodes():
            enc = cir.enc_tables
            return ck.dag_run_dense_batch(x, cir.nodes(), **cir.dense_families(), specs=cir.specs, tv=_tables(ck, cir) if cir.tables else None,
                                          enc_a=np.stack([e[0] for e in enc]) if enc else None, enc_b=np.stack([e[1] for e in enc]) if enc else None,
                                          trees=cir.tree_specs, tv1=np.stack(cir.tv1) if cir.tv1 else None, mvs=mvs, mv_tv0=tv0, mv_factors=fac,
                                          mv_out_bias=bias if mvs else None, out_wires=sel)
        if cir.has_tree_nodes() or any(g[0] == TREE_MV for g in cir.gates):
            enc = cir.enc_tables
            return ck.dag_run_tree_batch(x, cir.nodes(), cir.specs, _tables(ck, cir) if cir.tables else None, np.stack([e[0] for e in enc]) if enc else None,
                                         np.stack([e[1] for e in enc]) if enc else None, cir.tree_specs, np.stack(cir.tv1) if cir.tv1 else None, mvs, tv0,
                                         fac, bias, sel)
        return ck.dag_run_mv_batch(x, cir.nodes(), cir.specs, _tables(ck, cir) if cir.tables else None, mvs, tv0, fac, bias, sel)
    if cir.mv_out_bias:
        raise ValueError("out_bias on an MV node is the multi-key engine's; the single-key thfhe_dag_run_mv_batch has none")
    enc = cir.enc_tables
    args = (x, cir.nodes(), cir.specs, _tables(ck, cir) if cir.tables else None, np.stack([e[0] for e in enc]) if enc else None,
            np.stack([e[1] for e in enc]) if enc else None, cir.tree_specs, np.stack(cir.tv1) if cir.tv1 else None)
    if cir.has_cb_nodes() or cir.has_dense_nodes():
        if len(tgsw_sets or ()) < cir.n_lhe_sets():
            raise ValueError("the circuit holds leveled nodes: tgsw_sets must give the %d TgswSets they name" % cir.n_lhe_sets())
        names = ("specs", "tv", "enc_a", "enc_b", "trees", "tv1", "mvs", "mv_tv0", "mv_factors")
        kw = dict(zip(names, args[2:] + tuple(cir.mv_families())), tgsw_sets=list(tgsw_sets or ())[:cir.n_lhe_sets()], **cir.lhe_families(), out_wires=sel, pack=pack)
        if cir.has_cb_nodes():
            kw.update(cir.cb_families(), one_rotation=one_rotation, level2=level2)
        if cir.has_dense_nodes():
            return ck.dag_run_dense_batch(x, cir.nodes(), **cir.dense_families(), **kw)
        return ck.dag_run_cb_batch(x, cir.nodes(), **kw)
    if cir.has_lhe_nodes():
        if tgsw_sets is None or len(tgsw_sets) < cir.n_lhe_sets():
            raise ValueError("the circuit holds leveled nodes: tgsw_sets must give the %d TgswSets they name" % cir.n_lhe_sets())
        return ck.dag_run_lhe_batch(*args, *cir.mv_families(), tgsw_sets=list(tgsw_sets), **cir.lhe_families(), out_wires=sel, pack=pack)
    if cir.has_mv_nodes():
        return ck.dag_run_mv_batch(*args, *cir.mv_families(), sel, pack)
    return ck.dag_run_tree_batch(*args, sel, pack)


def evaluate(ck, cir, input_records, stats=None, pack=None, tgsw_sets=None, level2=None, one_rotation=False):
    """Run the DAG on the engine.  input_records: int32[n_inputs][n+1].  Returns int32[n_wires][n+1].
    Single-key contexts use the native scheduler / executor (thfhe_dag_run: wires stay in HBM, no host round trip per level);
    multi-key contexts go level by level through thfhe_mk_gates_mixed (evaluate_levels).  Circuits with LUT nodes run on
    thfhe_dag_run_lut_batch / thfhe_mk_dag_run_lut_batch, circuits with encrypted-table, select or tree nodes on thfhe_dag_run_tree_batch
    (pack: the threshold.PolyContext holding the packing key), circuits with leveled nodes on thfhe_dag_run_lhe_batch (tgsw_sets: the TgswSets they
    name; sample 0 is read), circuits with CB nodes on thfhe_dag_run_cb_batch (level2: the level-2 key, default the one cb_key_set named; one_rotation:
    CloudKey.circuit_bootstrap's)."""
    if cir.has_luts() or cir.has_tree_nodes() or cir.has_mv_nodes() or cir.has_lhe_nodes() or cir.has_cb_nodes() or cir.has_dense_nodes():
        x = np.ascontiguousarray(input_records, np.int32).reshape(1, cir.n_inputs, ck.words)
        if cir.has_tree_nodes() or cir.has_mv_nodes() or cir.has_lhe_nodes() or cir.has_cb_nodes() or cir.has_dense_nodes():
            out, st = _run_tree_batch(ck, cir, x, None, pack, tgsw_sets, level2, one_rotation)
        else:
            out, st = ck.dag_run_lut_batch(x, cir.nodes(), cir.specs, _tables(ck, cir))
        if stats is not None:
            stats.update(cir.census(), **st)
        return np.concatenate([x[0], out[0]])
    if hasattr(ck, "dag_run"):
        vals, st = ck.dag_run(input_records, np.array(cir.gates, np.int32).reshape(-1, 4))
        if stats is not None:
            stats.update(cir.census(), **st)
        return vals
    return evaluate_levels(ck, cir, input_records, stats)


def evaluate_batch(ck, cir, input_records, out_wires=None, stats=None, pack=None, tgsw_sets=None, level2=None, one_rotation=False):
    """`instances` evaluations of one DAG side by side.  input_records: int32[instances][n_inputs][words]; out_wires: wire ids to return
    (None: every wire).  Returns int32[instances][len(out_wires) or n_wires][words].  Contexts with the native executor use
    thfhe_dag_run_batch / thfhe_mk_dag_run_batch (wire tables stay in HBM), circuits with LUT nodes thfhe_dag_run_lut_batch /
    thfhe_mk_dag_run_lut_batch, circuits with encrypted-table, select or tree nodes thfhe_dag_run_tree_batch (pack: the threshold.PolyContext
    holding the packing key), circuits with leveled nodes thfhe_dag_run_lhe_batch (tgsw_sets: the TgswSets they name, instance q reads sample q);
    circuits with CB nodes thfhe_dag_run_cb_batch (level2, one_rotation: as evaluate); others are driven level by level from the host, a level's call
    holding the gates of all instances."""
    x = np.ascontiguousarray(input_records, np.int32)
    Q, n_in, words = x.shape
    assert n_in == cir.n_inputs
    if cir.has_luts() or cir.has_tree_nodes() or cir.has_mv_nodes() or cir.has_lhe_nodes() or cir.has_cb_nodes() or cir.has_dense_nodes() or hasattr(ck, "dag_run_batch"):
        sel = None if out_wires is None else np.asarray(out_wires, np.int32)
        if cir.has_tree_nodes() or cir.has_mv_nodes() or cir.has_lhe_nodes() or cir.has_cb_nodes() or cir.has_dense_nodes():
            out, st = _run_tree_batch(ck, cir, x, sel, pack, tgsw_sets, level2, one_rotation)
        elif cir.has_luts():
            out, st = ck.dag_run_lut_batch(x, cir.nodes(), cir.specs, _tables(ck, cir), sel)
        else:
            out, st = ck.dag_run_batch(x, np.array(cir.gates, np.int32).reshape(-1, 4), sel)
        if stats is not None:
            stats.update(cir.census(), **st)
        return out if out_wires is not None else np.concatenate([x, out], axis=1)
    from . import AND3 as _AND3
    vals = np.zeros((Q, cir.n_wires(), words), np.int32)
    vals[:, :n_in] = x
    gates, base, launches = cir.gates, cir.n_inputs, 0
    flat = lambda a: a.reshape(-1, words)
    for level in cir.levels():
        if gates[level[0]][0] in (NOT, COPY):
            for g in level:
                src = vals[:, gates[g][1]]
                vals[:, base + g] = (0 - src.astype(np.int64)).astype(np.int32) if gates[g][0] == NOT else src
            continue
        for cls in ("two", "mux", "and3"):
            G = [g for g in level if (gates[g][0] == MUX) == (cls == "mux") and (gates[g][0] == _AND3) == (cls == "and3")]
            if not G:
                continue
            a, b = (flat(vals[:, [gates[g][q] for g in G]]) for q in (1, 2))
            if cls == "two":
                r = ck.gates_mixed(np.tile(np.array([gates[g][0] for g in G], np.int32), Q), a, b)
            else:
                r = ck.gates(MUX if cls == "mux" else _AND3, a, b, flat(vals[:, [gates[g][3] for g in G]]))
            vals[:, base + np.array(G)] = r.reshape(Q, len(G), words)
            launches += 1
    if stats is not None:
        stats.update(cir.census(), launches=launches, instances=Q)
    return vals if out_wires is None else vals[:, np.asarray(out_wires, np.int64)]


def _levels_ext(ck, cir, level, vals, pack):
    """The LUT_ENC, SELECT and TREE nodes of one level through the public flat calls (lut_bootstrap_enc, PackBoxes, tree_lut_bootstrap); returns
    the number of calls' groups."""
    from .threshold import PackBoxes
    gates, base, groups = cir.gates, cir.n_inputs, 0
    mk = ck._tv_dtype == np.int64   # the 3-gen engine: the context holds the packing key, and it runs no SELECT
    by = {}
    for g in level:
        if gates[g][0] in (LUT_ENC, SELECT, TREE):
            x, _ = cir.ext_rows[g]
            by.setdefault((gates[g][0], cir.specs[x][3] if gates[g][0] == LUT_ENC else 0, x), []).append(g)
    for (op, theta, x), G in sorted(by.items()):
        groups += 1
        out = base + np.array(G)
        if op == LUT_ENC:
            nin, w, bias, _ = cir.specs[x]
            ins = [vals[[gates[g][1 + q] for g in G]] for q in range(nin)]
            r = ck.lut_bootstrap_enc(np.stack([e[0] for e in cir.enc_tables]), np.stack([e[1] for e in cir.enc_tables]), *ins, weights=w[:nin], bias=bias,
                                     theta=theta, lut_index=[cir.ext_rows[g][1] for g in G])
            for j in range(theta):
                vals[out + j] = r[:, j]
            continue
        lo, hi, p = cir.tree_specs[x]
        if op == SELECT and mk:
            raise ValueError("the multi-key engine runs no SELECT node")
        if op == SELECT:
            cands = vals[np.concatenate([cir.ext_rows[g][1] + np.arange(p) for g in G])]
            a, b = PackBoxes(pack, cands, p)
            ins = [vals[[gates[g][1 + q] for g in G]] for q in range(hi[0])]
            vals[out] = ck.lut_bootstrap_enc(a, b, *ins, weights=hi[1][:hi[0]], bias=hi[2], lut_index=np.arange(len(G)))[:, 0]
        else:
            R = p // lo[3]
            row0s = sorted({cir.ext_rows[g][1] for g in G})
            tv1 = np.stack([np.stack(cir.tv1[r:r + R]) for r in row0s])
            lo_in = tuple(vals[[gates[g][1 + q] for g in G]] for q in range(lo[0]))
            hi_in = tuple(vals[[gates[g][1 + lo[0] + q] for g in G]] for q in range(hi[0]))
            vals[out] = ck.tree_lut_bootstrap(*(() if mk else (pack,)), tv1, lo_in, hi_in, p_hi=p, weights_lo=lo[1][:lo[0]], bias_lo=lo[2], theta=lo[3], weights_hi=hi[1][:hi[0]],
                                              bias_hi=hi[2], table_index=[row0s.index(cir.ext_rows[g][1]) for g in G])
    return groups


def _levels_mv(ck, cir, level, vals, pack):
    """The MV and TREE_MV nodes of one level through the public flat calls (mv_lut_bootstrap, tree_lut_bootstrap_mvk), one call per spec; returns
    the number of calls."""
    gates, base, by = cir.gates, cir.n_inputs, {}
    mk = ck._tv_dtype == np.int64   # the 3-gen engine: out_bias, and the context holds the packing key
    for g in level:
        if gates[g][0] in (MV, TREE_MV):
            by.setdefault((gates[g][0], cir.mv_rows[g][0]), []).append(g)
    for (op, mi), G in sorted(by.items()):
        lo, hi, p, q, k, b, tabs = cir.mv_specs[mi]
        out = base + np.array(G)
        idx = [cir.mv_rows[g][1] for g in G]
        lo_in = tuple(vals[[gates[g][1 + i] for g in G]] for i in range(lo[0]))
        extra = dict(out_bias=cir.mv_out_bias.get(mi, 0)) if mk else {}
        if op == MV:
            r = ck.mv_lut_bootstrap(np.stack([t[0] for t in tabs]), *lo_in, tv0=cir.mv_bases[b], weights=lo[1][:lo[0]], bias=lo[2], table_index=idx, **extra)
        else:
            hi_in = tuple(vals[[gates[g][1 + lo[0] + i] for g in G]] for i in range(hi[0]))
            r = ck.tree_lut_bootstrap_mvk(*(() if mk else (pack,)), np.stack(tabs), lo_in, hi_in, tv0=cir.mv_bases[b], weights_lo=lo[1][:lo[0]], bias_lo=lo[2],
                                          weights_hi=hi[1][:hi[0]], bias_hi=hi[2], table_index=idx, **extra)
        for j in range(r.shape[1]):
            vals[out + j] = r[:, j]
    return len(by)


def _levels_lhe(ck, cir, level, vals, pack, tgsw_sets, instance, computed=None):
    """The leveled nodes of one level through the public flat calls on sample `instance` of the sets (lhe_lookup; PackBoxes + lhe_lookup; lhe_wfa),
    one call per node; returns the number of calls.  computed: the one-sample TgswSets circuit_bootstrap made of the CB nodes above (sample 0 is read)."""
    from .threshold import PackBoxes
    gates, base, calls = cir.gates, cir.n_inputs, 0
    fam = cir.lhe_families()
    pick = lambda s: (computed[s - CB_SET_BASE], 0) if s >= CB_SET_BASE else (tgsw_sets[s], instance)
    for g in level:
        op = gates[g][0]
        if op not in _LHE_OPS:
            continue
        x, y = cir.lhe_rows[g]
        calls += 1
        if op == LHE_WFA:
            trans, step_bit, start, theta, set0, n_sets = cir.wfa_specs[x]
            n = trans.shape[1]
            r = ck.lhe_wfa([pick(s)[0] for s in range(set0, set0 + n_sets)], trans, step_bit, fam["fin_b"][y:y + n], start, theta=theta,
                           fin_a=None if fam["fin_a"] is None else fam["fin_a"][y:y + n], first=pick(set0)[1], count=1)
            vals[base + g:base + g + start.shape[0] * theta] = r[0].reshape(-1, r.shape[-1])
            continue
        set_id, d_tree, d_rot, theta = cir.lhe_specs[x]
        if op == LHE_GATHER:
            tab_a, tab_b = PackBoxes(pack, vals[y:y + (1 << (d_tree + d_rot))], 1 << d_rot)
        else:
            tab_b = fam["tab_b"][y:y + (1 << d_tree)]
            tab_a = None if fam["tab_a"] is None else fam["tab_a"][y:y + (1 << d_tree)]
        r = ck.lhe_lookup(pick(set_id)[0], tab_b, d_tree=d_tree, d_rot=d_rot, theta=theta, tab_a=tab_a, first=pick(set_id)[1], count=1)
        vals[base + g:base + g + theta] = r[0]
    return calls


def _levels_dense(ck, cir, level, vals):
    """The DENSE nodes of one level through the public flat call (linear_lut_bootstrap), one call per layer with its nodes as the samples; returns
    the number of calls."""
    gates, base, by = cir.gates, cir.n_inputs, {}
    for g in level:
        if gates[g][0] == DENSE:
            by.setdefault(cir.dense_rows[g][0], []).append(g)
    for layer, G in sorted(by.items()):
        W, bias, tids, theta = cir.dense_specs[layer]
        x = np.stack([vals[cir._dense_operands(g)] for g in G])
        r = ck.linear_lut_bootstrap(_tables(ck, cir), W, x, bias, theta=theta, lut_index=tids)
        for j, g in enumerate(G):
            vals[base + g:base + g + W.shape[0] * theta] = r[j].reshape(-1, r.shape[-1])
    return len(by)


def evaluate_levels(ck, cir, input_records, stats=None, pack=None, tgsw_sets=None, instance=0, level2=None, one_rotation=False):
    """The same schedule driven from the host: one host-buffer call per level (works for single-key and multi-key contexts).  LUT nodes go
    through ck.lut_bootstrap, one call per (theta, spec) of a level: the yardstick of the native LUT-node executor.  LUT_ENC, SELECT and TREE nodes
    go through lut_bootstrap_enc, PackBoxes + lut_bootstrap_enc and tree_lut_bootstrap (pack: the packing context): the yardstick of
    thfhe_dag_run_tree_batch.  MV and TREE_MV nodes go through mv_lut_bootstrap and tree_lut_bootstrap_mvk: the yardstick of thfhe_dag_run_mv_batch.
    Leveled nodes go through lhe_lookup, PackBoxes + lhe_lookup and lhe_wfa on sample `instance` of tgsw_sets: the yardstick of thfhe_dag_run_lhe_batch.
    A CB node goes through circuit_bootstrap of its wires' records (one sample; one_rotation: its mode; level2 is the key's own, cb_key_set's), the
    leveled nodes that read it through the flat calls on that set: the yardstick of thfhe_dag_run_cb_batch."""
    words = ck.words
    vals = np.zeros((cir.n_wires(), words), np.int32)
    vals[:cir.n_inputs] = np.asarray(input_records, np.int32).reshape(cir.n_inputs, words)
    computed = {}  # computed set -> the one-sample TgswSet circuit_bootstrap made of it
    try:
        launches = _evaluate_levels(ck, cir, vals, pack, tgsw_sets, instance, one_rotation, computed)
    finally:
        for t in computed.values():
            t.close()
    if stats is not None:
        stats.update(cir.census(), launches=launches)
    return vals


def _evaluate_levels(ck, cir, vals, pack, tgsw_sets, instance, one_rotation, computed):
    """evaluate_levels' walk over the levels, into vals; the TgswSets it makes of CB nodes go into `computed`, which the caller closes.  Returns the
    number of host-buffer calls."""
    from . import AND3 as _AND3
    gates, base, launches = cir.gates, cir.n_inputs, 0
    for level in cir.levels():
        op0 = gates[level[0]][0]
        if op0 in (NOT, COPY):
            for g in level:   # in gate order: a NOT may read another NOT of the same depth
                src = vals[gates[g][1]]
                vals[base + g] = (0 - src.astype(np.int64)).astype(np.int32) if gates[g][0] == NOT else src
            continue
        luts = [g for g in level if gates[g][0] == LUT]
        if luts:
            # LUT nodes grouped by (theta, spec): one lut_bootstrap per group, each node's table through lut_index
            tvs = _tables(ck, cir)
            groups = {}
            for g in luts:
                sp = cir.specs[cir.lut_rows[g][0]]
                groups.setdefault((sp[3], cir.lut_rows[g][0]), []).append(g)
            for (theta, si), G in sorted(groups.items()):
                nin, w, bias, _ = cir.specs[si]
                ins = [vals[[gates[g][1 + q] for g in G]] for q in range(nin)]
                r = ck.lut_bootstrap(tvs, *ins, weights=w[:nin], bias=bias, theta=theta, lut_index=[cir.lut_rows[g][1] for g in G])
                for j in range(theta):
                    vals[base + np.array(G) + j] = r[:, j]
                launches += 1
        if cir.ext_rows:
            launches += _levels_ext(ck, cir, level, vals, pack)
        if cir.mv_rows:
            launches += _levels_mv(ck, cir, level, vals, pack)
        if cir.lhe_rows:
            launches += _levels_lhe(ck, cir, level, vals, pack, tgsw_sets, instance, computed)
        if cir.dense_rows:
            launches += _levels_dense(ck, cir, level, vals)
        for g in level:
            if gates[g][0] == CB:
                wires = cir.cb_specs[cir.cb_rows[g][0]]
                computed[cir.cb_rows[g][0]] = ck.circuit_bootstrap(vals[wires], len(wires), one_rotation=one_rotation)
                vals[base + g] = vals[wires[0]]
                launches += 1
        two = [g for g in level if gates[g][0] not in (MUX, _AND3, LUT, LUT_OUT, LUT_ENC, SELECT, TREE, MV, TREE_MV, CB, DENSE) + _LHE_OPS]
        mux = [g for g in level if gates[g][0] == MUX]
        and3 = [g for g in level if gates[g][0] == _AND3]   # 3-gen three-input AND: its own gate class (thfhe_mk_gates)
        if and3:
            a, b, c = (vals[[gates[g][q] for g in and3]] for q in (1, 2, 3))
            vals[base + np.array(and3)] = ck.gates(_AND3, a, b, c)
            launches += 1
        if two:
            ops = np.array([gates[g][0] for g in two], np.int32)
            a = vals[[gates[g][1] for g in two]]
            b = vals[[gates[g][2] for g in two]]
            vals[base + np.array(two)] = ck.gates_mixed(ops, a, b)
            launches += 1
        if mux:
            a = vals[[gates[g][1] for g in mux]]
            b = vals[[gates[g][2] for g in mux]]
            c = vals[[gates[g][3] for g in mux]]
            vals[base + np.array(mux)] = ck.gates(MUX, a, b, c)
            launches += 1
    return launches


# ---- encrypted dense layers (CloudKey.lwe_linear / linear_lut_bootstrap): the plaintext side -------------------------------------------
def dense_plain(W, bias_msgs, m, p):
    """The plaintext twin of a dense layer on messages: (m @ W^T + bias_msgs) mod 2p for messages m int[count][K] (or int[K]) in the padding-bit
    encoding of modulus p.  bias_msgs: M integer message offsets (dense_bias_messages) or None.  A value in p .. 2p-1 has left the valid half of
    the torus: the table that follows would read it negated."""
    W = np.asarray(W, np.int64)
    m = np.asarray(m, np.int64)
    s = m @ W.T
    if bias_msgs is not None:
        s = s + np.asarray(bias_msgs, np.int64)
    return s % (2 * p)


def dense_bias_messages(W, p, lo=0, m_max=None):
    """The integer message offset of every output that moves its smallest reachable sum to message `lo`, the inputs being messages in 0 .. m_max
    (default p - 1): lo - sum_k min(0, W[m][k]) m_max.  Raises ValueError if an output's reachable sums then do not fit in [0, p): such a
    layer needs a larger p, smaller weights or fewer inputs."""
    W = np.asarray(W, np.int64)
    m_max = p - 1 if m_max is None else int(m_max)
    low = np.minimum(W, 0).sum(axis=1) * m_max
    high = np.maximum(W, 0).sum(axis=1) * m_max
    off = lo - low
    if lo < 0 or np.any(high + off >= p):
        raise ValueError(f"dense layer: reachable sums span up to {int((high - low).max()) + 1} messages from lo = {lo}, the encoding holds {p}")
    return off


def dense_bias(W, p, lo=0, m_max=None):
    """dense_bias_messages as the Torus32 bias words (int32[M]) linear_lut_bootstrap takes.  The padding-bit encoding needs EVERY reachable
    sum_k W[m][k] m_k + bias inside [0, p); the library adds words mod 2^32 and cannot see a sum that left the range -- keeping it inside is
    the caller's duty, and this function refuses a layer whose range cannot fit."""
    off = dense_bias_messages(W, p, lo, m_max)
    return ((off * ((1 << 32) // (2 * p))) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def conv2d_weights(kernel, in_shape, stride=1):
    """The dense W of a valid 2-D convolution (cross-correlation, as neural networks use the word), so that a convolution layer is the same call:
    out[f][y][x] = sum_{i,j} kernel[f][i][j] in[y stride + i][x stride + j].  kernel: int[kh][kw] or int[F][kh][kw]; in_shape = (H, Wd); inputs
    flattened row-major (K = H Wd), outputs row-major per filter (M = F oh ow, oh = (H - kh) // stride + 1).  Returns int32[M][K]."""
    k = np.asarray(kernel, np.int64)
    if k.ndim == 2:
        k = k[None]
    H, Wd = in_shape
    F, kh, kw = k.shape
    if stride < 1 or kh > H or kw > Wd:
        raise ValueError("conv2d_weights: the kernel must fit the input and stride must be >= 1")
    oh, ow = (H - kh) // stride + 1, (Wd - kw) // stride + 1
    out = np.zeros((F, oh, ow, H, Wd), np.int64)
    for y in range(oh):
        for x in range(ow):
            out[:, y, x, y * stride:y * stride + kh, x * stride:x * stride + kw] = k
    return out.reshape(F * oh * ow, H * Wd).astype(np.int32)


# ---- dense layers as nodes of a circuit (Circuit.dense_layer / dense) ---------------------------------------------------------------------
def dense_network(cir, inputs, layers):
    """Chain dense layers: `layers` holds layer ids (Circuit.dense_layer) or (W, bias, table_ids) triples registered here with theta = 1; the M
    outputs of a layer are the operands of the next.  Returns the output wires of every layer, the last list being the network's outputs."""
    outs, x = [], list(inputs)
    for l in layers:
        if not isinstance(l, (int, np.integer)):
            l = cir.dense_layer(*l)
        if cir.dense_specs[l][3] != 1:
            raise ValueError("dense_network: a chained layer has theta = 1")
        x = [o[0] for o in cir.dense(l, x)]
        outs.append(x)
    return outs


def dense_argmax(cir, scores, p, N=1024, torus_bits=32):
    """One-hot argmax of the score wires (messages 0 .. p/2 - 1 in the padding-bit encoding of modulus p): a LUT node per pair i < j on
    s_i - s_j + p/2 (inside [1, p - 1], table `>= p/2` in the gates' encoding), whose NOT is the reverse comparison, and an AND chain per score:
    winner i beats every later score or ties it, and beats every earlier one strictly, so exactly one gate bit is set -- the lowest index among
    the maxima.  Two levels and len(scores) (len(scores) - 1) / 2 rotations for the comparisons, then the AND chains.  Returns the winner wires."""
    from . import lut
    n = len(scores)
    if n < 2:
        raise ValueError("dense_argmax: at least two scores")
    ge = cir.table(lut.test_vector(lut.bool_outputs(lambda s: s >= p // 2, p, torus_bits=torus_bits), p, N=N, torus_bits=torus_bits))
    half = int(lut.encode(p // 2, p))
    beats = {}
    for i in range(n):
        for j in range(i + 1, n):
            beats[i, j] = cir.lut(ge, [scores[i], scores[j]], weights=(1, -1), bias=half)[0]   # s_i >= s_j
            beats[j, i] = cir.gate(NOT, beats[i, j])                                             # s_j > s_i
    winners = []
    for i in range(n):
        terms = [beats[i, j] for j in range(n) if j != i]
        w = terms[0]
        for t in terms[1:]:
            w = cir.gate(AND, w, t)
        winners.append(w)
    return winners


def dense_argmax_plain(scores):
    """The plain twin of dense_argmax: the one-hot vector of the lowest index among the maxima."""
    s = np.asarray(scores, np.int64)
    out = np.zeros(s.shape, np.int64)
    idx = s.argmax(axis=-1)
    np.put_along_axis(out, np.expand_dims(idx, -1), 1, axis=-1)
    return out
