/*
 * qsv.h -- C ABI of libqsv.so: MI355X (gfx950) state-vector gate application.
 *
 * This is the drop-in boundary for the gate-application hot path of the reference's
 * simulators/{dv,cv}_simulator.  The reference has no FFI layer: its boundary is the duck-typed
 * Python protocol `gate.apply(state)` (simulators/dv_simulator/simulator.py:47-52,
 * simulators/cv_simulator/simulator.py:66-70).  Each entry point below names the reference
 * code it replaces.  Python binds this header with ctypes (quantum_computations_amd/_lib.py);
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - All functions return an int status: QSV_OK (0) or a negative QSV_E* code; the message of
 *    the most recent failure on the calling thread is returned by qsv_last_error().
 *  - Amplitudes are complex128, interleaved (re, im) doubles -- the memory layout of a NumPy
 *    complex128 array.  Matrices are row-major, interleaved complex.
 *  - Qubit numbering is the reference's: qubit q of an n-qubit register is bit (n-1-q) of the
 *    flat amplitude index (qubit 0 = most significant; `X(0)|000>` -> index 4).  For a k-qubit
 *    matrix, qubits[0] is the most significant leg, matching expand_gate's kron(gate, I, ...) +
 *    `targets` order (simulators/dv_simulator/numpy_quantum.py:243-247).
 *  - A qsv_state is owned by the library and used from one host thread at a time; calls enqueue
 *    work on the state's HIP stream and return without waiting unless they return data.
 *    Distinct handles may be used concurrently from distinct threads.
 *  - Host buffers passed in are only read/written during the call.  Randomness stays with the
 *    caller (qsv_measure takes the uniform draw), so seeded runs and forced results reproduce.
 */
#ifndef QSV_H
#define QSV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QSV_VERSION 100 /* 0.1.0 */

enum {
    QSV_OK = 0,
    QSV_EINVAL = -1,  /* bad qubit / duplicate index / bad size -> Python ValueError (gates.py:9-19) */
    QSV_ENOMEM = -2,  /* device allocation failed or view capacity too small -> MemoryError */
    QSV_EHIP = -3,    /* HIP runtime error (no device, launch failure, ...) -> RuntimeError */
    QSV_ESTATE = -4   /* wrong kind of state for this call (qubit vs qudit) -> TypeError */
};

/* Options for qsv_set_option. */
enum {
    QSV_OPT_SPECIALIZE = 1, /* 1 (default): diagonal / controlled / permutation matrices take the
                               reduced-traffic kernels; 0: every gate runs the dense kernel */
    QSV_OPT_UNROLL = 2,     /* work items in flight per thread (1,2,4,8); 0 = built-in default */
    QSV_OPT_GRID_CAP = 3,   /* max workgroups per launch; 0 = one tile per workgroup */
    QSV_OPT_NONTEMPORAL = 4, /* 1 (default): nontemporal loads/stores in the streaming kernels */
    QSV_OPT_ITEM_STRIDE_BIT = 5, /* log2 of the distance (in work items) between the items one thread keeps in
                                    flight when unroll > 1; default 8 = consecutive 4 KiB tiles */
    QSV_OPT_TILE_REGIONS = 6, /* tile order of the streaming kernels: R > 1 walks R contiguous regions of the register
                                side by side (8 = one per XCD), 0 = plain order, -1 (default) = per-kernel choice */
    QSV_OPT_KQ_VARIANT = 7,  /* qsv_apply_kq, k = 3..5, how target bits below 6 reach the registers: 0 (default) =
                                the measured best per case, 1 = wave-shuffle butterflies, 2 = no exchange (per-thread
                                strided access), 3 = line-granular exchange (address arithmetic for bits 3..5, LDS for
                                bits 0..2), 4 = workgroup tile staged through LDS (k = 3..5, every target bit >= 3; other
                                placements as 0), 5 = f64 matrix cores for k = 5 (k = 3, 4 as 0), 6 = f64 matrix cores fed from the LDS
                                tile, matrix in registers, complex k = 5 on bits >= 3 (other cases as 0).  Values 1 and 2 also keep
                                1- and 2-qubit gates on the register kernels (k_dense) instead of the workgroup-tile
                                form (k_dense_tile12).  Same results; for measurements */
    QSV_OPT_PLANE_KERNEL = 8, /* qsv_apply_mode2_blocks on the last two modes with real blocks: 1 (default) = one
                                workgroup per (d x d) plane staged through LDS, 0 = one thread per plane */
    QSV_OPT_READOUT_VARIANT = 9, /* qsv_measure_probs / collapse / insert / permute / k-qubit diagonals: 0 (default) =
                                streaming kernels (whole 1 KiB segments per wave whatever the bit), 1 = plain
                                grid-stride kernels (always used below 14 qubits), 2 = as 0 but reduced density matrices
                                with round 2's per-lane row loads (k_rdm) instead of the LDS-staged workgroup tile
                                (k_rdm_tile).  Same results; for measurements */
    QSV_OPT_COMPLEX_PRODUCT = 10, /* complex 32 x 32 / 64 x 64 blocks (qsv_apply_kq, k = 5, 6): 0 (default) = three real
                                multiplications per matrix entry (Ar xr, Ai xi, (Ar + Ai)(xr + xi)) on the matrix cores (k = 6)
                                and four on the vector kernels (k = 5), 3 = three on the vector kernels too, 4 = four
                                everywhere.  Equal to rounding (normwise); for measurements */
    QSV_OPT_SEQUENCE_WORK = 11, /* qsv_apply_sequence: the largest gate sequence applied as a sequence, in multiply-adds
                                per 32 amplitudes (256 per one-qubit gate, 512 per two-qubit gate; the dense block costs
                                4096).  Longer sequences report handled = 0.  -1 (default) = $QSV_SEQUENCE_WORK or 0, 0 = never: the
                                sequence form measured no faster than the dense block; kept for measurements */
    QSV_OPT_TILE_SEQUENCE_GATES = 12, /* qsv_apply_sequence: blocks made of at most this many 1- and 2-qubit gates are
                                applied as that gate list on LDS-resident tiles (k_seq_tile) instead of their dense
                                product.  -1 (default) = 6-qubit blocks of at most 12 gates ($QSV_TILE_SEQUENCE_GATES);
                                an explicit value also admits 5-qubit blocks (slower than their dense product: for
                                measurements); 0 = never */
    QSV_OPT_DEFER = 13      /* deferred 1- and 2-qubit gates (see "deferred gates" below): 0 = off, every qsv_apply_* call
                               launches its own kernel; 1 = auto, on registers made by qsv_create of at least 2^22
                               amplitudes; 2 = always (registers made by qsv_create of at least 12 qubits); -1 (default)
                               = $QSV_DEFER or 1.  Same results bit for bit; only the number of passes over HBM changes */
};

typedef struct qsv_state qsv_state;

/* ---- deferred gates ------------------------------------------------------------------------
 * On a register the library allocated (qsv_create) with QSV_OPT_DEFER on, qsv_apply_1q / _2q / _diag_1q / _diag_2q / _cx
 * / _swap / _controlled_1q check their arguments, classify the gate and QUEUE it instead of launching a kernel.  The queue
 * is applied in passes: each pass brings every 4096-amplitude tile of the register into LDS once and applies an ordered
 * list of queued gates to it (k_pass_tile), each with the arithmetic of its own per-gate kernel, so the amplitudes are
 * bit for bit those of the per-gate path.  Gates keep call order, except that CX, CZ, SWAP (any gate whose matrix holds
 * only 0 and +-1) may move ahead of earlier gates on other qubits -- that changes no bit either.
 *  - A rejected call (QSV_EINVAL, ...) returns at once and leaves the queue as it was.
 *  - Every other entry point that takes the register flushes the queue first: sync, download, upload, copy (both
 *    registers), fill_random, scale, set_basis, norm2, inner, expect_*, probabilities, reduced_density, sample,
 *    measure*, collapse, insert, permute, apply_kq, apply_mcphase, apply_sequence, apply_pauli_rotation(s) (never
 *    queued themselves), apply_layer and ensemble_apply_layer (likewise), layer_adjoint and layer_transition (both registers), apply_pauli_sum, pauli_transition_sum, pauli_rotations_adjoint (both registers), set_stream,
 *    set_option, device_ptr,
 *    timer_*, event_*, last_kernel, density_expect_paulis, apply_channel with a general channel, and qsv_flush itself.
 *    qsv_apply_channel with a mixed-unitary channel does NOT flush: its gate is queued like any other, and
 *    qsv_channel_log_read leaves the queue alone.  qsv_destroy drops what is pending.
 *  - A launch error during a flush is returned by the call that flushed; the rest of the queue is dropped.
 *  - Views (qsv_create_view, qsv_rebind_view) never defer, nor does a register once qsv_device_ptr has handed out its
 *    address (the caller may then touch the amplitudes directly): that call flushes and switches deferral off for good.
 *  - Passes are launched while gates are still being queued (once 64 are pending), so the GPU is not idle meanwhile. */
int qsv_flush(qsv_state *st);
/* Gates that went through the queue, and the launches that applied them (passes plus gates run on their own). */
int qsv_defer_stats(const qsv_state *st, uint64_t *gates_queued, uint64_t *launches);

/* ---- library ---------------------------------------------------------------------------- */
int qsv_version(void);
const char *qsv_last_error(void);
int qsv_device_count(int *count);

/* ---- lifecycle -------------------------------------------------------------------------- */
/* Allocate an n-qubit register on `device` initialised to |0...0> (n = 0 is the 1-element
 * register [1.0] that parse_state(None) returns, simulators/dv_simulator/simulator.py:22). */
int qsv_create(int n_qubits, int device, qsv_state **out);
/* Wrap caller-owned device memory (e.g. a torch tensor's data_ptr()) holding `capacity_amps`
 * complex128 slots; `hip_stream` is a hipStream_t (NULL = the default stream).  The register's
 * amplitudes always start at dev_amps; measure/insert keep them there. */
int qsv_create_view(int n_qubits, int device, void *dev_amps, uint64_t capacity_amps, void *hip_stream,
                    qsv_state **out);
/* Re-point a view register (one made by qsv_create_view) at another window of caller-owned device memory, with a new
 * size: no allocation, no synchronisation -- the register's stream orders the launches on either side.  This is how the
 * sharded register applies a gate slice by slice inside an exchange step (one handle walks the landed slices), the
 * part of the reference's `for gate in circuit: state = gate.apply(state)` loop (dv_simulator/simulator.py:40-52) that
 * overlaps with the transfer.  QSV_ESTATE on a register that owns its memory. */
int qsv_rebind_view(qsv_state *st, int n_qubits, void *dev_amps, uint64_t capacity_amps);
int qsv_destroy(qsv_state *st);
int qsv_set_stream(qsv_state *st, void *hip_stream);
int qsv_set_option(qsv_state *st, int option, int64_t value);
int qsv_num_qubits(const qsv_state *st, int *n_qubits);
int qsv_num_amps(const qsv_state *st, uint64_t *n_amps);
int qsv_device_ptr(qsv_state *st, void **dev_amps);
int qsv_sync(qsv_state *st);

/* ---- data movement ---------------------------------------------------------------------- */
int qsv_set_basis(qsv_state *st, uint64_t index);
int qsv_upload(qsv_state *st, const double *host_interleaved, uint64_t offset_amps, uint64_t count_amps);
int qsv_download(qsv_state *st, double *host_interleaved, uint64_t offset_amps, uint64_t count_amps);
int qsv_copy(qsv_state *dst, const qsv_state *src);
/* Fill with pseudo-random complex normal amplitudes keyed by (seed, global amplitude index +
 * index_offset) and leave the squared norm of what was written in *norm2 (may be NULL);
 * qsv_scale() then normalises.  Used for states too large to come from the host. */
int qsv_fill_random(qsv_state *st, uint64_t seed, uint64_t index_offset, double *norm2);
int qsv_scale(qsv_state *st, double re, double im);

/* ---- gate application: replaces Gate.apply -> expand_gate -> `gate @ state`
 *      (simulators/dv_simulator/gates.py:44-54, numpy_quantum.py:243-247) ------------------- */
int qsv_apply_1q(qsv_state *st, int q, const double m[8]);
int qsv_apply_2q(qsv_state *st, int q0, int q1, const double m[32]);
/* Diagonal gates (Z, RZ, P, Pdg, T, Tdg, CZ: gates.py:79-114,128-130): d = the diagonal. */
int qsv_apply_diag_1q(qsv_state *st, int q, const double d[4]);
int qsv_apply_diag_2q(qsv_state *st, int q0, int q1, const double d[8]);
/* CX (gates.py:116-126) and SWAP (gates.py:132-134) as pure amplitude moves. */
int qsv_apply_cx(qsv_state *st, int control, int target);
int qsv_apply_swap(qsv_state *st, int q0, int q1);
/* `m` (2x2) on `target` for amplitudes whose `controls` are all 1 (add_control, numpy_quantum.py:250). */
int qsv_apply_controlled_1q(qsv_state *st, int n_controls, const int *controls, int target, const double m[8]);
/* Multiply the amplitudes whose `qubits` are all 1 by (re, im): multi-controlled phase / Z. */
int qsv_apply_mcphase(qsv_state *st, int n_qubits, const int *qubits, double re, double im);
/* Generic k-qubit matrix (2^k x 2^k), 1 <= k <= 6: Gate(indices, matrix).apply (gates.py:7-54). */
int qsv_apply_kq(qsv_state *st, int k, const int *qubits, const double *m);
/* A fused block given as the SEQUENCE of the gates it was made of instead of their product: the same state as
 * qsv_apply_kq with the product matrix (to rounding), i.e. consecutive iterations of the reference's loop
 * `for gate in circuit: state = gate.apply(state)` (dv_simulator/simulator.py:40-52) in ONE pass over the register.
 * Gate g acts on the block's legs legs[2 g] (and legs[2 g + 1] if arity[g] == 2) -- positions in `qubits` -- with the
 * 2 x 2 / 4 x 4 row-major complex matrix that follows the previous gate's in `matrices`.  A dense 5-qubit block is the one
 * gate shape bound by arithmetic (4 x 1024 FMAs per amplitude group); its few source gates cost a fraction of that on the
 * amplitudes the thread already holds.  Two forms: in registers (k = 5; measured no faster -- two waves per SIMD,
 * profiles/r03_sequence_blocks.txt -- so OFF unless QSV_OPT_SEQUENCE_WORK / $QSV_SEQUENCE_WORK allow it), and on LDS-resident
 * tiles (ON by default for 6-qubit blocks of at most 12 gates, QSV_OPT_TILE_SEQUENCE_GATES).  *handled = 0: no sequence
 * form for this block / register (switched off, over the limits, gates on more than two qubits, tiny registers) -- nothing
 * was applied, call qsv_apply_kq with the product matrix. */
int qsv_apply_sequence(qsv_state *st, int k, const int *qubits, int n_gates, const int *arity, const int *legs,
                       const double *matrices, int *handled);
/* psi <- exp(-i theta/2 P) psi, P = paulis[j] on qubits[j] ('I','X','Y','Z', either case), 0 <= k <= 64: the sign
 * convention of RZ (exp(-i angle/2 Z)).  P|i> = i^{nY} (-1)^{popcount(i & zmask)} |i ^ xmask> and P^2 = 1, so the rotation
 * is cos(theta/2) - i sin(theta/2) P: it mixes only the two amplitudes of each pair {i, i ^ xmask} (a diagonal phase for
 * Z-only strings).  A string of any weight is one pass over the register at the traffic of a one-qubit gate, without a
 * matrix.  The identity string, or k = 0, applies the global phase e^{-i theta/2}. */
int qsv_apply_pauli_rotation(qsv_state *st, int k, const int *qubits, const char *paulis, double theta);
/* psi <- R_{T-1} ... R_1 R_0 psi, R_t = exp(-i thetas[t]/2 P_t), term 0 applied first; layout of
 * term_offsets / qubits / paulis as in qsv_expect_pauli_sum; passes (may be NULL) = kernel launches made.
 * Consecutive rotations that are diagonal or flip the same qubits (equal X/Y positions) act inside the same pairs and
 * share a pass of at most 8 rotations, applied in registers in the caller's order (csrc/qsv_pauli_rotation_plan.h): XX,
 * YY and ZZ on one pair are one pass, T Z-strings are ceil(T / 8).  The list is never reordered.  The whole list is
 * validated before the first launch; QSV_EINVAL leaves the register and the deferred queue as they were; QSV_ESTATE on a
 * mode register; n_terms = 0 does nothing and launches nothing.  The launches go back to back on the register's stream
 * with no host synchronisation. */
int qsv_apply_pauli_rotations(qsv_state *st, int n_terms, const int *term_offsets, const int *qubits,
                              const char *paulis, const double *thetas, uint64_t *passes);
/* The quantum Fourier transform on the ordered qubits qubits[0 .. m-1] (qubits[0] the most significant leg), every other
 * qubit left alone: psi <- F psi with F[y, x] = 2^(-m/2) exp(+2 pi i x y / 2^m), x = sum_r x_r 2^(m-1-r) -- what
 * qsv_apply_kq would do with that matrix, for any m <= 64, and numpy.fft.ifft(norm="ortho") along the flattened legs.
 * flags, combinable: QSV_QFT_INVERSE = the adjoint F^dagger; QSV_QFT_NO_SWAPS = without the final reversal of the m qubits
 * (with INVERSE: without the initial one); QSV_QFT_CONJUGATE = conj(F) (conj(F^dagger) with INVERSE), which the column side
 * of a density matrix takes and which differs from the adjoint once the reversal is left out.
 * Every stage (a Hadamard and its controlled phases) whose qubit lies in one 4096-amplitude tile runs in the same pass over
 * the register (k_qft_tile; csrc/qsv_qft_plan.h): a full 28-qubit transform is 4 passes and one qubit permutation.
 * passes (may be NULL) = kernel launches made: tile passes plus the permutation.  The arguments are checked before the
 * deferred queue is flushed or anything is launched: QSV_EINVAL (null pointer, repeated or out-of-range qubit, unknown flag
 * bit) leaves the register and the queue as they were; QSV_ESTATE on a mode register; m = 0 does nothing.  The transform
 * never joins the deferred queue; it works on views. */
#define QSV_QFT_INVERSE 1
#define QSV_QFT_NO_SWAPS 2
#define QSV_QFT_CONJUGATE 4
int qsv_apply_qft(qsv_state *st, int m, const int *qubits, int flags, uint64_t *passes);
/* ---- product layers: a one-qubit gate on each of many qubits in a few tile passes (csrc/qsv_layer.hip) ----
 * psi <- (U_1 on qubits[0]) (x) ... (x) (U_k on qubits[k-1]) psi for k distinct qubits and any finite 2x2 complex matrices
 * (unitarity is not demanded), the identity on every other qubit: what k calls of qsv_apply_1q give, to rounding.  The
 * factors commute, so the layer is a SET: its stages are always applied in ascending order of the index bit n-1-qubit,
 * whatever order the list has, and the rounded result does not depend on that order.  Every stage whose bit lies in one
 * 4096-amplitude tile (index bits 0..5 and six more) runs in the same pass over the register (k_layer_tile;
 * csrc/qsv_layer_plan.h): *passes (may be NULL) = max(1, ceil(h / 6)) with h the stage bits >= 6 -- a full 28-qubit layer
 * is 4 passes, not 28; registers of at most 12 qubits take one.  k = 0 does nothing and launches nothing.
 * qsv_ensemble_apply_layer gives every member of an ensemble (notation of the ensemble calls below: members =
 * 2^(n_total - member_qubits), `qubits` are MEMBER qubits) matrices of its own, matrices[m][j] on qubits[j]; the plan is made on
 * member bits and never depends on the number of members.  One stage has one statement of its arithmetic
 * (csrc/qsv_layer_item.h): a member's amplitudes are bit for bit those of a register of its own after qsv_apply_layer with
 * the member's matrices, wherever it sits, and qsv_apply_layer on the member part of an ensemble register gives the bits of
 * qsv_ensemble_apply_layer with equal rows.
 * The arguments are checked before the deferred queue is flushed or anything is launched: QSV_EINVAL (null pointer where
 * k > 0, k < 0 or above the register's / member's qubits, a repeated or out-of-range qubit, an entry that is not finite; for
 * the ensemble call also a view or member_qubits outside 0 .. n_total) leaves the register and the queue as they were;
 * QSV_ESTATE on a mode register.  A valid call flushes the queue (a layer is never queued), is enqueued on the register's
 * stream and returns without waiting; the caller's arrays may be reused on return.  qsv_apply_layer works on views. */
int qsv_apply_layer(qsv_state *st, int k, const int *qubits, const double *matrices /* [k][2][2] complex, row-major */, uint64_t *passes);
int qsv_ensemble_apply_layer(qsv_state *st, int member_qubits, int k, const int *qubits /* member-local */,
                             const double *matrices /* [members][k][2][2] complex */, uint64_t *passes);
/* ---- adjoint walk through a product layer: every qubit's transition matrix in the layer's own passes
 *      (csrc/qsv_layer_adjoint.hip) ----
 * For a qubit q (index bit n-1-q) and two registers,
 *     T_q[a][b] = <lambda| (|a><b| on q) |psi> = sum over the other qubits of conj(lambda[a, rest]) psi[b, rest].
 * qsv_layer_adjoint walks the plan of qsv_apply_layer for `qubits` unchanged (csrc/qsv_layer_plan.h: the same passes in the
 * same order, the stages in ascending order of the index bit).  For stage s with W = inverse[s] it first sets
 * values[s][a][b] = T_q (interleaved complex, row-major: re T[0][0], im T[0][0], re T[0][1], ...; `values` and `inverse` are
 * indexed as `qubits` is) on the registers AS THEY STAND, the stages of lower bits already undone, and then applies W to that
 * qubit of BOTH registers with the one statement of a stage's arithmetic (csrc/qsv_layer_item.h).  So
 *  - on return each register holds, bit for bit, what qsv_apply_layer(reg, k, qubits, inverse) would have left in it: BOTH
 *    registers are consumed / rewound, as by qsv_pauli_rotations_adjoint;
 *  - for UNITARY inverse[s] every values[s] equals, up to rounding, the value on the registers at entry: a unitary on
 *    another qubit cancels in the sum over that qubit.  For other matrices the operational definition above is what holds.
 * With psi = (U_1 (x) ... (x) U_k) psi0, inverse[s] = U_s^dagger and lambda = H psi, the derivative of E = <psi|H|psi> in a
 * parameter of U_s is 2 Re sum_ab G[a][b] values[s][a][b], G = (dU_s/dtheta) U_s^dagger; for U = exp(-i theta/2 P) that is
 * Im <lambda|P|psi>, the convention of qsv_pauli_rotations_adjoint.
 * qsv_layer_transition returns the same values with nothing applied and nothing stored: both registers are read only, and
 * bra may be ket (the same handle or the same memory), which gives the one-qubit reduced density matrices of a ket,
 * rho_q[b][a] = values[q][a][b].
 * *passes (may be NULL) = the kernel launches = the passes of the forward plan, max(1, ceil(h / 6)); the sums add no launch.
 * A stage's eight doubles are summed in a fixed order -- over a wave by shuffles, over the four waves of a workgroup in wave
 * order, over the tiles a workgroup walks in index order, and over the workgroups' partials by the host in index order: no
 * atomics, and a call's values are the same bits from run to run at a given grid (QSV_OPT_GRID_CAP).
 * Everything is checked before either deferred queue is flushed or anything is launched: QSV_EINVAL for a null handle, a
 * null array where k > 0, k < 0 or above the register's qubits, a repeated or out-of-range qubit, an entry of `inverse` that
 * is not finite, registers of different sizes or devices and -- qsv_layer_adjoint only -- psi and lambda whose memory meets
 * (the same handle included); QSV_ESTATE for a mode register.  k = 0 returns QSV_OK with 0 passes, no launch and `values`
 * untouched.  A valid call flushes both queues, synchronises lambda's (bra's) stream, sends its launches back to back on
 * psi's (ket's) stream, and ends with one copy of the partial sums and one synchronisation: it returns with both
 * registers finished.  Both calls work on views.  Ensembles (values per member) and density registers are not served. */
int qsv_layer_adjoint(qsv_state *psi, qsv_state *lambda, int k, const int *qubits, const double *inverse /* [k][2][2] complex */,
                      double *values /* [k][2][2] complex */, uint64_t *passes);
int qsv_layer_transition(qsv_state *bra, qsv_state *ket, int k, const int *qubits, double *values /* [k][2][2] complex */,
                         uint64_t *passes);

/* ---- reversible register arithmetic: classical maps on the value of a qubit register ---- */
/* A map acts on the integer y that m TARGET qubits spell (the first listed qubit the most significant, as in qsv_apply_qft),
 * may read the integer x of mx SOURCE qubits, which it leaves alone, and acts only where every control qubit is 1.  It is a
 * permutation of basis states, so applying it is one gather pass over the register -- the traffic of a copy, no floating-
 * point operation, bit-exact amplitudes.  M is the modulus (0 stands for 2^m); values y >= M stay where they are.
 *   QSV_ARITH_ADD         y -> (y + c) mod M                              m <= 32, mx = 0
 *   QSV_ARITH_MUL         y -> (a y) mod M, gcd(a, M) = 1                 m <= 32, mx = 0
 *   QSV_ARITH_ADD_REG     y -> (y + a x + c) mod M                        m, mx <= 32
 *   QSV_ARITH_MUL_POW     y -> (y a^x) mod M, gcd(a, M) = 1               m <= 32, 1 <= mx <= 24
 *   QSV_ARITH_XOR_LOOKUP  y -> y xor table[x], 2^mx entries below 2^m     m <= 32, 1 <= mx <= 24, no modulus
 *   QSV_ARITH_PERMUTE     y -> table[y], a bijection of 0 .. 2^m - 1      m <= 24, mx = 0, no modulus
 * qsv_arith_create validates everything, forms the inverse map of the same family (M - c, the modular inverse of a, the
 * table of inverse powers, the inverted table) and keeps both on `device`; an argument a kind does not use must be 0 / NULL.
 * QSV_EINVAL with a message for: an unknown kind; m or mx out of range; a, c or a table entry out of range; M < 2 or
 * M > 2^m; gcd(a, M) != 1; a table that is no bijection; a wrong table_len; a null pointer.
 * qsv_apply_arith applies the map (QSV_ARITH_INVERSE in flags: its inverse) with target[0 .. m-1], source[0 .. mx-1] (NULL
 * when mx = 0) and n_controls control qubits; a qubit may appear once in the three lists together.  QSV_EINVAL for null
 * pointers, a handle on another device, repeated or out-of-range qubits, unknown flag bits; QSV_ESTATE for a mode register:
 * each before the deferred queue is flushed or anything is launched.  The result is written to the register's spare buffer
 * and swapped in (copied back into a view, whose pointer stays).  passes (may be NULL) = kernel launches made: 1, or 0 for
 * a map that moves nothing (ADD with c = 0, MUL with a = 1, ...).  A handle may be used any number of times and by any
 * register on its device; destroy it after the last use has been enqueued -- qsv_arith_destroy waits for the device. */
#define QSV_ARITH_ADD 0
#define QSV_ARITH_MUL 1
#define QSV_ARITH_ADD_REG 2
#define QSV_ARITH_MUL_POW 3
#define QSV_ARITH_XOR_LOOKUP 4
#define QSV_ARITH_PERMUTE 5
#define QSV_ARITH_INVERSE 1
typedef struct qsv_arith qsv_arith;
int qsv_arith_create(int kind, int m, int mx, uint64_t a, uint64_t c, uint64_t modulus, const uint64_t *table,
                     uint64_t table_len, int device, qsv_arith **out);
int qsv_arith_destroy(qsv_arith *op);
int qsv_arith_info(const qsv_arith *op, int *kind, int *m, int *mx);
int qsv_apply_arith(qsv_state *st, qsv_arith *op, const int *target, const int *source, int n_controls,
                    const int *controls, int flags, uint64_t *passes);
/* Qubit-axis permutation of the ket: permute_tensor_product (numpy_quantum.py:227-240); the qubit
 * at position j moves to position new_ordering[j]. */
int qsv_permute(qsv_state *st, const int *new_ordering);

/* ---- measurement / insertion: replace M.apply (gates.py:165-186), Insert.apply (:145-153) - */
/* Projects qubit q on eig0 / eig1 (each 2 complex numbers, used UNCONJUGATED exactly as the
 * reference does), leaves p0 = |res0|^2, p1 = |res1|^2, picks outcome = forced if forced is 0/1,
 * else (u01 < p0/(p0+p1) ? 0 : 1), and shrinks the register to the normalised (n-1)-qubit ket. */
int qsv_measure(qsv_state *st, int q, const double eig0[4], const double eig1[4], int forced, double u01,
                int *outcome, double *p0, double *p1);
/* The two halves of qsv_measure, for callers that draw the outcome themselves between them (the Python
 * layer calls np.random.choice exactly as gates.py:183 does): the reduction without collapsing, and the
 * collapse onto `eig` with the result multiplied by `scale` (1/norm of the chosen branch). */
int qsv_measure_probs(qsv_state *st, int q, const double eig0[4], const double eig1[4], double *p0, double *p1);
int qsv_collapse(qsv_state *st, int q, const double eig[4], double scale);
/* Grows the register: new qubit with amplitudes amp[0..1] (complex) at position q. */
int qsv_insert(qsv_state *st, int q, const double amp[4]);

/* ---- read-out (npq.norm, numpy_quantum.py:131-132; |amp|^2 of chosen indices) -------------- */
int qsv_norm2(qsv_state *st, double *out);
int qsv_probabilities(qsv_state *st, const uint64_t *indices, int count, double *out);
/* <a|b> with a conjugated: the ket-ket branch of npq.fidelity (numpy_quantum.py:151-152). */
int qsv_inner(qsv_state *a, qsv_state *b, double *re, double *im);
/* <psi| P |psi> for the Pauli string P = paulis[0] on qubits[0] (x) paulis[1] on qubits[1] ... ('I','X','Y','Z'):
 * npq.expect (numpy_quantum.py:194-201) for tensor products of npq.PAULIS without building the 2^N operator. */
int qsv_expect_pauli(qsv_state *st, int k, const int *qubits, const char *paulis, double *re, double *im);
/* <psi| H |psi> for H = sum_t c_t P_t, every P_t a Pauli string as in qsv_expect_pauli (same letters, same qubit
 * order): term t is paulis[j] on qubits[j] for j in [term_offsets[t], term_offsets[t+1]), at most 64 letters, qubits
 * distinct within a term; coeffs holds n_terms interleaved complex c_t (NULL: all 1).  Terms that flip the same
 * qubits (equal X/Y positions: all Z-only terms and the identity; XX and YY on one pair) share passes over the
 * register: each pass reads every amplitude once, forms conj(psi[i ^ xmask]) psi[i] once per pair and accumulates up
 * to 8 terms from it, where qsv_expect_pauli reads the register twice per term.  All passes of a call are launched back
 * to back with one synchronisation at the end.  term_values (may be NULL) receives the n_terms real numbers
 * <psi|P_t|psi> in the caller's order, (re, im) = sum_t c_t <psi|P_t|psi>, passes (may be NULL) the number of kernel
 * launches made.  The whole list is validated before the first launch; n_terms = 0 gives 0 and no launch. */
int qsv_expect_pauli_sum(qsv_state *st, int n_terms, const int *term_offsets, const int *qubits, const char *paulis,
                         const double *coeffs, double *term_values, double *re, double *im, uint64_t *passes);
/* H as an operator, H = sum_t c_t P_t (layout of term_offsets / qubits / paulis as in qsv_expect_pauli_sum; coeffs holds
 * n_terms interleaved complex c_t and is required):  dst = H src, or dst += H src with accumulate != 0.  dst and src are
 * two qubit registers on one device whose memory does not meet (QSV_EINVAL otherwise, QSV_ESTATE for a mode register);
 * dst needs room for src's amplitudes (QSV_ENOMEM) and takes src's size, and must already have it to accumulate
 * (QSV_EINVAL).  Terms that flip the same qubits share a pass of at most 8 (csrc/qsv_pauli_plan.h): a pass reads src once,
 * builds the two complex factors of each pair {i, i ^ xmask} from the terms' signs and writes dst once; only the first
 * pass of a call that overwrites skips reading the old dst.  The whole list is validated before either deferred queue
 * is flushed; src's stream is synchronised, then the launches go back to back on dst's stream with no host
 * synchronisation.  n_terms = 0 zeroes dst (leaves it alone with accumulate).  passes (may be NULL) = kernel launches. */
int qsv_apply_pauli_sum(qsv_state *dst, qsv_state *src, int n_terms, const int *term_offsets, const int *qubits,
                        const char *paulis, const double *coeffs, int accumulate, uint64_t *passes);
/* <bra| P_t |ket> for every term and (re, im) = <bra| H |ket> = sum_t c_t <bra|P_t|ket>, arguments as in
 * qsv_expect_pauli_sum (coeffs NULL: all 1) except that term_values (may be NULL) receives n_terms interleaved COMPLEX
 * numbers.  Read-only; the registers have the same size and device and may be the same register, which gives
 * qsv_expect_pauli_sum's numbers.  Same grouping, launch order and deterministic host summation as there: all passes back
 * to back on bra's stream (ket's is synchronised first), one copy and one synchronisation per call. */
int qsv_pauli_transition_sum(qsv_state *bra, qsv_state *ket, int n_terms, const int *term_offsets, const int *qubits,
                             const char *paulis, const double *coeffs, double *term_values, double *re, double *im,
                             uint64_t *passes);
/* The backward (adjoint) walk over a rotation list.  On entry psi = R_{T-1} ... R_0 psi0 with R_t = exp(-i thetas[t]/2 P_t),
 * the list exactly as qsv_apply_pauli_rotations took it, and lambda is any other register of the same size on the same
 * device (memory must not meet).  For t = T-1 ... 0:  values[2t], values[2t+1] = <lambda| P_t |psi>, then
 * psi <- R_t^dagger psi and lambda <- R_t^dagger lambda.  On exit psi holds psi0 up to rounding and lambda holds
 * U^dagger lambda: BOTH registers are consumed / rewound.  With lambda = H psi the gradient of E = <psi|H|psi> is
 * dE/dtheta_t = Im values[t].  The passes are those of the forward plan taken last first
 * (csrc/qsv_pauli_rotation_plan.h), so passes (may be NULL) equals the forward count and the cost does not grow with the
 * rotations per pass; there is no host synchronisation between passes except where the per-workgroup partial sums of a
 * long list on a large register outgrow a fixed scratch budget (csrc/qsv_pauli.hip).  Validation, flushes of both deferred
 * queues and streams as in qsv_apply_pauli_sum: lambda's stream is synchronised, the launches go on psi's, and the call
 * returns with both registers finished.  n_terms = 0 does nothing. */
int qsv_pauli_rotations_adjoint(qsv_state *psi, qsv_state *lambda, int n_terms, const int *term_offsets, const int *qubits,
                                const char *paulis, const double *thetas, double *values, uint64_t *passes);
/* Multi-register BLAS-1 passes (csrc/qsv_krylov.hip): what Lanczos and Krylov evolution need next
 * to qsv_apply_pauli_sum.  All operands are qubit registers (QSV_ESTATE for a mode register) on one device and of one
 * size (QSV_EINVAL); null handles, null arrays and negative counts are refused.  Everything is validated before any
 * deferred queue is flushed; then every operand's queue is flushed, the streams of the registers that are only read are
 * synchronised, and the launches go back to back on dst's (y's) stream.  passes (may be NULL) = kernel launches.
 *
 * qsv_lincomb: dst = beta dst + sum_k c_k src_k, k < n_src; coeffs holds n_src interleaved complex c_k, beta =
 * (beta_re, beta_im).  A pass takes up to 8 sources, loads each once (exactly as many streams as it has sources),
 * loads dst once only if its beta is not exactly 0, and stores dst once: ceil(n_src / 8) passes, at least one; the first
 * uses beta, the others 1.  With beta == 0 the old dst is never read (NaN in it does not spread) and dst takes the
 * sources' size if it has the room (QSV_ENOMEM), as in qsv_copy; otherwise it must have that size already.  n_src = 0
 * scales dst by beta (zeroes it for beta == 0).  dst's memory must not meet a source's (address ranges are compared:
 * QSV_EINVAL; fold dst's own coefficient into beta); sources may repeat and overlap.  norm2 (may be NULL) receives
 * ||dst||^2 after the update, formed in the last pass from the values it stores -- no extra read of dst -- and summed
 * on the host in index order; asking for it costs one copy and one synchronisation.
 *
 * qsv_inner_many: values[2k], values[2k+1] = <x_k|y> (x_k conjugated), k < n_x.  A pass reads y once and up to 8 x_k
 * once each; all passes are launched back to back, then one copy and one synchronisation per call.  One partial per
 * workgroup and x_k, summed by the host in index order: the same call gives the same bits.  x_k may be y.  Read-only. */
int qsv_lincomb(qsv_state *dst, double beta_re, double beta_im, int n_src, qsv_state *const *srcs, const double *coeffs,
                double *norm2, uint64_t *passes);
int qsv_inner_many(qsv_state *y, int n_x, qsv_state *const *xs, double *values, uint64_t *passes);

/* ---- real diagonal operators on the device (csrc/qsv_diagonal.hip) ----
 * A qsv_diag holds 2^n doubles d[i] in device memory, indexed exactly like the register (qubit q is bit n-1-q of i):
 * a classical cost function, an oracle on any marked set, the ZZ part of an Ising or MaxCut Hamiltonian.  It is owned
 * by the library and has a stream of its own (default: the null stream).  Every call on a register and a diagonal is ONE
 * pass over the register, whatever the number of terms the diagonal was built from. */
typedef struct qsv_diag qsv_diag;

/* Allocate, zero-filled; the sizes qsv_create accepts. */
int qsv_diag_create(int n_qubits, int device, qsv_diag **out);
int qsv_diag_destroy(qsv_diag *d);
int qsv_diag_set_stream(qsv_diag *d, void *hip_stream);
int qsv_diag_num_qubits(const qsv_diag *d, int *n_qubits);
/* Only QSV_OPT_GRID_CAP (max workgroups of the diagonal's own kernels); anything else is QSV_EINVAL. */
int qsv_diag_set_option(qsv_diag *d, int option, int64_t value);
/* Name of the kernel the most recent qsv_diag_set_pauli_sum / qsv_diag_extrema launched. */
int qsv_diag_last_kernel(const qsv_diag *d, char *buf, size_t buf_len);
/* Windows [offset, offset + count) of doubles, bounds-checked; the host buffer is only touched during the call. */
int qsv_diag_upload(qsv_diag *d, const double *host, uint64_t offset, uint64_t count);
int qsv_diag_download(qsv_diag *d, double *host, uint64_t offset, uint64_t count);
/* d[i] = (accumulate ? d[i] : 0) + sum_t c_t (-1)^popcount(i & zmask_t).  Term layout as in qsv_expect_pauli_sum, but
 * coeffs holds n_terms REAL numbers (NULL: all 1) and only the letters I and Z are accepted (X, Y: QSV_EINVAL); qubits in
 * range and distinct within a term, at most 64 letters; everything is validated before any launch.  One write pass for
 * any number of terms: masks and coefficients go to the device once as a table that every thread walks in the caller's
 * order, one rounded addition per term (c_t * (+-1) is exact), so the result equals the same loop in float64 on the
 * host bit for bit.  n_terms = 0 zeroes the vector (leaves it alone with accumulate); the empty term adds a constant.
 * passes (may be NULL) = kernel launches: 1, or 0 where nothing had to be done. */
int qsv_diag_set_pauli_sum(qsv_diag *d, int n_terms, const int *term_offsets, const int *qubits, const char *paulis,
                           const double *coeffs, int accumulate, uint64_t *passes);
/* Smallest and largest entry and their indices in one read pass; ties go to the lowest index; any pointer may be NULL. */
int qsv_diag_extrema(qsv_diag *d, double *min, uint64_t *argmin, double *max, uint64_t *argmax);
/* Register x diagonal passes.  Rules for all of them, as for qsv_lincomb and qsv_apply_pauli_sum: null handles are
 * refused; mode registers give QSV_ESTATE; registers and diagonal must be on one device and of one size (QSV_EINVAL);
 * everything is validated before any deferred queue is flushed, then every register's queue is flushed; the streams of
 * read-only operands are synchronised, the diagonal's too when it is not the stream that launches, and the launches go
 * on the written register's stream (st's / bra's for the read-only calls).  Reductions leave one partial per workgroup
 * (at most 1024) and slot, and the host sums them in index order after one copy and one synchronisation: the same call
 * gives the same bits.
 *
 * qsv_apply_diag_phase: psi[i] *= exp(-i gamma d[i]) in place; the sine and cosine are formed in double on the device.
 * qsv_apply_diag_mul: dst = c d.src, or dst += c d.src with accumulate, c = (c_re, c_im).  dst needs room for src's
 *   amplitudes (QSV_ENOMEM), takes src's size, and must have it already to accumulate; their memory must not meet, except
 *   that dst == src is allowed when not accumulating (D psi in place).  Without accumulate the old dst is never read.
 * qsv_expect_diag: out = { sum p_i, sum p_i d_i, sum p_i d_i^2, sum_{d_i <= *threshold} p_i }, p_i = |psi_i|^2;
 *   threshold may be NULL (then out[3] = 0).  Read-only.
 * qsv_diag_transition: (re, im) = <bra| D |ket>.  Read-only; the same register may be passed twice.
 * qsv_diag_phase_adjoint: (re, im) = <lambda| D |psi>, then psi *= exp(-i gamma d) and lambda *= exp(-i gamma d), all in
 *   one pass with one sincos per amplitude.  D commutes with the phase, so the value is the same before and after it.
 *   psi and lambda are two registers whose memory does not meet.  Both are finished when the call returns. */
int qsv_apply_diag_phase(qsv_state *st, qsv_diag *d, double gamma);
int qsv_apply_diag_mul(qsv_state *dst, qsv_state *src, qsv_diag *d, double c_re, double c_im, int accumulate);
int qsv_expect_diag(qsv_state *st, qsv_diag *d, const double *threshold, double *out);
int qsv_diag_transition(qsv_state *bra, qsv_state *ket, qsv_diag *d, double *re, double *im);
int qsv_diag_phase_adjoint(qsv_state *psi, qsv_state *lambda, qsv_diag *d, double gamma, double *re, double *im);

/* ---- noise: Kraus channels on kets and Pauli traces of density registers (csrc/qsv_channel.hip) ----
 * A qsv_channel holds 1 <= n_kraus <= 16 Kraus operators K_j on k = 1 or 2 qubits (n_kraus x 2^k x 2^k complex, row-major,
 * qubits[0] the most significant leg) and their effects E_j = K_j^dagger K_j in device memory, so a call uploads nothing.
 * Trace preservation is not demanded: branch weights are always taken relative to their sum, so a call preserves the
 * register's norm whatever it was.  A channel whose every E_j equals p_j I (to 16 eps per entry) is marked mixed-unitary
 * at creation: bit flip, phase flip, depolarising, any Pauli channel.  The 16 eps are ABSOLUTE, on purpose: the operators of
 * a trace-preserving channel have entries of at most 1, and the Python layer applies the same rule without a device.  A
 * list that is not normalised should be scaled to unit weight first: with entries far above 1 its own rounding may
 * keep it off the queued path (slower, never wrong); with entries below about 1e-8 every list is taken for mixed-unitary. */
typedef struct qsv_channel qsv_channel;
int qsv_channel_create(int k, int n_kraus, const double *kraus, int device, qsv_channel **out);
int qsv_channel_destroy(qsv_channel *c);
int qsv_channel_info(const qsv_channel *c, int *k, int *n_kraus, int *mixed_unitary);  /* any output may be NULL */
/* One quantum-trajectory step: psi <- K_j psi sqrt(total / w_j), w_j = <psi| E_j |psi>, total = sum_j w_j, where j = forced
 * if forced >= 0, else the first j with w_0 + ... + w_j > u01 total (the last j with w_j > 0 if rounding leaves none).  A
 * forced branch of weight 0 leaves an all-zero register and logs probability 0; no inf or nan is produced.
 *  - Mixed-unitary channel: the weights are the p_j whatever the state, so the host picks j and K_j / sqrt(p_j) goes through
 *    qsv_apply_1q / qsv_apply_2q: no reduction, no flush -- on a deferring register the gate joins the queue.
 *  - Any other channel flushes the queue and takes two passes over the register: a read pass that leaves the reduced
 *    density matrix of the target qubits in device memory, a one-workgroup kernel that forms the weights, takes the branch
 *    and writes the scaled K_j to a device slot, and an in-place update pass that reads that slot.  Everything is enqueued
 *    on the register's stream; the call returns without waiting and downloads nothing.
 * QSV_EINVAL for null pointers, u01 outside [0, 1), forced outside -1 .. n_kraus - 1, qubits repeated or out of range, a
 * channel on another device; QSV_ESTATE for a mode register: each before any launch and with the deferred queue untouched.
 * Every call appends (j, w_j / total) to the register's branch log, in call order.  The device part of the log has a fixed
 * number of slots; a call that finds it full drains it to host memory first -- the only time this call synchronises. */
int qsv_apply_channel(qsv_state *st, qsv_channel *c, const int *qubits, double u01, int forced);
/* The branch log: *count = entries pending.  With capacity >= *count they are copied out (after a synchronisation of the
 * register's stream) and the log is cleared; with a smaller capacity nothing is copied or cleared.  Pending gates of a
 * deferring register stay queued.  qsv_destroy frees the log. */
int qsv_channel_log_read(qsv_state *st, int32_t *branches, double *probs, uint64_t capacity, uint64_t *count);
/* tr(P_t rho) for every Pauli string of a list (layout of term_offsets / qubits / paulis as in qsv_expect_pauli_sum, qubits
 * numbered 0 .. n-1) and a density matrix held row-major as a 2n-qubit register: values[2t], values[2t+1] =
 * i^nY sum_k (-1)^popcount(k & zmask_t) rho[k][k ^ xmask_t].  One launch for all terms, one workgroup per term, each reading
 * 2^n of the 4^n entries; the empty term gives the trace.  Flushes the queue; QSV_EINVAL for a register with an odd number
 * of qubits.  The whole list is validated before the flush. */
int qsv_density_expect_paulis(qsv_state *rho, int n_terms, const int *term_offsets, const int *qubits, const char *paulis,
                              double *values);
/* ---- trajectory ensembles: many shots of a noisy circuit in one register (csrc/qsv_ensemble.hip) ----
 * An ensemble is a register of n_total qubits that the library allocated (qsv_create), read as 2^(n_total - member_qubits)
 * MEMBERS of member_qubits qubits each: member m holds the amplitudes [m 2^member_qubits, (m + 1) 2^member_qubits), i.e. the
 * member index is the leading n_total - member_qubits qubits of the register and member qubit q is register qubit
 * q + (n_total - member_qubits).  Any gate on register qubits of the member part acts on every member alike, deferred gates
 * included; the calls below are the steps that differ from member to member.  `qubits` are MEMBER qubits, 0 .. member_qubits - 1.
 *  - qsv_ensemble_broadcast copies member 0 into every other member (device-to-device, the filled part doubling).
 *  - qsv_ensemble_apply_channel is one trajectory step of every member at once, each with its own draw u01[m] and its own
 *    forced[m] (forced = NULL or forced[m] = -1: draw): the branch rule of qsv_apply_channel member by member.  A read pass
 *    leaves every member's reduced density matrix of the target qubits in parts, a select kernel adds a member's parts in
 *    index order, takes the member's branch and writes K_j sqrt(total / w_j) to the member's matrix slot, an in-place update
 *    pass multiplies every group of amplitudes by the matrix of its own member.  For a mixed-unitary channel the weights are
 *    the stored p_j: no read pass.  How a member's sums are formed depends on member_qubits, the target qubits and
 *    QSV_OPT_GRID_CAP only, never on the number of members: a member's results are bit-identical wherever it sits.
 *    Every call flushes the deferred queue (its matrix differs per member, so it cannot be queued), is enqueued on the
 *    register's stream and returns without waiting; the draws travel through a pinned ring.
 *  - Every call appends one STEP, (j, w_j / total) per member, to the register's ensemble log.  The device part holds 256
 *    steps (fewer beyond 16384 members); a call that finds it full drains it first -- the only time the call synchronises.
 *    qsv_ensemble_log_read: *steps = steps pending; with capacity_steps >= *steps they are copied out as [steps][members]
 *    and the log is cleared, otherwise nothing is copied or cleared.  The ensemble log and the log of qsv_apply_channel are
 *    separate and each keeps its own order.  member_qubits may change between calls only while the ensemble log is empty
 *    (QSV_ESTATE otherwise).
 *  - qsv_ensemble_norm2: out[m] = <psi_m|psi_m>.  qsv_ensemble_expect_pauli_sum: values[m] = sum_t coeffs[t] <psi_m|P_t|psi_m>
 *    (coeffs real, one per term, NULL = all 1; term list as in qsv_expect_pauli_sum) and, if term_values is given,
 *    term_values[m * n_terms + t]; the passes of qsv_expect_pauli_sum, each followed by a per-member sum on the device in a
 *    fixed order; one synchronisation at the end.  Both flush the queue.
 * QSV_EINVAL for null pointers, member_qubits outside k .. n_total (1 .. n_total for the read-outs, 0 .. n_total for the
 * broadcast), target or term qubits >= member_qubits or repeated, any u01[m] outside [0, 1), any forced[m] outside
 * -1 .. n_kraus - 1, a channel on another device, a view; QSV_ESTATE for a mode register: each before any launch and with the
 * deferred queue untouched. */
int qsv_ensemble_broadcast(qsv_state *st, int member_qubits);
int qsv_ensemble_apply_channel(qsv_state *st, int member_qubits, qsv_channel *c, const int *qubits, const double *u01 /* members */,
                               const int *forced /* NULL or members, -1 = draw */);
int qsv_ensemble_log_read(qsv_state *st, int32_t *branches, double *probs /* [steps][members] */, uint64_t capacity_steps, uint64_t *steps);
int qsv_ensemble_norm2(qsv_state *st, int member_qubits, double *out /* members */);
int qsv_ensemble_expect_pauli_sum(qsv_state *st, int member_qubits, int n_terms, const int *term_offsets, const int *qubits, const char *paulis,
                                  const double *coeffs, double *values /* members */, double *term_values /* NULL or [members][n_terms] */);
/* ---- ensembles: per-member measurement, classical bits and feed-forward (csrc/qsv_ensemble.hip) ----
 * Every member owns one uint64_t of CLASSICAL BITS, zero at creation, in a device allocation of its own that is made on the
 * first of the calls below, re-made and zeroed when member_qubits changes (only while the ensemble log is empty, QSV_ESTATE
 * otherwise) and freed with the register.
 *  - qsv_ensemble_measure is a projective measurement of member qubit `qubit` in every member at once; the qubit STAYS in the
 *    register.  eig_s = (Re, Im) of e_s[0], e_s[1].  phi_s = (e_s^T on the qubit) psi_m with the eigenvectors unconjugated, as
 *    in qsv_measure; w_s = |phi_s|^2, total = w_0 + w_1.  The outcome is forced[m] if it is >= 0, else the first s with
 *    w_0 + .. + w_s > u01[m] total (the last positive one if rounding leaves none): the branch rule of
 *    qsv_ensemble_apply_channel.  The member becomes v_s (x) phi_s sqrt(total / w_s) with v_s = conj(e_s) (after = 0) or
 *    |0> (after = 1); a forced outcome of weight 0 zeroes the member and logs probability 0; no inf or nan is produced.
 *    bit >= 0: bit `bit` of the member's word becomes the outcome.  The call appends one STEP (outcome, w_s / total) to the
 *    ensemble log exactly like a channel call, so qsv_ensemble_log_read keeps call order across channels and measurements.
 *    Three launches: the read pass and the update pass of a one-qubit channel call, and between them k_ens_measure_select,
 *    which has the eigenvectors in its kernel arguments: nothing is uploaded but the draws, through the pinned ring.
 *  - qsv_ensemble_apply_conditional applies the k-qubit matrix (k = 1 or 2) to the members whose word satisfies
 *    (word & all_of) == all_of && (word & none_of) == 0; all others are left bit-identical and their amplitudes are neither
 *    read nor written.  Both masks 0: every member.  One launch, nothing logged.
 *  - qsv_ensemble_bits_read copies the words out (one copy, one synchronisation); qsv_ensemble_bits_write sets them
 *    (bits = NULL: all zero; one copy, the words are staged before the call returns).
 * measure and apply_conditional flush the deferred queue, are enqueued on the register's stream and return without waiting.
 * QSV_EINVAL for null pointers, member_qubits outside k .. n_total (1 .. n_total for measure, 0 .. n_total for the bits), qubits
 * >= member_qubits or repeated, any u01[m] outside [0, 1), any forced[m] outside -1 .. 1, bit outside -1 .. 63, after outside
 * 0 .. 1, k outside 1 .. 2, all_of & none_of != 0, a view; QSV_ESTATE for a mode register: each before any launch and with the
 * deferred queue untouched. */
int qsv_ensemble_measure(qsv_state *st, int member_qubits, int qubit, const double eig0[4], const double eig1[4],
                         int after /* 0 keep, 1 reset */, int bit /* 0..63, -1 = none */,
                         const double *u01 /* members */, const int *forced /* NULL or members: -1 draw, 0, 1 */);
int qsv_ensemble_apply_conditional(qsv_state *st, int member_qubits, int k /* 1 or 2 */, const int *qubits,
                                   const double *matrix /* 4^k complex, row-major, qubits[0] most significant */,
                                   uint64_t all_of, uint64_t none_of);
int qsv_ensemble_bits_read(qsv_state *st, int member_qubits, uint64_t *bits /* members */);
int qsv_ensemble_bits_write(qsv_state *st, int member_qubits, const uint64_t *bits /* NULL = clear all */);
/* ---- parameter ensembles: per-member angles, matrices and cost phases (csrc/qsv_sweep.hip) ----
 * The members of an ensemble run the same circuit at different parameter points.  Notation as above: members =
 * 2^(n_total - member_qubits), `qubits` are MEMBER qubits, qsv_diag objects have member_qubits qubits (not n_total).
 *  - qsv_ensemble_apply_pauli_rotations: member m becomes what qsv_apply_pauli_rotations would make of it alone with row m of
 *    thetas.  Same term list, same planner (on member-local masks), same *passes -- which never depends on the number of
 *    members; the identity string (or an empty one) is a per-member global phase.  cos(theta / 2) and sin(theta / 2) are
 *    formed on the host as in qsv_apply_pauli_rotations and travel as one table [members][n_terms][2]; a member's bits are
 *    those of a register of its own, wherever it sits.  n_terms = 0 launches nothing.
 *  - qsv_ensemble_apply_matrices: member m takes matrices[m] on `qubits` (k = 1 or 2).  Unitarity is not demanded; nothing is
 *    drawn or logged.  The update pass of qsv_ensemble_apply_channel with the matrix slots filled by the caller.
 *  - qsv_ensemble_apply_diag_phase: psi_m[i] *= exp(-i gammas[m] d[i]), the arithmetic of qsv_apply_diag_phase.
 *  - qsv_ensemble_expect_diag: out[m] = { sum p, sum p d, sum p d^2, sum_{d <= *threshold} p } over member m, p = |psi_m[i]|^2
 *    (slot 3 is 0 when threshold is NULL).  Read-only; a member's sums depend on member_qubits and QSV_OPT_GRID_CAP only; one
 *    copy and one synchronisation at the end, as qsv_ensemble_norm2.
 * After its checks a call flushes the deferred queue, is enqueued on the register's stream and (the read-out apart) returns
 * without waiting for its kernels; the caller's arrays may be reused on return.  The diagonal's stream is synchronised as in
 * qsv_apply_diag_phase.
 * QSV_EINVAL for null pointers (passes and threshold may be NULL), a view, member_qubits outside k .. n_total for
 * apply_matrices and 0 .. n_total for the others, a qubit >= member_qubits or repeated, k outside 1 .. 2, a diagonal of another
 * size or on another device, any angle, gamma, matrix entry or threshold that is not finite; QSV_ESTATE for a mode register, or
 * where apply_matrices would change the member size while the ensemble log holds steps: each before any launch and with the
 * deferred queue untouched. */
int qsv_ensemble_apply_pauli_rotations(qsv_state *st, int member_qubits, int n_terms, const int *term_offsets,
                                       const int *qubits, const char *paulis,
                                       const double *thetas /* [members][n_terms] */, uint64_t *passes);
int qsv_ensemble_apply_matrices(qsv_state *st, int member_qubits, int k /* 1 or 2 */, const int *qubits,
                                const double *matrices /* [members][4^k] complex, row-major, qubits[0] most significant */);
int qsv_ensemble_apply_diag_phase(qsv_state *st, int member_qubits, qsv_diag *d, const double *gammas /* members */);
int qsv_ensemble_expect_diag(qsv_state *st, int member_qubits, qsv_diag *d, const double *threshold /* NULL or one value */,
                             double *out /* [members][4] */);
/* ---- per-member adjoint walks (csrc/qsv_ensemble_adjoint.hip) ----
 * Two ensembles of one shape, psi and lambda (a and b), member by member; notation as above.
 *  - qsv_ensemble_inner: values[m] = <a_m|b_m> (a conjugated), interleaved complex.  Read-only; a may be b, and <a_m|a_m> has an
 *    imaginary part of exactly 0.  One read pass, one copy and one synchronisation.
 *  - qsv_ensemble_apply_diag_mul: dst_m[i] = d[i] src_m[i], qsv_apply_diag_mul with the coefficient 1 and a diagonal of
 *    member_qubits qubits: lambda = D psi for the cost-phase walk.  dst may be src; otherwise their memory must not meet.  One
 *    pass on dst's stream, no synchronisation.
 *  - qsv_ensemble_pauli_rotations_adjoint is qsv_pauli_rotations_adjoint member by member with row m of thetas: for t = T-1 .. 0,
 *    values[m][t] = <lambda_m|P_t|psi_m>, then psi_m <- R_t(thetas[m][t])^dagger psi_m and the same for lambda_m.  Term list,
 *    planner and *passes are those of qsv_ensemble_apply_pauli_rotations; the passes are taken last first.  Every pass is
 *    followed by a per-member sum on the device; there is no host synchronisation between passes, and one copy and one
 *    synchronisation at the end whatever the list length.
 *  - qsv_ensemble_diag_phase_adjoint: values[m] = <lambda_m|D|psi_m> of the registers as they come in, then psi_m[i] *=
 *    exp(-i gammas[m] d[i]) and the same for lambda_m, in one pass (the arithmetic of qsv_diag_phase_adjoint); d has
 *    member_qubits qubits.
 * After either walk psi_m and lambda_m are bit for bit what the single-register call leaves on registers of the member's size
 * with the member's angles.  A member's values depend on member_qubits, the term list and QSV_OPT_GRID_CAP only: they are
 * bit-identical wherever the member sits and for any number of members, and agree with the single-register values to
 * rounding (the order of the sums differs).  Sums and partials live in psi's (a's) ensemble workspace.  After the checks both
 * deferred queues are flushed, lambda's (b's) stream is synchronised and the launches go on psi's (a's).  n_terms = 0
 * launches nothing.
 * QSV_EINVAL for null pointers (passes may be NULL), a view, member_qubits outside 0 .. n_total, a qubit >= member_qubits or
 * repeated, bad letters, offsets or lengths, any angle or gamma that is not finite, registers of different sizes or devices or
 * (the two walks) whose memory meets, a diagonal of another size or device; QSV_ESTATE for a mode register, or a call that
 * would change the member size while psi's (a's) ensemble log holds steps: each before any launch and with both deferred
 * queues untouched. */
int qsv_ensemble_inner(qsv_state *a, qsv_state *b, int member_qubits, double *values /* [members] complex */);
int qsv_ensemble_apply_diag_mul(qsv_state *dst, qsv_state *src, int member_qubits, qsv_diag *d);
int qsv_ensemble_pauli_rotations_adjoint(qsv_state *psi, qsv_state *lambda, int member_qubits, int n_terms,
                                         const int *term_offsets, const int *qubits, const char *paulis,
                                         const double *thetas /* [members][n_terms] */,
                                         double *values /* [members][n_terms] complex */, uint64_t *passes);
int qsv_ensemble_diag_phase_adjoint(qsv_state *psi, qsv_state *lambda, int member_qubits, qsv_diag *d,
                                    const double *gammas /* [members] */, double *values /* [members] complex */);
/* Reduced density matrix of the k <= 6 qubits `qubits` (all others traced out) in one read pass over the register:
 * rho[i][j] = sum_rest psi[i, rest] conj(psi[j, rest]), written row-major as 4^k complex numbers, qubits[0] the most
 * significant bit of i and j.  What a caller of the reference gets from npq.ket2dm (numpy_quantum.py:110-113)
 * followed by a partial trace -- without the 2^N x 2^N matrix. */
int qsv_reduced_density(qsv_state *st, int k, const int *qubits, double *rho);
/* ---- subsystem read-out past six qubits (csrc/qsv_subsystem.hip) ----
 * The reduced state of 1 <= k <= min(n, 12) distinct qubits of the n-qubit ket, LEFT ON THE DEVICE: `rho` is a register of
 * 2k qubits that the library allocated (qsv_create; not a view, not `ket`) on the same device, and receives the 2^k x 2^k
 * matrix row-major in the layout of a density register, row and column index bit k-1-j <-> qubits[j] (the order of
 * qsv_reduced_density); every other qubit is traced out.  rho_A = M M^dagger runs on the f64 matrix cores, the output cut
 * into 64-row blocks over workgroups and the traced index into slices; registers below 14 qubits and shapes with fewer than
 * 64 traced settings take a per-entry kernel (qsv_last_kernel of the ket: k_subsys_tile / k_subsys_entry).  Both
 * registers' queues are flushed; the work is enqueued on the ket's stream and the call does not wait for it (if `rho` lives
 * on another stream, that stream is waited for first, and ordering its later work is the caller's).  The matrix as stored
 * is exactly Hermitian with a real diagonal, and sums are taken in a fixed order: two calls give the same bits.
 * QSV_EINVAL for null pointers, k outside 1 .. min(n, 12), qubits repeated or out of range, a `rho` of another size, on
 * another device, equal to `ket` or a view; QSV_ESTATE for a mode register: each before any launch. */
int qsv_reduced_density_state(qsv_state *ket, int k, const int *qubits, qsv_state *rho);
/* The marginal distribution of 1 <= k <= min(n, 26) distinct qubits: out[i] = sum over the other qubits of |amp|^2, 2^k
 * doubles on the host, index bit k-1-j <-> qubits[j]; k = n is the permuted |amplitude|^2.  One read pass over the
 * register, fixed summation order, one synchronisation (k_marginal_stream where the traced index is long, else
 * k_marginal_entry). */
int qsv_marginal_probabilities(qsv_state *st, int k, const int *qubits, double *out);
/* <a| rho |a> for an n-qubit ket `ket` and a density matrix `rho` held row-major as a 2n-qubit register (the layout
 * Gate.apply uses for U rho U^dagger): the ket / density-matrix branches of npq.fidelity (numpy_quantum.py:153-156).
 * npq.purity (numpy_quantum.py:164-166) of such a register is qsv_norm2: tr(rho rho) = sum |rho_ij|^2 for a
 * hermitian rho. */
int qsv_expect_density(qsv_state *ket, qsv_state *rho, double *re, double *im);
/* Draw `shots` computational-basis outcomes from |amp|^2 by inverse-CDF sampling: out[s] is the smallest basis
 * index whose cumulative probability exceeds u[s] * norm^2 (u[s] in [0, 1), drawn by the caller).  The register
 * is not collapsed.  Equivalent to measuring every qubit with MZ (gates.py:188-190) on independent copies.  An index of
 * |amp|^2 = 0 is never returned: where rounding lets a draw fall past the last amplitude of positive weight that could
 * hold it, that amplitude is the answer. */
int qsv_sample(qsv_state *st, int shots, const double *u, uint64_t *out);

/* ---- d-level mode registers: the "d x d (d^2 x d^2) operator along mode axes" contraction of
 *      cv_simulator (np.tensordot at simulators/cv_simulator/utils.py:15,37; gates.py:73,160) --- */
int qsv_create_qudit(int n_modes, int d, int device, qsv_state **out);
int qsv_create_qudit_view(int n_modes, int d, int device, void *dev_amps, uint64_t capacity_amps,
                          void *hip_stream, qsv_state **out);
int qsv_qudit_shape(const qsv_state *st, int *n_modes, int *d);
int qsv_apply_mode1(qsv_state *st, int mode, const double *m /* d x d */);
int qsv_apply_mode1_diag(qsv_state *st, int mode, const double *diag /* d */);
int qsv_apply_mode2(qsv_state *st, int mode0, int mode1, const double *m /* d^2 x d^2 */);
int qsv_apply_mode2_diag(qsv_state *st, int mode0, int mode1, const double *diag /* d^2 */);
/* Sparse two-mode map: output plane point (i0, i1) = sum_k vals[(i0*d+i1)*nnz + k] * input plane point
 * cols[(i0*d+i1)*nnz + k] (= j0*d+j1; negative = unused slot).  The bilinear resampling of the (q1, q2)
 * plane that BS and CX do per bond pair with RegularGridInterpolator (cv_simulator/gates.py:74-80,187-189)
 * is nnz = 4; SWAP (gates.py:48-55) is nnz = 1. */
int qsv_apply_mode2_gather(qsv_state *st, int mode0, int mode1, int nnz, const int32_t *cols, const double *vals);
/* Block-diagonal two-mode operator, in place: `nblocks` disjoint sets of (d, d)-plane points, set k holding
 * sizes[k] (<= 32) points listed in plane_indices (= j0*d+j1 in (mode0, mode1) order, concatenated), mixed by
 * the dense sizes[k] x sizes[k] complex matrix found at the matching position of `mats` (row-major, concatenated).
 * Plane points in no block are left alone.  A Fock-basis beam splitter (it conserves n_a + n_b) is 2d-1 blocks. */
int qsv_apply_mode2_blocks(qsv_state *st, int mode0, int mode1, int nblocks, const int32_t *sizes,
                           const int32_t *plane_indices, const double *mats);
/* Homodyne read-out (Mq.apply, cv_simulator/gates.py:90-117): probs[j] = sum over the other modes of
 * |amp|^2 at level j of `mode` (the diagonal of partial_density_mps, mps.py:176-190, without the dq factors);
 * project keeps level `level` of `mode`, multiplies by `scale` and removes the mode. */
int qsv_mode_marginal(qsv_state *st, int mode, double *probs /* d */);
int qsv_mode_project(qsv_state *st, int mode, int level, double scale);
/* New mode with amplitudes vec[0..d) (complex) at position `mode` (Insert.apply, gates.py:24-45). */
int qsv_mode_insert(qsv_state *st, int mode, const double *vec /* d */);
/* out[l, :, r] = M @ in[l, :, r] on a raw (L, d_in, R) device tensor -> (L, d_out, R): the exact
 * tensordot+moveaxis of whittaker_shannon / rotation (cv_simulator/utils.py:9-39) on an MPS site. */
int qsv_tensor_apply_axis(int device, void *hip_stream, const void *dev_in, void *dev_out, uint64_t L,
                          uint64_t d_in, uint64_t d_out, uint64_t R, const double *m /* d_out x d_in */);
/* Same with the operator already in device memory (the reference's gates build their d x d matrix once in
 * __init__, cv_simulator/gates.py:48-52,61-66, and reuse it for every apply): nothing is uploaded and the call
 * is asynchronous on `hip_stream`.  Grids of >= 64 points go to rocBLAS zgemm when it can be loaded. */
int qsv_tensor_apply_axis_dev(int device, void *hip_stream, const void *dev_in, void *dev_out, uint64_t L,
                              uint64_t d_in, uint64_t d_out, uint64_t R, const void *dev_m /* d_out x d_in */);

/* ---- matrix-product-state sites (cv_simulator/mps.py:102-201) ------------------------------
 * The reference keeps a CV register as a list of (chi_l, d, chi_r) site tensors and, for every two-mode gate,
 * contracts two neighbours, maps the (q_left, q_right) plane and splits the result again with a truncated SVD
 * (cv_simulator/gates.py:48-84,151-192).  These entry points are that update on raw device tensors: every pointer
 * is device memory (row-major complex128 unless noted), every call runs on `hip_stream` of `device`; calls that
 * return data to the host synchronise the stream.  GEMM and SVD come from rocBLAS / rocSOLVER (bound by dlopen);
 * without them these calls return QSV_EHIP.
 *
 * Threading.  Every (device, stream) pair has a context of its own inside the library: a rocBLAS handle bound to that
 * stream, a grow-only scratch pool and the state of the QSV_RANK_NEEDS_OMEGA protocol.  Calls on distinct streams may
 * run concurrently from distinct threads; calls on one stream must come from one thread at a time.  No lock is held
 * across a kernel launch, a library call or a stream synchronisation.  A call waits for its own stream and frees no
 * device memory: a pool that grows keeps its old block until the context is released, and so does the shared cache of
 * the fixed probe matrices of the splits' low-rank route when it evicts one.  Only the two release calls below free
 * memory, and hipFree waits for the whole device: call them between batches, not while other streams work.  Run independent MPS
 * simulations side by side by giving each its own stream (quantum_computations_amd.concurrent.map_on_streams). */
/* C (m x n) = op(A) . op(B); op: 0 = as stored, 1 = transpose, 2 = conjugate transpose; A is (m x k) or, with an
 * op, (k x m); likewise B.  np.tensordot(m1, m2, (2, 0)) (gates.py:68) and the environment recursions of
 * MPS.norm / partial_density_mps (mps.py:166-190). */
int qsv_tensor_gemm(int device, void *hip_stream, int op_a, int op_b, uint64_t m, uint64_t n, uint64_t k,
                    const void *dev_a, const void *dev_b, void *dev_c);
/* tensor_svd (mps.py:52-97) of the (rows x cols) matrix `dev_theta` (destroyed): m1 = U[:, :r] sqrt(S[:r]) as
 * (rows x r), m2 = sqrt(S[:r]) Vh[:r, :] as (r x cols), r chosen by the reference's rule -- drop the longest tail of
 * singular values whose sum stays <= max(abs_err, rel_err * sum(S)), then cap at max_bond_dim (< 0 = no cap).
 * `capacity` = the r the output buffers can hold; *rank = r; singular_values (host, min(rows, cols) doubles) may be
 * NULL. */
int qsv_tensor_svd_split(int device, void *hip_stream, void *dev_theta, uint64_t rows, uint64_t cols,
                         int64_t max_bond_dim, double abs_err, double rel_err, void *dev_m1, void *dev_m2,
                         uint64_t capacity, uint64_t *rank, double *singular_values);
/* The same split on the reference's randomized branch (taken when max_bond_dim * 10 < min(rows, cols), mps.py:78):
 * Halko-Martinsson-Tropp range finder with `probes` = max_bond_dim + 10 Gaussian test vectors and
 * `power_iterations` passes (mps.py:5-50), SVD of the small projection, first max_bond_dim triplets, then the
 * truncation rule above.  `dev_omega` holds the test matrix the reference would draw,
 * rng.normal(size=(min(rows, cols), probes)), as complex128 in COLUMN-major order, so that a seeded run consumes
 * the same random stream and lands on the same subspace.  `dev_theta` is not modified.
 * `dev_omega` may be NULL on a first call: converting and uploading 10^5 normal deviates costs more than a split that
 * never reads them (under a loose tolerance a verified low-rank route with fixed probes decides most splits).  A caller
 * whose generator is shared with the rest of the simulation still has to DRAW them, as mps.py:14-15 does -- it can do so
 * while this call runs.  *rank = QSV_RANK_NEEDS_OMEGA then means nothing was computed: call again with the test matrix. */
#define QSV_RANK_NEEDS_OMEGA UINT64_MAX
int qsv_tensor_rsvd_split(int device, void *hip_stream, const void *dev_theta, uint64_t rows, uint64_t cols,
                          int64_t max_bond_dim, int probes, int power_iterations, const void *dev_omega,
                          double abs_err, double rel_err, void *dev_m1, void *dev_m2, uint64_t capacity,
                          uint64_t *rank, double *singular_values /* max_bond_dim doubles or NULL */);
/* Tall-skinny product on the f64 matrix cores, COLUMN-major with tight leading dimensions: Y = op(A) . Q with A (n x m)
 * and a panel of 1 <= l <= 256 columns (one pass over A per 64 of them); op: 0 = A, 3 = conj(A) (Q is m x l, Y is n x l); 1 = A^H, 2 = A^T (Q is n x l,
 * Y is m x l).  The building block of the range finder (A @ O, A^H @ Q, A @ Q of mps.py:15-21), where A is gigabytes
 * and the panel a few dozen columns: l is tiled in steps of 16 instead of the library's 64-wide macro tile, and the
 * transposed / conjugated forms let a row-major theta be used in either orientation without a re-ordered copy. */
int qsv_tensor_skinny_gemm(int device, void *hip_stream, int op, uint64_t n, uint64_t m, int l, const void *dev_a,
                           const void *dev_q, void *dev_y);
/* The splits keep their scratch memory (a copy-free pass needs panels only, the exact SVD its factors) in a grow-only
 * pool per (device, stream) context.  qsv_tensor_release_workspace frees the pools of every context of `device` (the
 * contexts and their rocBLAS handles stay) and the evicted probe matrices, after waiting for the whole device: it must
 * not be called while other streams of the device are working in the library.  Pools are re-grown on demand. */
int qsv_tensor_release_workspace(int device);
/* Free the context of one stream -- its rocBLAS handle and its pools -- after waiting for that stream.  The frees
 * themselves wait for the whole device.  A stream the library has not seen is no error.  Call it before destroying a
 * stream that ran tensor calls. */
int qsv_tensor_release_stream_workspace(int device, void *hip_stream);
/* Grow the pool of the stream's context to at least `bytes` now (a no-op when it is that large), so that the calls of
 * a batch never grow pools -- an allocation -- mid-flight. */
int qsv_tensor_reserve_workspace(int device, void *hip_stream, uint64_t bytes);
/* t[l, j, r] *= diag[j] in place: Z and P on a site (gates.py:223,245). */
int qsv_tensor_scale_axis(int device, void *hip_stream, void *dev_t, uint64_t L, uint64_t d, uint64_t R,
                          const void *dev_diag /* d */);
/* theta[a, j, l, b] *= plane[j, l] in place: the CZ phases on a two-site tensor (gates.py:159-160). */
int qsv_tensor_plane_diag(int device, void *hip_stream, void *dev_theta, uint64_t L, uint64_t d, uint64_t R,
                          const void *dev_plane /* d x d */);
/* out[a, p, b] = sum_e vals[p, e] in[a, cols[p, e], b] over the d*d plane points p: the bilinear (q1, q2)-plane
 * resampling of BS / CX for every bond pair at once (gates.py:74-80,187-189); cols < 0 are padding. */
int qsv_tensor_plane_gather(int device, void *hip_stream, const void *dev_in, void *dev_out, uint64_t L, uint64_t d,
                            uint64_t R, int per_point, const int32_t *dev_cols, const void *dev_vals);
/* The same two maps with nothing tabulated: theta[a, j, l, b] *= exp(i strength q_j q_l) (CZ), and
 * out[a, i0, i1, b] = bilinear interpolation of in[a, :, :, b] at (a00 q_i0 + a01 q_i1, a10 q_i0 + a11 q_i1), zero
 * outside the grid (BS: a rotation; CX: a shear).  `dev_grid` = the d grid points (doubles, ascending). */
int qsv_tensor_plane_phase(int device, void *hip_stream, void *dev_theta, uint64_t L, uint64_t d, uint64_t R,
                           const void *dev_grid, double strength);
int qsv_tensor_plane_affine(int device, void *hip_stream, const void *dev_in, void *dev_out, uint64_t L, uint64_t d,
                            uint64_t R, const void *dev_grid, const double *a /* a00 a01 a10 a11, host */);
/* out[l, r] = scale * in[l, level, r]: the site after a homodyne outcome (gates.py:108). */
int qsv_tensor_take_level(int device, void *hip_stream, const void *dev_in, void *dev_out, uint64_t L, uint64_t d,
                          uint64_t R, uint64_t level, double scale);
/* out[l, j, r] = vec[j] * in[l, r]: np.einsum("i,ajb -> aijb") of Insert.apply (gates.py:39). */
int qsv_tensor_insert_axis(int device, void *hip_stream, const void *dev_in, void *dev_out, uint64_t L, uint64_t d,
                           uint64_t R, const void *dev_vec /* d */);
/* out[x, y, z, w] = p[x, z] * q[y, w] (out[x, y, w, z] when swap_last != 0), p is (X x Z), q is (Y x W): the outer
 * products that attach the two halves of a GKP Bell pair to their neighbouring sites with the bond legs adjacent
 * (InsertBell.apply, gkp_simulator/insert_bell.py:80-90), ready for qsv_tensor_svd_split. */
int qsv_tensor_outer(int device, void *hip_stream, const void *dev_p, const void *dev_q, void *dev_out, uint64_t X,
                     uint64_t Y, uint64_t Z, uint64_t W, int swap_last);
/* out[j] = Re sum_{l, r} z[l, j, r] conj(t[l, j, r]) (d doubles in device memory): the diagonal of the reduced
 * density matrix once both environments are contracted into z (mps.py:188-189). */
int qsv_tensor_axis_overlap(int device, void *hip_stream, const void *dev_z, const void *dev_t, uint64_t L, uint64_t d,
                            uint64_t R, void *dev_out);
/* rho[i, j] = sum_{l, r} z[l, i, r] conj(t[l, j, r]) as a (d x d) device matrix: the whole reduced density matrix of a
 * site once both environments are contracted into z (partial_density_mps, mps.py:176-190, without the host einsum).
 * Synchronises `hip_stream` before it returns (the re-layout uses the decomposition pool). */
int qsv_tensor_axis_density(int device, void *hip_stream, const void *dev_z, const void *dev_t, uint64_t L, uint64_t d,
                            uint64_t R, void *dev_out);
/* Wigner functions of `batch` density matrices rho_b (batch x d x d, contiguous, device) sampled on x_k = x0 + k dx (hbar = 1):
 * W_b(q, p) = (1/pi) int rho_b(q - y, q + y) e^{2ipy} dy by the grid quadrature over x_k, the off-grid argument
 * sinc-interpolated (the Wigner function utils.wigner of the reference leaves unimplemented, cv_simulator/utils.py:6-7).
 * `q` (nq) and `p` (np) are HOST arrays; dev_w receives W as (batch x np x nq) doubles, row-major.  Nothing is
 * renormalised (the integral of W is dx Tr rho) unless `normalised` != 0, which divides by dx Tr rho_b.  QSV_EINVAL for
 * d < 2, batch < 1, nq < 1, np < 1, dx not positive and finite, any q or p not finite, or |p| > pi / (2 dx), past which
 * the quadrature aliases; every check runs before the first HIP call.  Synchronises `hip_stream` before it returns. */
int qsv_tensor_wigner(int device, void *hip_stream, const void *dev_rho, int batch, uint64_t d, double x0, double dx,
                      const double *q, uint64_t nq, const double *p, uint64_t np, int normalised, void *dev_w);
/* One site step of multi-shot homodyne sampling (SiteRegister.sample): S shots advance together through the site
 * `dev_site` (L x d x R) of a matrix-product state.  A shot is the outcome list of the chain Mq(0), Mq(0), ... of the
 * reference (cv_simulator/gates.py:87-117; the pre-rotations of Mp / Homodyne, :120-148, are applied to the site by the
 * caller), and rng.choice(range(d), p = w / w.sum()) of gates.py:98 is searchsorted(cumsum(p) / cumsum(p)[-1], u,
 * "right") of one uniform u.  With `dev_v` (S x L) the shots' boundary vectors -- the chain to the left collapsed onto
 * each shot's earlier picks -- and w[s, j, :] = v_s . site[:, j, :], the step is
 *     p[s, j]    = sum_b |w[s, j, b]|^2                      when dev_site_env is NULL (no sites to the right), else
 *                = Re sum_b conj(w[s, j, b]) (v_s . site_env[:, j, :])[b],   site_env = site . E (L x d x R), E the right
 *                  environment of mps.py:185-186: the diagonal of partial_density_mps (mps.py:176-190) of the collapsed
 *                  register without its grid measure;
 *     pick[s]    = the first j with cumsum(p[s, :])[j] / cumsum(p[s, :])[d - 1] > u[s]              (int32);
 *     density[s] = scale * p[s, pick[s]], `scale` = dq^(modes to the right): MeasurementResult.probability (gates.py:102);
 *     v_out[s,:] = v_s . site[:, pick[s], :] / sqrt(density[s])   (S x R; gates.py:108-113).  NULL: not computed.
 * p is never stored beyond a bounded block of shots, w not at all; nothing the caller passed is modified except the
 * outputs.  QSV_EINVAL for S < 1, d < 2, L < 1, R < 1, L > 512, a scale that is not positive and finite, or a NULL
 * dev_v / dev_site / dev_u / dev_pick / dev_density; every check runs before the first HIP call.  Synchronises
 * `hip_stream` before it returns. */
int qsv_tensor_sample_site(int device, void *hip_stream, const void *dev_v, const void *dev_site,
                           const void *dev_site_env /* may be NULL */, uint64_t S, uint64_t L, uint64_t d, uint64_t R,
                           double scale, const double *dev_u, int32_t *dev_pick, double *dev_density,
                           void *dev_v_out /* may be NULL */);

/* One step of bringing a matrix-product state into canonical form (SiteRegister.canonicalise / compress): factor the
 * site `dev_site` (L x d x R, read as it is stored, not modified) into an isometry and a small carry matrix.
 *   side = 0 (left):  site[(l,j), r] = sum_k iso[(l,j), k] carry[k, r];  iso (L, d, rank) with orthonormal columns,
 *                     carry (rank x R) = diag(s) Vh;   the bond that is orthogonalised is R.
 *   side = 1 (right): site[l, (j,r)] = sum_k carry[l, k] iso[k, (j,r)];  iso (rank, d, R) with orthonormal rows,
 *                     carry (L x rank) = U diag(s);    the bond that is orthogonalised is L.
 * s are the singular values of the site matrix in decreasing order (absolute accuracy of a few 8 eps max(bond,
 * sqrt(rows)) s[0]), *rank = the number of them above rank_tol * s[0].  Directions whose
 * singular value is below that rounding level (about 1e-13 s[0] for sites of a thousand rows, 1e-12 s[0] for 1e5 rows)
 * cannot be told from zero and come out as exactly 0: they are never kept, so
 * with rank_tol = 0 a site of full numerical rank keeps min(rows, cols) directions and a rank-deficient one its numerical
 * rank, and iso is an isometry either way.  Both outputs are written compactly for the returned rank; dev_iso must
 * hold L d R amplitudes, dev_carry bond^2.  singular_values (host, may be NULL) receives min(rows, cols) doubles with
 * (rows, cols) = (L d, R) resp. (L, d R).  The orthogonalised bond may be at most QSV_SITE_MAX_BOND wide.  The order of
 * every sum depends on (L, d, R, side) alone.  QSV_EINVAL, before the first HIP call, for d < 2, L < 1, R < 1, a side
 * other than 0 / 1, a bond above QSV_SITE_MAX_BOND, a NULL dev_site / dev_iso / dev_carry / rank, a rank_tol that is
 * negative or not finite.  Synchronises `hip_stream` before it returns. */
#define QSV_SITE_MAX_BOND 128
int qsv_tensor_site_orthogonalise(int device, void *hip_stream, const void *dev_site, uint64_t L, uint64_t d, uint64_t R,
                                  int side, double rank_tol, void *dev_iso, void *dev_carry, uint64_t *rank,
                                  double *singular_values);

/* ---- whole circuits in one launch (registers of at most 13 qubits) ------------------------------------------------
 * Replaces the caller loop itself -- `for gate in self.circuit: ... gate.apply(state)` with its measurement record and
 * ClassicalControl (dv_simulator/simulator.py:40-52, :6-17) -- for the register sizes the reference can run (4..12
 * qubits) and the batches of circuits its drivers push through a multiprocessing.Pool
 * (impact_.../randomised_benchmarking.py:60-76, average_clifford_fidelity.py:212): one workgroup per instance keeps the
 * register in LDS and walks its gate list; `count` instances run side by side on the CUs.  Everything is host memory,
 * the call returns when the results are in place.
 *   programs / prog_offsets[count + 1]: the instances' gate lists as 64-bit words (format: csrc/qsv_circuit.hip;
 *       built by quantum_computations_amd.dv_simulator.program), word offsets per instance.
 *   n_initial[count]; states_in + state_offsets[count + 1]: initial kets (interleaved complex128), amplitude offsets.
 *   states_out + out_offsets[count + 1]: final kets (their sizes follow from the programs: M removes, Insert adds a qubit).
 *   results / probabilities + result_offsets[count + 1]: outcome and the two branch norms (p0, p1) of every
 *       measurement, in program order.  A measurement op carries either a forced outcome (gates.py:183 `result=`) or
 *       the uniform number the host drew for it; outcome 0 iff u < p0 / (p0 + p1), as np.random.choice picks it.
 *   max_qubits: the largest register any instance reaches (<= 13). */
int qsv_run_programs(int device, int count, int max_qubits, const uint64_t *programs, const uint64_t *prog_offsets,
                     const int *n_initial, const double *states_in, const uint64_t *state_offsets, double *states_out,
                     const uint64_t *out_offsets, int *results, double *probabilities, const uint64_t *result_offsets);

/* ---- timing on the state's stream (HIP events), for bench.py's roofline figures ----------- */
int qsv_timer_start(qsv_state *st);
int qsv_timer_stop(qsv_state *st, float *elapsed_ms); /* records, synchronises the event, returns ms */
/* Name of the gate kernel the most recent qsv_apply_* call launched on this state, spelled as rocprofv3
 * prints it (e.g. "k_dense<1, 0, 1, true>"); "" if none.  Lets bench.py attribute its event timings. */
int qsv_last_kernel(const qsv_state *st, char *buf, size_t buf_len);
/* Non-blocking marks: record HIP event number `slot` (0 <= slot < 16384) on the state's stream;
 * qsv_event_elapsed_ms waits for mark `slot_b` and returns the device time between two marks. */
int qsv_event_record(qsv_state *st, int slot);
int qsv_event_elapsed_ms(qsv_state *st, int slot_a, int slot_b, float *elapsed_ms);

#ifdef __cplusplus
}
#endif
#endif /* QSV_H */
