// The deferred-gate pass of the qubit register: k_pass_tile with its pass_* bodies, and the launchers of a queued gate
// (qsvk_pass for a shared pass, qsvk_run_op for the gate on its own kernel, qsvk_op_exact).  The queue is cut by
// qsv_plan.h, the records are made by qsv_layout::pass_records.  The bodies repeat the expressions of the per-gate kernels
// of qsv_gate12.hip on purpose and call none of them: a deferred gate must round exactly as its own launch does.
// This file needs -mllvm -structurizecfg-skip-uniform-regions (build.py).

#include "qsv_internal.h"
#include "qsv_device.h"
#include "qsv_layout.h"
#include "qsv_plan.h"

#include <cstring>
#include <vector>

using namespace qsv_layout;   // the argument and record types of the kernels, and the host-side tables the launchers fill them from

// ---- deferred gates: one PASS of queued 1- and 2-qubit gates over LDS-resident tiles ----------------------------------
// The queue of a deferring register (qsv_api.hip) is cut into passes by qsv_plan.h.  A workgroup brings one 4096-amplitude
// tile into LDS -- bits 0..5 plus the pass's six further tile bits, so every tile row is one 1 KiB run of HBM, straight
// into LDS on the way in -- applies the pass's gates to it and stores it back: one round trip over HBM for the whole list.
// The gates are applied in GROUPS (qsv_plan::cut_groups: consecutive gates whose targets fit four tile bits): each of the
// 256 threads takes the 16 amplitudes of one setting of the other eight tile bits into registers, applies the group's
// gates there and puts them back -- one LDS round trip and one barrier per group, not per gate (the benchmark circuit: 123 groups for 399 gates in 40 passes;
// measured figures in DESIGN.md section 10).
// Register indices are compile-time: one unrolled body per register bit (1-qubit gates) or ordered pair of them (2-qubit
// gates) and summation form, behind a wave-uniform switch.
// A gate's control bits outside the tile are the same for every amplitude of a tile: they decide per workgroup whether
// the gate acts (omask); a group none of whose gates acts makes no LDS trip, and a tile on which no gate of the pass acts is
// neither loaded nor stored; when some gate of the pass has no outside control (PassArgs::every_tile) the tile is asked for
// first and the controls are looked at under the loads.  A control bit inside the tile is a register bit (rc: amplitudes of
// the thread that the gate skips, wave-uniform) or a thread bit (tc: the new values replace the old ones by a select); the
// bodies exist once per control class (PassGate::ctl), so a gate without controls pays for neither.  Each gate is computed with
// the expression and the summation order of the per-gate kernel it would have run on (tile12_body: products summed from
// zero in kernel-index order; dense_body: low-lane combinations outer, high rows inner; k_diag: one complex product), so
// the amplitudes are bit for bit those of the per-gate path.  A pair exchange moves registers.
constexpr int PASS_TILE = 1 << qsv_plan::TILE_BITS, PASS_ROWS = PASS_TILE / 64, PASS_THREADS = 256;
constexpr int PASS_ROWS_PER_WAVE = PASS_ROWS / (PASS_THREADS / 64);
static_assert(PASS_TILE == PASS_THREADS << qsv_plan::REG_BITS, "one thread per setting of the tile bits outside the registers");

struct PassArgs {
    BigArgs g;                     // pos[] = the 12 tile bits: the tile number is deposited around them, and tile row r
                                   // (tile bits 6..11) starts at the register offset sum_j ((r >> j) & 1) << pos[6 + j]
    uint32_t every_tile;           // some gate of the pass has no control outside the tile: every tile is loaded
};

// Kernel index of the j-th product summed into output row r.  NAT: tile12_body and dense_body without low targets;
// XOR: dense_body with every target a lane bit (x = j over the low combinations); HL: dense_body with one high and one low
// target (x = j >> 1 outer, hp = j & 1 inner, column (hp, l ^ x)).
template <int FORM>
__device__ __forceinline__ constexpr int pass_col(int r, int j) {
    return FORM == 0 ? j : FORM == 1 ? (j ^ r) : (((j & 1) << 1) | ((r & 1) ^ (j >> 1)));
}

// The controls of a gate inside the tile, as one thread sees them.  Every body is compiled once per control class CTL
// (PASS_CTL_*): without controls neither field is read and the new amplitudes are written in place; with controls on
// register bits the register indices b that the gate skips are branched around (wave-uniform); only with controls on
// thread bits do the new values replace the old ones by a select.
struct PassCtl {
    uint32_t rc;     // wave-uniform: register-index bits that must be 1
    bool ok;         // this thread's control bits are all 1
};

template <int CTL>
__device__ __forceinline__ bool pass_skips(int b, const PassCtl &ct) {
    return CTL != PASS_CTL_NONE && (static_cast<uint32_t>(b) & ct.rc) != ct.rc;
}

template <int CTL>
__device__ __forceinline__ void pass_put(amp_t &x, amp_t y, const PassCtl &ct) {
    if constexpr (CTL == PASS_CTL_THREAD) {
        x.x = ct.ok ? y.x : x.x;
        x.y = ct.ok ? y.y : x.y;
    } else {
        x = y;
    }
}

// Dense gate on D amplitudes: kernel index bit 0 <-> register bit P0, bit 1 <-> register bit P1 (D = 4).  Each output is the
// cfma chain from zero over j = 0 .. D - 1 of the per-gate kernels; the chains are written column by column, and in the
// last column every inner product before the first outer one, so that an amplitude has been read for the last time when
// the output that takes its register is produced: the amplitudes are then updated in place, with no second copy of x[].
template <int CTL, int D, int FORM, int P0, int P1>
__device__ __forceinline__ void pass_dense(amp_t (&x)[16], const double *__restrict__ m, const PassCtl &ct) {
    constexpr int TARGETS = (1 << P0) | (D == 4 ? (1 << P1) : 0);
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        if (b & TARGETS) continue;
        if (pass_skips<CTL>(b, ct)) continue;      // wave-uniform: a control on a register bit is 0 here
        int idx[D];
#pragma unroll
        for (int c = 0; c < D; ++c) idx[c] = b | ((c & 1) << P0) | (D == 4 ? ((c >> 1) << P1) : 0);
        amp_t acc[D];
#pragma unroll
        for (int r = 0; r < D; ++r) acc[r] = amp_t{0.0, 0.0};
#pragma unroll
        for (int j = 0; j < D - 1; ++j)
#pragma unroll
            for (int r = 0; r < D; ++r) {
                const int c = pass_col<FORM>(r, j);
                acc[r] = cfma(cplx{m[2 * (r * D + c)], m[2 * (r * D + c) + 1]}, x[idx[c]], acc[r]);
            }
        // the last column in cfma's two halves: every inner half before the first outer one
#pragma unroll
        for (int r = 0; r < D; ++r) {
            const int c = pass_col<FORM>(r, D - 1);
            acc[r] = cfma_inner(cplx{m[2 * (r * D + c)], m[2 * (r * D + c) + 1]}, x[idx[c]], acc[r]);
        }
        amp_t y[D];
#pragma unroll
        for (int r = 0; r < D; ++r) {
            const int c = pass_col<FORM>(r, D - 1);
            y[r] = cfma_outer(cplx{m[2 * (r * D + c)], m[2 * (r * D + c) + 1]}, x[idx[c]], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < D; ++r) pass_put<CTL>(x[idx[r]], y[r], ct);
    }
}

template <int CTL, int PA, int PB>
__device__ __forceinline__ void pass_pair(amp_t (&x)[16], const PassCtl &ct) {
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        if (b & ((1 << PA) | (1 << PB))) continue;
        if (pass_skips<CTL>(b, ct)) continue;
        const amp_t u = x[b | (1 << PA)], v = x[b | (1 << PB)];
        pass_put<CTL>(x[b | (1 << PA)], v, ct);
        pass_put<CTL>(x[b | (1 << PB)], u, ct);
    }
}

// Diagonal gate whose factor for register index c is d[SEL(c)] (d[] per thread or wave-uniform).
template <int CTL, class Sel>
__device__ __forceinline__ void pass_diag(amp_t (&x)[16], const cplx (&d)[4], const PassCtl &ct, Sel sel) {
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (pass_skips<CTL>(c, ct)) continue;
        pass_put<CTL>(x[c], cmul_diag(d[sel(c)], x[c]), ct);
    }
}

__device__ __forceinline__ cplx pass_pick(bool s, cplx one, cplx zero) {
    return cplx{s ? one.re : zero.re, s ? one.im : zero.im};
}

template <int CTL>
__device__ __forceinline__ void pass_gate16(amp_t (&x)[16], const PassGate &pg, uint32_t g0) {
    const double *__restrict__ m = pg.m;
    const PassCtl ct = {pg.rc, (g0 & pg.tc) == pg.tc};
#define QSV_PASS_D4(FORM, P0, P1) case (FORM) * 16 + (P0) * 4 + (P1): pass_dense<CTL, 4, (FORM) - PASS_D4, P0, P1>(x, m, ct); break;
#define QSV_PASS_D4_BOTH(FORM, LO, HI) QSV_PASS_D4(FORM, LO, HI) QSV_PASS_D4(FORM, HI, LO)
    switch (pg.form * 16 + pg.code) {     // wave-uniform (scalar loads)
        case PASS_D2 * 16 + 0: pass_dense<CTL, 2, 0, 0, 0>(x, m, ct); break;
        case PASS_D2 * 16 + 1: pass_dense<CTL, 2, 0, 1, 0>(x, m, ct); break;
        case PASS_D2 * 16 + 2: pass_dense<CTL, 2, 0, 2, 0>(x, m, ct); break;
        case PASS_D2 * 16 + 3: pass_dense<CTL, 2, 0, 3, 0>(x, m, ct); break;
        case PASS_D2X * 16 + 0: pass_dense<CTL, 2, 1, 0, 0>(x, m, ct); break;
        case PASS_D2X * 16 + 1: pass_dense<CTL, 2, 1, 1, 0>(x, m, ct); break;
        case PASS_D2X * 16 + 2: pass_dense<CTL, 2, 1, 2, 0>(x, m, ct); break;
        case PASS_D2X * 16 + 3: pass_dense<CTL, 2, 1, 3, 0>(x, m, ct); break;
        QSV_PASS_D4_BOTH(PASS_D4, 0, 1) QSV_PASS_D4_BOTH(PASS_D4, 0, 2) QSV_PASS_D4_BOTH(PASS_D4, 0, 3)
        QSV_PASS_D4_BOTH(PASS_D4, 1, 2) QSV_PASS_D4_BOTH(PASS_D4, 1, 3) QSV_PASS_D4_BOTH(PASS_D4, 2, 3)
        QSV_PASS_D4_BOTH(PASS_D4X, 0, 1) QSV_PASS_D4_BOTH(PASS_D4X, 0, 2) QSV_PASS_D4_BOTH(PASS_D4X, 0, 3)
        QSV_PASS_D4_BOTH(PASS_D4X, 1, 2) QSV_PASS_D4_BOTH(PASS_D4X, 1, 3) QSV_PASS_D4_BOTH(PASS_D4X, 2, 3)
        // one low and one high target: the low one (kernel bit 0) has the smaller tile index, so the smaller register bit
        QSV_PASS_D4(PASS_D4HL, 0, 1) QSV_PASS_D4(PASS_D4HL, 0, 2) QSV_PASS_D4(PASS_D4HL, 0, 3)
        QSV_PASS_D4(PASS_D4HL, 1, 2) QSV_PASS_D4(PASS_D4HL, 1, 3) QSV_PASS_D4(PASS_D4HL, 2, 3)
        case PASS_PAIR * 16 + 0 * 4 + 1: pass_pair<CTL, 0, 1>(x, ct); break;
        case PASS_PAIR * 16 + 0 * 4 + 2: pass_pair<CTL, 0, 2>(x, ct); break;
        case PASS_PAIR * 16 + 0 * 4 + 3: pass_pair<CTL, 0, 3>(x, ct); break;
        case PASS_PAIR * 16 + 1 * 4 + 2: pass_pair<CTL, 1, 2>(x, ct); break;
        case PASS_PAIR * 16 + 1 * 4 + 3: pass_pair<CTL, 1, 3>(x, ct); break;
        case PASS_PAIR * 16 + 2 * 4 + 3: pass_pair<CTL, 2, 3>(x, ct); break;
        case PASS_DIAG_T * 16: {       // both selector bits are thread bits: one factor per thread
            const bool s0 = (g0 >> pg.tz0) & 1, s1 = (g0 >> pg.tz1) & 1;
            const cplx d[4] = {pass_pick(s0, pass_pick(s1, cplx{m[6], m[7]}, cplx{m[4], m[5]}),
                                         pass_pick(s1, cplx{m[2], m[3]}, cplx{m[0], m[1]})), {}, {}, {}};
            pass_diag<CTL>(x, d, ct, [](int) { return 0; });
            break;
        }
#define QSV_PASS_R1(P) case PASS_DIAG_R1 * 16 + (P): { \
            const cplx d[4] = {{m[0], m[1]}, {m[2], m[3]}, {}, {}}; \
            pass_diag<CTL>(x, d, ct, [](int c) { return (c >> (P)) & 1; }); break; }
        QSV_PASS_R1(0) QSV_PASS_R1(1) QSV_PASS_R1(2) QSV_PASS_R1(3)
#define QSV_PASS_R2(P0, P1) case PASS_DIAG_R2 * 16 + (P0) * 4 + (P1): { \
            const cplx d[4] = {{m[0], m[1]}, {m[2], m[3]}, {m[4], m[5]}, {m[6], m[7]}}; \
            pass_diag<CTL>(x, d, ct, [](int c) { return (((c >> (P0)) & 1) << 1) | ((c >> (P1)) & 1); }); break; }
        QSV_PASS_R2(0, 1) QSV_PASS_R2(0, 2) QSV_PASS_R2(0, 3) QSV_PASS_R2(1, 2) QSV_PASS_R2(1, 3) QSV_PASS_R2(2, 3)
#define QSV_PASS_M(P) case PASS_DIAG_M * 16 + (P): { \
            const bool s = (g0 >> pg.tz0) & 1; \
            const cplx d[4] = {pass_pick(s, cplx{m[2], m[3]}, cplx{m[0], m[1]}), pass_pick(s, cplx{m[6], m[7]}, cplx{m[4], m[5]}), {}, {}}; \
            pass_diag<CTL>(x, d, ct, [](int c) { return (c >> (P)) & 1; }); break; }
        QSV_PASS_M(0) QSV_PASS_M(1) QSV_PASS_M(2) QSV_PASS_M(3)
        default: break;       // qsvk_pass builds no other record
    }
#undef QSV_PASS_D4
#undef QSV_PASS_D4_BOTH
#undef QSV_PASS_R1
#undef QSV_PASS_R2
#undef QSV_PASS_M
}

__device__ __forceinline__ void pass_gate16(amp_t (&x)[16], const PassGate &pg, uint32_t g0) {
    switch (pg.ctl) {                     // wave-uniform
        case PASS_CTL_NONE: pass_gate16<PASS_CTL_NONE>(x, pg, g0); break;
        case PASS_CTL_REG: pass_gate16<PASS_CTL_REG>(x, pg, g0); break;
        default: pass_gate16<PASS_CTL_THREAD>(x, pg, g0); break;
    }
}

// omask[]: the gates' omask fields packed, padded with zeros to a multiple of 8 entries (read eight at a time).
template <bool NT>
__global__ __launch_bounds__(PASS_THREADS) void k_pass_tile(amp_t *__restrict__ a, const PassArgs pa,
                                                            const PassGate *__restrict__ gates, int n_gates,
                                                            const PassGroup *__restrict__ groups, int n_groups,
                                                            const uint64_t *__restrict__ omask) {
    __shared__ amp_t tile[PASS_TILE];      // [row][64 lanes]: LDS index = tile index (bits 0..5 lane, 6..11 row)
    const BigArgs &g = pa.g;
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int RPW = PASS_ROWS_PER_WAVE;
    const uint64_t tile_id = (g.regions > 1 && gridDim.x % g.regions == 0)
                                 ? (blockIdx.x % g.regions) * (gridDim.x / g.regions) + blockIdx.x / g.regions
                                 : blockIdx.x;
    uint64_t base = g.w0 + tile_id;        // deposit() with the trip count known: pos[] arrives in wide loads
#pragma unroll
    for (int j = 0; j < qsv_plan::TILE_BITS; ++j) base = insert_zero(base, static_cast<int>(g.pos[j]));
    base |= g.or_mask;
    // this wave's rows are q RPW + i: the wave's own offset, plus those of the bits of i when a row is addressed (they are
    // not kept in scalar registers from the load to the store: sixteen 64-bit offsets would be a third of them)
    static_assert(RPW == 16 && PASS_ROWS == 64, "four row bits from i, two from the wave number");
    uint64_t row0 = base + (static_cast<uint64_t>(q & 1) << g.pos[10]) + (static_cast<uint64_t>(q >> 1) << g.pos[11]);
    auto row = [&](int i) {
        uint64_t r = row0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((i >> j) & 1) r += 1ull << g.pos[6 + j];
        return r;
    };
    auto request_tile = [&]() {
#if defined(__HIP_DEVICE_COMPILE__)   // the builtin exists in the device pass only
#pragma unroll
        for (int i = 0; i < RPW; ++i)
            __builtin_amdgcn_global_load_lds(a + row(i) + lane, tile + (q * RPW + i) * 64, 16, 0, NT ? 2 : 0);
#endif
    };
    // With a gate that acts on every tile in the pass, the tile is requested before the gates' outside controls are
    // looked at, and that look happens under the loads.
    if (pa.every_tile) request_tile();
    uint64_t active = 0;                   // wave-uniform: bit i = gate i acts on this tile
    for (int i0 = 0; i0 < n_gates; i0 += 8) {
        uint64_t om[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) om[j] = omask[i0 + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) active |= static_cast<uint64_t>((base & om[j]) == om[j]) << (i0 + j);
    }
    active &= ~0ull >> (64 - n_gates);     // the padding reads as gates without outside controls
    if (!pa.every_tile) {
        if (!active) return;
        request_tile();
    }
    __syncthreads();
#pragma unroll 1
    for (int p = 0; p < n_groups; ++p) {
        const PassGroup &gr = groups[p];
        if (!(active & gr.gates)) continue;     // no gate of the group acts on this tile: no LDS trip
        const int q0 = gr.q[0], q1 = gr.q[1], q2 = gr.q[2], q3 = gr.q[3];
        // this thread's setting of the other eight tile bits: its index with zeros inserted at the register bits
        uint32_t g0 = threadIdx.x;
        g0 = static_cast<uint32_t>(insert_zero(g0, q0));
        g0 = static_cast<uint32_t>(insert_zero(g0, q1));
        g0 = static_cast<uint32_t>(insert_zero(g0, q2));
        g0 = static_cast<uint32_t>(insert_zero(g0, q3));
        amp_t x[16];
#pragma unroll
        for (int c = 0; c < 16; ++c)
            x[c] = tile[g0 | ((c & 1) << q0) | (((c >> 1) & 1) << q1) | (((c >> 2) & 1) << q2) | (((c >> 3) & 1) << q3)];
#pragma unroll 1
        for (int i = gr.first; i < gr.first + gr.count; ++i)
            if ((active >> i) & 1) pass_gate16(x, gates[i], g0);
#pragma unroll
        for (int c = 0; c < 16; ++c)
            tile[g0 | ((c & 1) << q0) | (((c >> 1) & 1) << q1) | (((c >> 2) & 1) << q2) | (((c >> 3) & 1) << q3)] = x[c];
        __syncthreads();
    }
#if defined(__HIP_DEVICE_COMPILE__)
    // Without this the compiler keeps the sixteen row offsets of the load alive for the store: 32 SGPRs across the gate
    // loop, beside the 64 of a 4 x 4 matrix -- the build that did so spilled SGPRs into v_writelane / v_readlane in the
    // 2-qubit bodies (sgpr_spill_count 21 in the kernel's metadata; 0 with it).  row0 comes out as it went in.
    asm volatile("" : "+s"(row0));
#endif
#pragma unroll
    for (int i = 0; i < RPW; ++i) st<NT>(a + row(i) + lane, tile[(q * RPW + i) * 64 + lane]);
}

bool qsvk_op_exact(const QsvOp &op) {
    if (op.kind == QSV_OP_PAIR) return true;
    auto unit = [](double re, double im) { return im == 0.0 && (re == 1.0 || re == -1.0); };
    if (op.kind == QSV_OP_PHASE) return unit(op.m[0], op.m[1]);
    if (op.kind == QSV_OP_DIAG) {
        for (int i = 0; i < (1 << op.k); ++i)
            if (!unit(op.m[2 * i], op.m[2 * i + 1])) return false;
        return true;
    }
    // dense: one +-1 per row and per column, zeros elsewhere (every output is one input, negated or not)
    const int D = 1 << op.k;
    int per_col[4] = {0, 0, 0, 0};
    for (int r = 0; r < D; ++r) {
        int nz = 0;
        for (int c = 0; c < D; ++c) {
            const double re = op.m[2 * (r * D + c)], im = op.m[2 * (r * D + c) + 1];
            if (re == 0.0 && im == 0.0) continue;
            if (!unit(re, im)) return false;
            ++nz;
            ++per_col[c];
        }
        if (nz != 1) return false;
    }
    for (int c = 0; c < D; ++c)
        if (per_col[c] != 1) return false;
    return true;
}

int qsvk_run_op(qsv_state *st, const QsvOp &op) {
    switch (op.kind) {
        case QSV_OP_DENSE: return qsvk_dense(st, op.k, op.bits, op.nctrl, op.cbits, op.m);
        case QSV_OP_PAIR: return qsvk_pair_exchange(st, op.bits[0], op.bits[1]);
        case QSV_OP_DIAG: return qsvk_diag(st, op.k, op.bits, op.nctrl, op.cbits, op.m);
        case QSV_OP_PHASE: return qsvk_phase(st, op.nctrl, op.cbits, op.m[0], op.m[1]);
        default: return qsv_fail(QSV_EINVAL, "internal: unknown queued gate kind");
    }
}

// One k_pass_tile launch for `count` queued gates (in application order) on the tiles spanned by bits 0..5 and tile_high.
int qsvk_pass(qsv_state *st, const QsvOp *const *ops, int count, uint64_t tile_high) {
    const uint64_t low = (1ull << QSV_LANE_BITS) - 1;
    if (count < 1 || count > qsv_plan::MAX_PASS_GATES || st->n < qsv_plan::TILE_BITS || (tile_high & low) ||
        __builtin_popcountll(tile_high) != qsv_plan::HIGH_BITS || (tile_high >> st->n))
        return qsv_fail(QSV_EINVAL, "internal: malformed gate pass");
    const PassRecords pr = pass_records(ops, count, tile_high, st->amps);
    if (pr.status == PassRecords::TARGET_OUTSIDE_TILE) return qsv_fail(QSV_EINVAL, "internal: gate target outside its pass's tile");
    if (pr.status == PassRecords::TARGET_OUTSIDE_GROUP) return qsv_fail(QSV_EINVAL, "internal: gate target outside its group's register bits");
    // staged: the records, then the groups with the packed omasks behind them (padded to the eight the kernel reads at a time)
    const size_t grp_bytes = sizeof(PassGroup) * pr.grp.size(), omask_count = (pr.omask.size() + 7) / 8 * 8;
    std::vector<char> tail(grp_bytes + sizeof(uint64_t) * omask_count, 0);
    std::memcpy(tail.data(), pr.grp.data(), grp_bytes);
    std::memcpy(tail.data() + grp_bytes, pr.omask.data(), sizeof(uint64_t) * pr.omask.size());
    StageRef staged;
    int rc = qsvk_stage(st, pr.rec.data(), sizeof(PassGate) * pr.rec.size(), tail.data(), tail.size(), &staged);
    if (rc) return rc;
    const PassGate *dev_g = reinterpret_cast<const PassGate *>(staged.dev);
    const PassGroup *dev_p = reinterpret_cast<const PassGroup *>(staged.dev + qsv_pad16(sizeof(PassGate) * pr.rec.size()));
    const uint64_t *dev_o = reinterpret_cast<const uint64_t *>(reinterpret_cast<const char *>(dev_p) + grp_bytes);
    const int n_groups = static_cast<int>(pr.grp.size());
    const std::vector<int> tile_bits(pr.tile_bits, pr.tile_bits + qsv_plan::TILE_BITS);
    PassArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    pa.g = with_enumeration<BigArgs>(enumeration(st->amps >> qsv_plan::TILE_BITS, tile_bits));   // tiles: the index with every tile bit taken out
    pa.g.regions = regions_or(st, 8);
    pa.every_tile = pr.every_tile ? 1u : 0u;
    const bool nt = st->nontemporal != 0;
    snprintf(st->last_kernel, sizeof(st->last_kernel), "k_pass_tile<%s>", nt ? "true" : "false");
    rc = launch_ranges(pa.g, DISPATCH_TILES, [&](uint64_t tiles) {
        const dim3 gd(static_cast<unsigned>(tiles)), bd(PASS_THREADS);
        with_bool(nt, [&](auto NT) { hipLaunchKernelGGL(k_pass_tile<NT.value>, gd, bd, 0, st->stream, st->data, pa, dev_g, count, dev_p, n_groups, dev_o); });
    });
    return rc ? rc : qsvk_stage_done(st, staged);
}
