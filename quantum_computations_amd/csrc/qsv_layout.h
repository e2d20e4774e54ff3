// Host-side layouts and launch rules of the gate launchers (qsv_gate12.hip, qsv_gatek.hip, qsv_sequence.hip,
// qsv_pass.hip): plain C++, no HIP, so that the host tests can compile it alone (tests/test_layout_host.py).  The read-out
// and Pauli launchers have qsv_readout_layout.h.
//
// A launcher chooses a kernel form, asks this header for the tables of that form, stages them, fills the kernel's argument
// struct and launches over the dispatch ranges.  Everything here is integer and index arithmetic on three index spaces:
//   * ADDRESS bits: the bits of an amplitude's index in the register (bit 0..5 = the lane of a wave, 0..2 = inside one
//     128-byte line);
//   * KERNEL index bits: the bits of the index c of the 2^k amplitudes x[c] one work item gathers, x[c] = a[deposit(w) +
//     off[c]]; which target a kernel bit stands for is the form's choice (its KERNEL BIT ORDER);
//   * CALLER index bits: the bits of a row / column index of the caller's matrix, leg 0 most significant.
// deposit(w) spreads the work-item number w over the address bits that are not inserted positions (pos[], ascending) and
// ORs or_mask in.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <vector>

#include "qsv_plan.h"

namespace qsv_layout {

constexpr int LANE_BITS = 6;     // address bits 0..5 are spread over the 64 lanes of a wave
constexpr int LINE_BITS = 3;     // address bits 0..2 lie inside one 128-byte line
constexpr int MAX_K = 6;         // widest dense gate
constexpr int BLOCK = 256;       // threads per workgroup of the per-thread forms

// ---- argument and record types of the kernels (passed by value or staged as they are: field order and sizes are ABI) ----

// k_dense_big, k_seq_big and the tile forms (pos[] = whatever the form takes out of the enumeration).
struct BigArgs {
    uint64_t W;
    int32_t nins;
    uint32_t pos[2 * MAX_K];     // ascending: high targets and stand-in bits
    uint64_t or_mask;            // unused (0); lets deposit() serve this struct too
    uint64_t w0;                 // first work item of this launch (registers beyond 2^32 work items take several)
    uint32_t regions;            // tile order (see GateArgs::remap)
    int32_t lbit[MAX_K];         // lane-bit position of low target j (register index bit j)
};

struct LdsArgs {
    uint64_t W;
    int32_t nins;
    uint32_t pos[2 * MAX_K];     // ascending: high targets and stand-in bits
    uint64_t or_mask;            // unused (0); lets deposit() serve this struct too
    uint64_t w0;                 // first work item of this launch
    uint32_t regions;            // tile order (see GateArgs::remap)
    uint32_t amask;              // lane bits of the A targets
    int32_t abit[3], aE[3];      // A target j: lane bit, stand-in bit
    int32_t na;                  // number of A targets
    uint32_t bdep[8];            // dep(v): the KB bits of v spread onto the lane bits of the B targets
    uint32_t bmask;              // lane bits of the B targets
};

struct SmallGate {
    double m[32];      // [row][col] (re, im), kernel index bit i <-> leg i
    uint64_t off[4];   // amplitude offset of input / output row c
};

struct SeqGate {
    int32_t code;      // 0..4: 1-qubit gate on register bit `code`; 5 + p: 2-qubit gate on the p-th pair (hi, lo), hi > lo
    int32_t pad[3];
    double m[32];      // 2 x 2 or 4 x 4 row-major complex; 2-qubit: matrix index bit 1 <-> register bit hi
};
constexpr int SEQ_MAX_GATES = 48;

struct TilePass {
    int32_t first, count;      // gates [first, first + count) of the SeqGate list (codes relative to the pass's four bits)
    int32_t q[4];              // the pass's tile bits, ascending
    int32_t pad[2];
};
constexpr int TILE_SEQ_BITS = 12, TILE_SEQ_ROWS = 1 << (TILE_SEQ_BITS - 6), TILE_SEQ_THREADS = 256, TILE_SEQ_MAX_PASSES = 24;

enum {
    PASS_D2 = 0, PASS_D2X = 1, PASS_D4 = 2, PASS_D4X = 3, PASS_D4HL = 4,   // dense on 2 / 4 amplitudes, by summation form
    PASS_PAIR = 5,                                                          // exchange of (a, b) = (1, 0) and (0, 1)
    PASS_DIAG_T = 6, PASS_DIAG_R1 = 7, PASS_DIAG_R2 = 8, PASS_DIAG_M = 9    // diagonal, by where its selector bits sit
};
enum { PASS_CTL_NONE = 0, PASS_CTL_REG = 1, PASS_CTL_THREAD = 2 };   // where a gate's controls inside the tile sit
struct PassGate {
    int32_t form;        // PASS_*
    int32_t code;        // the body of the form: register bit P of kernel bit 0 (D2*, DIAG_R1, DIAG_M), or 4 P0 + P1 for
                         // the register bits of kernel bits 0 and 1 (D4*), of the two legs (PAIR) or P0 < P1 (DIAG_R2)
    uint32_t rc;         // controls on register bits, as a mask of the register index 0..15
    uint32_t tc;         // controls on thread bits, as a mask of tile indices
    int32_t tz0, tz1;    // DIAG_T: tile indices of the thread bits s0, s1 that select d[(s0 << 1) | s1]; DIAG_M: tz0 = the
                         // thread bit s of d[(register bit << 1) | s]
    int32_t ctl;         // PASS_CTL_*: no control inside the tile, on register bits only (rc), or on thread bits (tc, and
                         // maybe rc); the kernel has one body per class
    int32_t pad0;
    uint64_t omask;      // register bits outside the tile that must be 1 (the same for every amplitude of a tile); the
                         // kernel reads PassRecords::omask, the same values packed, and not this field
    double m[32];        // dense: D x D kernel-order matrix, (re, im) interleaved; diagonal: d[0..3] as the form reads them
};
static_assert(sizeof(PassGate) == 40 + 32 * sizeof(double), "no padding but pad0");
struct PassGroup {
    int32_t first, count;   // gates [first, first + count) of the pass
    int32_t q[4];           // the group's register bits as tile indices, ascending
    uint64_t gates;         // bit i = gate i of the pass belongs to the group
};

// One 1- or 2-qubit gate as the per-gate launcher runs it (qsvk_run_op): the classification of qsv_apply_* (diagonal,
// phase, CX / controlled-U, SWAP as a pair exchange, dense) with everything held by value, so that it can wait in a queue.
enum { OP_DENSE = 0, OP_PAIR = 1, OP_DIAG = 2, OP_PHASE = 3 };
constexpr int OP_MAX_CTRL = 40;
struct Op {
    int kind = OP_DENSE;
    int k = 0;                        // target legs (dense, diag: 1 or 2; pair: 2; phase: 0)
    int bits[2] = {-1, -1};           // target bits, leg 0 first (leg 0 = most significant matrix index bit)
    int nctrl = 0;
    int cbits[OP_MAX_CTRL] = {};      // control bits (phase: the bits that must all be 1)
    double m[32] = {};                // dense: 2^k x 2^k row-major complex; diag: 2^k complex; phase: (re, im)
};

// ---- target split ------------------------------------------------------------------------------------------------------
// The targets of a k-qubit gate on an n-qubit register: `high` (bits >= 6, in leg order), `low` (bits < 6, ascending: bits
// 0..2 inside a 128-byte line first, then bits 3..5) and one stand-in bit per low target (the lowest free bits >= 6).
struct Split {
    std::vector<int> high, low, standin;
    bool enough = true;   // every low target has its stand-in (needs n >= k + 6); false: only the untransposed form fits
    int KB = 0;           // low targets below bit 3
};
inline Split split_targets(int k, const int *bits, int n) {
    Split s;
    for (int j = 0; j < k; ++j) (bits[j] >= LANE_BITS ? s.high : s.low).push_back(bits[j]);
    std::sort(s.low.begin(), s.low.end());
    for (int b = LANE_BITS; b < n && s.standin.size() < s.low.size(); ++b)
        if (std::find(s.high.begin(), s.high.end(), b) == s.high.end()) s.standin.push_back(b);
    s.enough = s.standin.size() == s.low.size();
    for (int b : s.low) s.KB += b < LINE_BITS;
    return s;
}
// The same gate without a transpose: every target is its own address bit, the lanes are the lowest free bits.
inline Split untransposed(int k, const int *bits) {
    Split s;
    s.high.assign(bits, bits + k);
    return s;
}

// ---- offsets and index maps --------------------------------------------------------------------------------------------
// off[c] of the 2^k kernel indices: kernel index bit i is address bit addr_bit[i].
inline std::vector<uint64_t> offsets(const std::vector<int> &addr_bit) {
    std::vector<uint64_t> off(1ull << addr_bit.size(), 0);
    for (size_t c = 0; c < off.size(); ++c)
        for (size_t i = 0; i < addr_bit.size(); ++i)
            if ((c >> i) & 1) off[c] |= 1ull << addr_bit[i];
    return off;
}

// Kernel bit order of the per-thread forms (k_dense_big, k_dense_lds, k_seq_*): c = (h << KL) | t, t bit j <-> low[j],
// h bit i <-> high[i].
inline std::vector<int> kernel_bits(const Split &s) {
    std::vector<int> kb(s.low);
    kb.insert(kb.end(), s.high.begin(), s.high.end());
    return kb;
}
// Where those kernel bits are loaded from: a high target from its own bit, a low target from its stand-in -- except that
// the line-granular forms (`a_in_place`) address a target on lane bits 3..5 directly.
inline std::vector<int> address_bits(const Split &s, bool a_in_place) {
    std::vector<int> ab;
    for (size_t j = 0; j < s.low.size(); ++j) ab.push_back(a_in_place && s.low[j] >= LINE_BITS ? s.low[j] : s.standin[j]);
    ab.insert(ab.end(), s.high.begin(), s.high.end());
    return ab;
}

// The bits a transposed or untransposed launch takes out of its enumeration: high targets and stand-ins, ascending.
inline std::vector<int> inserted_bits(const Split &s) {
    std::vector<int> ins(s.high);
    ins.insert(ins.end(), s.standin.begin(), s.standin.end());
    std::sort(ins.begin(), ins.end());
    return ins;
}

// ui[c]: the caller's matrix index of kernel index c.  bits[leg] = target of matrix leg `leg` (leg 0 most significant);
// kernel_bit[i] = the target that kernel index bit i stands for.
inline std::vector<int> user_index(int k, const int *bits, const int *kernel_bit) {
    std::vector<int> ui(1u << k, 0);
    for (int c = 0; c < (1 << k); ++c)
        for (int i = 0; i < k; ++i)
            for (int leg = 0; leg < k; ++leg)
                if (bits[leg] == kernel_bit[i]) ui[c] |= ((c >> i) & 1) << (k - 1 - leg);
    return ui;
}

// ---- matrix writers ----------------------------------------------------------------------------------------------------
enum MatrixLayout {
    MAT_COMPLEX,        // [r][c] (re, im) interleaved
    MAT_REAL,           // [r][c] re only
    MAT_3M_ROWS,        // a row = three planes of D doubles: Ar | Ai | Ar + Ai
    MAT_3M_ENTRIES,     // [r][c] (Ar, Ai, Ar + Ai)
    MAT_COLUMNS,        // [plane][c][r]: the real plane, then the imaginary one (matrix cores)
    MAT_COLUMNS_REAL    // [c][r]: the real plane alone
};
inline size_t matrix_doubles(MatrixLayout layout, int D) {
    const size_t per = layout == MAT_REAL || layout == MAT_COLUMNS_REAL ? 1 : layout == MAT_3M_ROWS || layout == MAT_3M_ENTRIES ? 3 : 2;
    return per * D * D;
}
inline bool is_real(int D, const double *m_user) {
    for (int i = 0; i < D * D; ++i)
        if (m_user[2 * i + 1] != 0.0) return false;
    return true;
}
// out[layout(r, c)] = m_user[ui[r]][ui[c]].  rows > 0 (k_dense_tile; the [r][c] layouts only): the rows are regrouped into
// the slices of `rows` rows that one wave computes, [r / rows][c][r % rows].
inline void write_matrix(MatrixLayout layout, int D, const double *m_user, const int *ui, double *out, int rows = 0) {
    for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
            const double re = m_user[2 * (ui[r] * D + ui[c])], im = m_user[2 * (ui[r] * D + ui[c]) + 1];
            const size_t at = rows > 0 ? (static_cast<size_t>(r / rows) * D + c) * rows + r % rows : static_cast<size_t>(r) * D + c;
            switch (layout) {
                case MAT_COMPLEX:
                    out[2 * at] = re;
                    out[2 * at + 1] = im;
                    break;
                case MAT_REAL: out[at] = re; break;
                case MAT_3M_ROWS:
                    out[3 * D * r + c] = re;
                    out[3 * D * r + D + c] = im;
                    out[3 * D * r + 2 * D + c] = re + im;
                    break;
                case MAT_3M_ENTRIES:
                    out[3 * at] = re;
                    out[3 * at + 1] = im;
                    out[3 * at + 2] = re + im;
                    break;
                case MAT_COLUMNS: out[D * D + c * D + r] = im; [[fallthrough]];
                case MAT_COLUMNS_REAL: out[c * D + r] = re; break;
            }
        }
}
inline std::vector<double> matrix(MatrixLayout layout, int D, const double *m_user, const int *ui, int rows = 0) {
    std::vector<double> m(matrix_doubles(layout, D));
    write_matrix(layout, D, m_user, ui, m.data(), rows);
    return m;
}

// ---- enumeration -------------------------------------------------------------------------------------------------------
// The work items of a launch: W of them, deposited around the inserted positions.
struct Enumeration {
    uint64_t W = 0, or_mask = 0;
    int nins = 0;
    uint32_t pos[qsv_plan::TILE_BITS] = {};   // ascending
};
inline Enumeration enumeration(uint64_t W, std::vector<int> inserted, uint64_t or_mask = 0) {
    Enumeration e;
    std::sort(inserted.begin(), inserted.end());
    e.W = W;
    e.or_mask = or_mask;
    e.nins = static_cast<int>(inserted.size());
    for (int j = 0; j < e.nins; ++j) e.pos[j] = static_cast<uint32_t>(inserted[j]);
    return e;
}
// A zeroed argument struct (BigArgs, LdsArgs, Mfma6Args) with the enumeration filled in.
template <class Args>
inline Args with_enumeration(const Enumeration &e) {
    Args g;
    memset(&g, 0, sizeof(g));
    g.W = e.W;
    g.or_mask = e.or_mask;
    g.nins = e.nins;
    for (int j = 0; j < e.nins; ++j) g.pos[j] = e.pos[j];
    return g;
}

// ---- low-bit fields of the line-granular forms (k_dense_lds, k_seq_lds) ------------------------------------------------
// A targets (lane bits 3..5) are exchanged with their stand-ins by address arithmetic, B targets (lane bits 0..2) through
// LDS rows: dep(v) spreads the KB bits of v onto the B lane bits.
struct LowFields {
    uint32_t amask = 0, bmask = 0;
    int32_t abit[3] = {0, 0, 0}, aE[3] = {0, 0, 0}, na = 0;
    uint32_t bdep[8] = {};
};
inline LowFields low_fields(const Split &s) {
    LowFields f;
    for (size_t j = 0; j < s.low.size(); ++j) {
        if (s.low[j] >= LINE_BITS) {
            f.abit[f.na] = s.low[j];
            f.aE[f.na] = s.standin[j];
            f.amask |= 1u << s.low[j];
            ++f.na;
        } else {
            f.bmask |= 1u << s.low[j];
        }
    }
    for (int v = 0; v < (1 << s.KB); ++v)
        for (int j = 0; j < s.KB; ++j)
            if ((v >> j) & 1) f.bdep[v] |= 1u << s.low[j];
    return f;
}
inline void set_low_fields(LdsArgs &g, const LowFields &f) {
    g.amask = f.amask;
    g.bmask = f.bmask;
    g.na = f.na;
    memcpy(g.abit, f.abit, sizeof(f.abit));
    memcpy(g.aE, f.aE, sizeof(f.aE));
    memcpy(g.bdep, f.bdep, sizeof(f.bdep));
}

// ---- SeqGate records ---------------------------------------------------------------------------------------------------
// A 1- or 2-qubit gate of a sequence on the register bits j0 (leg 0) and j1 (leg 1) of the thread's amplitudes; m is the
// caller's 2 x 2 or 4 x 4 matrix.  The kernels index a 2-qubit record with bit 1 <-> the higher register bit, the caller
// with bit 1 <-> leg 0: the matrix is transposed in its index bits when leg 0 lands on the lower register bit.
inline SeqGate seq_record(int arity, int j0, int j1, const double *m) {
    SeqGate r;
    memset(&r, 0, sizeof(r));
    if (arity == 1) {
        r.code = j0;
        memcpy(r.m, m, sizeof(double) * 8);
        return r;
    }
    const int hi = std::max(j0, j1), lo = std::min(j0, j1);
    r.code = 5 + hi * (hi - 1) / 2 + lo;
    const int swapped[4] = {0, 2, 1, 3};
    int ui[4];
    for (int c = 0; c < 4; ++c) ui[c] = j0 > j1 ? c : swapped[c];
    write_matrix(MAT_COMPLEX, 4, m, ui, r.m);
    return r;
}

// ---- pass cutter of k_seq_tile -----------------------------------------------------------------------------------------
// A fused block of k qubits as the list of its source gates on tiles of 2^12 amplitudes: the tile's bits are the targets
// and the lowest other bits, ascending.  The gate list is cut into passes of consecutive gates whose legs fit four tile
// indices together; a pass with fewer is completed with the lowest unused tile indices.  Gate g acts on block legs
// legs[2 g] (and legs[2 g + 1] when arity[g] == 2), its matrix follows the previous gate's in `mats` (8 or 32 doubles).
struct TileCut {
    enum Status { OK, UNHANDLED /* arity, or too many passes */, LEG_OUTSIDE, LEGS_EQUAL } status = OK;
    std::vector<int> tile_bits;       // address bit of tile index 0..11
    std::vector<TilePass> passes;
    std::vector<SeqGate> rec;         // in application order, codes relative to their pass's four bits
};
inline TileCut cut_tile_passes(int n, int k, const int *bits, int n_gates, const int *arity, const int *legs,
                               const double *mats) {
    TileCut out;
    std::vector<int> &tile_bits = out.tile_bits;
    tile_bits.assign(bits, bits + k);
    for (int b = 0; b < n && static_cast<int>(tile_bits.size()) < TILE_SEQ_BITS; ++b)
        if (std::find(bits, bits + k, b) == bits + k) tile_bits.push_back(b);
    std::sort(tile_bits.begin(), tile_bits.end());
    auto position = [&](int bit) { return static_cast<int>(std::find(tile_bits.begin(), tile_bits.end(), bit) - tile_bits.begin()); };
    struct Draft {
        std::vector<int> q;      // tile indices of the pass
        std::vector<int> gate;   // indices into the gate list
    };
    std::vector<Draft> drafts;
    std::vector<std::array<int, 2>> where(n_gates);
    std::vector<size_t> mat_at(n_gates);
    size_t at = 0;
    for (int gi = 0; gi < n_gates; ++gi) {
        if (arity[gi] != 1 && arity[gi] != 2) return out.status = TileCut::UNHANDLED, out;
        mat_at[gi] = at;
        at += arity[gi] == 1 ? 8 : 32;
        for (int j = 0; j < 2; ++j) {
            const int leg = legs[2 * gi + (j < arity[gi] ? j : 0)];
            if (leg < 0 || leg >= k) return out.status = TileCut::LEG_OUTSIDE, out;
            where[gi][j] = position(bits[leg]);
        }
        if (arity[gi] == 2 && where[gi][0] == where[gi][1]) return out.status = TileCut::LEGS_EQUAL, out;
        std::vector<int> merged = drafts.empty() ? std::vector<int>() : drafts.back().q;
        for (int j = 0; j < arity[gi]; ++j)
            if (std::find(merged.begin(), merged.end(), where[gi][j]) == merged.end()) merged.push_back(where[gi][j]);
        if (drafts.empty() || merged.size() > 4) {
            drafts.push_back(Draft{});
            merged.assign(where[gi].begin(), where[gi].begin() + arity[gi]);
        }
        drafts.back().q = merged;
        drafts.back().gate.push_back(gi);
    }
    if (drafts.size() > static_cast<size_t>(TILE_SEQ_MAX_PASSES)) return out.status = TileCut::UNHANDLED, out;
    for (Draft &d : drafts) {
        for (int b = 0; d.q.size() < 4; ++b)          // fewer than four bits in use: any other tile bits complete the group
            if (std::find(d.q.begin(), d.q.end(), b) == d.q.end()) d.q.push_back(b);
        std::sort(d.q.begin(), d.q.end());
        TilePass ps;
        memset(&ps, 0, sizeof(ps));
        ps.first = static_cast<int32_t>(out.rec.size());
        ps.count = static_cast<int32_t>(d.gate.size());
        for (int j = 0; j < 4; ++j) ps.q[j] = d.q[j];
        out.passes.push_back(ps);
        auto local = [&](int tile_bit) { return static_cast<int>(std::find(d.q.begin(), d.q.end(), tile_bit) - d.q.begin()); };
        for (int gi : d.gate)
            out.rec.push_back(seq_record(arity[gi], local(where[gi][0]), local(where[gi][1]), mats + mat_at[gi]));
    }
    return out;
}

// ---- tile order --------------------------------------------------------------------------------------------------------
// Tile order of k_dense_tile / k_dense_tile12 by target placement.  Which DRAM channels the workgroups in flight hit
// together depends on the target bits; no single order wins everywhere: contiguous windows (the d = 2^K modes of the CV
// path) have a clear best order per position, scattered targets (fused qubit gates) are served well by 4 regions
// (K = 3) / 2 (K = 4) / 8 (K = 5).
// The rule is keyed on ABSOLUTE bit positions -- on the physical address bits a target toggles -- not on the distance
// from the register's top bit: the same bits want the same order on registers of 25, 26, 27, 28, 29 and 31 qubits
// (the shard sizes of the strong- and weak-scaling runs and of config 3; profiles/r03_tile_order_by_size.txt: bits 3-6
// want 2 regions, 17 / 21 / 25 eight, 20 / 22 / 23 four at every size, and a pair (lo >= 17, 27) wants four regions
// whether bit 27 is the top bit (n = 28) or not (n = 29, 31)).  Against the best of {0, 2, 4, 8, 16} regions per
// placement the rule is within 0.7-2.5 % on the sum over the sampled placements at every size.
inline uint32_t tile_regions(int k, const std::vector<int> &sorted_bits) {
    if (k == 1) {   // per target bit
        const int b = sorted_bits[0];
        return b <= 6 ? 2 : b == 7 ? 8 : b <= 16 ? 0 : b == 17 ? 8 : b <= 19 ? 0 : b == 20 ? 4 : b == 21 ? 8
             : b <= 23 ? 4 : b == 25 ? 8 : 0;
    }
    if (k == 2) {   // pairs of bits >= 6 (lower targets stay on the register form)
        const int lo = sorted_bits[0], hi = sorted_bits[1];
        if (lo <= 8) {
            // 8 regions, except where both strides are short: (7|8, <= 17), (6, <= 11) and (6..8, 24) run 3-12 % faster in
            // plain order at every size
            if ((lo >= 7 && hi <= 17) || (lo == 6 && hi <= 11) || hi == 24) return 0;
            return 8;
        }
        if (hi == 20 && lo >= 12 && lo <= 16) return 0;
        if (hi >= 20 && hi <= 21) return 8;
        if (hi == 22) return lo >= 13 ? 4 : 8;
        if (hi == 23 && lo >= 20) return 8;
        if (hi == 24 && lo >= 18) return 4;
        if (hi == 26 && lo == 22) return 4;
        if ((hi == 27 && lo >= 17) || (hi == 28 && lo >= 20)) return 4;
        return 0;
    }
    const int lo = sorted_bits.front(), top = sorted_bits.back();
    const bool window = top - lo == static_cast<int>(sorted_bits.size()) - 1;
    if (k == 3) {
        if (!window) return 4;
        return top <= 8 ? 4 : top <= 19 ? 2 : top <= 22 ? 8 : top <= 24 ? 2 : 0;
    }
    if (k == 4) {
        if (!window) return 2;
        return top <= 10 ? 4 : top <= 15 ? 2 : top <= 19 ? 0 : top == 20 ? 2 : top <= 23 ? 8 : 2;
    }
    if (!window) return 8;
    return top <= 11 ? 8 : top <= 13 ? 4 : top <= 20 ? 0 : 2;
}

// Does a dense 1- / 2-qubit gate take the tile form (k_dense_tile12*)?  Otherwise it runs on k_dense / k_dense_ctrl.  The
// pass kernel (k_pass_tile) asks too: it sums each gate's products in the order of the kernel the gate would have run on.
inline bool tile12_takes(uint64_t amps, int k, const int *bits, int nctrl, const int *cbits) {
    if (k + nctrl > 2 * MAX_K || (nctrl && k != 1)) return false;   // controlled 4 x 4 gates only arise with a folded narrow control
    for (int i = 0; i < nctrl; ++i)
        if (cbits[i] < LINE_BITS) return false;   // a control inside a 128-byte line cannot be skipped
    const uint64_t W = amps >> (k + nctrl);
    const int lowest = k == 1 ? bits[0] : std::min(bits[0], bits[1]);
    // 2-qubit gates with a target inside a wavefront (bits 3..5) are better off with k_dense<1, 1> (1.29-1.37 ms)
    return !(lowest < (k == 1 ? LINE_BITS : LANE_BITS) || W < 64 || W % 64);
}

// ---- dispatch ranges ---------------------------------------------------------------------------------------------------
// A launch of W work items is split into dispatches of at most `limit` each.
// Tiles per dispatch of the forms that walk their tiles in region order (k_dense_tile12*, k_dense_tile: 64 columns per
// tile; k_seq_tile, k_pass_tile): a power of two, so that every dispatch of a split launch has a tile count the region
// order divides (with 2^24 - 1 tiles per dispatch a 31-qubit shard ran its 1-qubit gates in plain order: 12.0 ms
// on bits 3..6 against 10.9 for the register form, profiles/r03_tile_order_by_size.txt).
constexpr uint64_t DISPATCH_TILES = 1ull << 23;
// Work items per dispatch of the other forms: an AQL dispatch counts work-items in 32 bits, at most 2^32 / 256 workgroups
// of 256 threads.
constexpr uint64_t DISPATCH_ITEMS = 0x00ffffffull * BLOCK;
struct Range {
    uint64_t w0, count;
};
inline std::vector<Range> dispatch_ranges(uint64_t W, uint64_t limit) {
    std::vector<Range> out;
    for (uint64_t w0 = 0; w0 < W; w0 += limit) out.push_back(Range{w0, std::min(limit, W - w0)});
    return out;
}

// Workgroups of a grid-stride launch over `items` work items, `per_block` each, at most `cap` (0: no cap).
inline int grid_for(uint64_t items, int per_block, int cap) {
    uint64_t blocks = (items + per_block - 1) / per_block;
    if (blocks < 1) blocks = 1;
    if (cap > 0 && blocks > static_cast<uint64_t>(cap)) blocks = cap;
    // an AQL dispatch counts work-ITEMS in 32 bits: at most 2^32 / 256 workgroups of 256 threads per launch
    // (a 33-qubit register would need 2^25); every kernel launched through here loops over the remainder
    if (blocks > 0x00ffffffull) blocks = 0x00ffffffull;
    return static_cast<int>(blocks);
}

// ---- launch rules of the register forms of 1- and 2-qubit gates (k_dense, k_dense_ctrl, k_diag) -------------------------
// What launch_dense and launch_diag (qsv_gate12.hip) put around their launch: the items a thread keeps in flight, the
// distance between them, the tile order and the grid.  All figures are MI355X at n = 28, from the sweeps under profiles/.
struct LaunchOptions {          // the register's options; the defaults are qsv_state's
    int unroll = 0;             // QSV_OPT_UNROLL: items per thread, 0 = the rule's choice
    int remap = -1;             // QSV_OPT_TILE_REGIONS: tile order, -1 = the rule's choice
    int ubit = 8;               // QSV_OPT_ITEM_STRIDE_BIT
    int grid_cap = 0;           // QSV_OPT_GRID_CAP
};
struct Launch12 {
    int U = 1;                  // items per thread, after the default choice and the halving for small W
    int ubit = 8;               // GateArgs::ubit after the clamp (k_diag's items are always back to back: left as given)
    int remap = 0;              // GateArgs::remap / DiagArgs::remap: tile-order regions
    int grid = 1;               // workgroups
};

// The pair strides of a dense launch: hbit[i] = address bit of high target i (the top set bit of GateArgs::hoff[1 << i]).
struct PairStrides {
    bool far = false;           // some stride is 16 MiB .. 512 MiB (bits 20..25)
    int top = 0;                // the highest target bit
};
inline PairStrides pair_strides(int KH, const int *hbit) {
    PairStrides s;
    for (int i = 0; i < KH; ++i) {
        s.far = s.far || (hbit[i] >= 20 && hbit[i] <= 25);
        s.top = std::max(s.top, hbit[i]);
    }
    return s;
}

// Work items in flight per thread: with nontemporal accesses one item per thread streams best (6.0-6.4 TB/s) until the
// pair stride reaches 16 MiB (bit 20), where four items per thread hold 5.8 TB/s and one item drops to 5.4.
inline int dense_default_unroll(int KH, int KL, const PairStrides &s) {
    if (KH == 0) return KL == 2 ? 2 : 1;
    if (KH == 1 && KL == 1) return 1;   // round 2 re-sweep: one item per thread at every stride (1.35-1.44 against 1.50-1.53 ms on bits 20..25)
    // single far pair stride: only 16 MiB (bit 20) wants four items per thread (profiles/r01_sweep_far_bits.txt)
    if (KH == 1 && KL == 0) return s.top == 20 ? 4 : 1;
    return s.far ? 4 : 1;
}

// Tile order (profiles/r01_sweep_tile_order.txt): natural-order kernels like 32 regions, pair kernels 8 (one per XCD),
// except at pair strides of 16..512 MiB where the plain order is best.  `sub`: a controlled or pair-exchange launch.
inline int dense_default_regions(int KH, int KL, bool sub, const PairStrides &s) {
    if (sub) return 0;                                  // controlled / pair-exchange launches: plain order
    if (KH == 0) return KL == 2 ? 0 : 32;               // round 2 re-sweep (tools/probe_low_pairs.py): 1.35 against 1.41 ms
    if (KH == 1 && KL == 0) return s.top == 20 ? 0 : s.top == 24 ? 2 : 8;   // per-stride winners of the sweeps
    if (KH == 1) return (s.top == 20 || s.top == 24) ? 32 : 8;              // KL = 1; round 2 re-sweep (tools/probe_retune.py)
    return s.top < 20 ? 8 : 0;
}

inline int halved_for(int U, uint64_t W) {   // never more unrolling than there is work for one tile
    while (U > 1 && W < static_cast<uint64_t>(BLOCK) * U) U >>= 1;
    return U;
}

// k_dense<KH, KL> / k_dense_ctrl<KH, KL> over W work items.
inline Launch12 dense_launch(int KH, int KL, const int *hbit, bool sub, uint64_t W, const LaunchOptions &o) {
    const PairStrides s = pair_strides(KH, hbit);
    Launch12 l;
    l.U = halved_for(o.unroll > 0 ? o.unroll : dense_default_unroll(KH, KL, s), W);
    l.remap = o.remap >= 0 ? o.remap : dense_default_regions(KH, KL, sub, s);
    l.ubit = o.ubit;
    while (l.ubit > 8 && (W >> l.ubit) < static_cast<uint64_t>(l.U)) --l.ubit;   // small registers
    l.grid = grid_for(W, BLOCK * l.U, o.grid_cap);
    return l;
}

// k_diag over W work items.  Full traffic: one item per thread, 32 regions; sub-space launches (Z, CZ, multi-controlled
// phases): four items per thread, one region per XCD (profiles/r01_sweep_sub_kernels.txt).
inline Launch12 diag_launch(bool sub, uint64_t W, const LaunchOptions &o) {
    Launch12 l;
    l.U = halved_for(o.unroll > 0 ? o.unroll : (sub ? 4 : 1), W);
    l.remap = o.remap >= 0 ? o.remap : (sub ? 8 : 32);
    l.ubit = o.ubit;
    l.grid = grid_for(W, BLOCK * l.U, o.grid_cap);
    return l;
}

// ---- form of a dense k-qubit gate (qsvk_generic) -----------------------------------------------------------------------
enum Form { FORM_GATHER /* k_generic */, FORM_MFMA, FORM_MTILE5, FORM_TILE, FORM_LDS, FORM_BIG };
struct FormChoice {
    Form form = FORM_GATHER;
    bool transposed = false;   // the low targets are exchanged with stand-in bits (FORM_LDS, FORM_BIG)
    bool realm = false;        // the kernel's real-matrix arithmetic
    bool m3 = false;           // three real multiplications per complex entry
};
struct FormOptions {
    int kq_variant = 0;        // QSV_OPT_KQ_VARIANT
    int complex_product = 0;   // QSV_OPT_COMPLEX_PRODUCT
    bool mtile = false;        // $QSV_MTILE
};
inline FormChoice choose_form(int n, uint64_t amps, int k, const int *bits, bool real_matrix, const FormOptions &o) {
    FormChoice f;
    // matrix-core form: the 2^(n-k) groups must fill whole waves of 16
    // (k = 5 on the matrix cores is a measurement variant only: on the benchmark circuit's fused blocks it wins where its
    // wave-instructions cover >= 512 contiguous bytes and the other targets are low (1.50 against 1.66 ms), loses with
    // targets above bit 18 (1.8-1.9 against 1.65), and over the whole circuit ties with the vector kernels: 28.3 ms both)
    const bool mfma_ok = n >= k && (amps >> k) >= 16;
    if (mfma_ok && ((k == 6 && o.kq_variant == 0) || (k == 5 && o.kq_variant == 5))) {
        f.form = FORM_MFMA;
        f.realm = real_matrix;
        f.m3 = !real_matrix && o.complex_product != 4;   // three real MFMAs per complex entry
        return f;
    }
    if (k < 3 || n < k) return f;
    const Split s = split_targets(k, bits, n);
    bool all_from_bit3 = true;
    for (int j = 0; j < k; ++j) all_from_bit3 = all_from_bit3 && bits[j] >= LINE_BITS;
    const bool fits = (amps >> k) >= 64 && (amps >> k) % 64 == 0;
    const bool tile_ok = k <= 5 && all_from_bit3 && fits;
    // shipped choice: k = 3, 4, and k = 5 with a real matrix (a complex 32 x 32 product per column keeps the FP64 pipe busy
    // for 0.9 of the 1.4 ms the memory traffic takes; the tile form's extra LDS round trip then costs more than it hides.
    // A persistent form with two LDS tiles and the next tile's loads in flight during the arithmetic was measured too:
    // 1.86 ms -- two workgroups per CU leave the FMA chains exposed to the scalar-load and LDS latencies)
    // complex 5-qubit blocks on bits >= 3: the tile-fed matrix-core kernel (k_dense_mtile5; QSV_OPT_KQ_VARIANT = 6 forces it)
    const bool use_mtile = tile_ok && k == 5 && !real_matrix && o.complex_product != 4 &&
                           (o.kq_variant == 6 || (o.kq_variant == 0 && o.mtile));
    const bool use_tile = use_mtile || (tile_ok && (o.kq_variant == 4 || (o.kq_variant == 0 && (k <= 4 || real_matrix))));
    // all targets high, or a register too small to transpose: lanes = lowest free bits
    f.transposed = !s.low.empty() && s.enough && o.kq_variant != 2 && !use_tile;
    const int KL = f.transposed ? static_cast<int>(s.low.size()) : 0;
    // Which form (MI355X, n = 28, profiles/r02_sweep_kq_kernels.txt): k = 5 with low targets -> the line-granular
    // kernel (4.9-5.2 TB/s at every placement; the shuffle form drops to 2.1-4.4 there); k = 5 real matrices ->
    // the same kernel's two-FMA arithmetic (5.4-5.8 TB/s); k = 3, 4 and k = 5 on high bits -> the shuffle form
    // (its butterflies are cheap up to 16 amplitudes per thread: 5.6-6.0 TB/s).  QSV_OPT_KQ_VARIANT overrides.
    const bool use_lds = !use_tile && fits && (k == 6 || o.kq_variant == 3 ||
                                               (o.kq_variant == 0 && k == 5 && (KL > 0 || real_matrix)));
    if (k == 6 && !use_lds) return FormChoice();   // only the line-granular kernel is built for 64 x 64 matrices
    f.form = use_mtile ? FORM_MTILE5 : use_tile ? FORM_TILE : use_lds ? FORM_LDS : FORM_BIG;
    f.realm = (use_lds || use_tile) && real_matrix;
    // complex 5-qubit blocks in three real multiplications per entry (row_product_3m): a measurement variant only
    // (QSV_OPT_COMPLEX_PRODUCT = 3).  On the vector pipe it does not pay (profiles/r03_complex_product.txt): a quarter
    // fewer FMAs, but a third plane of matrix rows through the scalar cache and xr + xi in 64 more registers -- 1.64-1.71
    // ms against 1.61-1.77 for k_dense_big<5, 0>, 1.80-1.99 against 1.66-1.73 for k_dense_lds with targets inside a line
    // (two waves per SIMD instead of three).  These kernels are not waiting for the FP64 pipe.  On the matrix cores (k = 6)
    // the same trick is worth 13 %: see FORM_MFMA.
    f.m3 = !use_mtile && k == 5 && !real_matrix && o.complex_product == 3 && (use_tile || use_lds || KL == 0);
    return f;
}

// ---- gate records of one pass (k_pass_tile) ----------------------------------------------------------------------------
// `count` queued gates, in application order, on the tiles spanned by bits 0..5 and tile_high, on a register of `amps`
// amplitudes: what each gate is in tile indices, the groups (qsv_plan::cut_groups), and each gate's record relative to
// the register bits of its group.
struct PassRecords {
    enum Status { OK, TARGET_OUTSIDE_TILE, TARGET_OUTSIDE_GROUP } status = OK;
    int tile_bits[qsv_plan::TILE_BITS] = {};     // address bit of tile index 0..11
    std::vector<PassGate> rec;
    std::vector<PassGroup> grp;
    std::vector<uint64_t> omask;                 // rec[i].omask, packed: the kernel reads them before any record
    bool every_tile = false;                     // some gate has no control outside the tile: no tile is skipped
};
inline PassRecords pass_records(const Op *const *ops, int count, uint64_t tile_high, uint64_t amps) {
    PassRecords out;
    int local_of[64];
    for (int b = 0; b < 64; ++b) {
        local_of[b] = qsv_plan::tile_index(b, tile_high);
        if (local_of[b] >= 0) out.tile_bits[local_of[b]] = b;
    }
    // leg[]: dense, kernel bit 0 first; pair: both legs; diagonal: the bits that select d[(s0 << 1) | s1], leg[1] < 0:
    // d[s0], leg[0] < 0: one factor for all
    std::vector<PassGate> &rec = out.rec;
    rec.resize(count);
    std::vector<std::array<int, 2>> leg(count, std::array<int, 2>{-1, -1});
    std::vector<uint32_t> cmask(count, 0), need(count, 0);
    for (int i = 0; i < count; ++i) {
        const Op &op = *ops[i];
        PassGate &pg = rec[i];
        memset(&pg, 0, sizeof(pg));
        uint64_t ctrl = 0;
        for (int c = 0; c < op.nctrl; ++c) ctrl |= 1ull << op.cbits[c];
        const qsv_plan::ControlMasks cm = qsv_plan::control_masks(ctrl, tile_high);
        cmask[i] = cm.inside;
        pg.omask = cm.outside;
        out.omask.push_back(pg.omask);
        out.every_tile = out.every_tile || pg.omask == 0;
        for (int j = 0; j < op.k; ++j)
            if (local_of[op.bits[j]] < 0) return out.status = PassRecords::TARGET_OUTSIDE_TILE, out;
        if (op.kind == OP_DIAG || op.kind == OP_PHASE) {
            pg.form = PASS_DIAG_T;
            if (op.kind == OP_PHASE) {           // k_diag with d0 = d1 = the phase (qsvk_phase)
                for (int e = 0; e < 4; ++e) {
                    pg.m[2 * e] = op.m[0];
                    pg.m[2 * e + 1] = op.m[1];
                }
            } else {
                leg[i][0] = local_of[op.bits[0]];
                if (op.k == 2) leg[i][1] = local_of[op.bits[1]];
                memcpy(pg.m, op.m, sizeof(double) * (2u << op.k));
            }
            continue;
        }
        if (op.kind == OP_PAIR) {               // qsvk_pair_exchange: (a, b) = (1, 0) <-> (0, 1)
            pg.form = PASS_PAIR;
            leg[i] = {local_of[op.bits[0]], local_of[op.bits[1]]};
            need[i] = (1u << leg[i][0]) | (1u << leg[i][1]);
            continue;
        }
        // dense: kernel index bit i <-> register bit kb[i], matrix re-indexed as the per-gate launcher does
        const int k = op.k;
        int kb[2] = {op.bits[0], op.bits[1]};
        if (tile12_takes(amps, k, op.bits, op.nctrl, op.cbits)) {      // launch_tile12: kernel bit leg <-> bits[leg]
            pg.form = k == 1 ? PASS_D2 : PASS_D4;
        } else {                                                       // qsvk_dense: low targets first, then high ones
            int nl = 0, nh = 0;
            for (int j = 0; j < k; ++j) nl += op.bits[j] < LANE_BITS;
            for (int j = 0, l = 0; j < k; ++j) kb[op.bits[j] < LANE_BITS ? l++ : nl + nh++] = op.bits[j];
            pg.form = nl == 0 ? (k == 1 ? PASS_D2 : PASS_D4) : nh == 0 ? (k == 1 ? PASS_D2X : PASS_D4X) : PASS_D4HL;
        }
        write_matrix(MAT_COMPLEX, 1 << k, op.m, user_index(k, op.bits, kb).data(), pg.m);
        for (int i2 = 0; i2 < k; ++i2) {
            leg[i][i2] = local_of[kb[i2]];
            need[i] |= 1u << leg[i][i2];
        }
    }
    const std::vector<qsv_plan::Group> cut = qsv_plan::cut_groups(need);
    out.grp.resize(cut.size());
    for (size_t p = 0; p < cut.size(); ++p) {
        PassGroup &gr = out.grp[p];
        memset(&gr, 0, sizeof(gr));
        gr.first = cut[p].first;
        gr.count = cut[p].count;
        int reg_of[qsv_plan::TILE_BITS];       // register bit of a tile index, -1: a thread bit
        for (int t = 0; t < qsv_plan::TILE_BITS; ++t) reg_of[t] = -1;
        for (int j = 0; j < qsv_plan::REG_BITS; ++j) {
            gr.q[j] = cut[p].reg[j];
            reg_of[gr.q[j]] = j;
        }
        for (int i = gr.first; i < gr.first + gr.count; ++i) {
            PassGate &pg = rec[i];
            gr.gates |= 1ull << i;
            for (int t = 0; t < qsv_plan::TILE_BITS; ++t)
                if ((cmask[i] >> t) & 1) {
                    if (reg_of[t] >= 0) pg.rc |= 1u << reg_of[t];
                    else pg.tc |= 1u << t;
                }
            pg.ctl = pg.tc ? PASS_CTL_THREAD : pg.rc ? PASS_CTL_REG : PASS_CTL_NONE;
            const int l0 = leg[i][0], l1 = leg[i][1];
            if (pg.form == PASS_DIAG_T) {
                const int r0 = l0 >= 0 ? reg_of[l0] : -1, r1 = l1 >= 0 ? reg_of[l1] : -1;
                auto swap_d1_d2 = [&pg]() {          // d[(s0 << 1) | s1] -> d[(s1 << 1) | s0]
                    std::swap(pg.m[2], pg.m[4]);
                    std::swap(pg.m[3], pg.m[5]);
                };
                if (l0 < 0) {                        // a phase: the same factor whatever the bits
                    pg.tz0 = pg.tz1 = 0;
                } else if (l1 < 0) {
                    if (r0 >= 0) {
                        pg.form = PASS_DIAG_R1;
                        pg.code = r0;
                    } else {                         // d[s0] as d[(s0 << 1) | s0]
                        pg.m[6] = pg.m[2];
                        pg.m[7] = pg.m[3];
                        pg.tz0 = pg.tz1 = l0;
                    }
                } else if (r0 >= 0 && r1 >= 0) {
                    pg.form = PASS_DIAG_R2;
                    if (r0 > r1) swap_d1_d2();
                    pg.code = std::min(r0, r1) * 4 + std::max(r0, r1);
                } else if (r0 >= 0 || r1 >= 0) {     // d[(register bit << 1) | thread bit]
                    pg.form = PASS_DIAG_M;
                    if (r0 < 0) swap_d1_d2();
                    pg.code = r0 >= 0 ? r0 : r1;
                    pg.tz0 = r0 >= 0 ? l1 : l0;
                } else {
                    pg.tz0 = l0;
                    pg.tz1 = l1;
                }
                continue;
            }
            const int r0 = reg_of[l0], r1 = l1 >= 0 ? reg_of[l1] : 0;
            if (r0 < 0 || r1 < 0) return out.status = PassRecords::TARGET_OUTSIDE_GROUP, out;
            if (pg.form == PASS_PAIR) pg.code = std::min(r0, r1) * 4 + std::max(r0, r1);
            else if (pg.form == PASS_D2 || pg.form == PASS_D2X) pg.code = r0;
            else pg.code = r0 * 4 + r1;
        }
    }
    return out;
}

}  // namespace qsv_layout
